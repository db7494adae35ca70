"""Build the OpenCV-free plugin core (hip_sgm_core.cpp) into lib/libsgm_plugin_core.so and
its C++ test drivers lib/plugin_core_test, lib/plugin_bm_test, lib/plugin_paths_test,
lib/plugin_frame_test, lib/plugin_fill_test, lib/plugin_window_test and lib/plugin_pyramid_test, all linked against lib/libsgm_hip.so with g++.
(matcherHIPSGM.cpp needs OpenCV + the reference headers and is built inside the ROS tree.)"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
LIBDIR = os.path.join(PKG, "lib")


def _stale(out, deps):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps)


def build():
    os.makedirs(LIBDIR, exist_ok=True)
    inc = ["-I" + HERE, "-I" + os.path.join(ROOT, "include")]
    core_src = os.path.join(HERE, "hip_sgm_core.cpp")
    deps = [core_src, os.path.join(HERE, "hip_sgm_core.h"), os.path.join(ROOT, "include", "sgm_hip.h")]
    so = os.path.join(LIBDIR, "libsgm_plugin_core.so")
    link = ["-L" + LIBDIR, "-lsgm_hip", "-Wl,-rpath,$ORIGIN"]
    if _stale(so, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra"] + inc +
                              [core_src, "-o", so] + link)
    drv_src = os.path.join(HERE, "plugin_core_test.cpp")
    drv = os.path.join(LIBDIR, "plugin_core_test")
    if _stale(drv, deps + [drv_src]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + inc +
                              [drv_src, core_src, "-o", drv] + link)
    bm_src = os.path.join(HERE, "plugin_bm_test.cpp")
    bm_drv = os.path.join(LIBDIR, "plugin_bm_test")
    if _stale(bm_drv, deps + [bm_src]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + inc +
                              [bm_src, core_src, "-o", bm_drv] + link)
    paths_src = os.path.join(HERE, "plugin_paths_test.cpp")
    paths_drv = os.path.join(LIBDIR, "plugin_paths_test")
    if _stale(paths_drv, deps + [paths_src]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + inc +
                              [paths_src, core_src, "-o", paths_drv] + link)
    frame_src = os.path.join(HERE, "plugin_frame_test.cpp")
    frame_drv = os.path.join(LIBDIR, "plugin_frame_test")
    if _stale(frame_drv, deps + [frame_src]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + inc +
                              [frame_src, core_src, "-o", frame_drv] + link)
    fill_src = os.path.join(HERE, "plugin_fill_test.cpp")
    fill_drv = os.path.join(LIBDIR, "plugin_fill_test")
    if _stale(fill_drv, deps + [fill_src]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + inc +
                              [fill_src, core_src, "-o", fill_drv] + link)
    window_src = os.path.join(HERE, "plugin_window_test.cpp")
    window_drv = os.path.join(LIBDIR, "plugin_window_test")
    if _stale(window_drv, deps + [window_src]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + inc +
                              [window_src, core_src, "-o", window_drv] + link)
    pyramid_src = os.path.join(HERE, "plugin_pyramid_test.cpp")
    pyramid_drv = os.path.join(LIBDIR, "plugin_pyramid_test")
    if _stale(pyramid_drv, deps + [pyramid_src]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra"] + inc +
                              [pyramid_src, core_src, "-o", pyramid_drv] + link)
    return so


if __name__ == "__main__":
    build()
