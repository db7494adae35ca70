"""sgm_node_frame, host side (no GPU): the layout of its two structs in C++ and in the ctypes
mirrors, the argument errors that need no device, and the disparity window MatcherCore::imageCb
computes against process_disparity's np.float32 values."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_frame_test")


def _run(*args):
    r = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_abi_layout_matches_the_ctypes_mirrors(pkg):
    """Every sizeof and field offset the C++ compiler gives equals the Python mirror's."""
    got = [ln.split() for ln in _run("abi").splitlines()]
    want = []
    for cname, cls in (("sgm_camera_info", pkg.CameraInfo), ("sgm_node_frame_io", pkg.NodeFrameIO)):
        want.append(["sizeof", cname, str(ctypes.sizeof(cls))])
        want += [["offset", f"{cname}.{n}", str(getattr(cls, n).offset)] for n, _ in cls._fields_]
    assert got == want
    # every field of the header's structs is mirrored, in order
    hdr = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    for cname, cls in (("sgm_camera_info", pkg.CameraInfo), ("sgm_node_frame_io", pkg.NodeFrameIO)):
        body = hdr.split(f"typedef struct {cname} {{")[1].split(f"}} {cname};")[0]
        decl = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert decl == [n for n, _ in cls._fields_], cname


def test_symbols_are_exported_under_abi_5(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"sgm_node_frame", "sgm_node_frame_map_builds"} <= syms
    assert {"sgm_node_frame", "sgm_node_frame_map_builds"} <= set(pkg.EXPORTS)
    assert pkg.load_library().sgm_abi_version() == 5 == pkg.ABI_VERSION


def test_null_handle(pkg):
    lib = pkg.load_library()
    cam, io = pkg.CameraInfo(), pkg.NodeFrameIO()
    io.struct_size = ctypes.sizeof(pkg.NodeFrameIO)
    assert lib.sgm_node_frame(None, ctypes.byref(cam), ctypes.byref(cam), ctypes.byref(io)) == pkg.SGM_ERR_ARG
    assert lib.sgm_node_frame(None, None, None, None) == pkg.SGM_ERR_ARG
    assert lib.sgm_node_frame_map_builds(None) == 0


def test_camera_info_mirror_takes_what_image_cb_takes(pkg):
    K, D, R, P = np.arange(9.0).reshape(3, 3), [0.1, 0.2, 0.3, 0.4, 0.5], None, np.arange(12.0).reshape(3, 4)
    for info in ((K, D, R, P), dict(K=K, D=D, R=R, P=P)):
        c = pkg.CameraInfo.of(info)
        assert list(c.K) == list(K.ravel()) and list(c.P) == list(P.ravel())
        assert c.n_dist == 5 and list(c.D) == D + [0.0] * 7 and c.has_R == 0
    c = pkg.CameraInfo.of((K, None, np.eye(3), P))
    assert c.n_dist == 0 and c.has_R == 1 and list(c.R) == list(np.eye(3).ravel())
    assert pkg.CameraInfo.of(c) is c


# (f, T, depth_min, depth_max): the test_image_cb window, depth_min 0 (Q8: +inf), a negative window
# (the right matcher's), a quotient that rounds differently in float and double, tiny and huge ones
WINDOWS = [(712.5, 0.119, 0.5, 20.0), (712.5, 0.119, 0.0, 20.0), (712.5, 0.119, -20.0, -0.5), (700.0, 0.1, 0.3, 7.0),
           (1234.567, 0.0654321, 1e-9, 1e9), (3551.2, 0.3001, 0.0, 3.0), (500.0, -0.12, 0.4, 12.0)]


@pytest.mark.parametrize("f,T,zmin,zmax", WINDOWS)
def test_image_cb_window_is_process_disparitys(pkg, f, T, zmin, zmax):
    """MatcherCore::disparityWindow (what imageCb passes on) equals the np.float32 values of
    process_disparity / image_cb bit for bit."""
    lo = np.float32(T * f / zmax)
    with np.errstate(divide="ignore"):
        hi = np.float32(T * f / zmin) if zmin != 0 else np.float32(np.inf)
    out = _run("window", repr(f), repr(T), repr(zmin), repr(zmax)).split()
    assert out == ["min_disp", "%08x" % lo.view(np.uint32), "max_disp", "%08x" % hi.view(np.uint32)]
