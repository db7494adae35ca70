"""CPU tests of the pyramid level: the C-ABI surface (symbols, defaults, null handles, validation),
sgm_pyramid_plan against the reference's formula and against the errors a match returns, the
adapters' environment variable in Python and C++ alike, and the two new kernels' resources.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_reference as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_pyramid_test")
NEW = ["sgm_default_pyramid_params", "sgm_set_pyramid_params", "sgm_get_pyramid_params", "sgm_check_pyramid_params",
       "sgm_pyramid_plan", "sgm_debug_pyr_down", "sgm_debug_pyr_refine"]


# --------------------------------------------------------------------------------- the C ABI
def test_symbols_exported_and_declared(pkg):
    lib = pkg.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgm_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sgm_\w+)", out))
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in exported and hasattr(lib, s) and s in pkg.EXPORTS, s
    assert re.search(r"typedef struct sgm_pyramid_params\s*\{\s*int level;\s*int radius;\s*\}", hdr)
    assert lib.sgm_abi_version() == 5                              # callers check for the symbols
    csrc = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "csrc")
    hip = open(os.path.join(csrc, "pyramid.hip")).read()
    assert "sgm_launch.h" in hip and "k_pyr_down" in hip and "k_pyr_refine" in hip
    launch = open(os.path.join(csrc, "sgm_launch.h")).read()
    assert "launch_pyr_down" in launch and "launch_pyr_refine" in launch
    be = open(os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "build_ext.py")).read()
    assert '"pyramid.hip"' in be


def test_defaults_and_null_handles(pkg):
    lib = pkg.load_library()
    assert ctypes.sizeof(pkg.PyramidParams) == 8
    y = pkg.default_pyramid_params()
    assert y.as_dict() == dict(level=0, radius=2)
    lib.sgm_default_pyramid_params(None)                          # ignored
    assert pkg.default_pyramid_params(level=1, radius=1).as_dict() == dict(level=1, radius=1)
    assert lib.sgm_set_pyramid_params(None, ctypes.byref(y)) == pkg.SGM_ERR_ARG
    assert lib.sgm_get_pyramid_params(None, ctypes.byref(y)) == pkg.SGM_ERR_ARG
    assert lib.sgm_check_pyramid_params(None) == pkg.SGM_ERR_ARG
    p = pkg.default_params(pkg.MODE_CENSUS8)
    out = (ctypes.c_int * 6)()
    assert lib.sgm_pyramid_plan(None, None, ctypes.byref(y), 64, 64, ctypes.byref(out)) == pkg.SGM_ERR_ARG
    assert lib.sgm_pyramid_plan(ctypes.byref(p), None, None, 64, 64, ctypes.byref(out)) == pkg.SGM_ERR_ARG
    assert lib.sgm_pyramid_plan(ctypes.byref(p), None, ctypes.byref(y), 64, 64, None) == pkg.SGM_ERR_ARG
    assert lib.sgm_debug_pyr_down(None, None, None, 4, 4, 4, None, None) == pkg.SGM_ERR_ARG
    assert lib.sgm_debug_pyr_refine(None, None, None, 4, 4, 4, None, 0, 16, 0, 2, 1, None) == pkg.SGM_ERR_ARG


@pytest.mark.parametrize("level,radius,status", [(0, 2, 0), (0, 0, 0), (0, -7, 0), (0, 99, 0), (1, 1, 0), (1, 2, 0),
                                                 (1, 0, -2), (1, 3, -2), (1, -1, -2), (2, 2, -2), (-1, 2, -2),
                                                 (7, 0, -2)])
def test_validation(pkg, level, radius, status):
    """Level 0 or 1; at level 1 a radius in 1..2 (at level 0 the radius is not looked at)."""
    y = pkg.PyramidParams(level, radius)
    assert pkg.load_library().sgm_check_pyramid_params(ctypes.byref(y)) == status
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=32)
    if status:
        with pytest.raises(pkg.SGMError) as e:
            pkg.pyramid_plan(p, y, 200, 100)
        assert e.value.code == status
    else:
        assert pkg.pyramid_plan(p, y, 200, 100)["invalid"] == -16


# ------------------------------------------------------------------------------------ the plan
MODES = ["census", "sgbm5", "hh8", "bm"]


def _params(pkg, mode, m, D):
    mid = {"sgbm5": pkg.MODE_OCV_SGBM5, "hh8": pkg.MODE_OCV_HH8, "census": pkg.MODE_CENSUS8, "bm": pkg.MODE_OCV_BM}[mode]
    return pkg.default_params(mid, min_disparity=m, num_disparities=D, block_size=5)


def test_plan_examples(pkg):
    y = pkg.default_pyramid_params(level=1)
    for m, D, mc, Dc in [(0, 256, 0, 128), (0, 752, 0, 384), (147, 480, 73, 256)]:
        for mode in ("census", "sgbm5", "bm"):
            got = pkg.pyramid_plan(_params(pkg, mode, m, D), y, 2448, 2048)
            assert (got["Wc"], got["Hc"], got["mc"], got["Dc"]) == (1224, 1024, mc, Dc), (mode, m, D)
            assert got["invalid_c"] == (mc - 1) * 16 and got["invalid"] == (m - 1) * 16
    # level 0: the match geometry itself
    got = pkg.pyramid_plan(_params(pkg, "census", 3, 64), pkg.default_pyramid_params(), 333, 121)
    assert tuple(got.values()) == (333, 121, 3, 64, 32, 32)


def test_plan_sweep(pkg):
    """Seeded sweep over (W, H, m, D, mode) with negative and odd m, odd W / H: the formula of
    tests/pyramid_reference.py, and the status where the coarse match cannot run."""
    rng = np.random.default_rng(20260)
    y = pkg.default_pyramid_params(level=1, radius=1)
    seen = {"ok": 0, "refused": 0}
    for i in range(400):
        mode = MODES[i % 4]
        W, H = int(rng.integers(12, 5000)), int(rng.integers(12, 3200))
        m = int(rng.integers(-300, 300))
        D = 16 * int(rng.integers(1, 129))                   # 16 .. 2048
        want = pr.plan(W, H, m, D)
        refused = (mode == "census" and want[3] > 512) or (mode == "bm" and 5 >= min(want[0], want[1]))
        p = _params(pkg, mode, m, D)
        if refused:
            with pytest.raises(pkg.SGMError) as e:
                pkg.pyramid_plan(p, y, W, H)
            assert e.value.code == (pkg.SGM_ERR_UNSUPPORTED if mode == "census" else pkg.SGM_ERR_PARAM)
            seen["refused"] += 1
        else:
            assert tuple(pkg.pyramid_plan(p, y, W, H).values()) == want, (mode, W, H, m, D)
            seen["ok"] += 1
    assert seen["ok"] > 300 and seen["refused"] > 10, seen


def test_plan_errors_are_a_match_s_errors(pkg):
    y1 = pkg.default_pyramid_params(level=1)
    y0 = pkg.default_pyramid_params()

    def code(p, y, W, H, bm=None):
        try:
            pkg.pyramid_plan(p, y, W, H, bm)
            return 0
        except pkg.SGMError as e:
            return e.code

    c = _params(pkg, "census", 0, 1024)
    assert code(c, y0, 1100, 24) == pkg.SGM_ERR_UNSUPPORTED and code(c, y1, 1100, 24) == 0     # Dc = 512
    assert code(_params(pkg, "census", 0, 1040), y1, 1100, 24) == pkg.SGM_ERR_UNSUPPORTED      # Dc = 528
    assert code(_params(pkg, "sgbm5", 0, 2048), y1, 3000, 24) == 0
    assert code(_params(pkg, "sgbm5", 0, 2064), y1, 3000, 24) == pkg.SGM_ERR_UNSUPPORTED       # D <= 2048 stays
    assert code(_params(pkg, "census", 0, 2064), y1, 3000, 24) == pkg.SGM_ERR_UNSUPPORTED
    assert code(_params(pkg, "census", 0, 40), y1, 300, 24) == pkg.SGM_ERR_PARAM               # D % 16
    assert code(_params(pkg, "census", 0, 0), y1, 300, 24) == pkg.SGM_ERR_PARAM
    assert code(_params(pkg, "census", 0, 64), y1, 0, 24) == pkg.SGM_ERR_ARG
    assert code(_params(pkg, "census", 0, 64), y1, 40000, 24) == pkg.SGM_ERR_UNSUPPORTED
    # BM: the window is checked against the coarse size too; the BM-only pair as at level 0
    b = _params(pkg, "bm", 0, 32).copy(block_size=21)
    assert code(b, y0, 40, 40) == 0 and code(b, y1, 40, 40) == pkg.SGM_ERR_PARAM               # 21 >= 20
    assert code(b, y1, 44, 43) == 0                                                            # 21 < 22
    assert code(b, y1, 44, 43, pkg.default_bm_params(texture_threshold=-1)) == pkg.SGM_ERR_PARAM
    assert code(b.copy(disp12_max_diff=1), y1, 44, 43) == pkg.SGM_ERR_UNSUPPORTED
    p = pkg.default_params(7)
    assert code(p, y1, 300, 24) == pkg.SGM_ERR_PARAM                                            # unknown mode


def test_census_cap_note(pkg):
    """d 1..1024 halves to 0..512: 513 values, Dc 528, over the census cap."""
    assert pr.plan(1100, 24, 1, 1024)[3] == 528
    with pytest.raises(pkg.SGMError) as e:
        pkg.pyramid_plan(_params(pkg, "census", 1, 1024), pkg.default_pyramid_params(level=1), 1100, 24)
    assert e.value.code == pkg.SGM_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------ the adapters
PYR_ENV = [(None, (0, 0)), ("", (0, 0)), ("  ", (0, 0)), ("0", (0, 0)), ("1", (1, 0)), (" 1\t", (1, 0)),
           ("scale", (0, 1)), (" Scale ", (0, 1)), ("2", (0, 0)), ("on", (0, 0)), ("01", (0, 0)), ("1.0", (0, 0)),
           ("-1", (0, 0)), ("scale:1", (0, 0))]


def _driver(monkeypatch, val):
    if val is None:
        monkeypatch.delenv("SGM_HIP_PYRAMID", raising=False)
    else:
        monkeypatch.setenv("SGM_HIP_PYRAMID", val)
    r = subprocess.run([DRIVER, "env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


@pytest.mark.parametrize("val,want", PYR_ENV)
def test_pyramid_env_parses_the_same_in_python_and_cpp(pkg, monkeypatch, capfd, val, want):
    lines, err = _driver(monkeypatch, val)
    assert pkg.pyramid_from_env() == (want[0], bool(want[1]))
    py_err = capfd.readouterr().err
    assert lines[0] == "env level %d follow %d" % want
    m = pkg.MatcherHIPSGM(" ", (0, 0), mode=pkg.MODE_CENSUS8)
    assert (m.pyramid_level, m.pyramid_scale) == (want[0], bool(want[1]))
    noted = val is not None and val.strip() not in ("", "0", "1") and val.strip().lower() != "scale"
    assert ("SGM_HIP_PYRAMID=" in err) == noted and ("SGM_HIP_PYRAMID=" in py_err) == noted
    # setDownsampleScale drives the level only under "scale": s <= 0.5 -> 1, else 0
    got = {}
    for s in (1.0, 0.5, 0.25, 0.75):
        m.setDownsampleScale(s)
        got[s] = m.pyramid_level
    follow = {1.0: 0, 0.5: 1, 0.25: 1, 0.75: 0}
    assert got == (follow if want[1] else {s: want[0] for s in follow})
    assert lines[1:5] == ["scale %.2f level %d" % (s, got[s]) for s in (1.0, 0.5, 0.25, 0.75)]
    m.setPyramidLevel(1)
    m.setDownsampleScale(1)                       # the node's per-frame call
    assert m.pyramid_level == (0 if want[1] else 1)
    assert lines[5] == "set level %d" % m.pyramid_level
    assert m.downsample_scale == 1                # stored; no CPU resize exists in the adapter


# ------------------------------------------------------------------------------ the new kernels
def test_the_pyramid_kernels(pkg):
    """The feature adds three gfx950 kernels (k_pyr_down, k_pyr_refine<1>, k_pyr_refine<2>): no
    scratch, 256-thread blocks, the down kernel's 1440 B LDS tile and no LDS in the refinement, and
    few enough VGPRs for eight waves per SIMD (64) in every one."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgm_kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    kernels = kd.library_kernels(pkg.LIB_PATH)
    down = [k for k in kernels if "k_pyr_down" in k]
    refine = [k for k in kernels if "k_pyr_refine" in k]
    assert len(down) == 1 and len(refine) == 2, (down, refine)
    for k in down + refine:
        meta = kernels[k]["meta"]
        assert meta[".private_segment_fixed_size"] == "0", (k, meta)
        assert int(meta[".max_flat_workgroup_size"]) == 256 and int(meta[".vgpr_count"]) <= 64, (k, meta)
    assert int(kernels[down[0]]["meta"][".group_segment_fixed_size"]) == 1440
    assert all(int(kernels[k]["meta"][".group_segment_fixed_size"]) == 0 for k in refine)
