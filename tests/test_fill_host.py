"""CPU tests of the hole-filling feature: the numpy reference against its known answers, the C-ABI
surface (symbols, defaults, null handles, validation), the adapters' two environment variables in
Python and C++ alike, and the new kernel's resources.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_reference as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fill")
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_fill_test")
NEW = ["sgm_default_fill_params", "sgm_set_fill_params", "sgm_get_fill_params", "sgm_check_fill_params",
       "sgm_fill_holes", "sgm_debug_fill"]


# ------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("case", fr.KAT_CASES)
def test_reference_known_answers(case):
    kat = np.load(os.path.join(GOLDEN, "fill_kat.npz"))
    fresh = fr.make_kat()
    assert sorted(kat.files) == sorted(fresh)
    for k in kat.files:                       # the committed file is what make_kat() writes
        assert np.array_equal(kat[k], fresh[k]) and kat[k].dtype == fresh[k].dtype, k
    inv, mode, G, N, x0, y0, x1, y1 = (int(v) for v in kat[case + "_par"])
    img = fr.kat_input(kat, case)
    for f in (fr.fill_holes, fr.fill_holes_naive):
        got = f(img, inv, mode, G, N, (x0, y0, x1, y1))
        assert got.dtype == np.int16 and np.array_equal(got, kat[case + "_out"]), f.__name__


def test_reference_known_answers_by_hand():
    """The golden outputs say what the specification says (independent of both reference forms)."""
    kat = np.load(os.path.join(GOLDEN, "fill_kat.npz"))
    s = kat["single_out"]
    G = int(kat["single_par"][2])
    assert (s == 777).sum() == 8 * G + 1
    for dx, dy in fr.DIRS:
        assert s[20 + G * dy, 20 + G * dx] == 777 and s[20 + (G + 1) * dy, 20 + (G + 1) * dx] == -16
    assert kat["eight_bg_out"][4, 4] == 20 and kat["eight_med_out"][4, 4] == 40      # of 10, 20, .. 80
    assert kat["few_out"][3, 3] == -16 and kat["few3_out"][3, 3] == 7                # 3 candidates: 5, 7, 9
    r = kat["rect_out"]
    assert r[2, 1] == -16 and r[2, 6] == -16 and r[2, 3] == 100 and r[2, 4] == 100


def test_reference_forms_agree_and_order_does_not_matter():
    rng = np.random.default_rng(12)
    for _ in range(40):
        h, w = int(rng.integers(1, 20)), int(rng.integers(1, 26))
        inv = int(rng.choice([-16, 128]))
        img = rng.integers(-40, 200, (h, w)).astype(np.int16)
        img[rng.random((h, w)) < rng.choice([0.1, 0.5, 0.95])] = inv
        G, N, mode = int(rng.choice([1, 2, 5, 30])), int(rng.integers(1, 9)), int(rng.choice([1, 2]))
        x0, y0 = int(rng.integers(0, w + 1)), int(rng.integers(0, h + 1))
        rect = (x0, y0, int(rng.integers(x0, w + 1)), int(rng.integers(y0, h + 1)))
        a = fr.fill_holes(img, inv, mode, G, N, rect)
        assert np.array_equal(a, fr.fill_holes_naive(img, inv, mode, G, N, rect))
        # mirrored input, mirrored output: nothing depends on a scan order
        b = fr.fill_holes(img[::-1, ::-1], inv, mode, G, N, (w - rect[2], h - rect[3], w - rect[0], h - rect[1]))
        assert np.array_equal(a, b[::-1, ::-1])
        keep = np.ones((h, w), bool)
        keep[rect[1]:rect[3], rect[0]:rect[2]] = img[rect[1]:rect[3], rect[0]:rect[2]] != inv
        assert np.array_equal(a[keep], img[keep])
    assert np.array_equal(fr.fill_holes(img, inv, fr.OFF, 0, 0), img)


def test_match_rectangle():
    assert fr.match_rect(False, 3, 64, 0, 300, 70) == (67, 0, 300, 70)
    assert fr.match_rect(False, -5, 128, 0, 330, 120) == (123, 0, 325, 120)
    assert fr.match_rect(True, 0, 32, 9, 96, 48) == (31, 4, 96, 44)
    assert fr.match_rect(True, -4, 32, 5, 96, 48) == (27, 2, 92, 46)
    x0, _, x1, _ = fr.match_rect(False, 0, 64, 0, 40, 10)
    assert x0 == x1                                                # no window: nothing to fill


# --------------------------------------------------------------------------------- the C ABI
def test_symbols_exported_and_declared(pkg):
    lib = pkg.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgm_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sgm_\w+)", out))
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in exported and hasattr(lib, s) and s in pkg.EXPORTS, s
    for name, val in (("SGM_FILL_OFF", 0), ("SGM_FILL_BACKGROUND", 1), ("SGM_FILL_MEDIAN", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"typedef struct sgm_fill_params\s*\{\s*int mode;.*?int max_gap;.*?int min_neighbours;", hdr, re.S)
    assert (pkg.FILL_OFF, pkg.FILL_BACKGROUND, pkg.FILL_MEDIAN) == (0, 1, 2) == (fr.OFF, fr.BACKGROUND, fr.MEDIAN)
    assert lib.sgm_abi_version() == 5                              # callers check for the symbols
    assert "sgm_launch.h" in open(os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "csrc", "fill.hip")).read()
    be = open(os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "build_ext.py")).read()
    assert '"fill.hip"' in be


def test_defaults_and_null_handles(pkg):
    lib = pkg.load_library()
    assert ctypes.sizeof(pkg.FillParams) == 12
    f = pkg.default_fill_params()
    assert (f.mode, f.max_gap, f.min_neighbours) == (pkg.FILL_OFF, 16, 2)
    lib.sgm_default_fill_params(None)                             # ignored
    assert pkg.default_fill_params(mode=2, max_gap=9).as_dict() == dict(mode=2, max_gap=9, min_neighbours=2)
    assert f.copy(min_neighbours=5).min_neighbours == 5 and f.min_neighbours == 2
    assert lib.sgm_set_fill_params(None, ctypes.byref(f)) == pkg.SGM_ERR_ARG
    assert lib.sgm_get_fill_params(None, ctypes.byref(f)) == pkg.SGM_ERR_ARG
    assert lib.sgm_check_fill_params(None) == pkg.SGM_ERR_ARG
    assert lib.sgm_fill_holes(None, None, 0, 4, 4, -16, ctypes.byref(f), 0, 0, 4, 4, None, 0, None) == pkg.SGM_ERR_ARG
    assert lib.sgm_debug_fill(None, None, 4, 4, -16, ctypes.byref(f), 0, 0, 4, 4) == pkg.SGM_ERR_ARG


@pytest.mark.parametrize("mode,gap,n,status", [(0, 16, 2, 0), (0, 0, 0, 0), (0, 999, -3, 0), (1, 1, 1, 0), (2, 255, 8, 0),
                                               (1, 0, 2, -2), (1, 256, 2, -2), (2, -1, 2, -2), (2, 16, 0, -2),
                                               (1, 16, 9, -2), (3, 16, 2, -2), (-1, 16, 2, -2)])
def test_validation(pkg, mode, gap, n, status):
    """With a mode other than OFF: a known mode, max_gap in 1..255, min_neighbours in 1..8."""
    f = pkg.FillParams(mode, gap, n)
    assert pkg.load_library().sgm_check_fill_params(ctypes.byref(f)) == status


# ------------------------------------------------------------------------------ the adapters
FILL_ENV = [(None, (0, 16, 2)), ("", (0, 16, 2)), ("  ", (0, 16, 2)), ("off", (0, 16, 2)), ("background", (1, 16, 2)),
            ("median", (2, 16, 2)), ("Median:7", (2, 7, 2)), (" background:31:4\t", (1, 31, 4)), ("median:0:9", (2, 0, 9)),
            ("median:999999:1", (2, 999999, 1)), ("off:5:5", (0, 5, 5)), ("median:1234567", (0, 16, 2)),
            ("median:", (0, 16, 2)), ("median:7:", (0, 16, 2)), ("median:-7", (0, 16, 2)), ("median:+7", (0, 16, 2)),
            ("median:7:3:1", (0, 16, 2)), ("fast", (0, 16, 2)), ("median:0x10", (0, 16, 2)), ("median: 7", (0, 16, 2)),
            ("1", (0, 16, 2))]


def _driver_env(monkeypatch, fill, when):
    for k, v in (("SGM_HIP_FILL", fill), ("SGM_HIP_FILL_WHEN", when)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    r = subprocess.run([DRIVER, "env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        *tag, a, b, c = line.split() if line.startswith(("env fill", "interp", "set fill")) else (line.split() + ["", ""])
        out[" ".join(tag)] = (int(a), int(b), int(c)) if b != "" else int(a)
    return out, r.stderr


@pytest.mark.parametrize("val,want", FILL_ENV)
def test_fill_env_parses_the_same_in_python_and_cpp(pkg, monkeypatch, capfd, val, want):
    out, err = _driver_env(monkeypatch, val, None)
    assert pkg.fill_from_env() == want
    py_err = capfd.readouterr().err
    assert out["env fill"] == want
    m = pkg.MatcherHIPSGM(" ", (0, 0), mode=pkg.MODE_CENSUS8)
    assert (m.fill.mode, m.fill.max_gap, m.fill.min_neighbours) == want and m.fill_when == "always"
    noted = val is not None and val.strip() != "" and want == (0, 16, 2) and not val.strip().lower().startswith("off")
    assert ("SGM_HIP_FILL=" in err) == noted and ("SGM_HIP_FILL=" in py_err) == noted      # a note on stderr, both


@pytest.mark.parametrize("when,interp_drives", [(None, False), ("", False), ("always", False), ("interp", True),
                                                (" Interp ", True), ("never", False)])
@pytest.mark.parametrize("fill", [None, "median:5:3"])
def test_fill_when(pkg, monkeypatch, fill, when, interp_drives):
    """always (the default): the configured filter runs whatever interp says, and interp on is Q3.
    interp: off without the flag; with it the configured filter (background when none is named)
    and no Q3."""
    out, err = _driver_env(monkeypatch, fill, when)
    conf = (2, 5, 3) if fill else (0, 16, 2)
    m = pkg.MatcherHIPSGM(" ", (0, 0), mode=pkg.MODE_CENSUS8)
    assert m.fill_when == ("interp" if interp_drives else "always")
    assert ("SGM_HIP_FILL_WHEN=" in err) == (when == "never")
    eff = {}
    for flag in (False, True):
        m.setInterpolation(flag)
        e = m.effective_fill()
        eff[flag] = ((e.mode, e.max_gap, e.min_neighbours), int(m.q3()))
    if interp_drives:
        on = conf if fill else (1, 16, 2)
        want = {False: ((0,) + conf[1:], 0), True: (on, 0)}
    else:
        want = {False: (conf, 0), True: (conf, 1)}
    assert eff == want
    assert (out["interp off"], out["q3 off"]) == want[False] and (out["interp on"], out["q3 on"]) == want[True]
    assert out["set fill"] == (2, 7, 3)
    m.setHoleFilling(pkg.FILL_MEDIAN, 7, 3)
    assert m.fill.as_dict() == dict(mode=2, max_gap=7, min_neighbours=3)


# ------------------------------------------------------------------------------ the new kernel
def test_the_fill_kernel(pkg):
    """The feature adds one gfx950 kernel, k_fill: no scratch, and within the 128 VGPRs that let a
    1024-thread block (the launcher's largest, for gaps above 160) be resident. That every earlier
    kernel stayed as it was is a comparison of two builds (tools/kernel_diff.py), not a
    property a test can hold on to."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgm_kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    kernels = kd.library_kernels(pkg.LIB_PATH)
    fill = [k for k in kernels if re.search(r"k_fill(?!16)", k)]
    assert len(fill) == 1, fill
    meta = kernels[fill[0]]["meta"]
    assert meta[".private_segment_fixed_size"] == "0" and int(meta[".vgpr_count"]) <= 128, meta
    assert int(meta[".max_flat_workgroup_size"]) == 1024, meta
