"""Census path sets (sgm_set_census_paths), host side (no GPU): the composed reference the GPU
tests compare with, the exported symbols and defaults, the SGM_HIP_CENSUS_PATHS parser of the
C++ adapter core and of the Python mirror, and the 4-path work list of a steady batch launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import census_paths_reference as cpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_paths_test")

# (h, w, parameters): the four frames the composition was pinned on
CONFIGS = [
    (48, 96, dict(num_disparities=32)),
    (37, 150, dict(num_disparities=64, min_disparity=3, median=1, speckle_window_size=30, speckle_range=2)),
    (40, 300, dict(num_disparities=144, min_disparity=-5)),
    (33, 330, dict(num_disparities=272, subpixel=0, lr_check=0)),
]


@pytest.mark.parametrize("h,w,kw", CONFIGS, ids=[str(i) for i in range(len(CONFIGS))])
def test_eight_direction_composition_is_the_oracle_match(oracle, synth, h, w, kw):
    """The helper with all eight directions equals oracle.match bit for bit, and with the four
    axis directions it gives another image (a wrong path set cannot pass the GPU tests)."""
    D, minD = kw["num_disparities"], kw.get("min_disparity", 0)
    left, right, _ = synth.stereo_pair(h, w, max(minD, 0), D, seed=D + 5)
    p = oracle.make_params(oracle.MODE_CENSUS8, **kw)
    full = oracle.match(p, left, right)
    assert np.array_equal(cpr.match_paths(oracle, p, left, right, dirs=range(8)), full)
    four = cpr.match_paths(oracle, p, left, right)
    frac = float((four != full).mean())
    print(f"{h}x{w} D={D}: 4 paths differ from 8 paths in {100 * frac:.1f} % of the pixels")
    assert frac > 0.01


def test_no_window_frame_is_all_invalid(oracle):
    p = oracle.make_params(oracle.MODE_CENSUS8, num_disparities=64, median=1, speckle_window_size=10, speckle_range=1)
    z = np.zeros((9, 40), np.uint8)
    assert (cpr.match_paths(oracle, p, z, z) == -16).all()
    assert np.array_equal(cpr.match_paths(oracle, p, z, z), oracle.match(p, z, z))


def test_library_exports_the_path_set_entry_points(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"sgm_set_census_paths", "sgm_get_census_paths"} <= syms
    assert {"sgm_set_census_paths", "sgm_get_census_paths"} <= set(pkg.EXPORTS)
    lib = pkg.load_library()
    assert lib.sgm_set_census_paths and lib.sgm_get_census_paths
    hdr = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    assert "sgm_set_census_paths(sgm_handle* h, int paths)" in hdr
    assert "sgm_get_census_paths(const sgm_handle* h, int* paths)" in hdr


def test_default_is_eight_paths(pkg, monkeypatch):
    """A fresh handle reports 8 where a handle can be made; without a device the null-handle
    answers and the Python defaults are checked."""
    lib = pkg.load_library()
    n = ctypes.c_int(-1)
    assert lib.sgm_get_census_paths(None, ctypes.byref(n)) == pkg.SGM_ERR_ARG
    assert lib.sgm_set_census_paths(None, 4) == pkg.SGM_ERR_ARG
    h = ctypes.c_void_p()
    if lib.sgm_create(ctypes.byref(h), 0) == pkg.SGM_OK:
        try:
            assert lib.sgm_get_census_paths(h, ctypes.byref(n)) == pkg.SGM_OK and n.value == 8
            assert lib.sgm_get_census_paths(h, None) == pkg.SGM_ERR_ARG
            assert lib.sgm_set_census_paths(h, 5) == pkg.SGM_OK          # setters store any value
            assert lib.sgm_get_census_paths(h, ctypes.byref(n)) == pkg.SGM_OK and n.value == 5
        finally:
            lib.sgm_destroy(h)
    monkeypatch.delenv("SGM_HIP_CENSUS_PATHS", raising=False)
    assert pkg.census_paths_from_env() == 8
    assert pkg.MatcherHIPSGM(mode=pkg.MODE_CENSUS8).census_paths == 8
    assert pkg.MatcherHIPSGM(mode=pkg.MODE_CENSUS8, census_paths=4).census_paths == 4


@pytest.mark.parametrize("val,want", [(None, 8), ("4", 4), ("8", 8), (" 4\t", 4), ("", 8), ("  ", 8), ("+4", 4),
                                      ("5", 5), ("-4", -4), ("four", 8), ("4x", 8), ("0x4", 8), ("4.0", 8),
                                      ("99999999999999999999", 8), ("+", 8)])
def test_env_parses_alike_in_cpp_and_python(pkg, monkeypatch, val, want):
    if val is None:
        monkeypatch.delenv("SGM_HIP_CENSUS_PATHS", raising=False)
    else:
        monkeypatch.setenv("SGM_HIP_CENSUS_PATHS", val)
    assert pkg.census_paths_from_env() == want
    assert pkg.MatcherHIPSGM(mode=pkg.MODE_CENSUS8).census_paths == want
    r = subprocess.run([DRIVER, "env"], capture_output=True, text=True, env=dict(os.environ))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == f"env paths {want}" and lines[1] == "set paths 4"


def _items(pkg, W, H, D, minD, mask, slots, group, up):
    lib = pkg.load_library()
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=minD)
    n = lib.sgm_debug_path_items(ctypes.byref(p), W, H, mask, slots, group, up, None, 0)
    assert n >= 0
    out = np.zeros(max(n, 1), np.uint32)
    assert lib.sgm_debug_path_items(ctypes.byref(p), W, H, mask, slots, group, up,
                                     out.ctypes.data_as(ctypes.c_void_p), n) == n
    return out[:n]


@pytest.mark.parametrize("W,H,D,minD", [(1920, 1080, 128, 0), (640, 45, 48, 3), (500, 20, 400, -7)])
def test_four_path_work_list(pkg, W, H, D, minD):
    """Mask 0xC3 lists dirs 0, 1, 6, 7 (the steady launch skips dir 1 in the kernel) next to the
    up+WTA blocks (code 8) and nothing else: no diagonal blocks."""
    it = _items(pkg, W, H, D, minD, cpr.MASK4, 256, 2, 2)
    code = it >> 24
    assert set(code.tolist()) == {0, 1, 6, 7, 8}
    assert set(code[code != 1].tolist()) == {0, 6, 7, 8}            # what a steady launch sweeps
    full = _items(pkg, W, H, D, minD, 0xFF, 256, 2, 2)
    for d in (0, 1, 6, 7, 8):                                       # the same blocks as in the 8-path list
        assert sorted(it[code == d].tolist()) == sorted(full[(full >> 24) == d].tolist())
    # the list without the skipped direction (mask 0xC3 minus bit 1): only dirs 0, 6, 7 and code 8
    steady = _items(pkg, W, H, D, minD, cpr.MASK4 & ~2, 256, 2, 2)
    assert set((steady >> 24).tolist()) == {0, 6, 7, 8}
    assert sorted(steady.tolist()) == sorted(it[code != 1].tolist())
    n_up = int((code == 8).sum())
    assert n_up and (code[:min(n_up, 256)] == 8).all()              # the longest chains lead
