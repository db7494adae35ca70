"""Census windows (sgm_set_census_window), host side (no GPU): the exported symbols, the defaults,
the setter that stores anything, sgm_check_census_window over every window, the one slider table
(sgm_census_window_from_size, in C and in the Python mirror) and the SGM_HIP_CENSUS_WINDOW parser
of the C++ adapter core (plugin_window_test env) and of the Python mirror on one value list."""
import ctypes
import os
import subprocess

import pytest

import census_window_reference as cwr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_window_test")
NAMES = {"sgm_default_census_window", "sgm_set_census_window", "sgm_get_census_window", "sgm_check_census_window",
         "sgm_census_window_from_size"}


def test_library_exports_the_window_entry_points_under_abi_5(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert NAMES <= syms and NAMES <= set(pkg.EXPORTS)
    lib = pkg.load_library()
    assert lib.sgm_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "sgm_hip.h")).read()
    assert "#define SGM_ABI_VERSION 5" in hdr
    assert "typedef struct sgm_census_window { int taps_x, taps_y, step; } sgm_census_window;" in hdr
    assert ctypes.sizeof(pkg.CensusWindow) == 12
    assert ctypes.sizeof(pkg.SgmParams) == 15 * 4           # no struct grew


def test_default_window_and_null_handles(pkg):
    """What needs no handle. A handle needs a device (sgm_create checks that it is visible), so the
    setter that stores anything is tested on the GPU: test_gpu_census_window.py
    test_setter_stores_anything, and through the adapter core, which stores without a handle, in
    test_cpp_core_setters below."""
    lib = pkg.load_library()
    w = pkg.CensusWindow(1, 2, 3)
    lib.sgm_default_census_window(ctypes.byref(w))
    assert w.as_tuple() == (9, 7, 1) == cwr.DEFAULT == pkg.CENSUS_WINDOW_DEFAULT
    lib.sgm_default_census_window(None)                      # tolerated, like the other defaults
    assert lib.sgm_set_census_window(None, ctypes.byref(w)) == pkg.SGM_ERR_ARG
    assert lib.sgm_get_census_window(None, ctypes.byref(w)) == pkg.SGM_ERR_ARG


def test_check_accepts_exactly_the_24_windows(pkg):
    lib = pkg.load_library()
    assert lib.sgm_check_census_window(None) == pkg.SGM_ERR_ARG
    ok = set()
    for tx in range(-1, 13):
        for ty in range(-1, 11):
            for step in range(-1, 5):
                rc = lib.sgm_check_census_window(ctypes.byref(pkg.CensusWindow(tx, ty, step)))
                assert rc in (pkg.SGM_OK, pkg.SGM_ERR_PARAM)
                if rc == pkg.SGM_OK:
                    ok.add((tx, ty, step))
    assert ok == set(cwr.WINDOWS) and len(ok) == 24


TABLE = {-7: (3, 3, 1), 0: (3, 3, 1), 1: (3, 3, 1), 2: (3, 3, 1), 3: (3, 3, 1), 4: (5, 5, 1), 5: (5, 5, 1),
         6: (7, 7, 1), 7: (7, 7, 1), 8: (9, 7, 1), 9: (9, 7, 1), 10: (7, 7, 2), 11: (7, 7, 2), 12: (7, 7, 2),
         13: (7, 7, 2), 14: (9, 7, 2), 15: (9, 7, 2), 17: (9, 7, 2), 21: (9, 7, 2), 255: (9, 7, 2)}


def test_from_size_table(pkg):
    lib = pkg.load_library()
    assert lib.sgm_census_window_from_size(9, None) == pkg.SGM_ERR_ARG
    for size, want in TABLE.items():
        w = pkg.CensusWindow()
        assert lib.sgm_census_window_from_size(size, ctypes.byref(w)) == pkg.SGM_OK
        assert w.as_tuple() == want == pkg.census_window_from_size(size), size
        assert lib.sgm_check_census_window(ctypes.byref(w)) == pkg.SGM_OK


@pytest.mark.parametrize("val,want", [
    (None, ((9, 7, 1), False)), ("", ((9, 7, 1), False)), ("  ", ((9, 7, 1), False)),
    ("7x7", ((7, 7, 1), False)), ("9x7/2", ((9, 7, 2), False)), (" 5X3/1\t", ((5, 3, 1), False)),
    ("4x7", ((4, 7, 1), False)), ("9x7/3", ((9, 7, 3), False)),          # passed on: refused at match time
    ("cfg", ((9, 7, 1), True)), (" CFG ", ((9, 7, 1), True)),
    ("7", ((9, 7, 1), False)), ("7x", ((9, 7, 1), False)), ("x7", ((9, 7, 1), False)), ("7x7/", ((9, 7, 1), False)),
    ("7x7x7", ((9, 7, 1), False)), ("-7x7", ((9, 7, 1), False)), ("7x7/2/2", ((9, 7, 1), False)),
    ("7.0x7", ((9, 7, 1), False)), ("1234567x7", ((9, 7, 1), False)), ("seven", ((9, 7, 1), False)),
])
def test_env_parses_alike_in_cpp_and_python(pkg, monkeypatch, val, want):
    """One value list through the Python mirror and through the C++ adapter core (plugin_window_test
    env): the same window and cfg flag, and with cfg the same window after every setWindowSize."""
    if val is None:
        monkeypatch.delenv("SGM_HIP_CENSUS_WINDOW", raising=False)
    else:
        monkeypatch.setenv("SGM_HIP_CENSUS_WINDOW", val)
    assert pkg.census_window_from_env() == want
    m = pkg.MatcherHIPSGM(mode=pkg.MODE_CENSUS8)
    assert (m.census_window, m.census_window_cfg) == want
    lines = _driver_env()
    (tx, ty, step), cfg = want
    assert lines[0] == f"env window {tx} {ty} {step}" and lines[1] == f"env cfg {int(cfg)}"
    sizes = [l.split() for l in lines if l.startswith("size ")]
    assert [int(t[1]) for t in sizes] == list(TABLE)
    for t in sizes:
        m.setWindowSize(int(t[1]))
        assert tuple(int(v) for v in t[3:6]) == m.census_window == (TABLE[int(t[1])] if cfg else want[0])
    # a bad value warns on stderr in both, naming the variable
    bad = val is not None and val.strip() and want == ((9, 7, 1), False) and val.strip().lower() != "9x7"
    assert ("SGM_HIP_CENSUS_WINDOW" in _driver_env.stderr) == bool(bad)


def _driver_env():
    r = subprocess.run([DRIVER, "env"], capture_output=True, text=True, env=dict(os.environ), timeout=60)
    assert r.returncode == 0, r.stderr
    _driver_env.stderr = r.stderr
    return r.stdout.split("\n")


def test_cpp_core_setters(monkeypatch):
    """MatcherCore::setCensusWindow stores anything, and setWindowSize keeps block_size (the driver
    checks it) whether or not it drives the window."""
    monkeypatch.delenv("SGM_HIP_CENSUS_WINDOW", raising=False)
    lines = _driver_env()
    assert "set window 5 3 2" in lines and "set window 4 0 -1" in lines


def test_adapter_window_is_opt_in(pkg, monkeypatch):
    """Unset: setWindowSize leaves the census window alone (the node's default slider value is 15
    and existing census users keep their results); cfg: it drives it through the one table."""
    monkeypatch.delenv("SGM_HIP_CENSUS_WINDOW", raising=False)
    m = pkg.MatcherHIPSGM(mode=pkg.MODE_CENSUS8)
    m.setWindowSize(15)
    assert m.census_window == (9, 7, 1) and m.params.block_size == 15
    m.setCensusWindow(5, 3, 2)
    assert m.census_window == (5, 3, 2)
    monkeypatch.setenv("SGM_HIP_CENSUS_WINDOW", "cfg")
    m = pkg.MatcherHIPSGM(mode=pkg.MODE_CENSUS8)
    assert m.census_window == (9, 7, 1)
    for size, want in TABLE.items():
        m.setWindowSize(size)
        assert m.census_window == want
