"""CPU tests of MODE_OCV_BM: self-checks of the numpy reference (tests/bm_reference.py), its
golden fixtures, and the C-ABI / Python surface of the mode (no compute calls)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bm_reference as br  # noqa: E402


# ---------------------------------------------------------------- the reference itself
def test_reference_constant_image_has_no_texture():
    z = np.full((40, 96), 77, np.uint8)
    assert (br.compute(br.BM(0, 32, 9, 31, 10, 15), z, z) == -16).all()


def test_reference_constant_image_ties_take_largest_disparity():
    z = np.full((40, 96), 77, np.uint8)
    d = br.compute(br.BM(0, 32, 9, 31, 0, 0), z, z)
    assert (d[4:36, 31:] == (0 + 32 - 1) * 16).all()          # every computed pixel: 496
    assert (d[:4] == -16).all() and (d[36:] == -16).all() and (d[:, :31] == -16).all()


def test_reference_integer_shift(synth):
    left, right = synth.integer_shift_pair(40, 96, 11, seed=5)
    d = br.compute(br.BM(0, 32, 9, 31, 10, 15), left, right)[4:36, 35:81].astype(int)
    assert (d != -16).all()
    print("max |out - 176| =", np.abs(d - 176).max())
    assert np.abs(d - 176).max() <= 8 and (((d + 8) >> 4) == 11).all()


def test_reference_odd_height_rule(synth):
    """H odd: the last row of the pre-filtered image is the cap, so an H = 41 frame and the first
    41 rows of its H = 42 version differ exactly where a window (w = 5) reaches row 40."""
    left, right, _ = synth.stereo_pair(42, 90, -8, 16, seed=2)
    bm = br.BM(-8, 16, 5, 7, 10, 2)
    a = br.compute(bm, left[:41], right[:41])
    b = br.compute(bm, left, right)[:41]
    assert sorted(set(np.nonzero((a != b).any(1))[0].tolist())) == [38, 39]


@pytest.mark.parametrize("name", ["bm_node_defaults_64x128", "bm_negmin_41x90"])
def test_reference_golden(name):
    g = np.load(os.path.join(HERE, "golden", "bm", name + ".npz"))
    bm = br.BM(*[int(v) for v in g["bm"]])
    assert np.array_equal(br.compute(bm, g["left"], g["right"]), g["disp"])
    assert np.array_equal(br.prefilter(g["left"], bm.c), g["prefiltered_left"])


# ---------------------------------------------------------------- C-ABI
def bm_defaults(pkg, **kw):
    return pkg.default_params(pkg.MODE_OCV_BM, **kw)


def test_abi_version_and_struct_sizes(pkg):
    assert pkg.load_library().sgm_abi_version() == 5 == pkg.ABI_VERSION
    assert ctypes.sizeof(pkg.SgmParams) == 60 and ctypes.sizeof(pkg.BmParams) == 8
    assert pkg.MODE_OCV_BM == 3 and pkg.HIP_StereoBM == 7


def test_bm_defaults_are_the_node_defaults(pkg):
    p = bm_defaults(pkg)
    assert (p.mode, p.min_disparity, p.num_disparities, p.block_size, p.uniqueness_ratio, p.prefilter_cap,
            p.speckle_window_size, p.speckle_range, p.disp12_max_diff) == (3, 9, 64, 15, 15, 31, 100, 4, -1)
    b = pkg.default_bm_params()
    assert (b.texture_threshold, b.prefilter_size) == (10, 9)
    assert pkg.load_library().sgm_check_params(ctypes.byref(p), 640, 480) == pkg.SGM_OK


@pytest.mark.parametrize("kw", [dict(prefilter_cap=0), dict(prefilter_cap=64), dict(block_size=3), dict(block_size=257),
                                dict(block_size=14), dict(block_size=481),
                                dict(num_disparities=0), dict(num_disparities=-16), dict(num_disparities=40),
                                dict(uniqueness_ratio=-1)], ids=str)
def test_check_params_rejects(pkg, kw):
    lib = pkg.load_library()
    p = bm_defaults(pkg, **kw)
    assert lib.sgm_check_params(ctypes.byref(p), 640, 480) == pkg.SGM_ERR_PARAM


@pytest.mark.parametrize("kw", [dict(prefilter_size=3), dict(prefilter_size=257), dict(prefilter_size=8),
                                dict(texture_threshold=-1)], ids=str)
def test_check_bm_params_rejects(pkg, kw):
    lib = pkg.load_library()
    p = bm_defaults(pkg)
    b = pkg.default_bm_params(**kw)
    assert lib.sgm_check_bm_params(ctypes.byref(p), ctypes.byref(b), 640, 480) == pkg.SGM_ERR_PARAM
    b = pkg.default_bm_params()
    assert lib.sgm_check_bm_params(ctypes.byref(p), ctypes.byref(b), 640, 480) == pkg.SGM_OK


def test_check_params_unsupported(pkg):
    lib = pkg.load_library()
    for kw in (dict(disp12_max_diff=0), dict(disp12_max_diff=1), dict(num_disparities=2064)):
        p = bm_defaults(pkg, **kw)
        assert lib.sgm_check_params(ctypes.byref(p), 4096, 3000) == pkg.SGM_ERR_UNSUPPORTED
    p = bm_defaults(pkg, num_disparities=2048)
    assert lib.sgm_check_params(ctypes.byref(p), 4096, 3000) == pkg.SGM_OK
    p = bm_defaults(pkg)
    assert lib.sgm_check_params(ctypes.byref(p), 100, 15) == pkg.SGM_ERR_PARAM      # w >= min(W, H)
    assert lib.sgm_check_params(ctypes.byref(p), 100, 16) == pkg.SGM_OK
    p.mode = 4
    assert lib.sgm_check_params(ctypes.byref(p), 640, 480) == pkg.SGM_ERR_PARAM


def test_bm_params_round_trip_without_a_device(pkg):
    """set / get on a handle need a device only to create it: the null-handle paths are checked
    here, the round trip on a real handle in the GPU suite (Engine.set_bm_params / get_bm_params)."""
    lib = pkg.load_library()
    b = pkg.default_bm_params(texture_threshold=33, prefilter_size=11)
    assert lib.sgm_set_bm_params(None, ctypes.byref(b)) == pkg.SGM_ERR_ARG
    assert lib.sgm_get_bm_params(None, ctypes.byref(b)) == pkg.SGM_ERR_ARG
    assert (b.texture_threshold, b.prefilter_size) == (33, 11)
    c = b.copy(prefilter_size=13)
    assert (c.texture_threshold, c.prefilter_size, b.prefilter_size) == (33, 13, 11)
    if pkg.device_count() > 0:
        eng = pkg.Engine(0)
        eng.set_bm_params(b)
        assert eng.get_bm_params().as_dict() == dict(texture_threshold=33, prefilter_size=11)
        eng.close()


# ---------------------------------------------------------------- Python mirror / plugin core
def test_matcher_bm_mode_setters(pkg):
    m = pkg.MatcherHIPSGM(" ", (640, 480), mode=pkg.MODE_OCV_BM)
    p = m.params                                     # cv::StereoBM::create(64, 9)
    assert (p.mode, p.min_disparity, p.num_disparities, p.block_size, p.prefilter_cap, p.uniqueness_ratio,
            p.speckle_window_size, p.disp12_max_diff) == (3, 0, 64, 9, 31, 15, 0, -1)
    assert m.bm_params.as_dict() == dict(texture_threshold=10, prefilter_size=9)
    pkg.update_matcher(m, dict(pkg.NODE_DEFAULTS, texture_threshold=25, prefilter_size=11))
    assert m.bm_params.as_dict() == dict(texture_threshold=25, prefilter_size=11)
    assert (m.params.min_disparity, m.params.block_size, m.params.speckle_window_size, m.params.disp12_max_diff) == \
        (9, 15, 100, -1)                             # disp12MaxDiff is not forwarded by the node
    r = pkg.right_matcher_params(m.params)
    assert (r.min_disparity, r.num_disparities, r.block_size, r.uniqueness_ratio, r.speckle_window_size,
            r.disp12_max_diff) == (-72, 64, 15, 0, 0, -1)
    assert pkg.right_matcher_bm_params(m.bm_params).as_dict() == dict(texture_threshold=0, prefilter_size=11)
    s = pkg.MatcherHIPSGM(" ", (640, 480), mode=pkg.MODE_OCV_SGBM5)
    s.setTextureThreshold(25)                        # still a no-op outside BM mode
    assert s.bm_params.texture_threshold == 10


def test_parameter_callback_treats_hip_bm_like_opencv(pkg):
    state = {"first": True}
    cfg = pkg.parameter_callback({}, state)
    cfg.update(stereo_algorithm=pkg.HIP_StereoBM, correlation_window_size=20, disparity_range=100, prefilter_size=6)
    cfg = pkg.parameter_callback(cfg, state)
    assert (cfg["correlation_window_size"], cfg["disparity_range"], cfg["prefilter_size"]) == (21, 96, 7)


def test_plugin_core_bm_setters():
    exe = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_bm_test")
    r = subprocess.run([exe, "setters"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
