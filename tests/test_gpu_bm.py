"""GPU parity of MODE_OCV_BM (cv::StereoBM, csrc/bm.hip) against tests/bm_reference.py, the numpy
reference written from the specification in DESIGN.md. Every result must be bit-exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm_reference as br  # noqa: E402

pytestmark = pytest.mark.gpu

# (H, W, m, D, w, c, t, u, seed): the issue's table; '-' entries filled in here
CASES = [
    (48, 96, 0, 32, 9, 31, 10, 15, 0),
    (64, 128, 9, 64, 15, 31, 10, 15, 1),       # node defaults, m > 0
    (41, 90, -8, 16, 5, 7, 10, 2, 2),          # odd H
    (47, 160, 3, 48, 21, 63, 0, 0, 3),         # D not a multiple of 64
    (33, 70, -40, 16, 5, 31, 10, 15, 4),       # s < 0: right offset
    (56, 333, 0, 272, 23, 63, 10, 15, 5),      # 529 * 126 > 65535: u32 sums, D over several chunks, odd W
]
_refs = {}


def params_of(pkg, bm, **kw):
    d = dict(min_disparity=bm.m, num_disparities=bm.D, block_size=bm.w, prefilter_cap=bm.c,
             uniqueness_ratio=bm.u, speckle_window_size=0, speckle_range=0, disp12_max_diff=-1)
    d.update(kw)
    return pkg.default_params(pkg.MODE_OCV_BM, **d)


def setup(engine, pkg, bm, **kw):
    engine.set_params(params_of(pkg, bm, **kw))
    engine.set_bm_params(pkg.default_bm_params(texture_threshold=bm.t))


def case(synth, c):
    """(bm, left, right, reference disparity), computed once per case and never modified."""
    if c not in _refs:
        H, W, m, D, w, cap, t, u, seed = c
        left, right, _ = synth.stereo_pair(H, W, m, D, seed=seed)
        bm = br.BM(m, D, w, cap, t, u)
        ref = br.compute(bm, left, right)
        ref.setflags(write=False)
        _refs[c] = (bm, left, right, ref)
    return _refs[c]


def diff_msg(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} pixels differ, first {bad[:5].tolist()}: got {[int(got[tuple(b)]) for b in bad[:5]]} " \
           f"ref {[int(ref[tuple(b)]) for b in bad[:5]]}"


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"{c[0]}x{c[1]}_m{c[2]}_D{c[3]}_w{c[4]}_c{c[5]}")
def test_bm_match_is_bit_exact(engine, synth, pkg, c):
    bm, left, right, ref = case(synth, c)
    setup(engine, pkg, bm)
    got = engine.match(left, right)
    if c in CASES[:3]:                      # non-vacuity: most of the core must be valid disparities
        share = br.valid_share(bm, ref)
        print("valid share", share)
        assert share >= 0.5
    assert np.array_equal(got, ref), diff_msg(got, ref)


@pytest.mark.parametrize("c", [(20, 600, 0, 528, 5, 31, 10, 15, 9), (20, 1100, -3, 1040, 5, 63, 0, 5, 10),
                               (30, 1100, 0, 1040, 23, 63, 10, 0, 11)], ids=["D528", "D1040", "D1040_u32"])
def test_bm_wide_searches(engine, synth, pkg, c):
    """D > 512 and D > 1024: 16 and 32 disparity chunks per lane (the latter in 8-wave workgroups)."""
    bm, left, right, ref = case(synth, c)
    setup(engine, pkg, bm)
    got = engine.match(left, right)
    assert (ref != br.filtered(bm)).any()
    assert np.array_equal(got, ref), diff_msg(got, ref)


@pytest.mark.parametrize("c", [CASES[1], CASES[5]], ids=["u16", "u32"])
def test_bm_column_sums_in_hbm(engine, synth, pkg, monkeypatch, c):
    """SGM_BM_VGLOBAL=1: the path taken when D x window does not fit the LDS budget (the column
    sums then live in the workspace), at both accumulator widths."""
    monkeypatch.setenv("SGM_BM_VGLOBAL", "1")
    bm, left, right, ref = case(synth, c)
    setup(engine, pkg, bm)
    got = engine.match(left, right)
    assert np.array_equal(got, ref), diff_msg(got, ref)


def test_bm_empty_column_range_is_all_filtered(engine, synth, pkg):
    left, right, _ = synth.stereo_pair(30, 40, 0, 16, seed=6)
    bm = br.BM(0, 48, 5, 31, 10, 15)                    # X0 = 47 >= W: nothing computed, status OK
    setup(engine, pkg, bm)
    got = engine.match(left, right)
    assert (got == -16).all() and np.array_equal(got, br.compute(bm, left, right))


def test_bm_single_column(engine, synth, pkg):
    left, right, _ = synth.stereo_pair(24, 64, 0, 64, seed=7)
    bm = br.BM(0, 64, 5, 31, 0, 0)                      # X0 = 63, X1 = 64
    assert br.column_range(bm, 64) == (63, 64)
    setup(engine, pkg, bm)
    got = engine.match(left, right)
    ref = br.compute(bm, left, right)
    assert (ref[2:22, 63] != -16).all()
    assert np.array_equal(got, ref), diff_msg(got, ref)


@pytest.mark.parametrize("H", [48, 41])
def test_bm_prefilter_stage(engine, synth, pkg, H):
    left, _, _ = synth.stereo_pair(H, 96, 0, 32, seed=8)
    for cap in (31, 7):
        setup(engine, pkg, br.BM(0, 32, 9, cap, 10, 15))
        assert np.array_equal(engine.bm_prefilter(left), br.prefilter(left, cap))


def test_bm_sad_stage(engine, synth, pkg):
    bm, left, right, _ = case(synth, CASES[0])
    setup(engine, pkg, bm)
    sad, tex = engine.bm_sad(left, right)
    _, rsad, rtex = br.compute(bm, left, right, return_stages=True)
    w2 = bm.w // 2
    assert sad.shape == (48, 96 - 31, 32)
    assert np.array_equal(sad[w2:48 - w2], rsad) and np.array_equal(tex[w2:48 - w2], rtex)
    assert not sad[:w2].any() and not sad[48 - w2:].any()


def test_bm_speckles_use_unscaled_range(engine, oracle, synth, pkg):
    bm, left, right, ref = case(synth, CASES[1])
    setup(engine, pkg, bm, speckle_window_size=100, speckle_range=4)
    got = engine.match(left, right)
    exp = oracle.filter_speckles(ref, br.filtered(bm), 100, 4)       # max_diff = 4, not 64
    assert (exp != ref).any()                                         # the filter removes something
    assert np.array_equal(got, exp), diff_msg(got, exp)


def test_bm_strided_buffers(engine, synth, pkg):
    bm, left, right, ref = case(synth, CASES[0])
    setup(engine, pkg, bm)
    H, W = left.shape
    L = np.full((H, W + 13), 255, np.uint8)
    R = np.full((H, W + 13), 255, np.uint8)
    L[:, :W], R[:, :W] = left, right
    out = np.full((H, W + 7), 12345, np.int16)
    vp = ctypes.c_void_p
    rc = engine.lib.sgm_match(engine.h, vp(L.ctypes.data), vp(R.ctypes.data), W, H, W + 13, vp(out.ctypes.data), W + 7)
    assert rc == 0, engine.error()
    assert np.array_equal(out[:, :W], ref) and (out[:, W:] == 12345).all()


def test_bm_match_f32(engine, synth, pkg):
    bm, left, right, ref = case(synth, CASES[2])
    setup(engine, pkg, bm)
    got = engine.match_f32(left, right)
    assert got.dtype == np.float32 and np.array_equal(got, ref.astype(np.float32))


def test_bm_device_batch(engine, synth, pkg):
    torch = pytest.importorskip("torch")
    H, W, m, D, w, cap, t, u, _ = CASES[1]
    bm = br.BM(m, D, w, cap, t, u)
    setup(engine, pkg, bm)
    frames = [synth.stereo_pair(H, W, m, D, seed=40 + i)[:2] for i in range(3)]
    singles = [engine.match(l, r) for l, r in frames]
    assert np.array_equal(singles[0], br.compute(bm, *frames[0]))
    dl = [torch.from_numpy(f[0]).cuda() for f in frames]
    dr = [torch.from_numpy(f[1]).cuda() for f in frames]
    out = torch.full((3, H, W), 777, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    engine.match_device_batch([x.data_ptr() for x in dl], [x.data_ptr() for x in dr], W, H, W,
                              [out[i].data_ptr() for i in range(3)], W, stream.cuda_stream)
    stream.synchronize()
    got = out.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], singles[i]), f"frame {i}: " + diff_msg(got[i], singles[i])


def test_bm_matcher_node_defaults(synth, pkg, oracle):
    """MatcherHIPSGM(mode=MODE_OCV_BM) driven by updateMatcher(NODE_DEFAULTS): the node's default
    path (block 15, minD 9, D 64, texture 10, speckles 100 / 4; disp12MaxDiff is not forwarded)."""
    left, right, _ = synth.stereo_pair(64, 128, 9, 64, seed=1)
    m = pkg.MatcherHIPSGM(" ", (128, 64), mode=pkg.MODE_OCV_BM)
    pkg.update_matcher(m, pkg.NODE_DEFAULTS)
    m.setImages(left, right)
    assert m.forwardMatch() == 0
    bm = br.BM(9, 64, 15, 31, 10, 15)
    exp = oracle.filter_speckles(br.compute(bm, left, right), br.filtered(bm), 100, 4)
    assert np.array_equal(m.getDisparity(), exp.astype(np.float32))
    m.setWindowSize(14)                                 # even window: cv::Exception -> -1
    assert m.forwardMatch() == -1
    # the right matcher: minD' = -(minD + D) + 1, texture 0, uniqueness 0, no speckles
    m.setWindowSize(15)
    assert m.backwardMatch() == 0
    rbm = br.BM(-(9 + 64) + 1, 64, 15, 31, 0, 0)
    assert np.array_equal(m.getBackDisparity(), br.compute(rbm, right, left))


def test_bm_fuzz(engine, pkg):
    """60 seeded random valid configurations; the frames are noise pairs with a random shift."""
    rng = np.random.default_rng(20240)
    for it in range(60):
        w = int(rng.choice(np.arange(5, 27, 2)))
        H = int(rng.integers(w + 1, 65))
        D = int(rng.choice([16, 32, 48, 64, 80, 96, 112, 128]))
        W = int(rng.integers(max(w + 1, 24), 193))
        m = int(rng.integers(-48, 33))
        bm = br.BM(m, D, w, int(rng.integers(1, 64)), int(rng.choice([0, 10, 200])), int(rng.choice([0, 5, 15])))
        left = rng.integers(0, 256, (H, W), dtype=np.uint8)
        left = ((left.astype(np.int32) + np.roll(left, 1, 1) + np.roll(left, 1, 0) + 1) // 3).astype(np.uint8)
        right = np.roll(left, -int(rng.integers(0, 9)), 1)
        right = np.where(rng.random((H, W)) < 0.05, rng.integers(0, 256, (H, W)), right).astype(np.uint8)
        setup(engine, pkg, bm)
        got = engine.match(left, right)
        ref = br.compute(bm, left, right)
        assert np.array_equal(got, ref), f"iteration {it} {bm} {H}x{W}: " + diff_msg(got, ref)


def test_bm_plugin_driver():
    """plugin/plugin_bm_test.cpp: MatcherCore in BM mode, forward and backward, against values the
    reference printed for one 48x96 frame (the frame is regenerated in C++, see the driver)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "i3dr_stereo_camera-ros_amd", "lib", "plugin_bm_test")
    r = subprocess.run([exe, "match"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
