"""GPU parity of the hole-filling post filter on raw frames and through the node-level mirrors.

1. sgm_match_device_batch_rect (and sgm_match_device with rectification set) in the census, SGBM, HH
   and BM modes, mono and colour, filter on and off: bit-exact against rectify -> the mode's unfilled
   CPU reference (tests/rect_modes_reference.py) -> tests/fill_reference.py on the mode's rectangle;
   the rectified images stay what they were.
2. The Python image_cb (one match_device_batch_rect call) with the filter on.
3. SGM_HIP_FILL_WHEN=interp end to end: image_cb_host, image_cb and the matcher's match() return the
   forward image filled, with the rectified images on their own sides.
4. A single census frame after a pipelined batch of the same geometry (filter off): the path work
   list is uploaded again after the batch has carved the workspace differently.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_reference as cr  # noqa: E402
import fill_reference as fr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402
from conftest import to_oracle_params  # noqa: E402
from test_gpu_rect_modes import _batch, _dev  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

pytestmark = pytest.mark.gpu

# a raised uniqueness ratio, so that the windows of rect_modes_reference's frames really have holes
# (CPU, first frame: 203x70 49 % census, 21-23 % SGBM / HH, 30-31 % BM; 130x41 13 % census, 13-14 % BM)
UNIQ = {"census": 40, "sgbm5": 40, "hh8": 40, "bm": 25}


def diff_msg(got, ref):
    bad = np.argwhere(np.asarray(got) != np.asarray(ref))
    if not len(bad):
        return "equal"
    y, x = bad[0][:2]
    return f"{len(bad)} pixels differ, first at (y {y}, x {x}): got {got[y, x]}, want {ref[y, x]}"


def window_holes(ref, rect, invalid):
    x0, y0, x1, y1 = rect
    return float((ref[y0:y1, x0:x1] == invalid).mean())


def case_kw(name, mode):
    return dict(rm.case_kw(name, mode), uniqueness_ratio=UNIQ[mode])


def unfilled(oracle, synth, name, mode, paths, ch, s, i):
    """Disparity of frame i of a rect_modes_reference case at the raised uniqueness, computed once."""
    def make():
        import census_paths_reference as cpr
        rect = rm.setup(oracle, synth, name, ch)[2]
        gl = np.ascontiguousarray(rm.grey_of(rect[i][0], s))
        gr = np.ascontiguousarray(rm.grey_of(rect[i][1], s))
        kw = case_kw(name, mode)
        if mode == "census" and paths == 4:
            return cpr.match_paths(oracle, oracle.make_params(rm.MODE_ID[mode], **kw), gl, gr)
        return rm.match_ref(oracle, mode, kw, gl, gr)
    return rm.once(("fill ref", name, mode, paths, ch, s if ch == 3 else 0, i), make)


@pytest.fixture
def eng(engine, pkg):
    """The shared engine; fill off and 8 paths again afterwards."""
    try:
        yield engine
    finally:
        engine.set_fill_params(pkg.default_fill_params())
        engine.set_census_paths(8)


# ------------------------------------------------------------------ 1. raw frames, device entries
@pytest.mark.parametrize("mode,paths,name,ch,n,single", [
    ("census", 8, "203x70", 1, 3, False), ("census", 8, "203x70", 3, 2, False), ("census", 4, "203x70", 1, 2, False),
    ("census", 8, "130x41", 1, 5, False), ("census", 8, "130x41", 3, 1, False),
    ("sgbm5", 8, "203x70", 1, 2, False), ("sgbm5", 8, "203x70", 3, 5, False),
    ("hh8", 8, "203x70", 3, 2, False), ("hh8", 8, "203x70", 1, 1, True),
    ("bm", 8, "203x70", 1, 5, False), ("bm", 8, "203x70", 3, 2, False), ("bm", 8, "130x41", 1, 3, False),
    ("bm", 8, "203x70", 3, 1, True)])
def test_raw_frames_fill(eng, oracle, pkg, synth, mode, paths, name, ch, n, single):
    """n = 5 wraps the four OCV lanes and runs three pipelined census groups; every frame of a batch
    is another frame. The filter off gives the unfilled reference through the same call."""
    torch = pytest.importorskip("torch")
    rh, rw, h, w, m, D, _ = rm.CASES[name]
    s = cr.GRAY_Y15 if ch == 3 and mode != "census" else cr.GRAY_Y14
    maps, frames, rect = rm.setup(oracle, synth, name, ch)
    kw = case_kw(name, mode)
    eng.set_params(pkg.default_params(rm.MODE_ID[mode], **kw))
    eng.set_census_paths(paths)
    eng.set_bm_params(pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE))
    inv = (m - 1) * 16
    win = fr.match_rect(mode == "bm", m, D, kw.get("block_size", 0), w, h)
    refs = [unfilled(oracle, synth, name, mode, paths, ch, s, i) for i in range(n)]
    share = window_holes(refs[0], win, inv)
    print(mode, paths, name, ch, "window holes", share)
    assert share >= 0.05, "the input needs window holes, or a no-op passes"
    for fill in (pkg.default_fill_params(mode=fr.BACKGROUND), pkg.default_fill_params(),
                 pkg.default_fill_params(mode=fr.MEDIAN, max_gap=3, min_neighbours=3)):
        eng.set_fill_params(fill)
        got, gl, gr = _batch(torch, eng, maps, frames[:n], h, w, ch, s, single=single)
        for i in range(n):
            want = fr.fill_holes(refs[i], inv, fill.mode, fill.max_gap, fill.min_neighbours, win)
            assert np.array_equal(got[i], want), f"fill {fill.as_dict()} frame {i}: " + diff_msg(got[i], want)
            if fill.mode == fr.BACKGROUND:
                assert (want != refs[i]).mean() >= 0.02
            for g, side in ((gl, 0), (gr, 1)):
                if g is not None:
                    assert np.array_equal(g[i], rect[i][side]), f"frame {i} rectified {'LR'[side]}"


# ------------------------------------------------------------------------------------ 2. image_cb
H, W, D, MIND, F, T = 70, 300, 64, 3, 712.5, 0.119      # the frame of test_gpu_fill's node_frame cases
ZMIN, ZMAX = 0.05, 100.0


def _matcher(pkg, mode):
    kw = dict(min_disparity=MIND, num_disparities=D, uniqueness_ratio=60) if mode == "census" else \
        dict(rm.mode_kw(mode, MIND, D), uniqueness_ratio=UNIQ[mode])
    m = pkg.MatcherHIPSGM(" ", (W, H), mode=rm.MODE_ID[mode], census_paths=8)
    m.params = pkg.default_params(rm.MODE_ID[mode], **kw)
    m.bm_params = pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE)
    return m


def _wanted(pkg, m, mode, plain, fmode, G, N):
    """The windowed DisparityImage image of the unfilled, unwindowed one `plain` filled on the CPU,
    and the int16 image in between."""
    d16 = np.round(plain * 16).astype(np.int16)
    assert np.array_equal(d16.astype(np.float32) * np.float32(1 / 16), plain)
    inv = (MIND - 1) * 16
    win = fr.match_rect(mode == "bm", MIND, D, m.params.block_size, W, H)
    assert window_holes(d16, win, inv) >= 0.05
    want16 = fr.fill_holes(d16, inv, fmode, G, N, win)
    assert (want16 != d16).mean() >= 0.02
    lo, hi = np.float32(T * F / ZMAX), np.float32(T * F / ZMIN)
    want = want16.astype(np.float32) * np.float32(1 / 16)
    want[(want < lo) | (want > hi)] = pkg.MISSING_Z
    return want, want16


@pytest.mark.parametrize("mode,ch", [("census", 1), ("census", 3), ("sgbm5", 3), ("bm", 1)])
def test_image_cb_fills(pkg, synth, mode, ch):
    """image_cb with the filter on: the rectified images of the unfilled call, and its image (read
    through an unbounded window, where the float image is d / 16 exactly) filled by the numpy filter
    and packed again; image_cb_host gives the same three."""
    pytest.importorskip("torch")
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    raw = rm.raw_frames(synth, H, W, MIND, D, D + 5, ch)
    m = _matcher(pkg, mode)
    try:
        state = {}
        plain = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, 0.0, np.inf, state)   # window [0, inf]
        assert plain is not None and not np.array_equal(plain[0], raw[0])
        want, _ = _wanted(pkg, m, mode, plain[2]["image"], fr.MEDIAN, 16, 2)
        m.setHoleFilling(fr.MEDIAN, 16, 2)
        got = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, ZMIN, ZMAX, state)
        assert np.array_equal(got[2]["image"], want), "image_cb: " + diff_msg(got[2]["image"], want)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        assert state["map_builds"] == 1
        host = pkg.image_cb_host(m, raw[0], raw[1], infos[0], infos[1], F, T, ZMIN, ZMAX)
        for a, b in zip(host[:2], got[:2]):
            assert np.array_equal(a, b)
        assert np.array_equal(host[2]["image"], want)
        m.setHoleFilling(fr.OFF)
        off = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, 0.0, np.inf, state)
        assert np.array_equal(off[2]["image"], plain[2]["image"])
    finally:
        if m._engine is not None:
            m._engine.close()


# ---------------------------------------------------------------- 3. SGM_HIP_FILL_WHEN=interp
@pytest.mark.parametrize("mode,ch,env_fill", [("census", 1, None), ("sgbm5", 3, "median:5:3")])
def test_interp_drives_the_filter(pkg, synth, monkeypatch, mode, ch, env_fill):
    """With SGM_HIP_FILL_WHEN=interp, interp on is the forward match filled (background 16 2 when
    SGM_HIP_FILL names no filter) on (left, right) with the rectified images not swapped, not Q3's
    right-view image; interp off is the forward match unfilled."""
    pytest.importorskip("torch")
    monkeypatch.setenv("SGM_HIP_FILL_WHEN", "interp")
    if env_fill is None:
        monkeypatch.delenv("SGM_HIP_FILL", raising=False)
    else:
        monkeypatch.setenv("SGM_HIP_FILL", env_fill)
    fmode, G, N = (fr.BACKGROUND, 16, 2) if env_fill is None else (fr.MEDIAN, 5, 3)
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    raw = rm.raw_frames(synth, H, W, MIND, D, D + 5, ch)
    m = _matcher(pkg, mode)
    assert m.fill_when == "interp"
    try:
        m.setInterpolation(False)
        plain = pkg.image_cb_host(m, raw[0], raw[1], infos[0], infos[1], F, T, 0.0, np.inf)
        assert plain is not None and not np.array_equal(plain[0], plain[1])
        want, want16 = _wanted(pkg, m, mode, plain[2]["image"], fmode, G, N)
        d16 = np.round(plain[2]["image"] * 16).astype(np.int16)
        m.setInterpolation(True)
        for name, cb in (("image_cb_host", pkg.image_cb_host), ("image_cb", pkg.image_cb)):
            got = cb(m, raw[0], raw[1], infos[0], infos[1], F, T, ZMIN, ZMAX)
            assert np.array_equal(got[2]["image"], want), name + ": " + diff_msg(got[2]["image"], want)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), name + ": rectified sides"
        # the matcher itself, on the rectified pair: forwardMatch, no backward match
        assert np.array_equal(pkg.stereo_match(m, plain[0], plain[1]), want16.astype(np.float32))
        assert m.getBackDisparity() is None
        m.setInterpolation(False)
        assert np.array_equal(pkg.stereo_match(m, plain[0], plain[1]), d16.astype(np.float32))
        off = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, 0.0, np.inf)
        assert np.array_equal(off[2]["image"], plain[2]["image"])
    finally:
        if m._engine is not None:
            m._engine.close()


# ------------------------------------------- 4. a single census frame after a pipelined batch
@pytest.mark.parametrize("paths", [8, 4])
def test_single_frame_after_a_pipelined_batch(oracle, pkg, synth, paths):
    """Census, filter off, one handle of its own: batch (the workspace grows to the batch's size),
    single frame (uploads its path work list into that workspace), batches of the same geometry
    (their volume sets cover the list), single frame again and a device single frame: each equals
    the reference."""
    torch = pytest.importorskip("torch")
    import census_paths_reference as cpr
    h, w, minD, nD = 70, 300, 3, 64
    left, right, _ = synth.stereo_pair(h, w, minD, nD, seed=nD + 5)
    p = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=minD, num_disparities=nD, uniqueness_ratio=15)
    op = to_oracle_params(oracle, p)
    ref = oracle.match(op, left, right) if paths == 8 else cpr.match_paths(oracle, op, left, right)
    assert (ref != (minD - 1) * 16).mean() > 0.3
    dl, dr = _dev(torch, left), _dev(torch, right)
    eng = pkg.Engine(0)
    try:
        eng.set_params(p)
        eng.set_census_paths(paths)

        def batch(n):
            out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            eng.match_device_batch([dl.data_ptr()] * n, [dr.data_ptr()] * n, w, h, w,
                                   [out[i].data_ptr() for i in range(n)], w)
            eng.synchronize()
            got = out.cpu().numpy()
            for i in range(n):
                assert np.array_equal(got[i], ref), f"batch of {n}, frame {i}: " + diff_msg(got[i], ref)

        batch(3)
        assert np.array_equal(eng.match(left, right), ref), "single frame after the first batch"
        batch(3)
        got = eng.match(left, right)
        assert np.array_equal(got, ref), "single frame after a pipelined batch: " + diff_msg(got, ref)
        batch(5)
        out = torch.full((h, w), 777, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.match_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w)
        eng.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref), "device single frame after a pipelined batch"
        batch(2)
        assert np.array_equal(eng.match(left, right), ref)
    finally:
        eng.close()
