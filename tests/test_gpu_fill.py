"""GPU parity of the hole-filling post filter (sgm_set_fill_params, sgm_fill_holes, stage `fill`).

Part 1: Engine.fill (sgm_debug_fill -> sgm_fill_holes -> k_fill) against tests/fill_reference.py, bit
for bit, over shapes smaller than the gap, widths that cut waves and the kernel's column blocks,
heights that cut its row bands, every gap class of the launcher (256 / 512 / 1024 threads) and both
selection rules.
Part 2: end to end. Every mode and every entry point that honours the filter equals the unfilled
reference of the mode (the CPU oracle, tests/bm_reference.py, tests/census_paths_reference.py)
followed by the numpy filter on the mode's rectangle; with the filter off every output equals the
unfilled reference; the two overlap tile modes refuse.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_paths_reference as cpr  # noqa: E402
import fill_reference as fr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402
from conftest import to_oracle_params  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (7, 1), (33, 65), (70, 300), (130, 520)]
GAPS = [1, 2, 3, 16, 63, 64, 65, 255]
NEIGHBOURS = [1, 2, 4, 8]
PATTERNS = ["salt10", "salt50", "salt95", "blocky", "all_invalid", "no_hole", "inner_rect"]
INVALID = -16


def diff_msg(got, ref):
    bad = np.argwhere(np.asarray(got) != np.asarray(ref))
    if not len(bad):
        return "equal"
    y, x = bad[0][:2]
    return f"{len(bad)} pixels differ, first at (y {y}, x {x}): got {got[y, x]}, want {ref[y, x]}"


def pattern(name, h, w, G, rng):
    """(image, rectangle) of an input pattern: values 0..4000 with holes = INVALID."""
    img = rng.integers(0, 4000, (h, w)).astype(np.int16)
    rect = (0, 0, w, h)
    if name.startswith("salt"):
        img[rng.random((h, w)) < int(name[4:]) / 100.0] = INVALID
    elif name == "blocky":              # holes wider and taller than the gap (where the image allows)
        for _ in range(6):
            bh, bw = min(h, G + 1 + int(rng.integers(0, 9))), min(w, G + 1 + int(rng.integers(0, 9)))
            y, x = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
            img[y:y + bh, x:x + bw] = INVALID
    elif name == "all_invalid":
        img[...] = INVALID
    elif name == "inner_rect":          # strictly inside wherever the image has an inside
        img[rng.random((h, w)) < 0.5] = INVALID
        x0, x1 = (1 + w // 5, w - 1 - w // 7) if w >= 3 else (0, w)
        y0, y1 = (1 + h // 6, h - 1 - h // 9) if h >= 3 else (0, h)
        rect = (x0, y0, x1, y1)
    return img, rect


def fill_params(pkg, mode, G, N):
    return pkg.default_fill_params(mode=mode, max_gap=G, min_neighbours=N)


# ---------------------------------------------------------------------------- 1. the filter alone
@pytest.mark.parametrize("h,w", SHAPES)
def test_fill_against_reference(engine, pkg, h, w):
    rng = np.random.default_rng(1000 * h + w)
    n_filled = 0
    for name in PATTERNS:
        for G in GAPS:
            img, rect = pattern(name, h, w, G, rng)
            cands = fr.candidates(img, INVALID, G)
            for N in NEIGHBOURS:
                for mode in (fr.BACKGROUND, fr.MEDIAN):
                    ref = fr.fill_holes(img, INVALID, mode, G, N, rect, cands=cands)
                    got = engine.fill(img, INVALID, fill_params(pkg, mode, G, N), rect)
                    assert np.array_equal(got, ref), f"{name} {h}x{w} G {G} N {N} mode {mode} rect {rect}: " + \
                        diff_msg(got, ref)
                    n_filled += int((ref != img).sum())
    if h * w > 9:
        assert n_filled > 0, "no pattern filled a pixel"


def test_fill_known_answers_and_off(engine, pkg):
    kat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fill", "fill_kat.npz"))
    for case in fr.KAT_CASES:
        inv, mode, G, N, x0, y0, x1, y1 = (int(v) for v in kat[case + "_par"])
        got = engine.fill(fr.kat_input(kat, case), inv, fill_params(pkg, mode, G, N), (x0, y0, x1, y1))
        assert np.array_equal(got, kat[case + "_out"]), case + ": " + diff_msg(got, kat[case + "_out"])
    img, _ = pattern("salt50", 40, 70, 4, np.random.default_rng(5))
    assert np.array_equal(engine.fill(img, INVALID, fill_params(pkg, fr.OFF, 0, 0)), img)      # OFF: nothing is checked
    assert np.array_equal(engine.fill(img, INVALID, fill_params(pkg, fr.MEDIAN, 4, 1), (9, 9, 9, 30)), img)   # empty


def test_fill_holes_device_entry(engine, pkg):
    """Padded strides on both sides, a caller's stream, another invalid value; d_dst == d_src and bad
    rectangles are SGM_ERR_ARG, bad parameters SGM_ERR_PARAM, and nothing is written then."""
    torch = pytest.importorskip("torch")
    h, w, G, inv = 57, 301, 7, 128
    rng = np.random.default_rng(77)
    img = rng.integers(-300, 300, (h, w)).astype(np.int16)
    img[rng.random((h, w)) < 0.4] = inv
    rect = (5, 3, 290, 50)
    src = torch.full((h, w + 7), 555, dtype=torch.int16, device="cuda")
    src[:, :w] = torch.from_numpy(img).cuda()
    dst = torch.full((h, w + 3), 999, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    par = fill_params(pkg, fr.MEDIAN, G, 3)
    engine.fill_holes(src.data_ptr(), w + 7, w, h, inv, par, rect, dst.data_ptr(), w + 3, stream.cuda_stream)
    stream.synchronize()
    got = dst.cpu().numpy()
    ref = fr.fill_holes(img, inv, fr.MEDIAN, G, 3, rect)
    assert np.array_equal(got[:, :w], ref), diff_msg(got[:, :w], ref)
    assert (got[:, w:] == 999).all() and (ref != img).sum() > 100
    dst[...] = 999
    torch.cuda.synchronize()
    bad = [(dict(d=src.data_ptr()), pkg.SGM_ERR_ARG), (dict(rect=(5, 3, w + 1, 50)), pkg.SGM_ERR_ARG),
           (dict(rect=(6, 3, 5, 50)), pkg.SGM_ERR_ARG), (dict(rect=(0, -1, 5, 50)), pkg.SGM_ERR_ARG),
           (dict(par=fill_params(pkg, fr.MEDIAN, 0, 3)), pkg.SGM_ERR_PARAM),
           (dict(par=fill_params(pkg, fr.MEDIAN, 256, 3)), pkg.SGM_ERR_PARAM),
           (dict(par=fill_params(pkg, fr.BACKGROUND, 4, 0)), pkg.SGM_ERR_PARAM),
           (dict(par=fill_params(pkg, fr.BACKGROUND, 4, 9)), pkg.SGM_ERR_PARAM),
           (dict(par=fill_params(pkg, 3, 4, 2)), pkg.SGM_ERR_PARAM)]
    for kw, code in bad:
        with pytest.raises(pkg.SGMError) as e:
            engine.fill_holes(src.data_ptr(), w + 7, w, h, inv, kw.get("par", par), kw.get("rect", rect),
                              kw.get("d", dst.data_ptr()), w + 3)
        assert e.value.code == code, kw
    engine.synchronize()
    assert (dst.cpu().numpy() == 999).all() and np.array_equal(src.cpu().numpy()[:, :w], img)


# --------------------------------------------------------------------------------- 2. end to end
# Frames whose window really has holes (census, synth.stereo_pair(seed = D + 5)); the OpenCV and BM
# modes run frame A with a raised uniqueness ratio.
FRAMES = {
    "A": dict(h=48, w=96, kw=dict(min_disparity=0, num_disparities=32, uniqueness_ratio=40)),
    "B": dict(h=70, w=300, kw=dict(min_disparity=3, num_disparities=64, uniqueness_ratio=60)),
    "C": dict(h=120, w=330, kw=dict(min_disparity=-5, num_disparities=128, uniqueness_ratio=40, median=1,
                                     speckle_window_size=40, speckle_range=1)),
}
MODE_CASES = [("census", 8, "A"), ("census", 8, "B"), ("census", 8, "C"), ("census", 4, "A"), ("census", 4, "B"),
              ("sgbm5", 8, "A"), ("hh8", 8, "A"), ("bm", 8, "A")]
_cache = {}


def case(oracle, synth, pkg, mode, paths, frame):
    """(params, bm params, left, right, unfilled reference, rectangle) of a mode case, computed once."""
    key = (mode, paths, frame)
    if key not in _cache:
        f = FRAMES[frame]
        D, minD = f["kw"]["num_disparities"], f["kw"]["min_disparity"]
        left, right, _ = synth.stereo_pair(f["h"], f["w"], max(minD, 0), D, seed=D + 5)
        if mode == "census":
            p = pkg.default_params(pkg.MODE_CENSUS8, **f["kw"])
            op = to_oracle_params(oracle, p)
            ref = oracle.match(op, left, right) if paths == 8 else cpr.match_paths(oracle, op, left, right)
        else:
            kw = dict(rm.mode_kw(mode, minD, D), uniqueness_ratio=40 if mode != "bm" else 25)
            p = pkg.default_params(rm.MODE_ID[mode], **kw)
            ref = rm.match_ref(oracle, mode, kw, left, right)
        rect = fr.match_rect(mode == "bm", minD, D, p.block_size, f["w"], f["h"])
        for a in (left, right, ref):
            a.setflags(write=False)
        _cache[key] = (p, pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE), left, right, ref, rect)
    return _cache[key]


def window_holes(ref, rect, invalid):
    x0, y0, x1, y1 = rect
    return float((ref[y0:y1, x0:x1] == invalid).mean())


@pytest.fixture
def eng(engine, pkg):
    """The shared engine; fill off, 8 paths, mono, no profiling again afterwards."""
    try:
        yield engine
    finally:
        engine.set_fill_params(pkg.default_fill_params())
        engine.set_census_paths(8)
        engine.set_profiling(False)


def setup(eng, pkg, p, bm, paths, fill):
    eng.set_params(p)
    eng.set_bm_params(bm)
    eng.set_census_paths(paths)
    eng.set_fill_params(fill)


@pytest.mark.parametrize("mode,paths,frame", MODE_CASES)
def test_match_every_mode(eng, oracle, synth, pkg, mode, paths, frame):
    p, bm, left, right, ref, rect = case(oracle, synth, pkg, mode, paths, frame)
    inv = (p.min_disparity - 1) * 16
    share = window_holes(ref, rect, inv)
    print(mode, paths, frame, "window holes", share)
    assert share >= 0.05, "the input needs window holes, or a no-op passes"
    setup(eng, pkg, p, bm, paths, pkg.default_fill_params())
    got = eng.match(left, right)
    assert np.array_equal(got, ref), "fill off: " + diff_msg(got, ref)
    outs = {}
    for fmode, G, N in [(fr.BACKGROUND, 16, 2), (fr.MEDIAN, 16, 2), (fr.BACKGROUND, 2, 2), (fr.MEDIAN, 3, 5)]:
        want = fr.fill_holes(ref, inv, fmode, G, N, rect)
        setup(eng, pkg, p, bm, paths, fill_params(pkg, fmode, G, N))
        got = eng.match(left, right)
        assert np.array_equal(got, want), f"fill {fmode} G {G} N {N}: " + diff_msg(got, want)
        outs[(fmode, G)] = want
        x0, y0, x1, y1 = rect
        outside = np.ones(ref.shape, bool)
        outside[y0:y1, x0:x1] = False
        assert np.array_equal(want[outside], ref[outside])
    assert (outs[(fr.BACKGROUND, 16)] != ref).mean() >= 0.02
    assert not np.array_equal(outs[(fr.BACKGROUND, 16)], outs[(fr.MEDIAN, 16)])


def test_window_fill_shares(oracle, synth, pkg):
    """The figures the issue gives for its three census frames, from the CPU references alone (they
    say that the GPU cases above have something to fill): 27, 34 and 13 % window holes; at G = 16
    every window fills completely; at G = 2 frame B keeps 15 % invalid; over the three frames and
    G = 16 and 2 the two selection rules differ in 1.6 to 24 % of the frame's pixels."""
    differ = []
    for frame, holes in (("A", 27), ("B", 34), ("C", 13)):
        p, _, _, _, ref, rect = case(oracle, synth, pkg, "census", 8, frame)
        inv = (p.min_disparity - 1) * 16
        assert round(100 * window_holes(ref, rect, inv)) == holes, frame
        for G in (16, 2):
            bg, med = (fr.fill_holes(ref, inv, m, G, 2, rect) for m in (fr.BACKGROUND, fr.MEDIAN))
            differ.append(float((bg != med).mean()))
            if G == 16:
                assert window_holes(bg, rect, inv) == 0.0 and window_holes(med, rect, inv) == 0.0, frame
            elif frame == "B":
                assert round(100 * window_holes(bg, rect, inv)) == 15
    print("the two rules differ in", differ)
    assert round(1000 * min(differ)) == 16 and round(100 * max(differ)) == 24, differ


def _device_batch(torch, eng, frames, h, w, pad_in=0, pad_out=0):
    n = len(frames)
    dl = torch.zeros((n, h, w + pad_in), dtype=torch.uint8, device="cuda")
    dr = torch.zeros((n, h, w + pad_in), dtype=torch.uint8, device="cuda")
    for i, f in enumerate(frames):
        dl[i, :, :w] = torch.from_numpy(np.array(f[0])).cuda()
        dr[i, :, :w] = torch.from_numpy(np.array(f[1])).cuda()
    out = torch.full((n, h, w + pad_out), 777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.match_device_batch([dl[i].data_ptr() for i in range(n)], [dr[i].data_ptr() for i in range(n)], w, h,
                           w + pad_in, [out[i].data_ptr() for i in range(n)], w + pad_out)
    eng.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :, w:] == 777).all()
    return got[:, :, :w]


@pytest.mark.parametrize("mode,paths,frame", [("census", 8, "B"), ("census", 8, "C"), ("census", 4, "B"), ("sgbm5", 8, "A"),
                                              ("bm", 8, "A")])
def test_entry_points(eng, oracle, synth, pkg, mode, paths, frame):
    """match, match_f32 (plain and into a registered buffer: no WTA-written rows while the filter is
    on), match_device with padded strides, device batches of 1, 2, 3 and 5 frames, match_batch."""
    torch = pytest.importorskip("torch")
    p, bm, left, right, ref, rect = case(oracle, synth, pkg, mode, paths, frame)
    h, w = ref.shape
    inv = (p.min_disparity - 1) * 16
    fp = fill_params(pkg, fr.BACKGROUND, 16, 2)
    want = fr.fill_holes(ref, inv, fr.BACKGROUND, 16, 2, rect)
    assert (want != ref).mean() >= 0.02
    for fill, exp in ((fp, want), (pkg.default_fill_params(), ref)):
        setup(eng, pkg, p, bm, paths, fill)
        assert np.array_equal(eng.match(left, right), exp)
        assert np.array_equal(eng.match_f32(left, right), exp.astype(np.float32))
        buf = np.full((h, w + 5), -7, np.float32)
        eng.host_register(buf)
        try:
            eng.match_f32(left, right, out=buf[:, :w])
            assert np.array_equal(buf[:, :w], exp.astype(np.float32)), "match_f32 registered"
            assert (buf[:, w:] == -7).all()
        finally:
            eng.host_unregister(buf)
        for n in (1, 2, 3, 5):
            got = _device_batch(torch, eng, [(left, right)] * n, h, w, pad_in=3, pad_out=5)
            for i in range(n):
                assert np.array_equal(got[i], exp), f"device batch {n}, frame {i}: " + diff_msg(got[i], exp)
        dl, dr = torch.from_numpy(np.array(left)).cuda(), torch.from_numpy(np.array(right)).cuda()
        out = torch.full((h, w + 3), 1234, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.match_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w + 3)
        eng.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :w], exp) and (got[:, w:] == 1234).all(), "match_device"
        outs = eng.match_batch([left] * 3, [right] * 3, devices=[0, 0])
        for i in range(3):
            assert np.array_equal(outs[i], exp), f"match_batch frame {i}"


def test_stage_and_bytes(eng, oracle, synth, pkg):
    """`fill` is the last stage, 4 B/px, and is absent with the filter off."""
    p, bm, left, right, ref, rect = case(oracle, synth, pkg, "census", 8, "C")
    h, w = ref.shape
    setup(eng, pkg, p, bm, 8, fill_params(pkg, fr.MEDIAN, 16, 2))
    eng.set_profiling(True)
    eng.match(left, right)
    st = eng.stage_times()
    eng.set_profiling(False)
    assert [s[0] for s in st][-2:] == ["median3+speckle", "fill"], st
    assert st[-1][2] == 4.0 * w * h
    setup(eng, pkg, p, bm, 8, pkg.default_fill_params())
    eng.set_profiling(True)
    eng.match(left, right)
    names = [s[0] for s in eng.stage_times()]
    eng.set_profiling(False)
    assert "fill" not in names and names[-1] == "median3+speckle"


def test_tiled_exact_fills_and_overlap_modes_refuse(eng, oracle, synth, pkg):
    torch = pytest.importorskip("torch")
    p, bm, left, right, ref, rect = case(oracle, synth, pkg, "census", 8, "C")
    h, w = ref.shape
    inv = (p.min_disparity - 1) * 16
    want = fr.fill_holes(ref, inv, fr.MEDIAN, 16, 2, rect)
    setup(eng, pkg, p, bm, 8, fill_params(pkg, fr.MEDIAN, 16, 2))
    got = eng.match_tiled_exact(left, right, 3)
    assert np.array_equal(got, want), diff_msg(got, want)
    with pytest.raises(pkg.SGMError) as e:
        eng.match_tiled(left, right, 3, 16)
    assert e.value.code == pkg.SGM_ERR_UNSUPPORTED and "fill" in eng.error()
    dl, dr = torch.from_numpy(np.array(left)).cuda(), torch.from_numpy(np.array(right)).cuda()
    out = torch.full((h, w), 1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(pkg.SGMError) as e:
        eng.match_tiled_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w, 3, 16, devices=[0])
    assert e.value.code == pkg.SGM_ERR_UNSUPPORTED
    assert (out.cpu().numpy() == 1234).all()
    # without a median the assembled frame goes straight in front of the fill
    q = p.copy(median=0, speckle_window_size=0)
    ref0 = oracle.match(to_oracle_params(oracle, q), left, right)
    eng.set_params(q)
    got = eng.match_tiled_exact(left, right, 2)
    want0 = fr.fill_holes(ref0, inv, fr.MEDIAN, 16, 2, rect)
    assert np.array_equal(got, want0), diff_msg(got, want0)
    eng.set_fill_params(pkg.default_fill_params())
    assert np.array_equal(eng.match_tiled_exact(left, right, 3), ref0)
    assert np.array_equal(eng.match_tiled(left, right, 1, 0), ref0)


def test_bad_values_fail_at_match_time(eng, oracle, synth, pkg):
    p, bm, left, right, ref, rect = case(oracle, synth, pkg, "census", 8, "A")
    for f in [fill_params(pkg, fr.MEDIAN, 0, 2), fill_params(pkg, fr.MEDIAN, 256, 2), fill_params(pkg, fr.MEDIAN, 16, 0),
              fill_params(pkg, fr.BACKGROUND, 16, 9), fill_params(pkg, 7, 16, 2)]:
        setup(eng, pkg, p, bm, 8, f)                           # setters store any value
        assert eng.get_fill_params().as_dict() == f.as_dict()
        for call in (lambda: eng.match(left, right), lambda: eng.match_tiled_exact(left, right, 2),
                     lambda: eng.match_batch([left], [right], devices=[0])):
            with pytest.raises(pkg.SGMError) as e:
                call()
            assert e.value.code == pkg.SGM_ERR_PARAM, f.as_dict()
    setup(eng, pkg, p, bm, 8, fill_params(pkg, fr.OFF, 0, 0))  # OFF: the other two are not looked at
    assert np.array_equal(eng.match(left, right), ref)


def test_frame_without_a_window_stays_invalid(eng, pkg):
    rng = np.random.default_rng(4)
    left = rng.integers(0, 256, (20, 30), dtype=np.uint8)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=32)
    setup(eng, pkg, p, pkg.default_bm_params(), 8, fill_params(pkg, fr.BACKGROUND, 16, 1))
    assert (eng.match(left, left) == -16).all()


@pytest.mark.parametrize("mode,ch", [("census", 1), ("census", 3), ("sgbm5", 3), ("bm", 1)])
def test_node_frame_and_image_cb_host(pkg, synth, mode, ch):
    """node_frame with the filter on: the DisparityImage equals the unfilled frame's int16 image (read
    back through an unbounded window, where the float image is d / 16 exactly) filled by the numpy
    filter and packed again, in a plain and in a registered buffer; the depth image equals
    disp_info_to_depth of that image; image_cb_host returns the same image."""
    pytest.importorskip("torch")
    h, w, D, minD, f, T = 70, 300, 64, 3, 712.5, 0.119
    infos = [calib(seed=11, w=w, h=h), calib(seed=12, w=w, h=h)]
    raw = rm.raw_frames(synth, h, w, minD, D, D + 5, ch)
    kw = dict(min_disparity=minD, num_disparities=D, uniqueness_ratio=60) if mode == "census" else \
        dict(rm.mode_kw(mode, minD, D), uniqueness_ratio=40 if mode != "bm" else 25)
    m = pkg.MatcherHIPSGM(" ", (w, h), mode=rm.MODE_ID[mode], census_paths=8)
    m.params = pkg.default_params(rm.MODE_ID[mode], **kw)
    m.bm_params = pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE)
    engine = m._engine_for()
    try:
        big = np.float32(3.0e38)
        assert pkg.image_cb_host(m, raw[0], raw[1], infos[0], infos[1], f, T, 0.05, 100.0) is not None   # sets the engine up
        plain = engine.node_frame(raw[0], raw[1], infos[0], infos[1], -big, big)
        d16 = np.round(plain[2] * 16).astype(np.int16)
        assert np.array_equal(d16.astype(np.float32) * np.float32(1 / 16), plain[2])
        inv = (minD - 1) * 16
        rect = fr.match_rect(mode == "bm", minD, D, m.params.block_size, w, h)
        assert window_holes(d16, rect, inv) >= 0.05
        want16 = fr.fill_holes(d16, inv, fr.BACKGROUND, 16, 2, rect)
        assert (want16 != d16).mean() >= 0.02
        lo, hi = np.float32(T * f / 100.0), np.float32(T * f / 0.05)
        want = want16.astype(np.float32) * np.float32(1 / 16)
        want[(want < lo) | (want > hi)] = pkg.MISSING_Z
        Q = pkg.calc_q(infos[0][0], infos[1][3], infos[0][3])
        want_depth = pkg.disp_info_to_depth(engine, want, None, Q, 0.05, 100.0, gen_point_cloud=False)[0]
        m.setHoleFilling(fr.BACKGROUND, 16, 2)
        got = pkg.image_cb_host(m, raw[0], raw[1], infos[0], infos[1], f, T, 0.05, 100.0)
        assert np.array_equal(got[2]["image"], want), "image_cb_host: " + diff_msg(got[2]["image"], want)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        for registered in (False, True):
            disp, depth = np.full((h, w), -1.0, np.float32), np.full((h, w), -2.0, np.float32)
            if registered:
                engine.host_register(disp)
            try:
                engine.node_frame(raw[0], raw[1], infos[0], infos[1], lo, hi, disparity=disp, depth=depth,
                                  q5=pkg.q_terms(Q), depth_min=0.05, depth_max=100.0)
            finally:
                if registered:
                    engine.host_unregister(disp)
            assert np.array_equal(disp, want), f"registered {registered}: " + diff_msg(disp, want)
            assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)), "depth"
        m.setHoleFilling(fr.OFF)
        got = pkg.image_cb_host(m, raw[0], raw[1], infos[0], infos[1], f, T, 0.0, 100.0)
        off = engine.node_frame(raw[0], raw[1], infos[0], infos[1], np.float32(T * f / 100.0), np.float32(np.inf))
        assert np.array_equal(got[2]["image"], off[2])
        assert np.array_equal(np.round(engine.node_frame(raw[0], raw[1], infos[0], infos[1], -big, big)[2] * 16), d16)
    finally:
        engine.close()
