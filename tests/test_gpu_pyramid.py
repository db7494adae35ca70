"""GPU parity of the half-resolution pyramid level (sgm_set_pyramid_params, stages `pyr_down` and
`pyr_refine`).

Part 1: Engine.pyr_down and Engine.pyr_refine against tests/pyramid_reference.py, bit for bit, over
shapes smaller than a census window, widths and heights that cut the kernels' 64 x 16 and 64 x 4
blocks, negative and positive minimum disparities, both radii, sub-pixel on and off, and coarse
images whose values run past both ends of the range (clipped and empty candidate sets, right-column
clamps).
Part 2: end to end. Level 1 through every entry point that honours it equals the composition
down -> the engine's own level-0 match of the coarse pair -> numpy refine (-> numpy fill); once
against the CPU oracle's coarse match; the refusals; level 0 untouched afterwards; the profile.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_paths_reference as cpr  # noqa: E402
import color_reference as cr  # noqa: E402
import fill_reference as fr  # noqa: E402
import pyramid_reference as pr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402
from conftest import to_oracle_params  # noqa: E402
from test_gpu_rect_modes import _batch  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_pyramid_test")
SHAPES = [(1, 1), (1, 9), (7, 1), (2, 2), (33, 65), (64, 256), (121, 333), (130, 520)]


def diff_msg(got, ref):
    bad = np.argwhere(np.asarray(got) != np.asarray(ref))
    if not len(bad):
        return "equal"
    y, x = bad[0][:2]
    return f"{len(bad)} pixels differ, first at (y {y}, x {x}): got {got[y, x]}, want {ref[y, x]}"


# ------------------------------------------------------------------------------ 1. the two stages
@pytest.mark.parametrize("h,w", SHAPES)
def test_pyr_down(engine, h, w):
    rng = np.random.default_rng(3000 * h + w)
    left = rng.integers(0, 256, (h, w), dtype=np.uint8)
    right = rng.integers(0, 256, (h, w), dtype=np.uint8)
    right[rng.random((h, w)) < 0.2] = 255                       # sums that need all 10 bits
    gl, gr = engine.pyr_down(left, right)
    assert gl.dtype == np.uint8 and gl.shape == ((h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(gl, pr.down(left)), diff_msg(gl, pr.down(left))
    assert np.array_equal(gr, pr.down(right)), diff_msg(gr, pr.down(right))


@pytest.mark.parametrize("h,w", SHAPES)
def test_pyr_refine(engine, synth, h, w):
    rng = np.random.default_rng(7000 * h + w)
    seen = {"valid": 0, "invalid": 0}
    for m in (0, 3, -5):
        for D in (16, 64, 96):
            if w > m + D + 8:
                left, right, _ = synth.stereo_pair(h, w, max(m, 0), D, seed=h + w + D)
                left, right = np.array(left), np.array(right)
            else:
                left = rng.integers(0, 256, (h, w), dtype=np.uint8)
                right = rng.integers(0, 256, (h, w), dtype=np.uint8)
            Wc, Hc, mc, _, inv_c, inv = pr.plan(w, h, m, D)
            coarse = rng.integers((m - 3) * 8, (m + D + 2) * 8 + 1, (Hc, Wc)).astype(np.int16)
            coarse[rng.random((Hc, Wc)) < 0.3] = inv_c
            for radius in (1, 2):
                for sub in (0, 1):
                    ref = pr.refine(left, right, coarse, m, D, mc, radius, sub)
                    got = engine.pyr_refine(left, right, coarse, m, D, mc, radius, sub)
                    assert got.dtype == np.int16 and np.array_equal(got, ref), \
                        f"{h}x{w} m {m} D {D} radius {radius} subpixel {sub}: " + diff_msg(got, ref)
                    seen["valid"] += int((ref != inv).sum())
                    seen["invalid"] += int((ref == inv).sum())
    assert seen["invalid"] > 0
    if w > 30:
        assert seen["valid"] > 0


def test_known_answers(engine, pkg):
    kat = np.load(os.path.join(ROOT, "tests", "golden", "pyramid", "pyramid_kat.npz"))
    for name in sorted(pr.KAT_SHAPES):
        left, right, coarse = kat[name + "_left"], kat[name + "_right"], kat[name + "_coarse"]
        m, D, radius, sub = (int(v) for v in kat[name + "_par"])
        assert np.array_equal(engine.pyr_down(left, right)[0], kat[name + "_down"]), name
        got = engine.pyr_refine(left, right, coarse, m, D, m >> 1, radius, sub)
        assert np.array_equal(got, kat[name + "_out"]), name + ": " + diff_msg(got, kat[name + "_out"])
    left, right, coarse = kat["c_left"], kat["c_right"], kat["c_coarse"]
    for radius in (0, 3):
        with pytest.raises(pkg.SGMError) as e:
            engine.pyr_refine(left, right, coarse, 3, 16, 1, radius, 1)
        assert e.value.code == pkg.SGM_ERR_PARAM


# --------------------------------------------------------------------------------- 2. end to end
FRAMES = {"A": (120, 330, 0, 64, 5), "B": (121, 333, 3, 96, 9)}       # H, W, minD, D, seed
MODES = ["census", "census4", "census7x7", "sgbm5", "hh8", "bm"]
_cache = {}


@pytest.fixture
def eng(engine, pkg):
    """The shared engine; everything a case may set goes back to its default afterwards."""
    try:
        yield engine
    finally:
        engine.set_pyramid_params(pkg.default_pyramid_params())
        engine.set_fill_params(pkg.default_fill_params())
        engine.set_census_paths(8)
        engine.set_census_window()
        engine.set_raw_format(1, cr.GRAY_Y14)
        engine.set_rectification()
        engine.set_profiling(False)


def frame(synth, name):
    if name not in _cache:
        h, w, m, D, seed = FRAMES[name]
        left, right, _ = synth.stereo_pair(h, w, m, D, seed)
        left.setflags(write=False)
        right.setflags(write=False)
        _cache[name] = (left, right)
    return _cache[name]


def mode_params(pkg, mode, m, D):
    """(sgm_params, paths, census window) of a test mode."""
    if mode.startswith("census"):
        p = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D)
        return p, 4 if mode == "census4" else 8, (7, 7, 1) if mode == "census7x7" else (9, 7, 1)
    return pkg.default_params(rm.MODE_ID[mode], **rm.mode_kw(mode, m, D)), 8, (9, 7, 1)


def configure(eng, pkg, p, paths, cwin, level, radius=2, fill=None):
    eng.set_params(p)
    eng.set_bm_params(pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE))
    eng.set_census_paths(paths)
    eng.set_census_window(*cwin)
    eng.set_fill_params(fill if fill is not None else pkg.default_fill_params())
    eng.set_pyramid_params(pkg.default_pyramid_params(level=level, radius=radius))


def composed(eng, pkg, p, paths, cwin, left, right, radius=2, fill=None, coarse_match=None):
    """down -> a level-0 match of the coarse pair (the engine's own, or coarse_match) -> numpy refine
    (-> numpy fill). left / right: the full-resolution grey pair."""
    h, w = left.shape
    m, D = p.min_disparity, p.num_disparities
    Wc, Hc, mc, Dc, inv_c, inv = pr.plan(w, h, m, D)
    pc = p.copy(min_disparity=mc, num_disparities=Dc)
    lc, rc = pr.down(left), pr.down(right)
    if coarse_match is None:
        configure(eng, pkg, pc, paths, cwin, 0)
        coarse = eng.match(lc, rc)
    else:
        coarse = coarse_match(pc, lc, rc)
    sub = p.subpixel if p.mode == pkg.MODE_CENSUS8 else 1
    out = pr.refine(left, right, coarse, m, D, mc, radius, sub)
    if fill is not None and fill.mode != fr.OFF:
        rect = pr.fill_rect(p.mode == pkg.MODE_OCV_BM, m, D, p.block_size, w, h)
        out = fr.fill_holes(out, inv, fill.mode, fill.max_gap, fill.min_neighbours, rect)
    return out, coarse


@pytest.mark.parametrize("name", sorted(FRAMES))
@pytest.mark.parametrize("mode", MODES)
def test_level1_every_mode(eng, pkg, synth, mode, name):
    left, right = frame(synth, name)
    h, w, m, D, _ = FRAMES[name]
    p, paths, cwin = mode_params(pkg, mode, m, D)
    inv = (m - 1) * 16
    fill = pkg.default_fill_params(mode=fr.BACKGROUND)
    want = {}
    for radius in (2, 1):
        want[radius], coarse = composed(eng, pkg, p, paths, cwin, left, right, radius)
    want["fill"], _ = composed(eng, pkg, p, paths, cwin, left, right, 2, fill)
    configure(eng, pkg, p, paths, cwin, 0)
    lvl0 = eng.match(left, right)
    for radius in (2, 1):
        configure(eng, pkg, p, paths, cwin, 1, radius)
        got = eng.match(left, right)
        assert np.array_equal(got, want[radius]), f"radius {radius}: " + diff_msg(got, want[radius])
    configure(eng, pkg, p, paths, cwin, 1, 2, fill)
    got = eng.match(left, right)
    assert np.array_equal(got, want["fill"]), "fill: " + diff_msg(got, want["fill"])
    # the case says something: valid pixels, a result that is neither level 0's nor the plain upsample
    valid = want[2] != inv
    plain = pr.upsample2(coarse, w, h, m >> 1, m)
    print(mode, name, "valid", float(valid.mean()), "differs from level 0", float((want[2] != lvl0).mean()))
    assert valid.mean() > 0.15 and (want[2] != lvl0).mean() > 0.02 and (want[2] != plain)[valid].mean() > 0.3
    assert not np.array_equal(want[1], want[2])
    if mode != "bm":
        assert (want["fill"] != want[2]).any()


def test_census_subpixel_off_and_the_oracle(eng, pkg, oracle, synth):
    """Census once more with the coarse match done by the CPU oracle; and sub-pixel off."""
    left, right = frame(synth, "B")
    h, w, m, D, _ = FRAMES["B"]
    for sub in (1, 0):
        p = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D, subpixel=sub, median=1,
                               speckle_window_size=20, speckle_range=2)
        want, _ = composed(eng, pkg, p, 8, (9, 7, 1), left, right,
                           coarse_match=lambda pc, lc, rc: oracle.match(to_oracle_params(oracle, pc), lc, rc))
        configure(eng, pkg, p, 8, (9, 7, 1), 1)
        got = eng.match(left, right)
        assert np.array_equal(got, want), f"subpixel {sub}: " + diff_msg(got, want)
        if not sub:
            assert (got[got != (m - 1) * 16] % 16 == 0).all()


def _device_batch(torch, eng, frames, h, w, pad_in=0, pad_out=0, stream=None, single=False):
    n = len(frames)
    dl = torch.zeros((n, h, w + pad_in), dtype=torch.uint8, device="cuda")
    dr = torch.zeros((n, h, w + pad_in), dtype=torch.uint8, device="cuda")
    for i, f in enumerate(frames):
        dl[i, :, :w] = torch.from_numpy(np.array(f[0])).cuda()
        dr[i, :, :w] = torch.from_numpy(np.array(f[1])).cuda()
    out = torch.full((n, h, w + pad_out), 777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    s = stream.cuda_stream if stream is not None else None
    if single:
        eng.match_device(dl[0].data_ptr(), dr[0].data_ptr(), w, h, w + pad_in, out[0].data_ptr(), w + pad_out, s)
    else:
        eng.match_device_batch([dl[i].data_ptr() for i in range(n)], [dr[i].data_ptr() for i in range(n)], w, h,
                               w + pad_in, [out[i].data_ptr() for i in range(n)], w + pad_out, s)
    if stream is not None:
        stream.synchronize()
    else:
        eng.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :, w:] == 777).all()
    return got[:, :, :w]


@pytest.mark.parametrize("mode,filled", [("census", False), ("census", True), ("census4", False), ("sgbm5", False),
                                         ("bm", True)])
def test_entry_points(eng, pkg, synth, mode, filled):
    """match, match_f32 (plain and into a registered buffer: no WTA-written rows at level 1),
    match_device with padded strides on a caller's stream, device batches of 1, 2 and 5 frames whose
    frames differ (a batch equals n single calls)."""
    torch = pytest.importorskip("torch")
    h, w, m, D, _ = FRAMES["A"]
    pairs = [frame(synth, "A"), synth.stereo_pair(h, w, m, D, seed=6)[:2]]
    p, paths, cwin = mode_params(pkg, mode, m, D)
    fill = pkg.default_fill_params(mode=fr.MEDIAN, max_gap=8, min_neighbours=2) if filled else None
    want = [composed(eng, pkg, p, paths, cwin, l, r, 2, fill)[0] for l, r in pairs]
    assert not np.array_equal(want[0], want[1])
    configure(eng, pkg, p, paths, cwin, 1, 2, fill)
    left, right = pairs[0]
    assert np.array_equal(eng.match(left, right), want[0])
    assert np.array_equal(eng.match_f32(left, right), want[0].astype(np.float32))
    buf = np.full((h, w + 5), -7, np.float32)
    eng.host_register(buf)
    try:
        eng.match_f32(left, right, out=buf[:, :w])
        assert np.array_equal(buf[:, :w], want[0].astype(np.float32)), "match_f32 registered"
        assert (buf[:, w:] == -7).all()
    finally:
        eng.host_unregister(buf)
    stream = torch.cuda.Stream()
    got = _device_batch(torch, eng, [pairs[1]], h, w, pad_in=3, pad_out=5, stream=stream, single=True)
    assert np.array_equal(got[0], want[1]), "match_device: " + diff_msg(got[0], want[1])
    for n in (1, 2, 5):
        got = _device_batch(torch, eng, [pairs[i % 2] for i in range(n)], h, w, pad_in=3, pad_out=5,
                            stream=stream if n == 2 else None)
        for i in range(n):
            assert np.array_equal(got[i], want[i % 2]), f"device batch {n}, frame {i}: " + diff_msg(got[i], want[i % 2])


def test_batch_longer_than_a_plane_group(eng, pkg, synth):
    """11 frames: the planes hold 8 at a time, the second group starts after the first's refinement."""
    torch = pytest.importorskip("torch")
    h, w, m, D = 40, 150, 0, 32
    pairs = [synth.stereo_pair(h, w, m, D, seed=60 + i)[:2] for i in range(3)]
    p, paths, cwin = mode_params(pkg, "census", m, D)
    want = [composed(eng, pkg, p, paths, cwin, l, r)[0] for l, r in pairs]
    configure(eng, pkg, p, paths, cwin, 1)
    got = _device_batch(torch, eng, [pairs[i % 3] for i in range(11)], h, w)
    for i in range(11):
        assert np.array_equal(got[i], want[i % 3]), f"frame {i}: " + diff_msg(got[i], want[i % 3])


@pytest.mark.parametrize("mode,ch,n,single", [("census", 1, 2, False), ("census", 3, 5, False), ("census", 1, 1, True),
                                              ("sgbm5", 3, 2, False), ("bm", 1, 1, False), ("hh8", 1, 2, False)])
def test_raw_frames(eng, oracle, pkg, synth, mode, ch, n, single):
    """match_device_batch_rect (and match_device) on raw mono and raw colour frames under
    sgm_set_rectification: level 1 of grey(remap(raw)), and the rectified outputs unchanged."""
    torch = pytest.importorskip("torch")
    name = "203x70"
    rh, rw, h, w, m, D, _ = rm.CASES[name]
    s = cr.GRAY_Y15 if ch == 3 and mode != "census" else cr.GRAY_Y14
    maps, frames, rect = rm.setup(oracle, synth, name, ch)
    p, paths, cwin = mode_params(pkg, mode, m, D)
    fill = pkg.default_fill_params(mode=fr.BACKGROUND) if mode == "census" and ch == 3 else None
    want = [composed(eng, pkg, p, paths, cwin, rm.grey_of(rect[i][0], s), rm.grey_of(rect[i][1], s), 2, fill)[0]
            for i in range(n)]
    configure(eng, pkg, p, paths, cwin, 1, 2, fill)
    got, gl, gr = _batch(torch, eng, maps, frames[:n], h, w, ch, s, single=single)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), f"frame {i}: " + diff_msg(got[i], want[i])
        for g, side in ((gl, 0), (gr, 1)):
            if g is not None:
                assert np.array_equal(g[i], rect[i][side]), f"frame {i} rectified {'LR'[side]}"
    assert (want[0] != (m - 1) * 16).mean() > 0.2


@pytest.mark.parametrize("mode,ch", [("census", 1), ("sgbm5", 3), ("bm", 1)])
def test_node_frame(eng, pkg, synth, mode, ch):
    """node_frame at level 1: the DisparityImage (read back through an unbounded window, where the
    float image is d / 16 exactly) is level 1 of the grey rectified pair that level 0 returns; the
    rectified images do not change; a registered output takes no WTA-written rows."""
    h, w, D, m = 70, 300, 64, 3
    infos = [calib(seed=11, w=w, h=h), calib(seed=12, w=w, h=h)]
    raw = rm.raw_frames(synth, h, w, m, D, D + 5, ch)
    s = cr.GRAY_Y15 if ch == 3 else cr.GRAY_Y14
    p, paths, cwin = mode_params(pkg, mode, m, D)
    big = np.float32(3.0e38)
    configure(eng, pkg, p, paths, cwin, 0)
    eng.set_raw_format(ch, s)
    plain = eng.node_frame(raw[0], raw[1], infos[0], infos[1], -big, big)
    eng.set_raw_format(1, cr.GRAY_Y14)
    want, _ = composed(eng, pkg, p, paths, cwin, rm.grey_of(plain[0], s), rm.grey_of(plain[1], s))
    configure(eng, pkg, p, paths, cwin, 1)
    eng.set_raw_format(ch, s)
    for registered in (False, True):
        disp = np.full((h, w), -1.0, np.float32)
        if registered:
            eng.host_register(disp)
        try:
            got = eng.node_frame(raw[0], raw[1], infos[0], infos[1], -big, big, disparity=disp)
        finally:
            if registered:
                eng.host_unregister(disp)
        d16 = np.round(disp * 16).astype(np.int16)
        assert np.array_equal(d16.astype(np.float32) * np.float32(1 / 16), disp)
        assert np.array_equal(d16, want), f"registered {registered}: " + diff_msg(d16, want)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    assert (want != (m - 1) * 16).mean() > 0.2 and not np.array_equal(want, np.round(plain[2] * 16).astype(np.int16))


def test_census_range_1024(eng, pkg, synth):
    """Census m 0, D 1024 on 24 x 1100: refused at level 0 (the 512 cap), matched at level 1 with a
    coarse range of 512."""
    h, w, D = 24, 1100, 1024
    left, right, _ = synth.stereo_pair(h, w, 0, D, seed=21)
    p, paths, cwin = mode_params(pkg, "census", 0, D)
    configure(eng, pkg, p, paths, cwin, 0)
    with pytest.raises(pkg.SGMError) as e:
        eng.match(left, right)
    assert e.value.code == pkg.SGM_ERR_UNSUPPORTED
    want, _ = composed(eng, pkg, p, paths, cwin, left, right)
    configure(eng, pkg, p, paths, cwin, 1)
    assert eng.pyramid_plan(w, h) == dict(Wc=550, Hc=12, mc=0, Dc=512, invalid_c=-16, invalid=-16)
    got = eng.match(left, right)
    assert np.array_equal(got, want), diff_msg(got, want)
    assert (got[:, :1024] == -16).all() and (got[:, 1024:] != -16).mean() > 0.05


def test_refusals_leave_outputs_untouched(eng, pkg, synth):
    """sgm_match_batch and the three tile modes return SGM_ERR_UNSUPPORTED at level 1."""
    torch = pytest.importorskip("torch")
    left, right = frame(synth, "A")
    h, w, m, D, _ = FRAMES["A"]
    p, paths, cwin = mode_params(pkg, "census", m, D)
    configure(eng, pkg, p, paths, cwin, 1)
    lib, vp = eng.lib, ctypes.c_void_p
    out = np.full((h, w), 4321, np.int16)
    lp, rp, op = vp(left.ctypes.data), vp(right.ctypes.data), vp(out.ctypes.data)
    one = ctypes.c_void_p * 1
    dev0 = (ctypes.c_int * 1)(0)
    calls = {
        "sgm_match_batch": lambda: lib.sgm_match_batch(eng.h, one(lp), one(rp), 1, w, h, w, one(op), w, dev0, 1),
        "sgm_match_tiled": lambda: lib.sgm_match_tiled(eng.h, lp, rp, w, h, w, op, w, 2, 8, dev0, 1),
        "sgm_match_tiled_exact": lambda: lib.sgm_match_tiled_exact(eng.h, lp, rp, w, h, w, op, w, 2, dev0, 1)}
    for name, call in calls.items():
        assert call() == pkg.SGM_ERR_UNSUPPORTED, name
        assert name in eng.error() and "level" in eng.error()
        assert (out == 4321).all(), name
    dl, dr = torch.from_numpy(np.array(left)).cuda(), torch.from_numpy(np.array(right)).cuda()
    dout = torch.full((h, w), 1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(pkg.SGMError) as e:
        eng.match_tiled_device(dl.data_ptr(), dr.data_ptr(), w, h, w, dout.data_ptr(), w, 2, 8, devices=[0])
    assert e.value.code == pkg.SGM_ERR_UNSUPPORTED
    assert (dout.cpu().numpy() == 1234).all()
    eng.set_pyramid_params(pkg.default_pyramid_params())
    for name, call in calls.items():                         # level 0: they run
        assert call() == pkg.SGM_OK, name
        assert (out != 4321).any()
        out[...] = 4321


def test_bad_values_fail_at_match_time(eng, pkg, synth):
    """Setters store anything; a match decides, before any output byte is written, and the errors of
    the coarse match name the coarse geometry."""
    torch = pytest.importorskip("torch")
    left, right = frame(synth, "A")
    h, w, m, D, _ = FRAMES["A"]
    p, paths, cwin = mode_params(pkg, "census", m, D)
    dl, dr = torch.from_numpy(np.array(left)).cuda(), torch.from_numpy(np.array(right)).cuda()
    dout = torch.full((h, w), 1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for level, radius in [(2, 2), (-1, 2), (1, 0), (1, 3)]:
        configure(eng, pkg, p, paths, cwin, level, radius)
        assert eng.get_pyramid_params().as_dict() == dict(level=level, radius=radius)
        for call in (lambda: eng.match(left, right), lambda: eng.match_f32(left, right),
                     lambda: eng.match_device(dl.data_ptr(), dr.data_ptr(), w, h, w, dout.data_ptr(), w),
                     lambda: eng.match_device_batch([dl.data_ptr()] * 2, [dr.data_ptr()] * 2, w, h, w,
                                                    [dout.data_ptr()] * 2, w)):
            with pytest.raises(pkg.SGMError) as e:
                call()
            assert e.value.code == pkg.SGM_ERR_PARAM, (level, radius)
    eng.synchronize()
    assert (dout.cpu().numpy() == 1234).all()
    # the coarse match's own errors: census Dc 528; a BM window that fits 60 x 44 but not 30 x 22
    wide = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=1040)
    configure(eng, pkg, wide, 8, (9, 7, 1), 1)
    with pytest.raises(pkg.SGMError) as e:
        eng.match_device(dl.data_ptr(), dr.data_ptr(), w, h, w, dout.data_ptr(), w)
    assert e.value.code == pkg.SGM_ERR_UNSUPPORTED and "coarse" in eng.error() and "528" in eng.error()
    bm = pkg.default_params(pkg.MODE_OCV_BM, **rm.mode_kw("bm", 0, 16, block=23))
    configure(eng, pkg, bm, 8, (9, 7, 1), 1)
    with pytest.raises(pkg.SGMError) as e:
        eng.match_device(dl.data_ptr(), dr.data_ptr(), 60, 44, w, dout.data_ptr(), w)
    assert e.value.code == pkg.SGM_ERR_PARAM and "coarse" in eng.error() and "30 x 22" in eng.error()
    configure(eng, pkg, bm, 8, (9, 7, 1), 0)
    eng.match_device(dl.data_ptr(), dr.data_ptr(), 60, 44, w, dout.data_ptr(), w)       # level 0 takes it
    eng.synchronize()
    assert (dout.cpu().numpy()[44:] == 1234).all() and (dout.cpu().numpy()[:44, :60] != 1234).all()
    # level 0 does not look at the radius
    configure(eng, pkg, p, paths, cwin, 0, 99)
    eng.match(left, right)


def test_level0_after_level1(eng, pkg, synth):
    """One handle: level 0, level 1 (single, batch), level 0 again, bit for bit; and the caller's
    configuration is what it was after every level-1 call, also a failed one."""
    torch = pytest.importorskip("torch")
    left, right = frame(synth, "B")
    h, w, m, D, _ = FRAMES["B"]
    for mode in ("census", "sgbm5"):
        p, paths, cwin = mode_params(pkg, mode, m, D)
        fill = pkg.default_fill_params(mode=fr.MEDIAN, max_gap=5, min_neighbours=3)
        configure(eng, pkg, p, paths, cwin, 0, 2, fill)
        before = eng.match(left, right)
        before_batch = _device_batch(torch, eng, [(left, right)] * 3, h, w)
        configure(eng, pkg, p, paths, cwin, 1, 1, fill)
        one = eng.match(left, right)
        many = _device_batch(torch, eng, [(left, right)] * 3, h, w)
        assert all(np.array_equal(one, many[i]) for i in range(3)) and not np.array_equal(one, before)
        assert eng.get_params().as_dict() == p.as_dict() and eng.get_fill_params().as_dict() == fill.as_dict()
        assert eng.get_pyramid_params().as_dict() == dict(level=1, radius=1)
        eng.set_params(p.copy(num_disparities=2064))
        with pytest.raises(pkg.SGMError):
            eng.match(left, right)
        assert eng.get_params().num_disparities == 2064 and eng.get_fill_params().as_dict() == fill.as_dict()
        configure(eng, pkg, p, paths, cwin, 0, 2, fill)
        assert np.array_equal(eng.match(left, right), before)
        after_batch = _device_batch(torch, eng, [(left, right)] * 3, h, w)
        assert np.array_equal(after_batch, before_batch)


def test_stage_names_and_bytes(eng, pkg, synth):
    """A profiled level-1 frame: pyr_down, the coarse match's stages under their usual names with the
    bytes of the coarse geometry, pyr_refine, then fill; level 0 lists neither new stage."""
    left, right = frame(synth, "B")
    h, w, m, D, _ = FRAMES["B"]
    Wc, Hc, mc, Dc, _, _ = pr.plan(w, h, m, D)
    p = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D, median=1)
    configure(eng, pkg, p, 8, (9, 7, 1), 1, 2, pkg.default_fill_params(mode=fr.MEDIAN))
    eng.set_profiling(True)
    eng.match(left, right)
    st = eng.stage_times()
    assert eng.profiled_matches() == 1
    eng.set_profiling(False)
    assert [s[0] for s in st] == ["pyr_down", "census", "paths8", "wta_lr", "median3", "pyr_refine", "fill"], st
    by = {s[0]: s[2] for s in st}
    assert by["pyr_down"] == 10.5 * w * h and by["pyr_refine"] == 10.5 * w * h and by["fill"] == 4.0 * w * h
    width1c = Wc + min(mc, 0) - max(mc + Dc, 0)
    assert by["census"] == 18.0 * Wc * Hc and by["median3"] == 4.0 * Wc * Hc
    assert by["paths8"] == 8.0 * width1c * Hc * Dc
    assert all(s[1] > 0 for s in st)
    configure(eng, pkg, p, 8, (9, 7, 1), 0)
    eng.set_profiling(True)
    eng.match(left, right)
    names = [s[0] for s in eng.stage_times()]
    eng.set_profiling(False)
    assert names == ["census", "paths8", "wta_lr", "median3"]


# ------------------------------------------------------------------------------------ adapters
def test_python_adapter(pkg, synth, monkeypatch):
    """MatcherHIPSGM: setPyramidLevel, SGM_HIP_PYRAMID=1 and =scale with setDownsampleScale(0.5) give
    the engine's level-1 image; the right matcher inherits the level."""
    left, right = (np.array(a) for a in frame(synth, "A"))
    h, w, m, D, _ = FRAMES["A"]

    def matcher():
        mt = pkg.MatcherHIPSGM(" ", (w, h), mode=pkg.MODE_CENSUS8, census_paths=8)
        mt.params = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D)
        mt.setImages(left, right)
        return mt

    monkeypatch.delenv("SGM_HIP_PYRAMID", raising=False)
    mt = matcher()
    try:
        assert mt.forwardMatch() == 0
        lvl0 = mt.getDisparity()
        mt.setDownsampleScale(0.5)                   # not followed: nothing changes
        assert mt.forwardMatch() == 0 and np.array_equal(mt.getDisparity(), lvl0)
        mt.setPyramidLevel(1)
        assert mt.forwardMatch() == 0
        lvl1 = mt.getDisparity()
        want, _ = composed(mt._engine_for(), pkg, mt.params, 8, (9, 7, 1), left, right)
        assert np.array_equal(lvl1, want.astype(np.float32))
        assert mt.backwardMatch() == 0
        back1 = mt.getBackDisparity()
        mt.setPyramidLevel(0)
        assert mt.backwardMatch() == 0 and not np.array_equal(mt.getBackDisparity(), back1)
        mt.setPyramidLevel(3)
        assert mt.forwardMatch() == -1
    finally:
        mt._engine_for().close()
    for env, scale, exp in (("1", 1.0, lvl1), ("scale", 0.5, lvl1), ("scale", 1.0, lvl0)):
        monkeypatch.setenv("SGM_HIP_PYRAMID", env)
        mt = matcher()
        try:
            mt.setDownsampleScale(scale)
            assert mt.forwardMatch() == 0 and np.array_equal(mt.getDisparity(), exp), (env, scale)
        finally:
            mt._engine_for().close()


def test_plugin_driver(eng, pkg):
    """plugin_pyramid_test match: the C++ adapter core's forwardMatch at level 0 and 1, with the scale
    driving the level, and the right matcher at level 1."""
    left, right = cpr.driver_frame()
    p = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=0, num_disparities=32, uniqueness_ratio=10, p1=8, p2=64,
                           disp12_max_diff=1, block_size=5, prefilter_cap=0, speckle_window_size=0, speckle_range=0)
    want = {}
    configure(eng, pkg, p, 8, (9, 7, 1), 0)
    want["level0"] = want["scale_one"] = eng.match(left, right)
    want["level1"], _ = composed(eng, pkg, p, 8, (9, 7, 1), left, right)
    want["scale_half"] = want["level1"]
    configure(eng, pkg, pkg.right_matcher_params(p), 8, (9, 7, 1), 1)
    want["backward_half"] = eng.match(right, left)
    assert len({cpr.fnv1a16(v) for v in (want["level0"], want["level1"], want["backward_half"])}) == 3
    env = {k: v for k, v in os.environ.items() if k not in ("SGM_HIP_PYRAMID", "SGM_HIP_FILL", "SGM_HIP_CENSUS_WINDOW",
                                                             "SGM_HIP_CENSUS_PATHS")}
    r = subprocess.run([DRIVER, "match"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "pyramid match ok" in r.stdout, r.stdout + r.stderr
    got = dict(line.split(" hash ") for line in r.stdout.splitlines() if " hash " in line)
    assert got == {k: "%016x" % cpr.fnv1a16(v) for k, v in want.items()}
