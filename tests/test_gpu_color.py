"""GPU parity of the colour stage: sgm_bgr2gray, sgm_remap_cubic_c3 and 8UC3 frames through the
match entry points (sgm_set_raw_format), bit-exact against references composed from the oracle
(remap per channel plane, rectify_map, match), tests/census_paths_reference.py, tests/bm_reference.py
and the numpy grey conversion of tests/color_reference.py.

The colour frames are synth.stereo_pair through three different monotone per-channel tables; every
frame is checked on the CPU to tell a wrong channel order, plane or grey set apart
(color_reference.check_discriminating), so such a mistake cannot pass.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm_reference as br  # noqa: E402
import census_paths_reference as cpr  # noqa: E402
import color_reference as cr  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

pytestmark = pytest.mark.gpu

SETS = [cr.GRAY_Y14, cr.GRAY_Y15]
_cache = {}


def _once(key, fn):
    """A reference computed once, shared by the tests that need it, never modified."""
    if key not in _cache:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


@contextlib.contextmanager
def raw_format(engine, channels, gray_set):
    """The session's engine is shared: the raw format always goes back to mono."""
    engine.set_raw_format(channels, gray_set)
    try:
        yield
    finally:
        engine.set_raw_format(1, cr.GRAY_Y14)


def _dev(torch, a):
    return torch.as_tensor(np.array(a, copy=True)).cuda()      # the cached references are read-only


def diff_msg(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} differ, first {bad[:4].tolist()}"


# ------------------------------------------------------------------------------ 1. sgm_bgr2gray
@pytest.mark.parametrize("s", SETS, ids=["Y14", "Y15"])
@pytest.mark.parametrize("w,h,stride", [(1, 1, 3), (67, 5, 3 * 67 + 5), (64, 4, 192), (257, 9, 771)])
def test_bgr2gray(engine, w, h, stride, s):
    """Odd strides take the byte path, dword-aligned rows the packed one, 257 both plus a tail."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(w * 11 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if w * h > 1:
        cr.check_discriminating(img)
    buf = np.full((h, stride), 201, np.uint8)
    buf[:, :3 * w] = img.reshape(h, 3 * w)
    src = _dev(torch, buf)
    out = torch.full((h, w + 3), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.bgr2gray(src.data_ptr(), stride, w, h, out.data_ptr(), w + 3, s)
    engine.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :w], cr.gray(img, s)), diff_msg(got[:, :w], cr.gray(img, s))
    assert (got[:, w:] == 99).all()


def test_bgr2gray_unknown_set(engine, pkg):
    torch = pytest.importorskip("torch")
    src = torch.zeros((4, 12), dtype=torch.uint8, device="cuda")
    out = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.SGMError) as e:
        engine.bgr2gray(src.data_ptr(), 12, 4, 4, out.data_ptr(), 4, 7)
    assert e.value.code == pkg.SGM_ERR_PARAM


# ------------------------------------------------------------------------ 2. sgm_remap_cubic_c3
def _tap_border(mx, my, sw, sh):
    """Pixels whose 4 x 4 tap window is not wholly inside the source (the remap's border path)."""
    with np.errstate(invalid="ignore", over="ignore"):
        X, Y = np.rint(mx.astype(np.float64) * 32), np.rint(my.astype(np.float64) * 32)
    ok = np.isfinite(X) & np.isfinite(Y) & (np.abs(X) < 2.0 ** 31) & (np.abs(Y) < 2.0 ** 31)
    sx = np.where(ok, np.floor(np.where(ok, X, 0) / 32), -9) - 1
    sy = np.where(ok, np.floor(np.where(ok, Y, 0) / 32), -9) - 1
    return ~(ok & (sx >= 0) & (sx + 3 < sw) & (sy >= 0) & (sy + 3 < sh))


def _remap_c3(torch, engine, src, mx, my, pad=5):
    sh, sw = src.shape[:2]
    h, w = mx.shape
    d_src = _dev(torch, src)
    d_mx, d_my = _dev(torch, mx), _dev(torch, my)
    out = torch.full((h, 3 * w + pad), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.remap_cubic(d_src.data_ptr(), 3 * sw, sw, sh, d_mx.data_ptr(), d_my.data_ptr(), w, w, h, out.data_ptr(),
                       3 * w + pad, channels=3)
    engine.synchronize()
    got = out.cpu().numpy()
    assert (got[:, 3 * w:] == 99).all()
    return got[:, :3 * w].reshape(h, w, 3)


def _c3_maps(oracle, sw, sh, w, h):
    """Maps of a w x h output out of a sw x sh source: rectify_map with distortion (the new camera
    zoomed so that the output stays mostly inside the source), plus hand-made entries."""
    K, D, R, P = calib(seed=sw, w=sw, h=sh)
    P = np.array(P, np.float64)
    P[0, 0] *= 1.25 * w / sw
    P[1, 1] *= 1.25 * h / sh
    P[0, 2], P[1, 2] = w / 2.0, h / 2.0
    mx, my = (m.copy() for m in oracle.rectify_map(K, D, R, P, w, h))
    # taps partly / wholly outside, negative coordinates, exact 1/64 ties, one NaN and one value
    # outside the int range
    mx[0, :8] = [-0.5, -1.25, -4.0, -300.0, sw - 2.5, sw - 0.5, sw + 2.0, sw + 400.0]
    my[0, :8] = 3.0
    my[1, :6] = [-0.5, -2.75, -50.0, sh - 1.5, sh + 1.0, sh + 99.0]
    mx[1, :6] = 7.25
    mx[2] = np.round(mx[2] * 64) / 64 + 1.0 / 64        # exact 1/64 ties (round half to even)
    my[3] = np.floor(my[3]) + 0.515625
    mx[4, 0], my[4, 1] = np.nan, 1e30
    mx[5:8] -= 0.7 * sw                                   # three rows run off the left edge
    my[9:12] += 0.8 * sh                                  # ... and three off the bottom
    return mx, my


@pytest.mark.parametrize("sw,sh,w,h", [(50, 41, 70, 37), (160, 48, 130, 40)])
def test_remap_cubic_c3(engine, oracle, sw, sh, w, h):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(sw + h)
    src = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    mx, my = _c3_maps(oracle, sw, sh, w, h)
    share = _tap_border(mx, my, sw, sh).mean()
    print("border share", share)
    assert 0.0 < share < 0.5                             # both remap paths run
    got = _remap_c3(torch, engine, src, mx, my)
    ref = cr.remap3(oracle, src, mx, my)
    assert np.array_equal(got, ref), diff_msg(got, ref)
    assert (ref[0, 3] == 0).all() and (ref[0, 7] == 0).all()      # wholly outside: 0 in every channel


def test_remap_cubic_c3_identity(engine):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (23, 70, 3), dtype=np.uint8)
    my, mx = (a.astype(np.float32) for a in np.mgrid[0:23, 0:70])
    assert np.array_equal(_remap_c3(torch, engine, src, mx, my), src)


# --------------------------------------------- 3. census device batch, raw colour + rectification
# (raw h, raw w, h, w, minD, D, seed)
RECT_CASES = {"130x40": (50, 140, 40, 130, 0, 32, 5), "200x70": (80, 210, 70, 200, -8, 64, 6),
              "1920x70": (70, 1920, 70, 1920, 0, 32, 8)}
NMAX = 5


def _rect_setup(oracle, synth, name):
    """Raw colour frames, host maps and rectified colour references of a case."""
    def make():
        rh, rw, h, w, m, D, seed = RECT_CASES[name]
        n = 1 if name == "1920x70" else NMAX
        cal = [calib(seed=11, w=rw, h=rh), calib(seed=12, w=rw, h=rh)]
        maps = [oracle.rectify_map(*c, w, h) for c in cal]
        frames = [cr.color_pair(synth, rh, rw, m, D, seed + 10 * i) for i in range(n)]
        for f in frames:
            cr.check_discriminating(f[0])
            cr.check_discriminating(f[1])
        rect = [(cr.remap3(oracle, f[0], *maps[0]), cr.remap3(oracle, f[1], *maps[1])) for f in frames]
        return maps, frames, rect
    return _once(("rect", name), make)


def _rect_ref(oracle, pkg, synth, name, i, paths, s):
    """Disparity of frame i: the oracle on gray(remap3(raw)), the node's order."""
    def make():
        rh, rw, h, w, m, D, seed = RECT_CASES[name]
        _, _, rect = _rect_setup(oracle, synth, name)
        gl, gr = cr.gray(rect[i][0], s), cr.gray(rect[i][1], s)
        op = oracle.make_params(oracle.MODE_CENSUS8, min_disparity=m, num_disparities=D)
        ref = oracle.match(op, gl, gr) if paths == 8 else cpr.match_paths(oracle, op, gl, gr)
        assert (ref != (m - 1) * 16).mean() > 0.3          # a real disparity map, not an empty one
        return ref
    return _once(("rect_ref", name, i, paths, s), make)


def _run_rect(torch, engine, pkg, oracle, synth, name, n, paths, s, want_l=True, want_r=True):
    rh, rw, h, w, m, D, seed = RECT_CASES[name]
    maps, frames, rect = _rect_setup(oracle, synth, name)
    engine.set_params(pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D))
    engine.set_census_paths(paths)
    dm = [_dev(torch, a) for mp in maps for a in mp]
    dl = [_dev(torch, f[0]) for f in frames[:n]]
    dr = [_dev(torch, f[1]) for f in frames[:n]]
    out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
    rs = 3 * w + 7                                         # padded rectified rows (bytes)
    recl = torch.full((n, h, rs), 99, dtype=torch.uint8, device="cuda")
    recr = torch.full((n, h, rs), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        with raw_format(engine, 3, s):
            engine.set_rectification((dm[0].data_ptr(), dm[1].data_ptr()), (dm[2].data_ptr(), dm[3].data_ptr()), w, rw, rh)
            engine.match_device_batch_rect([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, 3 * rw,
                                           [recl[i].data_ptr() for i in range(n)] if want_l else None,
                                           [recr[i].data_ptr() for i in range(n)] if want_r else None,
                                           rs, [out[i].data_ptr() for i in range(n)], w)
            engine.synchronize()
    finally:
        engine.set_rectification()
        engine.set_census_paths(8)
    got, gl, gr = out.cpu().numpy(), recl.cpu().numpy(), recr.cpu().numpy()
    for i in range(n):
        ref = _rect_ref(oracle, pkg, synth, name, i, paths, s)
        assert np.array_equal(got[i], ref), f"frame {i} disparity: " + diff_msg(got[i], ref)
        for g, e, want in ((gl[i], rect[i][0], want_l), (gr[i], rect[i][1], want_r)):
            if want:
                assert np.array_equal(g[:, :3 * w].reshape(h, w, 3), e), f"frame {i} rectified colour"
                assert (g[:, 3 * w:] == 99).all()
            else:
                assert (g == 99).all()


@pytest.mark.parametrize("upwta", [None, "0"], ids=["upwta", "upwta0"])
@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("name", ["130x40", "200x70"])
def test_census_batch_raw_colour_rectified(engine, oracle, pkg, synth, monkeypatch, name, n, paths, upwta):
    """First, steady and last launches of the pipelined batch (n = 1, 2, 3, 5), both path sets and
    both batch schemes; 130x40 is two full x-tiles + 2 px and one tile row + 8 rows."""
    torch = pytest.importorskip("torch")
    if upwta is not None:
        monkeypatch.setenv("SGM_UPWTA", upwta)
    s = cr.GRAY_Y14 if name == "130x40" else cr.GRAY_Y15
    _run_rect(torch, engine, pkg, oracle, synth, name, n, paths, s)


@pytest.mark.parametrize("want_l,want_r", [(True, False), (False, True), (False, False)], ids=["L", "R", "none"])
def test_census_batch_raw_colour_rect_outputs(engine, oracle, pkg, synth, want_l, want_r):
    torch = pytest.importorskip("torch")
    _run_rect(torch, engine, pkg, oracle, synth, "130x40", 3, 8, cr.GRAY_Y14, want_l, want_r)


def test_census_raw_colour_rectified_production_width(engine, oracle, pkg, synth):
    """One 1920 x 70 frame: every x-tile of the production width."""
    torch = pytest.importorskip("torch")
    _run_rect(torch, engine, pkg, oracle, synth, "1920x70", 1, 8, cr.GRAY_Y15)


def test_single_frame_device_match_raw_colour_rectified(engine, oracle, pkg, synth):
    """sgm_match_device takes raw colour too while rectification is on."""
    torch = pytest.importorskip("torch")
    name, s = "130x40", cr.GRAY_Y15
    rh, rw, h, w, m, D, seed = RECT_CASES[name]
    maps, frames, _ = _rect_setup(oracle, synth, name)
    engine.set_params(pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D))
    dm = [_dev(torch, a) for mp in maps for a in mp]
    dl, dr = _dev(torch, frames[0][0]), _dev(torch, frames[0][1])
    out = torch.full((h, w), 555, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    try:
        with raw_format(engine, 3, s):
            engine.set_rectification((dm[0].data_ptr(), dm[1].data_ptr()), (dm[2].data_ptr(), dm[3].data_ptr()), w, rw, rh)
            engine.match_device(dl.data_ptr(), dr.data_ptr(), w, h, 3 * rw, out.data_ptr(), w)
            engine.synchronize()
            with pytest.raises(pkg.SGMError):                  # a stride in pixels is too short
                engine.match_device(dl.data_ptr(), dr.data_ptr(), w, h, rw, out.data_ptr(), w)
    finally:
        engine.set_rectification()
    assert np.array_equal(out.cpu().numpy(), _rect_ref(oracle, pkg, synth, name, 0, 8, s))


# ----------------------------------------------------------- 4. colour without rectification
def _bm_sad_volume_fast(bm, PL, PR):
    """bm_reference.sad_volume with the window sums taken as box sums of per-disparity difference
    images (the same clamped window of the same definition, summed in another order; integers, so
    the results are equal: checked against the direct sums on the small case below). The direct
    double sum takes most of a minute at 640 x 480."""
    PL, PR = np.asarray(PL).astype(np.int64), np.asarray(PR).astype(np.int64)
    H, W = PL.shape
    rng = br.column_range(bm, W)
    if rng is None:
        return None
    w2, s = bm.w // 2, bm.D - 1 + bm.m
    x0, x1 = rng
    u = np.arange(x0 - w2, x1 + w2)                            # window columns of every output column
    lu = PL[:, np.clip(u, 0, W - 1)]
    ru0 = np.clip(u - s, 0, W - bm.D)

    def box(a):                                                # sums over (2 w2 + 1)^2, valid positions only
        c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
        c[1:, 1:] = a.cumsum(0).cumsum(1)
        k = 2 * w2 + 1
        return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]

    sad = np.stack([box(np.abs(lu - PR[:, ru0 + e])) for e in range(bm.D)], axis=2)
    return sad, box(np.abs(lu - bm.c))


NOREC_CASES = {"96x48": (48, 96, 0, 32, 7), "640x480": (480, 640, 9, 64, 9)}
MODES = ["census", "sgbm", "hh", "bm"]


def _norec_params(pkg, name, mode):
    h, w, m, D, _ = NOREC_CASES[name]
    if name == "640x480":            # the node defaults (generate_disparity.cpp:100-112) of every mode
        if mode == "census":
            return pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D)
        return pkg.default_params({"sgbm": pkg.MODE_OCV_SGBM5, "hh": pkg.MODE_OCV_HH8, "bm": pkg.MODE_OCV_BM}[mode])
    if mode == "census":
        return pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D, median=1)
    if mode == "bm":
        return pkg.default_params(pkg.MODE_OCV_BM, min_disparity=m, num_disparities=D, block_size=9,
                                  speckle_window_size=0, speckle_range=0)
    return pkg.default_params(pkg.MODE_OCV_SGBM5 if mode == "sgbm" else pkg.MODE_OCV_HH8, min_disparity=m,
                              num_disparities=D, block_size=5, p1=40, p2=160)


def _norec_frames(synth, name):
    def make():
        h, w, m, D, seed = NOREC_CASES[name]
        frames = [cr.color_pair(synth, h, w, m, D, seed + i) for i in range(3)]
        cr.check_discriminating(frames[0][0])
        cr.check_discriminating(frames[0][1])
        return frames
    return _once(("norec", name), make)


def _norec_ref(oracle, pkg, synth, monkeypatch, name, mode, s):
    """The oracle's disparity of frame 0 on the host-converted grey pair."""
    def make():
        from conftest import to_oracle_params
        p = _norec_params(pkg, name, mode)
        l, r = _norec_frames(synth, name)[0]
        gl, gr = cr.gray(l, s), cr.gray(r, s)
        if mode != "bm":
            return oracle.match(to_oracle_params(oracle, p), gl, gr)
        bm = br.BM(p.min_disparity, p.num_disparities, p.block_size, p.prefilter_cap, 10, p.uniqueness_ratio)
        if name == "96x48":           # the fast window sums equal bm_reference's direct ones
            PL, PR = br.prefilter(gl, bm.c), br.prefilter(gr, bm.c)
            for a, b in zip(_bm_sad_volume_fast(bm, PL, PR), br.sad_volume(bm, PL, PR)):
                assert np.array_equal(a, b)
            ref = br.compute(bm, gl, gr)
        else:
            with monkeypatch.context() as mp:
                mp.setattr(br, "sad_volume", _bm_sad_volume_fast)
                ref = br.compute(bm, gl, gr)
        if p.speckle_window_size > 0:
            ref = oracle.filter_speckles(ref, br.filtered(bm), p.speckle_window_size, p.speckle_range)
        return ref
    return _once(("norec_ref", name, mode, s), make)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(NOREC_CASES))
def test_colour_frames_without_rectification(engine, oracle, pkg, synth, monkeypatch, name, mode):
    """sgm_match, sgm_match_f32, sgm_match_device and sgm_match_device_batch on 8UC3 frames: each
    equals the same call on the host-converted grey frames, and the oracle."""
    torch = pytest.importorskip("torch")
    h, w, m, D, _ = NOREC_CASES[name]
    s = cr.GRAY_Y15 if mode in ("census", "hh") else cr.GRAY_Y14
    p = _norec_params(pkg, name, mode)
    frames = _norec_frames(synth, name)
    grey = [(cr.gray(l, s), cr.gray(r, s)) for l, r in frames]
    ref = _norec_ref(oracle, pkg, synth, monkeypatch, name, mode, s)
    assert (ref != (p.min_disparity - 1) * 16).mean() > 0.3
    engine.set_params(p)
    engine.set_bm_params(pkg.default_bm_params())

    def device_calls(pairs, bpp):
        dl = [_dev(torch, a) for a, _ in pairs]
        dr = [_dev(torch, b) for _, b in pairs]
        one = torch.full((h, w + 2), 555, dtype=torch.int16, device="cuda")
        out = torch.full((3, h, w), 777, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        engine.match_device(dl[0].data_ptr(), dr[0].data_ptr(), w, h, bpp * w, one.data_ptr(), w + 2)
        engine.match_device_batch([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, bpp * w,
                                  [out[i].data_ptr() for i in range(3)], w)
        engine.synchronize()
        one = one.cpu().numpy()
        assert (one[:, w:] == 555).all()
        return one[:, :w], out.cpu().numpy()

    m_host, f_host = engine.match(*grey[0]), engine.match_f32(*grey[0])
    d_host, b_host = device_calls(grey, 1)
    with raw_format(engine, 3, s):
        m_col, f_col = engine.match(*frames[0]), engine.match_f32(*frames[0])
        d_col, b_col = device_calls(frames, 3)
    assert np.array_equal(m_col, ref), "sgm_match vs the oracle: " + diff_msg(m_col, ref)
    assert np.array_equal(m_col, m_host) and np.array_equal(f_col, f_host)
    assert f_col.dtype == np.float32 and np.array_equal(f_col, ref.astype(np.float32))
    assert np.array_equal(d_col, ref) and np.array_equal(d_col, d_host)
    assert np.array_equal(b_col, b_host) and np.array_equal(b_col[0], ref)
    assert not np.array_equal(b_col[1], b_col[0])


def test_gray_stage_is_profiled(engine, pkg, synth):
    """The OCV / BM pre-pass is a stage named `gray`; the census stage counts 3 B/px read."""
    h, w, m, D, _ = NOREC_CASES["96x48"]
    l, r = _norec_frames(synth, "96x48")[0]
    for mode, stage, nbytes in (("bm", "gray", 8 * h * w), ("census", "census", 6 * h * w + 16 * h * w)):
        engine.set_params(_norec_params(pkg, "96x48", mode))
        with raw_format(engine, 3, cr.GRAY_Y14):
            engine.set_profiling(True)
            try:
                engine.match(l, r)
                st = {n: b for n, _, b in engine.stage_times()}
            finally:
                engine.set_profiling(False)
        assert stage in st and st[stage] == nbytes, st
        assert ("gray" in st) == (mode == "bm")


# ----------------------------------------------------------- 5. entry points without colour
def test_entry_points_without_colour_support(engine, pkg, synth):
    torch = pytest.importorskip("torch")
    h, w, m, D, _ = NOREC_CASES["96x48"]
    left, right, _ = synth.stereo_pair(h, w, m, D, seed=3)
    engine.set_params(pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D))
    before = engine.match(left, right)
    dl, dr = _dev(torch, left), _dev(torch, right)
    out = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with raw_format(engine, 3, cr.GRAY_Y14):
        assert engine.get_raw_format() == (3, cr.GRAY_Y14)
        col, colr = np.repeat(left[:, :, None], 3, axis=2), np.repeat(right[:, :, None], 3, axis=2)
        assert np.array_equal(engine.match(col, colr), before)                # (v, v, v) -> v
        for call in (lambda: engine.match_batch([left], [right], devices=[0]),
                     lambda: engine.match_tiled(left, right, 2, 4, devices=[0]),
                     lambda: engine.match_tiled_exact(left, right, 2, devices=[0]),
                     lambda: engine.match_tiled_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w, 2, 4,
                                                       devices=[0])):
            with pytest.raises(pkg.SGMError) as e:
                call()
            assert e.value.code == pkg.SGM_ERR_UNSUPPORTED, str(e.value)
    for ch, s in ((2, cr.GRAY_Y14), (3, 7), (0, cr.GRAY_Y14)):
        with raw_format(engine, ch, s):
            assert engine.get_raw_format() == (ch, s)              # stored as given
            for call in (lambda: engine.match(col, colr) if ch == 3 else engine.match(left, right),
                         lambda: engine.match_device(dl.data_ptr(), dr.data_ptr(), w, h, 3 * w, out.data_ptr(), w)):
                with pytest.raises(pkg.SGMError) as e:
                    call()
                assert e.value.code == pkg.SGM_ERR_PARAM, str(e.value)
    assert engine.get_raw_format() == (1, cr.GRAY_Y14)
    assert np.array_equal(engine.match(left, right), before)       # the workspace is laid out again
    assert np.array_equal(engine.match_tiled(left, right, 1, 0, devices=[0]), before)


# ----------------------------------------------------------- 6. node-level functions
@pytest.mark.parametrize("mode", ["census", "bm"])
def test_process_disparity_gray_on_device(pkg, synth, mode):
    """process_disparity(gray_on_device=True) on a colour pair equals the host-converted default,
    field for field (a melodic matcher: both sides use the 14-bit set), and with a 4.x compat
    setting the device path takes the 15-bit set."""
    h, w = 64, 160
    left, right = cr.color_pair(synth, h, w, 9, 64, seed=31)
    cr.check_discriminating(left)
    m = pkg.MatcherHIPSGM(" ", (w, h), mode=pkg.MODE_CENSUS8 if mode == "census" else pkg.MODE_OCV_BM)
    pkg.update_matcher(m, pkg.NODE_DEFAULTS)
    m.params.ocv_compat = pkg.COMPAT_MELODIC
    host = pkg.process_disparity(m, left, right, 712.5, 0.119, 0.5, 20.0)
    dev = pkg.process_disparity(m, left, right, 712.5, 0.119, 0.5, 20.0, gray_on_device=True)
    assert host is not None and dev is not None and set(host) == set(dev)
    for k in host:
        if k == "image":
            assert np.array_equal(host[k].view(np.uint32), dev[k].view(np.uint32))
            assert (host[k] != pkg.MISSING_Z).mean() > 0.3
        else:
            assert host[k] == dev[k], k
    m.params.ocv_compat = pkg.COMPAT_NOETIC
    dev15 = pkg.process_disparity(m, left, right, 712.5, 0.119, 0.5, 20.0, gray_on_device=True)
    host15 = pkg.process_disparity(m, pkg.bgr2gray(left, pkg.GRAY_Y15), pkg.bgr2gray(right, pkg.GRAY_Y15), 712.5, 0.119,
                                   0.5, 20.0)
    assert np.array_equal(dev15["image"].view(np.uint32), host15["image"].view(np.uint32))
    m._engine.close()


# ----------------------------------------------------------- 7. the whole chain
def test_raw_colour_to_cloud_chain(engine, oracle, pkg, synth):
    """Raw colour -> sgm_match_device_batch_rect -> sgm_disparity_to_msg -> sgm_depth_points with
    the rectified colour image: the cloud's xyz and packed rgba equal the host chain's."""
    torch = pytest.importorskip("torch")
    from test_depth_oracle import _q
    name, s = "200x70", cr.GRAY_Y14
    rh, rw, h, w, m, D, seed = RECT_CASES[name]
    maps, frames, rect = _rect_setup(oracle, synth, name)
    engine.set_params(pkg.default_params(pkg.MODE_CENSUS8, min_disparity=m, num_disparities=D))
    dm = [_dev(torch, a) for mp in maps for a in mp]
    dl, dr = _dev(torch, frames[0][0]), _dev(torch, frames[0][1])
    disp = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    recl = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    msg = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    pts = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    f, T, zmin, zmax = 712.5, 0.119, 0.5, 100.0
    lo, hi = np.float32(T * f / zmax), np.float32(T * f / zmin)
    Q = oracle.calc_q(*_q())
    torch.cuda.synchronize()
    try:
        with raw_format(engine, 3, s):
            engine.set_rectification((dm[0].data_ptr(), dm[1].data_ptr()), (dm[2].data_ptr(), dm[3].data_ptr()), w, rw, rh)
            engine.match_device_batch_rect([dl.data_ptr()], [dr.data_ptr()], w, h, 3 * rw, [recl.data_ptr()], None, 3 * w,
                                           [disp.data_ptr()], w)
            engine.disparity_to_msg(disp.data_ptr(), w, w, h, lo, hi, msg.data_ptr(), w)
            engine.depth_points(msg.data_ptr(), w, w, h, pkg.q_terms(Q), zmin, zmax, recl.data_ptr(), 3 * w, 3,
                                depth.data_ptr(), w, pts.data_ptr(), h * w, cnt.data_ptr())
            engine.synchronize()
    finally:
        engine.set_rectification()
    el = rect[0][0]
    rm = oracle.disparity_to_msg(_rect_ref(oracle, pkg, synth, name, 0, 8, s), lo, hi)
    rd, rp, rr = oracle.depth_points(rm, Q, zmin, zmax, el)
    k = int(cnt.item())
    got = pts[:k].cpu().numpy()
    assert k == len(rp) and k > 0.2 * h * w
    assert np.array_equal(recl.cpu().numpy(), el)
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(got[:, :3].copy().view(np.uint32), rp.view(np.uint32))
    assert np.array_equal(got[:, 3].copy().view(np.uint32), rr)
    assert len(np.unique(rr)) > 50                                  # real colours, not one grey
