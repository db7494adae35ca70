"""GPU parity of raw frames through the OpenCV and BM modes: sgm_set_rectification ahead of
SGM_MODE_OCV_SGBM5 / OCV_HH8 / OCV_BM (the k_rectify_pair pre-pass of csrc/rectify.hip), through
sgm_match_device_batch_rect, sgm_match_device and the Python image_cb. Every comparison is bit-exact
over the whole image against the references composed in tests/rect_modes_reference.py (checked for
substance on the CPU by tests/test_rect_modes_reference.py).
"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_reference as cr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

pytestmark = pytest.mark.gpu


def _mode(pkg, mode):
    return {"sgbm5": pkg.MODE_OCV_SGBM5, "hh8": pkg.MODE_OCV_HH8, "bm": pkg.MODE_OCV_BM, "census": pkg.MODE_CENSUS8}[mode]


def _dev(torch, a):
    return torch.as_tensor(np.array(a, copy=True)).cuda()       # the cached references are read-only


def diff_msg(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} differ, first {bad[:4].tolist()}"


def _set_mode(engine, pkg, oracle, mode, kw):
    from conftest import to_oracle_params
    p = pkg.default_params(_mode(pkg, mode), **kw)
    if mode != "bm":      # the references' parameters are the engine's, through the suite's own translation
        assert to_oracle_params(oracle, p).as_dict() == oracle.make_params(rm.MODE_ID[mode], **kw).as_dict()
    engine.set_params(p)
    engine.set_census_paths(8)
    engine.set_bm_params(pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE))
    return p


@contextlib.contextmanager
def raw_input(engine, ch, s, dm, map_stride, rw, rh):
    """Raw format and rectification on the shared engine; both always go back to their defaults."""
    engine.set_raw_format(ch, s)
    try:
        engine.set_rectification((dm[0].data_ptr(), dm[1].data_ptr()), (dm[2].data_ptr(), dm[3].data_ptr()), map_stride,
                                 rw, rh)
        yield
    finally:
        engine.set_rectification()
        engine.set_raw_format(1, cr.GRAY_Y14)


def _batch(torch, engine, maps, frames, h, w, ch, s, want_l=True, want_r=True, single=False):
    """One sgm_match_device_batch_rect (or sgm_match_device) call on raw frames with pre-filled,
    padded outputs. Returns (disparities n x h x w, rectified left, right: n x h x w [x 3] or None)."""
    n = len(frames)
    rh, rw = frames[0][0].shape[:2]
    dm = [_dev(torch, a) for mp in maps for a in mp]
    dl = [_dev(torch, f[0]) for f in frames]
    dr = [_dev(torch, f[1]) for f in frames]
    out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
    rs = w * ch + 7
    recl = torch.full((n, h, rs), 99, dtype=torch.uint8, device="cuda")
    recr = torch.full((n, h, rs), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with raw_input(engine, ch, s, dm, w, rw, rh):
        if single:
            engine.match_device(dl[0].data_ptr(), dr[0].data_ptr(), w, h, rw * ch, out[0].data_ptr(), w)
        else:
            engine.match_device_batch_rect([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, rw * ch,
                                           [recl[i].data_ptr() for i in range(n)] if want_l else None,
                                           [recr[i].data_ptr() for i in range(n)] if want_r else None,
                                           rs, [out[i].data_ptr() for i in range(n)], w)
        engine.synchronize()
    res = []
    for buf, want in ((recl.cpu().numpy(), want_l and not single), (recr.cpu().numpy(), want_r and not single)):
        if want:
            assert (buf[:, :, w * ch:] == 99).all(), "the padding of a rectified image was written"
            res.append(buf[:, :, :w * ch].reshape((n, h, w, 3) if ch == 3 else (n, h, w)))
        else:
            assert (buf == 99).all(), "a rectified image that was not requested was written"
            res.append(None)
    return out.cpu().numpy(), res[0], res[1]


def _run_case(torch, engine, pkg, oracle, synth, name, mode, n, ch, s, speckle=False, **kw):
    rh, rw, h, w, m, D, _ = rm.CASES[name]
    maps, frames, rect = rm.setup(oracle, synth, name, ch)
    _set_mode(engine, pkg, oracle, mode, rm.case_kw(name, mode, speckle))
    got, gl, gr = _batch(torch, engine, maps, frames[:n], h, w, ch, s, **kw)
    for i in range(n):
        ref = rm.reference(oracle, synth, name, mode, ch, s, i, speckle)
        assert np.array_equal(got[i], ref), f"frame {i} disparity: " + diff_msg(got[i], ref)
        for g, side in ((gl, 0), (gr, 1)):
            if g is not None:
                assert np.array_equal(g[i], rect[i][side]), f"frame {i} rectified {'LR'[side]}: " + diff_msg(g[i], rect[i][side])
    return got


# ------------------------------------------------------------------------------ 1. raw mono batch
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("name", list(rm.CASES))
@pytest.mark.parametrize("mode", rm.MODES)
def test_raw_mono_batch(engine, oracle, pkg, synth, mode, name, n):
    """n = 5 wraps the four OCV lanes: frame 4 runs on lane 0 again."""
    torch = pytest.importorskip("torch")
    _run_case(torch, engine, pkg, oracle, synth, name, mode, n, 1, cr.GRAY_Y14)


@pytest.mark.parametrize("mode", ["sgbm5", "bm"])
def test_raw_mono_batch_with_the_nodes_speckle_filter(engine, oracle, pkg, synth, mode):
    torch = pytest.importorskip("torch")
    _run_case(torch, engine, pkg, oracle, synth, "203x70", mode, 2, 1, cr.GRAY_Y14, speckle=True)


# ---------------------------------------------------------------------------- 2. raw colour batch
@pytest.mark.parametrize("s", [cr.GRAY_Y14, cr.GRAY_Y15], ids=["Y14", "Y15"])
@pytest.mark.parametrize("name", list(rm.CASES))
@pytest.mark.parametrize("mode", rm.MODES)
def test_raw_colour_batch(engine, oracle, pkg, synth, mode, name, s):
    """Rectified 8UC3 = remap3(raw), disparities = the mode on gray(remap3(raw))."""
    torch = pytest.importorskip("torch")
    _run_case(torch, engine, pkg, oracle, synth, name, mode, 2, 3, s)


# ------------------------------------------------------------- 3. rectified outputs are optional
@pytest.mark.parametrize("want_l,want_r", [(True, False), (False, True), (False, False)], ids=["L", "R", "none"])
@pytest.mark.parametrize("mode,ch", [("sgbm5", 3), ("bm", 1)])
def test_rectified_outputs_are_optional(engine, oracle, pkg, synth, mode, ch, want_l, want_r):
    torch = pytest.importorskip("torch")
    _run_case(torch, engine, pkg, oracle, synth, "130x41", mode, 3, ch, cr.GRAY_Y14, want_l=want_l, want_r=want_r)


# ------------------------------------------------------------------ 4. the single-frame entry point
@pytest.mark.parametrize("ch", [1, 3], ids=["mono", "colour"])
@pytest.mark.parametrize("mode", ["hh8", "bm"])
def test_match_device_takes_raw_frames(engine, oracle, pkg, synth, mode, ch):
    torch = pytest.importorskip("torch")
    name, s = "203x70", cr.GRAY_Y15
    _run_case(torch, engine, pkg, oracle, synth, name, mode, 1, ch, s, single=True)
    if ch == 3:                                   # a colour stride given in pixels is too short
        rh, rw, h, w = rm.CASES[name][:4]
        maps, frames, _ = rm.setup(oracle, synth, name, 3)
        dm = [_dev(torch, a) for mp in maps for a in mp]
        dl, dr = _dev(torch, frames[0][0]), _dev(torch, frames[0][1])
        out = torch.zeros((h, w), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        with raw_input(engine, 3, s, dm, w, rw, rh):
            with pytest.raises(pkg.SGMError) as e:
                engine.match_device(dl.data_ptr(), dr.data_ptr(), w, h, rw, out.data_ptr(), w)
        assert e.value.code == pkg.SGM_ERR_ARG


# ------------------------------------------------------------------------------------ 5. map edges
def _edge_maps(maps, sw, sh):
    """The hand-made entries of test_gpu_color._c3_maps on copies of a case's maps: taps partly and
    wholly outside, negative coordinates, exact 1/64 ties, a NaN and a value beyond the int range."""
    out = []
    for mx, my in maps:
        mx, my = mx.copy(), my.copy()
        mx[0, :8] = [-0.5, -1.25, -4.0, -300.0, sw - 2.5, sw - 0.5, sw + 2.0, sw + 400.0]
        my[0, :8] = 3.0
        my[1, :6] = [-0.5, -2.75, -50.0, sh - 1.5, sh + 1.0, sh + 99.0]
        mx[1, :6] = 7.25
        mx[2] = np.round(mx[2] * 64) / 64 + 1.0 / 64
        my[3] = np.floor(my[3]) + 0.515625
        mx[4, 0], my[4, 1] = np.nan, 1e30
        mx[5:8] -= 0.7 * sw
        my[9:12] += 0.8 * sh
        out.append((mx, my))
    return out


@pytest.mark.parametrize("ch", [1, 3], ids=["mono", "colour"])
def test_map_edges_in_bm_mode(engine, oracle, pkg, synth, ch):
    torch = pytest.importorskip("torch")
    name, s = "130x41", cr.GRAY_Y14
    rh, rw, h, w = rm.CASES[name][:4]
    maps0, frames, _ = rm.setup(oracle, synth, name, ch)
    maps = _edge_maps(maps0, rw, rh)
    kw = rm.case_kw(name, "bm")
    _set_mode(engine, pkg, oracle, "bm", kw)
    got, gl, gr = _batch(torch, engine, maps, frames[:1], h, w, ch, s)
    el, er = rm.rectified(oracle, frames[0][0], *maps[0]), rm.rectified(oracle, frames[0][1], *maps[1])
    assert (el[0, 3] == 0).all() and (el[0, 7] == 0).all()          # wholly outside: 0
    assert np.array_equal(gl[0], el), diff_msg(gl[0], el)
    assert np.array_equal(gr[0], er), diff_msg(gr[0], er)
    ref = rm.match_ref(oracle, "bm", kw, rm.grey_of(el, s), rm.grey_of(er, s))
    assert np.array_equal(got[0], ref), diff_msg(got[0], ref)


# --------------------------------------------------------------------------- 6. unaligned everything
@pytest.mark.parametrize("mode,ch", [("bm", 1), ("hh8", 3)], ids=["mono", "colour"])
def test_unaligned_strides_and_bases(engine, oracle, pkg, synth, mode, ch):
    """Raw stride rw (* 3) + 3, map stride w + 1, an odd rectified stride, out_stride w + 5, and raw
    and rectified base pointers one byte off: the byte paths of every load and store."""
    torch = pytest.importorskip("torch")
    name, s, n = "203x70", cr.GRAY_Y15, 2
    rh, rw, h, w = rm.CASES[name][:4]
    maps, frames, rect = rm.setup(oracle, synth, name, ch)
    _set_mode(engine, pkg, oracle, mode, rm.case_kw(name, mode))
    sstride, mstride, rstride, ostride = rw * ch + 3, w + 1, (w * ch + 7) | 1, w + 5
    assert sstride % 2 == 1 and rstride % 2 == 1

    def padded(img, stride, fill):
        """img rows at `stride` bytes in a flat device buffer that starts one byte off alignment."""
        rows = np.full((img.shape[0], stride), fill, np.uint8)
        flat = img.reshape(img.shape[0], -1)
        rows[:, :flat.shape[1]] = flat
        buf = torch.full((rows.size + 1,), fill, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.as_tensor(rows.ravel()).cuda()
        return buf

    dm = []
    for mp in maps:
        for a in mp:
            m = np.full((h, mstride), 1e9, np.float32)
            m[:, :w] = a
            dm.append(torch.as_tensor(m).cuda())
    dl = [padded(f[0], sstride, 201) for f in frames[:n]]
    dr = [padded(f[1], sstride, 201) for f in frames[:n]]
    recl = [torch.full((h * rstride + 1,), 99, dtype=torch.uint8, device="cuda") for _ in range(n)]
    recr = [torch.full((h * rstride + 1,), 99, dtype=torch.uint8, device="cuda") for _ in range(n)]
    out = torch.full((n, h, ostride), 777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with raw_input(engine, ch, s, dm, mstride, rw, rh):
        engine.match_device_batch_rect([t.data_ptr() + 1 for t in dl], [t.data_ptr() + 1 for t in dr], w, h, sstride,
                                       [t.data_ptr() + 1 for t in recl], [t.data_ptr() + 1 for t in recr], rstride,
                                       [out[i].data_ptr() for i in range(n)], ostride)
        engine.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :, w:] == 777).all()
    for i in range(n):
        ref = rm.reference(oracle, synth, name, mode, ch, s, i)
        assert np.array_equal(got[i, :, :w], ref), f"frame {i} disparity: " + diff_msg(got[i, :, :w], ref)
        for bufs, side in ((recl, 0), (recr, 1)):
            b = bufs[i].cpu().numpy()
            assert b[0] == 99
            rows = b[1:].reshape(h, rstride)
            assert np.array_equal(rows[:, :w * ch].reshape(rect[i][side].shape), rect[i][side]), f"frame {i} rectified"
            assert (rows[:, w * ch:] == 99).all()


# --------------------------------------------------------------------------------- 7. smallest frames
@pytest.mark.parametrize("ch", [1, 3], ids=["mono", "colour"])
@pytest.mark.parametrize("mode,h,w", [("sgbm5", 6, 21), ("hh8", 6, 21), ("bm", 7, 23), ("sgbm5", 6, 19), ("bm", 7, 19),
                                      ("hh8", 6, 17), ("bm", 7, 17)])
def test_smallest_frames(engine, oracle, pkg, synth, mode, h, w, ch):
    """D = 16 with block 3 (OCV) / window 5 (BM) out of a 9 x 24 raw frame; W = 19 and 17 leave 3
    and 1 computed columns and a row tail of 3 and 1 pixels in every store of the pre-pass."""
    torch = pytest.importorskip("torch")
    rh, rw, m, D, s = 9, 24, 0, 16, cr.GRAY_Y14
    maps = [oracle.rectify_map(*calib(seed=11, w=rw, h=rh), w, h), oracle.rectify_map(*calib(seed=12, w=rw, h=rh), w, h)]
    frames = [rm.raw_frames(synth, rh, rw, m, D, 40 + i, ch) for i in range(2)]
    kw = rm.mode_kw(mode, m, D, block=5 if mode == "bm" else 3)
    _set_mode(engine, pkg, oracle, mode, kw)
    got, gl, gr = _batch(torch, engine, maps, frames, h, w, ch, s)
    for i, f in enumerate(frames):
        el, er = rm.rectified(oracle, f[0], *maps[0]), rm.rectified(oracle, f[1], *maps[1])
        assert np.array_equal(gl[i], el) and np.array_equal(gr[i], er), f"frame {i} rectified"
        ref = rm.match_ref(oracle, mode, kw, rm.grey_of(el, s), rm.grey_of(er, s))
        assert np.array_equal(got[i], ref), f"frame {i}: " + diff_msg(got[i], ref)


# ------------------------------------------------------------------- 8. lanes and profiling agree
@pytest.mark.parametrize("mode,ch", [("sgbm5", 3), ("bm", 1)])
def test_lanes_and_profiling_agree(engine, oracle, pkg, synth, mode, ch):
    """n = 5 unprofiled (frames dealt over the lanes) equals n = 5 with profiling on (one frame after
    another on the handle's stream); the pre-pass is a stage named `rectify`, one launch per frame,
    and with colour frames it replaces the `gray` stage."""
    torch = pytest.importorskip("torch")
    name, s, n = "130x41", cr.GRAY_Y14, 5
    h, w = rm.CASES[name][2:4]
    lanes = _run_case(torch, engine, pkg, oracle, synth, name, mode, n, ch, s)
    engine.set_profiling(True)
    try:
        seq = _run_case(torch, engine, pkg, oracle, synth, name, mode, n, ch, s)
        st = {k: b for k, _, b in engine.stage_times()}
        launches = engine.stage_launches()
    finally:
        engine.set_profiling(False)
    assert np.array_equal(lanes, seq)
    assert "rectify" in st and "gray" not in st, st
    assert st["rectify"] == (16 + 2 * ch + 2 + 2 * ch) * w * h, st
    assert launches["rectify"] == n, launches


# ----------------------------------------------------------------------------- 9. the handle recovers
def test_the_handle_recovers(oracle, pkg, synth):
    """One engine: OCV raw match, rectification off and pre-rectified frames, census with
    rectification on, BM raw match. Every switch lays the workspace out again."""
    torch = pytest.importorskip("torch")
    from conftest import to_oracle_params
    name, s = "203x70", cr.GRAY_Y14
    rh, rw, h, w, m, D, _ = rm.CASES[name]
    maps, frames, rect = rm.setup(oracle, synth, name, 1)
    eng = pkg.Engine(0)
    try:
        _run_case(torch, eng, pkg, oracle, synth, name, "sgbm5", 2, 1, s)
        # rectification off: the same handle on the rectified frames
        dl, dr = _dev(torch, rect[0][0]), _dev(torch, rect[0][1])
        out = torch.full((h, w), 777, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.match_device_batch([dl.data_ptr()], [dr.data_ptr()], w, h, w, [out.data_ptr()], w)
        eng.synchronize()
        ref = rm.reference(oracle, synth, name, "sgbm5", 1, s, 0)
        assert np.array_equal(out.cpu().numpy(), ref), diff_msg(out.cpu().numpy(), ref)
        # the census mode rectifies inside its tiles, as before
        p = _set_mode(eng, pkg, oracle, "census", rm.mode_kw("census", m, D))
        got, gl, gr = _batch(torch, eng, maps, frames[:3], h, w, 1, s)
        for i in range(3):
            assert np.array_equal(gl[i], rect[i][0]) and np.array_equal(gr[i], rect[i][1])
            cref = oracle.match(to_oracle_params(oracle, p), np.ascontiguousarray(rect[i][0]), np.ascontiguousarray(rect[i][1]))
            assert np.array_equal(got[i], cref), f"census frame {i}: " + diff_msg(got[i], cref)
        assert (cref != (m - 1) * 16).mean() > 0.3
        _run_case(torch, eng, pkg, oracle, synth, name, "bm", 2, 1, s)
        _run_case(torch, eng, pkg, oracle, synth, "130x41", "hh8", 5, 3, cr.GRAY_Y15)
    finally:
        eng.close()


# ------------------------------------------------------------------------------ 10. pinned refusals
@pytest.mark.parametrize("mode", ["sgbm5", "bm"])
def test_pinned_refusals(engine, oracle, pkg, synth, mode):
    """Host-buffer matches and the device tile entry point still refuse while rectification is on
    (the host tile entry points run on sub-handles of their own, which never see the rectification
    state), and so does a frame without a disparity window."""
    torch = pytest.importorskip("torch")
    name = "130x41"
    rh, rw, h, w = rm.CASES[name][:4]
    maps, frames, rect = rm.setup(oracle, synth, name, 1)
    _set_mode(engine, pkg, oracle, mode, rm.case_kw(name, mode))
    dm = [_dev(torch, a) for mp in maps for a in mp]
    dl, dr = _dev(torch, frames[0][0]), _dev(torch, frames[0][1])
    out = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    gl, gr = np.array(rect[0][0]), np.array(rect[0][1])
    with raw_input(engine, 1, cr.GRAY_Y14, dm, w, rw, rh):
        for call in (lambda: engine.match(gl, gr), lambda: engine.match_f32(gl, gr),
                     lambda: engine.match_tiled_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w, 2, 4,
                                                       devices=[0])):
            with pytest.raises(pkg.SGMError) as e:
                call()
            assert e.value.code == pkg.SGM_ERR_UNSUPPORTED, str(e.value)
        # D = 32 leaves no computed column in a 30-pixel row
        for call in (lambda: engine.match_device(dl.data_ptr(), dr.data_ptr(), 30, 20, rw, out.data_ptr(), 30),
                     lambda: engine.match_device_batch_rect([dl.data_ptr()], [dr.data_ptr()], 30, 20, rw, None, None, 0,
                                                            [out.data_ptr()], 30)):
            with pytest.raises(pkg.SGMError) as e:
                call()
            assert e.value.code == pkg.SGM_ERR_UNSUPPORTED, str(e.value)
        # none of the refusals leaves the handle unable to take the raw frame
        engine.match_device(dl.data_ptr(), dr.data_ptr(), w, h, rw, out.data_ptr(), w)
        engine.synchronize()
    ref = rm.reference(oracle, synth, name, mode, 1, 0, 0)
    assert np.array_equal(out.cpu().numpy(), ref), diff_msg(out.cpu().numpy(), ref)
    assert np.array_equal(engine.match(gl, gr), rm.reference(oracle, synth, name, mode, 1, 0, 0))


# ------------------------------------------------------------------------------------- 11. image_cb
def _same_msg(a, b):
    assert a is not None and b is not None and set(a) == set(b)
    for k in a:
        if k == "image":
            assert a[k].dtype == np.float32 and b[k].dtype == np.float32
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), diff_msg(a[k], b[k])
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


@pytest.mark.parametrize("mode,ch,interp", [("bm", 1, False), ("bm", 3, False), ("sgbm5", 1, False), ("sgbm5", 3, True),
                                            ("census", 1, False), ("census", 3, False), ("bm", 1, True)])
def test_image_cb(engine, pkg, synth, mode, ch, interp):
    """image_cb on raw frames equals rectify() of each image followed by process_disparity on the
    rectified pair, field by field; the maps are computed once per calibration."""
    h, w, f, T, zmin, zmax = 96, 224, 712.5, 0.119, 0.5, 20.0
    if interp:                  # the right matcher's disparities are negative: a window that holds them
        zmin, zmax = -20.0, -0.5
    infos = [calib(seed=11, w=w, h=h), calib(seed=12, w=w, h=h)]
    m = pkg.MatcherHIPSGM(" ", (w, h), mode=_mode(pkg, mode))
    cfg = dict(pkg.NODE_DEFAULTS, interp=interp)
    pkg.update_matcher(m, cfg)                                      # the node defaults of the mode
    state = {}
    try:
        for k in range(2):
            raw = rm.raw_frames(synth, h, w, 9, 64, 31 + k, ch)
            res = pkg.image_cb(m, raw[0], raw[1], infos[0], dict(zip("KDRP", infos[1])), f, T, zmin, zmax, state)
            assert res is not None
            rl, _ = pkg.rectify(engine, raw[0], *infos[0])
            rr, _ = pkg.rectify(engine, raw[1], *infos[1])
            assert not np.array_equal(rl, raw[0])
            assert np.array_equal(res[0], rl) and np.array_equal(res[1], rr)
            ref = pkg.process_disparity(m, rl, rr, f, T, zmin, zmax, gray_on_device=True)
            _same_msg(res[2], ref)
            # a real disparity map: neither outside the depth window nor the matcher's invalid value (the
            # sparsest, BM at the node defaults: bm_reference + the oracle's speckle filter give 0.42 and
            # 0.25 on these two rectified pairs)
            used = pkg.right_matcher_params(m.params) if interp else m.params
            img = ref["image"]
            share = float(((img != pkg.MISSING_Z) & (img != used.min_disparity - 1)).mean())
            print(mode, ch, interp, "frame", k, "valid share", share)
            assert share > 0.2
            assert state["map_builds"] == 1                         # the second frame reuses the maps
        # the engine is left as a host-buffer match needs it: rectification off
        assert pkg.process_disparity(m, rl, rr, f, T, zmin, zmax, gray_on_device=True) is not None
        K2 = infos[0][0].copy()
        K2[0, 2] += 1.5                                             # a changed K recomputes the maps
        res2 = pkg.image_cb(m, raw[0], raw[1], (K2,) + tuple(infos[0][1:]), infos[1], f, T, zmin, zmax, state)
        assert state["map_builds"] == 2
        rl2, _ = pkg.rectify(engine, raw[0], K2, *infos[0][1:])
        assert np.array_equal(res2[0], rl2) and not np.array_equal(rl2, rl) and np.array_equal(res2[1], rr)
        _same_msg(res2[2], pkg.process_disparity(m, rl2, rr, f, T, zmin, zmax, gray_on_device=True))
    finally:
        m._engine.close()


def test_image_cb_reports_a_failed_match(pkg, synth, capsys):
    """Parameters the matcher refuses: nothing is published, as when the node's stereo_match fails."""
    h, w = 48, 96
    m = pkg.MatcherHIPSGM(" ", (w, h), mode=pkg.MODE_OCV_BM)
    pkg.update_matcher(m, dict(pkg.NODE_DEFAULTS, disparity_range=24))        # not a multiple of 16
    raw = rm.raw_frames(synth, h, w, 0, 32, 3, 1)
    info = calib(seed=11, w=w, h=h)
    try:
        assert pkg.image_cb(m, raw[0], raw[1], info, info, 700.0, 0.1, 0.5, 20.0) is None
        assert "Failed to compute stereo match" in capsys.readouterr().err
        assert pkg.process_disparity(m, raw[0], raw[1], 700.0, 0.1, 0.5, 20.0) is None
    finally:
        m._engine.close()
