"""GPU parity of sgm_node_frame (the node's imageCb in one host call) through Engine.node_frame,
image_cb_host and the C++ adapter core's MatcherCore::imageCb: every output equals, bit for bit over
the whole array, what today's pieces give: the Python image_cb (sgm_rectify_map, the rectified
outputs of sgm_match_device_batch_rect, sgm_disparity_to_msg) and disp_info_to_depth.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_reference as cr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402
from test_gpu_rect_modes import _dev, _mode, diff_msg, raw_input  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_frame_test")
H, W, F, T = 96, 224, 712.5, 0.119


def same_f32(got, ref, what):
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape, what
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), what + ": " + diff_msg(got, ref)


def same_msg(a, b):
    assert a is not None and b is not None and set(a) == set(b)
    for k in a:
        if k == "image":
            same_f32(a[k], b[k], "msg image")
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


def valid_share(pkg, img, params):
    """test_image_cb's guard: neither outside the depth window nor the matcher's invalid value."""
    return float(((img != pkg.MISSING_Z) & (img != params.min_disparity - 1)).mean())


def node_matcher(pkg, mode, interp=False, census_paths=None):
    m = pkg.MatcherHIPSGM(" ", (W, H), mode=_mode(pkg, mode), census_paths=census_paths)
    pkg.update_matcher(m, dict(pkg.NODE_DEFAULTS, interp=interp))       # the node defaults of the mode
    return m


class shared_matcher:
    """A matcher on the suite's shared engine with parameters set directly; on exit the engine's raw
    format and rectification are back at their defaults, as raw_input leaves them."""

    def __init__(self, pkg, engine, mode, **kw):
        self.m = pkg.MatcherHIPSGM(" ", (W, H), mode=_mode(pkg, mode), census_paths=8)
        self.m.params = pkg.default_params(_mode(pkg, mode), **kw)
        self.m.bm_params = pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE)
        self.m._engine = engine
        self.engine = engine

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.engine.set_rectification()
        self.engine.set_raw_format(1, cr.GRAY_Y14)
        self.engine.set_profiling(False)


def window(f, T, zmin, zmax):
    with np.errstate(divide="ignore"):
        return np.float32(T * f / zmax), (np.float32(T * f / zmin) if zmin != 0 else np.float32(np.inf))


# ------------------------------------------------------------------------- 1. parity with image_cb
@pytest.mark.parametrize("mode,ch,paths", [("bm", 1, 8), ("bm", 3, 8), ("sgbm5", 1, 8), ("sgbm5", 3, 8), ("hh8", 1, 8),
                                           ("hh8", 3, 8), ("census", 1, 8), ("census", 3, 8), ("census", 1, 4),
                                           ("census", 3, 4)])
def test_parity_with_image_cb(pkg, synth, mode, ch, paths):
    """Two frames, a changed K, a changed size: image_cb_host equals image_cb in both rectified images
    and every msg field; the cached maps are built 1, 1, 2 and 3 times."""
    pytest.importorskip("torch")
    zmin, zmax = 0.5, 20.0
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    m = node_matcher(pkg, mode, census_paths=paths)
    state, ref_state = {}, {}
    try:
        for k in range(2):
            raw = rm.raw_frames(synth, H, W, 9, 64, 31 + k, ch)
            ref = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, zmin, zmax, ref_state)
            got = pkg.image_cb_host(m, raw[0], raw[1], infos[0], dict(zip("KDRP", infos[1])), F, T, zmin, zmax, state)
            assert ref is not None and got is not None
            assert np.array_equal(got[0], ref[0]), "rectified left: " + diff_msg(got[0], ref[0])
            assert np.array_equal(got[1], ref[1]), "rectified right: " + diff_msg(got[1], ref[1])
            assert not np.array_equal(ref[0], raw[0])
            same_msg(got[2], ref[2])
            share = valid_share(pkg, ref[2]["image"], m.params)
            print(mode, ch, paths, "frame", k, "valid share", share)
            assert share > 0.2
            assert state["map_builds"] == 1
        K2 = infos[0][0].copy()
        K2[0, 2] += 1.5
        info2 = (K2,) + tuple(infos[0][1:])
        ref = pkg.image_cb(m, raw[0], raw[1], info2, infos[1], F, T, zmin, zmax, ref_state)
        got = pkg.image_cb_host(m, raw[0], raw[1], info2, infos[1], F, T, zmin, zmax, state)
        assert state["map_builds"] == 2
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        same_msg(got[2], ref[2])
        # the same calibration bytes at another size: one more build
        small = rm.raw_frames(synth, 64, 160, 9, 64, 33, ch)
        ref = pkg.image_cb(m, small[0], small[1], info2, infos[1], F, T, zmin, zmax, ref_state)
        got = pkg.image_cb_host(m, small[0], small[1], info2, infos[1], F, T, zmin, zmax, state)
        assert state["map_builds"] == 3
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        same_msg(got[2], ref[2])
    finally:
        m._engine.close()


# ---------------------------------------------------------------------------- 2. strides and padding
@pytest.mark.parametrize("mode", ["sgbm5", "bm", "census"])
def test_strides_and_padding(engine, pkg, synth, mode):
    """203x70 colour, minD -8, every buffer with its own padded stride and pre-filled with sentinels:
    the images equal image_cb's, the padding is unchanged, a NULL rect_right writes nothing."""
    pytest.importorskip("torch")
    h, w = 70, 203
    infos = [calib(seed=11, w=w, h=h), calib(seed=12, w=w, h=h)]
    raw = rm.raw_frames(synth, h, w, -8, 64, 16, 3)
    lo, hi = window(F, T, 0.0, 20.0)
    with shared_matcher(pkg, engine, mode, **rm.case_kw("203x70", mode)) as m:
        ref = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, 0.0, 20.0)
        assert ref is not None
        rawbuf = np.full((2, h, 3 * w + 5), 201, np.uint8)
        rectbuf = np.full((2, h, 3 * w + 7), 99, np.uint8)
        dispbuf = np.full((h, w + 3), -7.5, np.float32)
        views = [rawbuf[i, :, :3 * w].reshape(h, w, 3) for i in range(2)]
        for v, r in zip(views, raw):
            v[...] = r
        assert views[0].base is not None and views[0].strides == (3 * w + 5, 3, 1)
        rv = [rectbuf[i, :, :3 * w].reshape(h, w, 3) for i in range(2)]
        for want_right in (True, False):
            rectbuf[...] = 99
            dispbuf[...] = -7.5
            out = engine.node_frame(views[0], views[1], infos[0], infos[1], lo, hi, rect_left=rv[0],
                                    rect_right=rv[1] if want_right else None, disparity=dispbuf[:, :w])
            assert out[0] is rv[0] and out[2].base is dispbuf
            assert np.array_equal(rv[0], ref[0]), diff_msg(rv[0], ref[0])
            assert (rectbuf[:, :, 3 * w:] == 99).all(), "the padding of a rectified image was written"
            if want_right:
                assert np.array_equal(rv[1], ref[1]), diff_msg(rv[1], ref[1])
            else:
                assert out[1] is None and (rectbuf[1] == 99).all(), "a rectified image that was not requested was written"
            same_f32(np.ascontiguousarray(dispbuf[:, :w]), ref[2]["image"], "disparity")
            assert (dispbuf[:, w:] == np.float32(-7.5)).all(), "the padding of the disparity image was written"
            assert (rawbuf[:, :, 3 * w:] == 201).all()


# -------------------------------------------------------------------------------- 3. WTA-written rows
def _stages(engine):
    return [s[0] for s in engine.stage_times()]


@pytest.mark.parametrize("ch,paths", [(1, 8), (3, 4)])
def test_wta_written_rows(engine, pkg, synth, ch, paths):
    """Census without median and speckle filter: into a registered buffer the final WTA launch writes
    the DisparityImage rows (no `msg` stage), into an unregistered one the tail kernel does (one `msg`
    stage); both equal image_cb. With a median the tail kernel runs for the registered buffer too."""
    pytest.importorskip("torch")
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    raw = rm.raw_frames(synth, H, W, 9, 64, 31, ch)
    lo, hi = window(F, T, 0.5, 20.0)
    for median in (0, 1):
        with shared_matcher(pkg, engine, "census", min_disparity=9, num_disparities=64, median=median) as m:
            m.census_paths = paths
            ref = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, 0.5, 20.0)
            assert ref is not None and valid_share(pkg, ref[2]["image"], m.params) > 0.2
            buf = np.full((H, W + 5), -3.0, np.float32)
            engine.host_register(buf)
            try:
                engine.set_profiling(True)
                out = engine.node_frame(raw[0], raw[1], infos[0], infos[1], lo, hi, disparity=buf[:, :W])
                reg_stages = _stages(engine)
                reg = np.array(buf[:, :W])
                assert (buf[:, W:] == np.float32(-3.0)).all()
            finally:
                engine.set_profiling(False)
                engine.host_unregister(buf)
            assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
            same_f32(reg, ref[2]["image"], "registered rows")
            assert ("msg" in reg_stages) == bool(median), reg_stages
            buf[...] = -3.0
            engine.set_profiling(True)
            engine.node_frame(raw[0], raw[1], infos[0], infos[1], lo, hi, disparity=buf[:, :W])
            stages = _stages(engine)
            launches = engine.stage_launches()
            msg_bytes = dict((s[0], s[2]) for s in engine.stage_times()).get("msg")
            engine.set_profiling(False)
            same_f32(np.array(buf[:, :W]), reg, "unregistered rows")
            assert stages.count("msg") == 1 and launches["msg"] == 1, stages
            # the byte basis of `msg`: 2 B/px read, 4 B/px per float image written
            assert msg_bytes == 6.0 * W * H


# ------------------------------------------------------------------------------------------ 4. depth
def _depth_case(pkg, engine, m, raw, infos, zmin, zmax, dwin, registered=False):
    """node_frame with depth against disp_info_to_depth on image_cb's msg image. dwin: the depth
    window (the node uses zmin / zmax; a narrower one cuts points at both ends)."""
    ref = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, zmin, zmax)
    assert ref is not None
    Q = pkg.calc_q(infos[0][0], infos[1][3], infos[0][3])
    ref_depth = pkg.disp_info_to_depth(engine, ref[2]["image"], None, Q, dwin[0], dwin[1], gen_point_cloud=False)[0]
    lo, hi = window(F, T, zmin, zmax)
    assert float(hi) == ref[2]["max_disparity"] and float(lo) == ref[2]["min_disparity"]
    disp = np.full((H, W), -1.0, np.float32)
    depth = np.full((H, W + 2), -2.0, np.float32)
    if registered:
        engine.host_register(disp)
    try:
        engine.set_profiling(True)
        out = engine.node_frame(raw[0], raw[1], infos[0], infos[1], lo, hi, disparity=disp, depth=depth[:, :W],
                                q5=pkg.q_terms(Q), depth_min=dwin[0], depth_max=dwin[1])
        stages = dict((s[0], s[2]) for s in engine.stage_times())
    finally:
        engine.set_profiling(False)
        if registered:
            engine.host_unregister(disp)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
    same_f32(disp, ref[2]["image"], "disparity")
    same_f32(np.array(depth[:, :W]), ref_depth, "depth")
    assert (depth[:, W:] == np.float32(-2.0)).all()
    return ref[2]["image"], ref_depth, stages


@pytest.mark.parametrize("mode", ["bm", "census"])
def test_depth(engine, pkg, synth, mode):
    pytest.importorskip("torch")
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    raw = rm.raw_frames(synth, H, W, 9, 64, 31, 1)
    kw = dict(min_disparity=9, num_disparities=64)
    if mode == "bm":
        kw = rm.mode_kw("bm", 9, 64, block=15, speckle=True)
    with shared_matcher(pkg, engine, mode, **kw) as m:
        # the node's own window: every point of the msg image is inside it
        _, full, stages = _depth_case(pkg, engine, m, raw, infos, 0.05, 100.0, (0.05, 100.0))
        assert stages["msg"] == 10.0 * W * H                       # 2 read, two float images written
        z = full[full > 0]
        assert z.size > 0.2 * W * H
        # a window that cuts points at both ends
        # (the matcher's invalid value minD - 1 is a point too, the farthest: the quartiles of the rest)
        near = z[z < z.max()]
        zlo, zhi = float(np.quantile(near, 0.25)), float(np.quantile(near, 0.75))
        assert (z < zlo).any() and (z > zhi).any()
        _, cut, _ = _depth_case(pkg, engine, m, raw, infos, 0.05, 100.0, (zlo, zhi))
        kept = cut[cut > 0]
        assert 0 < kept.size < z.size and kept.min() >= zlo and kept.max() <= zhi
        # depth_min 0: the Q8 rule, max_disparity = +inf
        img, _, _ = _depth_case(pkg, engine, m, raw, infos, 0.0, 100.0, (0.0, 100.0))
        assert window(F, T, 0.0, 100.0)[1] == np.inf and (img != pkg.MISSING_Z).any()


def test_depth_with_wta_written_rows(engine, pkg, synth):
    """Census rows written by the WTA into a registered buffer, with depth requested: the depth comes
    from one pass over the device int16 image (a `msg` launch that writes one float image)."""
    pytest.importorskip("torch")
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    raw = rm.raw_frames(synth, H, W, 9, 64, 32, 3)
    with shared_matcher(pkg, engine, "census", min_disparity=9, num_disparities=64) as m:
        _, full, stages = _depth_case(pkg, engine, m, raw, infos, 0.05, 100.0, (0.05, 100.0), registered=True)
        assert stages["msg"] == 6.0 * W * H and (full > 0).mean() > 0.2
        _, _, stages = _depth_case(pkg, engine, m, raw, infos, 0.05, 100.0, (0.2, 0.6), registered=True)
        assert stages["msg"] == 6.0 * W * H


# ------------------------------------------------------------------------------------------ 5. state
@pytest.mark.parametrize("mode", ["sgbm5", "census"])
def test_callers_rectification_state_survives(engine, oracle, pkg, synth, mode):
    """With the caller's sgm_set_rectification on, a match_device on a raw frame after node_frame
    still goes through the caller's maps; with it off, a host match on a rectified pair still runs."""
    torch = pytest.importorskip("torch")
    name = "130x41"
    rh, rw, h, w, _, _, _ = rm.CASES[name]
    if mode == "census":
        maps, frames, rect = rm.setup(oracle, synth, name, 1)
        from conftest import to_oracle_params
        kw = rm.case_kw(name, "census")
        ref = oracle.match(to_oracle_params(oracle, pkg.default_params(pkg.MODE_CENSUS8, **kw)),
                           np.ascontiguousarray(rect[0][0]), np.ascontiguousarray(rect[0][1]))
    else:
        maps, frames, rect = rm.setup(oracle, synth, name, 1)
        kw = rm.case_kw(name, mode)
        ref = rm.reference(oracle, synth, name, mode, 1, 0, 0)
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    raw = rm.raw_frames(synth, H, W, 0, 32, 31, 1)
    lo, hi = window(F, T, 0.5, 20.0)
    dm = [_dev(torch, a) for mp in maps for a in mp]
    dl, dr = _dev(torch, frames[0][0]), _dev(torch, frames[0][1])
    out = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    try:
        engine.set_params(pkg.default_params(_mode(pkg, mode), **kw))
        engine.set_census_paths(8)
        with raw_input(engine, 1, cr.GRAY_Y14, dm, w, rw, rh):
            first = engine.node_frame(raw[0], raw[1], infos[0], infos[1], lo, hi)
            engine.match_device(dl.data_ptr(), dr.data_ptr(), w, h, rw, out.data_ptr(), w)
            engine.synchronize()
            assert np.array_equal(out.cpu().numpy(), ref), diff_msg(out.cpu().numpy(), ref)
            # a failing call leaves it on as well
            with pytest.raises(pkg.SGMError):
                engine.node_frame(raw[0], raw[1], (infos[0][0], [0.1, 0.2, 0.3], None, infos[0][3]), infos[1], lo, hi)
            out.zero_()
            torch.cuda.synchronize()
            engine.match_device(dl.data_ptr(), dr.data_ptr(), w, h, rw, out.data_ptr(), w)
            engine.synchronize()
            assert np.array_equal(out.cpu().numpy(), ref), diff_msg(out.cpu().numpy(), ref)
        # off: the host-buffer match (which refuses rectification) runs, on the rectified pair
        again = engine.node_frame(raw[0], raw[1], infos[0], infos[1], lo, hi)
        same_f32(again[2], first[2], "disparity")
        got = engine.match(np.array(rect[0][0]), np.array(rect[0][1]))
        assert np.array_equal(got, ref), diff_msg(got, ref)
    finally:
        engine.set_rectification()
        engine.set_raw_format(1, cr.GRAY_Y14)


# ---------------------------------------------------------------------------------------- 6. failure
def test_failures_touch_no_output(engine, pkg, synth):
    pytest.importorskip("torch")
    infos = [calib(seed=11, w=W, h=H), calib(seed=12, w=W, h=H)]
    raw = rm.raw_frames(synth, H, W, 9, 64, 31, 1)
    lo, hi = window(F, T, 0.5, 20.0)
    Q = pkg.calc_q(infos[0][0], infos[1][3], infos[0][3])
    with shared_matcher(pkg, engine, "sgbm5", **rm.mode_kw("sgbm5", 9, 64)) as m:
        ref = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, 0.5, 20.0)
        rl, rr = np.full((H, W), 77, np.uint8), np.full((H, W), 78, np.uint8)
        disp, depth = np.full((H, W), -5.0, np.float32), np.full((H, W), -6.0, np.float32)

        def call(il=infos[0], ir=infos[1]):
            return engine.node_frame(raw[0], raw[1], il, ir, lo, hi, rect_left=rl, rect_right=rr, disparity=disp,
                                     depth=depth, q5=pkg.q_terms(Q), depth_min=0.5, depth_max=20.0)

        def untouched():
            return (rl == 77).all() and (rr == 78).all() and (disp == np.float32(-5.0)).all() and \
                (depth == np.float32(-6.0)).all()

        builds = engine.node_frame_map_builds()
        engine.set_params(pkg.default_params(pkg.MODE_OCV_SGBM5, **rm.mode_kw("sgbm5", 9, 24)))
        with pytest.raises(pkg.SGMError) as e:
            call()
        assert e.value.code == pkg.SGM_ERR_PARAM and untouched()
        engine.set_params(m.params)
        # a three-element distortion vector: sgm_rectify_map's refusal
        with pytest.raises(pkg.SGMError) as e:
            call(il=(infos[0][0], [0.1, 0.2, 0.3], infos[0][2], infos[0][3]))
        assert e.value.code == pkg.SGM_ERR_UNSUPPORTED and untouched()
        # a singular P[:, :3] * R
        with pytest.raises(pkg.SGMError) as e:
            call(ir=(infos[1][0], infos[1][1], infos[1][2], np.zeros((3, 4))))
        assert e.value.code == pkg.SGM_ERR_ARG and untouched()
        # a short struct_size, through the C ABI itself
        io = pkg.NodeFrameIO()
        io.struct_size = ctypes.sizeof(pkg.NodeFrameIO) - 8
        io.raw_left, io.raw_right, io.raw_stride, io.width, io.height = raw[0].ctypes.data, raw[1].ctypes.data, W, W, H
        io.min_disparity, io.max_disparity = float(lo), float(hi)
        io.disparity, io.disparity_stride = disp.ctypes.data, W
        cl, cr_ = pkg.CameraInfo.of(infos[0]), pkg.CameraInfo.of(infos[1])
        lib = pkg.load_library()
        assert lib.sgm_node_frame(engine.h, ctypes.byref(cl), ctypes.byref(cr_), ctypes.byref(io)) == pkg.SGM_ERR_ARG
        io.struct_size = ctypes.sizeof(pkg.NodeFrameIO)
        io.disparity_stride = W - 1                                 # a stride smaller than a row
        assert lib.sgm_node_frame(engine.h, ctypes.byref(cl), ctypes.byref(cr_), ctypes.byref(io)) == pkg.SGM_ERR_ARG
        io.disparity_stride, io.disparity = W, None                 # a required pointer
        assert lib.sgm_node_frame(engine.h, ctypes.byref(cl), ctypes.byref(cr_), ctypes.byref(io)) == pkg.SGM_ERR_ARG
        assert untouched()
        # none of them built maps, and the next valid call is correct
        assert engine.node_frame_map_builds() == builds
        call()
        assert np.array_equal(rl, ref[0]) and np.array_equal(rr, ref[1])
        same_f32(disp, ref[2]["image"], "disparity after the failures")
        ref_depth = pkg.disp_info_to_depth(engine, ref[2]["image"], None, Q, 0.5, 20.0, gen_point_cloud=False)[0]
        same_f32(depth, ref_depth, "depth after the failures")


# ---------------------------------------------------------------------------------------- 7. adapter
_frames = {}


def driver_frame(ch):
    """plugin_frame_test's generated raw pair (the same 32-bit LCG)."""
    if ch not in _frames:
        NW, NH = W + 32, H + 1
        s, vals = 7331, np.empty(ch * NH * NW, np.int32)
        for i in range(vals.size):
            s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
            vals[i] = s >> 24
        N = vals.reshape(ch, NH, NW)
        B = (N[:, :-1, :-1] + N[:, :-1, 1:] + N[:, 1:, :-1] + N[:, 1:, 1:] + 2) >> 2     # ch x H x (NW - 1)
        L = B[:, :, :W]
        R = np.stack([np.stack([B[c, y, 20 + y // 16:20 + y // 16 + W] for y in range(H)]) for c in range(ch)])
        pair = [np.ascontiguousarray(np.moveaxis(a, 0, -1).astype(np.uint8)) for a in (L, R)]
        if ch == 1:
            pair = [a[:, :, 0].copy() for a in pair]
        for a in pair:
            a.setflags(write=False)
        _frames[ch] = pair
    return _frames[ch]


def driver_calib():
    """plugin_frame_test's two CameraInfos."""
    K = np.array([201.6, 0, 115.3, 0, 203.616, 45.9, 0, 0, 1]).reshape(3, 3)
    D = np.array([-0.21, 0.07, 0.0012, -0.0009, -0.011])
    R = np.array([0.99995, -0.008, 0.006, 0.00806, 0.99992, -0.0095, -0.00592, 0.00955, 0.99994]).reshape(3, 3)
    P = np.array([197.568, 0, 107.0, -24.192, 0, 197.568, 49.5, 0, 0, 0, 1, 0]).reshape(3, 4)
    Pl, Kr, Dr = P.copy(), K.copy(), D.copy()
    Pl[0, 3] = 0.0
    Kr[0, 2] += 0.75
    Dr[0] += 0.01
    return (K, D, R, Pl), (Kr, Dr, R, P)


def fnv1a(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


@pytest.mark.parametrize("mode,ch,interp", [("bm", 1, 0), ("sgbm5", 3, 1), ("census", 1, 0)])
def test_adapter_core_image_cb(pkg, mode, ch, interp):
    """MatcherCore::imageCb on the driver's generated pair and calibration: its checksums are those
    of the Python image_cb (interp: the right matcher on (right, left), a negative window)."""
    pytest.importorskip("torch")
    r = subprocess.run([DRIVER, "frame", mode, str(ch), str(interp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "frame ok", r.stdout
    zmin, zmax = (-20.0, -0.5) if interp else (0.5, 20.0)
    raw, infos = [np.array(a) for a in driver_frame(ch)], driver_calib()
    m = node_matcher(pkg, mode, interp=bool(interp))
    try:
        ref = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, zmin, zmax)
        assert ref is not None
        lo, hi = window(F, T, zmin, zmax)
        assert lines[0] == "min_disp %08x max_disp %08x" % (lo.view(np.uint32), hi.view(np.uint32))
        assert lines[1] == "rect_left hash " + fnv1a(ref[0])
        assert lines[2] == "rect_right hash " + fnv1a(ref[1])
        assert lines[3] == "disparity hash " + fnv1a(ref[2]["image"])
        used = pkg.right_matcher_params(m.params) if interp else m.params
        share = valid_share(pkg, ref[2]["image"], used)
        print(mode, ch, interp, "valid share", share)
        assert share > 0.2
        # and the Python host entry agrees on the same pair
        got = pkg.image_cb_host(m, raw[0], raw[1], infos[0], infos[1], F, T, zmin, zmax)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        same_msg(got[2], ref[2])
    finally:
        m._engine.close()
