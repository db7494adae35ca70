"""GPU parity — census windows (sgm_set_census_window) through every census entry point, bit-exact
against the reference composed in tests/census_window_reference.py (numpy codes, cost volume and
path recurrence; the oracle's WTA, median and speckle filter). The shared engine is set back to the
default window after every test."""
import numpy as np
import pytest

import census_window_reference as cwr
from conftest import to_oracle_params
from test_gpu_census_paths import _device_batch

pytestmark = pytest.mark.gpu

WINS4 = [(3, 3, 1), (7, 7, 1), (7, 7, 2), (9, 7, 2)]


@pytest.fixture
def eng(engine):
    try:
        yield engine
    finally:
        engine.set_census_window(*cwr.DEFAULT)
        engine.set_census_paths(8)
        engine.set_raw_format(1)
        engine.set_fill_params(engine.get_fill_params().copy(mode=0))
        engine.set_profiling(False)


def same(got, ref, what=""):
    assert np.array_equal(got, ref), f"{what}: {(np.asarray(got) != np.asarray(ref)).sum()} values differ"


def ref_match(oracle, p, left, right, win, dirs=range(8)):
    return cwr.match(oracle, to_oracle_params(oracle, p), left, right, win, dirs)


# ---- codes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(4, 5), (37, 70), (34, 130)], ids=["5x4", "70x37", "130x34"])
def test_codes_of_all_windows(eng, h, w):
    """5x4: smaller than any window, every tap clamps; 70x37: a partial tile on both axes; 130x34:
    three tile columns, two tile rows. Dense windows also against the default codes AND-ed."""
    img = np.random.default_rng(h * w).integers(0, 256, (h, w), dtype=np.uint8)
    eng.set_census_window(*cwr.DEFAULT)
    base = eng.census(img)
    same(base, cwr.census(img), "default")
    for win in cwr.WINDOWS:
        eng.set_census_window(*win)
        assert eng.get_census_window() == win
        got = eng.census(img)
        same(got, cwr.census(img, win), str(win))
        if win[2] == 1:
            same(got, base & np.uint64(cwr.mask(win[0], win[1])), f"{win} masked")


@pytest.mark.parametrize("win", [(5, 5, 1), (9, 7, 2)], ids=str)
def test_path_volumes(eng, oracle, synth, pkg, win):
    h, w, D = 40, 96, 32
    left, right, _ = synth.stereo_pair(h, w, 0, D, seed=21)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng.set_params(p)
    eng.set_census_window(*win)
    for d in range(8):
        same(eng.census_path(left, right, d), cwr.census_path(oracle, to_oracle_params(oracle, p), left, right, d, win),
             f"dir {d}")


# ---- matches -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(synth):
    out = {}
    for (h, w) in [(40, 96), (56, 144)]:
        for D in (32, 64):
            out[(h, w, D)] = [synth.stereo_pair(h, w, 0, D, seed=900 + D + i)[:2] for i in range(5)]
    return out


@pytest.mark.parametrize("win", WINS4, ids=str)
@pytest.mark.parametrize("minD", [0, 5, -3])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("h,w", [(40, 96), (56, 144)], ids=["96x40", "144x56"])
def test_match(eng, oracle, pkg, frames, h, w, D, minD, win):
    left, right = frames[(h, w, D)][0]
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=minD)
    eng.set_params(p)
    eng.set_census_window(*win)
    same(eng.match(left, right), ref_match(oracle, p, left, right, win), "match")


@pytest.mark.parametrize("win", WINS4, ids=str)
def test_entry_points(eng, oracle, pkg, frames, win):
    """match_f32, match_device, a 5-frame device batch (first, steady and tail groups) with its stage
    names, 4 paths, median + speckles, hole filling, the host batch on two sub-handles."""
    torch = pytest.importorskip("torch")
    h, w, D = 56, 144, 64
    fs = frames[(h, w, D)]
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=5)
    refs = [ref_match(oracle, p, l, r, win) for l, r in fs]
    eng.set_params(p)
    eng.set_census_window(*win)
    left, right = fs[0]
    same(eng.match_f32(left, right), refs[0].astype(np.float32), "match_f32")
    dl, dr = torch.from_numpy(np.array(left)).cuda(), torch.from_numpy(np.array(right)).cuda()
    out = torch.full((h, w + 3), 1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.match_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w + 3)
    eng.synchronize()
    same(out.cpu().numpy()[:, :w], refs[0], "match_device")
    eng.set_profiling(True)
    got = _device_batch(torch, eng, fs, h, w, pad_in=3, pad_out=5)
    launches = eng.stage_launches()
    eng.set_profiling(False)
    for i in range(5):
        same(got[i], refs[i], f"batch frame {i}")
    assert launches["census_win"] == 3 and not any("census" in k and k != "census_win" for k in launches), launches
    assert launches["paths7"] == 1 and launches["paths7+up_wta"] == 1 and launches["paths8+up_wta"] == 1, launches
    outs = eng.match_batch([f[0] for f in fs[:3]], [f[1] for f in fs[:3]], devices=[0, 0])
    for i in range(3):
        same(outs[i], refs[i], f"host batch frame {i}")
    # 4 paths
    eng.set_census_paths(4)
    r4 = [ref_match(oracle, p, l, r, win, (0, 1, 6, 7)) for l, r in fs[:3]]
    same(eng.match(left, right), r4[0], "4 paths")
    got = _device_batch(torch, eng, fs[:3], h, w)
    for i in range(3):
        same(got[i], r4[i], f"4 paths batch frame {i}")
    eng.set_census_paths(8)
    # median + speckles, then hole filling on top
    import fill_reference as fr
    q = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=5, median=1, speckle_window_size=20,
                           speckle_range=2)
    eng.set_params(q)
    rq = [ref_match(oracle, q, l, r, win) for l, r in fs[:3]]
    same(eng.match(left, right), rq[0], "median + speckles")
    got = _device_batch(torch, eng, fs[:3], h, w)
    for i in range(3):
        same(got[i], rq[i], f"median + speckles batch frame {i}")
    f = pkg.default_fill_params(mode=pkg.FILL_BACKGROUND, max_gap=8, min_neighbours=2)
    eng.set_fill_params(f)
    e = oracle.effective(to_oracle_params(oracle, q), w, h)
    filled = eng.fill(rq[0], e["invalid"], f, (e["minX1"], 0, e["maxX1"], h))
    same(eng.match(left, right), filled, "fill")


@pytest.mark.parametrize("win", WINS4, ids=str)
def test_entry_points_small_negative_min_disparity(eng, oracle, pkg, frames, win):
    """96x40, D 32, minD -3 (two tile columns, a partial tile row, a window cut on the right):
    match_f32, match_device with padded strides and the 5-frame device batch."""
    torch = pytest.importorskip("torch")
    h, w, D = 40, 96, 32
    fs = frames[(h, w, D)]
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=-3)
    refs = [ref_match(oracle, p, l, r, win) for l, r in fs]
    eng.set_params(p)
    eng.set_census_window(*win)
    left, right = fs[0]
    same(eng.match_f32(left, right), refs[0].astype(np.float32), "match_f32")
    dl = torch.zeros((h, w + 7), dtype=torch.uint8, device="cuda")
    dr = torch.zeros((h, w + 7), dtype=torch.uint8, device="cuda")
    dl[:, :w], dr[:, :w] = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.full((h, w + 3), 1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.match_device(dl.data_ptr(), dr.data_ptr(), w, h, w + 7, out.data_ptr(), w + 3)
    eng.synchronize()
    got = out.cpu().numpy()
    same(got[:, :w], refs[0], "match_device")
    assert (got[:, w:] == 1234).all()
    got = _device_batch(torch, eng, fs, h, w, pad_in=5, pad_out=1)
    for i in range(5):
        same(got[i], refs[i], f"batch frame {i}")


def test_setter_stores_anything(eng, pkg):
    """On a real handle: the default, null arguments, and any triple stored and read back."""
    import ctypes
    lib, h = eng.lib, eng.h
    got = pkg.CensusWindow()
    assert eng.get_census_window() == (9, 7, 1)
    assert lib.sgm_set_census_window(h, None) == pkg.SGM_ERR_ARG
    assert lib.sgm_get_census_window(h, None) == pkg.SGM_ERR_ARG
    for bad in [(4, 7, 1), (0, 0, 0), (-9, 700, 3)]:
        assert lib.sgm_set_census_window(h, ctypes.byref(pkg.CensusWindow(*bad))) == pkg.SGM_OK
        assert lib.sgm_get_census_window(h, ctypes.byref(got)) == pkg.SGM_OK and got.as_tuple() == bad


def test_debug_census_in_other_modes(eng, pkg):
    """The OCV and BM modes ignore the window: with an invalid one stored, sgm_debug_census keeps
    giving the 9x7 codes there and fails in the census mode only; a valid one is honoured anywhere."""
    img = np.random.default_rng(11).integers(0, 256, (21, 70), dtype=np.uint8)
    for mode in (pkg.MODE_OCV_SGBM5, pkg.MODE_OCV_BM):
        eng.set_params(pkg.default_params(mode))
        eng.set_census_window(4, 7, 1)
        same(eng.census(img), cwr.census(img), f"mode {mode}, invalid window")
        eng.set_census_window(5, 5, 2)
        same(eng.census(img), cwr.census(img, (5, 5, 2)), f"mode {mode}, valid window")
    eng.set_params(pkg.default_params(pkg.MODE_CENSUS8))
    eng.set_census_window(4, 7, 1)
    with pytest.raises(pkg.SGMError) as e:
        eng.census(img)
    assert e.value.code == pkg.SGM_ERR_PARAM


def test_plugin_driver_checksums(oracle):
    """plugin_window_test match: forwardMatch and backwardMatch16 through the C++ adapter core with
    the window (7, 7, 2) chosen by setWindowSize(11) under the cfg route; its checksums are those of
    the reference for the parameter blocks it prints."""
    import os
    import subprocess
    import census_paths_reference as cpr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "i3dr_stereo_camera-ros_amd", "lib", "plugin_window_test")
    env = {k: v for k, v in os.environ.items() if k not in ("SGM_HIP_CENSUS_WINDOW", "SGM_HIP_CENSUS_PATHS", "SGM_HIP_FILL")}
    r = subprocess.run([exe, "match"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        t = line.split()
        if len(t) > 2 and t[1] in ("params", "hash"):
            out[(t[0], t[1])] = t[2:]
    assert "window 7 7 2" in r.stdout.splitlines() and "window match ok" in r.stdout
    left, right = cpr.driver_frame()
    names = [n for n, _ in oracle.SgmParams._fields_]
    hashes = {}
    for side, (a, b) in (("forward", (left, right)), ("backward", (right, left))):
        vals = [int(v) for v in out[(side, "params")]]
        assert len(vals) == len(names) and vals[0] == oracle.MODE_CENSUS8 and vals[3] == 11      # block_size kept
        p = oracle.make_params(vals[0], **dict(zip(names[1:], vals[1:])))
        ref = cwr.match(oracle, p, a, b, (7, 7, 2))
        assert (ref != (p.min_disparity - 1) * 16).mean() > 0.2          # a real match, not an empty image
        assert not np.array_equal(ref, cwr.match(oracle, p, a, b))       # and not the default window's
        hashes[side] = cpr.fnv1a16(ref)
        assert int(out[(side, "hash")][0], 16) == hashes[side], side
    assert int(out[("again", "hash")][0], 16) == hashes["forward"]       # setWindowSize(15) unfollowed: unchanged


def test_explicit_default_changes_nothing(eng, oracle, pkg, frames):
    torch = pytest.importorskip("torch")
    h, w, D = 56, 144, 64
    fs = frames[(h, w, D)]
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng.set_params(p)
    runs = []
    for explicit in (False, True):
        if explicit:
            eng.set_census_window(9, 7, 1)
        eng.set_profiling(True)
        one = eng.match(*fs[0])
        got = _device_batch(torch, eng, fs, h, w)
        names = [s[0] for s in eng.stage_times()]
        eng.set_profiling(False)
        runs.append((one, got, names))
    same(runs[0][0], runs[1][0], "match")
    same(runs[0][1], runs[1][1], "batch")
    assert runs[0][2] == runs[1][2] and "census_win" not in runs[0][2]
    same(runs[0][0], oracle.match(to_oracle_params(oracle, p), *fs[0]), "oracle")


def test_single_frame_stage_and_bytes(eng, pkg, frames):
    h, w, D = 56, 144, 64
    eng.set_params(pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D))
    eng.set_census_window(7, 7, 2)
    eng.set_profiling(True)
    eng.match(*frames[(h, w, D)][0])
    st = eng.stage_times()
    eng.set_profiling(False)
    assert [s[0] for s in st] == ["census_win", "paths8", "wta_lr"]
    assert st[0][2] == 18.0 * w * h


def test_invalid_window(eng, oracle, synth, pkg):
    import bm_reference as br
    h, w, D = 48, 160, 32
    left, right, _ = synth.stereo_pair(h, w, 0, D, seed=8)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng.set_params(p)
    eng.set_census_window(4, 7, 1)
    for call in (lambda: eng.match(left, right), lambda: eng.match_f32(left, right), lambda: eng.census(left),
                 lambda: eng.match_tiled(left, right, 2, 8), lambda: eng.match_tiled_exact(left, right, 2)):
        with pytest.raises(pkg.SGMError) as e:
            call()
        assert e.value.code == pkg.SGM_ERR_PARAM, eng.error()
    assert "window" in eng.error()
    q = pkg.default_params(pkg.MODE_OCV_SGBM5, num_disparities=D, min_disparity=0, block_size=5)
    eng.set_params(q)
    same(eng.match(left, right), oracle.match(to_oracle_params(oracle, q), left, right), "MODE_SGBM ignores it")
    bm = br.BM(0, D, 9, 31, 10, 15)
    eng.set_params(pkg.default_params(pkg.MODE_OCV_BM, min_disparity=bm.m, num_disparities=bm.D, block_size=bm.w,
                                      prefilter_cap=bm.c, uniqueness_ratio=bm.u, speckle_window_size=0,
                                      speckle_range=0, disp12_max_diff=-1))
    eng.set_bm_params(pkg.default_bm_params(texture_threshold=bm.t))
    same(eng.match(left, right), br.compute(bm, left, right), "MODE_OCV_BM ignores it")
    eng.set_params(p)


# ---- tile modes ----------------------------------------------------------------------------
@pytest.mark.parametrize("win", [(7, 7, 1), (9, 7, 2)], ids=str)
def test_tiled_modes(eng, oracle, synth, pkg, win):
    torch = pytest.importorskip("torch")
    h, w, D, bands, halo = 90, 150, 32, 3, 12
    left, right, _ = synth.stereo_pair(h, w, 0, D, seed=47)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng.set_params(p)
    eng.set_census_window(*win)
    full = ref_match(oracle, p, left, right, win)
    same(eng.match(left, right), full, "match")
    same(eng.match_tiled(left, right, 1, 0), full, "1 band")
    same(eng.match_tiled_exact(left, right, bands), full, "tiled_exact")
    got = eng.match_tiled(left, right, bands, halo)
    for b in range(bands):
        c0, c1 = b * h // bands, (b + 1) * h // bands
        e0, e1 = max(0, c0 - halo), min(h, c1 + halo)
        same(got[c0:c1], ref_match(oracle, p, left[e0:e1], right[e0:e1], win)[c0 - e0:c1 - e0], f"band {b}")
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    for nb, want in ((1, full), (bands, got)):
        out = torch.full((h, w + 4), 1234, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.match_tiled_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w + 4, nb, halo if nb > 1 else 0,
                               devices=[0, 0])
        dev = out.cpu().numpy()
        same(dev[:, :w], want, f"tiled_device {nb}")
        assert (dev[:, w:] == 1234).all()


# ---- raw and colour frames -----------------------------------------------------------------
def _gray(pkg, img):
    return pkg.bgr2gray(img, pkg.GRAY_Y14) if img.ndim == 3 else img


@pytest.mark.parametrize("ch", [1, 3])
def test_raw_frames_rectified(eng, oracle, pkg, synth, ch):
    """match_device_batch_rect (3 frames) and node_frame on raw mono / colour frames with (7, 7, 2):
    the rectified outputs are those of the default window bit for bit, the disparity is the
    reference's on the rectified (then converted) images."""
    torch = pytest.importorskip("torch")
    from test_gpu_rectify import _maps
    from test_rectify_oracle import calib
    n, h, w, D, win = 3, 120, 200, 32, (7, 7, 2)
    infos = [calib(seed=11, w=w, h=h), calib(seed=12, w=w, h=h)]
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng.set_params(p)
    eng.set_raw_format(ch, pkg.GRAY_Y14)
    mxl, myl = _maps(torch, eng, *infos[0], w, h)
    mxr, myr = _maps(torch, eng, *infos[1], w, h)
    rng = np.random.default_rng(3)
    raws = []
    for i in range(n):
        l, r = synth.stereo_pair(h, w, 0, 24, seed=70 + i)[:2]
        if ch == 3:       # a colour frame whose channels differ
            l = np.stack([l, l // 2 + 30, 255 - l], -1).astype(np.uint8)
            r = np.stack([r, r // 2 + 30, 255 - r], -1).astype(np.uint8)
        raws.append((np.ascontiguousarray(l), np.ascontiguousarray(r)))
    dl = [torch.as_tensor(f[0]).cuda() for f in raws]
    dr = [torch.as_tensor(f[1]).cuda() for f in raws]
    res = {}
    for wn in (cwr.DEFAULT, win):
        eng.set_census_window(*wn)
        out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
        recl = torch.zeros((n, h, w * ch + 8), dtype=torch.uint8, device="cuda")
        recr = torch.zeros((n, h, w * ch + 8), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.set_rectification((mxl.data_ptr(), myl.data_ptr()), (mxr.data_ptr(), myr.data_ptr()), w, w, h)
        try:
            eng.match_device_batch_rect([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, w * ch,
                                         [recl[i].data_ptr() for i in range(n)], [recr[i].data_ptr() for i in range(n)],
                                         w * ch + 8, [out[i].data_ptr() for i in range(n)], w)
            eng.synchronize()
        finally:
            eng.set_rectification()
        res[wn] = (out.cpu().numpy(), recl.cpu().numpy(), recr.cpu().numpy())
    same(res[win][1], res[cwr.DEFAULT][1], "rectified left")
    same(res[win][2], res[cwr.DEFAULT][2], "rectified right")
    shape = (h, w, 3) if ch == 3 else (h, w)
    for i in range(n):
        el = _gray(pkg, res[win][1][i, :, :w * ch].reshape(shape))
        er = _gray(pkg, res[win][2][i, :, :w * ch].reshape(shape))
        same(res[win][0][i], ref_match(oracle, p, el, er, win), f"frame {i}")
        same(res[cwr.DEFAULT][0][i], ref_match(oracle, p, el, er, cwr.DEFAULT), f"frame {i}, default window")
    # node_frame: the same frame 0, in one host call
    eng.set_census_window(*win)
    rl, rr, disp, _ = eng.node_frame(raws[0][0], raws[0][1], infos[0], infos[1], -1e9, 1e9)
    same(rl.reshape(h, -1), res[win][1][0, :, :w * ch], "node_frame rectified left")
    same(rr.reshape(h, -1), res[win][2][0, :, :w * ch], "node_frame rectified right")
    same(disp, res[win][0][0].astype(np.float32) * np.float32(0.0625), "node_frame disparity")


def test_colour_frames_without_rectification(eng, oracle, pkg, synth):
    torch = pytest.importorskip("torch")
    h, w, D, win = 56, 144, 32, (9, 7, 2)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng.set_params(p)
    eng.set_raw_format(3, pkg.GRAY_Y15)
    eng.set_census_window(*win)
    fs = []
    for i in range(3):
        l, r = synth.stereo_pair(h, w, 0, D, seed=300 + i)[:2]
        fs.append((np.ascontiguousarray(np.stack([l, 255 - l, l // 3], -1)), np.ascontiguousarray(np.stack([r, 255 - r, r // 3], -1))))
    refs = [ref_match(oracle, p, pkg.bgr2gray(l, pkg.GRAY_Y15), pkg.bgr2gray(r, pkg.GRAY_Y15), win) for l, r in fs]
    same(eng.match(*fs[0]), refs[0], "match")
    dl = [torch.as_tensor(f[0]).cuda() for f in fs]
    dr = [torch.as_tensor(f[1]).cuda() for f in fs]
    out = torch.full((3, h, w), 777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.match_device_batch([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, 3 * w,
                           [out[i].data_ptr() for i in range(3)], w)
    eng.synchronize()
    got = out.cpu().numpy()
    for i in range(3):
        same(got[i], refs[i], f"batch frame {i}")
