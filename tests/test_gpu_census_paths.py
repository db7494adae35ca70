"""GPU parity — the census mode's 4-path set (sgm_set_census_paths(4): directions 0, 1, 6, 7)
through every entry point, bit-exact against the reference composed from the oracle's stages
(tests/census_paths_reference.py: sum of the four oracle path volumes, oracle WTA, median,
speckles). The shared engine is set back to 8 paths after every test.
"""
import os
import subprocess

import numpy as np
import pytest

import census_paths_reference as cpr
from conftest import to_oracle_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FUZZ = max(1, int(os.environ.get("SGM_FUZZ_CASES", "120")) // 3)   # 40 by default, scaled like test_gpu_fuzz.py


@pytest.fixture
def eng4(engine):
    """The shared engine with 4 census paths; 8 again afterwards."""
    engine.set_census_paths(4)
    try:
        yield engine
    finally:
        engine.set_census_paths(8)
        engine.set_profiling(False)


def ref4(oracle, p, left, right):
    return cpr.match_paths(oracle, to_oracle_params(oracle, p), left, right)


def same(got, ref, what=""):
    assert np.array_equal(got, ref), f"{what}: {(np.asarray(got) != np.asarray(ref)).sum()} pixels differ"


CASES = [
    dict(num_disparities=16, p1=3, p2=20, disp12_max_diff=3),
    dict(num_disparities=32, min_disparity=-9),
    dict(num_disparities=32, min_disparity=5, uniqueness_ratio=15),
    dict(num_disparities=64),
    dict(num_disparities=64, subpixel=0),
    dict(num_disparities=64, lr_check=0),
    dict(num_disparities=64, p2=250),              # clamped to 193 (u8 path costs)
    dict(num_disparities=96, speckle_window_size=30, speckle_range=2, median=1),
    dict(num_disparities=128, median=1),
    dict(num_disparities=256, uniqueness_ratio=0),
    dict(num_disparities=272),                     # 32 values per lane, a lane straddles D
    dict(num_disparities=400, min_disparity=3),
    dict(num_disparities=512),
    dict(num_disparities=64, uniqueness_ratio=99),
    dict(num_disparities=64, uniqueness_ratio=100),
    dict(num_disparities=48, uniqueness_ratio=130),
]


@pytest.mark.parametrize("kw", CASES, ids=[str(i) for i in range(len(CASES))])
def test_pipeline(eng4, oracle, synth, pkg, kw):
    D, minD = kw["num_disparities"], kw.get("min_disparity", 0)
    h, w = 61, max(D + minD, 0) + 133
    left, right, _ = synth.stereo_pair(h, w, max(minD, 0), D, seed=D + 17)
    p = pkg.default_params(pkg.MODE_CENSUS8, **kw)
    eng4.set_params(p)
    assert eng4.get_census_paths() == 4
    same(eng4.match(left, right), ref4(oracle, p, left, right), str(kw))


@pytest.mark.parametrize("h,w,D,minD", [(4, 20, 16, 0), (3, 17, 16, 0), (9, 16, 16, 0), (2, 200, 64, -30),
                                        (270, 480, 128, 0)])
def test_edge_geometry(eng4, oracle, synth, pkg, h, w, D, minD):
    if h >= 100:     # several blocks per direction and several rounds of the work list
        left, right, _ = synth.stereo_pair(h, w, 0, D, seed=31)
    else:
        rng = np.random.default_rng(3 + h)
        left = rng.integers(0, 256, (h, w), dtype=np.uint8)
        right = rng.integers(0, 256, (h, w), dtype=np.uint8)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=minD, median=1)
    eng4.set_params(p)
    same(eng4.match(left, right), ref4(oracle, p, left, right), f"{h}x{w}")


def _device_batch(torch, eng, frames, h, w, pad_in=0, pad_out=0):
    n = len(frames)
    dl = torch.zeros((n, h, w + pad_in), dtype=torch.uint8, device="cuda")
    dr = torch.zeros((n, h, w + pad_in), dtype=torch.uint8, device="cuda")
    for i, f in enumerate(frames):
        dl[i, :, :w] = torch.from_numpy(f[0]).cuda()
        dr[i, :, :w] = torch.from_numpy(f[1]).cuda()
    out = torch.full((n, h, w + pad_out), 777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.match_device_batch([dl[i].data_ptr() for i in range(n)], [dr[i].data_ptr() for i in range(n)], w, h,
                           w + pad_in, [out[i].data_ptr() for i in range(n)], w + pad_out)
    eng.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :, w:] == 777).all()
    return got[:, :, :w]


@pytest.fixture(scope="module")
def d64(oracle, synth, pkg):
    """Five D = 64 frames (61 x 197) and their 4-path references, shared by the entry-point tests."""
    h, w, D = 61, 197, 64
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    frames = [synth.stereo_pair(h, w, 0, D, seed=500 + i)[:2] for i in range(5)]
    refs = [ref4(oracle, p, l, r) for l, r in frames]
    for r in refs:
        r.setflags(write=False)
    return h, w, p, frames, refs


def test_host_and_device_entry_points(eng4, pkg, d64):
    """match, match_f32 (plain and into a registered, mapped buffer: the WTA's float rows) and
    match_device with padded strides."""
    torch = pytest.importorskip("torch")
    h, w, p, frames, refs = d64
    (left, right), ref = frames[0], refs[0]
    eng4.set_params(p)
    same(eng4.match(left, right), ref, "match")
    same(eng4.match_f32(left, right), ref.astype(np.float32), "match_f32")
    buf = np.full((h, w + 5), -7, np.float32)
    eng4.host_register(buf)
    try:
        eng4.match_f32(left, right, out=buf[:, :w])
        same(buf[:, :w], ref.astype(np.float32), "match_f32 registered")
        assert (buf[:, w:] == -7).all()
    finally:
        eng4.host_unregister(buf)
    dl = torch.zeros((h, w + 11), dtype=torch.uint8, device="cuda")
    dr = torch.zeros((h, w + 11), dtype=torch.uint8, device="cuda")
    dl[:, :w], dr[:, :w] = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.full((h, w + 3), 1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng4.match_device(dl.data_ptr(), dr.data_ptr(), w, h, w + 11, out.data_ptr(), w + 3)
    eng4.synchronize()
    got = out.cpu().numpy()
    same(got[:, :w], ref, "match_device")
    assert (got[:, w:] == 1234).all()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_device_batch_launch_forms(eng4, pkg, d64, n):
    """n = 1: the single-frame pipeline; 2: one group; 3: first + last with an odd tail; 5: first,
    steady and last launches (groups of 2)."""
    torch = pytest.importorskip("torch")
    h, w, p, frames, refs = d64
    eng4.set_params(p)
    eng4.set_profiling(True)
    got = _device_batch(torch, eng4, frames[:n], h, w, pad_in=3, pad_out=5)
    launches = eng4.stage_launches()
    eng4.set_profiling(False)
    for i in range(n):
        same(got[i], refs[i], f"frame {i} of {n}")
    ng = (n + 1) // 2
    assert not any("paths8" in k or "paths7" in k for k in launches)
    if n <= 2:
        assert launches["paths4"] == 1 and launches["wta_lr"] == 1
    else:
        assert launches["paths3+census"] == 1 and launches["paths4+up_wta"] == 1
        assert launches.get("paths3+up_wta+census", 0) == ng - 2
        assert launches["rowfin"] == ng - 1 and launches["wta_lr"] == 1


def test_device_batch_median_scratch(eng4, oracle, synth, pkg):
    torch = pytest.importorskip("torch")
    h, w, D = 45, 214, 64
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, median=1)
    eng4.set_params(p)
    frames = [synth.stereo_pair(h, w, 0, D, seed=520 + i)[:2] for i in range(3)]
    got = _device_batch(torch, eng4, frames, h, w)
    for i, (l, r) in enumerate(frames):
        same(got[i], ref4(oracle, p, l, r), f"frame {i}")


@pytest.mark.parametrize("up_wta", [1, 0])
def test_device_batch_paths_wta_scheme(eng4, oracle, synth, pkg, monkeypatch, up_wta):
    """The batch scheme without up+WTA blocks: D > 256 always takes it, and SGM_UPWTA=0 at D 64."""
    torch = pytest.importorskip("torch")
    D = 272 if up_wta else 64
    monkeypatch.setenv("SGM_UPWTA", str(up_wta))
    h, w = 33, D + 90
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng4.set_params(p)
    frames = [synth.stereo_pair(h, w, 0, D, seed=540 + i)[:2] for i in range(3)]
    eng4.set_profiling(True)
    got = _device_batch(torch, eng4, frames, h, w)
    launches = eng4.stage_launches()
    eng4.set_profiling(False)
    for i, (l, r) in enumerate(frames):
        same(got[i], ref4(oracle, p, l, r), f"frame {i}")
    assert launches["paths4+census"] == 1 and launches["paths4+wta_lr"] == 1 and launches["wta_lr"] == 1


def test_host_batch_sub_handles_inherit(eng4, pkg, d64):
    h, w, p, frames, refs = d64
    eng4.set_params(p)
    outs = eng4.match_batch([f[0] for f in frames[:3]], [f[1] for f in frames[:3]], devices=[0, 0])
    for i in range(3):
        same(outs[i], refs[i], f"frame {i}")


def test_tiled_modes(eng4, oracle, synth, pkg):
    """One band = match; three bands with a halo = the 4-path match of each band's rows + halo, own
    rows kept; the device-buffer tile mode gives the same image."""
    torch = pytest.importorskip("torch")
    h, w, D, bands, halo = 120, 200, 64, 3, 16
    left, right, _ = synth.stereo_pair(h, w, 0, D, seed=47)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    eng4.set_params(p)
    same(eng4.match_tiled(left, right, 1, 0), ref4(oracle, p, left, right), "1 band")
    got = eng4.match_tiled(left, right, bands, halo)
    for b in range(bands):
        c0, c1 = b * h // bands, (b + 1) * h // bands
        e0, e1 = max(0, c0 - halo), min(h, c1 + halo)
        same(got[c0:c1], ref4(oracle, p, left[e0:e1], right[e0:e1])[c0 - e0:c1 - e0], f"band {b}")
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.full((h, w + 4), 1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng4.match_tiled_device(dl.data_ptr(), dr.data_ptr(), w, h, w, out.data_ptr(), w + 4, bands, halo, devices=[0, 0])
    dev = out.cpu().numpy()
    same(dev[:, :w], got, "tiled_device")
    assert (dev[:, w:] == 1234).all()


def test_fused_rectification(eng4, oracle, pkg, synth):
    torch = pytest.importorskip("torch")
    from test_gpu_rectify import _maps
    from test_rectify_oracle import calib
    n, h, w = 3, 240, 320
    KL, DL, RL, PL = calib(seed=11, w=w, h=h)
    KR, DR, RR, PR = calib(seed=12, w=w, h=h)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=64)
    eng4.set_params(p)
    mxl, myl = _maps(torch, eng4, KL, DL, RL, PL, w, h)
    mxr, myr = _maps(torch, eng4, KR, DR, RR, PR, w, h)
    frames = [synth.stereo_pair(h, w, 0, 48, seed=70 + i)[:2] for i in range(n)]
    dl = [torch.as_tensor(f[0]).cuda() for f in frames]
    dr = [torch.as_tensor(f[1]).cuda() for f in frames]
    out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
    recl = torch.zeros((n, h, w + 8), dtype=torch.uint8, device="cuda")
    recr = torch.zeros((n, h, w + 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng4.set_rectification((mxl.data_ptr(), myl.data_ptr()), (mxr.data_ptr(), myr.data_ptr()), w, w, h)
    try:
        eng4.match_device_batch_rect([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, w,
                                     [recl[i].data_ptr() for i in range(n)], [recr[i].data_ptr() for i in range(n)],
                                     w + 8, [out[i].data_ptr() for i in range(n)], w)
        eng4.synchronize()
    finally:
        eng4.set_rectification()
    rxl, ryl = oracle.rectify_map(KL, DL, RL, PL, w, h)
    rxr, ryr = oracle.rectify_map(KR, DR, RR, PR, w, h)
    got, gl, gr = out.cpu().numpy(), recl.cpu().numpy(), recr.cpu().numpy()
    for i, (l_raw, r_raw) in enumerate(frames):
        el, er = oracle.remap_cubic(l_raw, rxl, ryl), oracle.remap_cubic(r_raw, rxr, ryr)
        assert np.array_equal(gl[i, :, :w], el) and np.array_equal(gr[i, :, :w], er), f"frame {i} rectified"
        same(got[i], ref4(oracle, p, el, er), f"frame {i} disparity")


def test_path_set_changes_on_one_handle(engine, oracle, synth, pkg):
    """8 -> 4 -> 8 on one handle and one frame, single frame and a 3-frame batch: the workspace is
    laid out again and the uploaded work lists are replaced."""
    torch = pytest.importorskip("torch")
    h, w, D = 61, 197, 64
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    frames = [synth.stereo_pair(h, w, 0, D, seed=560 + i)[:2] for i in range(3)]
    op = to_oracle_params(oracle, p)
    ref8 = [oracle.match(op, l, r) for l, r in frames]
    r4 = [ref4(oracle, p, l, r) for l, r in frames]
    engine.set_params(p)
    try:
        for paths, refs in [(8, ref8), (4, r4), (8, ref8)]:
            engine.set_census_paths(paths)
            same(engine.match(*frames[0]), refs[0], f"{paths} paths, single frame")
            got = _device_batch(torch, engine, frames, h, w)
            for i in range(3):
                same(got[i], refs[i], f"{paths} paths, batch frame {i}")
    finally:
        engine.set_census_paths(8)


def test_errors_and_scope(engine, oracle, synth, pkg):
    import bm_reference as br
    h, w, D = 48, 160, 32
    left, right, _ = synth.stereo_pair(h, w, 0, D, seed=8)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    engine.set_params(p)
    try:
        engine.set_census_paths(5)                  # setters never fail
        assert engine.get_census_paths() == 5
        with pytest.raises(pkg.SGMError) as e:
            engine.match(left, right)
        msg = engine.error()
        assert e.value.code == pkg.SGM_ERR_PARAM and "4" in msg and "8" in msg, msg
        engine.set_census_paths(4)
        with pytest.raises(pkg.SGMError) as e:
            engine.match_tiled_exact(left, right, 3)
        assert e.value.code == pkg.SGM_ERR_UNSUPPORTED
        # the other modes ignore the value
        q = pkg.default_params(pkg.MODE_OCV_SGBM5, num_disparities=D, min_disparity=0, block_size=5)
        engine.set_params(q)
        same(engine.match(left, right), oracle.match(to_oracle_params(oracle, q), left, right), "MODE_SGBM")
        bm = br.BM(0, D, 9, 31, 10, 15)
        engine.set_params(pkg.default_params(pkg.MODE_OCV_BM, min_disparity=bm.m, num_disparities=bm.D,
                                             block_size=bm.w, prefilter_cap=bm.c, uniqueness_ratio=bm.u,
                                             speckle_window_size=0, speckle_range=0, disp12_max_diff=-1))
        engine.set_bm_params(pkg.default_bm_params(texture_threshold=bm.t))
        same(engine.match(left, right), br.compute(bm, left, right), "MODE_OCV_BM")
        engine.set_params(p)
        engine.set_census_paths(8)
        ref = oracle.match(to_oracle_params(oracle, p), left, right)
        same(engine.match_tiled_exact(left, right, 3), ref, "tiled_exact after restoring 8")
        same(engine.match(left, right), ref, "match after restoring 8")
    finally:
        engine.set_params(p)
        engine.set_census_paths(8)


def test_profiling_stage_names_and_bytes(eng4, pkg, d64):
    torch = pytest.importorskip("torch")
    h, w, p, frames, refs = d64
    eng4.set_params(p)
    WH, cells = float(w * h), float((w - 64) * h * 64)
    eng4.set_profiling(True)
    eng4.match(*frames[0])
    st = eng4.stage_times()
    eng4.set_profiling(False)
    assert [s[0] for s in st] == ["census", "paths4", "wta_lr"]
    by = {s[0]: s[2] for s in st}
    assert by["paths4"] == 4 * cells and by["wta_lr"] == 4 * cells + 2 * WH
    eng4.set_profiling(True)
    _device_batch(torch, eng4, frames[:4], h, w)
    st = eng4.stage_times()
    eng4.set_profiling(False)
    by = {s[0]: s[2] for s in st}
    assert [s[0] for s in st] == ["census", "paths3+census", "paths4+up_wta", "rowfin", "wta_lr"]
    # groups of 2: the 8-path formulas (7 | 8 volumes written, 9 per up+WTA frame, 8 read) with 3 | 4, 5, 4
    assert by["paths3+census"] == 3 * cells * 2 + 18 * WH * 2
    assert by["paths4+up_wta"] == 4 * cells * 2 + (5 * cells + 2 * WH) * 2
    assert by["rowfin"] == 10 * WH * 2
    assert by["wta_lr"] == (4 * cells + 2 * WH) * 2
    assert all(t >= 0 for _, t, _ in st)


def _fuzz_case(seed):
    rng = np.random.default_rng(40_000 + seed)
    D = 16 * int(rng.integers(1, 33))
    minD = int(rng.integers(-40, 41))
    h = int(rng.integers(1, 81))
    # W <= 400: mostly wider than the search (a valid window) where D allows it, else any width
    span = max(D + minD, 0)
    w = min(400, span + int(rng.integers(1, 120))) if span < 399 and rng.random() < 0.85 else int(rng.integers(1, 401))
    p1 = int(rng.integers(1, 40))
    kw = dict(num_disparities=D, min_disparity=minD, p1=p1, p2=int(rng.integers(p1 + 1, 260)),
              uniqueness_ratio=int(rng.choice([0, 1, 5, 10, 15, 30, 99, 100, 120])),
              disp12_max_diff=int(rng.choice([-1, 0, 1, 2, 5])), subpixel=int(rng.integers(0, 2)),
              lr_check=int(rng.integers(0, 2)), median=int(rng.integers(0, 2)),
              speckle_window_size=int(rng.choice([0, 0, 10, 50])), speckle_range=int(rng.integers(1, 4)))
    entry = str(rng.choice(["match", "match_f32", "match_device", "batch"]))
    n = int(rng.integers(1, 5)) if entry == "batch" else 1
    return rng, h, w, kw, entry, n


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz(eng4, oracle, synth, pkg, seed):
    torch = pytest.importorskip("torch")
    rng, h, w, kw, entry, n = _fuzz_case(seed)
    D, minD = kw["num_disparities"], kw["min_disparity"]
    p = pkg.default_params(pkg.MODE_CENSUS8, **kw)
    eng4.set_params(p)
    frames = []
    for i in range(n):
        if rng.random() < 0.3:
            frames.append((rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)))
        else:
            frames.append(synth.stereo_pair(h, w, max(minD, 0), D, seed=1000 * seed + i, with_truth=False)[:2])
    refs = [ref4(oracle, p, l, r) for l, r in frames]
    what = f"{entry} n={n} {h}x{w} {kw}"
    if entry == "match":
        same(eng4.match(*frames[0]), refs[0], what)
    elif entry == "match_f32":
        same(eng4.match_f32(*frames[0]), refs[0].astype(np.float32), what)
    else:
        got = _device_batch(torch, eng4, frames, h, w, pad_in=int(rng.integers(0, 9)), pad_out=int(rng.integers(0, 9)))
        for i in range(n):
            same(got[i], refs[i], f"{what} frame {i}")


def test_plugin_driver_checksums(oracle):
    """plugin_paths_test match: a 4-path forwardMatch and backwardMatch16 through the C++ adapter
    core (the backward match with rightMatcherParams); its checksums are those of the composed
    reference for the parameter blocks it prints."""
    exe = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_paths_test")
    env = {k: v for k, v in os.environ.items() if k != "SGM_HIP_CENSUS_PATHS"}
    r = subprocess.run([exe, "match"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        t = line.split()
        if len(t) > 2 and t[1] in ("params", "hash"):
            out[(t[0], t[1])] = t[2:]
    assert "paths match ok" in r.stdout
    left, right = cpr.driver_frame()
    names = [n for n, _ in oracle.SgmParams._fields_]
    for side, (a, b) in (("forward", (left, right)), ("backward", (right, left))):
        vals = [int(v) for v in out[(side, "params")]]
        assert len(vals) == len(names) and vals[0] == oracle.MODE_CENSUS8
        p = oracle.make_params(vals[0], **dict(zip(names[1:], vals[1:])))
        ref = cpr.match_paths(oracle, p, a, b)
        assert (ref != (p.min_disparity - 1) * 16).mean() > 0.2          # a real match, not an empty image
        assert int(out[(side, "hash")][0], 16) == cpr.fnv1a16(ref), side
    # the backward block is the right matcher's: mirrored window, uniqueness 0, no speckles
    fw = [int(v) for v in out[("forward", "params")]]
    bw = [int(v) for v in out[("backward", "params")]]
    assert bw[1] == -(fw[1] + fw[2]) + 1 and bw[6] == 0 and bw[9] == 0 and bw[7] == 1000000
