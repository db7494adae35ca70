"""CPU tests of the MODE_OCV_BM tiling (csrc/bm.hip bm_plan) through sgm_debug_bm_plan, which needs
no device: invariants of the plan over a seeded sweep, the plans of the production frames pinned at
256 CUs, and the entry point's errors. On a 256-CU device every frame the explicit-sum reference
(tests/bm_reference.py) can afford is planned with strips of at most 32 columns (asserted below). The
box-sum reference (tests/bm_fast_reference.py) affords frames that such a device plans like production
frames by itself; they and their pinned plans are in tests/bm_tiling_cases.py and
tests/test_bm_fast_reference.py. No GPU test in the suite compares those tilings yet (BM
section, says where that stands); bands longer than 41 rows and the full-size frames pinned here are
compared by nothing."""
import ctypes

import numpy as np
import pytest

LDS_BUDGET = 128 * 1024         # csrc/bm.hip kBmLdsBudget
LDS_CU = 160 * 1024             # LDS of a gfx950 CU


def bm_params(pkg, m, D, w, cap):
    return pkg.default_params(pkg.MODE_OCV_BM, min_disparity=m, num_disparities=D, block_size=w, prefilter_cap=cap)


def plan(pkg, H, W, m, D, w, cap, n_cu):
    return pkg.bm_plan(bm_params(pkg, m, D, w, cap), pkg.default_bm_params(), W, H, n_cu)


def clean_env(monkeypatch):
    monkeypatch.delenv("SGM_BM_VGLOBAL", raising=False)


def draw(rng):
    w = int(rng.choice(np.arange(5, 43, 2)))

    def size(lo):   # lo .. 4096: three in ten close to lo, the rest log-uniform
        if rng.random() < 0.3:
            return int(min(rng.integers(lo, lo + 40), 4096))
        return int(np.exp(rng.uniform(np.log(lo), np.log(4096.999))))

    D = int(rng.choice([16, 32, 48, 64, 80, 96, 128, 144, 256, 272, 480, 512, 528, 1024, 1040, 2032, 2048]))
    m = int(rng.integers(-64, 201))
    # nine widths in ten leave at least one computed column (X0 = max(D - 1 + m, 0) < X1 = min(W, W + m))
    first = max(D - 1 + m, 0) - min(m, 0) + 1
    W = size(max(first, w + 1)) if rng.random() < 0.9 and first <= 4096 else size(w + 1)
    return dict(H=size(w + 1), W=W, m=m, D=D, w=w, cap=int(rng.integers(1, 64)),
                n_cu=int(rng.choice([1, 2, 4, 8, 16, 32, 64, 256, 304])))


@pytest.mark.parametrize("forced", [0, 1], ids=["lds", "SGM_BM_VGLOBAL"])
def test_plan_invariants(pkg, monkeypatch, forced):
    clean_env(monkeypatch)
    if forced:
        monkeypatch.setenv("SGM_BM_VGLOBAL", "1")
    rng = np.random.default_rng(5150 + forced)
    seen = dict(vglobal=0, wide=0, w16=0, halved=0, full=0, empty=0)
    for _ in range(2500):
        k = draw(rng)
        pl = plan(pkg, **k)
        msg = f"{k} -> {pl}"
        w, w2 = k["w"], k["w"] // 2
        es = 4 if pl["wide"] else 2
        nc = pl["TX"] + 2 * w2
        stage_l, stage_r = (nc + 3) & ~3, (nc + pl["Dp"] + 3) & ~3
        assert pl["nk"] == (k["D"] + 63) // 64 and pl["Dp"] == 64 * pl["nk"], msg
        assert pl["rows"] == k["H"] - 2 * w2 and pl["rows"] >= 1, msg
        x0, x1 = max(k["D"] - 1 + k["m"], 0), min(k["W"], k["W"] + k["m"])
        assert pl["width1"] == max(x1 - x0, 0), msg
        width1 = max(pl["width1"], 1)
        assert 1 <= pl["TX"] <= 128, msg
        assert (pl["nsx"] - 1) * pl["TX"] < width1 <= pl["nsx"] * pl["TX"], msg
        assert (pl["nsy"] - 1) * pl["RB"] < pl["rows"] <= pl["nsy"] * pl["RB"], msg
        assert pl["waves"] in (8, 16) and (pl["waves"] == 8 or pl["nk"] <= 16), msg
        assert pl["lds"] <= LDS_CU, msg
        assert pl["vglobal"] or pl["lds"] <= LDS_BUDGET + 2 * stage_l + 2 * stage_r, msg
        assert pl["wide"] == (1 if w * w * 2 * k["cap"] > 65535 else 0), msg
        # w + 3 strip columns (a window and three outputs) of column sums, texture sum and staged
        # bytes, with the staged right segments' D bytes and padding
        fits = (w + 3) * (pl["Dp"] * es + 8) + 2 * (pl["Dp"] + 8) + 16 <= LDS_BUDGET
        assert pl["vglobal"] == (1 if forced or not fits else 0), msg
        assert pl["lds"] == nc * 4 + 2 * stage_l + 2 * stage_r + (0 if pl["vglobal"] else nc * pl["Dp"] * es), msg
        seen["vglobal"] += pl["vglobal"]
        seen["wide"] += pl["wide"]
        seen["w16"] += pl["waves"] == 16
        seen["halved"] += 32 < pl["TX"] < 100
        seen["full"] += pl["TX"] >= 100
        seen["empty"] += pl["width1"] == 0
    print(seen)
    # the sweep reaches both sides of every rule it checks
    assert seen["wide"] and seen["empty"] and seen["vglobal"] and (forced or (seen["w16"] and seen["halved"] and
                                                                              seen["full"]))
    assert forced or seen["vglobal"] < 2500


# H, W, minD, D, window at cap 31 -> TX, nsx, nsy, RB, waves on a 256-CU device. A change of the
# heuristic changes these on purpose, and GPU cases under the new plans belong with it.
PRODUCTION = [
    ((480, 640, 9, 64, 15), (32, 18, 32, 15, 8)),             # the node's defaults: a last band of one row
    ((2048, 2448, 147, 480, 21), (102, 18, 14, 145, 16)),     # the shipped launch frame
    ((1080, 1920, 0, 128, 15), (120, 15, 67, 16, 8)),
    ((1080, 1920, 0, 256, 21), (119, 14, 36, 30, 16)),
    ((3000, 4096, 0, 512, 21), (103, 35, 7, 426, 16)),
]


@pytest.mark.parametrize("frame,expect", PRODUCTION, ids=[f"{f[0]}x{f[1]}_D{f[3]}" for f, _ in PRODUCTION])
def test_production_plans_are_pinned(pkg, monkeypatch, frame, expect):
    clean_env(monkeypatch)
    H, W, m, D, w = frame
    pl = plan(pkg, H, W, m, D, w, 31, 256)
    assert (pl["TX"], pl["nsx"], pl["nsy"], pl["RB"], pl["waves"]) == expect, pl
    assert not pl["vglobal"] and not pl["wide"]
    if frame[:2] == (480, 640):
        assert pl["rows"] - (pl["nsy"] - 1) * pl["RB"] == 1 and pl["lds"] < 8 * 1024
    if frame[:2] == (2048, 2448):
        assert 120 * 1024 <= pl["lds"] <= LDS_BUDGET


def test_small_frames_never_plan_wide_strips(pkg, monkeypatch):
    """Why the explicit-sum reference cannot reach the production tilings: at 256 CUs a frame of up to
    2.5 M volume cells (about 10 s of tests/bm_reference.py) is never planned with a strip wider than 32
    columns, while the production frames above get 102 to 120. The frames of tests/bm_tiling_cases.py
    (13 M to 484 M cells, for the box-sum reference) are."""
    clean_env(monkeypatch)
    rng = np.random.default_rng(77)
    n = 0
    while n < 500:
        k = dict(draw(rng), n_cu=256)
        pl = plan(pkg, **k)
        if pl["vglobal"] or pl["rows"] * pl["width1"] * k["D"] > 2_500_000:
            continue
        n += 1
        assert pl["TX"] <= 32, f"{k} -> {pl}"


def test_plan_entry_point_errors(pkg):
    lib = pkg.load_library()
    out = (ctypes.c_int * 12)(*([-7] * 12))
    b = pkg.default_bm_params()

    def call(p, bm=b, W=640, H=480):
        return lib.sgm_debug_bm_plan(ctypes.byref(p), ctypes.byref(bm), W, H, 256, ctypes.byref(out))

    ok = bm_params(pkg, 9, 64, 15, 31)
    assert lib.sgm_debug_bm_plan(None, ctypes.byref(b), 640, 480, 256, ctypes.byref(out)) == pkg.SGM_ERR_ARG
    assert lib.sgm_debug_bm_plan(ctypes.byref(ok), None, 640, 480, 256, ctypes.byref(out)) == pkg.SGM_ERR_ARG
    assert lib.sgm_debug_bm_plan(ctypes.byref(ok), ctypes.byref(b), 640, 480, 256, None) == pkg.SGM_ERR_ARG
    assert call(pkg.default_params(pkg.MODE_OCV_SGBM5)) == pkg.SGM_ERR_ARG
    # what a match would return (sgm_check_bm_params)
    for kw, bkw, W, H in ((dict(block_size=14), {}, 640, 480), (dict(num_disparities=40), {}, 640, 480),
                          (dict(prefilter_cap=64), {}, 640, 480), ({}, dict(prefilter_size=8), 640, 480),
                          (dict(disp12_max_diff=1), {}, 640, 480), (dict(num_disparities=2064), {}, 4096, 3000),
                          ({}, {}, 100, 15), ({}, {}, 0, 480)):
        p, bm = pkg.default_params(pkg.MODE_OCV_BM, **kw), pkg.default_bm_params(**bkw)
        rc = call(p, bm, W, H)
        assert rc != pkg.SGM_OK and rc == lib.sgm_check_bm_params(ctypes.byref(p), ctypes.byref(bm), W, H), (kw, bkw)
    assert list(out) == [-7] * 12                       # nothing written on an error
    assert call(ok) == pkg.SGM_OK and list(out)[:5] != [-7] * 5
    with pytest.raises(pkg.SGMError):
        pkg.bm_plan(pkg.default_params(pkg.MODE_OCV_BM, block_size=14), b, 640, 480, 256)
