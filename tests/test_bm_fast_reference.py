"""CPU tests of tests/bm_fast_reference.py, the box-sum reference of MODE_OCV_BM for frames large
enough to be planned like production frames: it equals the explicit-sum reference
tests/bm_reference.py bit for bit on seeded random configurations and on the edges of the definition,
and the frames of tests/bm_tiling_cases.py are planned at 256 CUs as that table says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm_fast_reference as bf  # noqa: E402
import bm_reference as br  # noqa: E402
import bm_tiling_cases as tc  # noqa: E402


def noise_pair(rng, H, W):
    """test_bm_fuzz's frames: smoothed noise, the right image shifted with 5 % outliers."""
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    left = ((left.astype(np.int32) + np.roll(left, 1, 1) + np.roll(left, 1, 0) + 1) // 3).astype(np.uint8)
    right = np.roll(left, -int(rng.integers(0, 9)), 1)
    right = np.where(rng.random((H, W)) < 0.05, rng.integers(0, 256, (H, W)), right).astype(np.uint8)
    return left, right


def same(bm, left, right, what):
    slow, fast = br.compute(bm, left, right), bf.compute(bm, left, right)
    assert fast.dtype == np.int16 and fast.shape == slow.shape
    bad = np.argwhere(fast != slow)
    assert not len(bad), f"{what}: {len(bad)} pixels differ, first {bad[:5].tolist()}"
    return slow


@pytest.mark.parametrize("part", range(4))
def test_equals_slow_reference_on_random_configurations(part):
    """4 x 50 configurations drawn like test_gpu_bm.test_bm_fuzz: w 5-25, D 16-128, m -48..32."""
    rng = np.random.default_rng(31337 + part)
    valid = 0
    for it in range(50):
        w = int(rng.choice(np.arange(5, 27, 2)))
        H = int(rng.integers(w + 1, 65))
        D = int(rng.choice([16, 32, 48, 64, 80, 96, 112, 128]))
        W = int(rng.integers(max(w + 1, 24), 193))
        m = int(rng.integers(-48, 33))
        bm = br.BM(m, D, w, int(rng.integers(1, 64)), int(rng.choice([0, 10, 200])), int(rng.choice([0, 5, 15])))
        left, right = noise_pair(rng, H, W)
        ref = same(bm, left, right, f"part {part} iteration {it} {bm} {H}x{W}")
        valid += int((ref != br.filtered(bm)).any())
    assert valid >= 25                                  # most draws compute something


# H, W, BM(m, D, w, c, t, u)
EDGES = {
    "s<0": (33, 70, br.BM(-40, 16, 5, 31, 10, 15)),
    "X0=0": (40, 90, br.BM(-20, 16, 9, 31, 10, 15)),            # left clamp below 0, right clamp at W - D
    "X1=W": (40, 90, br.BM(4, 32, 9, 31, 10, 15)),              # left clamp at W - 1, right clamp below 0
    "D48": (47, 160, br.BM(3, 48, 21, 63, 10, 15)),
    "odd_H": (41, 90, br.BM(-8, 16, 5, 7, 10, 2)),
    "u0_t0": (48, 96, br.BM(0, 32, 9, 31, 0, 0)),
    "u32": (40, 120, br.BM(0, 80, 23, 63, 10, 15)),             # 529 * 126 > 65535
    "t_high": (48, 96, br.BM(0, 32, 9, 31, 2000, 15)),          # the texture test rejects pixels
    "empty": (30, 40, br.BM(0, 48, 5, 31, 10, 15)),
    "single_column": (24, 64, br.BM(0, 64, 5, 31, 0, 0)),
    "two_rows": (10, 64, br.BM(0, 16, 9, 31, 0, 0)),             # H = w + 1, the smallest valid height
}


@pytest.mark.parametrize("name", list(EDGES))
def test_equals_slow_reference_on_edges(synth, name):
    H, W, bm = EDGES[name]
    left, right, _ = synth.stereo_pair(H, W, bm.m, bm.D, seed=len(name))
    rng = br.column_range(bm, W)
    w2, s = bm.w // 2, bm.D - 1 + bm.m
    # each case is the edge its name says
    if name == "s<0":
        assert s < 0
    if name == "X0=0":
        assert rng[0] == 0 and rng[1] < W and rng[1] + w2 - 1 - s > W - bm.D
    if name == "X1=W":
        assert rng[1] == W and rng[0] > 0 and rng[0] - w2 - s < 0
    if name == "D48":
        assert bm.D % 64
    if name == "odd_H":
        assert H % 2
    if name == "u32":
        assert bm.w * bm.w * 2 * bm.c > 65535
    if name == "empty":
        assert rng is None
    if name == "single_column":
        assert rng[1] - rng[0] == 1
    if name == "two_rows":
        assert H - 2 * w2 == 2
    ref = same(bm, left, right, name)
    if name == "empty":
        assert (ref == br.filtered(bm)).all()
    else:
        assert (ref != br.filtered(bm)).any()
    if name == "t_high":
        loose = br.compute(bm._replace(t=0), left, right)
        assert (ref != loose).any()


@pytest.mark.parametrize("name", ["X1=W", "odd_H", "u32", "empty"])
def test_row_slices_equal_the_rows_of_the_whole_frame(synth, name):
    H, W, bm = EDGES[name]
    left, right, _ = synth.stereo_pair(H, W, bm.m, bm.D, seed=len(name))
    full = br.compute(bm, left, right)
    w2 = bm.w // 2
    for y0, y1 in ((0, H), (0, w2 + 1), (w2, H - w2), (w2 + 3, w2 + 4), (H - w2 - 2, H), (H - 1, H), (5, 5), (0, 1)):
        got = bf.compute(bm, left, right, rows=(y0, y1))
        assert got.shape == (y1 - y0, W) and np.array_equal(got, full[y0:y1]), (name, y0, y1)


def test_row_bands_do_not_change_the_result(synth, monkeypatch):
    """compute cuts large frames into row bands; with a tiny band budget a small frame is cut too."""
    H, W, bm = EDGES["D48"]
    left, right, _ = synth.stereo_pair(H, W, bm.m, bm.D, seed=3)
    whole = bf.compute(bm, left, right)
    rng = br.column_range(bm, W)
    per_row = (rng[1] - rng[0] + 2 * (bm.w // 2)) * bm.D
    for rows_per_band in (1, 2, 5):
        monkeypatch.setattr(bf, "BAND_CELLS", per_row * (rows_per_band + 2 * (bm.w // 2)))
        assert np.array_equal(bf.compute(bm, left, right), whole), rows_per_band
    assert np.array_equal(whole, br.compute(bm, left, right))


def test_sad_volume_and_texture_equal_the_explicit_sums(synth):
    H, W, bm = EDGES["X1=W"]
    left, right, _ = synth.stereo_pair(H, W, bm.m, bm.D, seed=1)
    PL, PR = br.prefilter(left, bm.c), br.prefilter(right, bm.c)
    sad, tex = br.sad_volume(bm, PL, PR)
    fsad, ftex = bf.sad_volume(bm, PL, PR)
    assert fsad.dtype == np.int32 and fsad.shape == sad.shape and ftex.shape == tex.shape
    assert np.array_equal(fsad, sad) and np.array_equal(ftex, tex)
    w2 = bm.w // 2
    part = bf.sad_volume(bm, PL, PR, rows=(w2 + 2, w2 + 9))
    assert np.array_equal(part[0], sad[2:9]) and np.array_equal(part[1], tex[2:9])


# ------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("c", tc.CASES, ids=[c.name for c in tc.CASES])
def test_tiling_cases_are_planned_as_listed(pkg, monkeypatch, c):
    """bm_plan at 256 CUs (host-only) gives each frame of the table the listed plan, and that plan has
    the property the case is there for."""
    monkeypatch.delenv("SGM_BM_VGLOBAL", raising=False)
    H, W, m, D, w, cap = c.frame
    pl = tc.plan_of(pkg, c.frame, 256)
    assert (pl["TX"], pl["nsx"], pl["nsy"], pl["RB"], pl["waves"], pl["lds"]) == c.plan, pl
    assert not tc.misses(pl, c.prop), (tc.misses(pl, c.prop), pl)
    last_strip = pl["width1"] - (pl["nsx"] - 1) * pl["TX"]
    last_band = pl["rows"] - (pl["nsy"] - 1) * pl["RB"]
    if c.name == "A":
        assert last_strip == 100
    if c.name == "E":
        assert (last_strip, last_band) == (48, 9)
    if c.name == "C":
        assert (last_strip, last_band) == (57, 7) and m < 0
    if c.name == "D":
        # the compared rows: both bands of the first, a middle and the last pair, at least a fifth
        w2, RB, nsy = w // 2, pl["RB"], pl["nsy"]
        pairs = [(w2 + b * RB, min(w2 + (b + 2) * RB, H - w2)) for b in (0, nsy // 2 - 1, nsy - 2)]
        assert pairs == tc.D_ROWS
        assert sum(y1 - y0 for y0, y1 in tc.D_ROWS) * 5 >= pl["rows"]
    if c.name == "G":
        # 8 waves prefetch 4 bytes per thread: the commit's tail loop runs past 2048 staged bytes
        assert tc.staged_bytes(pl, c.frame) > 4 * 64 * pl["waves"] == 2048
    if c.name == "H":
        assert D % 64 and pl["nk"] == 32
    if c.name in "ABCDE":
        # planned like a production frame without being one: within the fast reference's reach
        assert pl["rows"] * pl["width1"] * D < 500_000_000


def test_frames_of_the_slow_reference_reach_none_of_it(pkg, monkeypatch):
    """Why the table is needed: the frames test_gpu_bm.py compares (all affordable for the explicit-sum
    reference) are planned at 256 CUs with strips of at most 32 columns, LDS column sums and at most
    2048 staged bytes per row. Two of them launch with more than 64 KB of LDS, both with u32 sums and
    narrow strips (16 waves at 67 KB, D = 272; 8 waves at 126 KB, D = 1040); no u16 kernel does."""
    monkeypatch.delenv("SGM_BM_VGLOBAL", raising=False)
    big = {}
    for frame in ((48, 96, 0, 32, 9, 31), (64, 128, 9, 64, 15, 31), (41, 90, -8, 16, 5, 7), (47, 160, 3, 48, 21, 63),
                  (33, 70, -40, 16, 5, 31), (56, 333, 0, 272, 23, 63), (20, 600, 0, 528, 5, 31),
                  (20, 1100, -3, 1040, 5, 63), (30, 1100, 0, 1040, 23, 63)):
        pl = tc.plan_of(pkg, frame, 256)
        assert pl["TX"] <= 32 and not pl["vglobal"] and tc.staged_bytes(pl, frame) <= 2048, (frame, pl)
        if pl["lds"] > 64 * 1024:
            big[frame] = (pl["TX"], pl["waves"], pl["lds"], pl["wide"])
        else:
            assert pl["waves"] == 8, (frame, pl)
    assert big == {(56, 333, 0, 272, 23, 63): (31, 16, 68916, 1), (30, 1100, 0, 1040, 23, 63): (7, 8, 128628, 1)}
