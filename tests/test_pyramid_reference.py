"""The pyramid reference (tests/pyramid_reference.py) on the CPU: known answers for the two new
stages (by hand, a per-pixel restatement, and tests/golden/pyramid/pyramid_kat.npz), the plan
formula, and the quality of a level-1 census match composed with the CPU oracle on two frames."""
import os

import numpy as np
import pytest

import pyramid_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pyramid")


# ----------------------------------------------------------------------------------------- down
def test_down_by_hand():
    img = np.array([[0, 1, 10], [2, 4, 20], [255, 255, 7]], np.uint8)
    # (0+1+2+4+2)>>2 = 2; column 2 pairs with itself: (10+10+20+20+2)>>2 = 15;
    # row 2 pairs with itself: (255*4+2)>>2 = 255; the corner is (7*4+2)>>2 = 7
    assert np.array_equal(pr.down(img), np.array([[2, 15], [255, 7]], np.uint8))
    assert np.array_equal(pr.down(np.array([[9]], np.uint8)), np.array([[9]], np.uint8))
    assert np.array_equal(pr.down(np.array([[1, 2, 4]], np.uint8)), np.array([[2, 4]], np.uint8))   # (1+2+1+2+2)>>2
    assert pr.down(np.zeros((7, 1), np.uint8)).shape == (4, 1)


def test_plan_examples():
    assert pr.plan(100, 50, 0, 256)[2:4] == (0, 128)
    assert pr.plan(2448, 2048, 0, 752)[:4] == (1224, 1024, 0, 384)
    assert pr.plan(2448, 2048, 147, 480)[2:] == (73, 256, 72 * 16, 146 * 16)
    assert pr.plan(333, 121, -5, 96) == (167, 61, -3, 64, -64, -96)
    assert pr.plan(9, 1, 3, 16)[2:4] == (1, 16)                  # d 3..18 -> 1..9


# ---------------------------------------------------------------------------------- census, refine
def test_census5_by_hand():
    img = np.full((9, 9), 100, np.uint8)
    img[2, 2] = 10            # offset (-2, -2) of the centre (4, 4): bit 0
    img[4, 5] = 10            # offset (0, 1): bit 12 (the centre is skipped)
    img[6, 6] = 10            # offset (2, 2): bit 23
    assert int(pr.census5(img)[4, 4]) == (1 << 0) | (1 << 12) | (1 << 23)
    assert int(pr.census5(img)[4, 3]) == (1 << 13) | (1 << 1)     # (4, 5) at offset (0, 2); (2, 2) at (-2, -1)
    flat = np.full((3, 2), 7, np.uint8)
    assert not pr.census5(flat).any()
    # a raster ramp: the centre's darker neighbours are the 12 before it; the darkest pixel has none,
    # also among its clamped (replicated) neighbours
    ramp = np.arange(25, dtype=np.uint8).reshape(5, 5)
    assert int(pr.census5(ramp)[2, 2]) == (1 << 12) - 1 and int(pr.census5(ramp)[0, 0]) == 0
    # the brightest pixel, in the corner: every tap that clamps onto the pixel itself reads 0
    assert int(pr.census5(ramp)[4, 4]) == sum(1 << (5 * dy + dx - (5 * dy + dx > 12))
                                              for dy in range(5) for dx in range(5)
                                              if (dy, dx) != (2, 2) and not (dy >= 2 and dx >= 2))


def _refine_naive(left, right, coarse, m, D, mc, radius, subpixel):
    """The specification read pixel by pixel (python ints throughout)."""
    H, W = left.shape
    KL, KR = pr.census5(left), pr.census5(right)

    def h(x, y, d):
        s = 0
        for j in (-1, 0, 1):
            yy = min(max(y + j, 0), H - 1)
            for i in (-1, 0, 1):
                a = int(KL[yy, min(max(x + i, 0), W - 1)])
                b = int(KR[yy, min(max(x + i - d, 0), W - 1)])
                s += bin(a ^ b).count("1")
        return s

    inv = (m - 1) * 16
    out = np.full((H, W), inv, np.int16)
    for y in range(H):
        for x in range(max(m + D, 0), W + min(m, 0)):
            c = int(coarse[y >> 1, x >> 1])
            if c == (mc - 1) * 16:
                continue
            d0 = (2 * c + 8) >> 4
            best = None
            for k in [0] + [s * t for t in range(1, radius + 1) for s in (-1, 1)]:
                d = d0 + k
                if m <= d <= m + D - 1:
                    v = h(x, y, d)
                    if best is None or v < best[0]:
                        best = (v, d)
            if best is None:
                continue
            c0, ds = best
            off = 0
            if subpixel and m < ds < m + D - 1:
                cm, cp = h(x, y, ds - 1), h(x, y, ds + 1)
                den = cm + cp - 2 * c0
                if cm >= c0 and cp >= c0 and den > 0:
                    num = (cm - cp) * 16 + den
                    off = abs(num) // (2 * den) * (1 if num >= 0 else -1)
            out[y, x] = ds * 16 + off
    return out


@pytest.mark.parametrize("name", sorted(pr.KAT_SHAPES))
def test_refine_equals_the_per_pixel_reading(name):
    left, right, coarse, (m, D, radius, sub) = pr.kat_inputs(name)
    want = _refine_naive(left, right, coarse, m, D, m >> 1, radius, sub)
    got = pr.refine(left, right, coarse, m, D, m >> 1, radius, sub)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert (got == (m - 1) * 16).any() and (got != (m - 1) * 16).any()


def test_refine_finds_an_integer_shift(synth):
    """A pair shifted by 7 with a coarse image that says 3 (x2 = 6) or 4 (8) everywhere: both within
    radius 1 of the truth, so every interior pixel comes back as exactly 7."""
    left, right = synth.integer_shift_pair(24, 64, 7, seed=3)
    for cval in (3, 4):
        coarse = np.full((12, 32), cval * 16, np.int16)
        out = pr.refine(left, right, coarse, 0, 16, 0, 1, 0)
        assert (out[:, :16] == -16).all()
        assert (out[3:-3, 20:-3] == 7 * 16).all()
    far = pr.refine(left, right, np.full((12, 32), 1 * 16, np.int16), 0, 16, 0, 2, 0)
    assert (far[3:-3, 20:-3] != 7 * 16).all()                     # 2 +- 2 does not reach 7
    none = pr.refine(left, right, np.full((12, 32), 20 * 16, np.int16), 0, 16, 0, 2, 1)
    assert (none == -16).all()                                    # 40 +- 2 lies outside [0, 15]


def test_golden_file_is_what_the_reference_writes():
    kat = np.load(os.path.join(GOLDEN, "pyramid_kat.npz"))
    fresh = pr.make_kat()
    assert sorted(kat.files) == sorted(fresh)
    for k in kat.files:
        assert np.array_equal(kat[k], fresh[k]) and kat[k].dtype == fresh[k].dtype, k


def test_fill_rect():
    assert pr.fill_rect(False, 3, 64, 0, 330, 120) == (67, 0, 330, 120)
    assert pr.fill_rect(False, -5, 96, 0, 333, 121) == (91, 0, 328, 121)
    assert pr.fill_rect(True, 0, 32, 9, 96, 49) == (32, 8, 96, 42)       # Hc 25: 2 * (25 - 4) = 42
    assert pr.fill_rect(False, 0, 64, 0, 40, 10) == (0, 0, 0, 0)


# --------------------------------------------------------------------------------------- quality
FRAMES = [(120, 330, 0, 64, 5), (121, 333, 3, 96, 9)]


@pytest.mark.parametrize("H,W,m,D,seed", FRAMES)
def test_level1_quality_with_the_oracle(oracle, synth, H, W, m, D, seed):
    """The census mode composed on the CPU: down -> the oracle's match of the coarse pair -> refine
    (radius 2, default census parameters). Mean |error| against the truth over valid pixels."""
    left, right, truth = synth.stereo_pair(H, W, m, D, seed)
    Wc, Hc, mc, Dc, inv_c, inv = pr.plan(W, H, m, D)
    p0 = oracle.make_params(oracle.MODE_CENSUS8, min_disparity=m, num_disparities=D)
    pc = oracle.make_params(oracle.MODE_CENSUS8, min_disparity=mc, num_disparities=Dc)
    lvl0 = oracle.match(p0, left, right)
    coarse = oracle.match(pc, pr.down(left), pr.down(right))
    lvl1 = pr.refine(left, right, coarse, m, D, mc, 2, 1)
    plain = pr.upsample2(coarse, W, H, mc, m)

    def err(d):
        v = d != inv
        return float(np.abs(d[v] / 16.0 - truth[v]).mean()), float(v.mean())      # share of the whole frame

    e0, s0 = err(lvl0)
    e1, s1 = err(lvl1)
    eu, _ = err(plain)
    changed = float((lvl1 != plain)[lvl1 != inv].mean())
    print(f"level0 {e0:.3f} level1 {e1:.3f} upsample {eu:.3f} valid share level1 {s1:.2f} level0 {s0:.2f} "
          f"changed {changed:.2f}")
    assert e1 < 0.5 * eu
    assert e1 <= e0 + 0.05
    assert s1 >= 0.5
