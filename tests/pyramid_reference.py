"""The half-resolution pyramid level in numpy: the executable statement of sgm_pyramid_params.

Level 1 of a W x H frame under (m = min_disparity, D = num_disparities):
  plan()    the coarse geometry (Wc, Hc, mc, Dc) and the two invalid values
  down()    the 2x2 box average with replicate clamping, rounded to nearest
  refine()  around twice each coarse disparity, the +-radius full-resolution disparities compared
            on 3x3 sums of 5x5 census Hamming distances of the full-resolution images
  fill_rect() the rectangle the hole filter works on after the refinement
Everything between down() and refine() is an ordinary level-0 match of the coarse pair with
(mc, Dc) and hole filling off. Test infrastructure only: nothing in the package imports it.
"""
import numpy as np


def plan(W, H, m, D):
    """(Wc, Hc, mc, Dc, invalid_c, invalid) of a level-1 match; >> is the arithmetic shift."""
    mc = m >> 1
    span = ((m + D - 1) >> 1) - mc + 1
    Dc = 16 * ((span + 15) // 16)
    return ((W + 1) >> 1, (H + 1) >> 1, mc, Dc, (mc - 1) * 16, (m - 1) * 16)


def down(img):
    """Ic(xc, yc) = (I(x0,y0) + I(x1,y0) + I(x0,y1) + I(x1,y1) + 2) >> 2, x1 = min(2xc + 1, W - 1)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    Hc, Wc = (H + 1) >> 1, (W + 1) >> 1
    x0 = 2 * np.arange(Wc)
    y0 = 2 * np.arange(Hc)
    x1 = np.minimum(x0 + 1, W - 1)
    y1 = np.minimum(y0 + 1, H - 1)
    a = img.astype(np.int32)
    s = a[np.ix_(y0, x0)] + a[np.ix_(y0, x1)] + a[np.ix_(y1, x0)] + a[np.ix_(y1, x1)]
    return ((s + 2) >> 2).astype(np.uint8)


def census5(img):
    """24-bit 5x5 census codes (uint32): raster over dy = -2..2, dx = -2..2, centre skipped, LSB
    first; bit = I(clamp(y + dy), clamp(x + dx)) < I(y, x)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    p = np.pad(img, 2, mode="edge")
    code = np.zeros((H, W), np.uint32)
    bit = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy == 0 and dx == 0:
                continue
            nb = p[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
            code |= (nb < img).astype(np.uint32) << np.uint32(bit)
            bit += 1
    return code


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _popcount32(v):
    return _POP8[v & 0xFF] + _POP8[(v >> 8) & 0xFF] + _POP8[(v >> 16) & 0xFF] + _POP8[(v >> 24) & 0xFF]


def _h(KL, KR, d):
    """h(x, y, d) for a per-pixel disparity image d (int array, any values)."""
    H, W = KL.shape
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((H, W), np.int32)
    for j in (-1, 0, 1):
        yy = np.clip(ys + j, 0, H - 1)
        for i in (-1, 0, 1):
            xl = np.clip(xs + i, 0, W - 1)
            xr = np.clip(xs + i - d, 0, W - 1)
            out += _popcount32(KL[yy, xl] ^ KR[yy, xr])
    return out


def refine(left, right, coarse, m, D, mc, radius, subpixel):
    """Step 4 of the specification: int16 W x H disparity from the coarse int16 image."""
    left = np.asarray(left, np.uint8)
    right = np.asarray(right, np.uint8)
    H, W = left.shape
    coarse = np.asarray(coarse, np.int16)
    assert coarse.shape == ((H + 1) >> 1, (W + 1) >> 1)
    KL, KR = census5(left), census5(right)
    ys, xs = np.mgrid[0:H, 0:W]
    c = coarse[ys >> 1, xs >> 1].astype(np.int32)
    invalid = (m - 1) * 16
    live = c != (mc - 1) * 16
    live &= (xs >= max(m + D, 0)) & (xs < W + min(m, 0))
    d0 = (2 * c + 8) >> 4
    big = np.int32(1 << 20)
    best = np.full((H, W), big, np.int32)
    dstar = np.zeros((H, W), np.int32)
    order = [0]
    for k in range(1, radius + 1):
        order += [-k, k]
    for k in order:
        d = d0 + k
        ok = live & (d >= m) & (d <= m + D - 1)
        hk = _h(KL, KR, d)
        win = ok & (hk < best)
        best = np.where(win, hk, best)
        dstar = np.where(win, d, dstar)
    found = best < big
    off = np.zeros((H, W), np.int32)
    if subpixel:
        inner = found & (dstar > m) & (dstar < m + D - 1)
        cm = _h(KL, KR, dstar - 1)
        cp = _h(KL, KR, dstar + 1)
        den = cm + cp - 2 * best
        use = inner & (cm >= best) & (cp >= best) & (den > 0)
        num = (cm - cp) * 16 + den
        den2 = np.where(use, 2 * den, 1)
        q = np.abs(num) // den2                      # C division truncates towards zero
        off = np.where(use, np.where(num < 0, -q, q), 0)
    out = np.where(found, dstar * 16 + off, invalid)
    return out.astype(np.int16)


def fill_rect(bm, m, D, block, W, H):
    """The hole filter's rectangle (x0, y0, x1, y1) after a level-1 match: the full-resolution
    columns, all rows, and for BM the rows the coarse match computes, doubled."""
    x0, x1 = max(m + D, 0), W + min(m, 0)
    if x1 <= x0:
        return (0, 0, 0, 0)
    if not bm:
        return (x0, 0, x1, H)
    Hc = (H + 1) >> 1
    y0 = min(2 * (block // 2), H)
    return (x0, y0, x1, max(min(H, 2 * (Hc - block // 2)), y0))


def upsample2(coarse, W, H, mc, m):
    """The plain x2 upsample the refinement is compared with: twice the coarse value per pixel."""
    ys, xs = np.mgrid[0:H, 0:W]
    c = np.asarray(coarse, np.int16)[ys >> 1, xs >> 1].astype(np.int32)
    return np.where(c == (mc - 1) * 16, (m - 1) * 16, 2 * c).astype(np.int16)


# ---------------------------------------------------------------- known answers (tests/golden/pyramid)
KAT_SHAPES = {"a": (5, 23), "b": (8, 30), "c": (13, 41)}


def kat_inputs(name):
    """The seeded inputs of known-answer case `name`: left, right, coarse and (m, D, radius, subpixel)."""
    H, W = KAT_SHAPES[name]
    rng = np.random.default_rng({"a": 101, "b": 202, "c": 303}[name])
    left = rng.integers(0, 256, (H, W)).astype(np.uint8)
    right = np.roll(left, -2, axis=1) if name != "a" else rng.integers(0, 256, (H, W)).astype(np.uint8)
    m, D, radius, sub = {"a": (0, 16, 1, 0), "b": (-5, 16, 2, 1), "c": (3, 16, 2, 1)}[name]
    Wc, Hc, mc, _, inv_c, _ = plan(W, H, m, D)
    coarse = rng.integers((m - 3) * 8, (m + D + 2) * 8 + 1, (Hc, Wc)).astype(np.int16)
    coarse[rng.random((Hc, Wc)) < 0.3] = inv_c
    return left, right, coarse, (m, D, radius, sub)


def make_kat():
    """What tests/golden/pyramid/pyramid_kat.npz holds."""
    out = {}
    for name in sorted(KAT_SHAPES):
        left, right, coarse, (m, D, radius, sub) = kat_inputs(name)
        mc = m >> 1
        out[name + "_left"], out[name + "_right"], out[name + "_coarse"] = left, right, coarse
        out[name + "_par"] = np.array([m, D, radius, sub], np.int32)
        out[name + "_down"] = down(left)
        out[name + "_code"] = census5(left)
        out[name + "_out"] = refine(left, right, coarse, m, D, mc, radius, sub)
    return out


if __name__ == "__main__":
    import os
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyramid")
    os.makedirs(dst, exist_ok=True)
    np.savez_compressed(os.path.join(dst, "pyramid_kat.npz"), **make_kat())
