"""Reference of the census mode with a selectable census window (sgm_set_census_window).

The executable statement of the window semantics (include/sgm_hip.h): numpy census codes for any
(taps_x, taps_y, step), a numpy Hamming cost volume and the 8-direction path recurrence transcribed
from oracle/sgm_oracle.c (census_step / census_path: path start L = C, direction table kDirRX /
kDirRY), then the oracle's own WTA, 3x3 median and speckle filter, composed like
census_paths_reference.match_paths. With the window (9, 7, 1) every stage equals the oracle's bit
for bit (tests/test_census_window_reference.py).
"""
import numpy as np

DEFAULT = (9, 7, 1)
WINDOWS = [(tx, ty, s) for s in (1, 2) for ty in (3, 5, 7) for tx in (3, 5, 7, 9)]     # the 24 valid ones
DIR_RX = (0, 0, 1, -1, 1, -1, 1, -1)       # oracle/sgm_oracle.c kDirRX / kDirRY: L(p) depends on L(p - r)
DIR_RY = (1, -1, 1, 1, -1, -1, 0, 0)


def bit_index(dy, dx):
    """Bit of the offset (dy, dx) in the 9x7 code: raster over dy = -3..3, dx = -4..4, centre skipped."""
    i = (dy + 3) * 9 + (dx + 4)
    return i - (1 if i > 31 else 0)


def mask(taps_x, taps_y):
    """The bits a taps_x x taps_y window has."""
    m = 0
    for j in range(-(taps_y // 2), taps_y // 2 + 1):
        for i in range(-(taps_x // 2), taps_x // 2 + 1):
            if (j, i) != (0, 0):
                m |= 1 << bit_index(j, i)
    return m


def census(img, window=DEFAULT):
    """uint64 codes: tap (j, i) sets bit_index(j, i) iff I(clamp(y + step*j), clamp(x + step*i)) < I(y, x)."""
    tx, ty, step = window
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    ys, xs = np.arange(h), np.arange(w)
    out = np.zeros((h, w), np.uint64)
    for j in range(-(ty // 2), ty // 2 + 1):
        rows = img[np.clip(ys + step * j, 0, h - 1)]
        for i in range(-(tx // 2), tx // 2 + 1):
            if (j, i) == (0, 0):
                continue
            tap = rows[:, np.clip(xs + step * i, 0, w - 1)]
            out |= (tap < img).astype(np.uint64) << np.uint64(bit_index(j, i))
    return out


def _popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(-1, dtype=np.int32)


def cost_volume(e, cL, cR):
    """C[y, x1, d] = popcount(cL[y, x] ^ cR[y, x - minD - d]), x = x1 + minX1 (int32)."""
    D, w1 = e["D"], e["width1"]
    x = np.arange(w1)[:, None] + e["minX1"]
    idx = x - e["minD"] - np.arange(D)[None, :]
    return _popcount(cL[:, e["minX1"]:e["minX1"] + w1, None] ^ cR[:, idx])


def _step(C, Lp, P1, P2):
    """census_step for a batch of pixels: C, Lp [..., D] int32 -> L."""
    mn = Lp.min(-1, keepdims=True)
    best = np.minimum(Lp, mn + P2)
    best[..., 1:] = np.minimum(best[..., 1:], Lp[..., :-1] + P1)
    best[..., :-1] = np.minimum(best[..., :-1], Lp[..., 1:] + P1)
    return C + best - mn


def path_volume(e, C, direction):
    """u8 path volume [H][width1][D] of one direction (census_path)."""
    rx, ry = DIR_RX[direction], DIR_RY[direction]
    h, w1, _ = C.shape
    L = np.empty_like(C)
    if ry == 0:
        order = range(w1) if rx > 0 else range(w1 - 1, -1, -1)
        prev = None
        for x1 in order:
            L[:, x1] = C[:, x1] if prev is None else _step(C[:, x1], L[:, prev], e["P1"], e["P2"])
            prev = x1
    else:
        order = range(h) if ry > 0 else range(h - 1, -1, -1)
        prev = None
        for y in order:
            L[y] = C[y]                                    # path starts: L = C
            if prev is not None:
                lo, hi = max(rx, 0), w1 + min(rx, 0)       # pixels whose predecessor x1 - rx is inside
                if hi > lo:
                    L[y, lo:hi] = _step(C[y, lo:hi], L[prev, lo - rx:hi - rx], e["P1"], e["P2"])
            prev = y
    assert L.max(initial=0) <= 255
    return L.astype(np.uint8)


def census_path(oracle, p, left, right, direction, window=DEFAULT):
    left = np.ascontiguousarray(left, np.uint8)
    right = np.ascontiguousarray(right, np.uint8)
    h, w = left.shape
    e = oracle.effective(p, w, h)
    if e["width1"] <= 0:
        return np.zeros((h, 0, e["D"]), np.uint8)
    return path_volume(e, cost_volume(e, census(left, window), census(right, window)), direction)


def match(oracle, p, left, right, window=DEFAULT, dirs=range(8)):
    """Disparity (int16, x16) of the census pipeline of parameters p (an oracle SgmParams) with
    census window `window`, aggregating over the directions `dirs`."""
    left = np.ascontiguousarray(left, np.uint8)
    right = np.ascontiguousarray(right, np.uint8)
    h, w = left.shape
    e = oracle.effective(p, w, h)
    if e["width1"] <= 0:
        return np.full((h, w), e["invalid"], np.int16)
    C = cost_volume(e, census(left, window), census(right, window))
    S = np.zeros(C.shape, np.uint16)
    for d in dirs:
        S += path_volume(e, C, d)
    disp = oracle.wta(p, S, w)
    if e["median"]:
        disp = oracle.median3(disp)
    if p.speckle_window_size > 0:
        disp = oracle.filter_speckles(disp, e["invalid"], p.speckle_window_size, 16 * p.speckle_range)
    return disp
