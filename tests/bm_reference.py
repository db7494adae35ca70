"""numpy reference of MODE_OCV_BM (cv::StereoBM as restated in DESIGN.md, BM section), written
directly from that definition: every SAD is an explicit double sum over the clamped window, there
are no sliding sums, and nothing is shared with the kernel or the package. Test infrastructure
only. Unverified against a real OpenCV (none is available to this project); the three points
where OpenCV releases may differ are marked in DESIGN.md.

    bm = BM(min_disparity, num_disparities, block_size, prefilter_cap, texture_threshold, uniqueness_ratio)
    disp = compute(bm, left, right)            int16, x16 fixed point, FILTERED = (m - 1) * 16
"""
import collections

import numpy as np

BM = collections.namedtuple("BM", "m D w c t u")


def filtered(bm):
    return (bm.m - 1) * 16


def prefilter(img, cap):
    """XSOBEL: clamp(dx(ya) + 2 dx(y) + dx(yb), -c, c) + c, rows reflect-101, columns 0 and W-1 = c,
    and the whole last row = c when H is odd."""
    I = np.asarray(img).astype(np.int64)
    H, W = I.shape
    P = np.full((H, W), cap, np.int64)
    for y in range(H):
        if H % 2 == 1 and y == H - 1:
            continue
        ya = y - 1 if y > 0 else 1
        yb = y + 1 if y < H - 1 else H - 2
        s = (I[ya, 2:] - I[ya, :-2]) + 2 * (I[y, 2:] - I[y, :-2]) + (I[yb, 2:] - I[yb, :-2])
        P[y, 1:W - 1] = np.clip(s, -cap, cap) + cap
    return P.astype(np.uint8)


def column_range(bm, W):
    """(X0, X1), or None when no column is computed."""
    s = bm.D - 1 + bm.m
    x0, x1 = max(s, 0), min(W, W + bm.m)
    if x0 >= W or x1 <= 0 or x1 <= x0:
        return None
    return x0, x1


def sad_volume(bm, PL, PR):
    """(SAD [H - 2 w2][X1 - X0][D] indexed by e = D - 1 - (d - m), texture [H - 2 w2][X1 - X0]) over
    rows [w2, H - w2) and columns [X0, X1); None when the column range is empty."""
    PL = np.asarray(PL).astype(np.int64)
    PR = np.asarray(PR).astype(np.int64)
    H, W = PL.shape
    rng = column_range(bm, W)
    if rng is None:
        return None
    w2 = bm.w // 2
    s = bm.D - 1 + bm.m
    xs = np.arange(rng[0], rng[1])
    ys = np.arange(w2, H - w2)
    e = np.arange(bm.D)
    sad = np.zeros((len(ys), len(xs), bm.D), np.int64)
    tex = np.zeros((len(ys), len(xs)), np.int64)
    for j in range(-w2, w2 + 1):
        for i in range(-w2, w2 + 1):
            lc = np.clip(xs + i, 0, W - 1)
            rc = np.clip(xs + i - s, 0, W - bm.D)[:, None] + e[None, :]     # d = m + D - 1 - e
            l = PL[ys + j][:, lc]
            r = PR[(ys + j)[:, None, None], rc[None, :, :]]
            sad += np.abs(l[:, :, None] - r)
            tex += np.abs(l - bm.c)
    return sad, tex


def compute(bm, left, right, return_stages=False):
    left = np.asarray(left)
    H, W = left.shape
    F = filtered(bm)
    out = np.full((H, W), F, np.int64)
    PL, PR = prefilter(left, bm.c), prefilter(right, bm.c)
    vol = sad_volume(bm, PL, PR)
    if vol is None:
        return (out.astype(np.int16), None, None) if return_stages else out.astype(np.int16)
    sad, tex = vol
    D, w2 = bm.D, bm.w // 2
    x0, x1 = column_range(bm, W)
    mind = np.argmin(sad, axis=2)                       # first minimum: strict '<' scanning e upwards
    minsad = np.take_along_axis(sad, mind[:, :, None], 2)[:, :, 0]
    ok = tex >= bm.t
    if bm.u > 0:
        thr = minsad + minsad * bm.u // 100
        e = np.arange(D)[None, None, :]
        outside = (e < mind[:, :, None] - 1) | (e > mind[:, :, None] + 1)
        ok &= ~np.any(outside & (sad <= thr[:, :, None]), axis=2)
    ep = np.where(mind + 1 < D, mind + 1, D - 2)        # SAD[D] := SAD[D - 2]
    en = np.where(mind > 0, mind - 1, 1)                # SAD[-1] := SAD[1]
    p = np.take_along_axis(sad, ep[:, :, None], 2)[:, :, 0]
    n = np.take_along_axis(sad, en[:, :, None], 2)[:, :, 0]
    q = p + n - 2 * minsad + np.abs(p - n)
    num = (p - n) * 256
    frac = np.where(q != 0, np.sign(num) * (np.abs(num) // np.maximum(q, 1)), 0)   # C division
    val = ((D - mind - 1 + bm.m) * 256 + frac + 15) >> 4
    out[w2:H - w2, x0:x1] = np.where(ok, val, F)
    out = out.astype(np.int16)
    return (out, sad, tex) if return_stages else out


def valid_share(bm, disp):
    """Share of valid pixels over rows [w2, H - w2) x columns [X0 + w2, X1 - w2)."""
    H, W = disp.shape
    w2 = bm.w // 2
    x0, x1 = column_range(bm, W)
    core = disp[w2:H - w2, x0 + w2:x1 - w2]
    return float((core != filtered(bm)).mean())
