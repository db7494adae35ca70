"""Second numpy reference of MODE_OCV_BM, for frames tests/bm_reference.py cannot afford. Written from
the same definition (BM section), not from the kernel: it must return what
bm_reference.compute returns, bit for bit (tests/test_bm_fast_reference.py holds it to that on seeded
random configurations). Test infrastructure only.

What makes it w^2 times cheaper: with c the unclamped strip column in [X0 - w2, X1 + w2),

    A[y, c, e] = |PL[y, clip(c, 0, W - 1)] - PR[y, clip(c - s, 0, W - D) + e]|

depends on (y, c, e) only, not on the output pixel whose window holds it, so SAD[y, X, e] is the 2-D
box sum of plane e of A over rows [y - w2, y + w2] and strip columns [X - w2, X + w2]: a cumulative
sum along each axis and a difference w apart. The texture sum is the same box over |PL - c|. The sums
are int32 (w^2 * 2c < 2^23). Frames are cut into row bands so that the volume in memory stays small.

    disp = compute(bm, left, right)                     the whole frame
    rows = compute(bm, left, right, rows=(y0, y1))      output rows [y0, y1) only, that slice
"""
import numpy as np

from bm_reference import BM, column_range, filtered, prefilter  # noqa: F401  (BM: for the callers)

BAND_CELLS = 24_000_000         # input rows x strip columns x D of one band: about 0.4 GB at the peak


def _box(a, w):
    """Sums of a over windows of w along axes 0 and 1 (int32): shape (n0 - w + 1, n1 - w + 1, ...)."""
    for axis in (0, 1):
        cs = np.moveaxis(np.cumsum(a, axis=axis, dtype=np.int32), axis, 0)
        a = cs[w - 1:].copy()
        a[1:] -= cs[:len(cs) - w]
        a = np.moveaxis(a, 0, axis)
    return a


def sad_volume(bm, PL, PR, rows=None):
    """(SAD [y1 - y0][X1 - X0][D] indexed by e = D - 1 - (d - m), texture [y1 - y0][X1 - X0]), int32,
    of output rows [y0, y1) (default [w2, H - w2)) from the pre-filtered images; None when the column
    range is empty."""
    PL = np.asarray(PL, np.uint8)
    PR = np.asarray(PR, np.uint8)
    H, W = PL.shape
    rng = column_range(bm, W)
    if rng is None:
        return None
    w2 = bm.w // 2
    y0, y1 = rows if rows is not None else (w2, H - w2)
    assert w2 <= y0 <= y1 <= H - w2
    s = bm.D - 1 + bm.m
    c = np.arange(rng[0] - w2, rng[1] + w2)
    l = PL[y0 - w2:y1 + w2][:, np.clip(c, 0, W - 1)]                         # [row][c]
    seg = np.lib.stride_tricks.sliding_window_view(PR[y0 - w2:y1 + w2], bm.D, axis=1)
    r = seg[:, np.clip(c - s, 0, W - bm.D), :]                               # [row][c][e]
    l3 = l[:, :, None]
    a = np.maximum(l3, r) - np.minimum(l3, r)                                # |l - r| in u8
    tex = np.abs(l.astype(np.int32) - bm.c)
    return _box(a, bm.w), _box(tex, bm.w)


def _wta(bm, sad, tex):
    """Step 5 of the specification on a band's SAD volume: int64 disparities, FILTERED included."""
    D = bm.D
    mind = np.argmin(sad, axis=2)                       # the first minimum in e order

    def at(e):
        return np.take_along_axis(sad, e[:, :, None], 2)[:, :, 0].astype(np.int64)

    minsad = at(mind)
    ok = tex >= bm.t
    if bm.u > 0:
        thr = minsad + minsad * bm.u // 100
        # every e at or below the bound, less those of them inside [mind - 1, mind + 1]
        cnt = np.count_nonzero(sad <= thr[:, :, None], axis=2)
        inside = np.ones(mind.shape, np.int64)          # mind itself: minsad <= thr
        inside += (mind > 0) & (at(np.maximum(mind - 1, 0)) <= thr)
        inside += (mind + 1 < D) & (at(np.minimum(mind + 1, D - 1)) <= thr)
        ok &= cnt == inside
    p = at(np.where(mind + 1 < D, mind + 1, D - 2))     # SAD[D] := SAD[D - 2]
    n = at(np.where(mind > 0, mind - 1, 1))             # SAD[-1] := SAD[1]
    q = p + n - 2 * minsad + np.abs(p - n)
    num = (p - n) * 256
    frac = np.where(q != 0, np.sign(num) * (np.abs(num) // np.maximum(q, 1)), 0)    # C division
    val = ((D - mind - 1 + bm.m) * 256 + frac + 15) >> 4
    return np.where(ok, val, filtered(bm))


def compute(bm, left, right, rows=None):
    left = np.asarray(left)
    H, W = left.shape
    y0, y1 = rows if rows is not None else (0, H)
    assert 0 <= y0 <= y1 <= H
    out = np.full((y1 - y0, W), filtered(bm), np.int64)
    rng = column_range(bm, W)
    w2 = bm.w // 2
    c0, c1 = max(y0, w2), min(y1, H - w2)               # the computed rows of the slice
    if rng is not None and c0 < c1:
        PL, PR = prefilter(left, bm.c), prefilter(right, bm.c)
        per_row = (rng[1] - rng[0] + 2 * w2) * bm.D
        step = max(BAND_CELLS // per_row - 2 * w2, 1)
        for b0 in range(c0, c1, step):
            b1 = min(b0 + step, c1)
            sad, tex = sad_volume(bm, PL, PR, (b0, b1))
            out[b0 - y0:b1 - y0, rng[0]:rng[1]] = _wta(bm, sad, tex)
    return out.astype(np.int16)
