"""numpy statement of the hole-filling post filter (include/sgm_hip.h "hole filling", csrc/fill.hip).

A hole is a pixel of the rectangle [x0, x1) x [y0, y1) that equals `invalid`. Each of the 8
directions gives at most one candidate: in[p + k*r] for the smallest k in 1..max_gap for which that
pixel lies inside the image and is not invalid (a diagonal step moves one pixel on both axes).
Candidates are always read from the input. With n candidates sorted v_0 <= .. <= v_{n-1}:
n < min_neighbours stays invalid, BACKGROUND takes v_1 (v_0 when n == 1), MEDIAN takes v_{(n-1)/2},
OFF copies. tests/golden/fill/fill_kat.npz (make_kat below) pins this file.
"""
import numpy as np

OFF, BACKGROUND, MEDIAN = 0, 1, 2
# (dx, dy): left, right, up, down, up-left, up-right, down-left, down-right
DIRS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]
_NONE = np.int32(2 ** 31 - 1)


def candidates(disp, invalid, max_gap):
    """(8, H, W) int32: the candidate of every pixel per direction of DIRS, _NONE where there is none."""
    d = np.asarray(disp, np.int16)
    H, W = d.shape
    out = np.full((8, H, W), _NONE, np.int32)
    for i, (dx, dy) in enumerate(DIRS):
        c = out[i]
        for k in range(1, min(int(max_gap), max(H, W) - 1) + 1):
            sx, sy = k * dx, k * dy
            # destination pixels p whose p + k*r lies inside the image
            ys = slice(max(0, -sy), min(H, H - sy))
            xs = slice(max(0, -sx), min(W, W - sx))
            if ys.start >= ys.stop or xs.start >= xs.stop:
                break
            src = d[ys.start + sy:ys.stop + sy, xs.start + sx:xs.stop + sx]
            dst = c[ys, xs]
            take = (dst == _NONE) & (src != invalid)
            dst[take] = src[take]
    return out


def fill_holes(disp, invalid, mode, max_gap, min_neighbours, rect=None, cands=None):
    """cands: candidates(disp, invalid, max_gap) when the caller already has them."""
    d = np.asarray(disp, np.int16)
    H, W = d.shape
    if mode == OFF:
        return d.copy()
    assert mode in (BACKGROUND, MEDIAN) and 1 <= max_gap <= 255 and 1 <= min_neighbours <= 8
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
    hole = np.zeros((H, W), bool)
    hole[y0:y1, x0:x1] = d[y0:y1, x0:x1] == invalid
    v = np.sort(candidates(d, invalid, max_gap) if cands is None else cands, axis=0)
    n = (v != _NONE).sum(axis=0)
    k = np.where(n >= 2, 1, 0) if mode == BACKGROUND else np.maximum(n - 1, 0) // 2
    pick = np.take_along_axis(v, k[None].astype(np.int64), axis=0)[0]
    out = d.copy()
    ok = hole & (n >= min_neighbours) & (n >= 1)
    out[ok] = pick[ok].astype(np.int16)
    return out


def fill_holes_naive(disp, invalid, mode, max_gap, min_neighbours, rect=None):
    """The specification word for word, pixel by pixel (small images only)."""
    d = np.asarray(disp, np.int16)
    H, W = d.shape
    out = d.copy()
    if mode == OFF:
        return out
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
    for y in range(y0, y1):
        for x in range(x0, x1):
            if d[y, x] != invalid:
                continue
            c = []
            for dx, dy in DIRS:
                for k in range(1, max_gap + 1):
                    xx, yy = x + k * dx, y + k * dy
                    if 0 <= xx < W and 0 <= yy < H and d[yy, xx] != invalid:
                        c.append(int(d[yy, xx]))
                        break
            c.sort()
            n = len(c)
            if n < min_neighbours or n == 0:
                continue
            out[y, x] = (c[1] if n >= 2 else c[0]) if mode == BACKGROUND else c[(n - 1) // 2]
    return out


def match_rect(mode_is_bm, min_disparity, num_disparities, block_size, W, H):
    """(x0, y0, x1, y1) of the fill inside a match: where the mode can produce a disparity (an empty
    rectangle for a frame without a disparity window)."""
    if mode_is_bm:
        x0, x1 = max(num_disparities - 1 + min_disparity, 0), min(W, W + min_disparity)
        sw2 = block_size // 2
        y0, y1 = min(sw2, H), max(H - sw2, min(sw2, H))
    else:
        x0, x1 = max(min_disparity + num_disparities, 0), W + min(min_disparity, 0)
        y0, y1 = 0, H
    if x0 >= W or x1 <= x0:
        return (0, y0, 0, y1)
    return (x0, y0, x1, y1)


def make_kat():
    """The known answers of tests/golden/fill/fill_kat.npz: name -> array (inputs, parameters as int
    arrays [invalid, mode, G, N, x0, y0, x1, y1], outputs)."""
    out = {}
    inv, G = -16, 5
    # a single valid pixel in an all-invalid 41 x 41 image: seen from distance G in each direction,
    # not from G + 1
    img = np.full((41, 41), inv, np.int16)
    img[20, 20] = 777
    out["single_in"] = img
    out["single_par"] = np.array([inv, BACKGROUND, G, 1, 0, 0, 41, 41])
    exp = img.copy()
    for dx, dy in DIRS:
        for k in range(1, G + 1):
            exp[20 + k * dy, 20 + k * dx] = 777
    out["single_out"] = exp
    # a hole whose 8 candidates are 8 distinct values, at distances 1..3: both rules
    img = np.full((9, 9), inv, np.int16)
    vals = [80, 10, 70, 20, 60, 30, 50, 40]
    for i, ((dx, dy), v) in enumerate(zip(DIRS, vals)):
        k = 1 + i % 3
        img[4 + k * dy, 4 + k * dx] = v
    out["eight_in"] = img
    for name, mode, want in (("bg", BACKGROUND, 20), ("med", MEDIAN, 40)):
        out[f"eight_{name}_par"] = np.array([inv, mode, 3, 8, 4, 4, 5, 5])
        exp = img.copy()
        exp[4, 4] = want
        out[f"eight_{name}_out"] = exp
    # n < N: three candidates, four wanted; then three wanted
    img = np.full((7, 7), inv, np.int16)
    img[3, 0], img[0, 3], img[6, 6] = 5, 9, 7
    out["few_in"] = img
    out["few_par"] = np.array([inv, MEDIAN, 3, 4, 3, 3, 4, 4])
    out["few_out"] = img.copy()
    out["few3_par"] = np.array([inv, MEDIAN, 3, 3, 3, 3, 4, 4])
    exp = img.copy()
    exp[3, 3] = 7
    out["few3_out"] = exp
    # a rectangle that excludes holes: only the two holes inside it are filled
    img = np.full((5, 8), 100, np.int16)
    img[2, 1], img[2, 3], img[2, 4], img[2, 6] = inv, inv, inv, inv
    img[1, 3] = 40
    out["rect_in"] = img
    out["rect_par"] = np.array([inv, BACKGROUND, 2, 2, 3, 1, 5, 4])
    exp = img.copy()
    exp[2, 3], exp[2, 4] = 100, 100
    out["rect_out"] = exp
    return out


KAT_CASES = ["single", "eight_bg", "eight_med", "few", "few3", "rect"]


def kat_input(kat, case):
    return kat[{"eight_bg": "eight", "eight_med": "eight", "few3": "few"}.get(case, case) + "_in"]
