"""A second reference for the stages after the matcher, written from the comments of csrc/post.hip and
csrc/depth.hip and sharing nothing with oracle/: numpy and plain Python.

  median3            medianBlur(3): the middle of the sorted 3x3 neighbourhood, replicate border
  components         explicit 4-connected labelling of {p : d(p) != new_val} with an edge p~q iff
                     |d(p) - d(q)| <= max_diff (union-find over the edge list) -> labels, size map
  filter_speckles    a component of <= max_size pixels becomes new_val
  disparity_to_msg   int16 x16 -> float, MISSING_Z below lo, then above hi
  depth_points       depth_pixel's expressions in its order, every intermediate an np.float32 array
                     (one IEEE rounding per operation, nothing fused), the window compared in float64,
                     points in raster order, rgba packed as k_depth_write packs it

test_post_reference.py holds this file equal to the oracle on the CPU; the GPU edge tests compare the
kernels with both."""
import numpy as np

f32 = np.float32
MISSING_Z = f32(10000.0)


def median3(d):
    d = np.asarray(d, np.int16)
    h, w = d.shape
    ys = np.clip(np.arange(-1, h + 1), 0, h - 1)
    xs = np.clip(np.arange(-1, w + 1), 0, w - 1)
    p = d[np.ix_(ys, xs)]                                     # replicate border
    nine = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.ascontiguousarray(np.sort(nine, axis=0)[4])


def components(d, new_val, max_diff):
    """(labels, sizes): labels int32 HxW, -1 where d == new_val, else the smallest raster index of the
    pixel's component; sizes int32 HxW, the pixel count of the pixel's component (0 where d == new_val)."""
    v = np.asarray(d, np.int16).astype(np.int64)
    h, w = v.shape
    ok = v != new_val
    idx = np.arange(h * w).reshape(h, w)
    right = ok[:, :-1] & ok[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= max_diff)
    down = ok[:-1, :] & ok[1:, :] & (np.abs(v[:-1, :] - v[1:, :]) <= max_diff)
    edges = [(int(a), int(a) + 1) for a in idx[:, :-1][right]] + [(int(a), int(a) + w) for a in idx[:-1, :][down]]
    parent = list(range(h * w))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            if ra < rb:
                parent[rb] = ra
            else:
                parent[ra] = rb
    labels = np.full(h * w, -1, np.int32)
    for a in np.flatnonzero(ok.ravel()):
        labels[a] = find(int(a))
    sizes = np.zeros(h * w, np.int32)
    valid = labels >= 0
    sizes[valid] = np.bincount(labels[valid], minlength=h * w)[labels[valid]]
    return labels.reshape(h, w), sizes.reshape(h, w)


def filter_speckles(d, new_val, max_size, max_diff, return_sizes=False):
    d = np.asarray(d, np.int16)
    _, sizes = components(d, new_val, max_diff)
    out = np.where((sizes > 0) & (sizes <= max_size), np.int16(new_val), d).astype(np.int16)
    return (out, sizes) if return_sizes else out


def disparity_to_msg(d16, lo, hi):
    v = np.asarray(d16, np.int16).astype(np.float32) * f32(0.0625)
    with np.errstate(invalid="ignore"):
        v = np.where(v < f32(lo), MISSING_Z, v)
        v = np.where(v > f32(hi), MISSING_Z, v)              # sees the first pass's MISSING_Z
    return v.astype(np.float32)


def depth_points(d, Q, zmin, zmax, color=None):
    """(depth float32 HxW, points float32 Nx3, rgba uint32 N)."""
    d = np.asarray(d, np.float32)
    h, w = d.shape
    Q = np.asarray(Q, np.float64)
    wz, q03, q13, q32, q33 = f32(Q[2, 3]), f32(Q[0, 3]), f32(Q[1, 3]), f32(Q[3, 2]), f32(Q[3, 3])
    j = np.tile(np.arange(w, dtype=np.int32).astype(np.float32), (h, 1))
    i = np.repeat(np.arange(h, dtype=np.int32).astype(np.float32), w).reshape(h, w)
    with np.errstate(all="ignore"):
        live = np.logical_not(np.logical_not((d != f32(0)) & (d != MISSING_Z)))
        t = np.multiply(d, q32, dtype=np.float32)
        ww = np.add(t, q33, dtype=np.float32)
        xn = np.add(j, q03, dtype=np.float32)
        x = np.divide(xn, ww, dtype=np.float32)
        yn = np.add(i, q13, dtype=np.float32)
        y = np.divide(yn, ww, dtype=np.float32)
        z = np.divide(np.full((h, w), wz, np.float32), ww, dtype=np.float32)
        front = (ww > f32(0)) & (z > f32(0))
        z64 = z.astype(np.float64)
        inside = (z64 <= np.float64(zmax)) & (z64 >= np.float64(zmin))
    ok = live & front & inside
    depth = np.zeros((h, w), np.float32)
    depth[ok] = z[ok]
    pts = np.empty((int(ok.sum()), 3), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = x[ok], y[ok], z[ok]     # boolean indexing walks in raster order
    if color is None:
        b = g = r = np.zeros(len(pts), np.uint32)
    else:
        c = np.asarray(color, np.uint8)
        if c.ndim == 2:
            b = g = r = c[ok].astype(np.uint32)
        else:
            px = c[ok].astype(np.uint32)
            b, g, r = px[:, 0], px[:, 1], px[:, 2]
    rgba = (np.uint32(0xFF000000) | (r << np.uint32(16)) | (g << np.uint32(8)) | b).astype(np.uint32)
    return depth, pts, rgba
