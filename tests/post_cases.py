"""The inputs of the post-filter and depth edge tests, shared by test_post_reference.py (the two CPU
references against each other) and test_gpu_post_edges.py / test_gpu_depth_edges.py (the kernels
against both). Everything is deterministic and small; nothing here computes an expected result beyond
the pixel counts that the shapes have by construction."""
import numpy as np

TW, TH = 64, 16                     # the speckle filter's union-find tile (post.hip kSpkTW x kSpkTH)
BG = -16                            # new_val of the shape cases: (minD - 1) * 16 for minD = 0
NEW_VALS = (-16, 0, (-9 - 1) * 16)  # ... and for minD = 1 and minD = -9


def _case(name, d, new_val, max_diff, max_sizes, sizes=None, fat=None):
    """sizes: the component sizes the image has by construction (the test asserts them on the
    reference's size map before it looks at the GPU). fat: the max_size at which, after the median,
    components of exactly max_size and max_size + 1 pixels exist, each on >= 2 tiles."""
    return dict(name=name, d=np.ascontiguousarray(d, np.int16), new_val=int(new_val), max_diff=int(max_diff),
                max_sizes=sorted(set(int(m) for m in max_sizes)), sizes=sizes, fat=fat)


def _around(*ns):
    return [m for n in ns for m in (n - 1, n, n + 1)]


def exact_size_cases():
    out = []
    d = np.full((40, 200), BG, np.int16)
    d[14:18, 60:70] = 64                        # 4 x 10 = 40 pixels over four tiles (seams 15|16, 63|64)
    out.append(_case("rect40_four_tiles", d, BG, 16, _around(40), sizes=[40]))
    d = np.full((40, 200), BG, np.int16)
    d[2:6, 10:20] = 64                          # the same inside tile (0, 0)
    out.append(_case("rect40_one_tile", d, BG, 16, _around(40), sizes=[40]))
    return out


def line_cases():
    out = []
    hsums = _around(7, 64, 128)
    d = np.full((20, 583), BG, np.int16)
    d[5, :] = 64                                # parts of 64 x 9 and 7; the root's part has 64
    out.append(_case("hline583", d, BG, 16, _around(583) + hsums, sizes=[583]))
    d = np.full((20, 640), BG, np.int16)
    d[5, 57:640] = 64                           # the part with the global root (cols 57..63) has 7
    out.append(_case("hline583_root7", d, BG, 16, _around(583) + hsums, sizes=[583]))
    d = np.full((149, 100), BG, np.int16)
    d[:, 70] = 64                               # parts of 16 x 9 and 5
    out.append(_case("vline149", d, BG, 16, _around(149) + _around(16, 32), sizes=[149]))
    return out


SEAMS = ("col63", "row15", "inner")
PLANE_VALUES = (                    # (tag, a, b when joined, b when not, max_diff joined, max_diff not)
    ("neg640_md16", -640, -640 + 16, -640 + 17, 16, 16),
    ("zero_md16", 0, 16, 17, 16, 16),
    ("neg640_md0", -640, -640, -639, 0, 0),
    ("zero_md0", 0, 0, 1, 0, 0),
    # the int16 ends are 65535 apart: one step less of max_diff stands for "max_diff + 1 apart"
    ("ends_md65535", 32767, -32768, -32768, 65535, 65534),
)


def _half_planes(seam, a, b, new_val):
    if seam == "row15":
        d = np.full((40, 70), a, np.int16)
        d[16:, :] = b
        holes = [(15, 7), (16, 20)]
    else:
        c = 64 if seam == "col63" else 31
        d = np.full((20, 130), a, np.int16)
        d[:, c:] = b
        holes = [(4, c - 1), (9, c)]
    d[2::7, 3::11] = new_val                    # new_val as an ordinary value: isolated pixels, some on the seam
    for y, x in holes:
        d[y, x] = new_val
    return d


def max_diff_cases(seam, tag):
    """Two half-planes a | b that join (|a - b| == max_diff) or not (max_diff + 1), for every new_val."""
    _, a, b_join, b_apart, md_join, md_apart = next(v for v in PLANE_VALUES if v[0] == tag)
    out = []
    for nv in NEW_VALS:
        for join, b, md in ((True, b_join, md_join), (False, b_apart, md_apart)):
            d = _half_planes(seam, a, b, nv)
            na = int(((d == a) & (d != nv)).sum())
            nb = int(((d == b) & (d != nv)).sum()) if b != a else 0
            sizes = [na + nb] if join else [na, nb]
            sizes = sorted(s for s in sizes if s > 0)
            ms = [m for s in sizes for m in (s - 1, s)] or [5]
            out.append(_case(f"{seam}_{tag}_nv{nv}_{'join' if join else 'apart'}", d, nv, md, ms, sizes=sizes))
    return out


def fat_cases():
    """Shapes that keep a known size through the 3x3 median: on a new_val ground it takes the four
    corner pixels of a rectangle at least 3 thick and nothing else. 3 x 29 -> 83 and 4 x 22 -> 84."""
    out = []
    d = np.full((40, 200), BG, np.int16)
    d[3:6, 40:69] = 64                          # over the seam 63|64
    d[20:24, 120:142] = 96                      # over the seam 127|128
    out.append(_case("fat_horizontal", d, BG, 16, [0] + _around(83), fat=83))
    d = np.full((60, 140), BG, np.int16)
    d[5:34, 10:13] = 64                         # over the seams 15|16 and 31|32
    d[20:42, 100:104] = 96                      # over the seam 31|32
    out.append(_case("fat_vertical", d, BG, 16, [0] + _around(83), fat=83))
    d = np.full((40, 200), BG, np.int16)
    d[14:17, 50:79] = 64                        # four tiles
    d[30:34, 120:142] = 96                      # four tiles (seams 31|32, 127|128)
    out.append(_case("fat_four_tiles", d, BG, 16, [0] + _around(83), fat=83))
    return out


RAGGED = ((1, 300), (300, 1), (17, 130), (65, 64))


def ragged_cases():
    out = []
    for h, w in RAGGED:
        rng = np.random.default_rng(h * 1000 + w)
        d = (rng.integers(0, 3, (h, w)) * 16).astype(np.int16)
        d[rng.random((h, w)) < 0.15] = BG
        out.append(_case(f"ragged_{h}x{w}", d, BG, 16, [0, 3, 40]))
    return out


def speckle_groups():
    """{group name: list of cases}: one GPU test per group."""
    g = {"exact": exact_size_cases(), "lines": line_cases(), "fat": fat_cases(), "ragged": ragged_cases()}
    for seam in SEAMS:
        for v in PLANE_VALUES:
            g[f"maxdiff_{seam}_{v[0]}"] = max_diff_cases(seam, v[0])
    return g


# ------------------------------------------------------------------------------------ depth ----
def q_matrix(fx=712.5, cx=331.2, cy=247.9, q32=1.0 / 0.119, q33=-(331.2 - 329.8) / 0.119):
    """Q with the five entries the depth node reads (calc_q's layout)."""
    q = np.zeros((4, 4), np.float64)
    q[0, 0] = q[1, 1] = 1.0
    q[0, 3], q[1, 3], q[2, 3], q[3, 2], q[3, 3] = -cx, -cy, fx, q32, q33
    return q


def sample_disp(rng, h, w):
    d = (rng.integers(-40, 2000, (h, w)) / 16.0).astype(np.float32)
    d[rng.random((h, w)) < 0.1] = 0
    d[rng.random((h, w)) < 0.1] = 10000
    return d


def _dcase(name, d, Q=None, window=(0.0, 100.0)):
    return dict(name=name, d=np.ascontiguousarray(d, np.float32), Q=q_matrix() if Q is None else Q,
                window=(float(window[0]), float(window[1])))


TALL = ((1024, 5), (1025, 5), (2048, 3), (2049, 257), (3000, 7))


def tall_case(h, w):
    """k_depth_scan with 1 and 2 and 3 rows per thread: every 7th row empty, every 11th full."""
    rng = np.random.default_rng(h * 7 + w)
    d = sample_disp(rng, h, w)
    d[::7] = 0
    full = (rng.integers(64, 2000, (h, w)) / 16.0).astype(np.float32)     # >= 4 px: a point under q_matrix()
    d[::11] = full[::11]
    d[0], d[h - 1] = full[0], full[h - 1]
    return _dcase(f"tall_{h}x{w}", d)


CARRY_W = (255, 256, 257, 512, 513, 769)


def carry_case(w):
    """k_depth_write's 256-pixel chunks and four waves: a point only in lane 0 of every wave, only in
    lane 63, and everywhere."""
    rng = np.random.default_rng(w)
    full = (rng.integers(64, 2000, (3, w)) / 16.0).astype(np.float32)
    d = np.zeros((3, w), np.float32)
    d[0, 0::64] = full[0, 0::64]
    d[1, 63::64] = full[1, 63::64]
    d[2] = full[2]
    return _dcase(f"carry_w{w}", d)


def small_case():
    """The frame of the max_points, stride and null-pointer cases: two chunks, ragged."""
    return _dcase("small_9x300", sample_disp(np.random.default_rng(77), 9, 300))


def _special_image():
    rng = np.random.default_rng(123)
    d = sample_disp(rng, 6, 70)
    ten_k = np.float32(10000.0)
    sp = [np.nan, np.inf, -np.inf, -0.0, 1e-40, ten_k, np.nextafter(ten_k, np.float32(np.inf)),
          np.nextafter(ten_k, np.float32(0)), -3.5, -0.0625, 2.0]
    sp = np.array(sp, np.float32)
    assert 0 < abs(sp[4]) < np.finfo(np.float32).tiny          # a float32 denormal
    d[0, :len(sp)] = sp
    d[3, 70 - len(sp):] = sp[::-1]
    d[5, 60:70] = 2.0
    d[2, 30:40] = np.float32(1e-40)
    return d


def value_cases():
    d = _special_image()
    inf = float("inf")
    qs = {"std": q_matrix(), "q33zero": q_matrix(q33=0.0), "q32neg": q_matrix(q32=-0.05, q33=3.0),
          "wzero": q_matrix(q32=1.0, q33=-2.0)}
    out = []
    for qn, Q in qs.items():
        for wn, win in (("open", (0.0, inf)), ("node", (0.0, 100.0)), ("empty", (5.0, 2.0))):
            out.append(_dcase(f"values_{qn}_{wn}", d, Q, win))
    return out


def window_edge_cases(reference_depth_points):
    """Windows whose bound is a z that the image produces (taken from `reference_depth_points`'s output),
    and the float64 next to it that shuts that z out. Returns (cases, z)."""
    base = small_case()
    depth, _, _ = reference_depth_points(base["d"], base["Q"], 0.0, 100.0)
    zs = np.sort(depth[depth > 0])
    z = float(zs[len(zs) // 2])
    lo, hi = float(np.nextafter(z, -np.inf)), float(np.nextafter(z, np.inf))
    wins = (("zmax_eq", (0.0, z)), ("zmax_below", (0.0, lo)), ("zmin_eq", (z, 100.0)), ("zmin_above", (hi, 100.0)))
    return [_dcase(f"window_{n}", base["d"], base["Q"], w) for n, w in wins], z


def depth_cases(reference_depth_points):
    out = [tall_case(h, w) for h, w in TALL] + [carry_case(w) for w in CARRY_W] + [small_case()] + value_cases()
    return out + window_edge_cases(reference_depth_points)[0]


def color_for(case, channels):
    if channels == 0:
        return None
    h, w = case["d"].shape
    rng = np.random.default_rng(h * 31 + w + channels)
    return rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3), dtype=np.uint8)


def msg_cases():
    """(name, int16 image, lo, hi) of disparity_to_msg."""
    inf, nan = float("inf"), float("nan")
    rng = np.random.default_rng(9)
    a = rng.integers(-32768, 32768, (2, 257)).astype(np.int16)
    a[0, 0], a[0, 1], a[1, 255], a[1, 256] = -32768, 32767, 32767, -32768
    a[0, 2], a[0, 3], a[1, 64] = 32, 2400, 160
    b = rng.integers(-300, 4000, (1025, 3)).astype(np.int16)
    b[0, 0], b[1024, 2], b[512, 1] = 32, 2400, -32768
    wins = (("open", 0.0, inf), ("ends", -2048.0, 2047.9375), ("present", 2.0, 150.0), ("lo_gt_hi", 50.0, 10.0),
            ("nan_lo", nan, 100.0), ("nan_hi", 0.0, nan), ("nan_both", nan, nan))
    return [(f"{n}_{wn}", img, lo, hi) for n, img in (("2x257", a), ("1025x3", b)) for wn, lo, hi in wins]
