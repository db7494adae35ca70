"""Frames that a 256-CU device plans like production frames of MODE_OCV_BM by itself (no override of
the CU count) and that tests/bm_fast_reference.py can afford: the plan bm_plan gives each at 256 CUs
(pinned host-only in tests/test_bm_fast_reference.py), the property each is there for, and the seed
whose synth.stereo_pair frames leave enough valid pixels. A GPU comparison over them asserts the
property at the device's own CU count (misses), runs engine.match and requires equality with the
reference; DESIGN.md (BM section) says where that comparison stands. Test infrastructure only."""
import collections

T, U = 10, 15                   # texture threshold and uniqueness ratio of every case

# frame: H, W, m, D, w, cap.  plan at 256 CUs: TX, nsx, nsy, RB, waves, lds.
# prop: what must hold of the plan at any CU count for the case to reach what it is there for:
#   tx (lo, hi) inclusive, waves, lds (lo, hi) inclusive, wide, vglobal, nk
Case = collections.namedtuple("Case", "name frame plan prop seed reaches")

KB = 1024
CASES = [
    Case("A", (2056, 232, 0, 32, 5, 31), (101, 2, 228, 9, 8, 14420),
         dict(tx=(100, 128), waves=8, lds=(0, 48 * KB), wide=0, vglobal=0, nk=1), 3,
         "full-width strips in 8-wave workgroups; last strip 100 of 101 columns"),
    Case("E", (1808, 264, 0, 64, 15, 31), (51, 4, 120, 15, 8, 8980),
         dict(tx=(33, 99), waves=8, lds=(0, 48 * KB), wide=0, vglobal=0, nk=1), 3,
         "halved strips; last strip 48 of 51 columns, last band 9 of 15 rows"),
    Case("B", (1032, 728, 3, 256, 9, 31), (118, 4, 128, 8, 16, 66040),
         dict(tx=(100, 128), waves=16, lds=(64 * KB + 1, 128 * KB), wide=0, vglobal=0, nk=4), 3,
         "16 waves, dynamic LDS above 64 KB, K = 4"),
    Case("C", (1432, 648, -5, 144, 23, 63), (64, 8, 62, 23, 16, 67128),
         dict(tx=(33, 128), waves=16, lds=(64 * KB + 1, 128 * KB), wide=1, vglobal=0, nk=3), 3,
         "u32 sums in 16-wave workgroups, m < 0; last strip 57 of 64 columns, last band 7 of 23 rows"),
    Case("D", (1160, 1384, 20, 480, 21, 31), (99, 9, 28, 41, 16, 123836),
         dict(tx=(64, 128), waves=16, lds=(120 * KB, 128 * KB), wide=0, vglobal=0, nk=8), 3,
         "the shipped launch configuration's kernel (K = 8, 16 waves) at 121 KB of LDS"),
    Case("G", (16, 2130, 0, 2048, 5, 31), (21, 4, 1, 12, 8, 106708),
         dict(tx=(1, 32), waves=8, lds=(64 * KB + 1, 128 * KB), wide=0, vglobal=0, nk=32), 6,
         "more than 2048 staged bytes per row: the commit's tail loop; K = 32"),
    Case("H", (16, 2130, 0, 2032, 5, 31), (25, 4, 1, 12, 8, 123124),
         dict(tx=(1, 32), waves=8, lds=(120 * KB, 128 * KB), wide=0, vglobal=0, nk=32), 6,
         "8-wave launch at 120 KB; D no multiple of 64 in the last of 32 chunks"),
    Case("I", (30, 2130, 0, 2048, 23, 63), (28, 3, 1, 8, 8, 4504),
         dict(tx=(1, 32), waves=8, lds=(0, 48 * KB), wide=1, vglobal=1, nk=32), 6,
         "column sums in HBM chosen by the plan itself (no environment variable), u32"),
]
BY_NAME = {c.name: c for c in CASES}

# case D is compared on the rows of its first, a middle and its last band pair (RB = 41, w2 = 10)
D_ROWS = [(10, 92), (543, 625), (1076, 1150)]


def plan_of(pkg, frame, n_cu):
    H, W, m, D, w, cap = frame
    p = pkg.default_params(pkg.MODE_OCV_BM, min_disparity=m, num_disparities=D, block_size=w, prefilter_cap=cap)
    return pkg.bm_plan(p, pkg.default_bm_params(), W, H, n_cu)


def misses(pl, prop):
    """The entries of prop that the plan pl does not have (empty: the case reaches its paths)."""
    bad = []
    if not prop["tx"][0] <= pl["TX"] <= prop["tx"][1]:
        bad.append(f"TX {pl['TX']} outside {prop['tx']}")
    if not prop["lds"][0] <= pl["lds"] <= prop["lds"][1]:
        bad.append(f"lds {pl['lds']} outside {prop['lds']}")
    for k in ("waves", "wide", "vglobal", "nk"):
        if pl[k] != prop[k]:
            bad.append(f"{k} {pl[k]} != {prop[k]}")
    return bad


def staged_bytes(pl, frame):
    """The most bytes a workgroup stages of one image row pair (BM kernels): the strip's
    NC = nx + 2 w2 left pixels and the right segment [rc(first), rc(last) + D), with
    rc(c) = clip(c - s, 0, W - D)."""
    H, W, m, D, w, cap = frame
    w2, s = w // 2, D - 1 + m
    x0, x1 = max(s, 0), min(W, W + m)
    best = 0
    for i in range(pl["nsx"]):
        xs = x0 + i * pl["TX"]
        nc = min(pl["TX"], x1 - xs) + 2 * w2

        def rc(c):
            return min(max(c - s, 0), W - D)
        best = max(best, nc + rc(xs - w2 + nc - 1) - rc(xs - w2) + D)
    return best
