"""CPU: tests/post_reference.py (numpy and plain Python, written from the kernels' comments) against the
oracle, bit for bit, on random draws like the GPU fuzz tests' and on every input of the GPU edge tests
(tests/post_cases.py). Floats are compared through their bit patterns."""
import numpy as np
import pytest

import post_cases as pc
import post_reference as ref

N_RANDOM = 100                       # per family: 100 post-filter draws + 100 depth draws


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_depth(oracle, d, Q, zmin, zmax, color):
    rd, rp, rr = ref.depth_points(d, Q, zmin, zmax, color)
    od, op, orr = oracle.depth_points(d, Q, zmin, zmax, color)
    assert np.array_equal(_bits(rd), _bits(od)), "depth"
    assert rp.shape == op.shape and np.array_equal(_bits(rp), _bits(op)), f"{len(rp)} vs {len(op)} points"
    assert rr.dtype == np.uint32 and np.array_equal(rr, orr), "colour"
    return rd, rp


@pytest.mark.parametrize("seed", range(N_RANDOM))
def test_random_post_filters(oracle, seed):
    """Drawn like test_fuzz_post_filters."""
    rng = np.random.default_rng(50_000 + seed)
    h, w = int(rng.integers(1, 150)), int(rng.integers(1, 300))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        cy, cx = max(h // int(rng.integers(1, 12)), 1), max(w // int(rng.integers(1, 12)), 1)
        coarse = rng.integers(-40, 400, (h // cy + 1, w // cx + 1))
        disp = np.repeat(np.repeat(coarse, cy, 0), cx, 1)[:h, :w]
        m = rng.random((h, w)) < 0.05
        disp = np.where(m, rng.integers(-40, 400, (h, w)), disp)
    elif kind == 1:
        disp = (np.add.outer(np.arange(h) * int(rng.integers(0, 4)), np.arange(w) * int(rng.integers(0, 4))) % 500) - 20
    else:
        disp = rng.integers(-40, 400, (h, w))
    disp = disp.astype(np.int16)
    new_val = int(rng.choice([-16, -32, 0, int(disp.min())]))
    max_size, max_diff = int(rng.choice([0, 1, 5, 30, 100, 1000])), int(rng.choice([0, 1, 16, 32, 64]))
    assert np.array_equal(ref.median3(disp), oracle.median3(disp))
    assert np.array_equal(ref.filter_speckles(disp, new_val, max_size, max_diff),
                          oracle.filter_speckles(disp, new_val, max_size, max_diff)), \
        f"{h}x{w} kind {kind} new {new_val} size {max_size} diff {max_diff}"


@pytest.mark.parametrize("seed", range(N_RANDOM))
def test_random_depth(oracle, seed):
    """Drawn like test_fuzz_depth."""
    rng = np.random.default_rng(90_000 + seed)
    h, w = int(rng.integers(1, 120)), int(rng.integers(1, 300))
    f = float(rng.uniform(200, 2000))
    cx, cy = w / 2 + rng.normal(0, 10), h / 2 + rng.normal(0, 10)
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    Pl = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0]])
    Pr = Pl.copy()
    Pr[0, 3] = -f * float(rng.uniform(0.03, 0.5))
    Pr[0, 2] = cx + rng.normal(0, 3)
    Q = oracle.calc_q(K, Pr, Pl)
    d = (rng.integers(-40, 4000, (h, w)) / 16.0).astype(np.float32)
    d[rng.random((h, w)) < 0.15] = 0
    d[rng.random((h, w)) < 0.1] = 10000
    lo = float(rng.choice([0.0, 0.1, 0.5]))
    window = (lo, lo + float(rng.choice([0.5, 3.0, 50.0, 1e4])))
    channels = int(rng.choice([0, 1, 3]))
    color = None if channels == 0 else rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3), dtype=np.uint8)
    _same_depth(oracle, d, Q, *window, color)
    d16 = rng.integers(-300, 4000, (h, w)).astype(np.int16)
    assert np.array_equal(_bits(ref.disparity_to_msg(d16, *window)), _bits(oracle.disparity_to_msg(d16, *window)))


def test_q_matrix_is_calc_q(oracle):
    from test_depth_oracle import _q
    assert np.array_equal(pc.q_matrix(), oracle.calc_q(*_q()))


def tiles_of(labels, root):
    ys, xs = np.nonzero(labels == root)
    return {(int(y) // pc.TH, int(x) // pc.TW) for y, x in zip(ys, xs)}


def check_precondition(case, median):
    """What a speckle case promises about its own input, asserted on post_reference alone. Returns the
    image the speckle filter sees."""
    d = ref.median3(case["d"]) if median else case["d"]
    labels, sizes = ref.components(d, case["new_val"], case["max_diff"])
    roots = np.unique(labels[labels >= 0])
    comp = sorted(int(sizes.ravel()[r]) for r in roots)
    if not median and case["sizes"] is not None:
        assert comp == case["sizes"], f"{case['name']}: components {comp}, built as {case['sizes']}"
        for s in case["sizes"]:
            assert s in case["max_sizes"] and s - 1 in case["max_sizes"]
    if median and case["fat"] is not None:
        n = case["fat"]
        for want in (n, n + 1):
            hit = [r for r in roots if sizes.ravel()[r] == want]
            assert len(hit) == 1, f"{case['name']}: {len(hit)} components of {want} pixels after the median"
            assert len(tiles_of(labels, hit[0])) >= 2
        assert n in case["max_sizes"]
    return d


@pytest.mark.parametrize("group", sorted(pc.speckle_groups()))
def test_speckle_cases(oracle, group):
    for case in pc.speckle_groups()[group]:
        for median in (0, 1):
            d = check_precondition(case, median)
            if median:
                assert np.array_equal(d, oracle.median3(case["d"])), case["name"]
            _, sizes = ref.components(d, case["new_val"], case["max_diff"])
            for ms in case["max_sizes"]:
                want = np.where((sizes > 0) & (sizes <= ms), np.int16(case["new_val"]), d)
                assert np.array_equal(want, ref.filter_speckles(d, case["new_val"], ms, case["max_diff"]))
                assert np.array_equal(want, oracle.filter_speckles(d, case["new_val"], ms, case["max_diff"])), \
                    f"{case['name']} median {median} max_size {ms}"


def test_line_parts_are_what_the_issue_says():
    """The lines' tile-local parts: nine of a full tile side and one remainder, and which part holds
    the global root (the smallest raster index)."""
    for case, parts, first in zip(pc.line_cases(), ([64] * 9 + [7], [7] + [64] * 9, [16] * 9 + [5]), (64, 7, 16)):
        ys, xs = np.nonzero(case["d"] != case["new_val"])
        tiles = [(int(y) // pc.TH, int(x) // pc.TW) for y, x in zip(ys, xs)]
        counts = [tiles.count(t) for t in sorted(set(tiles))]
        assert counts == parts and counts[0] == first, case["name"]


def test_depth_cases(oracle):
    cases = pc.depth_cases(ref.depth_points)
    assert len({c["name"] for c in cases}) == len(cases)
    for case in cases:
        for channels in (0, 1, 3):
            _same_depth(oracle, case["d"], case["Q"], *case["window"], pc.color_for(case, channels))


def check_tall_precondition(case, n_points):
    h, w = case["d"].shape
    depth = ref.depth_points(case["d"], case["Q"], *case["window"])[0]
    empty = np.flatnonzero((depth > 0).sum(1) == 0)
    assert len(empty) > 0 and (depth[0] > 0).any() and (depth[h - 1] > 0).any()
    full = [r for r in range(0, h, 11)]
    assert ((depth[full] > 0).sum(1) == w).all()          # every 11th row: a point in every pixel
    if h > 1030:          # a row index above 1024 exists that the case leaves empty (a multiple of 7)
        assert empty.max() > 1024
    assert n_points > 0.3 * h * w


def test_tall_preconditions():
    for h, w in pc.TALL:
        case = pc.tall_case(h, w)
        check_tall_precondition(case, len(ref.depth_points(case["d"], case["Q"], *case["window"])[1]))


def test_window_edges_shut_a_point_out():
    cases, z = pc.window_edge_cases(ref.depth_points)
    n = {c["name"]: len(ref.depth_points(c["d"], c["Q"], *c["window"])[1]) for c in cases}
    assert n["window_zmax_eq"] > n["window_zmax_below"] > 0
    assert n["window_zmin_eq"] > n["window_zmin_above"] > 0
    assert z == float(np.float32(z))


def test_value_cases_reach_their_branches():
    """The special image has what it claims, and the odd Q's give w <= 0 and w == 0."""
    by = {c["name"]: c for c in pc.value_cases()}
    d = by["values_std_open"]["d"]
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d < 0).any()
    assert (np.signbit(d) & (d == 0)).any()
    q32, q33 = np.float32(-0.05), np.float32(3.0)
    w = d * q32 + q33
    assert (w[np.isfinite(d)] < 0).any() and (w[np.isfinite(d)] > 0).any()
    assert ((d * np.float32(1.0) + np.float32(-2.0)) == 0).sum() >= 10
    for name in ("values_q32neg_open", "values_wzero_open", "values_q33zero_open", "values_std_open"):
        assert len(ref.depth_points(by[name]["d"], by[name]["Q"], *by[name]["window"])[1]) > 0, name
    # a denormal disparity with q33 = 0: w is denormal, z overflows to +inf and passes zmax = inf
    pts = ref.depth_points(by["values_q33zero_open"]["d"], by["values_q33zero_open"]["Q"], 0.0, float("inf"))[1]
    assert np.isposinf(pts[:, 2]).any()
    assert len(ref.depth_points(d, by["values_std_empty"]["Q"], 5.0, 2.0)[1]) == 0


def test_msg_cases(oracle):
    for name, img, lo, hi in pc.msg_cases():
        got = ref.disparity_to_msg(img, lo, hi)
        assert np.array_equal(_bits(got), _bits(oracle.disparity_to_msg(img, lo, hi))), name
    by = {n: ref.disparity_to_msg(i, lo, hi) for n, i, lo, hi in pc.msg_cases()}
    a = by["2x257_ends"]
    assert a[0, 0] == -2048.0 and a[0, 1] == 2047.9375            # a bound equal to a value keeps it
    assert by["2x257_present"][0, 2] == 2.0 and by["2x257_present"][0, 3] == 150.0
    assert (by["2x257_lo_gt_hi"] == 10000.0).all()
    assert (by["2x257_nan_both"] != 10000.0).all()                # no compare with NaN is true
