"""GPU: DisparityImage packing and disparity -> depth / point cloud where only production-size frames
and odd callers go: frames taller than k_depth_scan's 1024 threads (2 and 3 rows per thread, idle
threads), k_depth_write's 256-pixel chunks and wave carries, max_points at the total, padded strides
of every image, non-finite and signed-zero disparities, w <= 0, and depth-window bounds equal to a z.
Bit-exact against tests/post_reference.py and against the oracle; inputs from tests/post_cases.py."""
import numpy as np
import pytest

import post_cases as pc
import post_reference as ref
from test_post_reference import check_tall_precondition

pytestmark = pytest.mark.gpu

DEPTH_CANARY, POINT_CANARY, DISP_FILL = -5.0, -7.0, 7.0      # the disparity pad would make points if read


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_side = []


def _stream(torch):
    """The file's one side stream, ordered after torch's queued work (the library's NULL stream argument
    means the handle's own stream); every call here ends in torch.cuda.synchronize()."""
    if not _side:
        _side.append(torch.cuda.Stream())
    _side[0].wait_stream(torch.cuda.current_stream())
    return _side[0].cuda_stream


def run_depth(engine, pkg, d, Q, window, color=None, pads=(0, 0, 0), max_points=None, points=True, depth=True,
              count=True):
    """sgm_depth_points on device tensors with row pads (disp, depth, colour) and canaries everywhere.
    Returns (depth image or None, depth pad, whole points buffer or None, count or None)."""
    import torch
    h, w = d.shape
    dd = torch.full((h, w + pads[0]), DISP_FILL, dtype=torch.float32)
    dd[:, :w] = torch.as_tensor(d)
    dd = dd.cuda()
    ch, cc = 0, None
    if color is not None:
        ch = 1 if color.ndim == 2 else 3
        cc = torch.full((h, w * ch + pads[2]), 0xA5, dtype=torch.uint8)
        cc[:, :w * ch] = torch.as_tensor(np.ascontiguousarray(color).reshape(h, w * ch))
        cc = cc.cuda()
    dep = torch.full((h, w + pads[1]), DEPTH_CANARY, dtype=torch.float32, device="cuda") if depth else None
    cap = h * w if max_points is None else max_points
    pts = torch.full((cap + 8, 4), POINT_CANARY, dtype=torch.float32, device="cuda") if points else None
    n = torch.full((1,), -1, dtype=torch.int32, device="cuda") if count else None
    engine.depth_points(dd.data_ptr(), w + pads[0], w, h, pkg.q_terms(Q), window[0], window[1],
                        d_color=cc.data_ptr() if cc is not None else None, color_stride=w * ch + pads[2] if ch else 0,
                        channels=ch, d_depth=dep.data_ptr() if depth else None, depth_stride=w + pads[1] if depth else 0,
                        d_points=pts.data_ptr() if points else None, max_points=cap if points else 0,
                        d_num_points=n.data_ptr() if count else None, stream=_stream(torch))
    torch.cuda.synchronize()
    dep = dep.cpu().numpy() if depth else None
    return (dep[:, :w] if depth else None, dep[:, w:] if depth else None, pts.cpu().numpy() if points else None,
            int(n.item()) if count else None)


def check_all(engine, oracle, pkg, case, channels, pads=(0, 0, 0)):
    """Depth image, point list, colours and the count against both references."""
    color = pc.color_for(case, channels)
    want = ref.depth_points(case["d"], case["Q"], *case["window"], color)
    depth, dpad, pts, n = run_depth(engine, pkg, case["d"], case["Q"], case["window"], color, pads)
    for who, (rd, rp, rr) in (("reference", want), ("oracle", oracle.depth_points(case["d"], case["Q"], *case["window"], color))):
        where = f"{case['name']} channels {channels} vs {who}"
        assert n == len(rp), f"{where}: count {n}, {len(rp)} points"
        assert np.array_equal(_bits(depth), _bits(rd)), f"{where}: depth"
        assert np.array_equal(_bits(pts[:n, :3]), _bits(rp)), f"{where}: points"
        assert np.array_equal(_bits(pts[:n, 3]), rr), f"{where}: colours"
    assert (pts[n:] == POINT_CANARY).all() and (dpad == DEPTH_CANARY).all(), case["name"]
    return want


_tall = {}


@pytest.mark.parametrize("channels", [0, 1, 3])
@pytest.mark.parametrize("shape", pc.TALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tall_frames(engine, oracle, pkg, shape, channels):
    """ceil(H / 1024) = 1, 2, 2, 3, 3 rows per k_depth_scan thread; H = 1025 and 2049 leave threads idle."""
    case = _tall.setdefault(shape, pc.tall_case(*shape))
    n = len(ref.depth_points(case["d"], case["Q"], *case["window"])[1])
    check_tall_precondition(case, n)
    check_all(engine, oracle, pkg, case, channels)


@pytest.mark.parametrize("w", pc.CARRY_W)
def test_chunk_and_wave_carries(engine, oracle, pkg, w):
    case = pc.carry_case(w)
    rows = (ref.depth_points(case["d"], case["Q"], *case["window"])[0] > 0).sum(1)
    assert list(rows) == [(w + 63) // 64, w // 64, w], rows        # lane 0 only, lane 63 only, every lane
    for channels in (0, 1, 3):
        check_all(engine, oracle, pkg, case, channels)


def test_max_points_at_the_total(engine, oracle, pkg):
    """The buffer is max_points + 8 long: nothing past max_points is written, the first
    min(max_points, total) points are the reference's, the count is always the full total."""
    case = pc.small_case()
    color = pc.color_for(case, 3)
    rd, rp, rr = ref.depth_points(case["d"], case["Q"], *case["window"], color)
    od, op, orr = oracle.depth_points(case["d"], case["Q"], *case["window"], color)
    total = len(rp)
    assert total > 600 and np.array_equal(_bits(rp), _bits(op)) and np.array_equal(rr, orr)
    for cap in (0, 1, total - 1, total, total + 1):
        depth, _, pts, n = run_depth(engine, pkg, case["d"], case["Q"], case["window"], color, max_points=cap)
        k = min(cap, total)
        assert n == total and len(pts) == cap + 8, cap
        assert np.array_equal(_bits(pts[:k, :3]), _bits(rp[:k])) and np.array_equal(_bits(pts[:k, 3]), rr[:k]), cap
        assert (pts[k:] == POINT_CANARY).all(), cap
        assert np.array_equal(_bits(depth), _bits(rd)), cap
    _, _, pts, n = run_depth(engine, pkg, case["d"], case["Q"], case["window"], points=False, depth=False)
    assert pts is None and n == total                                # the count alone
    depth, dpad, _, n = run_depth(engine, pkg, case["d"], case["Q"], case["window"], points=False, count=False,
                                  pads=(0, 5, 0))
    assert n is None and np.array_equal(_bits(depth), _bits(od)) and (dpad == DEPTH_CANARY).all()


@pytest.mark.parametrize("channels", [0, 1, 3])
def test_padded_strides(engine, oracle, pkg, channels):
    """disp_stride = W + 3, depth_stride = W + 5, color_stride = channels * W + 7."""
    for case in (pc.small_case(), pc.carry_case(513), pc.tall_case(1025, 5)):
        check_all(engine, oracle, pkg, case, channels, pads=(3, 5, 7))


_values = pc.value_cases() + pc.window_edge_cases(ref.depth_points)[0]


@pytest.mark.parametrize("case", _values, ids=[c["name"] for c in _values])
def test_values_and_windows(engine, oracle, pkg, case):
    """NaN, +-inf, -0.0, a denormal, MISSING_Z and its float neighbours, negative disparities; Q's with
    w <= 0 and w == 0; windows (0, inf), zmin > zmax, and bounds that equal a z or just miss it (what
    each reaches is asserted on the CPU in test_post_reference.py)."""
    for channels in (0, 1, 3):
        _, rp, _ = check_all(engine, oracle, pkg, case, channels, pads=(3, 0, 0))
    if case["name"].endswith("_empty"):
        assert len(rp) == 0


_msg = pc.msg_cases()


@pytest.mark.parametrize("case", _msg, ids=[c[0] for c in _msg])
def test_disparity_to_msg_edges(engine, oracle, case):
    import torch
    name, img, lo, hi = case
    h, w = img.shape
    src = torch.as_tensor(img).cuda()
    out = torch.full((h, w + 5), -1.0, dtype=torch.float32, device="cuda")
    engine.disparity_to_msg(src.data_ptr(), w, w, h, lo, hi, out.data_ptr(), w + 5, _stream(torch))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:, :w]), _bits(ref.disparity_to_msg(img, lo, hi))), name
    assert np.array_equal(_bits(got[:, :w]), _bits(oracle.disparity_to_msg(img, lo, hi))), name
    assert (got[:, w:] == -1).all(), name
