"""The up+WTA step of the census batch (the last sweep fused with the WTA) and the WTA rows,
bit-exact against the CPU oracle through Engine.match_device_batch, at the shapes where the
step's byte sums, its uniqueness-threshold table and its result stores can go wrong:

* widths of several 16-column blocks plus a partial one (a block count that is no multiple of 16),
* heights 17, 33, 50 (no multiple of 4 or 16: partial last groups of steps),
* D of every lane layout (32, 64, 128, 256) and D below the padded D (48, 208: masked halves),
* uniqueness ratios on both sides of every branch of T(minS) (0, 5, 15, 99, 100, 101),
* subpixel and LR check on and off, 8 and 4 paths, batches of 3 and 5 frames (odd groups; the
  last group goes through the WTA rows),
* flat image pairs (minS = 0 everywhere: the T = 0 / 1 table entries and the best = 0 edge).

Two CPU tests pin the arithmetic the kernels rely on: the wrapped-sum identity of the byte sums
and the closed form of the threshold table.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import census_paths_reference as cpr
from conftest import to_oracle_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------
# CPU: the arithmetic behind the kernels
# ------------------------------------------------------------------------------------------
def _odd_pairs(v):
    """v_perm 0x0c030c01 of a dword: byte 1 in the low half, byte 3 in the high half."""
    return ((v >> 8) & 0xFF) | (((v >> 24) & 0xFF) << 16)


@pytest.mark.parametrize("nv", [3, 7, 8])
def test_wrapped_sum_identity(nv):
    """e = sum(v) - (o << 8) in wrapping 32-bit arithmetic equals the sum of the even bytes as u16
    pairs, for every byte content (all-255 words included): the form sum_eo uses."""
    rng = np.random.default_rng(nv)
    words = rng.integers(0, 2 ** 32, size=(20000, nv), dtype=np.uint64)
    words[:64] = 0xFFFFFFFF
    words[64:128] = 0
    words[128:192, ::2] = 0xFFFFFFFF
    words[192:256] = rng.choice(np.array([0, 0xFF, 0xFF00, 0xFF0000, 0xFF000000, 0xFF00FF00, 0x00FF00FF],
                                         np.uint64), size=(64, nv))
    m32 = np.uint64(0xFFFFFFFF)
    e_ref = (words & np.uint64(0x00FF00FF)).sum(axis=1)           # no carry: halves <= nv * 255
    o_ref = _odd_pairs(words).sum(axis=1)
    assert ((e_ref & np.uint64(0xFFFF)) <= nv * 255).all() and ((e_ref >> np.uint64(16)) <= nv * 255).all()
    sv = words.sum(axis=1) & m32                                   # the plain wrapping sum
    e = (sv - ((o_ref << np.uint64(8)) & m32)) & m32
    assert np.array_equal(e, e_ref)
    assert np.array_equal((e + ((o_ref << np.uint64(8)) & m32)) & m32, sv)


def _thresh(min_s, u):
    """wta_thresh of census_sgm.hip, float32 step by step."""
    if u >= 100:
        return 1 if (min_s == 0 and u > 100) else 0
    if min_s == 0:
        return 0
    num, den = min_s * 100 - 1, 100 - u
    inv_u = np.float32(1.0) / np.float32(den)
    q = int(np.float32(num) * inv_u)
    q += 1 if (q + 1) * den <= num else 0
    q -= 1 if q * den > num else 0
    return min(q + 1, 8 * 255 + 1)


def test_threshold_table_closed_form():
    """Every entry of the table the up+WTA blocks build, T(minS) = (minS * 100 - 1) / (100 - u) + 1
    (0 at minS = 0, capped at 8 * 255 + 1), for every minS in [0, 2040] and every u in [0, 99]."""
    for u in range(100):
        for min_s in range(2041):
            want = 0 if min_s == 0 else min((min_s * 100 - 1) // (100 - u) + 1, 2041)
            assert _thresh(min_s, u) == want, (min_s, u)
    assert [_thresh(m, 100) for m in (0, 1, 2040)] == [0, 0, 0]
    assert [_thresh(m, 101) for m in (0, 1, 2040)] == [1, 0, 0]


# ------------------------------------------------------------------------------------------
# GPU: the batch pipeline against the oracle
# ------------------------------------------------------------------------------------------
def _frames(synth, kind, h, w, D, minD, n, seed):
    if kind == "flat":          # constant pairs: every cost 0, every d ties
        return [(np.full((h, w), 40 + 30 * i, np.uint8), np.full((h, w), 40 + 30 * i, np.uint8)) for i in range(n)]
    fr = [synth.stereo_pair(h, w, max(minD, 0), D, seed=seed + 7 * i)[:2] for i in range(n)]
    if kind == "half":          # the left part flat, the rest textured
        for l, r in fr:
            l[:, :w // 2 + 11] = 90
            r[:, :w // 2 + 11] = 90
    return fr


def _reference(oracle, p, paths, l, r):
    op = to_oracle_params(oracle, p)
    return oracle.match(op, l, r) if paths == 8 else cpr.match_paths(oracle, op, l, r)


def _run_batch(engine, frames, h, w):
    torch = pytest.importorskip("torch")
    n = len(frames)
    dl = [torch.from_numpy(np.ascontiguousarray(f[0])).cuda() for f in frames]
    dr = [torch.from_numpy(np.ascontiguousarray(f[1])).cuda() for f in frames]
    out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    engine.match_device_batch([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, w,
                              [out[i].data_ptr() for i in range(n)], w, stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy()


def _case(D, h, n, uniq, paths=8, w=360, kind="pair", **kw):
    return pytest.param(dict(num_disparities=D, uniqueness_ratio=uniq, **kw), h, w, n, paths, kind,
                        id=f"D{D}-h{h}-w{w}-n{n}-u{uniq}-p{paths}-{kind}" +
                           "".join(f"-{k}{v}" for k, v in sorted(kw.items())))


# W = 360: width1 = W - (D - 1) gives 21 / 20 / 19 / 15 / 10 / 7 blocks of 16 columns for D = 32 /
# 48 / 64 / 128 / 208 / 256, the last one partial; W = 347 moves the partial block's width.
BATCH_CASES = [
    _case(256, 50, 5, 15),
    _case(256, 17, 3, 0, subpixel=0),
    _case(256, 33, 3, 99, w=347, lr_check=0),
    _case(256, 17, 3, 100, w=347),
    _case(256, 33, 5, 5, subpixel=0, lr_check=0),
    _case(128, 33, 3, 5, lr_check=0),
    _case(128, 17, 5, 100, subpixel=0),
    _case(64, 50, 5, 99),
    _case(64, 17, 3, 100, w=347),
    _case(64, 33, 3, 101, subpixel=0, lr_check=0),
    _case(32, 33, 5, 101),
    _case(32, 50, 3, 5, min_disparity=-7),
    _case(48, 33, 3, 15, min_disparity=3),           # masked halves, 2 lanes past D
    _case(208, 17, 3, 5),                            # masked halves in the 16-per-lane layout
    _case(208, 50, 5, 101, w=347, subpixel=0),
    _case(256, 33, 3, 15, paths=4),
    _case(128, 50, 5, 101, paths=4),
    _case(64, 50, 5, 0, paths=4, subpixel=0, lr_check=0),
    _case(48, 17, 3, 100, paths=4),
    _case(32, 17, 3, 99, paths=4, w=347),
    _case(64, 33, 3, 15, kind="flat"),
    _case(64, 17, 3, 0, kind="flat", subpixel=0),
    _case(256, 33, 3, 101, kind="flat"),
    _case(48, 17, 5, 100, kind="flat", paths=4),
    _case(128, 33, 3, 15, kind="half"),
    _case(64, 50, 3, 101, kind="half", paths=4),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,h,w,n,paths,kind", BATCH_CASES)
def test_upwta_batch(engine, oracle, pkg, synth, kw, h, w, n, paths, kind):
    D, minD = kw["num_disparities"], kw.get("min_disparity", 0)
    p = pkg.default_params(pkg.MODE_CENSUS8, **kw)
    frames = _frames(synth, kind, h, w, D, minD, n, seed=500 + D + h)
    engine.set_params(p)
    engine.set_census_paths(paths)
    try:
        engine.set_profiling(True)
        got = _run_batch(engine, frames, h, w)
        launches = engine.stage_launches()
    finally:
        engine.set_profiling(False)
        engine.set_census_paths(8)
    # the frames before the last group went through up+WTA blocks, the last group through WTA rows
    assert launches.get(f"paths{paths}+up_wta", 0) == 1 and launches["wta_lr"] == 1
    assert launches.get("rowfin", 0) == (n + 1) // 2 - 1
    for i, (l, r) in enumerate(frames):
        ref = _reference(oracle, p, paths, l, r)
        assert np.array_equal(got[i], ref), f"frame {i}: {(got[i] != ref).sum()} pixels differ"


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import torch
import conftest, __graft_entry__ as ge
pkg = ge.load_package()
oracle = conftest._load("sgm_oracle", sys.argv[1] + "/oracle/sgm_oracle.py")
synth = conftest._load("sgm_synth", ge.PKG_DIR + "/synth.py")
h, w, D, n = 33, 360, 128, 3
p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, uniqueness_ratio=15)
eng = pkg.Engine(0, p)
frames = [synth.stereo_pair(h, w, 0, D, seed=900 + i)[:2] for i in range(n)]
dl = [torch.from_numpy(f[0]).cuda() for f in frames]
dr = [torch.from_numpy(f[1]).cuda() for f in frames]
out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
torch.cuda.synchronize()
eng.set_profiling(True)
eng.match_device_batch([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, w,
                       [out[i].data_ptr() for i in range(n)], w, None)
eng.synchronize()
launches = eng.stage_launches()
assert launches.get("paths8+wta_lr", 0) == 1 and not any("up_wta" in k for k in launches), launches
got = out.cpu().numpy()
op = conftest.to_oracle_params(oracle, p)
for i, (l, r) in enumerate(frames):
    ref = oracle.match(op, l, r)
    assert np.array_equal(got[i], ref), f"frame {i}: {(got[i] != ref).sum()} pixels differ"
eng.close()
print("upwta0 child ok")
"""


@pytest.mark.gpu
def test_upwta_off_child_process():
    """SGM_UPWTA=0 set before the process starts: eight volumes and WTA rows (wta_row16 with its
    in-place threshold) for every group, same results."""
    env = dict(os.environ, SGM_UPWTA="0")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "upwta0 child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
