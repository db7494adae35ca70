"""GPU parity of the interleaved pair layout of the census path volumes.

Inside every G-byte chunk of a volume cell (G = min(D_pad / 16, 16)) byte b holds the chunk's
disparity (b >> 1) + (G / 2)(b & 1), so that the d-1 / d+1 neighbours of a packed pair are whole
registers. Everything that reads the volumes by d has to agree: the debug read-back (which
returns the public [H][width1][D] order), the WTA's tie rule (first minimal d), its S[best +- 1]
look-ups and d >= D masks, and the band seams of the exact tile mode. Every comparison is
bit-exact against the CPU oracle; the frames are the smallest that still run every kernel shape
(2 .. 16 disparities per lane, 16- and 32-lane lines, D below the padded D, a lane straddling D).
"""
import numpy as np
import pytest

from conftest import to_oracle_params

pytestmark = pytest.mark.gpu

ROWS = 24


def _pair(synth, D, minD, seed, rows=ROWS):
    return synth.stereo_pair(rows, D + 96, max(minD, 0), D, seed=seed)[:2]


@pytest.mark.parametrize("minD", [0, 3])
@pytest.mark.parametrize("D", [32, 48, 64, 128, 144, 256, 512])
def test_path_volumes_all_directions(engine, oracle, synth, pkg, D, minD):
    """(a) the eight path volumes through sgm_debug_census_path, in [H][width1][D] order."""
    left, right = _pair(synth, D, minD, seed=1000 + D + minD)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=minD, p1=9, p2=110)
    engine.set_params(p)
    op = to_oracle_params(oracle, p)
    for dirn in range(8):
        got = engine.census_path(left, right, dirn)
        ref = oracle.census_path(op, left, right, dirn)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), f"dir {dirn}: {(got != ref).sum()} of {ref.size} cells differ"


@pytest.mark.parametrize("D", [64, 256, 512])
def test_batch_equals_single_and_oracle(engine, oracle, synth, pkg, D):
    """(b) sgm_match_device_batch of 5 frames (odd: the lone-tail path runs) against
    sgm_match_device and the oracle. Frame 2 is a constant-grey pair: every S ties, so the
    winner must be the first d (uniqueness 0 keeps the pixel, whose disparity is then minD)."""
    torch = pytest.importorskip("torch")
    n = 5
    h, w = ROWS, D + 96
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, uniqueness_ratio=0)
    engine.set_params(p)
    frames = [_pair(synth, D, 0, seed=2000 + 11 * i + D) for i in range(n)]
    grey = np.full((h, w), 128, dtype=np.uint8)
    frames[2] = (grey, grey.copy())
    dl = [torch.from_numpy(np.ascontiguousarray(f[0])).cuda() for f in frames]
    dr = [torch.from_numpy(np.ascontiguousarray(f[1])).cuda() for f in frames]
    out = torch.full((n, h, w), 777, dtype=torch.int16, device="cuda")
    one = torch.full((n, h, w), 555, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    engine.match_device_batch([t.data_ptr() for t in dl], [t.data_ptr() for t in dr], w, h, w,
                              [out[i].data_ptr() for i in range(n)], w, stream.cuda_stream)
    for i in range(n):
        engine.match_device(dl[i].data_ptr(), dr[i].data_ptr(), w, h, w, one[i].data_ptr(), w, stream.cuda_stream)
    stream.synchronize()
    got, single = out.cpu().numpy(), one.cpu().numpy()
    op = to_oracle_params(oracle, p)
    for i, (l, r) in enumerate(frames):
        ref = oracle.match(op, l, r)
        assert np.array_equal(single[i], ref), f"single frame {i}: {(single[i] != ref).sum()} pixels differ"
        assert np.array_equal(got[i], single[i]), f"batch frame {i}: {(got[i] != single[i]).sum()} pixels differ"
    # all S equal: best = the first d = 0 at every pixel the LR check keeps ((minD - 1) * 16: invalid)
    kept = got[2][got[2] != -16]
    assert kept.size > 0 and (kept == 0).all()


def test_tiled_exact_two_bands(engine, oracle, synth, pkg):
    """(c) sgm_match_tiled_exact, 2 bands of a 48-row frame at D = 256: the seam rows seed the
    next band's lines from stored (interleaved) volume rows."""
    D = 256
    left, right = _pair(synth, D, 0, seed=3000, rows=48)
    p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D)
    engine.set_params(p)
    got = engine.match_tiled_exact(left, right, 2)
    ref = oracle.match(to_oracle_params(oracle, p), left, right)
    assert np.array_equal(got, ref), f"{(got != ref).sum()} pixels differ"
