"""GPU fuzz — seeded random census windows, sizes, parameters and entry points, bit-exact against
tests/census_window_reference.py. SGM_FUZZ_CASES scales the case count like the other fuzz files
(120 -> 24 cases here)."""
import os

import numpy as np
import pytest

import census_window_reference as cwr
from conftest import to_oracle_params
from test_gpu_census_paths import _device_batch

pytestmark = pytest.mark.gpu

N_FUZZ = max(1, int(os.environ.get("SGM_FUZZ_CASES", "120")) // 5)


def _case(seed):
    rng = np.random.default_rng(70_000 + seed)
    win = cwr.WINDOWS[int(rng.integers(0, len(cwr.WINDOWS)))]
    D = 16 * int(rng.integers(1, 9))
    minD = int(rng.integers(-20, 21))
    h = int(rng.integers(1, 71))
    span = max(D + minD, 0)
    w = min(260, span + int(rng.integers(1, 100))) if rng.random() < 0.85 else int(rng.integers(1, 261))
    p1 = int(rng.integers(1, 40))
    kw = dict(num_disparities=D, min_disparity=minD, p1=p1, p2=int(rng.integers(p1 + 1, 260)),
              uniqueness_ratio=int(rng.choice([0, 5, 15, 99, 120])), disp12_max_diff=int(rng.choice([-1, 1, 3])),
              subpixel=int(rng.integers(0, 2)), lr_check=int(rng.integers(0, 2)), median=int(rng.integers(0, 2)),
              speckle_window_size=int(rng.choice([0, 0, 20])), speckle_range=int(rng.integers(1, 4)))
    entry = str(rng.choice(["match", "match_f32", "batch", "tiled_exact"]))
    paths = 8 if entry == "tiled_exact" else int(rng.choice([4, 8]))
    n = int(rng.integers(1, 6)) if entry == "batch" else 1
    return rng, win, h, w, kw, entry, paths, n


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz(engine, oracle, synth, pkg, seed):
    torch = pytest.importorskip("torch")
    rng, win, h, w, kw, entry, paths, n = _case(seed)
    D, minD = kw["num_disparities"], kw["min_disparity"]
    p = pkg.default_params(pkg.MODE_CENSUS8, **kw)
    frames = []
    for i in range(n):
        if rng.random() < 0.3:
            frames.append((rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)))
        else:
            frames.append(synth.stereo_pair(h, w, max(minD, 0), D, seed=1000 * seed + i, with_truth=False)[:2])
    dirs = range(8) if paths == 8 else (0, 1, 6, 7)
    refs = [cwr.match(oracle, to_oracle_params(oracle, p), l, r, win, dirs) for l, r in frames]
    what = f"{entry} n={n} {h}x{w} window {win} paths {paths} {kw}"
    engine.set_params(p)
    engine.set_census_window(*win)
    engine.set_census_paths(paths)
    try:
        if entry == "match":
            got = [engine.match(*frames[0])]
        elif entry == "match_f32":
            got = [engine.match_f32(*frames[0])]
            refs = [refs[0].astype(np.float32)]
        elif entry == "tiled_exact":
            got = [engine.match_tiled_exact(frames[0][0], frames[0][1], min(3, h))]
        else:
            got = _device_batch(torch, engine, frames, h, w, pad_in=int(rng.integers(0, 9)), pad_out=int(rng.integers(0, 9)))
    finally:
        engine.set_census_window(*cwr.DEFAULT)
        engine.set_census_paths(8)
    for i in range(n):
        assert np.array_equal(got[i], refs[i]), f"{what} frame {i}: {(got[i] != refs[i]).sum()} pixels differ"
