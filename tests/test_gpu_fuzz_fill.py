"""Seeded random cases of the hole filter: the stand-alone entry (sizes, invalid value, hole
pattern, rectangle, gap, neighbours, rule drawn per seed) and one match entry point (a device batch
in a drawn mode with the filter on), each bit for bit against tests/fill_reference.py; and the C++
adapter core's driver (plugin_fill_test match) against the oracle followed by the reference.
SGM_FILL_FUZZ_CASES (default 40) sets the number of cases.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_paths_reference as cpr  # noqa: E402
import fill_reference as fr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402
from conftest import to_oracle_params  # noqa: E402
from test_gpu_fill import _device_batch, diff_msg, fill_params, window_holes  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "plugin_fill_test")
N_CASES = int(os.environ.get("SGM_FILL_FUZZ_CASES", "40"))


@pytest.mark.parametrize("seed", range(N_CASES))
def test_fuzz_fill_alone(engine, pkg, seed):
    rng = np.random.default_rng(410_000 + seed)
    h, w = int(rng.integers(1, 150)), int(rng.integers(1, 420))
    inv = int(rng.choice([-16, -96, 32, 160]))
    img = rng.integers(-200, 2000, (h, w)).astype(np.int16)
    kind = seed % 4
    if kind == 0:
        img[rng.random((h, w)) < rng.choice([0.05, 0.3, 0.7, 0.97])] = inv
    elif kind == 1:                       # blocks
        for _ in range(int(rng.integers(1, 9))):
            bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
            y, x = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
            img[y:y + bh, x:x + bw] = inv
    elif kind == 2:                       # mostly invalid, a few islands
        keep = rng.random((h, w)) < 0.01
        img[~keep] = inv
    else:                                 # stripes: whole rows and columns
        img[rng.random(h) < 0.5, :] = inv
        img[:, rng.random(w) < 0.5] = inv
    G = int(rng.choice([1, 2, 5, 16, 47, 48, 49, 100, 160, 161, 255]))
    N, mode = int(rng.integers(1, 9)), int(rng.choice([fr.BACKGROUND, fr.MEDIAN]))
    x0, y0 = int(rng.integers(0, w + 1)), int(rng.integers(0, h + 1))
    rect = (x0, y0, int(rng.integers(x0, w + 1)), int(rng.integers(y0, h + 1))) if seed % 3 else (0, 0, w, h)
    ref = fr.fill_holes(img, inv, mode, G, N, rect)
    got = engine.fill(img, inv, fill_params(pkg, mode, G, N), rect)
    assert np.array_equal(got, ref), f"{h}x{w} inv {inv} kind {kind} G {G} N {N} mode {mode} rect {rect}: " + \
        diff_msg(got, ref)


@pytest.mark.parametrize("seed", range(N_CASES))
def test_fuzz_fill_in_a_device_batch(engine, oracle, synth, pkg, seed):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(420_000 + seed)
    mode = ["census", "census4", "sgbm5", "hh8", "bm"][seed % 5]
    D = int(rng.choice([16, 32, 64]))
    minD = int(rng.integers(-4, 8))
    h, w = int(rng.integers(12, 90)), int(rng.integers(D + minD + 12, D + minD + 160))
    n = int(rng.integers(1, 4))
    uniq = int(rng.choice([15, 40, 70]))
    frames = [synth.stereo_pair(h, w, max(minD, 0), D, seed=seed * 5 + i)[:2] for i in range(n)]
    if mode.startswith("census"):
        kw = dict(min_disparity=minD, num_disparities=D, uniqueness_ratio=uniq, median=int(rng.integers(0, 2)),
                  speckle_window_size=int(rng.choice([0, 30])), speckle_range=1)
        p = pkg.default_params(pkg.MODE_CENSUS8, **kw)
        op = to_oracle_params(oracle, p)
        refs = [oracle.match(op, l, r) if mode == "census" else cpr.match_paths(oracle, op, l, r) for l, r in frames]
    else:
        kw = dict(rm.mode_kw(mode, minD, D, block=5 if mode == "bm" else int(rng.choice([3, 5])),
                             speckle=bool(rng.random() < 0.3)), uniqueness_ratio=uniq)
        p = pkg.default_params(rm.MODE_ID[mode], **kw)
        refs = [rm.match_ref(oracle, mode, kw, l, r) for l, r in frames]
    G, N = int(rng.choice([1, 3, 16, 60, 200])), int(rng.integers(1, 6))
    fmode = int(rng.choice([fr.BACKGROUND, fr.MEDIAN]))
    rect = fr.match_rect(mode == "bm", minD, D, p.block_size, w, h)
    inv = (minD - 1) * 16
    what = f"{mode} {w}x{h} minD {minD} D {D} n {n} fill {fmode} G {G} N {N} {kw}"
    engine.set_params(p)
    engine.set_bm_params(pkg.default_bm_params(texture_threshold=rm.BM_TEXTURE))
    engine.set_census_paths(4 if mode == "census4" else 8)
    engine.set_fill_params(fill_params(pkg, fmode, G, N))
    try:
        got = _device_batch(torch, engine, frames, h, w, pad_out=int(rng.integers(0, 4)))
    finally:
        engine.set_fill_params(pkg.default_fill_params())
        engine.set_census_paths(8)
    for i in range(n):
        want = fr.fill_holes(refs[i], inv, fmode, G, N, rect)
        assert np.array_equal(got[i], want), f"frame {i}, {what}: " + diff_msg(got[i], want)


def driver_frame(w=144, h=56):
    """The frame of plugin/plugin_fill_test.cpp: plugin_paths_test's, with unrelated noise in the right
    image's 12 x 6 patches where (x // 12 + y // 6) % 3 == 0."""
    left, right = cpr.driver_frame(w, h)
    nw = w + 16
    n = np.empty(h * nw, np.int64)
    s = 2024
    for i in range(h * nw):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        n[i] = (s >> 24) & 255
    n = n.reshape(h, nw)
    y, x = np.mgrid[0:h, 0:w]
    patch = (x // 12 + y // 6) % 3 == 0
    right = right.copy()
    right[patch] = n[h - 1 - y, nw - 1 - x][patch]
    return left, right


def test_plugin_driver(oracle, pkg):
    """plugin_fill_test match: the adapter core's forwardMatch with the filter off / background /
    median, and with SGM_HIP_FILL_WHEN's rule (interp on: the forward disparity filled, not Q3;
    interp off: unfilled)."""
    left, right = driver_frame()
    p = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=0, num_disparities=32, uniqueness_ratio=40, p1=8, p2=64,
                           disp12_max_diff=1, block_size=5, prefilter_cap=0, speckle_window_size=0, speckle_range=0)
    ref = oracle.match(to_oracle_params(oracle, p), left, right)
    rect = fr.match_rect(False, 0, 32, 5, 144, 56)
    assert window_holes(ref, rect, -16) >= 0.05
    want = {"off": ref, "background": fr.fill_holes(ref, -16, fr.BACKGROUND, 16, 2, rect),
            "median": fr.fill_holes(ref, -16, fr.MEDIAN, 3, 1, rect)}
    want["interp_on"], want["interp_off"] = want["background"], ref
    assert len({cpr.fnv1a16(v) for v in (want["off"], want["background"], want["median"])}) == 3
    env = {k: v for k, v in os.environ.items() if k not in ("SGM_HIP_FILL", "SGM_HIP_FILL_WHEN")}
    r = subprocess.run([DRIVER, "match"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "fill match ok" in r.stdout, r.stdout + r.stderr
    got = dict(line.split(" hash ") for line in r.stdout.splitlines() if " hash " in line)
    assert got == {k: "%016x" % cpr.fnv1a16(v) for k, v in want.items()}
