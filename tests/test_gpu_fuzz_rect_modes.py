"""Seeded random cases of raw frames through the OpenCV and BM modes (sgm_set_rectification +
sgm_match_device_batch_rect): mode, channels, grey set, raw and rectified sizes, calibrations,
disparity range and frame count are drawn per seed, and every rectified image and disparity is
compared bit for bit with the reference composed in tests/rect_modes_reference.py.
SGM_RECT_FUZZ_CASES (default 24) sets the number of cases.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm_reference as br  # noqa: E402
import color_reference as cr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402
from test_gpu_color import _bm_sad_volume_fast  # noqa: E402
from test_gpu_rect_modes import _batch, _set_mode, diff_msg  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("SGM_RECT_FUZZ_CASES", "24"))


@pytest.mark.parametrize("seed", range(N_CASES))
def test_fuzz_raw_frames_in_ocv_and_bm_modes(engine, oracle, synth, pkg, monkeypatch, seed):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(230_000 + seed)
    mode = rm.MODES[seed % 3]                           # every mode gets a third of the cases
    ch = int(rng.choice([1, 3]))
    s = int(rng.choice([cr.GRAY_Y14, cr.GRAY_Y15]))
    D = int(rng.choice([16, 32, 64]))
    minD = int(rng.integers(-4, 8))
    rh, rw = int(rng.integers(8, 120)), int(rng.integers(D + minD + 8, D + minD + 200))
    h, w = max(int(rh * rng.uniform(0.8, 1.1)), 6), max(int(rw * rng.uniform(0.9, 1.1)), D + minD + 1)
    cal = [calib(seed=int(rng.integers(0, 1000)), w=rw, h=rh) for _ in range(2)]
    n = int(rng.integers(1, 5))
    block = 5 if min(h, w) <= 9 else int(rng.choice([5, 9]))        # BM: window < min(W, H)
    kw = rm.mode_kw(mode, minD, D, block=block if mode == "bm" else int(rng.choice([3, 5])),
                    speckle=bool(rng.random() < 0.25))
    maps = [oracle.rectify_map(*c, w, h) for c in cal]
    frames = [rm.raw_frames(synth, rh, rw, minD, D, seed * 7 + i, ch) for i in range(n)]
    what = f"{mode} ch {ch} set {s} raw {rw}x{rh} -> {w}x{h} minD {minD} D {D} n {n} {kw}"
    _set_mode(engine, pkg, oracle, mode, kw)
    got, gl, gr = _batch(torch, engine, maps, frames, h, w, ch, s)
    for i, f in enumerate(frames):
        el, er = rm.rectified(oracle, f[0], *maps[0]), rm.rectified(oracle, f[1], *maps[1])
        assert np.array_equal(gl[i], el) and np.array_equal(gr[i], er), f"frame {i} rectified, {what}"
        a, b = rm.grey_of(el, s), rm.grey_of(er, s)
        if mode == "bm" and i == 0 and h * w * D <= 300_000:
            # the box-sum form of the window sums used below equals bm_reference's direct sums
            assert np.array_equal(rm.match_ref(oracle, mode, kw, a, b), _fast_bm(monkeypatch, oracle, kw, a, b)), what
        ref = _fast_bm(monkeypatch, oracle, kw, a, b) if mode == "bm" else rm.match_ref(oracle, mode, kw, a, b)
        assert np.array_equal(got[i], ref), f"frame {i} disparity, {what}: " + diff_msg(got[i], ref)


def _fast_bm(monkeypatch, oracle, kw, a, b):
    with monkeypatch.context() as mp:
        mp.setattr(br, "sad_volume", _bm_sad_volume_fast)
        return rm.match_ref(oracle, "bm", kw, a, b)
