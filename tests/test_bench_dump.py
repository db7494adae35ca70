"""bench.py --dump-outputs on CPU: dump_outputs() writes an output within the size limit whole and
a larger one as first frame, last frame and a seeded sample that is the same in every run; the
files are float32 and stay within the limit. `--full` and `--dump-outputs` are options of the
command line."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _disp(frames, h, w, seed):
    return np.random.default_rng(seed).integers(-16, 4096, (frames, h, w)).astype(np.int16)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_output_is_written_whole(tmp_path):
    a = _disp(3, 17, 29, 1)
    shapes = bench.dump_outputs(str(tmp_path / "o"), a)
    got = _load(tmp_path / "o")
    assert list(got) == ["disparity"] and shapes == {"disparity": [3, 17, 29]}
    assert got["disparity"].dtype == np.float32 and np.array_equal(got["disparity"], a)


def test_list_of_host_frames_is_stacked(tmp_path):
    a = _disp(2, 5, 7, 2)
    bench.dump_outputs(str(tmp_path), [a[0], a[1]])
    assert np.array_equal(_load(tmp_path)["disparity"], a)


def test_large_output_is_sampled_the_same_way_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 300)
    a = _disp(6, 13, 23, 3)                       # 1794 elements: 7176 B as float32, over the limit
    bench.dump_outputs(str(tmp_path / "a"), a)
    bench.dump_outputs(str(tmp_path / "b"), a)
    ga, gb = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(ga) == ["disparity_first_frame", "disparity_last_frame", "disparity_sample"]
    assert all(v.dtype == np.float32 for v in ga.values())
    assert sum(v.nbytes for v in ga.values()) <= 4 * 1000
    assert np.array_equal(ga["disparity_first_frame"], a[0]) and np.array_equal(ga["disparity_last_frame"], a[-1])
    idx = np.sort(np.random.default_rng(0).integers(0, a.size, 300))
    assert np.array_equal(ga["disparity_sample"], a.reshape(-1)[idx])
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)
    # a change anywhere in a sampled element shows in the sample
    b = a.copy()
    b.reshape(-1)[idx[150]] += 1
    bench.dump_outputs(str(tmp_path / "c"), b)
    assert not np.array_equal(_load(tmp_path / "c")["disparity_sample"], ga["disparity_sample"])


def test_default_limits():
    assert bench.DUMP_LIMIT_BYTES == 64 * 1000 * 1000
    # the 64-frame 1080p batch: two whole frames and the sample fit
    assert 2 * 1920 * 1080 * 4 + bench.DUMP_SAMPLE * 4 <= bench.DUMP_LIMIT_BYTES


def test_options_exist():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs DIR" in p.stdout
