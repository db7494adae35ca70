"""A plain bench.py run on the GPU: `--steps` sets the number of timed steps, the legs beside the
headline figure stay out of it (they belong to `--full`), and `--dump-outputs` writes what the
timed path computed in its last step: the disparity maps of the batch call, equal to the
engine's single-frame result on the same seeded frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_VARS = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


@pytest.mark.timeout(300)
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, pkg, synth):
    import bench
    env = {k: v for k, v in os.environ.items() if k not in RANK_VARS}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "3",
                        "--warmup", "1", "--frames", "4", "--distinct", "2", "--dump-outputs", str(out)], env=env,
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["metric"] == bench.METRIC and res["unit"] == "pairs/s" and res["higher_is_better"] is True
    assert res["dtype"] == "u8" and res["steps"] == 3 and res["warmup"] == 1
    assert res["profiled_frames"] == 3 * 4                    # the timed region ran --steps steps of --frames frames
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(4 * 1000.0 / res["ms_per_step"], rel=1e-3)
    # nothing that takes a run of its own
    assert "c5" not in res and "cpu_baseline" not in res and res["single_frame"] is None
    assert res["roofline"]["measured_copy_GBps"] is None and res["roofline"]["frac"] > 0
    # the dump: the whole 4-frame output, float32, frame f = the seeded pair f % 2
    assert sorted(os.listdir(out)) == ["disparity.npy"] and res["dumped_outputs"] == {"disparity": [4, 1080, 1920]}
    got = np.load(out / "disparity.npy")
    assert got.dtype == np.float32 and got.shape == (4, 1080, 1920)
    cfg = bench.CONFIGS["c2"]
    eng = pkg.Engine(0, pkg.default_params(pkg.MODE_CENSUS8, num_disparities=cfg["D"], min_disparity=0, p1=10, p2=120,
                                           uniqueness_ratio=5, subpixel=cfg["subpixel"], lr_check=cfg["lr_check"],
                                           disp12_max_diff=1, median=0, speckle_window_size=0))
    try:
        for seed in range(2):
            left, right, _ = synth.stereo_pair(1080, 1920, 0, cfg["D"], seed=seed, with_truth=False)
            ref = eng.match(left, right).astype(np.float32)
            for f in (seed, seed + 2):
                assert np.array_equal(got[f], ref), f"frame {f}"
        assert (got[0] != got[1]).any() and (got >= 0).mean() > 0.5
    finally:
        eng.close()
