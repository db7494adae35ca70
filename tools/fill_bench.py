"""Device time of the hole filter (stage `fill`, csrc/fill.hip) next to the median3 stage, 1920x1080,
in one process and one run.

Per round, in this order (so the rows are interleaved over rounds):
  - one census C3 match (1920x1080, D = 256) with median on and the filter on at each gap, under the
    handle's profiling: the `median3` and `fill` stage times (hipEvents around each launch) of the
    same frame. The uniqueness ratio is raised until the window has at least --holes of holes.
  - sgm_fill_holes alone, HIP events around --reps launches on a stream, at each gap, on three inputs:
    that match's unfilled output, an all-invalid window, and 50 % salt-and-pepper holes.
The condition written with the record: at G = 16, fill <= 8 x median3 on each of the three inputs
(the factor comes from bytes: median3 moves 4 B/px, the carry form at most 2 + 2 B/px plus three
int16 planes written and read once = 16 B/px, doubled for the warm-up halos and the second dependent
sweep). The G = 255 times are reported beside them.

    python tools/fill_bench.py [--rounds 5] [--reps 20] [--holes 0.10] [--out profiles/fill.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

H, W, D = 1080, 1920, 256
GAPS = (16, 255)


def window_holes(disp, invalid):
    return float((disp[:, D:] == invalid).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--holes", type=float, default=0.10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill.jsonl"))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    left, right, _ = synth.stereo_pair(H, W, 0, D, seed=3)
    eng = pkg.Engine(0)
    invalid = -16
    # the census C3 output with the uniqueness ratio raised until the window has enough holes
    for uniq in (5, 20, 40, 60, 80, 95):
        p = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, uniqueness_ratio=uniq, median=1)
        eng.set_params(p)
        census = eng.match(left, right)
        share = window_holes(census, invalid)
        if share >= a.holes:
            break
    rng = np.random.default_rng(1)
    allinv = census.copy()
    allinv[:, D:] = invalid
    salt = census.copy()
    sub = salt[:, D:]
    sub[sub == invalid] = 800                   # a valid value first, then exactly the drawn holes
    sub[rng.random(sub.shape) < 0.5] = invalid
    inputs = {"census": census, "all_invalid": allinv, "salt50": salt}
    shares = {k: window_holes(v, invalid) for k, v in inputs.items()}
    dev = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}
    out = torch.empty((H, W), dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    rect = (D, 0, W, H)

    def alone(name, G):
        f = pkg.default_fill_params(mode=pkg.FILL_BACKGROUND, max_gap=G, min_neighbours=2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            eng.fill_holes(dev[name].data_ptr(), W, W, H, invalid, f, rect, out.data_ptr(), W, stream.cuda_stream)
            e0.record(stream)
            for _ in range(a.reps):
                eng.fill_holes(dev[name].data_ptr(), W, W, H, invalid, f, rect, out.data_ptr(), W, stream.cuda_stream)
            e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def staged(G):
        eng.set_fill_params(pkg.default_fill_params(mode=pkg.FILL_BACKGROUND, max_gap=G, min_neighbours=2))
        eng.match(left, right)
        eng.set_profiling(True)
        for _ in range(3):
            eng.match(left, right)
        st = {s[0]: s[1] for s in eng.stage_times()}
        eng.set_profiling(False)
        eng.set_fill_params(pkg.default_fill_params())
        return st["median3"], st["fill"]

    rows = {}
    for r in range(a.rounds):
        for G in GAPS:
            med, fill = staged(G)
            rows.setdefault(("stage", "median3", G), []).append(med)
            rows.setdefault(("stage", "fill census", G), []).append(fill)
            for name in inputs:
                rows.setdefault(("alone", name, G), []).append(alone(name, G))
    med16 = statistics.median(rows[("stage", "median3", 16)])
    rec = dict(tool="fill_bench", when=time.strftime("%Y-%m-%d %H:%M:%S"), frame=f"{W}x{H} D={D}", uniqueness=uniq,
               window_hole_share=shares, rounds=a.rounds, reps=a.reps, unit="ms per launch, per round",
               rows=[dict(kind=k[0], what=k[1], gap=k[2], ms=[round(v, 4) for v in vs],
                          median=round(statistics.median(vs), 4)) for k, vs in rows.items()])
    cond = {}
    for name in inputs:
        t16 = statistics.median(rows[("alone", name, 16)])
        t255 = statistics.median(rows[("alone", name, 255)])
        cond[name] = dict(fill_g16_ms=round(t16, 4), median3_ms=round(med16, 4), ratio=round(t16 / med16, 2),
                          met=bool(t16 <= 8 * med16), fill_g255_ms=round(t255, 4), g255_over_g16=round(t255 / t16, 2))
    rec["condition"] = "G = 16: fill <= 8 x median3 on each input"
    rec["result"] = cond
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec, indent=1))
    eng.close()


if __name__ == "__main__":
    main()
