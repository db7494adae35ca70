"""GPU timings of MODE_OCV_BM (cv::StereoBM, csrc/bm.hip) beside MODE_SGBM of the same frame, in
one process and one run: device-resident frames, HIP events around blocks of matches, BM and
SGBM blocks alternated, then a separate profiled pass for the per-stage times.

    python tools/bm_bench.py [--reps 20] [--rounds 5] [--out profiles/bm_modes.jsonl]
Cases: the node default (640x480, minD 9, D 64, window 15, speckles 100 / 4) and the shipped
launch frame (launch/stereo_matcher.launch:20-34: 2448x2048, minD 147, D 480, window 21,
uniqueness 2, texture 10, speckles 1000 / 4, pre-filter cap 7). One JSON line per case with both
modes' ms per frame (median of the rounds, and every round), the per-stage times, the measured
HBM copy rate of the box, and `bm_match` against the lane-op estimate of DESIGN.md (cells x 8
lane-ops at the VALU peak): the measured time and its ratio, never the estimate as a result.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz 32-bit lane-ops per second
VALU_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9
LANE_OPS_PER_CELL = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="matches per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="alternated BM / SGBM blocks")
    ap.add_argument("--case", default="", help="run only the cases whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm_modes.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    copy_gbps = bench.hbm_copy_gbps(0)
    cases = [
        ("node default 640x480 minD 9 D 64 window 15", 480, 640,
         dict(min_disparity=9, num_disparities=64, block_size=15, uniqueness_ratio=15, prefilter_cap=31,
              speckle_window_size=100, speckle_range=4), 10),
        ("shipped launch 2448x2048 minD 147 D 480 window 21", 2048, 2448,
         dict(min_disparity=147, num_disparities=480, block_size=21, uniqueness_ratio=2, prefilter_cap=7,
              speckle_window_size=1000, speckle_range=4), 10),
    ]
    engines = {"bm": pkg.Engine(0), "sgbm": pkg.Engine(0)}
    st = torch.cuda.Stream()
    lines = []
    for name, h, w, kw, tex in cases:
        if a.case not in name:
            continue
        engines["bm"].set_params(pkg.default_params(pkg.MODE_OCV_BM, **kw))
        engines["bm"].set_bm_params(pkg.default_bm_params(texture_threshold=tex))
        engines["sgbm"].set_params(pkg.default_params(pkg.MODE_OCV_SGBM5, p1=200, p2=400, **kw))
        left, right, _ = synth.stereo_pair(h, w, kw["min_disparity"], kw["num_disparities"], seed=3)
        dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        outs = {k: torch.empty((h, w), dtype=torch.int16, device="cuda") for k in engines}
        torch.cuda.synchronize()

        def run(k):
            engines[k].match_device(dl.data_ptr(), dr.data_ptr(), w, h, w, outs[k].data_ptr(), w, st.cuda_stream)

        rounds = {k: [] for k in engines}
        stages = {}
        with torch.cuda.stream(st):
            for k in engines:                      # warm-up: first launches, workspace allocation
                for _ in range(3):
                    run(k)
            st.synchronize()
            for _ in range(a.rounds):              # alternated blocks: same box, same run
                for k in engines:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(a.reps):
                        run(k)
                    e1.record(st)
                    st.synchronize()
                    rounds[k].append(e0.elapsed_time(e1) / a.reps)
            for k in engines:                      # per-stage HIP events, a separate pass
                engines[k].set_profiling(True)
                for _ in range(a.reps):
                    run(k)
                st.synchronize()
                stages[k] = [{"name": n, "avg_ms": round(t, 4), "alg_bytes": b} for n, t, b in engines[k].stage_times()]
                engines[k].set_profiling(False)
        g = pkg.bm_geometry(engines["bm"].get_params(), w, h)
        cells = g["width1"] * (h - 2 * (kw["block_size"] // 2)) * kw["num_disparities"]
        est_ms = cells * LANE_OPS_PER_CELL / VALU_LANE_OPS_PER_S * 1e3
        bm_match = next(s["avg_ms"] for s in stages["bm"] if s["name"] == "bm_match")
        valid = float((outs["bm"] != (kw["min_disparity"] - 1) * 16).float().mean().item())
        rec = {"case": name, "hbm_copy_GBps": copy_gbps, "reps": a.reps,
               "bm_ms_per_frame": round(statistics.median(rounds["bm"]), 4),
               "sgbm_ms_per_frame": round(statistics.median(rounds["sgbm"]), 4),
               "bm_rounds_ms": [round(v, 4) for v in rounds["bm"]],
               "sgbm_rounds_ms": [round(v, 4) for v in rounds["sgbm"]],
               "bm_faster_every_round": all(b < s for b, s in zip(rounds["bm"], rounds["sgbm"])),
               "bm_stages": stages["bm"], "sgbm_stages": stages["sgbm"],
               "bm_cells": cells, "bm_match_ms": bm_match,
               "bm_match_lane_op_estimate_ms": round(est_ms, 4),
               "bm_match_over_estimate": round(bm_match / est_ms, 1),
               "bm_valid_share_of_frame": round(valid, 3)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    for e in engines.values():
        e.close()
    if a.out and lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
