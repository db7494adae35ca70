"""GPU timings of the census mode with 4 aggregation paths (sgm_set_census_paths(4)) beside the
default 8, in one process and one run: device-resident frames, HIP events around blocks of
matches, 8-path and 4-path blocks alternated, then a separate profiled pass for the per-stage
times and their algorithmic bytes (sgm_stage_bytes).

    python tools/census_paths_bench.py [--rounds 5] [--frames 64] [--out profiles/census_paths.jsonl]
Geometries: 1920x1080 D=128 (BASELINE C2: no sub-pixel / LR) and D=256 (C3: sub-pixel + LR), each
as a 64-frame sgm_match_device_batch and as a lone sgm_match_device frame. One JSON line per
geometry and form with both sets' ms per frame and pairs/s (median of the rounds, and every
round), whether 4 paths won every round, the stages, the box's measured HBM copy rate, and the
4-path steady launch's algorithmic bytes over its time against that rate.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

STEADY = {8: "paths7+up_wta+census", 4: "paths3+up_wta+census"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternated 8-path / 4-path blocks")
    ap.add_argument("--frames", type=int, default=64, help="frames of a batch")
    ap.add_argument("--batch-reps", type=int, default=3, help="batches per timed block")
    ap.add_argument("--single-reps", type=int, default=30, help="lone frames per timed block")
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic pairs")
    ap.add_argument("--case", default="", help="run only the cases whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_paths.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    H, W = 1080, 1920
    geoms = [("C2 1920x1080 D=128", 128, dict(subpixel=0, lr_check=0)),
             ("C3 1920x1080 D=256", 256, dict(subpixel=1, lr_check=1))]
    engines = {8: pkg.Engine(0), 4: pkg.Engine(0)}
    engines[4].set_census_paths(4)
    st = torch.cuda.Stream()
    out = torch.empty((a.frames, H, W), dtype=torch.int16, device="cuda")
    lines = []
    for gname, D, flags in geoms:
        params = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=0, p1=10, p2=120,
                                    uniqueness_ratio=5, disp12_max_diff=1, median=0, speckle_window_size=0, **flags)
        for e in engines.values():
            e.set_params(params)
        dl, dr = [], []
        for i in range(a.distinct):
            l, r, _ = synth.stereo_pair(H, W, 0, D, seed=i, with_truth=False)
            dl.append(torch.from_numpy(l).cuda())
            dr.append(torch.from_numpy(r).cuda())
        ptr_l = [dl[f % len(dl)].data_ptr() for f in range(a.frames)]
        ptr_r = [dr[f % len(dr)].data_ptr() for f in range(a.frames)]
        ptr_o = [out[f].data_ptr() for f in range(a.frames)]
        torch.cuda.synchronize()
        forms = [("batch", a.batch_reps, a.frames,
                  lambda k: engines[k].match_device_batch(ptr_l, ptr_r, W, H, W, ptr_o, W, st.cuda_stream)),
                 ("lone frame", a.single_reps, 1,
                  lambda k: engines[k].match_device(ptr_l[0], ptr_r[0], W, H, W, ptr_o[0], W, st.cuda_stream))]
        for fname, reps, per_call, run in forms:
            name = f"{gname} {fname}"
            if a.case not in name:
                continue
            copy_gbps = bench.hbm_copy_gbps(0)
            rounds = {k: [] for k in engines}
            stages = {}
            with torch.cuda.stream(st):
                for k in engines:                      # warm-up: workspace, work lists, first launches
                    run(k)
                    run(k)
                st.synchronize()
                for _ in range(a.rounds):              # alternated blocks: same box, same run
                    for k in engines:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        for _ in range(reps):
                            run(k)
                        e1.record(st)
                        st.synchronize()
                        rounds[k].append(e0.elapsed_time(e1) / (reps * per_call))
                for k in engines:                      # per-stage HIP events, a separate pass
                    engines[k].set_profiling(True)
                    for _ in range(reps):
                        run(k)
                    st.synchronize()
                    launches = engines[k].stage_launches()
                    stages[k] = [{"name": n, "avg_ms": round(t, 4), "alg_bytes": b, "launches": launches.get(n, 0)}
                                 for n, t, b in engines[k].stage_times()]
                    engines[k].set_profiling(False)
            med = {k: statistics.median(rounds[k]) for k in engines}
            rec = {"case": name, "hbm_copy_GBps": copy_gbps, "frames_per_call": per_call, "reps": reps,
                   "paths8_ms_per_frame": round(med[8], 4), "paths4_ms_per_frame": round(med[4], 4),
                   "paths8_pairs_per_s": round(1e3 / med[8], 1), "paths4_pairs_per_s": round(1e3 / med[4], 1),
                   "speedup": round(med[8] / med[4], 3),
                   "paths8_rounds_ms": [round(v, 4) for v in rounds[8]],
                   "paths4_rounds_ms": [round(v, 4) for v in rounds[4]],
                   "paths4_faster_every_round": all(f < e for f, e in zip(rounds[4], rounds[8])),
                   "paths8_stages": stages[8], "paths4_stages": stages[4]}
            for k in engines:                          # the steady launch against the copy rate
                s = next((s for s in stages[k] if s["name"] == STEADY[k]), None)
                if s and s["avg_ms"] > 0:
                    gbps = s["alg_bytes"] / (s["avg_ms"] * 1e-3) / 1e9
                    rec[f"paths{k}_steady_alg_GBps"] = round(gbps, 1)
                    rec[f"paths{k}_steady_over_copy_rate"] = round(gbps / copy_gbps, 3)
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
