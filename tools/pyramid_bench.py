"""GPU timings of the pyramid level (sgm_set_pyramid_params level 1) beside level 0, in one process
and one run: device-resident frames, HIP events around blocks of matches, level-0 and level-1 blocks
alternated over the rounds, then a profiled pass for the per-stage times.

    python tools/pyramid_bench.py [--rounds 5] [--frames 64] [--case TEXT] [--out profiles/pyramid.jsonl]
Pairs: census 1920x1080 D=128 and D=256 as a lone sgm_match_device frame and as a 64-frame
sgm_match_device_batch; census 4096x3000 D=512; SGBM5 and BM 2448x2048 minD 147 D 480 window 21 (the
shipped launch frame); census 2448x2048 D=752 at level 1 only (level 0 refuses the range).
One JSON line per pair with both levels' ms per frame (median of the rounds, and every round),
whether level 1 won every round, the level-0 time of a frame of the coarse size and range (a third
engine, in the same alternation), the two new stages' device times from the profiled pass, the
stages of both levels, and the box's measured HBM copy rate.
A last line, at 1920x1080 D=256 with the median on: the `median3` stage of the level-0 frame and
`pyr_down` + `pyr_refine` of the level-1 frame, per round of the same run, and the condition
pyr_down + pyr_refine <= 10.5 x median3 (21 B/px against 4 B/px, doubled for the gathers and
popcounts). median3 is taken at level 0 because at level 1 it runs on the coarse image.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

BIG = dict(min_disparity=147, num_disparities=480, block_size=21, uniqueness_ratio=2, prefilter_cap=7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternated level-0 / level-1 blocks")
    ap.add_argument("--frames", type=int, default=64, help="frames of a batch")
    ap.add_argument("--batch-reps", type=int, default=2, help="batches per timed block")
    ap.add_argument("--single-reps", type=int, default=10, help="lone frames per timed block")
    ap.add_argument("--case", default="", help="run only the pairs whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    census = dict(p1=10, p2=120, uniqueness_ratio=5, disp12_max_diff=1, median=0, speckle_window_size=0)
    C, S, B = pkg.MODE_CENSUS8, pkg.MODE_OCV_SGBM5, pkg.MODE_OCV_BM
    # name, H, W, mode, parameters, frames per call, level 0 runs
    cases = [("census 1920x1080 D=128 lone frame", 1080, 1920, C, dict(census, num_disparities=128), 1, True),
             ("census 1920x1080 D=128 batch", 1080, 1920, C, dict(census, num_disparities=128), a.frames, True),
             ("census 1920x1080 D=256 lone frame", 1080, 1920, C, dict(census, num_disparities=256), 1, True),
             ("census 1920x1080 D=256 batch", 1080, 1920, C, dict(census, num_disparities=256), a.frames, True),
             ("census 4096x3000 D=512 lone frame", 3000, 4096, C, dict(census, num_disparities=512), 1, True),
             ("sgbm5 2448x2048 minD=147 D=480 window 21 lone frame", 2048, 2448, S,
              dict(BIG, speckle_window_size=1000, speckle_range=4, p1=200, p2=400), 1, True),
             ("bm 2448x2048 minD=147 D=480 window 21 lone frame", 2048, 2448, B,
              dict(BIG, speckle_window_size=1000, speckle_range=4), 1, True),
             ("census 2448x2048 D=752 lone frame", 2048, 2448, C, dict(census, num_disparities=752), 1, False)]
    st = torch.cuda.Stream()
    lines = []

    def timed(run, reps, per_call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1) / (reps * per_call)

    def profiled(eng, run, reps):
        eng.set_profiling(True)
        for _ in range(reps):
            run()
        st.synchronize()
        launches = eng.stage_launches()
        stages = [{"name": n, "avg_ms": round(t, 4), "alg_bytes": b, "launches": launches.get(n, 0)}
                  for n, t, b in eng.stage_times()]
        eng.set_profiling(False)
        return stages

    for name, H, W, mode, kw, per_call, has0 in cases:
        if a.case not in name:
            continue
        p = pkg.default_params(mode, **kw)
        m, D = p.min_disparity, p.num_disparities
        plan = pkg.pyramid_plan(p, pkg.default_pyramid_params(level=1), W, H)
        Wc, Hc = plan["Wc"], plan["Hc"]
        # level 0, level 1, and level 0 on a frame of the coarse size and range
        eng = {k: pkg.Engine(0) for k in ((0, 1, "coarse") if has0 else (1, "coarse"))}
        for k, e in eng.items():
            e.set_params(p if k != "coarse" else p.copy(min_disparity=plan["mc"], num_disparities=plan["Dc"]))
            e.set_pyramid_params(pkg.default_pyramid_params(level=1 if k == 1 else 0))
        nd = 4 if per_call > 1 else 1
        full = [synth.stereo_pair(H, W, max(m, 0), D, seed=i, with_truth=False)[:2] for i in range(nd)]
        small = [synth.stereo_pair(Hc, Wc, max(plan["mc"], 0), plan["Dc"], seed=i, with_truth=False)[:2] for i in range(nd)]
        dev = {"full": [[torch.from_numpy(x).cuda() for x in f] for f in full],
               "small": [[torch.from_numpy(x).cuda() for x in f] for f in small]}
        out = torch.empty((per_call, H, W), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()

        def runner(k):
            e = eng[k]
            fr = dev["small" if k == "coarse" else "full"]
            w, h = (Wc, Hc) if k == "coarse" else (W, H)
            pl = [fr[f % nd][0].data_ptr() for f in range(per_call)]
            pr_ = [fr[f % nd][1].data_ptr() for f in range(per_call)]
            po = [out[f].data_ptr() for f in range(per_call)]
            if per_call == 1:
                return lambda: e.match_device(pl[0], pr_[0], w, h, w, po[0], w, st.cuda_stream)
            return lambda: e.match_device_batch(pl, pr_, w, h, w, po, w, st.cuda_stream)

        runs = {k: runner(k) for k in eng}
        reps = a.single_reps if per_call == 1 else a.batch_reps
        copy_gbps = bench.hbm_copy_gbps(0)
        rounds = {k: [] for k in eng}
        with torch.cuda.stream(st):
            for k in eng:                                  # warm-up: workspaces, work lists, first launches
                runs[k]()
                runs[k]()
            st.synchronize()
            for _ in range(a.rounds):                      # alternated blocks: same box, same run
                for k in eng:
                    rounds[k].append(timed(runs[k], reps, per_call))
            stages = {k: profiled(eng[k], runs[k], reps) for k in eng}
        med = {k: statistics.median(v) for k, v in rounds.items()}
        new = {s["name"]: s["avg_ms"] for s in stages[1] if s["name"] in ("pyr_down", "pyr_refine")}
        rec = {"tool": "pyramid_bench", "when": time.strftime("%Y-%m-%d %H:%M:%S"), "case": name,
               "hbm_copy_GBps": copy_gbps, "frames_per_call": per_call, "reps": reps, "coarse": plan,
               "level1_ms_per_frame": round(med[1], 4), "level1_rounds_ms": [round(v, 4) for v in rounds[1]],
               "coarse_level0_ms_per_frame": round(med["coarse"], 4),
               "coarse_level0_rounds_ms": [round(v, 4) for v in rounds["coarse"]],
               "pyr_down_ms": new.get("pyr_down"), "pyr_refine_ms": new.get("pyr_refine"),
               "coarse_plus_new_stages_ms": round(med["coarse"] + sum(v for v in new.values()), 4),
               "level1_stages": stages[1], "coarse_level0_stages": stages["coarse"]}
        if has0:
            rec.update({"level0_ms_per_frame": round(med[0], 4), "level0_rounds_ms": [round(v, 4) for v in rounds[0]],
                        "speedup": round(med[0] / med[1], 3),
                        "level1_faster_every_round": all(x < y for x, y in zip(rounds[1], rounds[0])),
                        "level0_stages": stages[0]})
        else:
            rec["level0"] = "refused: SGM_ERR_UNSUPPORTED (census numDisparities > 512)"
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        for e in eng.values():
            e.close()
        del dev, out
        torch.cuda.empty_cache()

    if "stages" in a.case or not a.case:
        # the new stages beside median3, 1920x1080 D=256, the same frame, every round of one run
        H, W, D = 1080, 1920, 256
        p = pkg.default_params(C, **dict(census, num_disparities=D, median=1))
        left, right = synth.stereo_pair(H, W, 0, D, seed=3, with_truth=False)[:2]
        dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        out = torch.empty((H, W), dtype=torch.int16, device="cuda")
        eng = {k: pkg.Engine(0) for k in (0, 1)}
        for k, e in eng.items():
            e.set_params(p)
            e.set_pyramid_params(pkg.default_pyramid_params(level=k))
        copy_gbps = bench.hbm_copy_gbps(0)
        rows = {"median3": [], "pyr_down": [], "pyr_refine": []}
        with torch.cuda.stream(st):
            for k in eng:
                eng[k].match_device(dl.data_ptr(), dr.data_ptr(), W, H, W, out.data_ptr(), W, st.cuda_stream)
            st.synchronize()
            for _ in range(a.rounds):
                for k in eng:
                    got = {s["name"]: s["avg_ms"] for s in profiled(
                        eng[k], lambda: eng[k].match_device(dl.data_ptr(), dr.data_ptr(), W, H, W, out.data_ptr(), W,
                                                            st.cuda_stream), a.single_reps)}
                    for n in (("median3",) if k == 0 else ("pyr_down", "pyr_refine")):
                        rows[n].append(got[n])
        ratios = [(d + r) / m3 for d, r, m3 in zip(rows["pyr_down"], rows["pyr_refine"], rows["median3"])]
        rec = {"tool": "pyramid_bench", "when": time.strftime("%Y-%m-%d %H:%M:%S"),
               "case": "new stages alone 1920x1080 D=256", "hbm_copy_GBps": copy_gbps, "unit": "ms per launch, per round",
               "rows": {k: [round(v, 4) for v in vs] for k, vs in rows.items()},
               "median": {k: round(statistics.median(vs), 4) for k, vs in rows.items()},
               "new_stages_alg_GBps": round(21.0 * W * H / ((statistics.median(rows["pyr_down"]) +
                                                             statistics.median(rows["pyr_refine"])) * 1e-3) / 1e9, 1),
               "ratio_per_round": [round(v, 2) for v in ratios],
               "condition": "pyr_down + pyr_refine <= 10.5 x median3 (level-0 frame), every round",
               "met": all(v <= 10.5 for v in ratios)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        for e in eng.values():
            e.close()
    if a.out and lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
