"""GPU timings of raw frames through the OpenCV and BM modes, in one process and one run:
device-resident frames, HIP events around blocks of batches (about 150 ms of work each), the
configurations alternated over rounds (each round starts one configuration further on) and their
medians, minima and maxima reported (as tools/color_bench.py does):

  (a) rect_mono    pre-rectified 8UC1 frames, the matcher alone (sgm_match_device_batch)
  (b) remap_match  what a caller did before the pre-pass existed: two sgm_remap_cubic per frame
                   into its own rectified images, then the match on those
  (c) raw_mono     raw 8UC1 frames through sgm_set_rectification + sgm_match_device_batch_rect,
                   both rectified outputs requested
  (d) raw_colour   raw 8UC3 frames (sgm_set_raw_format(3, Y14)), both rectified 8UC3 outputs

for SGM_MODE_OCV_BM and SGM_MODE_OCV_SGBM5 at the node default (640x480, minD 9, D 64, window /
block 15, speckle filter 100 / 4) and at the shipped launch frame (2448x2048, minD 147, D 480,
block 21). The `rectify` stage's time comes from a separate profiled pass and is set against the
device's copy rate measured in the same run.

    python tools/rect_modes_bench.py [--rounds 7] [--parent-lib PATH] [--out profiles/rect_modes.jsonl]

--parent-lib: a libsgm_hip.so built from the parent commit; its row (a) is timed in the same
rounds (`parent_rect_mono`), and at the small size so is row (a) on a second handle of this build
(`rect_mono_2nd_handle`: what two handles of one library differ by; the shipped frame's
workspaces are too large for a third handle). Two conditions are evaluated and written with
their numbers:
  raw_mono median <= remap_match median + (remap_match max - min)
  rect_mono median <= parent_rect_mono median + (parent max - min)
"""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tools.color_bench import calibration, colourize, timed  # noqa: E402

CASES = [("node default 640x480 D=64", 480, 640, dict(), 8, 4),
         ("shipped 2448x2048 minD=147 D=480 block 21", 2048, 2448,
          dict(min_disparity=147, num_disparities=480, block_size=21), 1, 2)]


def load_variant(path):
    """A second copy of the package bound to another libsgm_hip.so (the module keeps one library)."""
    spec = importlib.util.spec_from_file_location("sgm_parent_variant", os.path.join(ge.PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[ge.PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["sgm_parent_variant"] = mod
    spec.loader.exec_module(mod)
    mod.load_library(path)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternated blocks per configuration")
    ap.add_argument("--block-ms", type=float, default=150.0, help="work per timed block")
    ap.add_argument("--parent-lib", default=None, help="libsgm_hip.so of the parent commit: its row (a) is timed too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_modes.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    parent = load_variant(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    st = torch.cuda.Stream()
    lines = []
    for cname, H, W, kw, n, reps in CASES:
        D = kw.get("num_disparities", 64)
        minD = kw.get("min_disparity", 9)
        l, r, _ = synth.stereo_pair(H, W, minD, D, seed=1, with_truth=False)
        mono = (torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda())
        colour = (torch.from_numpy(colourize(l)).cuda(), torch.from_numpy(colourize(r)).cuda())
        out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        rect1 = torch.empty((2, n, H, W), dtype=torch.uint8, device="cuda")
        rect3 = torch.empty((2, n, H, W, 3), dtype=torch.uint8, device="cuda")
        maps = torch.empty((4, H, W), dtype=torch.float32, device="cuda")
        ptr_o = [out[f].data_ptr() for f in range(n)]
        pm = [[mono[s].data_ptr()] * n for s in (0, 1)]
        pc = [[colour[s].data_ptr()] * n for s in (0, 1)]
        pr1 = [[rect1[s, f].data_ptr() for f in range(n)] for s in (0, 1)]
        pr3 = [[rect3[s, f].data_ptr() for f in range(n)] for s in (0, 1)]
        ml, mr = (maps[0].data_ptr(), maps[1].data_ptr()), (maps[2].data_ptr(), maps[3].data_ptr())
        for mode_name, mode in (("OCV_BM", pkg.MODE_OCV_BM), ("OCV_SGBM5", pkg.MODE_OCV_SGBM5)):
            eng = pkg.Engine(0, pkg.default_params(mode, **kw))
            peng = parent.Engine(0, parent.default_params(mode, **kw)) if parent else None
            # control at the small size: row (a) on a second handle of this build
            eng2 = pkg.Engine(0, pkg.default_params(mode, **kw)) if n > 1 else None
            for i, sign in enumerate((1, -1)):
                eng.rectify_map(*calibration(W, H, sign), W, H, maps[2 * i].data_ptr(), maps[2 * i + 1].data_ptr(), W)
            eng.synchronize()

            def rect_mono(e=eng):
                e.match_device_batch(pr1[0], pr1[1], W, H, W, ptr_o, W, st.cuda_stream)

            def remap_match():
                for f in range(n):
                    for s in (0, 1):
                        eng.remap_cubic(pm[s][f], W, W, H, maps[2 * s].data_ptr(), maps[2 * s + 1].data_ptr(), W, W, H,
                                        pr1[s][f], W, st.cuda_stream)
                eng.match_device_batch(pr1[0], pr1[1], W, H, W, ptr_o, W, st.cuda_stream)

            def raw(ch):
                eng.set_raw_format(ch, pkg.GRAY_Y14)
                eng.set_rectification(ml, mr, W, W, H)
                try:
                    if ch == 3:
                        eng.match_device_batch_rect(pc[0], pc[1], W, H, 3 * W, pr3[0], pr3[1], 3 * W, ptr_o, W,
                                                    st.cuda_stream)
                    else:
                        eng.match_device_batch_rect(pm[0], pm[1], W, H, W, pr1[0], pr1[1], W, ptr_o, W, st.cuda_stream)
                finally:
                    eng.set_rectification()
                    eng.set_raw_format(1, pkg.GRAY_Y14)

            run = {"remap_match": remap_match, "rect_mono": rect_mono, "raw_mono": lambda: raw(1),
                   "raw_colour": lambda: raw(3)}
            if peng:
                run["parent_rect_mono"] = lambda: rect_mono(peng)
            if eng2:
                run["rect_mono_2nd_handle"] = lambda: rect_mono(eng2)
            copy_gbps = bench.hbm_copy_gbps(0)
            rounds = {c: [] for c in run}
            stages = {}
            with torch.cuda.stream(st):
                for c in run:                              # warm-up: workspaces, lanes, first launches
                    run[c]()
                    run[c]()
                st.synchronize()
                # blocks of about --block-ms of work each, so that a block times the kernels, not the clock
                reps = max(reps, math.ceil(a.block_ms / timed(torch, st, 2, run["rect_mono"])))
                order = list(run)
                for k in range(a.rounds):                  # alternated blocks: same box, same run; every
                    for c in order[k % len(order):] + order[:k % len(order)]:   # round starts one further on
                        rounds[c].append(timed(torch, st, reps, run[c]) / n)
                for c in ("raw_mono", "raw_colour"):       # per-stage HIP events, a separate pass
                    st.synchronize()
                    eng.set_profiling(True)
                    run[c]()
                    st.synchronize()
                    launches = eng.stage_launches()
                    stages[c] = [{"name": s, "avg_ms": round(t, 5), "alg_bytes": b, "launches": launches.get(s, 0)}
                                 for s, t, b in eng.stage_times()]
                    eng.set_profiling(False)
            rec = {"case": f"{mode_name} {cname}, batch of {n}", "hbm_copy_GBps": copy_gbps, "reps": reps}
            for c in run:
                v = rounds[c]
                rec[c] = {"median_ms_per_frame": round(statistics.median(v), 5), "min": round(min(v), 5),
                          "max": round(max(v), 5), "rounds_ms": [round(x, 5) for x in v]}
            b, c = rec["remap_match"], rec["raw_mono"]
            rec["raw_mono_within_remap_match_spread"] = c["median_ms_per_frame"] <= b["median_ms_per_frame"] + b["max"] - b["min"]
            if peng:
                p, t = rec["parent_rect_mono"], rec["rect_mono"]
                rec["rect_mono_within_parent_spread"] = t["median_ms_per_frame"] <= p["median_ms_per_frame"] + p["max"] - p["min"]
            for c in stages:
                rec[f"{c}_stages"] = stages[c]
                for s in stages[c]:
                    if s["name"] == "rectify" and s["avg_ms"] > 0:
                        gbps = s["alg_bytes"] / (s["avg_ms"] * 1e-3) / 1e9
                        rec[f"{c}_rectify"] = {"ms": s["avg_ms"], "alg_GBps": round(gbps, 1),
                                               "over_copy_rate": round(gbps / copy_gbps, 3)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            eng.close()
            if eng2:
                eng2.close()
            if peng:
                peng.close()
    if a.out and lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
