#!/usr/bin/env python3
"""Census window cost: a lone frame and a 64-frame device batch, ms per frame, for the default
window, (7, 7, 1) and (9, 7, 2) at 1920x1080, D = 128 and 256; one run, interleaved rounds, then
one profiled pass per configuration for the per-stage times. Writes profiles/census_window.jsonl
(one JSON line per configuration) and checks the expectation of DESIGN.md §18:
    batch(window) <= batch(default) + 2 * census stage of the default lone frame.

usage: census_window_bench.py [--rounds N] [--batch N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

WINDOWS = [(9, 7, 1), (7, 7, 1), (9, 7, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_window.jsonl"))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    h, w, nsrc = 1080, 1920, 4
    eng = pkg.Engine(0)
    rows = []
    for D in (128, 256):
        src = [synth.stereo_pair(h, w, 0, D, seed=60 + i, with_truth=False)[:2] for i in range(nsrc)]
        dl = [torch.as_tensor(np.ascontiguousarray(f[0])).cuda() for f in src]
        dr = [torch.as_tensor(np.ascontiguousarray(f[1])).cuda() for f in src]
        outs = torch.empty((a.batch, h, w), dtype=torch.int16, device="cuda")
        lp = [dl[i % nsrc].data_ptr() for i in range(a.batch)]
        rp = [dr[i % nsrc].data_ptr() for i in range(a.batch)]
        op = [outs[i].data_ptr() for i in range(a.batch)]
        eng.set_params(pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D))
        torch.cuda.synchronize()

        def lone(n=20):
            t0 = time.perf_counter()
            for i in range(n):
                eng.match_device(lp[i % nsrc], rp[i % nsrc], w, h, w, op[0], w)
            eng.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def batch():
            t0 = time.perf_counter()
            eng.match_device_batch(lp, rp, w, h, w, op, w)
            eng.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.batch

        t = {win: {"lone": [], "batch": []} for win in WINDOWS}
        for r in range(a.rounds + 1):                     # round 0 warms up (workspace, work lists)
            for win in WINDOWS:
                eng.set_census_window(*win)
                lo, ba = lone(), batch()
                if r:
                    t[win]["lone"].append(lo)
                    t[win]["batch"].append(ba)
        for win in WINDOWS:
            eng.set_census_window(*win)
            stages = {}
            for kind, run in (("lone", lambda: lone(5)), ("batch", batch)):
                eng.set_profiling(True)
                run()
                launches = eng.stage_launches()
                stages[kind] = {s[0]: {"ms_per_launch": round(s[1], 4), "launches": launches.get(s[0], 0)}
                                for s in eng.stage_times()}
                eng.set_profiling(False)
            rows.append({"width": w, "height": h, "D": D, "window": list(win), "rounds": a.rounds, "batch": a.batch,
                         "lone_ms": [round(v, 4) for v in t[win]["lone"]],
                         "batch_ms_per_frame": [round(v, 4) for v in t[win]["batch"]],
                         "lone_ms_median": round(float(np.median(t[win]["lone"])), 4),
                         "batch_ms_per_frame_median": round(float(np.median(t[win]["batch"])), 4), "stages": stages})
        base = next(r for r in rows if r["D"] == D and r["window"] == [9, 7, 1])
        census = base["stages"]["lone"]["census"]["ms_per_launch"]
        for r in rows:
            if r["D"] == D:
                r["bound_ms"] = round(base["batch_ms_per_frame_median"] + 2 * census, 4)
                r["within_bound"] = bool(r["batch_ms_per_frame_median"] <= r["bound_ms"])
    eng.set_census_window(9, 7, 1)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps({k: v for k, v in r.items() if k != "stages"}))
            print("   stages", json.dumps(r["stages"]))


if __name__ == "__main__":
    main()
