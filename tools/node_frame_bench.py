"""Host wall time of the node's frame, in one process and one run: per configuration the rows

  (a) node_frame       Engine.node_frame (sgm_node_frame) with pageable outputs
  (b) node_frame_reg   the same with the rectified images and the DisparityImage buffer registered
                       (sgm_host_register)
  (c) parent_image_cb  image_cb of a build of the parent commit (--parent-pkg: that checkout's
                       package directory, built), the only frame entry that existed before
  (d) image_cb         image_cb of this build (what (c) differs from (a) by, apart from the build)

are timed with a host clock around blocks of synchronous calls (every call ends in a device
synchronise), about --block-ms of work per block, the rows alternated over rounds (each round
starts one row further on), after two warm-up calls of each. Configurations (mono and colour
each): 640x480 BM and SGBM5 at the node defaults; 2448x2048 minD 147 D 480 window 21, BM and
SGBM5; 1920x1080 census D = 128 and D = 256. With --parent-pkg the C3 host call (sgm_match_f32,
1920x1080 census D = 256) of both builds is timed the same way as a control for the default path.

The condition written with every record: at no configuration is (a) or (b) slower than (c) by
more than the spread (max - min) between (c)'s own rounds.

--second-handle adds, per configuration and to the control, this build's image_cb / sgm_match_f32 on
a handle opened after the parent's: what two handles of one build differ by (each handle has its
own workspace, tens of GB at the 2448x2048 frame).

    python tools/node_frame_bench.py [--rounds 5] [--parent-pkg DIR] [--only SUBSTR] [--second-handle]
                                     [--out profiles/node_frame.jsonl]
"""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tools.color_bench import calibration, colourize  # noqa: E402

NODE = dict(min_disparity=9, num_disparities=64, block_size=15)
BIG = dict(min_disparity=147, num_disparities=480, block_size=21)
CASES = [("640x480 node defaults", 480, 640, "bm", NODE), ("640x480 node defaults", 480, 640, "sgbm5", NODE),
         ("2448x2048 minD=147 D=480 window 21", 2048, 2448, "bm", BIG),
         ("2448x2048 minD=147 D=480 window 21", 2048, 2448, "sgbm5", BIG),
         ("1920x1080 D=128", 1080, 1920, "census", dict(min_disparity=0, num_disparities=128)),
         ("1920x1080 D=256", 1080, 1920, "census", dict(min_disparity=0, num_disparities=256))]
F, T, ZMIN, ZMAX = 712.5, 0.119, 0.05, 100.0


def load_parent(pkg_dir):
    """The parent commit's package (its own __init__.py and lib/libsgm_hip.so) under another name."""
    spec = importlib.util.spec_from_file_location("sgm_parent_pkg", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["sgm_parent_pkg"] = mod
    spec.loader.exec_module(mod)
    mod.load_library(os.path.join(pkg_dir, "lib", "libsgm_hip.so"))
    return mod


def matcher(pkg, mode, kw):
    m = pkg.MatcherHIPSGM(" ", (0, 0), mode={"bm": pkg.MODE_OCV_BM, "sgbm5": pkg.MODE_OCV_SGBM5,
                                             "census": pkg.MODE_CENSUS8}[mode], census_paths=8)
    cfg = dict(pkg.NODE_DEFAULTS, min_disparity=kw["min_disparity"], disparity_range=kw["num_disparities"])
    if "block_size" in kw:
        cfg["correlation_window_size"] = kw["block_size"]
    pkg.update_matcher(m, cfg)
    if mode == "census":       # the census defaults (no median, no speckle filter): the WTA-written rows
        m.params = pkg.default_params(pkg.MODE_CENSUS8, min_disparity=kw["min_disparity"],
                                      num_disparities=kw["num_disparities"])
    return m


def wall(reps, fn):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternate(run, rounds, block_ms, probe):
    for c in run:
        run[c]()
        run[c]()
    reps = max(1, math.ceil(block_ms / wall(2, run[probe])))
    order = list(run)
    out = {c: [] for c in run}
    for k in range(rounds):
        for c in order[k % len(order):] + order[:k % len(order)]:
            out[c].append(wall(reps, run[c]))
    return reps, {c: {"median_ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                      "rounds_ms": [round(x, 4) for x in v]} for c, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-ms", type=float, default=300.0)
    ap.add_argument("--parent-pkg", default=None, help="package directory of a built checkout of the parent commit")
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    ap.add_argument("--second-handle", action="store_true",
                    help="also time image_cb of this build on a second handle (what two handles of one build differ by)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_frame.jsonl"))
    a = ap.parse_args()
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    parent = load_parent(os.path.abspath(a.parent_pkg)) if a.parent_pkg else None
    lines = []
    for cname, H, W, mode, kw in CASES:
        if a.only and a.only not in f"{mode} {cname}":
            continue
        l, r, _ = synth.stereo_pair(H, W, kw["min_disparity"], kw["num_disparities"], seed=1, with_truth=False)
        infos = [calibration(W, H, 1), calibration(W, H, -1)]
        for ch in (1, 3):
            raw = (l, r) if ch == 1 else (colourize(l), colourize(r))
            m = matcher(pkg, mode, kw)
            eng = m._engine_for()
            pm = matcher(parent, mode, kw) if parent else None
            lo = np.float32(T * F / ZMAX)
            hi = np.float32(T * F / ZMIN)
            page = [np.empty(raw[0].shape, np.uint8), np.empty(raw[0].shape, np.uint8), np.empty((H, W), np.float32)]
            reg = [np.empty(raw[0].shape, np.uint8), np.empty(raw[0].shape, np.uint8), np.empty((H, W), np.float32)]
            # image_cb's configuration of the engine, then the rows on that configuration
            first = pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, ZMIN, ZMAX, {})
            for b in reg:
                eng.host_register(b)

            def frame(bufs):
                eng.node_frame(raw[0], raw[1], infos[0], infos[1], lo, hi, rect_left=bufs[0], rect_right=bufs[1],
                               disparity=bufs[2])

            state, pstate = {}, {}
            run = {"node_frame": lambda: frame(page), "node_frame_reg": lambda: frame(reg),
                   "image_cb": lambda: pkg.image_cb(m, raw[0], raw[1], infos[0], infos[1], F, T, ZMIN, ZMAX, state)}
            if pm:
                run["parent_image_cb"] = lambda: parent.image_cb(pm, raw[0], raw[1], infos[0], infos[1], F, T, ZMIN, ZMAX,
                                                                 pstate)
            m2 = matcher(pkg, mode, kw) if a.second_handle else None
            if m2:      # control: this build's image_cb on a handle opened after the parent's
                state2 = {}
                run["image_cb_2nd_handle"] = lambda: pkg.image_cb(m2, raw[0], raw[1], infos[0], infos[1], F, T, ZMIN, ZMAX,
                                                                  state2)
            reps, rows = alternate(run, a.rounds, a.block_ms, "node_frame")
            if m2:
                m2._engine_for().close()
            same = all(np.array_equal(x, y) for x, y in zip(page, reg)) and np.array_equal(page[0], first[0]) and \
                np.array_equal(page[1], first[1]) and np.array_equal(page[2].view(np.uint32), first[2]["image"].view(np.uint32))
            rec = {"case": f"{mode} {cname} ch{ch}", "reps_per_block": reps, "outputs_equal_image_cb": bool(same), **rows}
            base = rows.get("parent_image_cb", rows["image_cb"])
            spread = base["max"] - base["min"]
            rec["baseline"] = "parent_image_cb" if pm else "image_cb"
            rec["within_baseline_spread"] = {c: rows[c]["median_ms"] <= base["median_ms"] + spread
                                             for c in ("node_frame", "node_frame_reg")}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            for b in reg:
                eng.host_unregister(b)
            eng.close()
            if pm:
                pm._engine_for().close()
    if parent and (not a.only or a.only == "control" or a.second_handle):
        # control: the C3 host call on both builds, same alternation
        l, r, _ = synth.stereo_pair(1080, 1920, 0, 256, seed=1, with_truth=False)
        engs = {"match_f32": pkg.Engine(0, pkg.default_params(pkg.MODE_CENSUS8, num_disparities=256)),
                "parent_match_f32": parent.Engine(0, parent.default_params(parent.MODE_CENSUS8, num_disparities=256))}
        if a.second_handle:    # what two handles of one build differ by (this one opened after the parent's)
            engs["match_f32_2nd_handle"] = pkg.Engine(0, pkg.default_params(pkg.MODE_CENSUS8, num_disparities=256))
        outs = {c: np.empty((1080, 1920), np.float32) for c in engs}
        run = {c: (lambda c=c: engs[c].match_f32(l, r, outs[c])) for c in engs}
        reps, rows = alternate(run, a.rounds, a.block_ms, "match_f32")
        p = rows["parent_match_f32"]
        rec = {"case": "control: C3 sgm_match_f32 1920x1080 D=256", "reps_per_block": reps, **rows,
               "outputs_equal": bool(np.array_equal(outs["match_f32"].view(np.uint32), outs["parent_match_f32"].view(np.uint32))),
               "within_parent_spread": rows["match_f32"]["median_ms"] <= p["median_ms"] + p["max"] - p["min"]}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        for e in engs.values():
            e.close()
    if a.out and lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
