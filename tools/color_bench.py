"""GPU timings of colour frames through the census batch, in one process and one run:
device-resident 1920x1080 frames, HIP events around blocks of 64-frame batches, three
configurations alternated and their medians reported (as tools/census_paths_bench.py does):

  (a) rect_mono    rectified 8UC1 frames, sgm_match_device_batch
  (b) raw_mono     raw 8UC1 frames, rectification fused into the census, rectified 8UC1 outputs
  (c) raw_colour   raw 8UC3 frames (sgm_set_raw_format(3, Y14)), fused rectification + COLOR_BGR2GRAY
                   inside the census tiles, rectified 8UC3 outputs

at D = 256 (BASELINE C3: sub-pixel + LR) and D = 128 (C2), then a lone sgm_remap_cubic_c3 and a
lone sgm_bgr2gray at 1080p against the device's copy rate measured in the same run.

    python tools/color_bench.py [--rounds 5] [--frames 64] [--out profiles/color_rect.jsonl]
Byte model of (c) per image and pixel: 3 B of raw colour + 8 B of map read (the 4 x 4 taps come
from L1 / L2), 3 B of rectified colour + 8 B of census code written.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

CONFIGS = ("rect_mono", "raw_mono", "raw_colour")


def calibration(w, h, sign):
    """A plausible camera of a stereo rig: mild barrel distortion, a small rotation."""
    f = 0.9 * w
    K = np.array([[f, 0, w / 2 + 3.5 * sign], [0, f * 1.01, h / 2 - 2.25], [0, 0, 1]], np.float64)
    D = np.array([-0.11, 0.03, 0.0007 * sign, -0.0004, 0.002], np.float64)
    a, b = 0.004 * sign, -0.003
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    P = np.array([[f * 1.04, 0, w / 2, 0], [0, f * 1.04, h / 2, 0], [0, 0, 1, 0]], np.float64)
    return K, D, Rx @ Ry, P


def colourize(mono):
    """8UC3 from a mono frame through three different monotone per-channel tables."""
    v = np.arange(256, dtype=np.float64)
    t = np.stack([255.0 * (v / 255.0) ** 1.6, 0.7 * v + 70.0, 255.0 * (v / 255.0) ** 0.6])
    t = np.clip(np.floor(t + 0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([t[c][mono] for c in range(3)], axis=-1))


def timed(torch, st, reps, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternated blocks per configuration")
    ap.add_argument("--frames", type=int, default=64, help="frames of a batch")
    ap.add_argument("--batch-reps", type=int, default=2, help="batches per timed block")
    ap.add_argument("--kernel-reps", type=int, default=50, help="launches per timed block of the lone kernels")
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_rect.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = ge.load_package()
    synth = ge._load_file("sgm_synth", os.path.join(ge.PKG_DIR, "synth.py"))
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    H, W, n = 1080, 1920, a.frames
    eng = {c: pkg.Engine(0) for c in CONFIGS}
    st = torch.cuda.Stream()
    maps = []
    for sign in (1, -1):
        mx = torch.empty((H, W), dtype=torch.float32, device="cuda")
        my = torch.empty((H, W), dtype=torch.float32, device="cuda")
        eng["raw_mono"].rectify_map(*calibration(W, H, sign), W, H, mx.data_ptr(), my.data_ptr(), W)
        maps.append((mx, my))
    eng["raw_mono"].synchronize()
    for c in ("raw_mono", "raw_colour"):
        eng[c].set_rectification((maps[0][0].data_ptr(), maps[0][1].data_ptr()),
                                 (maps[1][0].data_ptr(), maps[1][1].data_ptr()), W, W, H)
    eng["raw_colour"].set_raw_format(3, pkg.GRAY_Y14)
    out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    rect1 = torch.empty((2, n, H, W), dtype=torch.uint8, device="cuda")
    rect3 = torch.empty((2, n, H, W, 3), dtype=torch.uint8, device="cuda")
    ptr_o = [out[f].data_ptr() for f in range(n)]
    lines = []
    for gname, D, flags in [("C3 1920x1080 D=256", 256, dict(subpixel=1, lr_check=1)),
                            ("C2 1920x1080 D=128", 128, dict(subpixel=0, lr_check=0))]:
        params = pkg.default_params(pkg.MODE_CENSUS8, num_disparities=D, min_disparity=0, p1=10, p2=120,
                                    uniqueness_ratio=5, disp12_max_diff=1, median=0, speckle_window_size=0, **flags)
        for e in eng.values():
            e.set_params(params)
        mono, colour = [], []
        for i in range(a.distinct):
            l, r, _ = synth.stereo_pair(H, W, 0, D, seed=i, with_truth=False)
            mono.append((torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()))
            colour.append((torch.from_numpy(colourize(l)).cuda(), torch.from_numpy(colourize(r)).cuda()))
        pm = [[mono[f % len(mono)][s].data_ptr() for f in range(n)] for s in (0, 1)]
        pc = [[colour[f % len(colour)][s].data_ptr() for f in range(n)] for s in (0, 1)]
        pr1 = [[rect1[s, f].data_ptr() for f in range(n)] for s in (0, 1)]
        pr3 = [[rect3[s, f].data_ptr() for f in range(n)] for s in (0, 1)]
        torch.cuda.synchronize()
        run = {
            "rect_mono": lambda: eng["rect_mono"].match_device_batch(pm[0], pm[1], W, H, W, ptr_o, W, st.cuda_stream),
            "raw_mono": lambda: eng["raw_mono"].match_device_batch_rect(pm[0], pm[1], W, H, W, pr1[0], pr1[1], W, ptr_o, W,
                                                                        st.cuda_stream),
            "raw_colour": lambda: eng["raw_colour"].match_device_batch_rect(pc[0], pc[1], W, H, 3 * W, pr3[0], pr3[1],
                                                                            3 * W, ptr_o, W, st.cuda_stream),
        }
        copy_gbps = bench.hbm_copy_gbps(0)
        rounds = {c: [] for c in CONFIGS}
        stages = {}
        with torch.cuda.stream(st):
            for c in CONFIGS:                          # warm-up: workspace, work lists, first launches
                run[c]()
                run[c]()
            st.synchronize()
            for _ in range(a.rounds):                  # alternated blocks: same box, same run
                for c in CONFIGS:
                    rounds[c].append(timed(torch, st, a.batch_reps, run[c]) / n)
            for c in CONFIGS:                          # per-stage HIP events, a separate pass
                eng[c].set_profiling(True)
                run[c]()
                st.synchronize()
                launches = eng[c].stage_launches()
                stages[c] = [{"name": s, "avg_ms": round(t, 4), "alg_bytes": b, "launches": launches.get(s, 0)}
                             for s, t, b in eng[c].stage_times()]
                eng[c].set_profiling(False)
        med = {c: statistics.median(rounds[c]) for c in CONFIGS}
        rec = {"case": f"{gname} batch of {n}", "hbm_copy_GBps": copy_gbps, "reps": a.batch_reps}
        for c in CONFIGS:
            rec[f"{c}_ms_per_frame"] = round(med[c], 4)
            rec[f"{c}_pairs_per_s"] = round(1e3 / med[c], 1)
            rec[f"{c}_rounds_ms"] = [round(v, 4) for v in rounds[c]]
            rec[f"{c}_stages"] = stages[c]
        rec["raw_mono_over_rect_mono"] = round(med["raw_mono"] / med["rect_mono"], 3)
        rec["raw_colour_over_raw_mono"] = round(med["raw_colour"] / med["raw_mono"], 3)
        rec["raw_colour_over_rect_mono"] = round(med["raw_colour"] / med["rect_mono"], 3)
        rec["raw_colour_census_bytes_per_px_per_image"] = {"read": 3 + 8, "written": 3 + 8}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    # the lone kernels at 1080p against the copy rate of the same run
    e = eng["rect_mono"]
    src3 = torch.from_numpy(colourize(synth.stereo_pair(H, W, 0, 64, seed=9, with_truth=False)[0])).cuda()
    dst3 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    dst1 = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kernels = [("sgm_remap_cubic_c3", 3 + 8 + 3,
                lambda: e.remap_cubic(src3.data_ptr(), 3 * W, W, H, maps[0][0].data_ptr(), maps[0][1].data_ptr(), W, W, H,
                                      dst3.data_ptr(), 3 * W, st.cuda_stream, channels=3)),
               ("sgm_bgr2gray", 3 + 1,
                lambda: e.bgr2gray(src3.data_ptr(), 3 * W, W, H, dst1.data_ptr(), W, pkg.GRAY_Y14, st.cuda_stream))]
    copy_gbps = bench.hbm_copy_gbps(0)
    with torch.cuda.stream(st):
        for name, bpp, fn in kernels:
            fn()
            st.synchronize()
            ms = [timed(torch, st, a.kernel_reps, fn) for _ in range(a.rounds)]
            m = statistics.median(ms)
            gbps = bpp * H * W / (m * 1e-3) / 1e9
            rec = {"case": f"{name} 1920x1080", "hbm_copy_GBps": copy_gbps, "ms": round(m, 5),
                   "rounds_ms": [round(v, 5) for v in ms], "alg_bytes_per_px": bpp, "alg_GBps": round(gbps, 1),
                   "over_copy_rate": round(gbps / copy_gbps, 3)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    for e in eng.values():
        e.set_rectification()
        e.close()
    if a.out and lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
