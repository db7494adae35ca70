"""Regenerates the MODE_OCV_BM fixtures from the numpy reference (tests/bm_reference.py):

    python tests/golden/make_golden_bm.py

writes bm/bm_node_defaults_64x128.npz and bm/bm_negmin_41x90.npz (inputs, parameters, pre-filtered
left image, disparity; in their own directory because the SGM fixture tests replay every .npz of
tests/golden/ through the SGM oracle) and prints the constants of plugin/plugin_bm_test.cpp (hash, valid count and a
sample of the forward and backward match of the driver's generated 48x96 frame).
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import bm_reference as br  # noqa: E402


def _synth():
    spec = importlib.util.spec_from_file_location("sgm_synth", os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def driver_frame():
    """The 48x96 pair plugin_bm_test.cpp generates (32-bit LCG noise, 2-tap blur, shift 7)."""
    W, H, shift = 96, 48, 7
    NW = W + 8
    s = 12345
    N = np.empty(H * NW, np.int64)
    for i in range(H * NW):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        N[i] = (s >> 24) & 255
    N = N.reshape(H, NW)
    B = (N[:, :-1] + N[:, 1:] + 1) >> 1
    return B[:, :W].astype(np.uint8), B[:, shift:shift + W].astype(np.uint8)


def fnv1a(disp):
    h = 1469598103934665603
    for b in np.ascontiguousarray(disp, "<i2").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def main():
    synth = _synth()
    os.makedirs(os.path.join(HERE, "bm"), exist_ok=True)
    for name, (H, W, seed), bm in (("bm_node_defaults_64x128", (64, 128, 1), br.BM(9, 64, 15, 31, 10, 15)),
                                   ("bm_negmin_41x90", (41, 90, 2), br.BM(-8, 16, 5, 7, 10, 2))):
        left, right, _ = synth.stereo_pair(H, W, bm.m, bm.D, seed=seed)
        disp = br.compute(bm, left, right)
        np.savez_compressed(os.path.join(HERE, "bm", name + ".npz"), left=left, right=right, bm=np.array(bm, np.int32),
                            prefiltered_left=br.prefilter(left, bm.c), disp=disp)
        print(name, "valid share", br.valid_share(bm, disp))
    left, right = driver_frame()
    fwd = br.compute(br.BM(0, 64, 9, 31, 10, 15), left, right)              # StereoBM::create(64, 9)
    bwd = br.compute(br.BM(-(0 + 64) + 1, 64, 9, 31, 0, 0), right, left)    # its right matcher
    print("kForwardHash  = 0x%016x, valid %d, sample(24, 80) %d" % (fnv1a(fwd), (fwd != -16).sum(), fwd[24, 80]))
    print("kBackwardHash = 0x%016x, valid %d, sample(24, 10) %d" % (fnv1a(bwd), (bwd != -64 * 16).sum(), bwd[24, 10]))


if __name__ == "__main__":
    main()
