"""References of the OCV / BM modes on raw frames (sgm_set_rectification ahead of those matchers),
composed from what exists: oracle.rectify_map, oracle.remap_cubic / color_reference.remap3,
color_reference.gray (after the remap: the node's order), then oracle.match or bm_reference.compute.
Test infrastructure only; every reference is computed once, shared and read-only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm_reference as br  # noqa: E402
import color_reference as cr  # noqa: E402
from test_rectify_oracle import calib  # noqa: E402

# name: (raw h, raw w, h, w, minD, D, seed). 130x41: odd H (BM's last-row rule), row tail 2;
# 203x70: row tail 3; 67x33: row tail 3, minD > 0.
CASES = {"130x41": (50, 140, 41, 130, 0, 32, 5), "203x70": (80, 210, 70, 203, -8, 64, 6),
         "67x33": (40, 75, 33, 67, 3, 16, 7)}
MODES = ["sgbm5", "hh8", "bm"]
MODE_ID = {"sgbm5": 0, "hh8": 1, "census": 2, "bm": 3}       # include/sgm_hip.h SGM_MODE_*
NMAX = 5
BM_TEXTURE = 10
_cache = {}


def once(key, fn):
    if key not in _cache:
        v = fn()
        for a in (v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def mode_kw(mode, m, D, block=None, speckle=False):
    """sgm_params fields of a mode's test settings. OCV: block 3 or 5, P1 8 b^2, P2 32 b^2,
    uniqueness 10, disp12 1, cap 31. BM: window 9, (texture 10,) uniqueness 15, cap 31.
    speckle: the node's filter (100, 4)."""
    spk = dict(speckle_window_size=100 if speckle else 0, speckle_range=4 if speckle else 0)
    if mode == "bm":
        return dict(min_disparity=m, num_disparities=D, block_size=block or 9, prefilter_cap=31, uniqueness_ratio=15,
                    disp12_max_diff=-1, **spk)
    if mode == "census":
        return dict(min_disparity=m, num_disparities=D)
    b = block or 5
    return dict(min_disparity=m, num_disparities=D, block_size=b, p1=8 * b * b, p2=32 * b * b, uniqueness_ratio=10,
                disp12_max_diff=1, prefilter_cap=31, **spk)


def case_kw(name, mode, speckle=False):
    m, D = CASES[name][4:6]
    return mode_kw(mode, m, D, block=None if mode == "bm" else (3 if name == "67x33" else 5), speckle=speckle)


def bm_of(kw, texture=BM_TEXTURE):
    return br.BM(kw["min_disparity"], kw["num_disparities"], kw["block_size"], kw["prefilter_cap"], texture,
                 kw["uniqueness_ratio"])


def match_ref(oracle, mode, kw, gl, gr, texture=BM_TEXTURE):
    """Disparity of a rectified grey pair in `mode` under the sgm_params fields kw."""
    gl, gr = np.ascontiguousarray(gl), np.ascontiguousarray(gr)
    if mode != "bm":
        return oracle.match(oracle.make_params(MODE_ID[mode], **kw), gl, gr)
    bm = bm_of(kw, texture)
    ref = br.compute(bm, gl, gr)
    if kw.get("speckle_window_size", 0) > 0:
        ref = oracle.filter_speckles(ref, br.filtered(bm), kw["speckle_window_size"], kw["speckle_range"])
    return ref


def rectified(oracle, raw, mx, my):
    """remap of a mono (H x W) or colour (H x W x 3) frame."""
    return cr.remap3(oracle, raw, mx, my) if raw.ndim == 3 else oracle.remap_cubic(np.ascontiguousarray(raw), mx, my)


def grey_of(img, s):
    return cr.gray(img, s) if img.ndim == 3 else img


def raw_frames(synth, rh, rw, m, D, seed, ch):
    if ch == 3:
        f = cr.color_pair(synth, rh, rw, m, D, seed)
        cr.check_discriminating(f[0])
        cr.check_discriminating(f[1])
        return f
    return synth.stereo_pair(rh, rw, m, D, seed=seed)[:2]


def setup(oracle, synth, name, ch):
    """(maps [(mx, my) left, right], raw frames [(l, r)] * NMAX, rectified [(l, r)] * NMAX) of a fixed case."""
    def make():
        rh, rw, h, w, m, D, seed = CASES[name]
        maps = [oracle.rectify_map(*calib(seed=11, w=rw, h=rh), w, h), oracle.rectify_map(*calib(seed=12, w=rw, h=rh), w, h)]
        frames = [raw_frames(synth, rh, rw, m, D, seed + 10 * i, ch) for i in range(NMAX)]
        rect = [(rectified(oracle, f[0], *maps[0]), rectified(oracle, f[1], *maps[1])) for f in frames]
        return maps, frames, rect
    return once(("setup", name, ch), make)


def reference(oracle, synth, name, mode, ch, s, i, speckle=False):
    """Disparity of frame i of a fixed case: `mode` on gray(remap(raw))."""
    def make():
        rect = setup(oracle, synth, name, ch)[2]
        return match_ref(oracle, mode, case_kw(name, mode, speckle), grey_of(rect[i][0], s), grey_of(rect[i][1], s))
    return once(("ref", name, mode, ch, s if ch == 3 else 0, i, speckle), make)


def valid_share(mode, kw, disp):
    if mode == "bm":
        return br.valid_share(bm_of(kw), disp)
    return float((disp != (kw["min_disparity"] - 1) * 16).mean())
