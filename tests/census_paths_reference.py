"""Reference of the census mode with a selectable path set, composed from the oracle's stages.

S = sum over the set's directions of the oracle's u8 path volumes (u16), then the oracle's WTA
(uniqueness, sub-pixel, disp2 / LR), 3x3 median and speckle filter: the way sgmref_match
composes its census pipeline, with the direction set a parameter. With dirs = range(8) it equals
oracle.match bit for bit (tests/test_census_paths_host.py).
"""
import numpy as np

DIRS4 = (0, 1, 6, 7)       # down, up, left-to-right, right-to-left: mask 0xC3
MASK4 = 0xC3


def match_paths(oracle, p, left, right, dirs=DIRS4):
    """Disparity (int16, x16) of the census pipeline of parameters p (an oracle SgmParams)
    aggregating over the directions `dirs` only."""
    left = np.ascontiguousarray(left, np.uint8)
    right = np.ascontiguousarray(right, np.uint8)
    h, w = left.shape
    e = oracle.effective(p, w, h)
    if e["width1"] <= 0:
        return np.full((h, w), e["invalid"], np.int16)
    S = np.zeros((h, e["width1"], e["D"]), np.uint16)
    for d in dirs:
        S += oracle.census_path(p, left, right, d)
    disp = oracle.wta(p, S, w)
    if e["median"]:
        disp = oracle.median3(disp)
    if p.speckle_window_size > 0:
        disp = oracle.filter_speckles(disp, e["invalid"], p.speckle_window_size, 16 * p.speckle_range)
    return disp


def fnv1a16(disp):
    """FNV-1a over the little-endian bytes of an int16 image (the plugin drivers' checksum)."""
    h = 1469598103934665603
    for b in np.ascontiguousarray(disp, "<i2").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def driver_frame(w=144, h=56):
    """The frame of plugin/plugin_paths_test.cpp: LCG noise, smoothed, right = left shifted by
    5 + y // 16 columns."""
    nw = w + 16
    n = np.empty(h * nw, np.int64)
    s = 2024
    for i in range(h * nw):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        n[i] = (s >> 24) & 255
    n = n.reshape(h, nw)
    left = np.empty((h, w), np.uint8)
    right = np.empty((h, w), np.uint8)
    for y in range(h):
        sh = 5 + y // 16
        left[y] = (n[y, :w] + n[y, 1:w + 1] + 1) >> 1
        right[y] = (n[y, sh:sh + w] + n[y, sh + 1:sh + w + 1] + 1) >> 1
    return left, right
