"""numpy reference of the colour stage: cv::cvtColor(COLOR_BGR2GRAY) for 8UC3 in its two
coefficient sets, the per-channel composition of the oracle's one-channel remap, and the synthetic
colour stereo frames of the colour tests. Written from the formulas in include/sgm_hip.h, sharing
nothing with the package. Test infrastructure only; like every OpenCV restatement of this project
the formulas are unverified against a real OpenCV.

    gray(img, GRAY_Y14)   (c0*1868 + c1*9617 + c2*4899 + 2^13) >> 14     OpenCV 3.2
    gray(img, GRAY_Y15)   (c0*3735 + c1*19235 + c2*9798 + 2^14) >> 15    OpenCV 4.x
over the bytes of a pixel in memory order c0, c1, c2 (no channel-order flag: an RGB8 frame gets
the R and B weights swapped, as in the node).
"""
import numpy as np

GRAY_Y14, GRAY_Y15 = 0, 1
COEFFS = {GRAY_Y14: ((1868, 9617, 4899), 14), GRAY_Y15: ((3735, 19235, 9798), 15)}


def gray(img, gray_set):
    """H x W x 3 u8 -> H x W u8."""
    (k0, k1, k2), bits = COEFFS[gray_set]
    c = np.asarray(img).astype(np.int64)
    assert c.ndim == 3 and c.shape[2] == 3
    return ((c[..., 0] * k0 + c[..., 1] * k1 + c[..., 2] * k2 + (1 << (bits - 1))) >> bits).astype(np.uint8)


def luts():
    """Three different monotone (non-decreasing) u8 look-up tables, one per channel."""
    v = np.arange(256, dtype=np.float64)
    c0 = np.clip(np.floor(255.0 * (v / 255.0) ** 1.6 + 0.5), 0, 255)
    c1 = np.clip(np.floor(0.7 * v + 70.0 + 0.5), 0, 255)   # v = 119..121 (common values): Y14 != Y15
    c2 = np.clip(np.floor(255.0 * (v / 255.0) ** 0.6 + 0.5), 0, 255)
    t = np.stack([c0, c1, c2]).astype(np.uint8)
    assert (np.diff(t.astype(int), axis=1) >= 0).all()
    return t


def colorize(mono):
    """H x W u8 -> H x W x 3 u8 through the three tables (a stereo-consistent pair stays one)."""
    t = luts()
    return np.ascontiguousarray(np.stack([t[c][mono] for c in range(3)], axis=-1))


def color_pair(synth, h, w, min_disp, num_disp, seed):
    """(left, right) H x W x 3 u8 from synth.stereo_pair."""
    left, right, _ = synth.stereo_pair(h, w, min_disp, num_disp, seed=seed)
    return colorize(left), colorize(right)


def check_discriminating(img):
    """The frame tells a wrong channel order, plane or grey set apart: the grey image of either set
    equals none of the three planes, the two sets differ on it, and so do the two channel orders."""
    g14, g15 = gray(img, GRAY_Y14), gray(img, GRAY_Y15)
    for g in (g14, g15):
        for c in range(3):
            assert not np.array_equal(g, img[..., c])
    assert not np.array_equal(g14, g15)
    assert not np.array_equal(g14, gray(img[..., ::-1], GRAY_Y14))


def remap3(oracle, src, map_x, map_y):
    """cv::remap(INTER_CUBIC, BORDER_CONSTANT 0) of an 8UC3 image: OpenCV's remapBicubic treats the
    channels independently with the same weights, so it is the oracle's one-channel remap of each
    plane."""
    return np.ascontiguousarray(np.stack(
        [oracle.remap_cubic(np.ascontiguousarray(src[..., c]), map_x, map_y) for c in range(3)], axis=-1))
