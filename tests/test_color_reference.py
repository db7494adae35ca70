"""CPU checks of the colour stage: the two COLOR_BGR2GRAY coefficient sets of tests/color_reference.py
and of the package's host bgr2gray(), and the C-ABI surface of the built library (new symbols, ABI
version unchanged). No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_reference as cr  # noqa: E402

# The first triple (c0, c1, 0), in raster order over (c0, c1), on which the two sets differ, with both
# results, worked out by hand:
#   Y14 (3*1868 + 157*9617 + 2^13) >> 14 = 1523665 >> 14 = 92   (1523665 / 16384 = 92.998)
#   Y15 (3*3735 + 157*19235 + 2^14) >> 15 = 3047484 >> 15 = 93  (3047484 / 32768 = 93.002)
PINNED_DIFF = (3, 157, 0, 92, 93)


def _one(c0, c1, c2, s):
    return int(cr.gray(np.array([[[c0, c1, c2]]], np.uint8), s)[0, 0])


def test_coefficients_sum_to_one():
    for s, one in ((cr.GRAY_Y14, 1 << 14), (cr.GRAY_Y15, 1 << 15)):
        k, bits = cr.COEFFS[s]
        assert sum(k) == one == 1 << bits


@pytest.mark.parametrize("s", [cr.GRAY_Y14, cr.GRAY_Y15])
def test_grey_pixels_stay(s):
    v = np.arange(256, dtype=np.uint8)
    img = np.stack([v, v, v], axis=-1)[None]
    assert np.array_equal(cr.gray(img, s)[0], v)


def test_sets_differ_somewhere():
    """Exhaustive over one channel pair (c2 = 0): the sets are different functions, and the pinned
    triple is one of the differences (so the two cannot be confused)."""
    c0, c1 = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    img = np.stack([c0, c1, np.zeros_like(c0)], axis=-1).astype(np.uint8)
    g14, g15 = cr.gray(img, cr.GRAY_Y14), cr.gray(img, cr.GRAY_Y15)
    diff = np.argwhere(g14 != g15)
    assert 0 < len(diff) < 256 * 256 // 50          # they differ, and only by rounding
    assert (np.abs(g14.astype(int) - g15.astype(int)) <= 1).all()
    a, b = (int(t) for t in diff[0])
    assert (a, b, 0) == PINNED_DIFF[:3], f"first differing (c0, c1, 0) is {(a, b)}"
    assert (_one(*PINNED_DIFF[:3], cr.GRAY_Y14), _one(*PINNED_DIFF[:3], cr.GRAY_Y15)) == PINNED_DIFF[3:]


def test_channel_order_matters():
    """Bytes are weighted in memory order: swapping c0 and c2 (an RGB8 frame) changes the result."""
    assert _one(255, 0, 0, cr.GRAY_Y14) == 29 and _one(0, 0, 255, cr.GRAY_Y14) == 76
    assert _one(0, 255, 0, cr.GRAY_Y14) == 150
    assert _one(255, 0, 0, cr.GRAY_Y15) == 29 and _one(0, 0, 255, cr.GRAY_Y15) == 76


def test_synthetic_frames_discriminate(synth):
    left, right = cr.color_pair(synth, 40, 130, 0, 32, seed=5)
    assert left.shape == (40, 130, 3) and left.dtype == np.uint8
    cr.check_discriminating(left)
    cr.check_discriminating(right)


def test_package_bgr2gray(pkg):
    """bgr2gray() with no argument is the 14-bit formula it always was; the argument picks a set."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    b, g, r = (img[..., i].astype(np.int32) for i in range(3))
    old = ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)
    assert np.array_equal(pkg.bgr2gray(img), old)
    assert np.array_equal(pkg.bgr2gray(img, pkg.GRAY_Y14), cr.gray(img, cr.GRAY_Y14))
    assert np.array_equal(pkg.bgr2gray(img, pkg.GRAY_Y15), cr.gray(img, cr.GRAY_Y15))
    mono = img[..., 0]
    out = pkg.bgr2gray(mono)
    assert np.array_equal(out, mono) and out is not mono
    assert (pkg.GRAY_Y14, pkg.GRAY_Y15) == (cr.GRAY_Y14, cr.GRAY_Y15)


def test_library_exports_colour_symbols(pkg):
    """New functions only: callers check for the symbols, the ABI version did not move."""
    if not os.path.exists(pkg.LIB_PATH):
        pytest.fail("libsgm_hip.so not built")
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("sgm_bgr2gray", "sgm_remap_cubic_c3", "sgm_set_raw_format", "sgm_get_raw_format"):
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS
    lib.sgm_abi_version.restype = ctypes.c_int
    assert lib.sgm_abi_version() == 5 == pkg.ABI_VERSION
    assert ctypes.sizeof(pkg.SgmParams) == 15 * 4
    header = open(os.path.join(os.path.dirname(pkg.HERE), "include", "sgm_hip.h")).read()
    assert "#define SGM_ABI_VERSION 5" in header
    assert "#define SGM_GRAY_Y14 0" in header and "#define SGM_GRAY_Y15 1" in header
