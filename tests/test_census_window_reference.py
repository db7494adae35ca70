"""The census-window reference (tests/census_window_reference.py) against the CPU oracle, no GPU:
with the window (9, 7, 1) its codes, every direction's path volume and the composed match equal
the oracle's bit for bit; a dense window's code is the 9x7 code AND-ed with the window's mask; a
(9, 7, 2) code is checked by hand."""
import numpy as np
import pytest

import census_window_reference as cwr

H, W, D = 40, 96, 32


@pytest.fixture(scope="module")
def pair(synth):
    left, right, _ = synth.stereo_pair(H, W, 0, D, seed=77)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


def test_default_window_codes_are_the_oracle_census(oracle, pair):
    for img in pair:
        assert np.array_equal(cwr.census(img), oracle.census(img))
    rng = np.random.default_rng(5)
    small = rng.integers(0, 256, (5, 4), dtype=np.uint8)         # smaller than the window: every tap clamps
    assert np.array_equal(cwr.census(small), oracle.census(small))


@pytest.mark.parametrize("minD", [0, 3, -2])
def test_default_window_paths_and_match_are_the_oracle(oracle, pair, minD):
    left, right = pair
    p = oracle.make_params(oracle.MODE_CENSUS8, num_disparities=D, min_disparity=minD)
    for d in range(8):
        assert np.array_equal(cwr.census_path(oracle, p, left, right, d), oracle.census_path(p, left, right, d)), d
    assert np.array_equal(cwr.match(oracle, p, left, right), oracle.match(p, left, right))
    q = oracle.make_params(oracle.MODE_CENSUS8, num_disparities=D, min_disparity=minD, median=1,
                           speckle_window_size=20, speckle_range=2, p2=250)
    assert np.array_equal(cwr.match(oracle, q, left, right), oracle.match(q, left, right))


def test_mask_and_bit_order():
    assert cwr.mask(9, 7) == (1 << 62) - 1
    assert cwr.bit_index(-3, -4) == 0 and cwr.bit_index(0, -1) == 30 and cwr.bit_index(0, 1) == 31
    assert cwr.bit_index(3, 4) == 61
    assert bin(cwr.mask(3, 3)).count("1") == 8 and bin(cwr.mask(7, 5)).count("1") == 34
    assert len(cwr.WINDOWS) == 24 and cwr.DEFAULT in cwr.WINDOWS


@pytest.mark.parametrize("tx,ty", [(tx, ty) for tx in (3, 5, 7, 9) for ty in (3, 5, 7)])
def test_dense_window_is_the_masked_default_code(oracle, pair, tx, ty):
    full = oracle.census(pair[0])
    assert np.array_equal(cwr.census(pair[0], (tx, ty, 1)), full & np.uint64(cwr.mask(tx, ty)))


def test_step_two_code_by_hand():
    """(9, 7, 2) at an interior pixel of an image that is dark exactly at four chosen taps."""
    img = np.full((20, 30), 100, np.uint8)
    y, x = 9, 14
    dark = [(-3, -4), (0, 1), (2, -3), (3, 4)]                 # (j, i): pixels (y + 2j, x + 2i)
    for j, i in dark:
        img[y + 2 * j, x + 2 * i] = 10
    img[y + 1, x + 1] = 10                                      # an odd offset: no tap of a step-2 window
    code = int(cwr.census(img, (9, 7, 2))[y, x])
    want = (1 << 0) | (1 << 31) | (1 << (5 * 9 + 1 - 1)) | (1 << 61)
    assert code == want
    # the dense window sees the odd-offset pixel, offset (1, 1) = bit 4*9 + 5 - 1, and of the four
    # only the pixel at (y, x + 2), offset (0, 2) = bit 3*9 + 6 - 1
    assert int(cwr.census(img, (9, 7, 1))[y, x]) == (1 << 40) | (1 << 32)
    # (7, 7, 2) loses the taps of the outer columns (i = -4 and 4)
    assert int(cwr.census(img, (7, 7, 2))[y, x]) == want & ~((1 << 0) | (1 << 61))


def test_other_windows_give_other_images(oracle, pair):
    """A window that was silently ignored cannot pass the GPU tests: the references differ."""
    left, right = pair
    p = oracle.make_params(oracle.MODE_CENSUS8, num_disparities=D)
    base = oracle.match(p, left, right)
    for win in [(3, 3, 1), (7, 7, 1), (7, 7, 2), (9, 7, 2)]:
        assert (cwr.match(oracle, p, left, right, win) != base).mean() > 0.005, win
