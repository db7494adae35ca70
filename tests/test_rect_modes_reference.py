"""CPU: the references of tests/test_gpu_rect_modes.py are worth comparing against. These are
conditions on the composed references (tests/rect_modes_reference.py), not measurements of the
library: a GPU test that passes on an empty map, on a rectification that changes nothing or on a
colour order that cannot be told apart would show nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_reference as cr  # noqa: E402
import rect_modes_reference as rm  # noqa: E402

CH_SETS = [(1, cr.GRAY_Y14), (3, cr.GRAY_Y14), (3, cr.GRAY_Y15)]


@pytest.mark.parametrize("ch,s", CH_SETS, ids=["mono", "Y14", "Y15"])
@pytest.mark.parametrize("mode", rm.MODES)
@pytest.mark.parametrize("name", list(rm.CASES))
def test_references_are_real_disparity_maps(oracle, synth, name, mode, ch, s):
    ref = rm.reference(oracle, synth, name, mode, ch, s, 0)
    share = rm.valid_share(mode, rm.case_kw(name, mode), ref)
    print(name, mode, ch, s, "valid share", share)
    assert share >= 0.5


@pytest.mark.parametrize("mode", rm.MODES)
@pytest.mark.parametrize("name", list(rm.CASES))
def test_rectification_changes_the_result(oracle, synth, name, mode):
    """The match of the unrectified frames (cropped to the rectified size) is another image."""
    rh, rw, h, w = rm.CASES[name][:4]
    _, frames, _ = rm.setup(oracle, synth, name, 1)
    ref = rm.reference(oracle, synth, name, mode, 1, 0, 0)
    plain = rm.match_ref(oracle, mode, rm.case_kw(name, mode), frames[0][0][:h, :w], frames[0][1][:h, :w])
    share = float((plain != ref).mean())
    print(name, mode, "differs on", share)
    assert share > 0.5


@pytest.mark.parametrize("s", [cr.GRAY_Y14, cr.GRAY_Y15], ids=["Y14", "Y15"])
@pytest.mark.parametrize("name", list(rm.CASES))
def test_colour_order_of_operations_is_visible(oracle, synth, name, s):
    """gray(remap3(raw)), the node's order, is not remap(gray(raw)) on these frames."""
    maps, frames, rect = rm.setup(oracle, synth, name, 3)
    for i in range(rm.NMAX):
        for side in (0, 1):
            other = oracle.remap_cubic(cr.gray(frames[i][side], s), *maps[side])
            assert not np.array_equal(cr.gray(rect[i][side], s), other), (name, i, side)


def test_speckle_cases_filter_something(oracle, synth):
    """The two cases run with the node's speckle filter differ from their unfiltered references."""
    for name, mode in (("203x70", "sgbm5"), ("203x70", "bm")):
        a = rm.reference(oracle, synth, name, mode, 1, 0, 0, speckle=True)
        b = rm.reference(oracle, synth, name, mode, 1, 0, 0)
        assert not np.array_equal(a, b), (name, mode)
