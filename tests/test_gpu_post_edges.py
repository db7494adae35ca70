"""GPU: the post filters at the edges that only assembled components and strided outputs reach,
launched the way a match launches them (Engine.post -> sgm_debug_post): the median alone, the speckle
filter alone and the fused median3+speckle tile kernel, into an image whose row stride is not W.

Every case (tests/post_cases.py) first asserts on tests/post_reference.py what it promises about its
own input (a component of exactly N pixels, two half-planes that join or do not, a component of
max_size and one of max_size + 1 pixels after the median, each on >= 2 tiles); then the GPU result is
compared bit for bit with post_reference for every max_size, median in {0, 1} and out_pad in {0, 5},
and once per case with the oracle. The speckle tiles are 64 x 16."""
import numpy as np
import pytest

import post_cases as pc
import post_reference as ref
from test_post_reference import check_precondition

pytestmark = pytest.mark.gpu

GROUPS = pc.speckle_groups()


def _run_case(engine, oracle, case):
    nv, md = case["new_val"], case["max_diff"]
    for median in (0, 1):
        d = check_precondition(case, median)              # the image the speckle filter sees
        _, sizes = ref.components(d, nv, md)
        for ms in case["max_sizes"]:
            if ms > 0:
                want = np.where((sizes > 0) & (sizes <= ms), np.int16(nv), d)
            else:
                want = d                                  # no speckle filter: the median alone, or nothing
            for pad in (0, 5):
                got, canary = engine.post(case["d"], median, nv, ms, md, out_pad=pad)
                where = f"{case['name']} median {median} max_size {ms} pad {pad}"
                assert np.array_equal(got, want), f"{where}: {int((got != want).sum())} pixels differ"
                assert canary.shape == (d.shape[0], pad) and (canary == engine.POST_CANARY).all(), where
        ms = case["fat"] if case["fat"] is not None else case["max_sizes"][-1]
        o = oracle.median3(case["d"]) if median else case["d"]
        if ms > 0:
            o = oracle.filter_speckles(o, nv, ms, md)
        assert np.array_equal(engine.post(case["d"], median, nv, ms, md, out_pad=5)[0], o), case["name"]


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_post_edges(engine, oracle, group):
    for case in GROUPS[group]:
        _run_case(engine, oracle, case)


def test_post_agrees_with_the_single_stage_entries(engine):
    """Engine.post with no pad and no median is the speckle entry; with max_size 0, the median entry."""
    case = pc.ragged_cases()[2]
    d = case["d"]
    assert np.array_equal(engine.post(d, 0, pc.BG, 40, 16)[0], engine.filter_speckles(d, pc.BG, 40, 16))
    assert np.array_equal(engine.post(d, 1, pc.BG, 0, 16)[0], engine.median3(d))
    assert np.array_equal(engine.post(d, 0, pc.BG, 0, 16, out_pad=3)[0], d)
