"""The bins of the coding tree against HM-16.15 itself: tests/golden/hm_cu_tree.npz holds what the tree's own
TEncSbac::codeSplitFlag and codePartSize add to a TEncBinCABACCounter at every QP, and TComDataCU::getCtxSplitFlag's truth table over a
CU with real neighbours (tests/golden/make_hm_cu_tree.py recorded them).  pnn_cu_tree_bins_host must equal every record, exactly; the
context rule of include/pnn_hip.h must equal the table, here and -- through one constructed CTU per entry -- in the host twin."""
import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cu_tree_cases as cc


@pytest.fixture(scope="module")
def recorded():
    return cc.fixture()


def test_fixture_is_complete(recorded):
    assert recorded["split_bits"].shape == (52, 3, 2) and recorded["part_bits"].shape == (52, 2) and recorded["split_ctx"].shape == (4, 4)
    assert (recorded["split_bits"] > 0).all() and (recorded["part_bits"] > 0).all()


def test_every_bin_equals_hm(recorded):
    for qp in range(52):
        bins = ip.cu_tree_bins(qp)
        assert np.array_equal(bins["split"].astype(np.int64), recorded["split_bits"][qp]), qp
        assert np.array_equal(bins["part"].astype(np.int64), recorded["part_bits"][qp]), qp


def test_context_rule_equals_hm(recorded):
    """[left available and deeper] + [above available and deeper]; states 0 absent, 1 shallower, 2 equal, 3 deeper"""
    for left in range(4):
        for above in range(4):
            assert int(recorded["split_ctx"][left, above]) == int(left == 3) + int(above == 3)


@pytest.mark.parametrize("left_state", range(4))
@pytest.mark.parametrize("above_state", range(4))
def test_host_twin_takes_hm_context(recorded, left_state, above_state):
    """The root of one CTU beside edges in the given states, D = F = 0 everywhere: the root stays whole (a tie at worst), so the CTU's
    rate is exactly the bin of value 0 of the context the twin took -- all 15 fractional bits of it"""
    qp = 30
    zero = {w: (np.zeros((1, (64 // w) ** 2), np.uint32), np.zeros((1, (64 // w) ** 2), np.uint64), np.zeros((1, (64 // w) ** 2), np.uint64), None)
            for w in cc.WIDTHS}
    # the root has depth 0: no neighbour is shallower, "equal" is depth 0, "deeper" any of 1 .. 3
    depth = {0: 255, 1: 0, 2: 0, 3: 2}
    left = np.full((1, 1, 8), depth[left_state], np.uint8)
    above = np.full((1, 1, 8), depth[above_state], np.uint8)
    got = ip.cu_tree(zero, (qp,), (1.,), left, above)
    ctx = int(recorded["split_ctx"][left_state, above_state])
    bins = [int(recorded["split_bits"][qp][c][0]) for c in range(3)]
    assert len(set(bins)) == 3
    assert (got["cu_depths"] == 0).all() and int(got["ctu_rates"][0, 0]) == bins[ctx]
