"""GPU tests of the transform-coding column against HM-16.15 DIRECTLY: trquant_kernel behind pnn_trquant_sdh_device and the second-pass
launches behind pnn_rd_pass_device on the units of tests/golden/hm_unit_coding.npz, whose levels, uiAbsSum, m_fracBits increase and
reconstructed residual HM's own transformNxN, codeCoeffNxN and invTransformNxN recorded (tests/golden/make_hm_unit_coding.py).  Not the
host twin: every expected number here is HM's.  Integer equality, every output between guard bytes; only the committed fixture is read."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import hm_unit_cases as units
from tests import util
from tests.trquant_cases import blocks_per_workgroup, specs_of
from tests.util import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hm():
    return dict(np.load(units.FIXTURE))


def expected(hm, t, flag):
    """{(pair, QP index): (sse_recon, nb_nonzero, uiAbsSum, reconstruction, bits)} from HM's records with the flag"""
    out = {}
    for k, (p, qp, f) in enumerate(zip(hm['case_pair_%d' % t], hm['case_qp_%d' % t], hm['case_sdh_%d' % t])):
        if int(f) != flag:
            continue
        prediction, target = hm['pair_predictions_%d' % t][p].astype(np.int64), hm['pair_targets_%d' % t][p].astype(np.int64)
        recon = np.clip(prediction + hm['case_residual_%d' % t][k], 0, 255)
        out[(int(p), units.QPS.index(int(qp)))] = (int(((recon - target) ** 2).sum()), int(np.count_nonzero(hm['case_levels_%d' % t][k])),
                                                    int(hm['case_abs_sum_%d' % t][k]), recon.astype(np.uint8), int(hm['case_bits_%d' % t][k]))
    return out


def device_call(w, predictions, targets, modes, flag):
    """pnn_trquant_sdh_device at the four QPs, every output between guard bytes: (sses, nb_nonzero, sum_abs, recon, rate)"""
    n, nq = predictions.shape[0], len(units.QPS)
    d_p, d_t, d_m = dev(predictions), dev(targets), None if modes is None else dev(modes)
    front = (ip._context(0), w, d_p.data_ptr(), d_t.data_ptr(), n, util.ptr(d_m), (ctypes.c_int * nq)(*units.QPS), nq)
    rc, outs, intact = util.call("pnn_trquant_sdh_device", front, (), specs_of(w, n, nq), (True,) * 5, after=(flag,))
    assert rc == 0 and intact
    return outs


@pytest.mark.parametrize("flag", (0, 1))
@pytest.mark.parametrize("t", units.SIZES)
def test_kernel_equals_hm(hm, t, flag):
    """n = 2 G + 1 units per launch (two full workgroups and a ragged one), launch after launch through all the fixture's pairs of
    that T, each with its mode, four QPs in one call; then n = 1.  A pair is compared at every QP HM coded it at."""
    want = expected(hm, t, flag)
    predictions, targets, modes = (hm['pair_%s_%d' % (name, t)] for name in ('predictions', 'targets', 'modes'))
    nb_pairs, n = len(modes), 2 * blocks_per_workgroup(t) + 1
    compared = 0
    for start in list(range(0, nb_pairs, n)) + [None]:
        pairs = np.array([4]) if start is None else (start + np.arange(n)) % nb_pairs         # (pair 4: a random pair, coded at every QP)
        outs = device_call(t, predictions[pairs], targets[pairs], modes[pairs], flag)
        for b, p in enumerate(pairs):
            for qi in range(len(units.QPS)):
                if (int(p), qi) not in want:
                    continue
                label = "T %d flag %d pair %d QP %d" % (t, flag, p, units.QPS[qi])
                sse, nonzero, abs_sum, recon, bits = want[(int(p), qi)]
                assert (int(outs[0][qi, b]), int(outs[1][qi, b]), int(outs[2][qi, b]), int(outs[4][qi, b])) == (sse, nonzero, abs_sum, bits), label
                assert np.array_equal(outs[3][qi, b], recon), label
                compared += 1
    assert compared >= len(want) + len(units.QPS)


@pytest.mark.parametrize("flag", (0, 1))
def test_quadrants_at_width_64_equal_hm(hm, flag):
    """Four fixture units of T = 32 as the quadrants of one 64 x 64 block: rate and sums added, each quadrant reconstructed as HM does."""
    want = expected(hm, 32, flag)
    predictions, targets = hm['pair_predictions_32'], hm['pair_targets_32']
    layouts = np.array([(4, 5, 0, 2), (2, 4, 1, 5), (5, 3, 4, 0)])                             # base pairs: coded at every QP
    assert layouts.max() < units.NB_BASE_PAIRS[32]

    def blocks(source):
        out = np.zeros((len(layouts), 64, 64), np.uint8)
        for b, layout in enumerate(layouts):
            for q, p in enumerate(layout):
                out[b, 32 * (q // 2):32 * (q // 2) + 32, 32 * (q % 2):32 * (q % 2) + 32] = source[p]
        return out

    for n in (len(layouts), 1):
        outs = device_call(64, blocks(predictions)[:n], blocks(targets)[:n], None, flag)
        for b in range(n):
            for qi in range(len(units.QPS)):
                parts = [want[(int(p), qi)] for p in layouts[b]]
                label = "flag %d block %d QP %d" % (flag, b, units.QPS[qi])
                for k, name in ((0, 'sses_recon'), (1, 'nb_nonzero'), (2, 'sum_abs_levels'), (4, 'rate')):
                    assert int(outs[k][qi, b]) == sum(part[k] for part in parts), (label, name)
                for q, part in enumerate(parts):
                    got = outs[3][qi, b, 32 * (q // 2):32 * (q // 2) + 32, 32 * (q % 2):32 * (q % 2) + 32]
                    assert np.array_equal(got, part[3]), (label, q)
        assert outs[4].all()


def test_second_pass_costs_equal_hm(hm):
    """pnn_rd_pass_device at w = 8 under the caller's lambdas, taken from triples that differ under a fused multiply-add: every winner's
    cost has the bits of HM's calcRdCost."""
    units.check_second_pass(hm, device=0)
