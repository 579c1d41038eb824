"""CPU tests of transform skip in the transform-coding column (include/pnn_hip.h, "transform skip"): the host twin
behind pnn_trquant_tskip_host and intraprediction.transform_code(transform_skip=...) against the Python restatement of
tests/transform_skip_cases.py (which tests/test_hm_transform_skip.py's fixture and the earlier fixtures pin to HM), exactly; known
answers derived here; conditions on the seeded cases with the shares written down; the refusals."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import transform_skip_cases as tc

PNN_E_ARG = -1


def assert_same(outs, want, label):
    for key, got in zip(tc.KEYS, outs):
        assert np.array_equal(got, want[key]), "%s %s: %d differing values" % (label, key, (got != want[key]).sum())


@pytest.mark.parametrize("qps", tc.QP_PAIRS)
@pytest.mark.parametrize("rdoq", (0, 1))
@pytest.mark.parametrize("sdh", (0, 1))
def test_host_twin_against_the_restatement(qps, rdoq, sdh):
    """n = 129 and n = 1; forced and decide; modes given and NULL; mode_bits given and NULL; charge_cbf 0 and 1; HM's lambdas and own"""
    predictions, targets, modes = tc.blocks(129)
    mode_bits = tc.seeded_mode_bits(2, 129)
    own = [ip.hm_intra_lambda(qps[0]) * 0.6, ip.hm_intra_lambda(qps[1]) * 1.7]
    for option, m, bits, cbf, lambdas in ((1, modes, None, 1, None), (2, modes, mode_bits, 1, None), (2, None, None, 0, own),
                                         (2, modes, None, 1, own), (2, None, mode_bits, 0, None)):
        label = "QPs %s rdoq %d sdh %d option %d modes %s bits %s cbf %d" % (qps, rdoq, sdh, option, m is not None, bits is not None, cbf)
        rc, outs = tc.host_entry(predictions, targets, m, qps, sdh, rdoq, lambdas, option, bits, cbf)
        assert rc == 0, label
        assert_same(outs, tc.column(predictions, targets, m, qps, sdh, rdoq, lambdas, option, bits, cbf), label)
    rc, outs = tc.host_entry(predictions[:1], targets[:1], modes[:1], qps, sdh, rdoq, None, 2, mode_bits[:, :1].copy(), 1)
    assert rc == 0
    assert_same(outs, tc.column(predictions[:1], targets[:1], modes[:1], qps, sdh, rdoq, None, 2, mode_bits[:, :1], 1), "n 1")


def test_conditions_on_the_seeded_cases():
    """Each on at least 5 % of the (QP, unit) pairs of the 129 seeded blocks at the QPs 22 and 37, RDOQ and hiding on, found with the
    restatement alone: the skipped form wins; the transformed form wins with cbf 1; the skipped form is forbidden by cbf 0."""
    predictions, targets, modes = tc.blocks(129)
    want = tc.column(predictions, targets, modes, (22, 37), 1, 1, None, 2, tc.seeded_mode_bits(2, 129), 1)
    flags = want['transform_skip_flags'].astype(bool)
    shares = {"skipped wins": flags.mean(), "transformed wins with cbf 1": (~flags & want['transformed_cbf']).mean(),
              "skipped forbidden": (~want['skipped_cbf']).mean()}
    print(shares)
    for name, share in shares.items():
        assert share >= 0.05, (name, share)


def test_known_answers():
    qps = (22, 51)
    zero = np.full((3, 4, 4), 128, np.uint8)
    rc, outs = tc.host_entry(zero, zero, None, qps, 1, 1, None, 2, None, 1)                 # a zero residual: never skipped, no flag
    assert rc == 0 and not outs[5].any() and not outs[4].any() and not outs[0].any()
    rc, outs = tc.host_entry(zero, zero, None, qps, 0, 0, None, 1, None, 1)                 # ... forced: skipped, still no flag bin
    assert rc == 0 and outs[5].all() and not outs[4].any() and not outs[1].any()
    target = zero.copy()
    target[:, ::2, ::2] += 1
    target[:, 1::2, 1::2] -= 1
    rc, outs = tc.host_entry(zero, target, None, (51,), 0, 0, None, 1, None, 1)             # +-1 at QP 51, forced: cbf 0
    assert rc == 0 and not outs[1].any() and not outs[4].any() and (outs[3][0] == zero).all()
    # the option off: pnn_trquant_rdoq_host byte for byte
    predictions, targets, modes = tc.blocks(40)
    for sdh, rdoq in ((0, 0), (1, 1)):
        rc, outs = tc.host_entry(predictions, targets, modes, qps, sdh, rdoq, None, 0, None, 1)
        want = ip.transform_code(predictions, targets, qps, keep_reconstructions=True, modes=modes, rate=True, sign_data_hiding=sdh, rdoq=rdoq)
        assert rc == 0 and not outs[5].any()
        for got, key in zip(outs[:4], tc.KEYS[:4]):
            assert got.tobytes() == want[key].tobytes(), key
        assert np.array_equal(outs[4], np.rint(want['rate_bits'] * 32768).astype(np.uint64))
        # a transformed unit with cbf 1 pays exactly the flag-0 bin more than today; one with cbf 0 nothing
        rc, decided = tc.host_entry(predictions, targets, modes, qps, sdh, rdoq, None, 2, None, 1)
        assert rc == 0
        kept = decided[5] == 0
        assert (kept & (outs[1] > 0)).any()
        for qi, qp in enumerate(qps):
            extra = decided[4][qi].astype(np.int64) - outs[4][qi].astype(np.int64)
            assert (extra[kept[qi] & (outs[1][qi] > 0)] == tc.flag_bins(qp)[0]).all() and (extra[kept[qi] & (outs[1][qi] == 0)] == 0).all()


def test_a_tie_stays_transformed():
    """Under the smallest positive lambda, lambda R is exact and vanishes beside any D > 0: J = D.  Both forms of a block of extremes
    clip to the same reconstruction, so their J are equal -- and the unit stays transformed (strict <)."""
    predictions, targets, modes = tc.blocks(129)
    tiny = [5e-324, 5e-324]
    for qps in tc.QP_PAIRS:
        want = tc.column(predictions, targets, modes, qps, 0, 0, tiny, 2, None, 0)
        rc, outs = tc.host_entry(predictions, targets, modes, qps, 0, 0, tiny, 2, None, 0)
        assert rc == 0 and np.array_equal(outs[5], want['transform_skip_flags'])
        if want['tie'].any():
            assert not outs[5][want['tie']].any()
            return
    assert False, "no tie among the seeded cases"


def test_transform_code_option():
    predictions, targets, modes = tc.blocks(20)
    got = ip.transform_code(predictions, targets, (22, 37), keep_reconstructions=True, modes=modes, rate=True, sign_data_hiding=True, rdoq=True,
                            transform_skip='decide')
    want = tc.column(predictions, targets, modes, (22, 37), 1, 1, None, 2, None, 1)
    for key in tc.KEYS:
        mine = np.rint(got['rate_bits'] * 32768).astype(np.uint64) if key == 'rate' else got[key]
        assert np.array_equal(mine, want[key]), key
    off = ip.transform_code(predictions, targets, (22, 37), rate=True, modes=modes)
    assert 'transform_skip_flags' not in off
    with pytest.raises(ValueError):
        ip.transform_code(np.zeros((2, 8, 8), np.uint8), np.zeros((2, 8, 8), np.uint8), (22,), transform_skip='decide')
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (22,), transform_skip='on')
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (22,), transform_skip='forced', mode_bits=np.zeros((1, 20), np.uint32))


def test_refusals():
    predictions, targets, modes = tc.blocks(6)
    eight = np.zeros((2, 8, 8), np.uint8)
    assert tc.host_entry(predictions, targets, None, (22,), 0, 0, None, 3, None, 1)[0] == PNN_E_ARG
    assert tc.host_entry(predictions, targets, None, (22,), 0, 0, None, -1, None, 1)[0] == PNN_E_ARG
    assert tc.host_entry(predictions, targets, None, (22,), 0, 0, None, 2, None, 2)[0] == PNN_E_ARG
    assert tc.host_entry(predictions, targets, None, (22,), 0, 0, [0.], 2, None, 1)[0] == PNN_E_ARG
    assert tc.host_entry(predictions, targets, None, (22,), 0, 0, [float('nan')], 2, None, 1)[0] == PNN_E_ARG
    assert tc.host_entry(predictions, targets, None, (52,), 0, 0, None, 1, None, 1)[0] == PNN_E_ARG
    assert tc.host_entry(predictions, targets, None, (22,), 0, 0, None, 1, None, 1, wanted=(False,) * 6)[0] == PNN_E_ARG
    n, nq = 2, 1
    out = np.zeros((nq, n), np.uint32)
    for option in (1, 2):                                                   # width 8 with the option on
        assert _lib.lib().pnn_trquant_tskip_host(eight.ctypes.data, eight.ctypes.data, 8, n, None, (ctypes.c_int * 1)(22), 1, out.ctypes.data,
                                                 None, None, None, None, 0, 0, None, option, None, 1, None) == PNN_E_ARG
    assert _lib.lib().pnn_trquant_tskip_host(eight.ctypes.data, eight.ctypes.data, 8, n, None, (ctypes.c_int * 1)(22), 1, out.ctypes.data,
                                             None, None, None, None, 0, 0, None, 0, None, 1, None) == 0
    L = _lib.lib()
    assert L.pnn_trquant_tskip_workspace_bytes(8, 10, 2) == 0 and L.pnn_trquant_tskip_workspace_bytes(4, 10, 9) == 0
    assert L.pnn_trquant_tskip_workspace_bytes(4, 10, 2) >= 2 * 10 * 2 * (8 + 4 + 4 + 4 + 16)
