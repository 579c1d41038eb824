"""CPU tests of HM's rate-distortion optimised quantisation (include/pnn_hip.h, "rate-distortion optimised quantisation"; DESIGN.md
section 5m) against HM-16.15 ITSELF: the host twin behind pnn_rdoq_unit_host, pnn_trquant_stages_rdoq_host, pnn_trquant_rdoq_host and
pnn_rdoq_est_bits_host on the units of tests/golden/hm_rdoq.npz, which HM's own transformNxN (xRateDistOptQuant), estBit, codeCoeffNxN
and invTransformNxN produced (tests/golden/make_hm_rdoq.py; layout, cases and edges: tests/hm_rdoq_cases.py).  Everything is compared
exactly.  Also: the option off is the old entries byte for byte, known answers derived here, the refusals."""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import hm_rdoq_cases as rq
from tests import trquant_cases as tq

PNN_E_ARG = -1
HM_TREE = "/root/reference/hevc/hm_16_15_regular"


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(rq.FIXTURE))


def lambda_of(fixture, t, k):
    return float(fixture["case_lambda_%d" % t][k:k + 1].view(np.float64)[0])


@pytest.mark.parametrize("t", rq.SIZES)
def test_est_bits_are_hm_s_tables(fixture, t):
    """Every entry estBit fills at this size (the others are -1 in the fixture) equals the twin's table, at every QP."""
    for qi, qp in enumerate(rq.QPS):
        mine = np.zeros(rq.EST_WORDS, np.int32)
        assert _lib.lib().pnn_rdoq_est_bits_host(t, qp, mine.ctypes.data) == 0
        hm = fixture["est_bits_%d" % t][qi]
        filled = hm >= 0
        assert filled.sum() >= 2 * (2 + 7 + 16 + 4) + 2 * (2 * (t.bit_length() - 1)) + 4
        np.testing.assert_array_equal(mine[filled], hm[filled])


@pytest.mark.parametrize("t", rq.SIZES)
def test_the_unit_entry_gives_hm_s_levels_and_abs_sum(fixture, t):
    """pnn_rdoq_unit_host on this project's coefficients of every recorded case: HM's levels and uiAbsSum, under HM's scan, lambda and
    cbf context, flag off and on."""
    cases = rq.cases_of(t)
    for k, (p, qp, f, sdh, depth) in enumerate(cases):
        residual = fixture["pair_targets_%d" % t][p].astype(np.int64) - fixture["pair_predictions_%d" % t][p].astype(np.int64)
        levels, abs_sum = ip.rdoq_unit(tq.forward(residual), int(fixture["case_scan_%d" % t][k]), qp, lambda_of(fixture, t, k),
                                       int(fixture["case_cbf_ctx_%d" % t][k]), bool(sdh))
        np.testing.assert_array_equal(levels, fixture["case_levels_%d" % t][k], err_msg="T %d case %d %r" % (t, k, cases[k]))
        assert abs_sum == fixture["case_abs_sum_%d" % t][k], (t, k, cases[k])
        assert int(fixture["case_cbf_ctx_%d" % t][k]) == 1 - depth


@pytest.mark.parametrize("t", rq.SIZES)
def test_the_stages_entry_gives_hm_s_levels_residual_and_bits(fixture, t):
    """pnn_trquant_stages_rdoq_host from the pair itself: levels_hidden and the inverse transform's residual are HM's, `levels` is what
    the same case gives with the flag off, and the rate of the levels is codeCoeffNxN's m_fracBits."""
    L = _lib.lib()
    cases = rq.cases_of(t)
    index = {case: k for k, case in enumerate(cases)}
    for k, (p, qp, f, sdh, depth) in enumerate(cases):
        if (p + k) % 3:                                  # a third of the cases: the unit entry above covers all of them
            continue
        scan = int(fixture["case_scan_%d" % t][k])
        outs = [np.zeros((t, t), np.int32) for _ in range(6)]
        assert L.pnn_trquant_stages_rdoq_host(fixture["pair_predictions_%d" % t][p].ctypes.data, fixture["pair_targets_%d" % t][p].ctypes.data,
                                              t, qp, scan, sdh, 1, lambda_of(fixture, t, k), 1 - depth, *[o.ctypes.data for o in outs]) == 0
        np.testing.assert_array_equal(outs[3], fixture["case_levels_%d" % t][k])
        np.testing.assert_array_equal(outs[1], fixture["case_levels_%d" % t][index[(p, qp, f, 0, depth)]])
        np.testing.assert_array_equal(outs[5], fixture["case_residual_%d" % t][k])
        assert ip.cabac_rate_of_levels(outs[3], scan, qp, bool(sdh)) == fixture["case_bits_%d" % t][k]


@pytest.mark.parametrize("t", rq.SIZES)
def test_the_batch_entry_gives_hm_s_counts_and_rate(fixture, t):
    """pnn_trquant_rdoq_host (behind transform_code) at w = T under HM's lambda: at w = 8, 16, 32 the recorded depth-0 cases (cbf context
    1), at w = 4 the depth-1 cases (context 0) -- uiAbsSum, the number of levels, the rate."""
    cases = rq.cases_of(t)
    depth = 1 if t == 4 else 0
    for sdh in (0, 1):
        res = ip.transform_code(fixture["pair_predictions_%d" % t], fixture["pair_targets_%d" % t], rq.QPS, rate=True,
                                modes=fixture["pair_modes_%d" % t], sign_data_hiding=bool(sdh), rdoq=True)
        for k, case in enumerate(cases):
            if case[2:] != (0, sdh, depth):
                continue
            p, qi = case[0], rq.QPS.index(case[1])
            assert res['sum_abs_levels'][qi, p] == fixture["case_abs_sum_%d" % t][k]
            assert res['nb_nonzero_levels'][qi, p] == np.count_nonzero(fixture["case_levels_%d" % t][k])
            assert res['rate_bits'][qi, p] * 32768 == fixture["case_bits_%d" % t][k]


@pytest.mark.parametrize("t", rq.SIZES)
def test_the_fixture_reaches_the_edges(fixture, t):
    count = rq.reached(fixture, t)
    assert not rq.wanted_edges(t) - set(count)
    assert count == rq.SHARES[t]


@pytest.mark.skipif(not os.path.isdir(HM_TREE), reason="the HM tree is not on this machine")
def test_the_fixture_regenerates_byte_for_byte(tmp_path):
    import subprocess
    import sys
    generator = os.path.join(os.path.dirname(rq.FIXTURE), "make_hm_rdoq.py")
    subprocess.check_call([sys.executable, generator, HM_TREE, "", str(tmp_path)], stdout=subprocess.DEVNULL)
    with open(os.path.join(str(tmp_path), "hm_rdoq.npz"), "rb") as new, open(rq.FIXTURE, "rb") as old:
        assert new.read() == old.read()


@pytest.mark.parametrize("w", (4, 8, 16, 32, 64))
def test_the_restatement_equals_the_twin_on_the_seeded_gpu_cases(w):
    """The blocks, QP lists, mode arrays and lambdas of tests/test_gpu_rdoq.py's parity test, where the kernel's only other yardstick is
    the twin: hm_rdoq_cases.walk -- written from HM's text in Python, equal to HM on every unit of the fixture -- gives the twin's levels
    and uiAbsSum on every unit, with the hiding off and on, under HM's lambda and the caller's."""
    from tests import cabac_rate_cases as cabac
    from tests.test_gpu_rdoq import QP_LISTS, seeded_blocks
    t = min(w, 32)
    cbf_ctx = 1 if w in (8, 16, 32) else 0
    for nb_qps in (1, 4, 8):
        predictions, targets, mode_array, own = seeded_blocks(w, nb_qps)
        blocks = range(len(predictions)) if w <= 8 else (0, 2, len(predictions) - 1)         # (the extremes, a random one, the ragged one)
        for b in blocks:
            for modes, flag, lambdas in ((None, 0, None), (mode_array, 1, None), (mode_array, 0, own), (None, 1, own)):
                scan = cabac.scan_of_mode(t, None if modes is None else int(modes[b]))
                for qi, qp in enumerate(QP_LISTS[nb_qps]):
                    lam = ip.hm_intra_lambda(qp) if lambdas is None else lambdas[qi]
                    for uy in range(w // t):
                        for ux in range(w // t):
                            window = (slice(uy * t, uy * t + t), slice(ux * t, ux * t + t))
                            coeffs = tq.forward(targets[b][window].astype(np.int64) - predictions[b][window].astype(np.int64))
                            want, want_sum = rq.walk(coeffs, scan, qp, lam, cbf_ctx, flag)
                            got, got_sum = ip.rdoq_unit(coeffs, scan, qp, lam, cbf_ctx, bool(flag))
                            assert np.array_equal(got, want) and got_sum == want_sum, (w, nb_qps, b, flag, qp, uy, ux)


def test_the_option_off_is_the_old_entries_byte_for_byte():
    """rdoq = 0 through the new entries (a lambda is not even read: NaN) equals pnn_trquant_sdh_host / _stages_sdh_host."""
    L = _lib.lib()
    nan = (ctypes.c_double * 2)(float('nan'), -1.)
    for w in (4, 8, 16, 32, 64):
        predictions, targets = tq.mixed_pairs(w, 6, 9300 + w)
        modes = np.array([0, 26, 10, 1, 22, 14], np.uint8)
        qps = (ctypes.c_int * 2)(22, 37)
        for flag in (0, 1):
            old = [np.zeros((2, 6), np.uint32) for _ in range(3)] + [np.zeros((2, 6, w, w), np.uint8), np.zeros((2, 6), np.uint64)]
            new = [np.zeros_like(o) for o in old]
            front = (predictions.ctypes.data, targets.ctypes.data, w, 6, modes.ctypes.data, qps, 2)
            assert L.pnn_trquant_sdh_host(*front, *[o.ctypes.data for o in old], flag) == 0
            assert L.pnn_trquant_rdoq_host(*front, *[o.ctypes.data for o in new], flag, 0, nan) == 0
            for a, b in zip(old, new):
                assert a.tobytes() == b.tobytes()
            old = [np.zeros((w, w), np.int32) for _ in range(6)]
            new = [np.zeros_like(o) for o in old]
            assert L.pnn_trquant_stages_sdh_host(predictions[4].ctypes.data, targets[4].ctypes.data, w, 30, 0, flag, *[o.ctypes.data for o in old]) == 0
            assert L.pnn_trquant_stages_rdoq_host(predictions[4].ctypes.data, targets[4].ctypes.data, w, 30, 0, flag, 0, float('nan'), 7,
                                                  *[o.ctypes.data for o in new]) == 0
            for a, b in zip(old, new):
                assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("t", rq.SIZES)
def test_known_answers(t):
    """Derived here.  (1) A zero residual costs nothing and changes nothing.  (2) Under a huge lambda every rate term dwarfs every
    distortion, and "nothing coded" (one cbf bin) is cheaper than any last position: all levels 0.  (3) Under a tiny lambda
    (2^-60: every lambda * bits is below 2^-35, while two candidate distortions differ by at least errScale > 2^-22 unless they are equal)
    the walk picks the level nearer to |C| scale / 2^qbits.  Where lLevelDouble mod 2^qbits is not exactly 2^(qbits - 1) -- the only
    tie between uiMaxAbsLevel and uiMaxAbsLevel - 1 -- and not below 2^(qbits - 1) with uiMaxAbsLevel < 3 turned to 0 (distortion
    alone never prefers 0 over the nearer level 1 or 2, the rounding being to nearest), that is uiMaxAbsLevel, and no group or last
    position is dropped, each drop raising the distortion."""
    zero, abs_sum = ip.rdoq_unit(np.zeros((t, t), np.int64), 0, 30)
    assert abs_sum == 0 and not zero.any()
    rng = np.random.default_rng(77 + t)
    coeffs = (2 * rng.integers(-1500, 1500, (t, t)) + 1) * (rng.random((t, t)) < 0.4)     # odd or 0: |C| scale has fewer than 15 factors 2, no tie
    for qp in (0, 22, 37, 51):
        levels, abs_sum = ip.rdoq_unit(coeffs, 0, qp, lam=1e30)
        assert abs_sum == 0 and not levels.any()
        top = rq.max_levels(coeffs, qp)
        log2_t = t.bit_length() - 1
        qbits = 14 + qp // 6 + 7 - log2_t
        level_double = np.abs(coeffs) * tq.QUANT_SCALES[qp % 6]
        assert not np.any((level_double & ((1 << qbits) - 1)) == 1 << (qbits - 1))        # no exact tie among these coefficients
        for cbf_ctx in (0, 1):
            levels, abs_sum = ip.rdoq_unit(coeffs, 0, qp, lam=2. ** -60, cbf_ctx=cbf_ctx)
            np.testing.assert_array_equal(levels, np.sign(coeffs) * top)
            assert abs_sum == top.sum()


def test_argument_errors():
    L = _lib.lib()
    coeffs, levels = np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int32)
    good = dict(t=4, scan=0, qp=22, lam=1., ctx=1)
    def unit(**kw):  # noqa: E306
        a = dict(good, **kw)
        return L.pnn_rdoq_unit_host(coeffs.ctypes.data, a['t'], a['scan'], a['qp'], a['lam'], a['ctx'], 0, levels.ctypes.data, None)
    assert unit() == 0
    for bad in (dict(t=5), dict(scan=3), dict(qp=52), dict(lam=0.), dict(lam=-1.), dict(lam=float('nan')), dict(lam=float('inf')), dict(ctx=2),
                dict(ctx=-1)):
        assert unit(**bad) == PNN_E_ARG
    assert L.pnn_rdoq_unit_host(None, 4, 0, 22, 1., 1, 0, levels.ctypes.data, None) == PNN_E_ARG
    big = np.full((4, 4), 40000, np.int32)
    assert L.pnn_rdoq_unit_host(big.ctypes.data, 4, 0, 22, 1., 1, 0, levels.ctypes.data, None) == PNN_E_ARG
    assert L.pnn_rdoq_unit_host(np.zeros((16, 16), np.int32).ctypes.data, 16, 1, 22, 1., 1, 0, np.zeros((16, 16), np.int32).ctypes.data, None) == PNN_E_ARG
    block = np.zeros((2, 8, 8), np.uint8)
    qps, out = (ctypes.c_int * 1)(22), np.zeros((1, 2), np.uint32)
    for lam in (0., -2., float('nan'), float('inf')):
        assert L.pnn_trquant_rdoq_host(block.ctypes.data, block.ctypes.data, 8, 2, None, qps, 1, out.ctypes.data, None, None, None, None, 0, 1,
                                       (ctypes.c_double * 1)(lam)) == PNN_E_ARG
        assert L.pnn_trquant_stages_rdoq_host(block.ctypes.data, block.ctypes.data, 8, 22, 0, 0, 1, lam, 1, out.ctypes.data, None, None, None, None,
                                              None) == PNN_E_ARG
    assert L.pnn_trquant_stages_rdoq_host(block.ctypes.data, block.ctypes.data, 8, 22, 0, 0, 1, 1., 2, out.ctypes.data, None, None, None, None,
                                          None) == PNN_E_ARG
    assert L.pnn_rdoq_est_bits_host(4, 22, None) == PNN_E_ARG
    with pytest.raises(ValueError):
        ip.transform_code(block, block, (22,), lambdas=(1.,))
    with pytest.raises(ValueError):
        ip.transform_code(block, block, (22,), rdoq=True, lambdas=(0.,))
    with pytest.raises(ValueError):
        ip.rdoq_unit(coeffs, 0, 22, lam=0.)
