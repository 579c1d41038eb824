"""CPU test of HM's transform skip for 4 x 4 luma units (include/pnn_hip.h, "transform skip") against HM-16.15
ITSELF: pnn_tskip_unit_host on every record of tests/golden/hm_transform_skip.npz, which HM's own transformNxN (xTransformSkip, xQuant /
xRateDistOptQuant), invTransformNxN, codeCoeffNxN with the PPS flag on and codeTransformSkipFlags produced
(tests/golden/make_hm_transform_skip.py: layout and the edges the recorded output has to reach).  Everything is compared exactly: the
coefficients, the levels and uiAbsSum of both forms, the decoded residual, the fractional bits with flag 0 and 1 and of the flag alone, at
the four QPs and three scans, RDOQ off and on, sign hiding off and on."""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hm_transform_skip.npz")
PNN_E_ARG = -1


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE))


def unit(residual, scan, qp, sdh, rdoq, lam, form):
    residual = np.ascontiguousarray(residual, np.int32)
    coeffs, levels, back = (np.zeros((4, 4), np.int32) for _ in range(3))
    abs_sum, bits, flag = ctypes.c_int32(-1), np.zeros(1, np.uint64), np.zeros(2, np.uint64)
    rc = _lib.lib().pnn_tskip_unit_host(residual.ctypes.data, scan, qp, sdh, rdoq, lam, form, coeffs.ctypes.data, levels.ctypes.data,
                                        ctypes.byref(abs_sum), back.ctypes.data, bits.ctypes.data, flag.ctypes.data)
    return rc, coeffs, levels, int(abs_sum.value), back, int(bits[0]), flag


def test_the_fixture_covers_what_the_issue_names(fixture):
    f = fixture
    assert set(f["case_qp"]) == {0, 22, 37, 51} and set(f["case_scan"]) == {0, 1, 2}
    assert set(f["case_rdoq"]) == {0, 1} and set(f["case_sdh"]) == {0, 1}
    cbf = f["case_abs_sum"] > 0
    assert (cbf[:, 0] & ~cbf[:, 1]).any() and (~cbf[:, 0] & cbf[:, 1]).any()
    for qp in (0, 22, 37, 51):
        assert (cbf[f["case_qp"] == qp]).any(0).all()
    assert f["residuals"].min() == -255 and f["residuals"].max() == 255 and not f["residuals"][0].any()


@pytest.mark.parametrize("rdoq", (0, 1))
@pytest.mark.parametrize("sdh", (0, 1))
def test_the_unit_entry_gives_hm_s_records(fixture, rdoq, sdh):
    f = fixture
    cases = np.nonzero((f["case_rdoq"] == rdoq) & (f["case_sdh"] == sdh))[0]
    assert cases.size == f["residuals"].shape[0] * 4 * 3
    for k in cases:
        residual, qp, scan = f["residuals"][f["case_residual"][k]], int(f["case_qp"][k]), int(f["case_scan"][k])
        lam = float(f["case_lambda"][k:k + 1].view(np.float64)[0])
        for form in (0, 1):
            rc, coeffs, levels, abs_sum, back, bits, flag = unit(residual, scan, qp, sdh, rdoq, lam, form)
            assert rc == 0
            where = "case %d form %d" % (k, form)
            np.testing.assert_array_equal(levels, f["case_levels"][k, form], where)
            assert abs_sum == f["case_abs_sum"][k, form], where
            assert bits == f["case_bits"][k, form], where
            if form:
                np.testing.assert_array_equal(coeffs, f["case_coeffs"][k], where)
                np.testing.assert_array_equal(coeffs, residual.astype(np.int32) * 32, where)
                np.testing.assert_array_equal(back, f["case_back"][k], where)
            np.testing.assert_array_equal(flag, f["flag_bits"][list(f["qps"]).index(qp)].astype(np.uint64), where)


def test_the_flag_bin_is_what_separates_the_forms_rates(fixture):
    """With the same levels the two flag values differ by the two bins of the flag's context; a unit without a level pays nothing."""
    rc, _, levels, abs_sum, _, bits, flag = unit(np.zeros((4, 4)), 0, 22, 0, 0, 1., 1)
    assert rc == 0 and not levels.any() and abs_sum == 0 and bits == 0 and flag[0] > 0 and flag[1] > 0


def test_refusals():
    ok = np.zeros((4, 4), np.int32)
    assert unit(ok, 3, 22, 0, 0, 1., 1)[0] == PNN_E_ARG
    assert unit(ok, 0, 52, 0, 0, 1., 1)[0] == PNN_E_ARG
    assert unit(ok, 0, 22, 0, 0, 1., 2)[0] == PNN_E_ARG
    assert unit(ok, 0, 22, 0, 1, 0., 1)[0] == PNN_E_ARG
    assert unit(ok + 256, 0, 22, 0, 0, 1., 1)[0] == PNN_E_ARG
    assert _lib.lib().pnn_tskip_unit_host(None, 0, 22, 0, 0, 1., 1, None, None, None, None, None, None) == PNN_E_ARG
