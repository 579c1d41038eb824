"""CPU tests of the open-loop transform coding's host twin (csrc/pnn_trquant.cpp; include/pnn_hip.h, "transform coding"): against a numpy
restatement written from the definition (tests/trquant_cases.py), against recorded outputs of HM's own xTrMxN / xITrMxN
(tests/golden/hm_transforms.npz, made by tests/golden/make_hm_transforms.py), on known answers, on bad arguments, and under
AddressSanitizer + UBSan as a stand-alone program.  Every comparison is integer equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import trquant_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNN_E_ARG = -1
INT_KEYS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels')


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_host_twin_against_numpy(w):
    """All three counts, the reconstruction and every stage, on random pairs, smooth pairs and the extremes, at the seven QPs."""
    predictions, targets = cases.mixed_pairs(w, 8 if w <= 16 else 6, 300 + w)
    want = cases.code(predictions, targets, cases.QPS)
    got = ip.transform_code(predictions, targets, cases.QPS, keep_reconstructions=True)
    for key in INT_KEYS + ('reconstructions_uint8',):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (w, key)
    assert np.array_equal(got['psnrs_recon'], ip.psnrs_from_sses(want['sses_recon'], w)) and got['psnrs_recon'].dtype == np.float64
    assert set(ip.transform_code(predictions, targets, cases.QPS)) == set(INT_KEYS) | {'psnrs_recon'}
    # [N, w, w, 1] in, the same out
    assert np.array_equal(ip.transform_code(predictions[..., None], targets[..., None], (22,))['sses_recon'][0], want['sses_recon'][2])
    for b in range(predictions.shape[0]):
        for qp in cases.QPS:
            model, twin = cases.stages(predictions[b], targets[b], qp), ip.transform_stages(predictions[b], targets[b], qp)
            assert set(twin) == {'coeffs', 'levels', 'dequant', 'residual'}
            for key, stage in twin.items():
                assert stage.dtype == np.int32 and stage.shape == (w, w) and np.array_equal(stage, model[key]), (w, b, qp, key)


@pytest.mark.parametrize("t", (4, 8, 16, 32))
def test_transforms_against_hm(t):
    """The forward transform's coefficients equal what HM's xTrMxN gave for the same residuals, and the inverse transform's residual what
    HM's xITrMxN gave for the same dequantised coefficients (the fixture's 'dequant', which the host twin must reproduce first)."""
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "hm_transforms.npz"))
    predictions, targets = fixture["predictions_%d" % t], fixture["targets_%d" % t]
    assert predictions.shape[0] >= 24
    for b in range(predictions.shape[0]):
        for qi, qp in enumerate(fixture["qps"]):
            twin = ip.transform_stages(predictions[b], targets[b], int(qp))
            assert np.array_equal(twin['coeffs'], fixture["coeffs_%d" % t][b]), (t, b)
            assert np.array_equal(twin['dequant'], fixture["dequant_%d" % t][qi, b]), (t, b, qp)
            assert np.array_equal(twin['residual'], fixture["residual_%d" % t][qi, b]), (t, b, qp)
    if t == 32:   # the four units of a 64 x 64 block are four such transforms, each where its quadrant lies
        p64, t64 = np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8)
        for q in range(4):
            unit = (slice(32 * (q // 2), 32 * (q // 2) + 32), slice(32 * (q % 2), 32 * (q % 2) + 32))
            p64[unit], t64[unit] = predictions[4 + q], targets[4 + q]
        twin = ip.transform_stages(p64, t64, int(fixture["qps"][1]))
        for q in range(4):
            unit = (slice(32 * (q // 2), 32 * (q // 2) + 32), slice(32 * (q % 2), 32 * (q % 2) + 32))
            assert np.array_equal(twin['coeffs'][unit], fixture["coeffs_32"][4 + q])
            assert np.array_equal(twin['residual'][unit], fixture["residual_32"][1, 4 + q])


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_zero_residual(w):
    predictions, _ = cases.random_pairs(w, 3, 40 + w)
    got = ip.transform_code(predictions, predictions, cases.QPS, keep_reconstructions=True)
    for key in INT_KEYS:
        assert not got[key].any(), key
    assert all(np.array_equal(r, predictions) for r in got['reconstructions_uint8'])


@pytest.mark.parametrize("w", (8, 16, 32, 64))
@pytest.mark.parametrize("d", (1, -3, 40, -100))
def test_constant_residual_at_qp_22(w, d):
    """A constant residual d, T >= 8, prediction + d in range.  Forward: row 0 of M is 64 everywhere and every other row sums to 0, so
    the first stage leaves Y[y][0] = (64 T d + 2^(L-2)) >> (L - 1) = 128 d and zeros, the second C[0][0] = (64 T 128 d + 2^(L+5)) >>
    (L + 6) = 128 d and zeros.  QP 22: per 3, rem 4, scale 2^14, qbits = 17 + ts = 24 - L, so mag = floor(128 |d| 2^14 / 2^(24-L) +
    171 / 512) = |d| 2^(L-3) = |d| T / 8: ONE nonzero level per unit.  Back: inv 64, rs = L - 4, C' = level 2^(10-L) = 128 d exactly;
    Z[y][0] = (64 * 128 d + 64) >> 7 = 64 d, R = (64 * 64 d + 2048) >> 12 = d: the reconstruction IS the target."""
    t, units = min(w, 32), (w // min(w, 32)) ** 2
    predictions = np.full((2, w, w), 120, np.uint8)
    predictions[1] = 104
    targets = (predictions.astype(np.int64) + d).astype(np.uint8)
    got = ip.transform_code(predictions, targets, (22,), keep_reconstructions=True)
    assert (got['nb_nonzero_levels'] == units).all()
    assert (got['sum_abs_levels'] == units * abs(d) * t // 8).all()
    assert not got['sses_recon'].any() and np.array_equal(got['reconstructions_uint8'][0], targets)
    stages = ip.transform_stages(predictions[0], targets[0], 22)
    assert stages['coeffs'][0, 0] == 128 * d and np.count_nonzero(stages['coeffs']) == units and (stages['residual'] == d).all()


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_sse_grows_with_qp_on_smooth_blocks(w):
    """sse_recon is non-decreasing from QP 22 to QP 51 on smooth residuals -- not a theorem (the dead zone can favour a coarser step), so
    only the blocks on which the numpy model itself says so are kept; most are."""
    qps = (22, 27, 32, 37, 51)
    predictions, targets = cases.smooth_pairs(w, 12, 500 + w)
    model = cases.code(predictions, targets, qps)['sses_recon'].astype(np.int64)
    keep = (np.diff(model, axis=0) >= 0).all(axis=0)
    assert keep.sum() >= 6, "the model itself is not monotone on most smooth blocks"
    got = ip.transform_code(predictions[keep], targets[keep], qps)['sses_recon'].astype(np.int64)
    assert np.array_equal(got, model[:, keep]) and (np.diff(got, axis=0) >= 0).all()


def test_argument_errors():
    L = _lib.lib()
    w = 8
    predictions, targets = cases.random_pairs(w, 2, 7)
    out = np.full(2, 0xA5A5A5A5, np.uint32)
    stage = np.full((w, w), 0x5A5A5A5A, np.int32)
    good = (ctypes.c_int * 1)(22)

    def host(width=w, n=2, qps=good, nb=1, p=predictions.ctypes.data, t=targets.ctypes.data, o=out.ctypes.data):
        return L.pnn_trquant_host(p, t, width, n, qps, nb, o, None, None, None)

    def stages(width=w, qp=22, p=predictions.ctypes.data, t=targets.ctypes.data, o=stage.ctypes.data):
        return L.pnn_trquant_stages_host(p, t, width, qp, o, None, None, None)
    assert host(width=12) == PNN_E_ARG and host(n=-1) == PNN_E_ARG and host(p=None) == PNN_E_ARG and host(t=None) == PNN_E_ARG
    assert host(nb=0) == PNN_E_ARG and host(qps=(ctypes.c_int * 9)(*[22] * 9), nb=9) == PNN_E_ARG and host(qps=None) == PNN_E_ARG
    assert host(qps=(ctypes.c_int * 1)(52)) == PNN_E_ARG and host(qps=(ctypes.c_int * 1)(-1)) == PNN_E_ARG and host(o=None) == PNN_E_ARG
    assert stages(width=0) == PNN_E_ARG and stages(qp=52) == PNN_E_ARG and stages(qp=-1) == PNN_E_ARG
    assert stages(p=None) == PNN_E_ARG and stages(t=None) == PNN_E_ARG and stages(o=None) == PNN_E_ARG
    assert (out == 0xA5A5A5A5).all() and (stage == 0x5A5A5A5A).all()
    # the device entry without a context refuses before it touches anything
    assert L.pnn_trquant_device(None, w, None, None, 2, good, 1, None, None, None, None, None) == PNN_E_ARG
    # the same calls with good arguments go through; n == 0 does nothing
    assert host(n=0, p=None, t=None) == 0 and (out == 0xA5A5A5A5).all()
    assert host() == 0 and stages() == 0 and not (out == 0xA5A5A5A5).any()
    # transform_code / transform_stages: ValueError for the QPs, TypeError for the arrays' type
    for qps in ((), (22,) * 9, (22.0,), (52,), (-1,), ('22',), (True,), 22, None):
        with pytest.raises(ValueError):
            ip.transform_code(predictions, targets, qps)
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets[:1], (22,))
    with pytest.raises(ValueError):
        ip.transform_code(predictions[:, :, :4], targets[:, :, :4], (22,))
    with pytest.raises(ValueError):
        ip.transform_code(np.zeros((1, 12, 12), np.uint8), np.zeros((1, 12, 12), np.uint8), (22,))
    with pytest.raises(TypeError):
        ip.transform_code(predictions.astype(np.int32), targets, (22,))
    with pytest.raises(ValueError):
        ip.transform_stages(predictions[0], targets[0], 52)
    with pytest.raises(ValueError):
        ip.transform_stages(predictions, targets, 22)


def test_host_twin_under_sanitizers(tmp_path):
    """tests/sanitize_trquant.cpp (its own main) and the host twin, compiled together under AddressSanitizer + UBSan and run as a child
    process: both host entries at every width, the extreme residuals and QPs, every output alone.  Any report aborts the program."""
    csrc = os.path.join(ROOT, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    exe = str(tmp_path / "sanitize_trquant")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                        "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize_trquant.cpp"),
                        os.path.join(csrc, "pnn_trquant.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_trquant: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
