"""CPU tests of HM's second intra pass as a column (include/pnn_hip.h, "the second intra pass"): the host twin
pnn_rd_pass_host behind intraprediction.rd_pass(device=None) against a Python restatement made of the existing Python entries, the
lambda, known answers derived here, the conditions the seeded cases of the GPU tests must meet, argument errors and the sanitizer
program.  Doubles are compared by bit pattern."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import rd_pass_cases as cases
from tests.rd_pass_cases import CANDIDATE, UNUSED

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QPS = (22, 27, 32, 37, 0, 51)


@pytest.mark.parametrize("sign_data_hiding", (False, True), ids=("plain", "sdh"))
@pytest.mark.parametrize("smoothing", (0, 2))
@pytest.mark.parametrize("w", cases.WIDTHS)
def test_host_twin_equals_restatement(w, smoothing, sign_data_hiding):
    n = 6 if w <= 16 else 4
    patterns, targets, candidates = cases.seeded(w, n, seed=900 + w)
    for lambdas in (None, [0.25 * (i + 1) for i in range(len(QPS))]):
        got = ip.rd_pass(patterns, targets, candidates, QPS, smoothing, sign_data_hiding, lambdas)
        want = cases.restatement(patterns, targets, candidates, QPS, smoothing, sign_data_hiding, lambdas)
        cases.same_bits(got, want, "w %d smoothing %d sdh %s" % (w, smoothing, sign_data_hiding))
        assert np.array_equal(got['psnrs_recon'], ip.psnrs_from_sses(got['sses'], w))
    assert np.isinf(got['costs'][:, got['candidates'][:, -1] == UNUSED, -1]).all()
    assert np.isfinite(got['costs'][:, :, :-1]).all()


def test_lambda():
    values = [ip.hm_intra_lambda(qp) for qp in range(52)]
    for qp, value in enumerate(values):
        if qp % 3 == 0:
            assert value == math.ldexp(0.57, (qp - 12) // 3), qp       # 0.57 * 2^k, exactly
        else:
            want = 0.57 * 2.0 ** ((qp - 12) / 3.0)
            assert abs(value - want) <= 1e-15 * want, qp
    assert all(a < b for a, b in zip(values, values[1:]))


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_constant_block(w):
    """A constant pattern and a candidate equal to that constant: every candidate predicts the same block, so the first-pass costs tie,
    the list is modes 0 .. K - 1 and 35 is appended.  Candidates under one scan then have equal J, and 35 (diagonal, as slot 0) loses the
    tie to slot 0.  At w >= 16 every scan is diagonal: all J are equal and slot 0 wins.  At w = 4 and 8 the listed modes 6 and 7 scan
    vertically (TComTU::getCoefScanIdx): they code the same residual into other bits, so their J equal each other, not slot 0's, and
    the winner is slot 0 unless theirs is strictly smaller, then slot 6.  D is one for all slots (no sign hiding: the scan does not
    shape the levels)."""
    k1 = ip.first_pass_list_size(w) + 1
    patterns = np.full((2, 2 * w + 1, 2 * w + 1), 90, np.uint8)
    targets = np.random.default_rng(w).integers(60, 120, (2, w, w), dtype=np.uint8)
    candidates = np.full((2, w, w), 90, np.uint8)
    r = ip.rd_pass(patterns, targets, candidates, QPS)
    assert np.array_equal(r['candidates'], np.tile(np.r_[np.arange(k1 - 1), CANDIDATE].astype(np.uint8), (2, 1)))
    assert r['costs'].shape[2] == k1
    distortion = ip.rd_pass(patterns, targets, candidates, QPS, lambdas=(0.,) * len(QPS))['costs']
    assert (distortion == distortion[:, :, :1]).all()                       # one prediction: one D
    diagonal = list(range(6)) + [k1 - 1] if w <= 8 else list(range(k1))
    vertical = [6, 7] if w <= 8 else []
    assert (r['costs'][:, :, diagonal] == r['costs'][:, :, :1]).all()
    if vertical:
        assert (r['costs'][:, :, vertical] == r['costs'][:, :, 6:7]).all()
        want = np.where(r['costs'][:, :, 6] < r['costs'][:, :, 0], 6, 0)
    else:
        want = np.zeros(r['slots'].shape, int)
    assert np.array_equal(r['slots'], want) and (r['modes'] == want).all() and (r['modes'] != CANDIDATE).all()


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_extreme_lambdas_and_perfect_candidate(w):
    n = 9
    patterns, targets, candidates = cases.seeded(w, n, seed=1700 + w)
    qps = (22, 37)
    plain = ip.rd_pass(patterns, targets, candidates, qps)
    slots = plain['candidates']
    # per-slot D and R from the costs at lambda 0 and at lambda 1 (both exact: integers below 2^53)
    zero = ip.rd_pass(patterns, targets, candidates, qps, lambdas=(0., 0.))
    one = ip.rd_pass(patterns, targets, candidates, qps, lambdas=(1., 1.))
    sse = zero['costs']
    with np.errstate(invalid='ignore'):                   # (inf - inf in the unused slots, masked below)
        bits = one['costs'] - zero['costs']
    used = np.broadcast_to(slots != UNUSED, sse.shape)
    assert np.isinf(sse[~used]).all()
    # lambda 0: the first slot of least sse_recon
    assert np.array_equal(zero['slots'], np.argmin(sse, axis=2)) and np.array_equal(zero['best_costs'], sse.min(axis=2))
    assert np.array_equal(zero['sses'].astype(np.float64), sse.min(axis=2))
    # a huge lambda: the first slot of least whole bits; D decides only among slots of zero bits, where lambda R is 0
    huge = ip.rd_pass(patterns, targets, candidates, qps, lambdas=(1e30, 1e30))
    for qi in range(2):
        for b in range(n):
            r = np.where(used[qi, b], bits[qi, b], np.inf)
            least = np.flatnonzero(r == r.min())
            want = least[np.argmin(sse[qi, b, least])] if r.min() == 0 else least[0]
            assert huge['slots'][qi, b] == want, (w, qi, b)
            assert (huge['rates'][qi, b] >> np.uint64(15)) == r.min()
    # a candidate equal to the target: 35 costs 0 and wins unless an earlier slot also reaches 0
    perfect = ip.rd_pass(patterns, targets, targets.copy(), qps)
    at = np.argmax(perfect['candidates'] == CANDIDATE, axis=1)
    assert (perfect['candidates'] == CANDIDATE).any(axis=1).all()
    for qi in range(2):
        for b in range(n):
            assert perfect['costs'][qi, b, at[b]] == 0. and perfect['best_costs'][qi, b] == 0.
            earlier = np.flatnonzero(perfect['costs'][qi, b, :at[b]] == 0.)
            assert perfect['slots'][qi, b] == (earlier[0] if earlier.size else at[b])
    assert (perfect['modes'] == CANDIDATE).any()


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_seeded_cases_decide_something(w):
    """The conditions of rd_pass_cases.assert_conditions on the blocks the GPU tests run, from the host twin; and the shares written
    into rd_pass_cases.py are the ones found."""
    n = 2 * cases.BLOCKS_PER_WORKGROUP[w] + 1
    result = ip.rd_pass(*cases.seeded(w, n), cases.QP_LISTS[4])
    cases.assert_conditions(result, "w %d" % w)
    found = cases.shares(result)
    print("w %d: %s" % (w, found))
    assert all(abs(found[key] - value) < 5e-5 for key, value in cases.SHARES_FOUND[w].items()), found


def test_argument_errors():
    L = _lib.lib()
    w, n = 8, 2
    patterns, targets, candidates = cases.seeded(w, n)
    qps = (ctypes.c_int * 2)(22, 37)
    out = np.zeros((2, n), np.uint8)

    def call(patterns_=patterns.ctypes.data, ph=17, pw=17, targets_=targets.ctypes.data, w_=w, n_=n, cand=candidates.ctypes.data, smoothing=0,
             qps_=qps, nq=2, lambdas=None, outs=(None, None, out.ctypes.data, None, None, None, None)):
        return L.pnn_rd_pass_host(patterns_, ph, pw, targets_, w_, n_, cand, smoothing, qps_, nq, lambdas, 0, *outs)

    assert call() == 0
    assert call(n_=0, patterns_=None, targets_=None, cand=None) == 0
    for bad in (dict(w_=12), dict(ph=8), dict(pw=18), dict(n_=-1), dict(patterns_=None), dict(targets_=None), dict(cand=None),
                dict(smoothing=3), dict(nq=0), dict(nq=9), dict(qps_=(ctypes.c_int * 2)(22, 52)), dict(qps_=None), dict(outs=(None,) * 7),
                dict(lambdas=(ctypes.c_double * 2)(1., -1.)), dict(lambdas=(ctypes.c_double * 2)(float('nan'), 1.)),
                dict(lambdas=(ctypes.c_double * 2)(1., float('inf')))):
        before = out.copy()
        assert call(**bad) == -1, bad
        assert np.array_equal(out, before)
    for kwargs, error in ((dict(qps=()), ValueError), (dict(qps=(22,), lambdas=(1., 2.)), ValueError), (dict(qps=(22,), lambdas=(-1.,)), ValueError),
                          (dict(qps=(22,), reference_smoothing=3), ValueError)):
        with pytest.raises(error):
            ip.rd_pass(patterns, targets, candidates, **kwargs)
    with pytest.raises(ValueError):
        ip.rd_pass(patterns, targets, candidates[:1], (22,))
    with pytest.raises(TypeError):
        ip.rd_pass(patterns, targets, candidates.astype(np.int32), (22,))
    assert L.pnn_rd_pass_workspace_bytes(12, 1, 1) == 0 and L.pnn_rd_pass_workspace_bytes(8, 1, 9) == 0
    assert L.pnn_rd_pass_workspace_bytes(8, 3, 2) >= 3 * 9 * (2 * 64 + 1 + 2 * 12) + 3 * 8


def test_sanitizer_program(tmp_path):
    """tests/sanitize_rd_pass.cpp, a stand-alone program over the new host entries, under AddressSanitizer + UBSan"""
    csrc = os.path.join(ROOT, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    exe = str(tmp_path / "sanitize_rd_pass")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                        "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "sanitize_rd_pass.cpp"),
                        os.path.join(csrc, "pnn_rd_pass.cpp"), os.path.join(csrc, "pnn_hevc_intra.cpp"), os.path.join(csrc, "pnn_trquant.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_rd_pass: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
