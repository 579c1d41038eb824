"""CPU tests of HM's reference-sample smoothing in the host twin: pnn_hevc_mode_uses_smoothing, pnn_hevc_smoothed_reference_host,
pnn_hevc_intra_predict_hm, pnn_hevc_mode_hads_hm_host and their Python faces.

The yardstick (tests/hevc_smoothing_cases.py) is a numpy restatement of the filter composed with untouched code: the UNSMOOTHED
predictor and the UNSMOOTHED first-pass costs, run on a pattern whose first row and column were smoothed in numpy, per mode as the
literally written decision table says.  No reference-held numeric output exists for this filter -- the reference's extracted
predictor lacks it and HM's copy cannot be called outside the codec -- so the restatement plus the known answers below are the
evidence.  Zero tolerance throughout: everything is an integer."""
import os
import subprocess

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import hevc_smoothing_cases as cases
from tests.hevc_smoothing_cases import SMOOTHED, WIDTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hevc_intra_ref.npz")
PNN_E_ARG = -1                       # include/pnn_hip.h


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLD)


def fixture_patterns(ref, w):
    """[(mask, patterns [n, h, w'])] of the reference's recordings: every mask of the fixture."""
    return [(m, ref["mode_w%d_m%dx%d_patterns" % (w, m[0], m[1])]) for m in cases.masks(w)]


def twin_predictions(pattern, w, smoothing):
    return np.array([ip.predict_via_hevc_mode(np.ascontiguousarray(pattern[..., None]), w, m, smoothing=smoothing)[..., 0] for m in range(35)])


def test_decision_table():
    L = _lib.lib()
    for w in WIDTHS:
        assert {m for m in range(35) if L.pnn_hevc_mode_uses_smoothing(w, m) == 1} == SMOOTHED[w], w
        assert {m for m in range(35) if L.pnn_hevc_mode_uses_smoothing(w, m) == 0} == cases.ALL - SMOOTHED[w], w
        assert {m for m in range(35) if ip.mode_uses_smoothing(w, m)} == SMOOTHED[w], w
        assert not SMOOTHED[w] & {1, 10, 26}                                 # DC and the pure directions never smooth


@pytest.mark.parametrize("w", WIDTHS)
def test_smoothed_line_equals_the_definition(ref, w):
    for mask, patterns in fixture_patterns(ref, w):
        assert patterns.shape[1:] == (2 * w + 1 - mask[1], 2 * w + 1 - mask[0])
        for pattern in patterns:
            plain = cases.line_of(pattern, w)
            got, strong = ip.smoothed_reference(pattern, w, 0)
            assert got.dtype == np.uint8 and np.array_equal(got, plain) and not strong, (w, mask)       # 0: the padded line
            for smoothing in (1, 2):
                got, strong = ip.smoothed_reference(pattern[..., None], w, smoothing)
                want, want_strong = cases.smooth(plain, w, smoothing)
                if w in (4, 64):                                             # no mode smooths: the entries keep the padded line
                    want, want_strong = plain, False
                assert np.array_equal(got, want) and strong == want_strong, (w, mask, smoothing)
                assert got[0] == plain[0] and got[-1] == plain[-1]           # the ends are never changed


@pytest.mark.parametrize("w", WIDTHS)
def test_predictions_equal_the_unsmoothed_predictor_on_smoothed_patterns(ref, w):
    differs = False
    for mask, patterns in fixture_patterns(ref, w):
        for pattern in patterns:
            plain = twin_predictions(pattern, w, 0)
            assert np.array_equal(plain, cases.model_predictions(pattern, w, 0))
            for smoothing in (1, 2):
                got = twin_predictions(pattern, w, smoothing)
                assert got.dtype == np.uint8 and np.array_equal(got, cases.model_predictions(pattern, w, smoothing)), (w, mask, smoothing)
                for m in cases.ALL - SMOOTHED[w]:                            # unsmoothed modes: the bits of smoothing = 0
                    assert np.array_equal(got[m], plain[m]), (w, mask, m)
                differs = differs or any((got[m] != plain[m]).any() for m in SMOOTHED[w])
    assert differs == bool(SMOOTHED[w])


@pytest.mark.parametrize("w", WIDTHS)
def test_costs_and_list_equal_the_merged_unsmoothed_costs(ref, w):
    rng = np.random.RandomState(40 + w)
    for mask, patterns in fixture_patterns(ref, w):
        n = patterns.shape[0]
        targets = rng.randint(0, 256, (n, w, w)).astype(np.uint8)
        candidate = np.clip(targets.astype(np.int64) + rng.randint(-20, 21, targets.shape), 0, 255).astype(np.uint8)
        plain = ip.mode_hads_host(patterns, targets, w, candidate)
        results = {}
        for smoothing in (0, 1, 2):
            for cand in (candidate, None):
                got = ip.mode_hads_host(patterns, targets, w, cand, smoothing=smoothing)
                want = cases.model_hads(patterns, targets, w, smoothing, cand)
                for key in want:
                    assert (got[key] is None and want[key] is None) or \
                        (got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes()), (w, mask, smoothing, key)
            results[smoothing] = ip.mode_hads_host(patterns, targets, w, candidate, smoothing=smoothing)
        for key in plain:                                                    # 0 through the new body: the old entry's bits
            assert results[0][key].tobytes() == plain[key].tobytes(), key
        keep = sorted(cases.ALL - SMOOTHED[w])
        for smoothing in (1, 2):
            assert np.array_equal(results[smoothing]['hads_modes'][:, keep], plain['hads_modes'][:, keep])    # equal in every unsmoothed mode
            if w in (4, 64):                                                 # ... and there, in everything
                assert all(results[smoothing][key].tobytes() == plain[key].tobytes() for key in plain)
        if w in (8, 16):                                                     # no strong filter below 32: 1 and 2 agree
            assert all(results[1][key].tobytes() == results[2][key].tobytes() for key in plain)


@pytest.mark.parametrize("w", (8, 16, 32))
def test_smoothed_costs_differ_on_random_patterns(w):
    rng = np.random.RandomState(60 + w)
    patterns = rng.randint(0, 256, (4, 2 * w + 1, 2 * w + 1)).astype(np.uint8)
    targets = rng.randint(0, 256, (4, w, w)).astype(np.uint8)
    plain = ip.mode_hads_host(patterns, targets, w)['hads_modes']
    for smoothing in (1, 2):
        got = ip.mode_hads_host(patterns, targets, w, smoothing=smoothing)['hads_modes']
        assert (got[:, sorted(SMOOTHED[w])] != plain[:, sorted(SMOOTHED[w])]).any()
        assert np.array_equal(got[:, sorted(cases.ALL - SMOOTHED[w])], plain[:, sorted(cases.ALL - SMOOTHED[w])])


@pytest.mark.parametrize("w", (8, 16, 32))
def test_known_answers(w):
    n = 4 * w + 1
    constant = cases.pattern_of_line(np.full(n, 97, np.int64), w)
    ramp_line = 20 + np.arange(n, dtype=np.int64)                             # a linear integer ramp along the whole line, corner included
    ramp = cases.pattern_of_line(ramp_line, w)
    bent = ramp_line.copy()
    bent[2 * w] += 40                                                        # a corner that sticks out of its two neighbours
    for smoothing in (1, 2):
        got, _ = ip.smoothed_reference(constant, w, smoothing)
        assert (got == 97).all()                                             # a constant line stays constant
        got, strong = ip.smoothed_reference(ramp, w, smoothing)
        assert strong == (w == 32 and smoothing == 2)                        # (a ramp is flat at its anchors)
        assert np.array_equal(got, ramp_line)                                # a linear ramp is a fixed point of both filters, ends included
        got, strong = ip.smoothed_reference(cases.pattern_of_line(bent, w), w, smoothing)
        assert got[0] == bent[0] and got[-1] == bent[-1]
        if strong:
            assert got[2 * w] == bent[2 * w]                                 # the strong filter copies the corner
        else:
            assert got[2 * w] == bent[2 * w] - 20                            # [1 2 1]: (a - 1 + 2 (a + 40) + a + 1 + 2) >> 2 = a + 20
    line = np.full(129, 100, np.int64)
    line[64] = 102                                                           # flat enough for strong (|100 + 102 - 200| = 2), corner off its neighbours
    got, strong = ip.smoothed_reference(cases.pattern_of_line(line, 32), 32, 2)
    assert strong and got[64] == 102
    got, strong = ip.smoothed_reference(cases.pattern_of_line(line, 32), 32, 1)
    assert not strong and got[64] == 101                                     # (100 + 204 + 100 + 2) >> 2


def test_strong_smoothing_on_crafted_lines():
    w = 32
    blocks = cases.crafted_blocks()
    assert [name for name, _, _ in blocks] == ['both_flat', 'only_above_flat', 'only_left_flat', 'neither_flat', 'difference_7',
                                               'difference_8', 'masked_flat']
    rng = np.random.RandomState(9)
    for name, pattern, want_strong in blocks:
        plain = cases.line_of(pattern, w)
        weak, _ = cases.smooth(plain, w, 1)
        model, model_strong = cases.smooth(plain, w, 2)
        assert model_strong == want_strong, name
        if name == 'difference_7':
            assert abs(plain[0] + plain[64] - 2 * plain[32]) == 7 and (plain[0] + plain[64]) % 2 == 1
        if name == 'difference_8':
            assert abs(plain[0] + plain[64] - 2 * plain[32]) == 8 and (plain[0] + plain[64]) % 2 == 0
        if name == 'masked_flat':                                            # the decision rests on padded samples
            assert pattern.shape == (w + 1, w + 1) and plain[0] == plain[32] and plain[128] == plain[96]
        if want_strong:
            assert (model != weak).any(), name                               # a "never strong" implementation cannot pass below
        got1, strong1 = ip.smoothed_reference(pattern, w, 1)
        got2, strong2 = ip.smoothed_reference(pattern, w, 2)
        assert not strong1 and np.array_equal(got1, weak), name
        assert strong2 == want_strong and np.array_equal(got2, model), name
        if not want_strong:
            assert np.array_equal(got2, got1), name                          # 2 equals 1 on the non-strong blocks
        targets = rng.randint(0, 256, (1, w, w)).astype(np.uint8)
        for smoothing in (1, 2):
            assert np.array_equal(twin_predictions(pattern, w, smoothing), cases.model_predictions(pattern, w, smoothing)), (name, smoothing)
            got = ip.mode_hads_host(pattern[None], targets, w, smoothing=smoothing)
            want = cases.model_hads(pattern[None], targets, w, smoothing)
            assert all(want[k] is None or got[k].tobytes() == want[k].tobytes() for k in want), (name, smoothing)
        same = np.array_equal(twin_predictions(pattern, w, 1), twin_predictions(pattern, w, 2))
        assert same == (not want_strong), name                               # the strong decision reaches the predictions


def test_bad_arguments_are_refused(capfd):
    L = _lib.lib()
    w = 8
    pattern = np.zeros((2 * w + 1, 2 * w + 1), np.uint8)
    out = np.full((w, w), 0xA5, np.uint8)
    line = np.full(4 * w + 1, 0xA5, np.uint8)
    targets = np.zeros((1, w, w), np.uint8)
    hads = np.full((1, 35), 0xA5A5A5A5, np.uint32)
    p, o = pattern.ctypes.data_as(_lib.u8p), out.ctypes.data_as(_lib.u8p)

    def refused(rc):
        err = capfd.readouterr().err
        return rc == PNN_E_ARG and len(err.strip()) > 0 and (out == 0xA5).all() and (line == 0xA5).all() and (hads == 0xA5A5A5A5).all()

    for smoothing in (-1, 3):
        assert refused(L.pnn_hevc_intra_predict_hm(p, 2 * w + 1, 2 * w + 1, w, 0, smoothing, o))
        assert refused(L.pnn_hevc_smoothed_reference_host(pattern.ctypes.data, 2 * w + 1, 2 * w + 1, w, smoothing, line.ctypes.data, None))
        assert refused(L.pnn_hevc_mode_hads_hm_host(pattern.ctypes.data, 2 * w + 1, 2 * w + 1, targets.ctypes.data, w, 1, None, smoothing,
                                                    hads.ctypes.data, None, None, None))
        for call in (lambda: ip.predict_via_hevc_mode(pattern[..., None], w, 0, smoothing=smoothing),
                     lambda: ip.smoothed_reference(pattern, w, smoothing),
                     lambda: ip.mode_hads_host(pattern[None], targets, w, smoothing=smoothing)):
            with pytest.raises(ValueError):
                call()
    assert refused(L.pnn_hevc_intra_predict_hm(p, 2 * w + 1, 2 * w + 1, w, 35, 2, o))          # mode 35
    assert refused(L.pnn_hevc_mode_uses_smoothing(w, 35)) and refused(L.pnn_hevc_mode_uses_smoothing(w, -1))
    assert refused(L.pnn_hevc_intra_predict_hm(p, 2 * w + 1, 2 * w + 1, 12, 0, 2, o))         # width 12
    assert refused(L.pnn_hevc_mode_uses_smoothing(12, 0))
    assert refused(L.pnn_hevc_smoothed_reference_host(pattern.ctypes.data, 2 * w + 1, 2 * w + 1, 12, 2, line.ctypes.data, None))
    assert refused(L.pnn_hevc_smoothed_reference_host(pattern.ctypes.data, w, 2 * w + 1, w, 2, line.ctypes.data, None))
    assert refused(L.pnn_hevc_smoothed_reference_host(None, 2 * w + 1, 2 * w + 1, w, 2, line.ctypes.data, None))
    assert L.pnn_hevc_mode_hads_hm_host(pattern.ctypes.data, 2 * w + 1, 2 * w + 1, targets.ctypes.data, 12, 1, None, 2, hads.ctypes.data,
                                        None, None, None) == PNN_E_ARG and (hads == 0xA5A5A5A5).all()
    with pytest.raises(ValueError):
        ip.mode_uses_smoothing(12, 0)
    with pytest.raises(ValueError):
        ip.mode_uses_smoothing(8, 35)
    # the same calls with good arguments go through
    assert L.pnn_hevc_intra_predict_hm(p, 2 * w + 1, 2 * w + 1, w, 34, 2, o) == 0 and not out.any()
    assert L.pnn_hevc_smoothed_reference_host(pattern.ctypes.data, w + 1, w + 1, w, 2, line.ctypes.data, None) == 0 and not line.any()


def test_host_twin_under_sanitizers(tmp_path):
    """tests/sanitize_hevc_smoothing.cpp (its own main) and the host twin, compiled together under AddressSanitizer + UBSan and run as a
    child process: the four host functions on the crafted blocks and on the smallest pattern sides.  Any report aborts the program."""
    csrc = os.path.join(ROOT, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    exe = str(tmp_path / "sanitize_hevc_smoothing")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                        "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize_hevc_smoothing.cpp"),
                        os.path.join(csrc, "pnn_hevc_intra.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_hevc_smoothing: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
