"""CPU tests of HM's sign-data hiding in the transform-coding column (include/pnn_hip.h, "sign-data hiding"): the host twin
(pnn_sign_hide_unit_host, pnn_trquant_sdh_host, pnn_trquant_stages_sdh_host, pnn_cabac_rate_levels_sdh_host of csrc/pnn_trquant.cpp)
against recorded calls of HM-16.15's own signBitHidingHDQ (tests/golden/hm_sign_hiding.npz, made by
tests/golden/make_hm_sign_hiding.py), against the Python restatement of tests/sign_hiding_cases.py, on properties of the final levels, on
a worked answer, on bad arguments and under AddressSanitizer + UBSan as a stand-alone program.  Every comparison is integer equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cabac_rate_cases as cabac
from tests import sign_hiding_cases as model
from tests import trquant_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PNN_E_ARG = -1
INT_KEYS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels')


# ---- 1. pinned to HM ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "hm_sign_hiding.npz"))


@pytest.mark.parametrize("t", cabac.SIZES)
def test_hm_sign_bit_hiding(golden, t):
    """Every record of HM's own signBitHidingHDQ: the host entry gives HM's levels, and so does the restatement; over the records of a
    size every row of the cost table is met and every allowed row wins (so the fixture shows what it is meant to show)."""
    taken = {}
    for scan in cabac.scans_of(t):
        coef, before, delta_u, after = (golden['%s_%d_%d' % (name, t, scan)] for name in ('coef', 'before', 'delta_u', 'after'))
        assert coef.shape[0] >= 12 and (after != before).any()
        for k in range(coef.shape[0]):
            kept = before[k].copy()
            assert np.array_equal(ip.sign_hide_levels(before[k], coef[k], delta_u[k], scan), after[k]), (t, scan, k)
            assert np.array_equal(before[k], kept)                          # the Python entry leaves its input alone
            assert np.array_equal(model.hide(before[k], coef[k], delta_u[k], scan, taken), after[k]), (t, scan, k)
    for row in model.ROWS:
        assert taken.get(row, 0) > 0, (t, row)
        assert row.endswith('forbidden') or taken.get('won:' + row, 0) > 0, (t, row)


# ---- 2. the restatement -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", trquant_cases.WIDTHS)
def test_host_twin_equals_restatement(w):
    """Every stage (the remainders and the levels after hiding among them), the counts, the reconstruction and the rate, at QPs 0, 22, 37
    and 51 under every scan the size allows, on dense, smooth and extreme pairs."""
    t = min(w, 32)
    n = 6 if w <= 16 else 3
    predictions, targets = model.dense_pairs(w, n, 700 + w)
    extremes, smooth = trquant_cases.extreme_pairs(w), trquant_cases.smooth_pairs(w, 1, 3 + w)
    predictions[0], targets[0] = extremes[0][0], extremes[1][0]
    predictions[1], targets[1] = extremes[0][2], extremes[1][2]
    predictions[2], targets[2] = smooth[0][0], smooth[1][0]
    mode_of_scan = {cabac.DIAG: 0, cabac.HOR: 26, cabac.VER: 10}
    for scan in cabac.scans_of(t):
        modes = np.full(n, mode_of_scan[scan], np.uint8)
        got = ip.transform_code(predictions, targets, model.QPS, keep_reconstructions=True, modes=modes, rate=True, sign_data_hiding=True)
        for b in range(n):
            for qi, qp in enumerate(model.QPS):
                want = model.stages(predictions[b], targets[b], qp, scan)
                twin = ip.transform_stages(predictions[b], targets[b], qp, sign_data_hiding=True, scan=scan)
                assert set(twin) == {'coeffs', 'levels', 'delta_u', 'levels_hidden', 'dequant', 'residual'}
                for key, stage in twin.items():
                    assert stage.dtype == np.int32 and np.array_equal(stage, want[key]), (w, scan, b, qp, key)
                assert got['sses_recon'][qi, b] == ((want['reconstruction'] - targets[b].astype(np.int64)) ** 2).sum()
                assert got['nb_nonzero_levels'][qi, b] == np.count_nonzero(want['levels_hidden'])
                assert got['sum_abs_levels'][qi, b] == want['magnitudes'].sum()                 # HM's uiAbsSum: before the hiding
                assert np.array_equal(got['reconstructions_uint8'][qi, b], want['reconstruction'])
                assert got['rate_bits'][qi, b] == want['rate'] / 32768., (w, scan, b, qp)
                units = model.units_of(w)
                assert want['rate'] == sum(ip.cabac_rate_of_levels(twin['levels_hidden'][u], scan, qp, sign_data_hiding=True) for u in units)


@pytest.mark.parametrize("w", trquant_cases.WIDTHS)
def test_flag_off_is_the_entry_without_it(w):
    """Flag 0: the bytes of pnn_trquant_rate_host, pnn_trquant_host, pnn_trquant_stages_host and pnn_cabac_rate_levels_host."""
    L = _lib.lib()
    n, qps = 5, (0, 22, 51)
    predictions, targets = trquant_cases.mixed_pairs(w, 6, 900 + w)
    predictions, targets = predictions[:n], targets[:n]
    modes = np.array([26, 10, 0, 30, 6], np.uint8)
    c_qps = (ctypes.c_int * 3)(*qps)
    specs = [(np.uint32, (3, n))] * 3 + [(np.uint8, (3, n, w, w)), (np.uint64, (3, n))]
    for mode_array in (None, modes):
        old, new = ([np.full(s, 0xA5, t) for t, s in specs] for _ in range(2))
        front = (predictions.ctypes.data, targets.ctypes.data, w, n, None if mode_array is None else mode_array.ctypes.data, c_qps, 3)
        assert L.pnn_trquant_rate_host(*front, *[o.ctypes.data for o in old]) == 0
        assert L.pnn_trquant_sdh_host(*front, *[o.ctypes.data for o in new], 0) == 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(old, new))
    plain = ip.transform_code(predictions, targets, qps, keep_reconstructions=True)
    off = ip.transform_code(predictions, targets, qps, keep_reconstructions=True, sign_data_hiding=False)
    assert set(plain) == set(off) and all(np.array_equal(plain[k], off[k]) for k in plain)
    assert all(np.array_equal(plain[k], new[i]) for i, k in enumerate(INT_KEYS))
    t = min(w, 32)
    for b in range(n):
        old = ip.transform_stages(predictions[b], targets[b], 22)
        stages = {name: np.zeros((w, w), np.int32) for name in ('coeffs', 'levels', 'delta_u', 'levels_hidden', 'dequant', 'residual')}
        assert L.pnn_trquant_stages_sdh_host(predictions[b].ctypes.data, targets[b].ctypes.data, w, 22, 0, 0,
                                             *[a.ctypes.data for a in stages.values()]) == 0
        assert set(old) == {'coeffs', 'levels', 'dequant', 'residual'} and all(np.array_equal(old[k], stages[k]) for k in old)
        assert np.array_equal(stages['levels_hidden'], stages['levels'])
        unit = old['levels'][:t, :t]
        assert ip.cabac_rate_of_levels(unit, 0, 22, sign_data_hiding=False) == ip.cabac_rate_of_levels(unit, 0, 22) == cabac.rate(unit, 0, 22)


# ---- 3. properties of the final levels ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", trquant_cases.WIDTHS)
def test_properties_of_the_hidden_levels(w):
    """In the host twin's final levels: every group whose first and last nonzero positions are at least 4 apart has the sign of its
    first level in the parity of its sum (what a decoder relies on); per group at most one level differs from the quantiser's, by
    exactly 1; a unit without a participating group is unchanged; and on those levels the rate with hiding is the rate without it minus
    one bypass bin per qualifying group."""
    t = min(w, 32)
    predictions, targets = model.dense_pairs(w, 4, 1100 + w)
    sparse = trquant_cases.smooth_pairs(w, 2, 1200 + w)
    predictions[2:], targets[2:] = sparse[0], sparse[1]
    groups = changed_groups = untouched_units = 0
    for scan in cabac.scans_of(t):
        order = cabac.grouped_scan(t, scan)
        for b in range(4):
            for qp in (0, 17, 27, 37, 45):
                s = ip.transform_stages(predictions[b], targets[b], qp, sign_data_hiding=True, scan=scan)
                for unit in model.units_of(w):
                    before, after = s['levels'][unit], s['levels_hidden'][unit]
                    participating = 0
                    for c in range(t * t // 16):
                        where = order[16 * c:16 * c + 16]
                        old = [int(before[y, x]) for x, y in where]
                        new = [int(after[y, x]) for x, y in where]
                        first, last = model.group_span(new)
                        groups += 1
                        if last - first >= model.THRESHOLD:
                            assert (0 if new[first] > 0 else 1) == sum(new[first:last + 1]) & 1, (w, scan, b, qp, c)
                        differing = [abs(o - v) for o, v in zip(old, new) if o != v]
                        assert differing in ([], [1]), (w, scan, b, qp, c)
                        changed_groups += len(differing)
                        first, last = model.group_span(old)
                        participating += last - first >= model.THRESHOLD
                        assert differing == [] or last - first >= model.THRESHOLD
                    if not participating:
                        untouched_units += 1
                        assert np.array_equal(before, after)
                    plain = ip.cabac_rate_of_levels(after, scan, qp)
                    hidden = ip.cabac_rate_of_levels(after, scan, qp, sign_data_hiding=True)
                    assert hidden == plain - cabac.BYPASS * model.qualifying_groups(after, scan)
    assert changed_groups * 8 >= groups and untouched_units > 0            # both kinds of unit were met


# ---- 4. a worked answer -------------------------------------------------------------------------------------------------------------

def test_worked_4x4_unit():
    """One 4 x 4 unit under the diagonal scan, whose first six positions are (x, y) = (0,0) (0,1) (1,0) (0,2) (1,1) (2,0).
        n        0     1     2     3     4     5     6 .. 15
        level    2    -1     0     1     0     3     0
        C      105   -40    12    44   -20   150    +-3 (small, never a candidate)
        deltaU  10   -30   120   -50    60     5
    first = 0, last = 5: 5 >= 4, the group takes part.  signbit = 0 (the level at n = 0 is positive); the sum 2 - 1 + 1 + 3 = 5 is odd:
    parity 1 != 0, a level must change.  The unit's only group is the last one: candidates n = 5 down to 0.
        n = 5: nonzero, deltaU 5 > 0       -> cost  -5, +1
        n = 4: zero, not below first       -> cost -60, +1
        n = 3: nonzero, deltaU -50 <= 0    -> cost -50, -1   (not n == first: allowed although |level| == 1)
        n = 2: zero, not below first       -> cost -120, +1  <- the smallest
        n = 1: nonzero, deltaU -30 <= 0    -> cost -30, -1
        n = 0: nonzero, deltaU 10 > 0      -> cost -10, +1
    The winner is n = 2, a zero level with C = 12 >= 0: it becomes +1.  New sum 6: even = signbit.  With C = -12 there it becomes -1 (sum
    4, even as well).  Rate: last - first = 5 >= 4 in the final levels, so one sign bin (32768) is not coded.
    Then the same levels with deltaU 120 -> -120 at n = 2: the smallest cost is -60 at n = 4, C = -20 < 0: it becomes -1 (sum 4)."""
    xy = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))
    assert cabac.grouped_scan(4, cabac.DIAG)[:6] == list(xy)
    levels, coeffs, delta_u = np.zeros((4, 4), np.int32), np.full((4, 4), 3, np.int32), np.zeros((4, 4), np.int32)
    coeffs[2:, 2:] = -3
    for (x, y), lv, c, d in zip(xy, (2, -1, 0, 1, 0, 3), (105, -40, 12, 44, -20, 150), (10, -30, 120, -50, 60, 5)):
        levels[y, x], coeffs[y, x], delta_u[y, x] = lv, c, d
    want = levels.copy()
    want[0, 1] = 1                                                           # (x, y) = (1, 0)
    for scan in (0, 'diagonal'):
        assert np.array_equal(ip.sign_hide_levels(levels, coeffs, delta_u, scan), want)
    assert np.array_equal(model.hide(levels, coeffs, delta_u, 0), want)
    negative = coeffs.copy()
    negative[0, 1] = -12
    want[0, 1] = -1
    assert np.array_equal(ip.sign_hide_levels(levels, negative, delta_u, 0), want)
    assert ip.cabac_rate_of_levels(want, 0, 22) - ip.cabac_rate_of_levels(want, 0, 22, sign_data_hiding=True) == 32768
    delta_u[0, 1] = -120
    want = levels.copy()
    want[1, 1] = -1
    assert np.array_equal(ip.sign_hide_levels(levels, coeffs, delta_u, 0), want)
    # three levels within four positions: first = 0, last = 3 -- the group does not take part, whatever the parity; no sign is hidden
    near = np.zeros((4, 4), np.int32)
    near[0, 0], near[1, 0], near[2, 0] = 2, -1, 2
    assert np.array_equal(ip.sign_hide_levels(near, coeffs, delta_u, 0), near)
    assert ip.cabac_rate_of_levels(near, 0, 22) == ip.cabac_rate_of_levels(near, 0, 22, sign_data_hiding=True)


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------------

def test_argument_errors():
    L = _lib.lib()
    predictions, targets = trquant_cases.random_pairs(8, 3, 5)
    qps = (ctypes.c_int * 1)(22)
    rate, sse = np.zeros((1, 3), np.uint64), np.zeros((1, 3), np.uint32)
    good, bad = np.array([0, 34, 26], np.uint8), np.array([0, 35, 26], np.uint8)
    call = lambda modes, sse_out, rate_out, flag, width=8: L.pnn_trquant_sdh_host(  # noqa: E731
        predictions.ctypes.data, targets.ctypes.data, width, 3, None if modes is None else modes.ctypes.data, qps, 1,
        None if sse_out is None else sse_out.ctypes.data, None, None, None, None if rate_out is None else rate_out.ctypes.data, flag)
    assert call(good, sse, rate, 1) == 0 and rate.all()
    assert call(good, sse, None, 1) == 0                                      # with the flag the scan shapes the levels: modes without a rate
    assert call(good, sse, None, 0) == PNN_E_ARG                              # without it only the rate reads them
    assert call(bad, sse, None, 1) == PNN_E_ARG and call(None, None, None, 1) == PNN_E_ARG and call(None, sse, None, 1, width=12) == PNN_E_ARG
    assert ip.transform_code(predictions, targets, (22,), modes=good, sign_data_hiding=True)['sses_recon'].shape == (1, 3)
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (22,), modes=bad, sign_data_hiding=True)
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (22,), modes=good)             # still refused without the flag
    unit = np.ones((16, 16), np.int32)
    one = np.ones((4, 4), np.int32)
    for args in ((unit, unit, unit, 1), (unit, unit, unit, 3), (np.ones((12, 12), np.int32),) * 3 + (0,), (one, one, unit, 0),
                 (np.full((4, 4), 32768), one, one, 0), (one.astype(np.float64), one, one, 0), (one, one, np.full((4, 4), -2 ** 31), 0)):
        with pytest.raises(ValueError):
            ip.sign_hide_levels(*args)
    level = np.ones((4, 4), np.int32)
    assert L.pnn_sign_hide_unit_host(None, level.ctypes.data, level.ctypes.data, 4, 0) == PNN_E_ARG
    assert L.pnn_sign_hide_unit_host(level.ctypes.data, level.ctypes.data, level.ctypes.data, 64, 0) == PNN_E_ARG
    assert (level == 1).all()
    with pytest.raises(ValueError):
        ip.transform_stages(predictions[0], targets[0], 22, sign_data_hiding=True, scan=3)
    with pytest.raises(ValueError):
        ip.transform_stages(np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8), 22, sign_data_hiding=True, scan=1)
    with pytest.raises(ValueError):
        ip.cabac_rate_of_levels(unit, 1, 22, sign_data_hiding=True)
    assert L.pnn_trquant_sdh_device(None, 8, None, None, 2, None, qps, 1, None, None, None, None, None, 1, None) == PNN_E_ARG
    # transform_sign_hiding without QPs: refused before anything touches the GPU (no predictor is ever looked at)
    channels = np.zeros((1, 64, 64, 1), np.uint8)
    where = np.zeros(1, np.int64)
    with pytest.raises(ValueError, match="transform_sign_hiding"):
        evaluation.score_masks_from_pictures(channels, 8, where, where, None, 0., ((0, 0),), transform_sign_hiding=True)
    with pytest.raises(ValueError, match="transform_sign_hiding"):
        evaluation.score_masks_from_picture_pairs(np.zeros((1, 64, 64, 2), np.uint8), 8, where, where, None, 0., ((0, 0),),
                                                  transform_sign_hiding=True)


# ---- 6. the sanitizer program -------------------------------------------------------------------------------------------------------

def test_sanitizer_program(tmp_path):
    """tests/sanitize_sign_hiding.cpp, a stand-alone program over the new host entries, under AddressSanitizer + UBSan"""
    csrc = os.path.join(ROOT, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    exe = str(tmp_path / "sanitize_sign_hiding")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                        "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "sanitize_sign_hiding.cpp"),
                        os.path.join(csrc, "pnn_trquant.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_sign_hiding: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
