"""Layout and cases of tests/golden/hm_rdoq.npz (made by tests/golden/make_hm_rdoq.py from HM-16.15's own transformNxN with RDOQ on),
shared by the generator, tests/test_hm_rdoq.py and tests/test_gpu_rdoq.py.

Per unit size T the fixture holds the pairs (pair_predictions_T, pair_targets_T uint8 [n, T, T], pair_modes_T uint8 [n]) and per case
(case_pair_T, case_qp_T, case_factor_T -- index into LAMBDA_FACTORS --, case_sdh_T, case_depth_T -- the transform depth, 0 or 1 --):
case_lambda_T (the lambda HM's quantiser was given, as the 64-bit pattern of the double), case_scan_T, case_abs_sum_T (uiAbsSum),
case_bits_T (m_fracBits of codeCoeffNxN on the levels), case_cbf_ctx_T (getCtxQtCbf), case_levels_T and case_residual_T int16 [T, T]
(invTransformNxN).  est_bits_T int32 [len(QPS), 184]: the tables estBit filled at each QP in the layout of pnn_rdoq_est_bits_host,
-1 where HM fills nothing at that size.

The cases: the pairs of trquant_cases.mixed_pairs (extremes, a zero residual, random and smooth ones) and four of a flat prediction
under small noise (coefficients near the decision thresholds), at T >= 8 two pairs built backwards from level patterns
(backwards_patterns), with modes that give every scan,
each at QPs 0, 22, 37, 51 under lambda = hm_intra_lambda(QP) times 1, 0.25 and 4, SignDataHidingEnabledFlag off and on, at transform
depth 0; and under the plain lambda at depth 1.  Last, per T, one TIE case: a pair at a QP of TIE_QPS under a lambda built so that the costs of the
two candidate levels at the unit's last position are equal up to rounding (tie_lambda): its levels differ under a fused multiply-add.

EDGES (conditions on HM's recorded output; the generator fails unless every wanted one is reached at every T where it can exist; what
can be told from HM's levels, the coefficients -- this project's forward transform, pinned to HM's elsewhere -- and the scan):
  max_minus_1      a level equal to uiMaxAbsLevel - 1 >= 1
  zero_from_1 / _2 a level 0 where uiMaxAbsLevel was 1 / 2
  level_ge_3       a level of magnitude >= 3
  all_zero         every level 0 (iBestLastIdxP1 == 0 or every level dropped) although some uiMaxAbsLevel > 0
  last_moved       the last nonzero level lies below the last position with uiMaxAbsLevel > 0
  group_emptied    a coefficient group below the last coded one without a level although it held uiMaxAbsLevel > 0   (told from the output: wanted at
                   T >= 16; the walk's own group_zeroed is wanted from T = 8 on)
  nine_in_group    nine or more levels in one group (c1Idx >= 8);  two_above_one: two levels > 1 in one group (c2Idx >= 1)
  cbf_ctx_0 / _1   both cbf contexts;  scan_0 / _1 / _2: the three scans (T <= 8)
  hide_up / hide_down / hide_zero_up   RDOQ's hiding changed a nonzero level by +1 / by -1 / a zero level to +-1 (flag on against off)
  abs_sum_lt_2     a unit with uiAbsSum < 2 and the flag on
  lambda_moves     the levels differ between two of the three lambdas
And, from the walk's own state (the restatement `walk` below, which must equal HM's levels on the case; WALK_EDGES): group_zeroed
(the d64CostZeroCG test taken on a group with levels; T >= 8), nnz_before_pos0_is_0 (T >= 8), found_last, rice_4, escape, forbidden_met,
bonus_met, nothing_coded; and fma_differs: a unit whose levels differ when dErr^2 * errScale + lambda * rate is rounded once."""
import os

import numpy as np

from tests import cabac_rate_cases as cabac
from tests import trquant_cases as tq

SIZES = (4, 8, 16, 32)
QPS = (0, 22, 37, 51)
LAMBDA_FACTORS = (1., 0.25, 4.)
MODES = (0, 26, 10, 1, 22, 14, 30, 6)                    # diagonal, horizontal and vertical scans at T = 4 and 8
NB_PAIRS = {4: 20, 8: 18, 16: 12, 32: 12}
NB_BACKWARDS = {4: 0, 8: 2, 16: 2, 32: 2}              # of NB_PAIRS: built backwards from wanted level patterns (backwards_patterns)
EST_WORDS = 184
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hm_rdoq.npz")

# the number of cases that reach each edge, as the generator printed them (T: {edge: cases}, of 641 / 577 / 385 / 385 cases)
SHARES = {
    4: {'abs_sum_lt_2': 119, 'all_zero': 20, 'bonus_met': 37, 'cbf_ctx_0': 160, 'cbf_ctx_1': 481, 'escape': 327, 'fma_differs': 1, 'forbidden_met': 10, 'found_last': 363, 'hide_down': 42, 'hide_up': 30, 'hide_zero_up': 18, 'lambda_moves': 122, 'last_moved': 41, 'level_ge_3': 361, 'max_minus_1': 40, 'nine_in_group': 291, 'nothing_coded': 40, 'rice_4': 168, 'scan_0': 192, 'scan_1': 225, 'scan_2': 224, 'two_above_one': 327, 'zero_from_1': 93, 'zero_from_2': 1},
    8: {'abs_sum_lt_2': 99, 'all_zero': 21, 'bonus_met': 14, 'cbf_ctx_0': 144, 'cbf_ctx_1': 433, 'escape': 321, 'fma_differs': 1, 'forbidden_met': 32, 'found_last': 353, 'group_zeroed': 16, 'hide_down': 58, 'hide_up': 49, 'hide_zero_up': 30, 'lambda_moves': 107, 'last_moved': 26, 'level_ge_3': 337, 'max_minus_1': 40, 'nine_in_group': 167, 'nnz_before_pos0_is_0': 64, 'nothing_coded': 42, 'rice_4': 72, 'scan_0': 160, 'scan_1': 225, 'scan_2': 192, 'two_above_one': 210, 'zero_from_1': 93, 'zero_from_2': 9},
    16: {'abs_sum_lt_2': 64, 'all_zero': 8, 'bonus_met': 12, 'cbf_ctx_0': 96, 'cbf_ctx_1': 289, 'escape': 217, 'fma_differs': 1, 'forbidden_met': 35, 'found_last': 243, 'group_emptied': 19, 'group_zeroed': 52, 'hide_down': 53, 'hide_up': 33, 'hide_zero_up': 27, 'lambda_moves': 71, 'last_moved': 24, 'level_ge_3': 225, 'max_minus_1': 29, 'nine_in_group': 71, 'nnz_before_pos0_is_0': 64, 'nothing_coded': 16, 'rice_4': 49, 'scan_0': 385, 'two_above_one': 105, 'zero_from_1': 67, 'zero_from_2': 9},
    32: {'abs_sum_lt_2': 64, 'all_zero': 13, 'bonus_met': 9, 'cbf_ctx_0': 96, 'cbf_ctx_1': 289, 'escape': 217, 'fma_differs': 1, 'forbidden_met': 41, 'found_last': 245, 'group_emptied': 28, 'group_zeroed': 78, 'hide_down': 56, 'hide_up': 41, 'hide_zero_up': 36, 'lambda_moves': 84, 'last_moved': 18, 'level_ge_3': 223, 'max_minus_1': 45, 'nine_in_group': 72, 'nnz_before_pos0_is_0': 88, 'nothing_coded': 26, 'rice_4': 48, 'scan_0': 385, 'two_above_one': 112, 'zero_from_1': 76, 'zero_from_2': 18},
}


NB_NOISE_PAIRS = 4                                       # of NB_PAIRS: a flat prediction under noise of amplitude 2, 3, 5, 8


def backwards_patterns(t):
    """Level patterns [T, T] for the inferred significance flag (iNNZbeforePos0 == 0): a coded group below the last one whose only level
    sits at its scan position 0 -- the group's top-left corner under every scan -- large enough to survive; once beside a small last
    level, once beside a large one"""
    out = []
    for corner, far in ((6, 3), (9, -7))[:NB_BACKWARDS[t]]:
        levels = np.zeros((t, t), np.int64)
        levels[0, 0], levels[0, 4], levels[t - 4, t - 4] = 12, corner, far
        out.append(levels)
    return out


def pairs_of(t):
    from tests import hm_unit_cases
    predictions, targets = tq.mixed_pairs(t, NB_PAIRS[t] - NB_NOISE_PAIRS - NB_BACKWARDS[t], 8100 + t)
    for levels in backwards_patterns(t):
        made = hm_unit_cases.backwards(levels, QPS[1:3])
        assert made is not None, "a wanted pattern fits no QP"
        predictions, targets = np.concatenate([predictions, made[0][None]]), np.concatenate([targets, made[1][None]])
    rng = np.random.default_rng(8200 + t)
    flat = np.full((NB_NOISE_PAIRS, t, t), 128, np.uint8)
    noise = np.stack([rng.integers(-a, a + 1, (t, t)) for a in (2, 3, 5, 8)])
    predictions, targets = np.concatenate([predictions, flat]), np.concatenate([targets, (flat.astype(np.int64) + noise).astype(np.uint8)])
    modes = np.array([MODES[k % len(MODES)] for k in range(len(predictions))], np.uint8)
    return np.array(predictions), np.array(targets), modes


TIE_FACTOR = len(LAMBDA_FACTORS)                         # the factor index of the tie case: its lambda is tie_lambda(t), not a multiple of HM's
TIE_QPS = (25, 23, 27, 29, 31, 20, 18, 33, 35, 13, 11)   # (quantiser scales that are no power of two: the costs round)
_TIES = {}


def tie_lambda(t):
    """(pair, QP, lambda): a lambda within a few units in the last place of the one at which, at the unit's LAST position (the walk's first
    decision: levels uiMaxAbsLevel and uiMaxAbsLevel - 1, no significance cost, context set and counters at their start), the two
    candidates' costs are equal -- the nearest such double for which the walk's levels differ between the two roundings of dErr^2 *
    errScale + lambda * rate.  Deterministic: the first pair from index 4 on, the first QP of TIE_QPS and the first offset in 0, 1, -1, 2, -2, ... that does."""
    from fractions import Fraction
    if t in _TIES:
        return _TIES[t]
    predictions, targets, modes = pairs_of(t)
    log2 = t.bit_length() - 1
    for p, qp in ((p, qp) for p in range(4, len(modes)) for qp in TIE_QPS):
        qbits, scale = 14 + qp // 6 + 7 - log2, tq.QUANT_SCALES[qp % 6]
        err_scale = float(1 << 15) * 2.0 ** (-2.0 * (7 - log2)) / scale / scale / 1
        e = est_bits(t, qp)
        coeffs = tq.forward(targets[p].astype(np.int64) - predictions[p].astype(np.int64))
        scan = cabac.scan_of_mode(t, int(modes[p]))
        top = max_levels(coeffs, qp)
        order = cabac.grouped_scan(t, scan)
        filled = [i for i, (x, y) in enumerate(order) if top[y, x] > 0]
        if not filled or top[order[filled[-1]][1], order[filled[-1]][0]] < 2:
            continue
        x, y = order[filled[-1]]
        a, level_double, ctx_set = int(top[y, x]), abs(int(coeffs[y, x])) * scale, 2 if filled[-1] >= 16 else 0
        one, two = e['one'][4 * ctx_set + 1], e['abs'][ctx_set]

        def rate(v):                                      # xGetICRate at the walk's start: c1 = 1, no flag spent, Rice parameter 0
            return 32768 + (one[0] if v == 1 else one[1] + two[0] if v == 2 else (cabac.remaining_bins(v - 3, 0) << 15) + one[1] + two[1])

        gain = Fraction(level_double - ((a - 1) << qbits)) ** 2 - Fraction(level_double - (a << qbits)) ** 2
        if rate(a) == rate(a - 1) or gain * (rate(a) - rate(a - 1)) <= 0:
            continue
        centre = np.float64(float(gain * Fraction(err_scale) / (rate(a) - rate(a - 1))))
        for step in range(0, 12):
            for sign in ((1,) if step == 0 else (1, -1)):
                lam = centre
                for _ in range(step):
                    lam = np.nextafter(lam, np.inf * sign)
                lam = float(lam)
                if not np.array_equal(walk(coeffs, scan, qp, lam, 1, 0)[0], walk(coeffs, scan, qp, lam, 1, 0, fused=True)[0]):
                    _TIES[t] = (p, qp, lam)
                    return _TIES[t]
    raise AssertionError("no tie found at T %d" % t)


def lambda_of_case(t, case):
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    return tie_lambda(t)[2] if case[2] == TIE_FACTOR else ip.hm_intra_lambda(case[1]) * LAMBDA_FACTORS[case[2]]


def cases_of(t):
    """[(pair, qp, factor index, sdh, depth)] in the fixture's order; the last one is the tie case (factor index TIE_FACTOR)"""
    return _grid_cases(t) + [(tie_lambda(t)[0], tie_lambda(t)[1], TIE_FACTOR, 0, 0)]


def _grid_cases(t):
    out = []
    for p in range(NB_PAIRS[t]):
        for qp in QPS:
            for sdh in (0, 1):
                out += [(p, qp, f, sdh, 0) for f in range(len(LAMBDA_FACTORS))]
                out.append((p, qp, 0, sdh, 1))
    return out


def max_levels(coeffs, qp):
    """uiMaxAbsLevel [T, T] of the coefficients at a QP"""
    log2_t = coeffs.shape[0].bit_length() - 1
    per, rem = qp // 6, qp % 6
    qbits = 14 + per + 7 - log2_t
    level_double = np.minimum(np.abs(coeffs.astype(np.int64)) * tq.QUANT_SCALES[rem], 2 ** 31 - 1 - (1 << (qbits - 1)))
    return np.minimum((level_double + (1 << (qbits - 1))) >> qbits, 32767)


# edges only the walk's own state shows: the d64CostZeroCG test taken while the group held levels, the inferred flag's d64SigCost_0, the
# search stopped by a level > 1, the Rice parameter reaching 4, an escape-coded remainder costed (symbol >= 3 << r), the forbidden hiding
# candidate and the 4 << 15 candidate met, iBestLastIdxP1 == 0, and -- the two forms evaluated side by side -- levels that differ when
# dErr^2 * errScale + lambda * rate is rounded once
WALK_EDGES = {'group_zeroed', 'nnz_before_pos0_is_0', 'found_last', 'rice_4', 'escape', 'forbidden_met', 'bonus_met', 'nothing_coded'}


def wanted_edges(t):
    edges = WALK_EDGES - ({'group_zeroed', 'nnz_before_pos0_is_0'} if t == 4 else set()) | {'fma_differs'} | {'max_minus_1', 'zero_from_1', 'zero_from_2', 'level_ge_3', 'all_zero', 'last_moved', 'nine_in_group', 'two_above_one', 'cbf_ctx_0',
             'cbf_ctx_1', 'hide_up', 'hide_down', 'hide_zero_up', 'abs_sum_lt_2', 'lambda_moves'}
    if t <= 8:
        edges |= {'scan_0', 'scan_1', 'scan_2'}
    if t >= 16:                                           # (told from the output; the walk's group_zeroed is wanted from T = 8 on)
        edges.add('group_emptied')
    return edges


def reached(arrays, t):
    """{edge: number of cases} of HM's recorded output at unit size T"""
    count = {}

    def hit(edge):
        count[edge] = count.get(edge, 0) + 1

    cases = cases_of(t)
    levels_all = arrays["case_levels_%d" % t].astype(np.int64)
    index = {case: k for k, case in enumerate(cases)}
    for k, (p, qp, f, sdh, depth) in enumerate(cases):
        coeffs = tq.forward(arrays["pair_targets_%d" % t][p].astype(np.int64) - arrays["pair_predictions_%d" % t][p].astype(np.int64))
        top, levels = max_levels(coeffs, qp), np.abs(levels_all[k])
        scan = int(arrays["case_scan_%d" % t][k])
        order = cabac.grouped_scan(t, scan)
        top_s, lev_s = np.array([top[y, x] for x, y in order]), np.array([levels[y, x] for x, y in order])
        hit('scan_%d' % scan)
        hit('cbf_ctx_%d' % int(arrays["case_cbf_ctx_%d" % t][k]))
        if sdh and arrays["case_abs_sum_%d" % t][k] < 2:
            hit('abs_sum_lt_2')
        if not sdh:
            if np.any((lev_s == top_s - 1) & (top_s >= 2)):
                hit('max_minus_1')
            for v in (1, 2):
                if np.any((lev_s == 0) & (top_s == v)):
                    hit('zero_from_%d' % v)
            if top_s.max() > 0 and lev_s.max() == 0:
                hit('all_zero')
            if lev_s.max() > 0 and np.nonzero(lev_s)[0][-1] < np.nonzero(top_s)[0][-1]:
                hit('last_moved')
            if lev_s.max() > 0:
                last_group = np.nonzero(lev_s)[0][-1] // 16
                if any(lev_s[16 * g:16 * g + 16].max() == 0 and top_s[16 * g:16 * g + 16].max() > 0 for g in range(1, last_group)):
                    hit('group_emptied')
        if lev_s.max() >= 3:
            hit('level_ge_3')
        groups = lev_s.reshape(-1, 16)
        if np.any((groups != 0).sum(1) >= 9):
            hit('nine_in_group')
        if np.any((groups > 1).sum(1) >= 2):
            hit('two_above_one')
        if sdh:
            off = np.abs(levels_all[index[(p, qp, f, 0, depth)]])
            if np.any((off != 0) & (levels == off + 1)):
                hit('hide_up')
            if np.any((off != 0) & (levels == off - 1)):
                hit('hide_down')
            if np.any((off == 0) & (levels == 1)):
                hit('hide_zero_up')
        if f in (1, 2) and not depth and np.any(levels_all[k] != levels_all[index[(p, qp, 0, sdh, 0)]]):
            hit('lambda_moves')
        # the walk's own events, from the restatement below -- which must give HM's levels on the case, or its events say nothing
        lam = float(arrays["case_lambda_%d" % t][k:k + 1].view(np.float64)[0])
        events = set()
        mine, abs_sum = walk(coeffs, scan, qp, lam, 1 - depth, sdh, events=events)
        assert np.array_equal(mine, levels_all[k]) and abs_sum == arrays["case_abs_sum_%d" % t][k], "the restatement differs from HM: T %d case %d" % (t, k)
        for event in events & WALK_EDGES:
            hit(event)
        if not sdh and not np.array_equal(walk(coeffs, scan, qp, lam, 1 - depth, 0, fused=True)[0], mine):
            hit('fma_differs')
    return count


# ---- a Python restatement of xRateDistOptQuant, written from HM's text with the helpers of cabac_rate_cases: the second yardstick of
# ---- the twin outside the fixture, and the source of the walk's own events for the edges no output shows

INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)
MAX_DOUBLE = 1.7e+308
INIT_CBF = (111, 141)


def _bits(init_value, qp):
    c = cabac.Context(init_value, qp)
    state = 2 * c.p + c.mps
    return (cabac.ENTROPY_BITS[state], cabac.ENTROPY_BITS[state ^ 1])


def est_bits(t, qp):
    """{'sig', 'one', 'abs', 'group', 'cbf': [(bits of bin 0, of bin 1)], 'last_x', 'last_y': cumulative lists} at unit size t"""
    log2 = t.bit_length() - 1
    offset, shift, top = 3 * (log2 - 2) + ((log2 - 1) >> 2), (log2 + 1) >> 2, 2 * log2 - 1
    e = {name: [_bits(v, qp) for v in init] for name, init in (('sig', cabac.INIT_SIG), ('one', cabac.INIT_ONE), ('abs', cabac.INIT_ABS),
                                                                ('group', cabac.INIT_GROUP), ('cbf', INIT_CBF))}
    for name in ('last_x', 'last_y'):
        table, running = [], 0
        for g in range(top):
            zero, one = _bits(cabac.INIT_LAST[offset + (g >> shift)], qp)
            table.append(running + zero)
            running += one
        e[name] = table + [running]
    return e


def _fma(a, b, c):
    """a * b + c rounded once"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def walk(coeffs, scan, qp, lam, cbf_ctx, sdh, fused=False, events=None):
    """(levels [T, T], uiAbsSum) of integer coefficients [T, T]: TComTrQuant::xRateDistOptQuant under the settings of include/pnn_hip.h.
    Python floats are IEEE doubles and round once per operation; fused=True rounds dErr^2 * errScale + lambda * rate of xGetCodedLevel once
    instead (what a contracted multiply-add would give).  events: a set that receives the names of the branches the walk took."""
    events = set() if events is None else events
    coeffs = np.asarray(coeffs).astype(np.int64)
    t = coeffs.shape[0]
    log2 = t.bit_length() - 1
    per, rem, ts = qp // 6, qp % 6, 7 - log2
    qbits, scale = 14 + per + ts, tq.QUANT_SCALES[rem]
    err_scale = float(1 << 15) * 2.0 ** (-2.0 * ts) / scale / scale / 1
    e = est_bits(t, qp)
    order = cabac.grouped_scan(t, scan)
    nb, wg = t * t, t // 4
    group_order = cabac.plain_scan(wg, scan)

    def ic_rate(a, one_ctx, abs_ctx, rice, c1_idx, c2_idx):
        base = (2 + (c2_idx < 1)) if c1_idx < 8 else 1
        rate = 32768
        if a >= base:
            if a - base >= (3 << rice):
                events.add('escape')
            rate += cabac.remaining_bins(a - base, rice) << 15
            if c1_idx < 8:
                rate += e['one'][one_ctx][1]
                if c2_idx < 1:
                    rate += e['abs'][abs_ctx][1]
        elif a == 1:
            rate += e['one'][one_ctx][0]
        elif a == 2:
            rate += e['one'][one_ctx][1] + e['abs'][abs_ctx][0]
        else:
            rate = 0
        return rate

    level_double = [min(abs(int(coeffs[y, x])) * scale, 2 ** 31 - 1 - (1 << (qbits - 1))) for x, y in order]
    max_abs = [min(32767, (v + (1 << (qbits - 1))) >> qbits) for v in level_double]
    cost0 = [float(v) * float(v) * err_scale for v in level_double]
    cost, cost_sig, dst = [0.] * nb, [0.] * nb, list(max_abs)
    rate_up, rate_down, sig_delta, delta_u = [0] * nb, [0] * nb, [0] * nb, [0] * nb
    group_sig, group_flag = [0.] * (wg * wg), {}
    block_uncoded = base_cost = 0.
    ctx_set, c1, c2, c1_idx, c2_idx, rice, last_pos, last_group = 0, 1, 0, 0, 0, 0, -1, -1
    for g in range(wg * wg - 1, -1, -1):
        gx, gy = group_order[g]
        right, below = (gx < wg - 1 and group_flag.get((gx + 1, gy), 0)), (gy < wg - 1 and group_flag.get((gx, gy + 1), 0))
        pattern = int(bool(right)) + 2 * int(bool(below))
        sig_cost = sig_cost_0 = coded_level_and_dist = uncoded_dist = 0.
        nnz_before_pos0 = 0
        for n in range(15, -1, -1):
            i = 16 * g + n
            x, y = order[i]
            block_uncoded += cost0[i]
            if max_abs[i] > 0 and last_pos < 0:
                last_pos, ctx_set, last_group = i, (2 if g > 0 else 0), g
            if last_pos >= 0:
                one_ctx, abs_ctx = 4 * ctx_set + c1, ctx_set + c2
                is_last = i == last_pos
                level, curr_sig = 0, 0.
                if not is_last:
                    sig_ctx = cabac.sig_context(t, scan, pattern, x, y)
                if not is_last and max_abs[i] < 3:
                    cost_sig[i] = lam * float(e['sig'][sig_ctx][0])
                    cost[i] = cost0[i] + cost_sig[i]
                else:
                    cost[i] = MAX_DOUBLE
                if is_last or max_abs[i] > 0:
                    if not is_last:
                        curr_sig = lam * float(e['sig'][sig_ctx][1])
                    for a in range(max_abs[i], max(max_abs[i] - 1, 1) - 1, -1):
                        err = float(level_double[i] - (a << qbits))
                        bits = lam * float(ic_rate(a, one_ctx, abs_ctx, rice, c1_idx, c2_idx))
                        curr = _fma(err * err, err_scale, bits) if fused else err * err * err_scale + bits
                        curr += curr_sig
                        if curr < cost[i]:
                            level, cost[i], cost_sig[i] = a, curr, curr_sig
                if not is_last:
                    sig_delta[i] = e['sig'][sig_ctx][1] - e['sig'][sig_ctx][0]
                delta_u[i] = (level_double[i] - (level << qbits)) >> (qbits - 8)
                if level > 0:
                    now = ic_rate(level, one_ctx, abs_ctx, rice, c1_idx, c2_idx)
                    rate_up[i] = ic_rate(level + 1, one_ctx, abs_ctx, rice, c1_idx, c2_idx) - now
                    rate_down[i] = ic_rate(level - 1, one_ctx, abs_ctx, rice, c1_idx, c2_idx) - now
                else:
                    rate_up[i] = e['one'][one_ctx][0]
                dst[i] = level
                base_cost += cost[i]
                base_level = (2 + (c2_idx < 1)) if c1_idx < 8 else 1
                if level >= base_level and level > 3 * (1 << rice):
                    rice = min(rice + 1, 4)
                    if rice == 4:
                        events.add('rice_4')
                if level >= 1:
                    c1_idx += 1
                    if c1_idx > 8:
                        events.add('ninth_level')
                if level > 1:
                    c1, c2, c2_idx = 0, c2 + (c2 < 2), c2_idx + 1
                    if c2_idx > 1:
                        events.add('second_above_one')
                elif 0 < c1 < 3 and level:
                    c1 += 1
                if i % 16 == 0 and i > 0:
                    ctx_set = (2 if ((i - 1) >> 4) > 0 else 0) + (c1 == 0)
                    c1, c2, c1_idx, c2_idx, rice = 1, 0, 0, 0, 0
            else:
                base_cost += cost0[i]
            sig_cost += cost_sig[i]
            if n == 0:
                sig_cost_0 = cost_sig[i]
            if dst[i]:
                group_flag[(gx, gy)] = 1
                coded_level_and_dist += cost[i] - cost_sig[i]
                uncoded_dist += cost0[i]
                if n != 0:
                    nnz_before_pos0 += 1
        if last_group >= 0:
            if g:
                ctx = int(bool(right) or bool(below))
                if not group_flag.get((gx, gy), 0):
                    base_cost += lam * float(e['group'][ctx][0]) - sig_cost
                    group_sig[g] = lam * float(e['group'][ctx][0])
                elif g < last_group:
                    if nnz_before_pos0 == 0:
                        events.add('nnz_before_pos0_is_0')
                        base_cost -= sig_cost_0
                        sig_cost -= sig_cost_0
                    zero_cost = base_cost
                    base_cost += lam * float(e['group'][ctx][1])
                    zero_cost += lam * float(e['group'][ctx][0])
                    group_sig[g] = lam * float(e['group'][ctx][1])
                    zero_cost += uncoded_dist
                    zero_cost -= coded_level_and_dist
                    zero_cost -= sig_cost
                    if zero_cost < base_cost:
                        events.add('group_zeroed')
                        group_flag[(gx, gy)] = 0
                        base_cost = zero_cost
                        group_sig[g] = lam * float(e['group'][ctx][0])
                        for i in range(16 * g, 16 * g + 16):
                            if dst[i]:
                                dst[i], cost[i], cost_sig[i] = 0, cost0[i], 0.
            else:
                group_flag[(gx, gy)] = 1
    levels = np.zeros((t, t), np.int64)
    if last_pos < 0:
        return levels, 0
    best_cost = block_uncoded + lam * float(e['cbf'][cbf_ctx][0])
    base_cost += lam * float(e['cbf'][cbf_ctx][1])
    best_last_p1, found_last = 0, False
    for g in range(last_group, -1, -1):
        base_cost -= group_sig[g]
        if group_flag.get(group_order[g], 0):
            for i in range(16 * g + 15, 16 * g - 1, -1):
                if i > last_pos:
                    continue
                if dst[i]:
                    x, y = order[i]
                    px, py = (y, x) if scan == cabac.VER else (x, y)
                    gxl, gyl = cabac.LAST_GROUP[px], cabac.LAST_GROUP[py]
                    bits = float(e['last_x'][gxl] + e['last_y'][gyl])
                    if gxl > 3:
                        bits += 32768. * ((gxl - 2) >> 1)
                    if gyl > 3:
                        bits += 32768. * ((gyl - 2) >> 1)
                    total = base_cost + lam * bits - cost_sig[i]
                    if total < best_cost:
                        best_last_p1, best_cost = i + 1, total
                    if dst[i] > 1:
                        found_last = True
                        events.add('found_last')
                        break
                    base_cost -= cost[i]
                    base_cost += cost0[i]
                else:
                    base_cost -= cost_sig[i]
            if found_last:
                break
    if best_last_p1 == 0:
        events.add('nothing_coded')
    if 0 < best_last_p1 < last_pos + 1:
        events.add('last_moved')
    abs_sum = 0
    for i in range(best_last_p1):
        x, y = order[i]
        abs_sum += dst[i]
        levels[y, x] = -dst[i] if coeffs[y, x] < 0 else dst[i]
    if sdh and abs_sum >= 2:
        inv = float(INV_QUANT_SCALES[rem])
        rd_factor = int(inv * inv * (1 << (2 * per)) / lam / 16 / 1 + 0.5)
        last_cg = -1
        for g in range(wg * wg - 1, -1, -1):
            at = [order[16 * g + n] for n in range(16)]
            value = [int(levels[y, x]) for x, y in at]
            nonzero = [n for n in range(16) if value[n]]
            first, last = (nonzero[0], nonzero[-1]) if nonzero else (16, -1)
            if last >= 0 and last_cg == -1:
                last_cg = 1
            if last - first >= 4:
                signbit = 0 if value[first] > 0 else 1
                if signbit != (sum(value[first:last + 1]) & 1):
                    min_cost, min_n, final = 2 ** 63 - 1, -1, 0
                    for n in range(last if last_cg == 1 else 15, -1, -1):
                        i = 16 * g + n
                        if value[n]:
                            up = rd_factor * -delta_u[i] + rate_up[i]
                            down = rd_factor * delta_u[i] + rate_down[i] - (sig_delta[i] if abs(value[n]) == 1 else 0)
                            if last_cg == 1 and last == n and abs(value[n]) == 1:
                                down -= 4 << 15
                                events.add('bonus_met')
                            if up < down:
                                cur, change = up, 1
                            else:
                                change = -1
                                if n == first and abs(value[n]) == 1:
                                    cur = 2 ** 63 - 1
                                    events.add('forbidden_met')
                                else:
                                    cur = down
                        else:
                            cur, change = rd_factor * -abs(delta_u[i]) + (1 << 15) + rate_up[i] + sig_delta[i], 1
                            x, y = at[n]
                            if n < first and (0 if coeffs[y, x] >= 0 else 1) != signbit:
                                cur = 2 ** 63 - 1
                        if cur < min_cost:
                            min_cost, min_n, final = cur, n, change
                    x, y = at[min_n]
                    events.add('hide_%s' % ('zero_up' if not value[min_n] else 'up' if final > 0 else 'down'))
                    levels[y, x] += final if coeffs[y, x] >= 0 else -final
            if last_cg == 1:
                last_cg = 0
    return levels, abs_sum
