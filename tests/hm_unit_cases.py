"""What tests/golden/make_hm_unit_coding.py, tests/test_hm_unit_coding.py and tests/test_gpu_hm_unit_coding.py share: the layout of
tests/golden/hm_unit_coding.npz (whole transform units coded by HM-16.15's own transformNxN, codeCoeffNxN and invTransformNxN), the pairs
that are built backwards from wanted levels, and the EDGES a set of recorded levels must reach -- read off HM's levels and HM's scan
index alone, in codeCoeffNxN's coding order, so that neither a thinner fixture nor a unit that codes nothing of interest passes silently.

The fixture, per T in SIZES (n pairs, k cases, c calls on given levels):
  pair_predictions_T, pair_targets_T uint8 [n, T, T]; pair_modes_T uint8 [n]         the units; a pair has ONE intra mode
  case_pair_T int16, case_qp_T, case_sdh_T, case_scan_T uint8 [k]                    case = pair at a QP with SignDataHidingEnabledFlag
  case_abs_sum_T int32, case_bits_T int64 [k]                                        uiAbsSum; m_fracBits increase (0: all levels zero)
  case_levels_T, case_residual_T int16 [k, T, T]                                     levels out of transformNxN; invTransformNxN of them
  code_levels_T int16 [c, T, T]; code_mode_T, code_qp_T, code_sdh_T, code_scan_T uint8, code_bits_T int64 [c]     codeCoeffNxN alone
and scan_of_mode uint8 [4, 35]; cost_lambda, cost_r, cost_j uint64 (doubles as bit patterns; R whole bits), cost_d uint32,
cost_fused_differs bool [m]; rd_lambdas uint64 [4]; rd_first int64 (the index of the first triple taken from a second-pass call)."""
import os
from fractions import Fraction

import numpy as np

from tests import cabac_rate_cases as cabac
from tests import trquant_cases as tq

SIZES = (4, 8, 16, 32)
QPS = (0, 22, 37, 51)
MODES = (0, 1, 10, 26, 5, 6, 14, 15, 21, 22, 30, 31)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hm_unit_coding.npz")
NB_BASE_PAIRS = {4: 12, 8: 12, 16: 8, 32: 6}              # of trquant_cases.mixed_pairs: coded at every QP with the flag off and on
# the second-pass call whose winners' (lambda, D, R) the generator hands to calcRdCost (rd_pass_cases.seeded(RD_WIDTH, RD_BLOCKS))
RD_WIDTH, RD_BLOCKS, RD_QPS = 8, 33, (22, 27, 32, 37)


def place(t, scan, wanted, dtype=np.int64):
    """levels [T, T] with wanted[scan position] at that position of the grouped scan"""
    order = cabac.grouped_scan(t, scan)
    levels = np.zeros((t, t), dtype)
    for pos, value in wanted.items():
        x, y = order[pos]
        levels[y, x] = value
    return levels


def backwards(levels, qps=QPS):
    """(prediction, target, qp): the largest QP of `qps` at which the inverse transform of the dequantised `levels` fits 8 bits around a
    flat prediction -- a pair whose coding gives `levels` back, up to the rounding of the samples.  None if no QP fits.  Levels given as
    floats aim at coefficients BETWEEN the quantiser's steps (1.7: a level of 1 with a large negative remainder deltaU)."""
    t = levels.shape[0]
    for qp in sorted(qps, reverse=True):
        if np.issubdtype(levels.dtype, np.integer):
            coeffs = tq.dequantise(levels, qp, t.bit_length() - 1)
        else:
            coeffs = np.rint(levels * 2. ** (14 + qp // 6 + 7 - (t.bit_length() - 1)) / tq.QUANT_SCALES[qp % 6]).astype(np.int64)
            if np.abs(coeffs).max() > 32767:
                continue
        residual = tq.inverse(coeffs)
        flat = int(np.clip(round(127.5 - (int(residual.max()) + int(residual.min())) / 2.), 0, 255))
        if 0 <= flat + residual.min() and flat + residual.max() <= 255:
            return np.full((t, t), flat, np.uint8), (flat + residual).astype(np.uint8), qp
    return None


def wanted_patterns(t):
    """[(name, intra mode, levels [T, T])]: the level patterns the backwards pairs aim at, per edge of the issue's list"""
    d, h, v = cabac.DIAG, cabac.HOR, cabac.VER
    out = []
    for p in sorted({0, 1, 2, 3, 4, 6, 8, 12, 16, 24} & set(range(t))):         # one position per last-position group, x and y alike
        lone = np.zeros((t, t), np.int64)
        lone[p, p] = 2 if p % 2 else -2
        out.append(("last_%d" % p, 0, lone))
    if t <= 8:
        for mode, scan in ((26, h), (10, v)):
            for x, y in ((3, 1), (1, 3), (t - 1, 0), (0, t - 1)):
                lone = np.zeros((t, t), np.int64)
                lone[y, x] = 3
                out.append(("off_diagonal_%d_%d_%d" % (scan, x, y), mode, lone))
    scans = ((0, d), (26, h), (10, v)) if t <= 8 else ((0, d),)
    for mode, scan in scans:
        out.append(("eight", mode, place(t, scan, {i: (1, -1)[i % 2] for i in range(8)})))
        out.append(("nine", mode, place(t, scan, {i: (1, -1, 1)[i % 3] for i in range(1, 12)})))
        out.append(("two_above_1", mode, place(t, scan, {0: 3, 1: -2, 2: 4, 3: 1})))
        out.append(("rice", mode, place(t, scan, {5: 4, 4: -7, 3: 13, 2: 25, 1: -27, 0: 30})))
        out.append(("escape", mode, place(t, scan, {0: 12, 2: -9})))
        for first, last, a, b in ((0, 3, 2, 1), (0, 3, 1, 2), (1, 4, 1, 1), (0, 4, 2, 1), (0, 4, 2, 2), (1, 5, -3, 1), (2, 6, 1, -1), (9, 12, 1, 1)):
            out.append(("span_%d" % (last - first), mode, place(t, scan, {first: a, last: b})))
        # the level at `first` is 1 just above its threshold (the cheapest change, were it allowed); the parity is wrong
        out.append(("first_one_rule", mode, place(t, scan, {0: 0.72, 4: 2.06}, np.float64)))
        out.append(("first_one_rule", mode, place(t, scan, {1: -0.75, 3: 0.2, 6: -2.1, 7: 1.05}, np.float64)))
        if t >= 8:
            out.append(("carried_c1", mode, place(t, scan, {16: 3, 17: 1, 20: -1, 0: 1, 1: -1, 2: 2})))
            out.append(("middle_groups", mode, place(t, scan, {0: 1, 32: -1, 50: 1})))
            out.append(("one_eight_nine", mode, place(t, scan, dict([(i, 1) for i in range(8)] + [(16 + i, -1) for i in range(9)] + [(40, 1)]))))
    return out


def edges_of(levels, scan, hiding=False):
    """The tags of the issue's edge list that ONE unit's levels reach, walking the groups as codeCoeffNxN does."""
    levels = np.asarray(levels).astype(np.int64)
    t = levels.shape[0]
    order = cabac.grouped_scan(t, scan)
    values = [int(levels[y, x]) for x, y in order]
    nonzero = [i for i, value in enumerate(values) if value]
    if not nonzero:
        return {'all_zero'}
    tags = set()
    last = nonzero[-1]
    lx, ly = order[last]
    tags.add('last_x_group_%d' % cabac.LAST_GROUP[ly if scan == cabac.VER else lx])
    tags.add('last_y_group_%d' % cabac.LAST_GROUP[lx if scan == cabac.VER else ly])
    if lx != ly and scan != cabac.DIAG:
        tags.add('last_off_diagonal_%s' % ('horizontal' if scan == cabac.HOR else 'vertical'))
    last_set, c1 = last >> 4, 1
    for s in range(last_set, -1, -1):
        group = values[16 * s:16 * s + 16]
        found = [abs(value) for value in reversed(group) if value]                 # in coding order
        middle = 0 < s < last_set
        if not found:
            if middle:
                tags.add('middle_group_not_coded')
            continue
        if middle and len(found) == 1 and group[0]:
            tags.add('middle_group_inferred_sig_flag')
        tags.add('group_of_1' if len(found) == 1 else 'group_of_8' if len(found) == 8 else 'group_of_9_or_more' if len(found) > 8 else 'group')
        if c1 == 0:
            tags.add('group_after_c1_0')
        c1, above_1 = 1, 0
        for a in found[:8]:
            if a > 1:
                c1, above_1 = 0, above_1 + 1
            elif 0 < c1 < 3:
                c1 += 1
        if above_1 >= 2:
            tags.add('second_level_above_1')
        if max(found) > 2:
            tags.add('level_above_2')
        rice, first2 = 0, 1
        for idx, a in enumerate(found):
            base = 2 + first2 if idx < 8 else 1
            if a >= base:
                if a - base >= 3 << rice:
                    tags.add('escape_exp_golomb')
                if rice == 4:
                    tags.add('remaining_at_rice_4')
                if a > 3 << rice:
                    rice = min(rice + 1, 4)
            if a >= 2:
                first2 = 0
        if hiding:
            where = [n for n, value in enumerate(group) if value]
            if where[-1] - where[0] in (3, 4):
                tags.add('hiding_span_%d' % (where[-1] - where[0]))
    return tags


def wanted_edges(t):
    """The tags that must be reached at size T (what T does not allow is left out)"""
    top = cabac.LAST_GROUP[t - 1]
    tags = {'last_%s_group_%d' % (c, g) for c in 'xy' for g in range(top + 1)}
    tags |= {'group_of_1', 'group_of_8', 'group_of_9_or_more', 'second_level_above_1', 'level_above_2', 'remaining_at_rice_4',
             'escape_exp_golomb', 'hiding_span_3', 'hiding_span_4', 'hidden_up', 'hidden_down', 'first_one_rule'}
    if t <= 8:
        tags |= {'last_off_diagonal_horizontal', 'last_off_diagonal_vertical'}
    if t >= 8:
        tags |= {'group_after_c1_0', 'middle_group_not_coded', 'middle_group_inferred_sig_flag'}
    return tags


def hiding_edges(prediction, target, qp, scan, plain, hidden):
    """'hidden_up' / 'hidden_down' / 'first_one_rule' of ONE unit from HM's levels without (`plain`) and with (`hidden`) the flag.  The
    last tag: in a group HM changed, the level at `first` was +-1 with a remainder <= 0 and, were it allowed, would have cost less than
    any allowed candidate -- HM changed another position.  Coefficients and remainders come from the numpy restatements (the forward
    transform is pinned to HM by hm_transforms.npz); they only say WHERE to look, the levels are HM's."""
    from tests import sign_hiding_cases as sdh
    tags = set()
    plain, hidden = np.asarray(plain).astype(np.int64), np.asarray(hidden).astype(np.int64)
    if (np.abs(hidden) > np.abs(plain)).any():
        tags.add('hidden_up')
    if (np.abs(hidden) < np.abs(plain)).any():
        tags.add('hidden_down')
    if tags:
        t = plain.shape[0]
        coeffs = tq.forward(target.astype(np.int64) - prediction.astype(np.int64))
        du = sdh.delta_u(coeffs, qp)
        order = cabac.grouped_scan(t, scan)
        met_a_level = False
        for c in range(t * t // 16 - 1, -1, -1):
            where = order[16 * c:16 * c + 16]
            values = [int(plain[y, x]) for x, y in where]
            first, last = sdh.group_span(values)
            if last < 0:
                continue
            in_last_group, met_a_level = not met_a_level, True
            if all(hidden[y, x] == plain[y, x] for x, y in where):
                continue
            signbit = 0 if values[first] > 0 else 1
            rows = [(n,) + sdh.row_of(values[n], int(coeffs[where[n][1], where[n][0]]), int(du[where[n][1], where[n][0]]), n, first, signbit)
                    for n in range(last if in_last_group else 15, -1, -1)]
            allowed = min(cost for _, _, cost, change in rows if change is not None)
            x, y = where[first]
            if any(row == 'nonzero_first_one_forbidden' for _, row, _, _ in rows) and int(du[y, x]) < allowed and hidden[y, x] == plain[y, x]:
                tags.add('first_one_rule')
    return tags


def reached(fixture, t):
    """Every tag the fixture's cases (and, for the level tags, its calls on given levels) of size T reach"""
    tags = set()
    pairs, qps, flags, scans = (fixture['case_%s_%d' % (name, t)] for name in ('pair', 'qp', 'sdh', 'scan'))
    levels = fixture['case_levels_%d' % t]
    index = {(int(p), int(q), int(f)): k for k, (p, q, f) in enumerate(zip(pairs, qps, flags))}
    for k in range(len(pairs)):
        tags |= edges_of(levels[k], int(scans[k]), hiding=bool(flags[k]))
        other = index.get((int(pairs[k]), int(qps[k]), 0))
        if flags[k] and other is not None:
            p = int(pairs[k])
            tags |= hiding_edges(fixture['pair_predictions_%d' % t][p], fixture['pair_targets_%d' % t][p], int(qps[k]), int(scans[k]),
                                 levels[other], levels[k])
    return tags


def fused(lam, d, r):
    """D + lambda R rounded ONCE: what a fused multiply-add returns (exact rational arithmetic, then the one rounding of float())"""
    return float(Fraction(lam) * int(r) + int(d))


def pattern(x):
    return int(np.float64(x).view(np.uint64))


def check_second_pass(hm, device):
    """rd_pass under the fixture's four lambdas: every winner's (lambda, D, R) is a recorded triple and its cost has HM's bits; at least
    one of them differs under a fused multiply-add."""
    from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
    from tests import rd_pass_cases
    first = int(hm['rd_first'])
    table = {key: (int(j), bool(f)) for key, j, f in zip(zip(hm['cost_lambda'][first:].tolist(), hm['cost_d'][first:].tolist(),
                                                              hm['cost_r'][first:].tolist()), hm['cost_j'][first:], hm['cost_fused_differs'][first:])}
    lambdas = hm['rd_lambdas'].view(np.float64)
    differing = 0
    for flag in (False, True):
        res = ip.rd_pass(*rd_pass_cases.seeded(RD_WIDTH, RD_BLOCKS), RD_QPS, sign_data_hiding=flag, lambdas=lambdas,
                         device=device)
        rd_pass_cases.assert_conditions(res, "flag %s" % flag)
        assert np.array_equal(res['lambdas'].view(np.uint64), hm['rd_lambdas'])
        for qi in range(len(RD_QPS)):
            for b in range(RD_BLOCKS):
                key = (int(hm['rd_lambdas'][qi]), int(res['sses'][qi, b]), int(res['rates'][qi, b]) >> 15)
                assert key in table, "the winner of block %d at QP %d is not a recorded triple: regenerate the fixture?" % (b, RD_QPS[qi])
                assert pattern(res['best_costs'][qi, b]) == table[key][0], key
                assert pattern(res['costs'][qi, b, res['slots'][qi, b]]) == table[key][0], key
                differing += table[key][1]
    assert differing > 0
