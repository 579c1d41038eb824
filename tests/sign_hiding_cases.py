"""HM's sign-data hiding with RDOQ 0 (include/pnn_hip.h, "sign-data hiding") restated in plain Python / numpy, straight from the
definition: the remainder deltaU, signBitHidingHDQ group by group with its cost table written out, the stages of a block and the rate
under hiding (the restatement of tests/cabac_rate_cases.py minus one bypass bin per qualifying group).  No shared code with
csrc/pnn_trquant.cpp or csrc/pnn_trquant_tables.h.  tests/test_sign_hiding.py pins the host twin to it; tests/test_gpu_sign_hiding.py
takes its blocks and its book-keeping of which rows of the cost table a run has taken."""
import numpy as np

from tests import cabac_rate_cases as cabac
from tests import trquant_cases as tq

INT32_MAX = 2 ** 31 - 1
THRESHOLD = 4
QPS = (0, 22, 37, 51)
# the rows of the cost table, in the order of the definition
ROWS = ('nonzero_up', 'nonzero_first_one_forbidden', 'nonzero_down', 'zero_below_first_forbidden', 'zero_up')


def delta_u(coeffs, qp):
    """xQuant's rounding remainder of every coefficient of a [T, T] unit"""
    log2_t = coeffs.shape[0].bit_length() - 1
    per, rem = qp // 6, qp % 6
    qbits = 14 + per + 7 - log2_t
    tmp = np.abs(coeffs.astype(np.int64)) * tq.QUANT_SCALES[rem]
    mag = (tmp + (171 << (qbits - 9))) >> qbits
    return (tmp - (mag << qbits)) >> (qbits - 8)


def row_of(level, coeff, du, n, first, signbit):
    """(row name, cost, change) of candidate position n"""
    if level != 0:
        if du > 0:
            return 'nonzero_up', -du, 1
        if n == first and abs(level) == 1:
            return 'nonzero_first_one_forbidden', INT32_MAX, None
        return 'nonzero_down', du, -1
    if n < first and (0 if coeff >= 0 else 1) != signbit:
        return 'zero_below_first_forbidden', INT32_MAX, None
    return 'zero_up', -du, 1


def group_span(values):
    """(first, last) of the nonzero entries of 16 levels in scan order; last = -1 without any"""
    nonzero = [n for n, v in enumerate(values) if v != 0]
    return (nonzero[0], nonzero[-1]) if nonzero else (16, -1)


def hide(levels, coeffs, du, scan, taken=None):
    """The levels [T, T] after hiding.  taken: a dictionary that counts, per row of the cost table, the candidates that fell under it
    ('<row>') and the winners it gave ('won:<row>'), over the groups that had to change."""
    levels = np.array(levels, dtype=np.int64)
    t = levels.shape[0]
    order = cabac.grouped_scan(t, scan)                                    # [(x, y)] in scan order
    met_a_level = False
    for c in range(t * t // 16 - 1, -1, -1):
        where = order[16 * c:16 * c + 16]
        values = [int(levels[y, x]) for x, y in where]
        first, last = group_span(values)
        if last < 0:
            continue
        in_last_group = not met_a_level
        met_a_level = True
        if last - first < THRESHOLD:
            continue
        signbit = 0 if values[first] > 0 else 1
        if signbit == sum(values[first:last + 1]) & 1:
            continue
        best = (INT32_MAX, None, None, None)                               # cost, n, change, row
        for n in range(last if in_last_group else 15, -1, -1):
            x, y = where[n]
            row, cost, change = row_of(values[n], int(coeffs[y, x]), int(du[y, x]), n, first, signbit)
            if taken is not None:
                taken[row] = taken.get(row, 0) + 1
            if cost < best[0]:
                best = (cost, n, change, row)
        _, n, change, row = best
        assert n is not None, "a participating group without an allowed candidate"
        if taken is not None:
            taken['won:' + row] = taken.get('won:' + row, 0) + 1
        x, y = where[n]
        if values[n] in (32767, -32768):
            change = -1
        levels[y, x] = values[n] + change if coeffs[y, x] >= 0 else values[n] - change
    return levels


def qualifying_groups(levels, scan):
    """The number of groups of a unit whose first and last nonzero scan positions are at least 4 apart"""
    t = levels.shape[0]
    order = cabac.grouped_scan(t, scan)
    count = 0
    for c in range(t * t // 16):
        first, last = group_span([int(levels[y, x]) for x, y in order[16 * c:16 * c + 16]])
        count += last - first >= THRESHOLD
    return count


def rate(levels, scan, qp):
    """Bits * 2^15 of one unit's (final) levels when the hidden signs are not coded"""
    return cabac.rate(levels, scan, qp) - cabac.BYPASS * qualifying_groups(np.asarray(levels), scan)


def units_of(w):
    t = min(w, 32)
    return [(slice(uy, uy + t), slice(ux, ux + t)) for uy in range(0, w, t) for ux in range(0, w, t)]


def stages(prediction, target, qp, scan, taken=None):
    """One block [w, w] uint8 under sign-data hiding: transform_stages' dictionary plus 'magnitudes', 'reconstruction' and 'rate'"""
    w = target.shape[0]
    names = ('coeffs', 'levels', 'magnitudes', 'delta_u', 'levels_hidden', 'dequant', 'residual')
    out = {name: np.zeros((w, w), np.int64) for name in names}
    out['rate'] = 0
    for unit in units_of(w):
        c = tq.forward(target[unit].astype(np.int64) - prediction[unit].astype(np.int64))
        levels, mag = tq.quantise(c, qp)
        du = delta_u(c, qp)
        hidden = hide(levels, c, du, scan, taken)
        d = tq.dequantise(hidden, qp, c.shape[0].bit_length() - 1)
        out['coeffs'][unit], out['levels'][unit], out['magnitudes'][unit], out['delta_u'][unit] = c, levels, mag, du
        out['levels_hidden'][unit], out['dequant'][unit], out['residual'][unit] = hidden, d, tq.inverse(d)
        out['rate'] += rate(hidden, scan, qp)
    out['reconstruction'] = np.clip(prediction.astype(np.int64) + out['residual'], 0, 255)
    return out


def book_keeping(levels, hidden, coeffs, du, scan, taken):
    """The same counts as hide(taken=...) makes, but read off somebody else's output: the groups of ONE unit whose `hidden` differs
    from `levels` are the ones that had to change; their candidates are classified from `levels`, the winner is where they differ.
    Returns the number of changed groups."""
    t = levels.shape[0]
    order = cabac.grouped_scan(t, scan)
    met_a_level, changed = False, 0
    for c in range(t * t // 16 - 1, -1, -1):
        where = order[16 * c:16 * c + 16]
        values = [int(levels[y, x]) for x, y in where]
        first, last = group_span(values)
        if last < 0:
            continue
        in_last_group = not met_a_level
        met_a_level = True
        differing = [n for n, (x, y) in enumerate(where) if hidden[y, x] != levels[y, x]]
        if not differing:
            continue
        changed += 1
        signbit = 0 if values[first] > 0 else 1
        for n in range(last if in_last_group else 15, -1, -1):
            x, y = where[n]
            row = row_of(values[n], int(coeffs[y, x]), int(du[y, x]), n, first, signbit)[0]
            taken[row] = taken.get(row, 0) + 1
            if n == differing[0]:
                taken['won:' + row] = taken.get('won:' + row, 0) + 1
    return changed


def dense_pairs(w, n, seed):
    """n predictions against unrelated targets: dense residuals, whose groups have the wrong parity about half the time"""
    return tq.random_pairs(w, n, seed)
