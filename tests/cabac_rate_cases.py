"""The CABAC rate of include/pnn_hip.h ("the CABAC rate of the coded levels") restated in plain Python / numpy, straight from the
definition and in codeCoeffNxN's own order of syntax elements: scans by the literal rule, every table written out again, no shared code
with csrc/pnn_cabac_tables.h.  tests/test_cabac_rate.py pins the host twin to it; tests/test_gpu_cabac_rate.py takes its level sets."""
import numpy as np

DIAG, HOR, VER = 0, 1, 2
SIZES = (4, 8, 16, 32)
QPS = (0, 22, 37, 51)
BYPASS = 32768

# I-slice initial values (H.265 tables 9-27 .. 9-32, luma)
INIT_LAST = (110, 110, 124, 125, 140, 153, 125, 127, 140, 109, 111, 143, 127, 111, 79)          # x and y alike
INIT_GROUP = (91, 171)
INIT_SIG = (111, 111, 125, 110, 110, 94, 124, 108, 124, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179,
            153, 125, 141)
INIT_ONE = (140, 92, 137, 138, 140, 152, 138, 139, 153, 74, 149, 92, 139, 107, 122, 152)
INIT_ABS = (138, 153, 136, 167)

# HM's ContextModel::m_entropyBits (FAST_BIT_EST), indexed by state ^ bin with state = 2 pStateIdx + valMps
ENTROPY_BITS = (
    0x07b23, 0x085f9, 0x074a0, 0x08cbc, 0x06ee4, 0x09354, 0x067f4, 0x09c1b, 0x060b0, 0x0a62a, 0x05a9c, 0x0af5b, 0x0548d, 0x0b955, 0x04f56,
    0x0c2a9, 0x04a87, 0x0cbf7, 0x045d6, 0x0d5c3, 0x04144, 0x0e01b, 0x03d88, 0x0e937, 0x039e0, 0x0f2cd, 0x03663, 0x0fc9e, 0x03347, 0x10600,
    0x03050, 0x10f95, 0x02d4d, 0x11a02, 0x02ad3, 0x12333, 0x0286e, 0x12cad, 0x02604, 0x136df, 0x02425, 0x13f48, 0x021f4, 0x149c4, 0x0203e,
    0x1527b, 0x01e4d, 0x15d00, 0x01c99, 0x166de, 0x01b18, 0x17017, 0x019a5, 0x17988, 0x01841, 0x18327, 0x016df, 0x18d50, 0x015d9, 0x19547,
    0x0147c, 0x1a083, 0x0138e, 0x1a8a3, 0x01251, 0x1b418, 0x01166, 0x1bd27, 0x01068, 0x1c77b, 0x00f7f, 0x1d18e, 0x00eda, 0x1d91a, 0x00e19,
    0x1e254, 0x00d4f, 0x1ec9a, 0x00c90, 0x1f6e0, 0x00c01, 0x1fef8, 0x00b5f, 0x208b1, 0x00ab6, 0x21362, 0x00a15, 0x21e46, 0x00988, 0x2285d,
    0x00934, 0x22ea8, 0x008a8, 0x239b2, 0x0081d, 0x24577, 0x007c9, 0x24ce6, 0x00763, 0x25663, 0x00710, 0x25e8f, 0x006a0, 0x26a26, 0x00672,
    0x26f23, 0x005e8, 0x27ef8, 0x005ba, 0x284b5, 0x0055e, 0x29057, 0x0050c, 0x29bab, 0x004c1, 0x2a674, 0x004a7, 0x2aa5e, 0x0046f, 0x2b32f,
    0x0041f, 0x2c0ad, 0x003e7, 0x2ca8d, 0x003ba, 0x2d323, 0x0010c, 0x3bfbb)
# H.265 table 9-41
TRANS_IDX_LPS = (0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24, 24,
                 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63)
CTX_IDX_MAP_4X4 = ((0, 1, 4, 5), (2, 3, 4, 5), (6, 6, 8, 8), (7, 7, 8, 8))                     # [y][x]
LAST_GROUP = (0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7) + (8,) * 8 + (9,) * 8


class Context:
    """One context model: H.265 9.3.2.2 at start, 9.3.4.3.2 per bin, HM's fractional bits."""
    def __init__(self, init_value, qp):
        slope, offset = (init_value >> 4) * 5 - 45, ((init_value & 15) << 3) - 16
        pre = min(max(1, ((slope * qp) >> 4) + offset), 126)
        self.mps = int(pre >= 64)
        self.p = pre - 64 if self.mps else 63 - pre

    def code(self, value):
        bits = ENTROPY_BITS[(2 * self.p + self.mps) ^ value]
        if value == self.mps:
            self.p = min(self.p + 1, 62)
        else:
            if self.p == 0:
                self.mps = 1 - self.mps
            self.p = TRANS_IDX_LPS[self.p]
        return bits


def plain_scan(n, scan):
    """[(x, y)] of an n x n array: rows, columns, or up-right diagonals starting at the top left"""
    if scan == HOR:
        return [(x, y) for y in range(n) for x in range(n)]
    if scan == VER:
        return [(x, y) for x in range(n) for y in range(n)]
    order = []
    for d in range(2 * n - 1):
        for y in range(min(d, n - 1), -1, -1):               # from the bottom left of the diagonal up to the right
            if d - y < n:
                order.append((d - y, y))
    return order


def grouped_scan(t, scan):
    """[(x, y)] of a t x t unit: its 4 x 4 groups in `scan` order, each group's 16 positions in `scan` order"""
    return [(4 * gx + x, 4 * gy + y) for gx, gy in plain_scan(t // 4, scan) for x, y in plain_scan(4, scan)]


def scan_of_mode(t, mode):
    if t > 8 or mode is None:
        return DIAG
    return HOR if abs(mode - 26) <= 4 else VER if abs(mode - 10) <= 4 else DIAG


def remaining_bins(value, rice):
    """the bins of coeff_abs_level_remaining: a unary prefix of up to 3 and `rice` bits, or 3 ones, an Exp-Golomb prefix and its suffix"""
    if value < (3 << rice):
        return (value >> rice) + 1 + rice
    length, value = rice, value - (3 << rice)
    while value >= (1 << length):
        value -= 1 << length
        length += 1
    return (3 + length + 1 - rice) + length


def sig_context(t, scan, pattern, x, y):
    """The index, among the 28 luma sig_coeff_flag contexts, of position (x, y) of a t x t unit whose group has the coded neighbours
    `pattern` = (right group coded) + 2 (lower group coded)"""
    if x + y == 0:
        return 0
    if t == 4:
        return CTX_IDX_MAP_4X4[y][x]
    first = (9 if scan == DIAG else 15) if t == 8 else 21
    px, py = x & 3, y & 3
    if pattern == 0:
        cnt = 0 if px + py >= 3 else 1 if px + py >= 1 else 2
    elif pattern == 1:
        cnt = 0 if py >= 2 else 1 if py >= 1 else 2
    elif pattern == 2:
        cnt = 0 if px >= 2 else 1 if px >= 1 else 2
    else:
        cnt = 2
    return first + (3 if (x >> 2) + (y >> 2) > 0 else 0) + cnt


def coded_neighbours(group_coded, gx, gy, wg):
    """(right, below): whether the groups to the right of and below group (gx, gy) of wg x wg hold a level"""
    return bool(gx < wg - 1 and group_coded[(gx + 1, gy)]), bool(gy < wg - 1 and group_coded[(gx, gy + 1)])


def rate(levels, scan, qp, trace=None):
    """Bits * 2^15 of one unit's levels [T, T] (rows y, columns x).  trace: a list that receives (name, context index or None, bin)."""
    levels = np.asarray(levels).astype(np.int64)
    t = levels.shape[0]
    log2 = t.bit_length() - 1
    if not levels.any():
        return 0
    ctx = {'last_x': [Context(v, qp) for v in INIT_LAST], 'last_y': [Context(v, qp) for v in INIT_LAST],
           'group': [Context(v, qp) for v in INIT_GROUP], 'sig': [Context(v, qp) for v in INIT_SIG],
           'one': [Context(v, qp) for v in INIT_ONE], 'abs': [Context(v, qp) for v in INIT_ABS]}
    total = 0

    def coded(name, index, value):
        nonlocal total
        total += ctx[name][index].code(int(value))
        if trace is not None:
            trace.append((name, index, int(value)))

    def bypass(count, name):
        nonlocal total
        total += BYPASS * count
        if trace is not None:
            trace.extend([(name, None, None)] * count)

    order = grouped_scan(t, scan)
    groups = plain_scan(t // 4, scan)
    wg = t // 4
    last = max(i for i, (x, y) in enumerate(order) if levels[y, x] != 0)
    group_coded = {(gx, gy): bool(levels[4 * gy:4 * gy + 4, 4 * gx:4 * gx + 4].any()) for gx, gy in groups}

    # 1. the last significant position
    lx, ly = order[last]
    if scan == VER:
        lx, ly = ly, lx
    offset, shift = 3 * (log2 - 2) + ((log2 - 1) >> 2), (log2 + 1) >> 2
    for name, pos in (('last_x', lx), ('last_y', ly)):
        g = LAST_GROUP[pos]
        for k in range(g):
            coded(name, offset + (k >> shift), 1)
        if g < LAST_GROUP[t - 1]:
            coded(name, offset + (g >> shift), 0)
    for pos in (lx, ly):
        if LAST_GROUP[pos] > 3:
            bypass((LAST_GROUP[pos] - 2) >> 1, 'last_suffix')

    # 2. the groups, from the last one back
    last_set = last >> 4
    c1 = 1
    for s in range(last_set, -1, -1):
        gx, gy = groups[s]
        right, below = coded_neighbours(group_coded, gx, gy, wg)
        if s != last_set and s != 0:
            coded('group', int(right or below), group_coded[(gx, gy)])
        if not (group_coded[(gx, gy)] or s == 0):
            continue
        pattern = int(right) + 2 * int(below)
        found = []                                          # the group's levels in coding order
        top = 16 * s + 15
        if s == last_set:
            found.append(int(levels[order[last][1], order[last][0]]))
            top = last - 1
        for i in range(top, 16 * s - 1, -1):
            x, y = order[i]
            sig = levels[y, x] != 0
            if i > 16 * s or s == 0 or found:               # else: the group is flagged and nothing else is set, so this one is
                index = sig_context(t, scan, pattern, x, y)
                coded('sig', index, sig)
            if sig:
                found.append(int(levels[y, x]))
        if not found:
            continue
        magnitudes = [abs(v) for v in found]
        ctx_set = (2 if s > 0 else 0) + int(c1 == 0)
        c1 = 1
        first_greater1 = None
        for idx, a in enumerate(magnitudes[:8]):
            coded('one', 4 * ctx_set + c1, a > 1)
            if a > 1:
                c1 = 0
                if first_greater1 is None:
                    first_greater1 = idx
            elif 0 < c1 < 3:
                c1 += 1
        if first_greater1 is not None:
            coded('abs', ctx_set, magnitudes[first_greater1] > 2)
        bypass(len(found), 'sign')
        rice, first2 = 0, 1
        for idx, a in enumerate(magnitudes):
            base = 2 + first2 if idx < 8 else 1
            if a >= base:
                bypass(remaining_bins(a - base, rice), 'remaining')
                if a > (3 << rice):
                    rice = min(rice + 1, 4)
            if a >= 2:
                first2 = 0
    return total


def level_sets(t, seed):
    """A dozen level arrays [T, T] int32: sparse, dense and extreme, +-32767 / -32768 included"""
    rng = np.random.default_rng(seed)
    out = []
    for density in (0.02, 0.1, 0.5):
        keep = rng.random((t, t)) < density
        out.append(np.where(keep, rng.integers(-3, 4, (t, t)), 0))
    yy, xx = np.mgrid[0:t, 0:t]
    out.append(np.where(yy + xx < max(2, t // 3), rng.integers(-40, 41, (t, t)), 0))                  # a low-frequency corner
    out.append(rng.integers(-2, 3, (t, t)))                                                           # dense and small
    out.append(rng.integers(-300, 301, (t, t)))                                                       # dense: every Rice parameter
    out.append(rng.choice(np.array([-32768, -32767, 32767, 0, 1, -1]), (t, t)))                        # the longest escape codes
    out.append(np.full((t, t), -32768))
    out.append(np.full((t, t), 32767))
    lone = np.zeros((t, t), np.int64)
    lone[t - 1, t - 1] = 1                                                                            # the farthest last position
    out.append(lone)
    lone = np.zeros((t, t), np.int64)
    lone[rng.integers(0, t), rng.integers(0, t)] = -5
    out.append(lone)
    edge = np.zeros((t, t), np.int64)
    edge[:, 0] = rng.integers(1, 4, t)                                                                # the first column only
    out.append(edge)
    return [np.ascontiguousarray(a.astype(np.int32)) for a in out]


def scans_of(t):
    return (DIAG, HOR, VER) if t <= 8 else (DIAG,)
