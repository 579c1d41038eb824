"""The open-loop transform coding of include/pnn_hip.h ("transform coding") restated in numpy, straight from the definition: int64
matrix products with literal matrices, no shared code with csrc/pnn_trquant.cpp.  tests/test_trquant.py pins the host twin to it;
tests/golden/make_hm_transforms.py uses it to make the inverse transform's inputs.  Plus the seeded blocks both test files code."""
import numpy as np

WIDTHS = (4, 8, 16, 32, 64)
QPS = (0, 17, 22, 27, 32, 37, 51)

# H.265 8.6.4.2, transMatrix: the 32-point core transform; the T-point one is its rows 0, 32 / T, 2 * 32 / T, ... and first T columns
M32 = np.array([
    [ 64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64,  64],
    [ 90,  90,  88,  85,  82,  78,  73,  67,  61,  54,  46,  38,  31,  22,  13,   4,  -4, -13, -22, -31, -38, -46, -54, -61, -67, -73, -78, -82, -85, -88, -90, -90],
    [ 90,  87,  80,  70,  57,  43,  25,   9,  -9, -25, -43, -57, -70, -80, -87, -90, -90, -87, -80, -70, -57, -43, -25,  -9,   9,  25,  43,  57,  70,  80,  87,  90],
    [ 90,  82,  67,  46,  22,  -4, -31, -54, -73, -85, -90, -88, -78, -61, -38, -13,  13,  38,  61,  78,  88,  90,  85,  73,  54,  31,   4, -22, -46, -67, -82, -90],
    [ 89,  75,  50,  18, -18, -50, -75, -89, -89, -75, -50, -18,  18,  50,  75,  89,  89,  75,  50,  18, -18, -50, -75, -89, -89, -75, -50, -18,  18,  50,  75,  89],
    [ 88,  67,  31, -13, -54, -82, -90, -78, -46,  -4,  38,  73,  90,  85,  61,  22, -22, -61, -85, -90, -73, -38,   4,  46,  78,  90,  82,  54,  13, -31, -67, -88],
    [ 87,  57,   9, -43, -80, -90, -70, -25,  25,  70,  90,  80,  43,  -9, -57, -87, -87, -57,  -9,  43,  80,  90,  70,  25, -25, -70, -90, -80, -43,   9,  57,  87],
    [ 85,  46, -13, -67, -90, -73, -22,  38,  82,  88,  54,  -4, -61, -90, -78, -31,  31,  78,  90,  61,   4, -54, -88, -82, -38,  22,  73,  90,  67,  13, -46, -85],
    [ 83,  36, -36, -83, -83, -36,  36,  83,  83,  36, -36, -83, -83, -36,  36,  83,  83,  36, -36, -83, -83, -36,  36,  83,  83,  36, -36, -83, -83, -36,  36,  83],
    [ 82,  22, -54, -90, -61,  13,  78,  85,  31, -46, -90, -67,   4,  73,  88,  38, -38, -88, -73,  -4,  67,  90,  46, -31, -85, -78, -13,  61,  90,  54, -22, -82],
    [ 80,   9, -70, -87, -25,  57,  90,  43, -43, -90, -57,  25,  87,  70,  -9, -80, -80,  -9,  70,  87,  25, -57, -90, -43,  43,  90,  57, -25, -87, -70,   9,  80],
    [ 78,  -4, -82, -73,  13,  85,  67, -22, -88, -61,  31,  90,  54, -38, -90, -46,  46,  90,  38, -54, -90, -31,  61,  88,  22, -67, -85, -13,  73,  82,   4, -78],
    [ 75, -18, -89, -50,  50,  89,  18, -75, -75,  18,  89,  50, -50, -89, -18,  75,  75, -18, -89, -50,  50,  89,  18, -75, -75,  18,  89,  50, -50, -89, -18,  75],
    [ 73, -31, -90, -22,  78,  67, -38, -90, -13,  82,  61, -46, -88,  -4,  85,  54, -54, -85,   4,  88,  46, -61, -82,  13,  90,  38, -67, -78,  22,  90,  31, -73],
    [ 70, -43, -87,   9,  90,  25, -80, -57,  57,  80, -25, -90,  -9,  87,  43, -70, -70,  43,  87,  -9, -90, -25,  80,  57, -57, -80,  25,  90,   9, -87, -43,  70],
    [ 67, -54, -78,  38,  85, -22, -90,   4,  90,  13, -88, -31,  82,  46, -73, -61,  61,  73, -46, -82,  31,  88, -13, -90,  -4,  90,  22, -85, -38,  78,  54, -67],
    [ 64, -64, -64,  64,  64, -64, -64,  64,  64, -64, -64,  64,  64, -64, -64,  64,  64, -64, -64,  64,  64, -64, -64,  64,  64, -64, -64,  64,  64, -64, -64,  64],
    [ 61, -73, -46,  82,  31, -88, -13,  90,  -4, -90,  22,  85, -38, -78,  54,  67, -67, -54,  78,  38, -85, -22,  90,   4, -90,  13,  88, -31, -82,  46,  73, -61],
    [ 57, -80, -25,  90,  -9, -87,  43,  70, -70, -43,  87,   9, -90,  25,  80, -57, -57,  80,  25, -90,   9,  87, -43, -70,  70,  43, -87,  -9,  90, -25, -80,  57],
    [ 54, -85,  -4,  88, -46, -61,  82,  13, -90,  38,  67, -78, -22,  90, -31, -73,  73,  31, -90,  22,  78, -67, -38,  90, -13, -82,  61,  46, -88,   4,  85, -54],
    [ 50, -89,  18,  75, -75, -18,  89, -50, -50,  89, -18, -75,  75,  18, -89,  50,  50, -89,  18,  75, -75, -18,  89, -50, -50,  89, -18, -75,  75,  18, -89,  50],
    [ 46, -90,  38,  54, -90,  31,  61, -88,  22,  67, -85,  13,  73, -82,   4,  78, -78,  -4,  82, -73, -13,  85, -67, -22,  88, -61, -31,  90, -54, -38,  90, -46],
    [ 43, -90,  57,  25, -87,  70,   9, -80,  80,  -9, -70,  87, -25, -57,  90, -43, -43,  90, -57, -25,  87, -70,  -9,  80, -80,   9,  70, -87,  25,  57, -90,  43],
    [ 38, -88,  73,  -4, -67,  90, -46, -31,  85, -78,  13,  61, -90,  54,  22, -82,  82, -22, -54,  90, -61, -13,  78, -85,  31,  46, -90,  67,   4, -73,  88, -38],
    [ 36, -83,  83, -36, -36,  83, -83,  36,  36, -83,  83, -36, -36,  83, -83,  36,  36, -83,  83, -36, -36,  83, -83,  36,  36, -83,  83, -36, -36,  83, -83,  36],
    [ 31, -78,  90, -61,   4,  54, -88,  82, -38, -22,  73, -90,  67, -13, -46,  85, -85,  46,  13, -67,  90, -73,  22,  38, -82,  88, -54,  -4,  61, -90,  78, -31],
    [ 25, -70,  90, -80,  43,   9, -57,  87, -87,  57,  -9, -43,  80, -90,  70, -25, -25,  70, -90,  80, -43,  -9,  57, -87,  87, -57,   9,  43, -80,  90, -70,  25],
    [ 22, -61,  85, -90,  73, -38,  -4,  46, -78,  90, -82,  54, -13, -31,  67, -88,  88, -67,  31,  13, -54,  82, -90,  78, -46,   4,  38, -73,  90, -85,  61, -22],
    [ 18, -50,  75, -89,  89, -75,  50, -18, -18,  50, -75,  89, -89,  75, -50,  18,  18, -50,  75, -89,  89, -75,  50, -18, -18,  50, -75,  89, -89,  75, -50,  18],
    [ 13, -38,  61, -78,  88, -90,  85, -73,  54, -31,   4,  22, -46,  67, -82,  90, -90,  82, -67,  46, -22,  -4,  31, -54,  73, -85,  90, -88,  78, -61,  38, -13],
    [  9, -25,  43, -57,  70, -80,  87, -90,  90, -87,  80, -70,  57, -43,  25,  -9,  -9,  25, -43,  57, -70,  80, -87,  90, -90,  87, -80,  70, -57,  43, -25,   9],
    [  4, -13,  22, -31,  38, -46,  54, -61,  67, -73,  78, -82,  85, -88,  90, -90,  90, -90,  88, -85,  82, -78,  73, -67,  61, -54,  46, -38,  31, -22,  13,  -4],
], dtype=np.int64)
# the 4 x 4 DST-VII of intra luma
DST4 = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], dtype=np.int64)
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)


def matrix(t):
    return DST4 if t == 4 else M32[::32 // t, :t]


def forward(residual):
    """C [T, T] of X [T, T] (rows y, columns x): Y = (X M^T + r1) >> s1, C = (M Y + r2) >> s2"""
    t = residual.shape[0]
    log2_t = t.bit_length() - 1
    m, s1, s2 = matrix(t), log2_t - 1, log2_t + 6
    y = (residual.astype(np.int64) @ m.T + (1 << (s1 - 1) if s1 > 0 else 0)) >> s1
    return (m @ y + (1 << (s2 - 1))) >> s2


def quantise(coeffs, qp):
    """(levels, magnitudes) of C at QP `qp`"""
    log2_t = coeffs.shape[0].bit_length() - 1
    per, rem, ts = qp // 6, qp % 6, 7 - log2_t
    qbits = 14 + per + ts
    mag = (np.abs(coeffs.astype(np.int64)) * QUANT_SCALES[rem] + (171 << (qbits - 9))) >> qbits
    return np.clip(np.sign(coeffs) * mag, -32768, 32767), mag


def dequantise(levels, qp, log2_t):
    per, rem, ts = qp // 6, qp % 6, 7 - log2_t
    rs = 6 - (ts + per)
    v = levels.astype(np.int64) * INV_QUANT_SCALES[rem]
    v = (v + (1 << (rs - 1))) >> rs if rs > 0 else v * (1 << -rs)
    return np.clip(v, -32768, 32767)


def inverse(dequant):
    """R [T, T] of C' [T, T]: Z = clip16((M^T C' + 64) >> 7), R = clip16((Z M + 2048) >> 12)"""
    m = matrix(dequant.shape[0])
    z = np.clip((m.T @ dequant.astype(np.int64) + 64) >> 7, -32768, 32767)
    return np.clip((z @ m + 2048) >> 12, -32768, 32767)


def stages(prediction, target, qp):
    """One block [w, w] uint8: the dictionary of intraprediction.transform_stages plus 'magnitudes' and 'reconstruction', int64 [w, w]"""
    w = target.shape[0]
    t = min(w, 32)
    out = {name: np.zeros((w, w), np.int64) for name in ('coeffs', 'levels', 'magnitudes', 'dequant', 'residual')}
    for uy in range(0, w, t):
        for ux in range(0, w, t):
            unit = (slice(uy, uy + t), slice(ux, ux + t))
            c = forward(target[unit].astype(np.int64) - prediction[unit].astype(np.int64))
            levels, mag = quantise(c, qp)
            d = dequantise(levels, qp, t.bit_length() - 1)
            out['coeffs'][unit], out['levels'][unit], out['magnitudes'][unit], out['dequant'][unit] = c, levels, mag, d
            out['residual'][unit] = inverse(d)
    out['reconstruction'] = np.clip(prediction.astype(np.int64) + out['residual'], 0, 255)
    return out


def code(predictions, targets, qps):
    """transform_code's integer keys (and 'reconstructions_uint8') for blocks [N, w, w] uint8"""
    n, w = targets.shape[0], targets.shape[1]
    res = {'sses_recon': np.zeros((len(qps), n), np.uint32), 'nb_nonzero_levels': np.zeros((len(qps), n), np.uint32),
           'sum_abs_levels': np.zeros((len(qps), n), np.uint32), 'reconstructions_uint8': np.zeros((len(qps), n, w, w), np.uint8)}
    for qi, qp in enumerate(qps):
        for b in range(n):
            s = stages(predictions[b], targets[b], qp)
            res['sses_recon'][qi, b] = ((s['reconstruction'] - targets[b].astype(np.int64)) ** 2).sum()
            res['nb_nonzero_levels'][qi, b] = np.count_nonzero(s['levels'])
            res['sum_abs_levels'][qi, b] = s['magnitudes'].sum()
            res['reconstructions_uint8'][qi, b] = s['reconstruction']
    return res


def extreme_pairs(w):
    """(predictions, targets) [4, w, w]: prediction 0 / target 255, the reverse, a checkerboard of the two, and a zero residual"""
    yy, xx = np.mgrid[0:w, 0:w]
    board = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)
    zero, full = np.zeros((w, w), np.uint8), np.full((w, w), 255, np.uint8)
    flat = np.full((w, w), 97, np.uint8)
    return np.stack([zero, full, board, flat]), np.stack([full, zero, 255 - board, flat])


def random_pairs(w, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, w, w), dtype=np.uint8), rng.integers(0, 256, (n, w, w), dtype=np.uint8)


def smooth_pairs(w, n, seed):
    """Smooth targets; the prediction is the target plus a ramp (and a little noise): residuals that compact, as an intra mode leaves"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:w, 0:w]
    f = rng.uniform(0.02, 0.3, (n, 4, 1, 1))
    tg = 128 + 50 * np.sin(f[:, 0] * xx + f[:, 1] * yy) + 30 * np.cos(f[:, 2] * xx - f[:, 3] * yy)
    g = rng.uniform(-12, 12, (n, 3, 1, 1))
    ramp = g[:, 0] * (xx / w - 0.5) + g[:, 1] * (yy / w - 0.5) + g[:, 2] + rng.integers(-1, 2, (n, w, w))
    targets = np.clip(np.rint(tg), 0, 255).astype(np.uint8)
    return np.clip(np.rint(tg + ramp), 0, 255).astype(np.uint8), targets


def mixed_pairs(w, n, seed):
    """n >= 6 blocks: the extremes and a zero residual first (all within one workgroup of the kernel, beside random ones), then random
    and smooth pairs alternating"""
    p0, t0 = extreme_pairs(w)
    pr, tr = random_pairs(w, n, seed)
    ps, ts = smooth_pairs(w, n, seed + 1)
    pr[1::2], tr[1::2] = ps[1::2], ts[1::2]
    k = min(4, n)
    pr[:k], tr[:k] = p0[:k], t0[:k]
    return pr, tr


# What the GPU tests of the three transform-coding entries (tests/test_gpu_trquant.py, _cabac_rate.py, _sign_hiding.py) share.
# MODES: all three scans and both ends of each angle window (6 .. 14 vertical scan, 22 .. 30 horizontal scan) with their outer neighbours
MODES = (5, 6, 14, 15, 21, 22, 30, 31, 0, 1, 10, 26, 2, 34, 18)


def blocks_per_workgroup(w):
    return 1 if w >= 32 else 1024 // (w * w)              # trquant_blocks_per_workgroup of csrc/pnn_trquant.hip


def specs_of(w, n, nq):
    """(dtype, shape) of the five outputs: sses_recon, nb_nonzero_levels, sum_abs_levels, the reconstructions, the rate (the entry
    without the rate has the first four)"""
    return [(np.uint32, (nq, n))] * 3 + [(np.uint8, (nq, n, w, w)), (np.uint64, (nq, n))]
