"""What the tests of transform skip (tests/test_transform_skip.py on the CPU, tests/test_gpu_transform_skip.py on the GPU; DESIGN.md
section 5p) share: the seeded 4 x 4 blocks and a Python restatement, written from HM-16.15's tree, of what transform skip ADDS to the
transform-coding column -- xTransformSkip's shift, xQuant's arithmetic on those coefficients, xDeQuant, xITransformSkip's shift, the
reconstruction, the flag's bin in codeCoeffNxN and the checkTransformSkip loop of TEncSearch::xRecurIntraCodingLumaQT.  What HM shares
between the two forms is taken from the entries that earlier fixtures pin to HM (sign hiding: ip.sign_hide_levels; RDOQ: ip.rdoq_unit;
the levels' bits: ip.cabac_rate_of_levels; the transformed form: ip.transform_code with the option off); the flag's two bins are HM's own
recorded numbers (tests/golden/hm_transform_skip.npz) and the cbf bins HM's estBit tables (pnn_rdoq_est_bits_host, pinned by
tests/test_hm_rdoq.py), so the restatement holds no table of this project."""
import os

import numpy as np

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests.trquant_cases import MODES, mixed_pairs

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hm_transform_skip.npz")
QP_PAIRS = ((22, 37), (0, 51))           # the QPs the fixture records the flag's bins at
QUANT_SCALE = (26214, 23302, 20560, 18396, 16384, 14564)
INV_QUANT_SCALE = (40, 45, 51, 57, 64, 72)


def blocks(n, seed=4404):
    """(predictions, targets uint8 [n, 4, 4], modes uint8 [n]): the pairs of trquant_cases at width 4; in every third block the prediction
    is replaced by one that leaves a two-valued ("text") or a single-edge residual of a seeded amplitude, which the DST codes badly"""
    predictions, targets = mixed_pairs(4, max(n, 6), seed)
    predictions, targets = np.ascontiguousarray(predictions[:n]), np.ascontiguousarray(targets[:n])
    rng = np.random.RandomState(seed + 1)
    for b in range(2, n, 3):
        a = int(rng.choice((3, 6, 12, 25, 60, 120)))
        if rng.randint(2):
            residual = np.where(rng.randint(2, size=(4, 4)) == 1, a, 0) * (1 if rng.randint(2) else -1)
        else:
            residual = np.zeros((4, 4), np.int64)
            residual[:, rng.randint(1, 4):] = a
            residual = residual if rng.randint(2) else -residual.T
        targets[b] = rng.randint(120, 136, size=(4, 4))
        predictions[b] = np.clip(targets[b].astype(np.int64) - residual, 0, 255)
    modes = np.array([MODES[(b + n) % len(MODES)] for b in range(n)], np.uint8)
    return predictions, targets, modes


def scan_of_mode(mode):
    return 0 if mode is None else 1 if 22 <= mode <= 30 else 2 if 6 <= mode <= 14 else 0


def flag_bins(qp):
    f = np.load(FIXTURE)
    return [int(v) for v in f["flag_bits"][list(f["qps"]).index(qp)]]


def cbf_bins(qp):
    est = np.zeros(184, np.int32)
    assert _lib.lib().pnn_rdoq_est_bits_host(4, qp, est.ctypes.data) == 0
    return [int(est[180]), int(est[181])]                 # blockCbpBits of context 0: a unit at transform depth 1


def skipped_form(prediction, target, mode, qp, sdh, rdoq, lam):
    """One unit's skipped form: (sse, number of levels, uiAbsSum, level bits, reconstruction)"""
    scan = scan_of_mode(mode)
    residual = target.astype(np.int64) - prediction.astype(np.int64)
    coeffs = residual << 5                                                   # xTransformSkip, shift 15 - 8 - 2
    per, rem = qp // 6, qp % 6
    qbits = 14 + per + 5                                                     # QUANT_SHIFT + per + the transform shift
    if rdoq:
        levels, abs_sum = ip.rdoq_unit(coeffs, scan, qp, lam, cbf_ctx=0, sign_data_hiding=sdh)
        levels = levels.astype(np.int64)
    else:
        tmp = np.abs(coeffs) * QUANT_SCALE[rem]
        mag = (tmp + (171 << (qbits - 9))) >> qbits
        delta_u = (tmp - (mag << qbits)) >> (qbits - 8)
        abs_sum = int(mag.sum())
        levels = np.clip(np.where(coeffs < 0, -mag, mag), -32768, 32767)
        if sdh:
            levels = ip.sign_hide_levels(levels, coeffs, delta_u, scan).astype(np.int64)
    shift = 6 - (5 + per)                                                    # IQUANT_SHIFT - QUANT_IQUANT_SHIFT ... of xDeQuant
    v = levels * INV_QUANT_SCALE[rem]
    dequant = np.clip((v + (1 << (shift - 1))) >> shift if shift > 0 else v << -shift, -32768, 32767)
    back = (dequant + 16) >> 5                                               # xITransformSkip
    recon = np.clip(prediction.astype(np.int64) + back, 0, 255)
    sse = int(((recon - target.astype(np.int64)) ** 2).sum())
    nonzero = int((levels != 0).sum())
    bits = ip.cabac_rate_of_levels(levels, scan, qp, sign_data_hiding=sdh) if nonzero else 0
    return sse, nonzero, abs_sum, bits, recon.astype(np.uint8)


def column(predictions, targets, modes, qps, sdh, rdoq, lambdas, option, mode_bits, charge_cbf):
    """The restated column: a dictionary of transform_code's arrays (rate in 2^-15 bit as 'rate') plus 'transform_skip_flags' and, for
    the conditions, 'skipped_cbf', 'transformed_cbf' and 'tie' (both J equal) [nb_qps, n]"""
    n, nq = len(predictions), len(qps)
    plain = ip.transform_code(predictions, targets, qps, keep_reconstructions=True, modes=modes, rate=True, sign_data_hiding=sdh, rdoq=rdoq,
                              lambdas=lambdas if rdoq else None)
    t_rate = np.rint(plain['rate_bits'] * 32768).astype(np.uint64)
    out = {'sses_recon': np.zeros((nq, n), np.uint32), 'nb_nonzero_levels': np.zeros((nq, n), np.uint32),
           'sum_abs_levels': np.zeros((nq, n), np.uint32), 'reconstructions_uint8': np.zeros((nq, n, 4, 4), np.uint8),
           'rate': np.zeros((nq, n), np.uint64), 'transform_skip_flags': np.zeros((nq, n), np.uint8),
           'skipped_cbf': np.zeros((nq, n), bool), 'transformed_cbf': plain['nb_nonzero_levels'] > 0, 'tie': np.zeros((nq, n), bool)}
    for qi, qp in enumerate(qps):
        lam = float(lambdas[qi]) if lambdas is not None else ip.hm_intra_lambda(qp)
        flag, cbf = flag_bins(qp), cbf_bins(qp)
        for b in range(n):
            s_sse, s_nz, s_sum, s_bits, s_recon = skipped_form(predictions[b], targets[b], None if modes is None else int(modes[b]), qp, sdh, rdoq, lam)
            t_sse, t_nz, t_bits = int(plain['sses_recon'][qi, b]), int(plain['nb_nonzero_levels'][qi, b]), int(t_rate[qi, b])
            out['skipped_cbf'][qi, b] = s_nz > 0
            skipped = True
            if option == 2:
                side = 0 if mode_bits is None else int(mode_bits[qi, b])
                r0 = side + (cbf[1 if t_nz else 0] if charge_cbf else 0) + (flag[0] + t_bits if t_nz else 0)
                r1 = side + (cbf[1 if s_nz else 0] if charge_cbf else 0) + (flag[1] + s_bits if s_nz else 0)
                j0 = float(t_sse) + lam * float(r0 >> 15)
                j1 = float(s_sse) + lam * float(r1 >> 15) if s_nz else 1.7e308    # MAX_DOUBLE: forbidden without a level
                skipped = j1 < j0
                out['tie'][qi, b] = j1 == j0
            kept = (s_sse, s_nz, s_sum, flag[1] + s_bits if s_nz else 0, s_recon) if skipped else \
                (t_sse, t_nz, int(plain['sum_abs_levels'][qi, b]), flag[0] + t_bits if t_nz else 0, plain['reconstructions_uint8'][qi, b])
            for key, value in zip(('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'rate', 'reconstructions_uint8'), kept):
                out[key][qi, b] = value
            out['transform_skip_flags'][qi, b] = skipped
    return out


def host_entry(predictions, targets, modes, qps, sdh, rdoq, lambdas, option, mode_bits, charge_cbf, wanted=(True,) * 6):
    """Raw call of pnn_trquant_tskip_host: (rc, [sses, nonzero, sum_abs, recon, rate, ts_flag] with None where not asked for)"""
    import ctypes
    n, nq = len(predictions), len(qps)
    specs = [(np.uint32, (nq, n))] * 3 + [(np.uint8, (nq, n, 4, 4)), (np.uint64, (nq, n)), (np.uint8, (nq, n))]
    outs = [np.full(s, 0xC5, t) if want else None for (t, s), want in zip(specs, wanted)]
    address = lambda a: None if a is None else a.ctypes.data                 # noqa: E731
    rc = _lib.lib().pnn_trquant_tskip_host(
        predictions.ctypes.data, targets.ctypes.data, predictions.shape[1], n, address(modes), (ctypes.c_int * nq)(*qps), nq,
        *[address(o) for o in outs[:5]], int(sdh), int(rdoq), None if lambdas is None else (ctypes.c_double * nq)(*lambdas), option,
        address(mode_bits), int(charge_cbf), address(outs[5]))
    return rc, outs


KEYS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'reconstructions_uint8', 'rate', 'transform_skip_flags')


def seeded_mode_bits(nq, n, seed=77):
    """Mode bits as the second pass charges them: between 1 and 7 bits in 2^-15 bit"""
    return np.random.RandomState(seed).randint(1 << 15, 7 << 15, size=(nq, n)).astype(np.uint32)
