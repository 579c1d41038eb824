"""HEVC intra prediction for the evaluator's best-mode competitor, mirroring the reference's
hevc/intraprediction/intraprediction.py (extract_intra_pattern(s), predict_via_hevc_best_mode,
predict_series_via_hevc_best_mode) and interface.pyx (predict_via_hevc_mode): same names, arguments, return
dtypes and shapes, same exceptions for bad arguments.

predict_via_hevc_mode is the per-block host twin (pnn_hevc_intra_predict_hm, pure host code).  The best-mode search runs
on the GPU (pnn_hevc_best_mode_hm_device: all 35 modes, their SSEs and the winner of n blocks in one launch) through a
model-less context per device; there is no CPU fallback.  PSNRs are recomputed on the host from the integer SSEs with
the reference's float64 expression: SSE / w^2 is exactly numpy.mean of the squared differences, so they match the
reference bit for bit.

HM's reference-sample smoothing, which the reference's extracted predictor left out, is the option `smoothing` of every predictor
here (include/pnn_hip.h): 0 (the default) reproduces the reference's predictor, 1 is HM with StrongIntraSmoothing 0, 2 is HM's
default.  mode_uses_smoothing and smoothed_reference show the decision table and the filtered line.

rd_pass is HM's second intra pass over the first-pass candidates and a candidate prediction (pnn_rd_pass_host / _device): the transform
coding of every candidate and the choice by D + lambda R, hm_intra_lambda its lambda.

Every option (`smoothing`, `rate`, `modes`, `sign_data_hiding`) travels as an argument of ONE C entry per operation, the widest one
(*_hm_*, *_sdh_*), with 0 or NULL for "off"; the narrower entries of include/pnn_hip.h forward to the same bodies with those very
values and are for integrators.
"""
import ctypes

import numpy as np

from . import _lib

NB_MODES = 35
WIDTHS = (4, 8, 16, 32, 64)
_contexts = {}                                  # device -> model-less pnn_ctx


def _address(buffer):
    """The address of a numpy array or a torch tensor; None (a NULL pointer) for None."""
    if buffer is None:
        return None
    return buffer.ctypes.data if isinstance(buffer, np.ndarray) else buffer.data_ptr()


def extract_intra_pattern(channel_uint8, width_target, row_ref, col_ref, tuple_width_height_masks):
    """intraprediction.py:10-101: the (2w+1-mask_h, 2w+1-mask_w, 1) uint8 intra pattern whose first row and column hold the
    channel's samples from (row_ref, col_ref) on; the rest is 255."""
    if channel_uint8.dtype != np.uint8:
        raise TypeError('`channel_uint8.dtype` is not equal to `numpy.uint8`.')
    if channel_uint8.ndim != 3:
        raise ValueError('`channel_uint8.ndim` is not equal to 3.')
    _check_position(width_target, row_ref, col_ref, tuple_width_height_masks)
    height_pattern = 2 * width_target + 1 - tuple_width_height_masks[1]
    width_pattern = 2 * width_target + 1 - tuple_width_height_masks[0]
    intra_pattern_uint8 = np.full((height_pattern, width_pattern, 1), 255, dtype=np.uint8)
    intra_pattern_uint8[:, 0, :] = channel_uint8[row_ref:row_ref + height_pattern, col_ref, :]
    intra_pattern_uint8[0, :, :] = channel_uint8[row_ref, col_ref:col_ref + width_pattern, :]
    return intra_pattern_uint8


def _check_position(width_target, row_ref, col_ref, tuple_width_height_masks):
    if width_target < 0:
        raise ValueError('`width_target` is not positive.')
    if row_ref < 0:
        raise ValueError('`row_ref` is not positive.')
    if col_ref < 0:
        raise ValueError('`col_ref` is not positive.')
    (width_mask_above, height_mask_left) = tuple_width_height_masks
    if width_mask_above < 0 or width_mask_above > width_target or width_mask_above % 4 != 0:
        raise ValueError('`tuple_width_height_masks[0]` does not belong to {0, 4, ..., `width_target`}.')
    if height_mask_left < 0 or height_mask_left > width_target or height_mask_left % 4 != 0:
        raise ValueError('`tuple_width_height_masks[1]` does not belong to {0, 4, ..., `width_target`}.')


def extract_intra_patterns(channels_uint8, width_target, row_refs, col_refs, tuple_width_height_masks):
    """intraprediction.py:103-181, vectorised: [images * positions, 2w+1-mask_h, 2w+1-mask_w, 1] uint8, image-major."""
    if not np.issubdtype(row_refs.dtype, np.integer):
        raise TypeError('`row_refs.dtype` is not smaller than `numpy.integer` in type hierarchy.')
    if not np.issubdtype(col_refs.dtype, np.integer):
        raise TypeError('`col_refs.dtype` is not smaller than `numpy.integer` in type hierarchy.')
    size_row_refs = row_refs.size
    if col_refs.size != size_row_refs:
        raise ValueError('`col_refs.size` is not equal to `row_refs.size`.')
    height_pattern = 2 * width_target + 1 - tuple_width_height_masks[1]
    width_pattern = 2 * width_target + 1 - tuple_width_height_masks[0]
    nb_images = channels_uint8.shape[0]
    intra_patterns_uint8 = np.zeros((nb_images * size_row_refs, height_pattern, width_pattern, 1), dtype=np.uint8)
    if intra_patterns_uint8.shape[0] == 0:
        return intra_patterns_uint8
    # the reference's per-pattern checks, on the first image and the extreme positions
    if channels_uint8.ndim < 4:
        raise IndexError('too many indices for array')
    if channels_uint8.dtype != np.uint8:
        raise TypeError('`channel_uint8.dtype` is not equal to `numpy.uint8`.')
    if channels_uint8.ndim != 4:
        raise ValueError('`channel_uint8.ndim` is not equal to 3.')
    rows, cols = row_refs.astype(np.int64).ravel(), col_refs.astype(np.int64).ravel()
    _check_position(width_target, int(rows.min()), int(cols.min()), tuple_width_height_masks)
    if channels_uint8.shape[3] != 1:
        raise ValueError('could not broadcast: `channels_uint8.shape[3]` is not equal to 1.')
    if rows.max() + height_pattern > channels_uint8.shape[1] or cols.max() + width_pattern > channels_uint8.shape[2]:
        raise ValueError('could not broadcast: an intra pattern does not fit into the channel.')
    out = np.full((nb_images, size_row_refs, height_pattern, width_pattern), 255, dtype=np.uint8)
    out[:, :, :, 0] = channels_uint8[:, rows[:, None] + np.arange(height_pattern), cols[:, None], 0]
    out[:, :, 0, :] = channels_uint8[:, rows[:, None], cols[:, None] + np.arange(width_pattern), 0]
    return out.reshape(intra_patterns_uint8.shape)


SMOOTHINGS = (0, 1, 2)                          # none, HM's [1 2 1] filter, HM's default (the strong filter allowed at w = 32)


def _check_smoothing(smoothing):
    if smoothing not in SMOOTHINGS:
        raise ValueError('`smoothing` does not belong to {0, 1, 2}.')
    return int(smoothing)


def mode_uses_smoothing(width_target, index_mode):
    """HM's decision table (TComPrediction.cpp:39-55): does mode `index_mode` read smoothed reference samples at this width?"""
    rc = _lib.lib().pnn_hevc_mode_uses_smoothing(int(width_target), int(index_mode))
    if rc < 0:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64} or `index_mode` not to [0, 34].')
    return bool(rc)


def smoothed_reference(intra_pattern_uint8, width_target, smoothing):
    """(line uint8 [4w + 1], strong_used bool): the reference samples of a [h, w'] or [h, w', 1] intra pattern, padded and then smoothed
    as `smoothing` says; index 2w is the corner, the left column runs below it (towards index 0), the above row above it."""
    if not isinstance(intra_pattern_uint8, np.ndarray) or intra_pattern_uint8.dtype != np.uint8:
        raise TypeError('`intra_pattern_uint8` is not a `numpy.ndarray` of dtype `numpy.uint8`.')
    pattern = intra_pattern_uint8[..., 0] if intra_pattern_uint8.ndim == 3 else intra_pattern_uint8
    if pattern.ndim != 2:
        raise ValueError('`intra_pattern_uint8` has neither 2 nor 3 dimensions.')
    pattern = np.ascontiguousarray(pattern)
    if width_target not in WIDTHS:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    line = np.zeros(4 * width_target + 1, np.uint8)
    strong = ctypes.c_int(0)
    rc = _lib.lib().pnn_hevc_smoothed_reference_host(pattern.ctypes.data, pattern.shape[0], pattern.shape[1], width_target,
                                                     _check_smoothing(smoothing), line.ctypes.data, ctypes.byref(strong))
    if rc != 0:
        raise ValueError('pnn_hevc_smoothed_reference_host refused the arguments (pattern %dx%d, width %d).'
                         % (pattern.shape[0], pattern.shape[1], width_target))
    return line, bool(strong.value)


def predict_via_hevc_mode(intra_pattern_uint8, width_target, index_mode, smoothing=0):
    """interface.pyx:15-64: the [w, w, 1] uint8 prediction of mode `index_mode` from a [h, w', 1] intra pattern (host twin).
    smoothing: 0 the reference's predictor, 1 / 2 HM's reference-sample smoothing (the argument of pnn_hevc_intra_predict_hm)."""
    if not isinstance(intra_pattern_uint8, np.ndarray):
        raise TypeError('Argument \'intra_pattern_uint8\' has incorrect type (expected numpy.ndarray)')
    if intra_pattern_uint8.ndim != 3:
        raise ValueError('Buffer has wrong number of dimensions (expected 3, got %d)' % intra_pattern_uint8.ndim)
    if intra_pattern_uint8.dtype != np.uint8:
        raise ValueError('Buffer dtype mismatch, expected \'uint8_t\' but got \'%s\'' % intra_pattern_uint8.dtype)
    if index_mode < 0:
        raise OverflowError('can\'t convert negative value to unsigned int')
    if not intra_pattern_uint8.flags.c_contiguous:
        raise ValueError('`intra_pattern_uint8` is not C-contiguous.')
    if intra_pattern_uint8.shape[2] != 1:
        raise ValueError('`intra_pattern_uint8.shape[2]` is not equal to 1.')
    prediction_uint8 = np.zeros((width_target, width_target, 1), dtype=np.uint8)
    rc = _lib.lib().pnn_hevc_intra_predict_hm(intra_pattern_uint8.ctypes.data_as(_lib.u8p), intra_pattern_uint8.shape[0],
                                              intra_pattern_uint8.shape[1], width_target, int(index_mode), _check_smoothing(smoothing),
                                              prediction_uint8.ctypes.data_as(_lib.u8p))
    if rc != 0:
        raise ValueError('hevc_intraprediction refused the arguments (pattern %dx%d, width %d, mode %d).'
                         % (intra_pattern_uint8.shape[0], intra_pattern_uint8.shape[1], width_target, index_mode))
    return prediction_uint8


def psnrs_from_sses(sses, width_target):
    """10 log10(255^2 / (SSE / w^2 + 1e-6)) in float64, tools/tools.py:364-401 term by term (SSE / w^2 == numpy.mean of the
    squared differences, exactly)."""
    mse_float64 = np.asarray(sses, dtype=np.uint64).astype(np.float64) / (width_target * width_target)
    return 10. * np.log10(255. ** 2 / (mse_float64 + 1.e-6))


def _context(device):
    if device not in _contexts:
        L = _lib.lib()
        ctx = ctypes.c_void_p()
        _lib.check(L.pnn_create_empty(ctypes.byref(ctx), ctypes.c_float(0.), device))
        _contexts[device] = ctx
    return _contexts[device]


def best_modes_device(intra_patterns, targets, width_target, best_pred=True, mode_sse=False, device=0, smoothing=0):
    """The GPU search (pnn_hevc_best_mode_hm_device) on torch uint8 tensors already on `device`: patterns [n, h, w'] and targets
    [n, w, w]; smoothing != 0: over HM's smoothed predictions.
    Returns (best index uint8 [n], best SSE int32 [n], best prediction uint8 [n, w, w] or None, SSE of every mode int32 [n, 35]
    or None), torch tensors on `device`, after the stream has finished."""
    import torch
    smoothing = _check_smoothing(smoothing)
    n = targets.shape[0]
    dev = torch.device("cuda", device)
    index = torch.empty(n, dtype=torch.uint8, device=dev)
    sse = torch.empty(n, dtype=torch.int32, device=dev)
    pred = torch.empty((n, width_target, width_target), dtype=torch.uint8, device=dev) if best_pred else None
    all_sse = torch.empty((n, NB_MODES), dtype=torch.int32, device=dev) if mode_sse else None
    stream = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pnn_hevc_best_mode_hm_device(
            _context(device), width_target, intra_patterns.data_ptr(), intra_patterns.shape[1], intra_patterns.shape[2], targets.data_ptr(), n,
            smoothing, index.data_ptr(), sse.data_ptr(), _address(pred), _address(all_sse), ctypes.c_void_p(stream.cuda_stream)),
            _context(device))
    stream.synchronize()
    return index, sse, pred, all_sse


def first_pass_list_size(width_target):
    """K of HM's first-pass candidate list (g_aucIntraModeNumFast_UseMPM): 8, 8, 3, 3, 3 for w = 4 .. 64."""
    k = _lib.lib().pnn_first_pass_list_size(int(width_target))
    if k < 0:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    return k


def _check_mode_hads_arguments(intra_patterns, targets, width_target, candidate_predictions):
    """Shapes of mode_hads_device / mode_hads_host: patterns [n, h, w'], targets [n, w, w], candidate None or [n, w, w]."""
    if width_target not in WIDTHS:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    if len(intra_patterns.shape) != 3 or len(targets.shape) != 3:
        raise ValueError('the intra patterns and the targets must have 3 dimensions.')
    n = targets.shape[0]
    if tuple(targets.shape[1:]) != (width_target, width_target):
        raise ValueError('the target patches are not w x w.')
    if intra_patterns.shape[0] != n:
        raise ValueError('the numbers of intra patterns and target patches differ.')
    if candidate_predictions is not None and tuple(candidate_predictions.shape) != tuple(targets.shape):
        raise ValueError('`candidate_predictions.shape` is not equal to `targets.shape`.')
    return n


def mode_hads_device(intra_patterns, targets, width_target, candidate_predictions=None, device=0, smoothing=0):
    """HM's first intra pass on the GPU (pnn_hevc_mode_hads_hm_device) on torch uint8 tensors already on `device`: patterns [n, h, w'],
    targets [n, w, w], candidate_predictions None or [n, w, w] (the PNN's uint8 predictions, candidate 35).  One launch.
    Returns numpy arrays {'hads_modes': uint32 [n, 35], 'hads_candidate': uint32 [n] or None, 'list_modes': uint8 [n, K],
    'list_costs': uint32 [n, K]}, K = first_pass_list_size(width_target); the list is in ascending cost, the lower index first among
    equal costs.  Costs: TComRdCost::xGetHADs of the predictions `smoothing` selects (0: the reference's predictor, no reference smoothing;
    2: HM's), without HM's mode-bit term."""
    import torch
    smoothing = _check_smoothing(smoothing)
    n = _check_mode_hads_arguments(intra_patterns, targets, width_target, candidate_predictions)
    k = first_pass_list_size(width_target)
    dev = torch.device("cuda", device)
    tensors = (intra_patterns, targets) + (() if candidate_predictions is None else (candidate_predictions,))
    if any(t.dtype != torch.uint8 or not t.is_contiguous() or t.device != dev for t in tensors):
        raise ValueError('the tensors must be contiguous uint8 tensors on the device.')
    hads = torch.empty((n, NB_MODES), dtype=torch.int32, device=dev)
    cand = torch.empty(n, dtype=torch.int32, device=dev) if candidate_predictions is not None else None
    modes = torch.empty((n, k), dtype=torch.uint8, device=dev)
    costs = torch.empty((n, k), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pnn_hevc_mode_hads_hm_device(
            _context(device), width_target, intra_patterns.data_ptr(), intra_patterns.shape[1], intra_patterns.shape[2], targets.data_ptr(), n,
            _address(candidate_predictions), smoothing, hads.data_ptr(), _address(cand), modes.data_ptr(), costs.data_ptr(),
            ctypes.c_void_p(stream.cuda_stream)), _context(device))
    stream.synchronize()
    return {'hads_modes': hads.cpu().numpy().view(np.uint32), 'hads_candidate': None if cand is None else cand.cpu().numpy().view(np.uint32),
            'list_modes': modes.cpu().numpy(), 'list_costs': costs.cpu().numpy().view(np.uint32)}


def mode_hads_host(intra_patterns, targets, width_target, candidate_predictions=None, smoothing=0):
    """mode_hads_device's host twin (pnn_hevc_mode_hads_hm_host; pure host code) on numpy uint8 arrays: same arguments, same dictionary,
    same bits."""
    smoothing = _check_smoothing(smoothing)
    arrays = [intra_patterns, targets] + ([] if candidate_predictions is None else [candidate_predictions])
    if any(not isinstance(a, np.ndarray) or a.dtype != np.uint8 for a in arrays):
        raise TypeError('the arrays must be `numpy.ndarray`s of dtype `numpy.uint8`.')
    n = _check_mode_hads_arguments(intra_patterns, targets, width_target, candidate_predictions)
    k = first_pass_list_size(width_target)
    patterns, targets = np.ascontiguousarray(intra_patterns), np.ascontiguousarray(targets)
    candidate = None if candidate_predictions is None else np.ascontiguousarray(candidate_predictions)
    hads = np.zeros((n, NB_MODES), np.uint32)
    cand = None if candidate is None else np.zeros(n, np.uint32)
    modes, costs = np.zeros((n, k), np.uint8), np.zeros((n, k), np.uint32)
    rc = _lib.lib().pnn_hevc_mode_hads_hm_host(patterns.ctypes.data, patterns.shape[1], patterns.shape[2], targets.ctypes.data, width_target, n,
                                               _address(candidate), smoothing, hads.ctypes.data, _address(cand), modes.ctypes.data,
                                               costs.ctypes.data)
    if rc != 0:
        raise ValueError('pnn_hevc_mode_hads_host refused the arguments (patterns %dx%d, width %d).'
                         % (patterns.shape[1], patterns.shape[2], width_target))
    return {'hads_modes': hads, 'hads_candidate': cand, 'list_modes': modes, 'list_costs': costs}


def predict_series_via_hevc_best_mode(intra_patterns_uint8, targets_uint8, device=0, smoothing=0):
    """intraprediction.py:183-229 on the GPU: (indices uint8 [N], PSNRs float64 [N], predictions uint8 [N, w, w, 1]) of the
    best HEVC intra mode per target (smallest SSE, lowest index among ties; index 0, 0 dB and zeros when no mode beats 0 dB).
    smoothing != 0: the modes predict with HM's reference-sample smoothing."""
    import torch
    smoothing = _check_smoothing(smoothing)
    if targets_uint8.dtype != np.uint8:
        raise TypeError('`array_0_uint8.dtype` is not equal to `numpy.uint8`.')
    if targets_uint8.ndim != 4 or targets_uint8.shape[3] != 1:
        raise ValueError('cannot select an axis to squeeze out which has size not equal to one')
    if intra_patterns_uint8.dtype != np.uint8 or intra_patterns_uint8.ndim != 4:
        raise ValueError('Buffer dtype mismatch or wrong number of dimensions (expected uint8, 4 dimensions)')
    if intra_patterns_uint8.shape[3] != 1:
        raise ValueError('`intra_pattern_uint8.shape[2]` is not equal to 1.')
    nb_targets, width_target = targets_uint8.shape[0], targets_uint8.shape[1]
    if targets_uint8.shape[2] != width_target or width_target not in WIDTHS:
        raise ValueError('the target patches are not w x w with w in {4, 8, 16, 32, 64}.')
    if intra_patterns_uint8.shape[0] < nb_targets:
        raise IndexError('fewer intra patterns than target patches')
    h, w = intra_patterns_uint8.shape[1:3]
    if not (width_target < h <= 2 * width_target + 1 and width_target < w <= 2 * width_target + 1):
        raise ValueError('The height or the width of the intra pattern does not belong to [%d, %d].'
                         % (width_target + 1, 2 * width_target + 1))
    if nb_targets == 0:
        return (np.zeros(0, dtype=np.uint8), np.zeros(0), np.zeros(targets_uint8.shape, dtype=np.uint8))
    dev = torch.device("cuda", device)
    d_patterns = torch.from_numpy(np.ascontiguousarray(intra_patterns_uint8[:nb_targets, :, :, 0])).to(dev)
    d_targets = torch.from_numpy(np.ascontiguousarray(targets_uint8[:, :, :, 0])).to(dev)
    index, sse, pred, _ = best_modes_device(d_patterns, d_targets, width_target, device=device, smoothing=smoothing)
    indices = index.cpu().numpy()
    sses = sse.cpu().numpy().view(np.uint32)
    psnrs = psnrs_from_sses(sses, width_target)
    psnrs[sses == 65025 * width_target * width_target] = 0.          # the reference's start value, never beaten
    return (indices, psnrs, pred.cpu().numpy()[..., None])


def predict_via_hevc_best_mode(intra_pattern_uint8, target_uint8, device=0, smoothing=0):
    """intraprediction.py:231-294 on the GPU: (index int, PSNR numpy.float64, prediction uint8 [w, w, 1])."""
    if target_uint8.dtype != np.uint8:
        raise TypeError('`array_0_uint8.dtype` is not equal to `numpy.uint8`.')
    if target_uint8.ndim != 3 or intra_pattern_uint8.ndim != 3:
        raise ValueError('Buffer has wrong number of dimensions (expected 3)')
    indices, psnrs, predictions = predict_series_via_hevc_best_mode(intra_pattern_uint8[None], target_uint8[None], device, smoothing)
    return (int(indices[0]), psnrs[0], predictions[0])


MAX_TRANSFORM_QPS = 8


def _check_qps(qps):
    """The QP list of the transform coding as a tuple of ints; ValueError unless it holds 1 to 8 integers in [0, 51]."""
    try:
        qps = tuple(qps)
    except TypeError:
        raise ValueError('`qps` is not a sequence of 1 to 8 integers.')
    if not 1 <= len(qps) <= MAX_TRANSFORM_QPS:
        raise ValueError('`qps` does not hold 1 to 8 quantisation parameters.')
    if any(isinstance(q, (bool, np.bool_)) or not isinstance(q, (int, np.integer)) for q in qps):
        raise ValueError('a quantisation parameter is not an integer.')
    if any(q < 0 or q > 51 for q in qps):
        raise ValueError('a quantisation parameter does not belong to [0, 51].')
    return tuple(int(q) for q in qps)


def _blocks_uint8(array_uint8, name):
    """A uint8 [N, w, w] or [N, w, w, 1] numpy array as contiguous [N, w, w]."""
    if not isinstance(array_uint8, np.ndarray) or array_uint8.dtype != np.uint8:
        raise TypeError('`%s` is not a `numpy.ndarray` of dtype `numpy.uint8`.' % name)
    if array_uint8.ndim == 4 and array_uint8.shape[3] == 1:
        array_uint8 = array_uint8[..., 0]
    if array_uint8.ndim != 3 or array_uint8.shape[1] != array_uint8.shape[2] or array_uint8.shape[1] not in WIDTHS:
        raise ValueError('`%s` is not [N, w, w] or [N, w, w, 1] with w in {4, 8, 16, 32, 64}.' % name)
    return np.ascontiguousarray(array_uint8)


_TRANSFORM_SKIP = {'off': 0, 'forced': 1, 'decide': 2}


def transform_code(predictions_uint8, targets_uint8, qps, device=None, keep_reconstructions=False, modes=None, rate=False,
                   sign_data_hiding=False, rdoq=False, lambdas=None, transform_skip='off', mode_bits=None, charge_cbf=True):
    """Open-loop HEVC transform coding of N predictions against their targets (uint8 [N, w, w] or [N, w, w, 1]) at the 1 to 8 QPs of
    `qps` (integers in [0, 51]): HM's residual path, with RDOQ 0 unless `rdoq` is set -- forward transform, quantisation, dequantisation, inverse transform,
    reconstruction -- as include/pnn_hip.h defines it (T = w up to 32, the four 32 x 32 quadrants of the one prediction at w = 64; no
    transform skip; RDOQ, sign-data hiding and the rate are the options below).  device=None runs the host twin (pnn_trquant_rdoq_host),
    an int that GPU (pnn_trquant_rdoq_device: one launch for all blocks and QPs); the bits are the same.  The options below are arguments of these two
    entries -- the rate pointer, the mode pointer, the flag -- NULL or 0 when off, which is what pnn_trquant_host / _device and
    pnn_trquant_rate_host / _device forward to them.
    Returns {'sses_recon', 'nb_nonzero_levels', 'sum_abs_levels': uint32 [nb_qps, N], 'psnrs_recon': float64 [nb_qps, N] (psnrs_from_sses)}
    and, with keep_reconstructions, 'reconstructions_uint8' [nb_qps, N, w, w].
    rate=True adds 'rate_bits', float64 [nb_qps, N]: the bits HM's CABAC counter reports for the levels of each block's transform
    unit(s) from the I-slice initial contexts of the QP (include/pnn_hip.h, "the CABAC rate of the coded levels"; cbf_luma and mode bits
    not counted) -- the uint64 count the entry writes through its rate pointer, over 32768.  modes (with rate only): uint8 [N] intra modes in
    [0, 34] that pick each block's scan at w = 4 and 8; None codes every block under the diagonal scan.  With rate=False the dictionary
    is the one above.
    sign_data_hiding=True codes the way HM does with SignHideFlag 1 (its default) and RDOQ 0: signBitHidingHDQ between quantisation and
    dequantisation (include/pnn_hip.h, "sign-data hiding"; the entries' flag).  Same keys; nb_nonzero_levels, the
    reconstruction, sses_recon and rate_bits follow the levels after hiding (the hidden signs cost no bin), sum_abs_levels stays the
    sum before it.  `modes` is then allowed without `rate`: the scan shapes the levels.  With False nothing changes.
    rdoq=True quantises the way HM does with RDOQ 1 (include/pnn_hip.h, "rate-distortion optimised quantisation"; the option of
    pnn_trquant_rdoq_host / _device, which every call here goes to, with 0 and NULL when off): xRateDistOptQuant under lambdas -- None
    (hm_intra_lambda of each QP) or one finite value > 0 per QP -- and, with sign_data_hiding, its own hiding.  Same keys, all of them
    those of the levels RDOQ leaves; sum_abs_levels is its uiAbsSum.  `modes` is then allowed too.  `lambdas` without rdoq is a
    ValueError.  With False nothing changes.
    transform_skip (include/pnn_hip.h, "transform skip"; width 4 only, what the reference's configuration does there): 'off', 'forced'
    (every unit in its skipped form) or 'decide' (both forms, HM's choice per unit and QP by D + lambda (R >> 15) under `lambdas` --
    then allowed without rdoq --, R with `mode_bits`, None or integers [nb_qps, N] in 2^-15 bit, and with the cbf_luma bin unless
    charge_cbf is False).  Adds the key 'transform_skip_flags' (uint8 [nb_qps, N]); the other keys are the kept form's, rate_bits with
    the flag's bin.  The calls go to pnn_trquant_tskip_host / _device, which with 'off' forward to the entries above: the same bytes
    and launches.  A width other than 4 with the option on is a ValueError before anything touches the GPU."""
    qps = _check_qps(qps)
    predictions, targets = _blocks_uint8(predictions_uint8, 'predictions_uint8'), _blocks_uint8(targets_uint8, 'targets_uint8')
    if predictions.shape != targets.shape:
        raise ValueError('`predictions_uint8.shape` is not equal to `targets_uint8.shape`.')
    n, w = targets.shape[0], targets.shape[1]
    if transform_skip not in _TRANSFORM_SKIP:
        raise ValueError("`transform_skip` is not 'off', 'forced' or 'decide'.")
    skip = _TRANSFORM_SKIP[transform_skip]
    if skip and w != 4:
        raise ValueError('`transform_skip` is on at a width other than 4.')
    if mode_bits is not None and skip != 2:
        raise ValueError("`mode_bits` is given without `transform_skip` 'decide'.")
    if mode_bits is not None:
        mode_bits = np.asarray(mode_bits)
        if mode_bits.shape != (len(qps), n) or not np.issubdtype(mode_bits.dtype, np.integer) or (n and (mode_bits.min() < 0 or mode_bits.max() >= 2 ** 32)):
            raise ValueError('`mode_bits` is not an array of shape [nb_qps, N] of integers in [0, 2^32).')
        mode_bits = np.ascontiguousarray(mode_bits.astype(np.uint32))
    cbf = int(bool(charge_cbf))
    nq = len(qps)
    c_qps = (ctypes.c_int * nq)(*qps)
    L = _lib.lib()
    flag, option = int(bool(sign_data_hiding)), int(bool(rdoq))
    if lambdas is not None and not option and skip != 2:
        raise ValueError('`lambdas` is given without `rdoq`.')
    c_lambdas = _check_lambdas(lambdas, nq, positive=True)
    if not (rate or flag or option or skip):
        if modes is not None:
            raise ValueError('`modes` is given without `rate`.')
    elif modes is not None:
        modes = np.asarray(modes)
        if modes.shape != (n,) or not np.issubdtype(modes.dtype, np.integer):
            raise ValueError('`modes` is not an integer array of shape [N].')
        if n and (modes.min() < 0 or modes.max() > 34):
            raise ValueError('`modes` has a value outside [0, 34].')
        modes = np.ascontiguousarray(modes.astype(np.uint8))
    if device is None:
        sses, nonzero, sum_abs = (np.zeros((nq, n), np.uint32) for _ in range(3))
        bits = np.zeros((nq, n), np.uint64) if rate else None
        recon = np.zeros((nq, n, w, w), np.uint8) if keep_reconstructions else None
        ts_flags = np.zeros((nq, n), np.uint8) if skip else None
        rc = L.pnn_trquant_tskip_host(predictions.ctypes.data, targets.ctypes.data, w, n, _address(modes), c_qps, nq, sses.ctypes.data,
                                      nonzero.ctypes.data, sum_abs.ctypes.data, _address(recon), _address(bits), flag, option, c_lambdas,
                                      skip, _address(mode_bits), cbf, _address(ts_flags))
        if rc != 0:                                       # (named as the ABI names the call with these options)
            raise ValueError('pnn_trquant_%shost refused the arguments (width %d, %d blocks).'
                             % ('tskip_' if skip else 'rdoq_' if option else 'sdh_' if flag else 'rate_' if rate else '', w, n))
    else:
        import torch
        dev = torch.device("cuda", device)
        d_pred, d_tg = torch.from_numpy(predictions).to(dev), torch.from_numpy(targets).to(dev)
        d_modes = None if modes is None else torch.from_numpy(modes).to(dev)
        d_counts = torch.zeros((3, nq, n), dtype=torch.int32, device=dev)
        d_bits = torch.zeros((nq, n), dtype=torch.int64, device=dev) if rate else None
        d_recon = torch.zeros((nq, n, w, w), dtype=torch.uint8, device=dev) if keep_reconstructions else None
        d_flags = torch.zeros((nq, n), dtype=torch.uint8, device=dev) if skip else None
        d_mode_bits = None if mode_bits is None else torch.from_numpy(mode_bits.view(np.int32)).to(dev)
        ws_bytes = L.pnn_trquant_tskip_workspace_bytes(w, n, nq) if skip else 0
        d_ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes else None
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check(L.pnn_trquant_tskip_device(_context(device), w, d_pred.data_ptr(), d_tg.data_ptr(), n, _address(d_modes), c_qps, nq,
                                                  d_counts[0].data_ptr(), d_counts[1].data_ptr(), d_counts[2].data_ptr(), _address(d_recon),
                                                  _address(d_bits), flag, option, c_lambdas, skip, _address(d_mode_bits), cbf,
                                                  _address(d_flags), _address(d_ws), ws_bytes, ctypes.c_void_p(stream.cuda_stream)),
                       _context(device))
        ts_flags = None if d_flags is None else d_flags.cpu().numpy()
        sses, nonzero, sum_abs = d_counts.cpu().numpy().view(np.uint32)      # (waits for the stream)
        bits = None if d_bits is None else d_bits.cpu().numpy().view(np.uint64)
        recon = None if d_recon is None else d_recon.cpu().numpy()
    result = {'sses_recon': sses, 'nb_nonzero_levels': nonzero, 'sum_abs_levels': sum_abs, 'psnrs_recon': psnrs_from_sses(sses, w)}
    if rate:
        result['rate_bits'] = bits.astype(np.float64) / 32768.
    if keep_reconstructions:
        result['reconstructions_uint8'] = recon
    if skip:
        result['transform_skip_flags'] = ts_flags
    return result


def hm_intra_lambda(qp):
    """HM's lambda of an I slice at QP `qp` (pnn_hm_intra_lambda): 0.57 * 2^((qp - 12) / 3), TEncSlice::calculateLambda for GOP size 1,
    8-bit video, no modifier."""
    return float(_lib.lib().pnn_hm_intra_lambda(int(qp)))


RD_PASS_OUTPUTS = (('candidates', np.uint8), ('costs', np.float64), ('modes', np.uint8), ('slots', np.uint8), ('best_costs', np.float64),
                   ('sses', np.uint32), ('rates', np.uint64))     # the outputs of pnn_rd_pass_*, in the entries' order


def rd_pass_shapes(n, nb_qps, width_target):
    """The shapes of RD_PASS_OUTPUTS for n blocks: candidates [n, K + 1], costs [nb_qps, n, K + 1], the others [nb_qps, n]."""
    k1 = first_pass_list_size(width_target) + 1
    return ((n, k1), (nb_qps, n, k1)) + ((nb_qps, n),) * 5


def _check_lambdas(lambdas, nb_qps, positive=False):
    """None (HM's lambda per QP: a NULL pointer) or nb_qps finite floats >= 0 (> 0 with `positive`: RDOQ divides by them) as a ctypes array."""
    if lambdas is None:
        return None
    values = np.asarray(lambdas, dtype=np.float64).ravel()
    if values.size != nb_qps or not np.all(np.isfinite(values)) or np.any(values < 0.):
        raise ValueError('`lambdas` does not hold one finite value >= 0 per quantisation parameter.')
    if positive and np.any(values <= 0.):
        raise ValueError('`lambdas` holds a value that is not above 0, with `rdoq`.')
    return (ctypes.c_double * nb_qps)(*values)


NO_NEIGHBOUR = 255                                        # a neighbour that does not exist or is not intra: HM takes DC


def _neighbour_array(modes, n, pnn_flag, name):
    """None, or [n] neighbour modes (0 .. 34, 35 with the PNN flag, 255) as a contiguous uint8 array; ValueError otherwise."""
    if modes is None:
        return None
    modes = np.asarray(modes)
    if modes.shape != (n,) or not np.issubdtype(modes.dtype, np.integer):
        raise ValueError('`%s` is not an integer array of shape [n].' % name)
    if n and not np.all((modes == NO_NEIGHBOUR) | ((modes >= 0) & (modes <= (35 if pnn_flag else 34)))):
        raise ValueError('`%s` has a value that is not 0 .. %d or 255.' % (name, 35 if pnn_flag else 34))
    return np.ascontiguousarray(modes.astype(np.uint8))


CODECS = {'switch': 0, 'substitution': 1}                 # the reference's two modified HM codecs, as the ABI's `codec`
SUBSTITUTED_MODE = 18                                     # the mode whose place the candidate takes under 'substitution'
NB_STATS_BINS = 36                                        # modes 0 .. 35 of the mode statistics


def _check_codec(codec, signalling):
    """The codec's name as the ABI's number; 'substitution' needs the signalling."""
    if codec not in CODECS:
        raise ValueError("`codec` is not 'switch' or 'substitution'.")
    if CODECS[codec] and not signalling:
        raise ValueError("the codec 'substitution' needs `signalling`: HM never searches without the mode bits.")
    return CODECS[codec]


def rd_pass_slot_count(width_target, signalling=False, codec='switch'):
    """Slots per block of rd_pass (pnn_rd_pass_codec_slot_count): K + 1, with signalling K + 3; codec 'substitution': K + 2."""
    count = _lib.lib().pnn_rd_pass_codec_slot_count(int(width_target), int(bool(signalling)), _check_codec(codec, signalling))
    if count < 0:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    return count


def rd_pass_mode_stats(candidates, modes, device=None):
    """The mode statistics of a second pass (pnn_rd_pass_mode_stats_host / _device; include/pnn_hip.h, "mode statistics"), the tables
    the reference's codecs accumulate per width.  candidates: rd_pass's 'candidates', uint8 [n, S] (shared by the QPs) or
    [nb_qps, n, S]; modes: its 'modes', uint8 [nb_qps, n].  Returns {'fast_selections', 'fast_wins', 'rd_wins': uint32 [nb_qps, 36]
    (a mode occupies a used slot; is in slot 0; wins), 'modes_for_rd': int64 [nb_qps] (the sum of 'fast_selections':
    m_cumNbModesForRD), 'runs': n (m_nbFastRDRuns)}.  255 -- an unused slot, a block without a winner -- counts nowhere."""
    arrays = (candidates, modes)
    if any(not isinstance(a, np.ndarray) or a.dtype != np.uint8 for a in arrays):
        raise TypeError('the arrays must be `numpy.ndarray`s of dtype `numpy.uint8`.')
    if modes.ndim != 2 or not 1 <= modes.shape[0] <= 8:
        raise ValueError('`modes` is not [nb_qps, n] with 1 to 8 QPs.')
    nq, n = modes.shape
    per_qp = candidates.ndim == 3
    if candidates.ndim not in (2, 3) or candidates.shape[-2] != n or not 1 <= candidates.shape[-1] <= 16 or (per_qp and candidates.shape[0] != nq):
        raise ValueError('`candidates` is not [n, S] or [nb_qps, n, S] with 1 to 16 slots.')
    candidates, modes = np.ascontiguousarray(candidates), np.ascontiguousarray(modes)
    slots = candidates.shape[-1]
    L = _lib.lib()
    if device is None:
        stats = np.zeros((nq, 3, NB_STATS_BINS), np.uint32)
        if L.pnn_rd_pass_mode_stats_host(candidates.ctypes.data, int(per_qp), slots, modes.ctypes.data, n, nq, stats.ctypes.data) != 0:
            raise ValueError('pnn_rd_pass_mode_stats_host refused the arguments.')
    else:
        import torch
        dev = torch.device("cuda", device)
        d_in = [torch.from_numpy(a).to(dev) for a in (candidates, modes)]
        d_stats = torch.empty((nq, 3, NB_STATS_BINS), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check(L.pnn_rd_pass_mode_stats_device(_context(device), _address(d_in[0]) if n else None, int(per_qp), slots,
                                                       _address(d_in[1]) if n else None, n, nq, d_stats.data_ptr(),
                                                       ctypes.c_void_p(stream.cuda_stream)), _context(device))
        stats = d_stats.cpu().numpy().view(np.uint32)     # (waits for the stream)
    return mode_stats_dictionary(stats, n)


def mode_stats_dictionary(stats, n):
    """uint32 [nb_qps, 3, 36] as the entries return it -> rd_pass_mode_stats's dictionary."""
    return {'fast_selections': stats[:, 0].copy(), 'fast_wins': stats[:, 1].copy(), 'rd_wins': stats[:, 2].copy(),
            'modes_for_rd': stats[:, 0].astype(np.int64).sum(axis=1), 'runs': int(n)}


def intra_mode_signal(left_modes, above_modes, qp, pnn_flag=True):
    """The side information of a luma prediction unit as include/pnn_hip.h defines it ("mode signalling"; pnn_intra_mode_signal_host):
    for n blocks whose left and above neighbours were coded with `left_modes` / `above_modes` (integer [n]: 0 .. 34, 35 with
    pnn_flag, 255 = no neighbour or not intra; None: 255 everywhere, but not both None) at QP `qp`,
    {'mpm': uint8 [n, 3] (getIntraDirPredictor of the switch codec), 'num_append': uint8 [n] (how many of them the search appends),
    'mode_frac_bits': uint32 [n, 36] (the bits of coding each mode, in 2^-15 bit; entry 35 is 0 without pnn_flag),
    'cbf_frac_bits': uint32 [2, 2] (cbf_luma: [context][value])}."""
    if left_modes is None and above_modes is None:
        raise ValueError('both `left_modes` and `above_modes` are None.')
    n = len(left_modes if left_modes is not None else above_modes)
    left, above = _neighbour_array(left_modes, n, pnn_flag, 'left_modes'), _neighbour_array(above_modes, n, pnn_flag, 'above_modes')
    if isinstance(qp, (bool, np.bool_)) or not isinstance(qp, (int, np.integer)) or not 0 <= qp <= 51:
        raise ValueError('`qp` is not an integer in [0, 51].')
    mpm, num = np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8)
    bits, cbf = np.zeros((n, 36), np.uint32), np.zeros((2, 2), np.uint32)
    rc = _lib.lib().pnn_intra_mode_signal_host(_address(left), _address(above), n, int(qp), int(bool(pnn_flag)), mpm.ctypes.data, num.ctypes.data,
                                               bits.ctypes.data, cbf.ctypes.data)
    if rc != 0:
        raise ValueError('pnn_intra_mode_signal_host refused the arguments.')
    return {'mpm': mpm, 'num_append': num, 'mode_frac_bits': bits, 'cbf_frac_bits': cbf}


RD_PASS_SIGNAL_OUTPUTS = RD_PASS_OUTPUTS + (('first_pass_costs', np.float64), ('side_rates', np.uint64))


def rd_pass_signal_shapes(n, nb_qps, width_target, codec='switch'):
    """The shapes of RD_PASS_SIGNAL_OUTPUTS: candidates and costs [nb_qps, n, K + 3] (codec 'substitution': K + 2), first_pass_costs
    [nb_qps, n, K], the others [nb_qps, n]."""
    k, s = first_pass_list_size(width_target), rd_pass_slot_count(width_target, True, codec)
    return ((nb_qps, n, s), (nb_qps, n, s)) + ((nb_qps, n),) * 5 + ((nb_qps, n, k), (nb_qps, n))


def _rd_pass_call(arrays, coding, neighbours, options, outputs, shapes, nb_padding, size_function, refused, device):
    """One call of the second pass: pnn_rd_pass_codec_host / _device or, with two `options` (the codec and transform skip),
    pnn_rd_pass_tskip_host / _device -- the host twin with device None or without a block (nothing to launch), else that GPU.
    arrays: contiguous patterns, targets, candidate; coding: the arguments from the smoothing to the signalling; neighbours: (left,
    above), each None or a uint8 array; outputs / shapes: (name, dtype) and shape of each output the call fills, behind which go
    nb_padding NULL outputs; size_function: the scratch's, called with (w, n, nb_qps, signalling, *options); refused: the name in the
    ValueError of a refusal by the host twin.  -> {name: array}."""
    patterns, targets, candidate = arrays
    n, w, (ph, pw) = targets.shape[0], targets.shape[1], patterns.shape[1:3]
    L = _lib.lib()
    entry = 'pnn_rd_pass_tskip_' if len(options) == 2 else 'pnn_rd_pass_codec_'
    padding = (None,) * nb_padding
    if device is None or n == 0:
        outs = [np.zeros(shape, dtype) for (_, dtype), shape in zip(outputs, shapes)]
        rc = getattr(L, entry + 'host')(patterns.ctypes.data, ph, pw, targets.ctypes.data, w, n, candidate.ctypes.data, *coding,
                                        *[_address(a) for a in neighbours], *options, *[o.ctypes.data for o in outs], *padding)
        if rc != 0:
            raise ValueError('%s refused the arguments (patterns %dx%d, width %d).' % (refused, ph, pw, w))
    else:
        import torch
        dev = torch.device("cuda", device)
        d_in = [torch.from_numpy(a).to(dev) for a in arrays]
        d_neighbours = [None if a is None else torch.from_numpy(a).to(dev) for a in neighbours]
        d_outs = [torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device=dev)
                  for (_, dtype), shape in zip(outputs, shapes)]
        nb_bytes = size_function(w, n, coding[2], coding[-1], *options)
        d_ws = torch.empty(max(nb_bytes, 8), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check(getattr(L, entry + 'device')(_context(device), w, d_in[0].data_ptr(), ph, pw, d_in[1].data_ptr(), n, d_in[2].data_ptr(),
                                                    *coding, *[_address(a) for a in d_neighbours], *options, *[o.data_ptr() for o in d_outs],
                                                    *padding, d_ws.data_ptr(), nb_bytes, ctypes.c_void_p(stream.cuda_stream)), _context(device))
        outs = [o.cpu().numpy().view(dtype).reshape(shape) for o, (_, dtype), shape in zip(d_outs, outputs, shapes)]   # (waits)
    return {name: out for (name, _), out in zip(outputs, outs)}


def rd_pass(intra_patterns, targets, candidate_predictions, qps, reference_smoothing=0, sign_data_hiding=False, lambdas=None, device=None,
            rdoq=False, signalling=False, neighbour_modes=None, codec='switch', transform_skip=False):
    """HM's second intra pass as include/pnn_hip.h defines it ("the second intra pass"): per block and QP the RD choice among the
    first-pass candidates (mode_hads_*'s list with the candidate prediction competing as 35) and the candidate itself, appended if the
    list lacks it.  numpy uint8 arrays: patterns [n, h, w'], targets and candidate_predictions [n, w, w]; qps: 1 to 8 integers in
    [0, 51]; lambdas None (hm_intra_lambda of each QP) or one finite value >= 0 per QP.  device=None runs the host twin
    (pnn_rd_pass_host), an int that GPU (pnn_rd_pass_device); the bits are the same.
    Returns {'candidates': uint8 [n, K + 1] (the slots' modes, 255 = unused), 'costs': float64 [nb_qps, n, K + 1] (J = D + lambda R, inf in
    an unused slot), 'modes', 'slots': uint8 [nb_qps, n] (the winner), 'best_costs': float64, 'sses': uint32 (the winner's sse_recon),
    'rates': uint64 (its rate in 2^-15 bit), 'rate_bits': float64 (the same in bits), 'psnrs_recon': float64 (psnrs_from_sses of
    'sses'), each [nb_qps, n], and 'lambdas': float64 [nb_qps], the values used}.
    rdoq=True (the option of pnn_rd_pass_rdoq_host / _device, which every call here goes to, with 0 when off): every candidate is coded
    with HM's RDOQ under the lambda that decides, which must then be > 0.  Same keys.  With False nothing changes.
    signalling=True (the option of pnn_rd_pass_signal_host / _device; include/pnn_hip.h, "mode signalling"): the first pass ranks on
    SATD + modeBits sqrt(lambda), the most probable modes the list lacks are appended in front of 35, and every candidate is charged
    its mode bits and cbf_luma.  neighbour_modes: None (no neighbour anywhere) or a pair (left, above) of integer [n] arrays, each
    None or 0 .. 35 / 255.  The list then depends on the QP: 'candidates' is [nb_qps, n, K + 3], 'costs' [nb_qps, n, K + 3]; 'rates'
    stays the rate of the winner's levels, and the dictionary gains 'side_rates' uint64 [nb_qps, n] (the winner's mode bits plus cbf bin,
    2^-15 bit), 'side_rate_bits' (the same in bits) and 'first_pass_costs' float64 [nb_qps, n, K].  At width 64 each of the four
    quadrants pays its own cbf bin.  With False nothing changes: the same entries are called with signalling 0, which forward to
    pnn_rd_pass_rdoq_host / _device.
    codec='substitution' (the argument of pnn_rd_pass_codec_host / _device, which every call here goes to, with 0 for 'switch';
    include/pnn_hip.h, "the substitution codec"; needs signalling=True): HM's own search over modes 0 .. 34 with the candidate as mode
    18's prediction -- no flag bin, no mode 35, neighbours 0 .. 34 / 255, 'candidates' and 'costs' [nb_qps, n, K + 2]; the winner is the
    candidate where 'modes' is 18.  Same keys.  With 'switch' nothing changes.
    transform_skip=True (pnn_rd_pass_tskip_host / _device; include/pnn_hip.h, "transform skip"; width 4 and signalling=True only, either
    codec; ValueError otherwise, before anything touches the GPU): every slot is coded transformed and transform-skipped and keeps the
    cheaper form by HM's rule before the slots are compared; 'rates' then holds the flag's bin, and the dictionary gains
    'best_transform_skip' uint8 [nb_qps, n], the winning slot's flag.  Every lambda must be > 0.  With False nothing changes: the same
    entries as before are called with the same arguments."""
    if transform_skip and not signalling:
        raise ValueError('`transform_skip` is given without `signalling`.')
    if transform_skip and not (isinstance(targets, np.ndarray) and len(targets.shape) == 3 and targets.shape[1] == 4):
        raise ValueError('`transform_skip` is on at a width other than 4.')
    number = _check_codec(codec, signalling)
    smoothing = _check_smoothing(reference_smoothing)
    qps = _check_qps(qps)
    arrays = (intra_patterns, targets, candidate_predictions)
    if any(not isinstance(a, np.ndarray) or a.dtype != np.uint8 for a in arrays):
        raise TypeError('the arrays must be `numpy.ndarray`s of dtype `numpy.uint8`.')
    if len(targets.shape) != 3 or targets.shape[1] not in WIDTHS:
        raise ValueError('the target patches are not [n, w, w] with w in {4, 8, 16, 32, 64}.')
    w, nq = targets.shape[1], len(qps)
    n = _check_mode_hads_arguments(intra_patterns, targets, w, candidate_predictions)
    patterns, targets, candidate = (np.ascontiguousarray(a) for a in arrays)
    flag, option = int(bool(sign_data_hiding)), int(bool(rdoq))
    c_qps, c_lambdas = (ctypes.c_int * nq)(*qps), _check_lambdas(lambdas, nq, positive=bool(option) or bool(transform_skip))
    if not signalling and neighbour_modes is not None:
        raise ValueError('`neighbour_modes` is given without `signalling`.')
    arrays, coding = (patterns, targets, candidate), (smoothing, c_qps, nq, c_lambdas, flag, option, int(bool(signalling)))
    L = _lib.lib()
    if not signalling:                                    # (the side outputs stay NULL)
        result = _rd_pass_call(arrays, coding, (None, None), (number,), RD_PASS_OUTPUTS, rd_pass_shapes(n, nq, w), 2,
                               L.pnn_rd_pass_codec_workspace_bytes, 'pnn_rd_pass_host', device)
    else:
        left, above = (None, None) if neighbour_modes is None else neighbour_modes
        with_35 = not number                              # a neighbour coded with 35 exists in the switch codec only
        neighbours = (_neighbour_array(left, n, with_35, 'neighbour_modes[0]'), _neighbour_array(above, n, with_35, 'neighbour_modes[1]'))
        outputs, shapes = RD_PASS_SIGNAL_OUTPUTS, rd_pass_signal_shapes(n, nq, w, codec)
        if transform_skip:                                # the option behind the codec, one more output behind the others, a scratch function of its own
            result = _rd_pass_call(arrays, coding, neighbours, (number, 1), outputs + (('best_transform_skip', np.uint8),), shapes + ((nq, n),), 0,
                                   L.pnn_rd_pass_tskip_workspace_bytes, 'pnn_rd_pass_tskip_host', device)
        else:
            result = _rd_pass_call(arrays, coding, neighbours, (number,), outputs, shapes, 0, L.pnn_rd_pass_codec_workspace_bytes,
                                   'pnn_rd_pass_signal_host', device)
        result['side_rate_bits'] = result['side_rates'].astype(np.float64) / 32768.
    result['rate_bits'] = result['rates'].astype(np.float64) / 32768.
    result['psnrs_recon'] = psnrs_from_sses(result['sses'], w)
    result['lambdas'] = np.array([hm_intra_lambda(q) for q in qps]) if c_lambdas is None else np.array(list(c_lambdas))
    return result


SCANS = {'diagonal': 0, 'horizontal': 1, 'vertical': 2}


def _check_scan(scan):
    """A scan, 0, 1, 2 or one of the names of SCANS, as its number."""
    scan = SCANS.get(scan, scan)
    if scan not in (0, 1, 2):
        raise ValueError('`scan` is not 0, 1, 2 or their names.')
    return scan


def _square_integer_array(array, name):
    """An integer [T, T] array, T in {4, 8, 16, 32}, as a numpy array of the dtype it came in."""
    array = np.asarray(array)
    if array.ndim != 2 or array.shape[0] != array.shape[1] or array.shape[0] not in (4, 8, 16, 32) or \
            not np.issubdtype(array.dtype, np.integer):
        raise ValueError('`%s` is not an integer [T, T] array with T in {4, 8, 16, 32}.' % name)
    return array


def _unit_array(array, name):
    """An integer [T, T] array, T in {4, 8, 16, 32}, as contiguous int32."""
    array = _square_integer_array(array, name)
    if array.min() < -2 ** 31 + 1 or array.max() > 2 ** 31 - 1:
        raise ValueError('`%s` has a value that does not fit 32 bits.' % name)
    return np.ascontiguousarray(array.astype(np.int32))


def sign_hide_levels(levels, coeffs, delta_u, scan):
    """HM's TComTrQuant::signBitHidingHDQ on ONE transform unit (pnn_sign_hide_unit_host; include/pnn_hip.h, "sign-data hiding"): the
    levels after hiding, int32 [T, T], given the levels (each in [-32768, 32767]), the coefficients and the rounding remainders deltaU
    -- integer [T, T] arrays, T in {4, 8, 16, 32} -- under scan 0 / 'diagonal', 1 / 'horizontal' or 2 / 'vertical' (diagonal only at
    T = 16 and 32).  The inputs are left as they are."""
    hidden, coeffs, delta_u = _unit_array(levels, 'levels'), _unit_array(coeffs, 'coeffs'), _unit_array(delta_u, 'delta_u')
    if hidden is levels:
        hidden = hidden.copy()
    if not hidden.shape == coeffs.shape == delta_u.shape:
        raise ValueError('`levels`, `coeffs` and `delta_u` differ in shape.')
    if hidden.min() < -32768 or hidden.max() > 32767:
        raise ValueError('`levels` has a value outside [-32768, 32767].')
    scan = _check_scan(scan)
    rc = _lib.lib().pnn_sign_hide_unit_host(hidden.ctypes.data, coeffs.ctypes.data, delta_u.ctypes.data, hidden.shape[0], int(scan))
    if rc != 0:
        raise ValueError('pnn_sign_hide_unit_host refused the arguments (T %d, scan %s).' % (hidden.shape[0], scan))
    return hidden


def rdoq_unit(coeffs, scan, qp, lam=None, cbf_ctx=1, sign_data_hiding=False):
    """HM's TComTrQuant::xRateDistOptQuant on ONE transform unit (pnn_rdoq_unit_host; include/pnn_hip.h, "rate-distortion optimised
    quantisation"): (levels int32 [T, T], uiAbsSum int) of the coefficients -- an integer [T, T] array, T in {4, 8, 16, 32}, each in
    [-32768, 32767] -- under scan 0 / 'diagonal', 1 / 'horizontal' or 2 / 'vertical' (diagonal only at T = 16 and 32) at QP `qp`,
    lambda `lam` (None: hm_intra_lambda(qp); else finite and > 0) and cbf context `cbf_ctx` (0 or 1); sign_data_hiding=True adds RDOQ's
    own hiding."""
    (qp,) = _check_qps((qp,))
    coeffs = _square_integer_array(coeffs, 'coeffs')
    if coeffs.min() < -32768 or coeffs.max() > 32767:
        raise ValueError('`coeffs` has a value outside [-32768, 32767].')
    scan = _check_scan(scan)
    lam = hm_intra_lambda(qp) if lam is None else float(lam)
    if not (np.isfinite(lam) and lam > 0.):
        raise ValueError('`lam` is not finite and above 0.')
    if cbf_ctx not in (0, 1):
        raise ValueError('`cbf_ctx` is not 0 or 1.')
    coeffs = np.ascontiguousarray(coeffs.astype(np.int32))
    levels, abs_sum = np.zeros(coeffs.shape, np.int32), ctypes.c_int32(0)
    rc = _lib.lib().pnn_rdoq_unit_host(coeffs.ctypes.data, coeffs.shape[0], int(scan), qp, lam, int(cbf_ctx), int(bool(sign_data_hiding)),
                                       levels.ctypes.data, ctypes.byref(abs_sum))
    if rc != 0:
        raise ValueError('pnn_rdoq_unit_host refused the arguments (T %d, scan %s, QP %d).' % (coeffs.shape[0], scan, qp))
    return levels, int(abs_sum.value)


def cabac_rate_of_levels(levels, scan, qp, sign_data_hiding=False):
    """The CABAC rate, in units of 2^-15 bit (a Python int), of ONE transform unit given its levels -- an integer [T, T] array, T in
    {4, 8, 16, 32}, each level in [-32768, 32767] -- under scan 0 / 'diagonal', 1 / 'horizontal' or 2 / 'vertical' (diagonal only at
    T = 16 and 32) at QP `qp`: pnn_cabac_rate_levels_sdh_host, the definition at include/pnn_hip.h.  0 for an all-zero unit.
    sign_data_hiding=True (the entry's flag; False is what pnn_cabac_rate_levels_host passes): the rate when the hidden signs are not
    coded -- one bypass bin fewer per group whose first and last nonzero scan positions are at least 4 apart."""
    (qp,) = _check_qps((qp,))
    levels = _square_integer_array(levels, 'levels')
    if levels.min() < -32768 or levels.max() > 32767:     # (before the cast: a value that overflows 32 bits is outside this range too)
        raise ValueError('`levels` has a value outside [-32768, 32767].')
    scan = _check_scan(scan)
    levels = np.ascontiguousarray(levels.astype(np.int32))
    bits = ctypes.c_uint64(0)
    rc = _lib.lib().pnn_cabac_rate_levels_sdh_host(levels.ctypes.data, levels.shape[0], int(scan), qp, int(bool(sign_data_hiding)),
                                                   ctypes.byref(bits))
    if rc != 0:
        raise ValueError('pnn_cabac_rate_levels_host refused the arguments (T %d, scan %s, QP %d).' % (levels.shape[0], scan, qp))
    return int(bits.value)


def transform_stages(prediction_uint8, target_uint8, qp, sign_data_hiding=False, scan=0):
    """Every stage of transform_code for ONE block (uint8 [w, w] or [w, w, 1]) at one QP, host code (pnn_trquant_stages_sdh_host):
    {'coeffs', 'levels', 'dequant', 'residual'}, int32 [w, w] -- the forward transform's coefficients, the quantised levels, the
    dequantised coefficients, the inverse transform's residual; at w = 64 each 32 x 32 unit's array lies where the unit lies.
    sign_data_hiding=True (the entry's flag) hides signs under `scan` (0, 1, 2 or their names; diagonal only at w >= 16) and
    adds 'delta_u', xQuant's rounding remainders, and 'levels_hidden', the levels after hiding, from which 'dequant' and 'residual'
    then come; 'levels' stays the quantiser's output.  `scan` is read with the flag only: without it the entry gets scan 0, the flag 0
    and NULL for the two added arrays, as pnn_trquant_stages_host passes them."""
    (qp,) = _check_qps((qp,))
    blocks = []
    for name, block in (('prediction_uint8', prediction_uint8), ('target_uint8', target_uint8)):
        if isinstance(block, np.ndarray) and block.ndim == 3 and block.shape[2] == 1:
            block = block[..., 0]
        if not isinstance(block, np.ndarray) or block.ndim != 2:
            raise ValueError('`%s` is not a [w, w] or [w, w, 1] `numpy.ndarray`.' % name)
        blocks.append(_blocks_uint8(block[None], name)[0])
    prediction, target = blocks
    if prediction.shape != target.shape:
        raise ValueError('`prediction_uint8.shape` is not equal to `target_uint8.shape`.')
    w = target.shape[0]
    flag = int(bool(sign_data_hiding))
    scan = _check_scan(scan) if flag else 0
    hiding = ('delta_u', 'levels_hidden')
    stages = {name: np.zeros((w, w), np.int32) for name in ('coeffs', 'levels') + (hiding if flag else ()) + ('dequant', 'residual')}
    rc = _lib.lib().pnn_trquant_stages_sdh_host(prediction.ctypes.data, target.ctypes.data, w, qp, int(scan), flag,
                                                stages['coeffs'].ctypes.data, stages['levels'].ctypes.data,
                                                *[_address(stages.get(name)) for name in hiding + ('dequant', 'residual')])
    if rc != 0:
        if flag:
            raise ValueError('pnn_trquant_stages_sdh_host refused the arguments (width %d, QP %d, scan %d).' % (w, qp, scan))
        raise ValueError('pnn_trquant_stages_host refused the arguments (width %d, QP %d).' % (w, qp))
    return stages




CTU_WIDTH = 64                                            # the coding tree (include/pnn_hip.h, "the coding tree"): CTU 64, minimum CU 8
CU_TREE_OUTPUTS = (('cu_depths', np.uint8), ('part_nxn', np.uint8), ('node_costs', np.float64), ('ctu_costs', np.float64),
                   ('ctu_dists', np.uint64), ('ctu_rates', np.uint64), ('selected', np.uint32), ('selected_pnn', np.uint32))


def cu_tree_shapes(nb_qps, n_ctu):
    """The shapes of CU_TREE_OUTPUTS, in the entries' order."""
    return ((nb_qps, n_ctu, 64), (nb_qps, n_ctu, 64), (nb_qps, n_ctu, 85, 2)) + ((nb_qps, n_ctu),) * 3 + ((nb_qps, len(WIDTHS)),) * 2


def z_order_offsets(side):
    """(x, y) of the side^2 cells of a square in HM's z-order (side a power of two): bit 2 j of the index is bit j of x, bit 2 j + 1
    bit j of y."""
    index = np.arange(side * side)
    x, y = np.zeros_like(index), np.zeros_like(index)
    for j in range(max(side.bit_length() - 1, 0)):
        x |= ((index >> (2 * j)) & 1) << j
        y |= ((index >> (2 * j + 1)) & 1) << j
    return x, y


def ctu_block_positions(width_target, ctu_row_1sts, ctu_col_1sts):
    """The positions of every aligned block of width `width_target` inside the listed 64 x 64 CTUs, in (CTU, z-order) order, as the
    `row_1sts` / `col_1sts` the evaluator expects -- the corner of the block's context, block position - width_target --, so that the
    outputs of a second pass over them arrive in the layout of cu_tree's leaves.  ctu_row_1sts / ctu_col_1sts: the CTUs' own top-left
    samples (integers, equally many, >= width_target so that the context exists).  Returns (row_1sts, col_1sts), int64
    [n_ctu * (64 / width_target)^2]."""
    if width_target not in WIDTHS:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    rows, cols = np.asarray(ctu_row_1sts), np.asarray(ctu_col_1sts)
    if rows.ndim != 1 or rows.shape != cols.shape or not (np.issubdtype(rows.dtype, np.integer) and np.issubdtype(cols.dtype, np.integer)):
        raise ValueError('`ctu_row_1sts` and `ctu_col_1sts` are not two integer arrays of one length.')
    if rows.size and (rows.min() < width_target or cols.min() < width_target):
        raise ValueError("a CTU lies closer than `width_target` to the picture's top or left: its first block has no context.")
    x, y = z_order_offsets(CTU_WIDTH // width_target)
    w = width_target
    return ((rows.astype(np.int64)[:, None] + y[None, :] * w - w).ravel(), (cols.astype(np.int64)[:, None] + x[None, :] * w - w).ravel())


def _cu_tree_leaf(leaf, width, nb_qps):
    """One width's leaves as (dist uint32, rate uint64, modes uint8 or None), each [nb_qps, n]; rate = 'rates' + 'side_rates'."""
    if isinstance(leaf, dict):
        missing = [k for k in ('sses', 'rates', 'side_rates', 'modes') if k not in leaf]
        if missing:
            raise ValueError('the leaves of width %d lack %s (rd_pass with signalling=True returns them).' % (width, missing))
        leaf = (leaf['sses'], leaf['rates'], leaf['side_rates'], leaf['modes'])
    if not isinstance(leaf, (tuple, list)) or len(leaf) != 4:
        raise ValueError('the leaves of width %d are not an rd_pass dictionary or (sses, rates, side_rates, modes).' % width)
    sses, rates, side_rates, modes = leaf
    for array, dtype, name in ((sses, np.uint32, 'sses'), (rates, np.uint64, 'rates'), (side_rates, np.uint64, 'side_rates'), (modes, np.uint8, 'modes')):
        if array is None and name == 'modes':
            continue
        if not isinstance(array, np.ndarray) or array.dtype != dtype or array.ndim != 2 or array.shape[0] != nb_qps:
            raise ValueError("`%s` of width %d is not a %s array [nb_qps, n]." % (name, width, np.dtype(dtype).name))
        if array.shape != sses.shape:
            raise ValueError('the leaves of width %d differ in shape.' % width)
    return np.ascontiguousarray(sses), np.ascontiguousarray(rates + side_rates), None if modes is None else np.ascontiguousarray(modes)


def _edge_depths(depths, nb_qps, n_ctu, name):
    if depths is None:
        return None
    depths = np.asarray(depths)
    if depths.shape != (nb_qps, n_ctu, 8) or not np.issubdtype(depths.dtype, np.integer):
        raise ValueError('`%s` is not an integer array [nb_qps, n_ctu, 8].' % name)
    if np.any((depths != NO_NEIGHBOUR) & ((depths < 0) | (depths > 3))):
        raise ValueError('`%s` holds a depth outside 0 .. 3 / 255.' % name)
    return np.ascontiguousarray(depths.astype(np.uint8))


def cu_tree(leaves, qps, lambdas=None, left_depths=None, above_depths=None, pnn_mode=35, device=None):
    """The coding-tree pass as include/pnn_hip.h defines it ("the coding tree"; pnn_cu_tree_host / _device): per QP and 64 x 64 CTU the
    partition HM's recursion (TEncCu::xCompressCU) chooses among the second pass's winners -- split or not at 64, 32 and 16, 2N x 2N
    or N x N at 8 -- its cost, and how many blocks of each width it selects.
    leaves: {4: .., 8: .., 16: .., 32: .., 64: ..}, each an rd_pass(signalling=True) dictionary or (sses, rates, side_rates, modes)
    with modes None allowed; each array [nb_qps, n_ctu * (64 / w)^2], the blocks in (CTU, z-order) order (ctu_block_positions).
    qps: 1 to 8 integers in [0, 51]; lambdas None (hm_intra_lambda of each QP) or one finite value >= 0 per QP; left_depths /
    above_depths None (no neighbouring CTU) or integer [nb_qps, n_ctu, 8], the CU depth 0 .. 3 beside each 8 samples of the CTU's
    left / upper edge, 255 = not available; pnn_mode: the mode that stands for the PNN, 35 (switch codec) or 18 (substitution).
    device=None runs the host twin, an int that GPU; the bits are the same.
    Returns {'cu_depths', 'part_nxn': uint8 [nb_qps, n_ctu, 64] (z-order over the 8 x 8 cells), 'node_costs': float64
    [nb_qps, n_ctu, 85, 2] (unsplit / split, at depth 3 2N x 2N / N x N), 'ctu_costs': float64, 'ctu_dists', 'ctu_rates': uint64
    [nb_qps, n_ctu] (rates in 2^-15 bit), 'selected': uint32 [nb_qps, 5] (blocks of width 4 .. 64 in the chosen partitions),
    'selected_pnn' (those whose mode is pnn_mode; only with modes at every width), 'frequency_selected_pnn': float64 [nb_qps, 5]
    (their share, NaN where a width is never selected; only with modes), 'area_share': float64 [nb_qps, 5] (the share of samples
    coded at each width), 'lambdas': float64 [nb_qps], the values used}."""
    qps = _check_qps(qps)
    nq = len(qps)
    if not isinstance(leaves, dict) or sorted(leaves) != list(WIDTHS):
        raise ValueError('`leaves` is not a dictionary with the keys 4, 8, 16, 32 and 64.')
    if isinstance(pnn_mode, (bool, np.bool_)) or not isinstance(pnn_mode, (int, np.integer)) or not 0 <= pnn_mode <= 255:
        raise ValueError('`pnn_mode` is not an integer in [0, 255].')
    arrays = [_cu_tree_leaf(leaves[w], w, nq) for w in WIDTHS]
    n_ctu = arrays[-1][0].shape[1]
    if n_ctu < 1 or any(a[0].shape[1] != n_ctu * (CTU_WIDTH // w) ** 2 for a, w in zip(arrays, WIDTHS)):
        raise ValueError('the leaves do not hold the blocks of one list of at least one CTU: n_ctu * (64 / w)^2 per width.')
    with_modes = all(a[2] is not None for a in arrays)
    c_qps, c_lambdas = (ctypes.c_int * nq)(*qps), _check_lambdas(lambdas, nq)
    left, above = _edge_depths(left_depths, nq, n_ctu, 'left_depths'), _edge_depths(above_depths, nq, n_ctu, 'above_depths')
    shapes = cu_tree_shapes(nq, n_ctu)
    wanted = [with_modes or name != 'selected_pnn' for name, _ in CU_TREE_OUTPUTS]
    pointers = ctypes.c_void_p * len(WIDTHS)
    L = _lib.lib()
    if device is None:
        outs = [np.zeros(shape, dtype) for (_, dtype), shape in zip(CU_TREE_OUTPUTS, shapes)]
        rc = L.pnn_cu_tree_host(c_qps, nq, c_lambdas, n_ctu, pointers(*[a[0].ctypes.data for a in arrays]),
                                pointers(*[a[1].ctypes.data for a in arrays]), pointers(*[a[2].ctypes.data for a in arrays]) if with_modes else None,
                                _address(left), _address(above), int(pnn_mode), *[o.ctypes.data if want else None for o, want in zip(outs, wanted)])
        if rc != 0:
            raise ValueError('pnn_cu_tree_host refused the arguments.')
    else:
        import torch
        dev = torch.device("cuda", device)
        d_in = [[None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32
                                                         else a).to(dev) for a in triple] for triple in arrays]
        d_edges = [None if a is None else torch.from_numpy(a).to(dev) for a in (left, above)]
        d_outs = [torch.zeros(max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 8), dtype=torch.uint8, device=dev)
                  for (_, dtype), shape in zip(CU_TREE_OUTPUTS, shapes)]
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check(L.pnn_cu_tree_device(_context(device), c_qps, nq, c_lambdas, n_ctu, pointers(*[t[0].data_ptr() for t in d_in]),
                                            pointers(*[t[1].data_ptr() for t in d_in]),
                                            pointers(*[t[2].data_ptr() for t in d_in]) if with_modes else None,
                                            *[None if e is None else e.data_ptr() for e in d_edges], int(pnn_mode),
                                            *[o.data_ptr() if want else None for o, want in zip(d_outs, wanted)],
                                            ctypes.c_void_p(stream.cuda_stream)), _context(device))
        outs = [o.cpu().numpy()[:int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)      # (waits for the stream)
                for o, (_, dtype), shape in zip(d_outs, CU_TREE_OUTPUTS, shapes)]
    return _cu_tree_dictionary(CU_TREE_OUTPUTS, outs, wanted, with_modes, n_ctu, qps, c_lambdas)


def _cu_tree_dictionary(outputs, outs, wanted, with_modes, n_ctu, qps, c_lambdas):
    """The dictionary cu_tree and cu_tree_picture return, from the entry's outputs: the derived shares and the lambdas used join them."""
    result = {name: out for (name, _), out, want in zip(outputs, outs, wanted) if want}
    selected = result['selected'].astype(np.float64)
    if with_modes:
        with np.errstate(invalid='ignore', divide='ignore'):
            result['frequency_selected_pnn'] = np.where(selected > 0, result['selected_pnn'] / selected, np.nan)
    result['area_share'] = selected * np.array([w * w for w in WIDTHS], np.float64) / float(n_ctu * CTU_WIDTH * CTU_WIDTH)
    result['lambdas'] = np.array([hm_intra_lambda(q) for q in qps]) if c_lambdas is None else np.array(list(c_lambdas))
    return result


CU_TREE_PICTURE_OUTPUTS = CU_TREE_OUTPUTS + (('image_dists', np.uint64), ('image_rates', np.uint64))


def cu_tree_picture_shapes(nb_qps, n_images, ctu_rows, ctu_cols):
    """The shapes of CU_TREE_PICTURE_OUTPUTS, in the entries' order."""
    return cu_tree_shapes(nb_qps, n_images * ctu_rows * ctu_cols) + ((nb_qps, n_images),) * 2


def _check_ctu_grid(ctu_rows, ctu_cols, n_images=1):
    for value, name in ((ctu_rows, 'ctu_rows'), (ctu_cols, 'ctu_cols'), (n_images, 'n_images')):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 1:
            raise ValueError('`%s` is not an integer >= 1.' % name)
    if int(n_images) * int(ctu_rows) * int(ctu_cols) > 2 ** 31 - 1:
        raise ValueError('the CTUs of the pictures do not fit an int.')
    return int(ctu_rows), int(ctu_cols), int(n_images)


def ctu_grid(row_1st, col_1st, ctu_rows, ctu_cols):
    """The top-left samples of the ctu_rows x ctu_cols CTUs of a grid whose first CTU starts at sample (row_1st, col_1st), in raster
    order -- the order of cu_tree_picture's CTUs inside an image -- as ctu_block_positions takes them.  Returns (ctu_row_1sts,
    ctu_col_1sts), int64 [ctu_rows * ctu_cols]."""
    ctu_rows, ctu_cols, _ = _check_ctu_grid(ctu_rows, ctu_cols)
    for value, name in ((row_1st, 'row_1st'), (col_1st, 'col_1st')):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 0:
            raise ValueError('`%s` is not an integer >= 0.' % name)
    return (int(row_1st) + CTU_WIDTH * np.repeat(np.arange(ctu_rows, dtype=np.int64), ctu_cols),
            int(col_1st) + CTU_WIDTH * np.tile(np.arange(ctu_cols, dtype=np.int64), ctu_rows))


def hm_context_masks(width_target, ctu_rows, ctu_cols):
    """Context availability (include/pnn_hip.h, "context availability"; pnn_hm_context_masks_host): for every aligned block of width
    `width_target` in a grid of ctu_rows x ctu_cols whole CTUs, the masks HM's z-scan coding order leaves it -- mask_w = 0 where the
    above-right portion is coded before the block, else width_target; mask_h likewise for the below-left portion.  Returns (masks_w,
    masks_h), uint8 [ctu_rows * ctu_cols * (64 / width_target)^2] in (CTU raster, z-order) order: the order of
    ctu_block_positions(width_target, *ctu_grid(row_1st, col_1st, ctu_rows, ctu_cols)).  ValueError for a width outside the five or a
    grid dimension that is not an integer >= 1."""
    if width_target not in WIDTHS:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    ctu_rows, ctu_cols, _ = _check_ctu_grid(ctu_rows, ctu_cols)
    count = ctu_rows * ctu_cols * (CTU_WIDTH // width_target) ** 2
    if count > 2 ** 31 - 1:
        raise ValueError('the blocks of the grid do not fit an int.')
    masks_w, masks_h = np.empty(count, np.uint8), np.empty(count, np.uint8)
    if _lib.lib().pnn_hm_context_masks_host(int(width_target), ctu_rows, ctu_cols, _address(masks_w), _address(masks_h)) != 0:
        raise ValueError('pnn_hm_context_masks_host refused its arguments.')
    return masks_w, masks_h


def _cu_tree_picture_device(device, leaf_pointers, with_modes, qps, c_lambdas, n_images, ctu_rows, ctu_cols, pnn_mode, wanted):
    """pnn_cu_tree_picture_device on leaves that lie on `device` -- leaf_pointers: three lists (dist, rate, mode) of five device
    addresses -- with every output in ONE buffer and one download of it.  Returns CU_TREE_PICTURE_OUTPUTS as numpy arrays."""
    import torch
    dev = torch.device("cuda", device)
    nq = len(qps)
    L = _lib.lib()
    shapes = cu_tree_picture_shapes(nq, n_images, ctu_rows, ctu_cols)
    begin, offset = [], 0
    for (_, dtype), shape in zip(CU_TREE_PICTURE_OUTPUTS, shapes):            # each output at a multiple of 8 bytes
        begin.append(offset)
        offset += (int(np.prod(shape)) * np.dtype(dtype).itemsize + 7) // 8 * 8
    nb_workspace = L.pnn_cu_tree_picture_workspace_bytes(nq, n_images, ctu_rows, ctu_cols)
    pointers = ctypes.c_void_p * len(WIDTHS)
    with torch.cuda.device(dev):
        d_out = torch.zeros(offset, dtype=torch.uint8, device=dev)
        d_workspace = torch.empty(nb_workspace, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _lib.check(L.pnn_cu_tree_picture_device(
            _context(device), (ctypes.c_int * nq)(*qps), nq, c_lambdas, n_images, ctu_rows, ctu_cols, pointers(*leaf_pointers[0]),
            pointers(*leaf_pointers[1]), pointers(*leaf_pointers[2]) if with_modes else None, int(pnn_mode),
            *[d_out.data_ptr() + b if want else None for b, want in zip(begin, wanted)], d_workspace.data_ptr(), nb_workspace,
            ctypes.c_void_p(stream.cuda_stream)), _context(device))
        out = d_out.cpu().numpy()                         # (waits for the stream)
    return [out[b:b + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape).copy()
            for b, (_, dtype), shape in zip(begin, CU_TREE_PICTURE_OUTPUTS, shapes)]


def _cu_tree_picture_dictionary(outs, wanted, with_modes, qps, c_lambdas, n_images, ctu_rows, ctu_cols):
    """cu_tree_picture's dictionary from the entry's ten outputs"""
    result = _cu_tree_dictionary(CU_TREE_PICTURE_OUTPUTS, outs, wanted, with_modes, n_images * ctu_rows * ctu_cols, qps, c_lambdas)
    samples = float(ctu_rows * ctu_cols * CTU_WIDTH * CTU_WIDTH)
    result['image_rate_bits'] = result.pop('image_rates').astype(np.float64) / 32768.
    result['psnr_images'] = 10. * np.log10(255. ** 2 / (result['image_dists'].astype(np.float64) / samples + 1.e-6))
    result['bits_per_pixel_images'] = result['image_rate_bits'] / samples
    return result


def cu_tree_picture(leaves, qps, n_images, ctu_rows, ctu_cols, lambdas=None, pnn_mode=35, device=None):
    """The coding tree over whole pictures as include/pnn_hip.h defines it ("the coding tree over a picture"; pnn_cu_tree_picture_host
    / _device): cu_tree with every CTU's edges taken from the final maps of the CTU left of it and the CTU above it in the same
    image and QP, as HM reads them inside one slice, instead of from the caller.
    leaves, qps, lambdas, pnn_mode, device: as for cu_tree; the blocks of each width in (image, CTU row, CTU column, z-order) order --
    what a second pass over ctu_block_positions(w, *ctu_grid(..)) returns --, n_images * ctu_rows * ctu_cols CTUs in all.
    Returns cu_tree's dictionary and 'image_dists': uint64 [nb_qps, n_images] (the SSE of an image's CTUs under the chosen
    partitions), 'image_rate_bits': float64 [nb_qps, n_images] (their rate in bits), 'psnr_images': float64 (10 log10(255^2 / (SSE /
    (ctu_rows ctu_cols 4096) + 1e-6)), as psnrs_from_sses), 'bits_per_pixel_images': float64 (the bits over the same samples)."""
    qps = _check_qps(qps)
    nq = len(qps)
    ctu_rows, ctu_cols, n_images = _check_ctu_grid(ctu_rows, ctu_cols, n_images)
    if not isinstance(leaves, dict) or sorted(leaves) != list(WIDTHS):
        raise ValueError('`leaves` is not a dictionary with the keys 4, 8, 16, 32 and 64.')
    if isinstance(pnn_mode, (bool, np.bool_)) or not isinstance(pnn_mode, (int, np.integer)) or not 0 <= pnn_mode <= 255:
        raise ValueError('`pnn_mode` is not an integer in [0, 255].')
    arrays = [_cu_tree_leaf(leaves[w], w, nq) for w in WIDTHS]
    n_ctu = n_images * ctu_rows * ctu_cols
    if any(a[0].shape[1] != n_ctu * (CTU_WIDTH // w) ** 2 for a, w in zip(arrays, WIDTHS)):
        raise ValueError('the leaves do not hold the blocks of n_images * ctu_rows * ctu_cols CTUs: n_ctu * (64 / w)^2 per width.')
    with_modes = all(a[2] is not None for a in arrays)
    c_lambdas = _check_lambdas(lambdas, nq)
    shapes = cu_tree_picture_shapes(nq, n_images, ctu_rows, ctu_cols)
    wanted = [with_modes or name != 'selected_pnn' for name, _ in CU_TREE_PICTURE_OUTPUTS]
    if device is None:
        pointers = ctypes.c_void_p * len(WIDTHS)
        outs = [np.zeros(shape, dtype) for (_, dtype), shape in zip(CU_TREE_PICTURE_OUTPUTS, shapes)]
        rc = _lib.lib().pnn_cu_tree_picture_host(
            (ctypes.c_int * nq)(*qps), nq, c_lambdas, n_images, ctu_rows, ctu_cols, pointers(*[a[0].ctypes.data for a in arrays]),
            pointers(*[a[1].ctypes.data for a in arrays]), pointers(*[a[2].ctypes.data for a in arrays]) if with_modes else None,
            int(pnn_mode), *[o.ctypes.data if want else None for o, want in zip(outs, wanted)])
        if rc != 0:
            raise ValueError('pnn_cu_tree_picture_host refused the arguments.')
    else:
        import torch
        dev = torch.device("cuda", device)
        d_in = [[None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32
                                                         else a).to(dev) for a in triple] for triple in arrays]
        leaf_pointers = [[None if t[k] is None else t[k].data_ptr() for t in d_in] for k in range(3)]
        outs = _cu_tree_picture_device(device, leaf_pointers, with_modes, qps, c_lambdas, n_images, ctu_rows, ctu_cols, pnn_mode, wanted)
    return _cu_tree_picture_dictionary(outs, wanted, with_modes, qps, c_lambdas, n_images, ctu_rows, ctu_cols)


def cu_tree_bins(qp):
    """The bins of the coding tree at QP `qp` in 2^-15 bit (pnn_cu_tree_bins_host): {'split': uint32 [3, 2] ([context][value] of
    split_cu_flag), 'part': uint32 [2] (part_mode: [0] N x N, [1] 2N x 2N)}, each from the state an I slice of the QP starts with."""
    out = np.zeros(8, np.uint32)
    if isinstance(qp, (bool, np.bool_)) or not isinstance(qp, (int, np.integer)) or _lib.lib().pnn_cu_tree_bins_host(int(qp), out.ctypes.data) != 0:
        raise ValueError('`qp` is not an integer in [0, 51].')
    return {'split': out[:6].reshape(3, 2).copy(), 'part': out[6:].copy()}
