"""Python-side evaluation of PNN predictions on images, mirroring the PNN half of the reference's
comparing_pnn_ipfcns_hevc_best_mode.py:162-322 (`predict_mask`) without TensorFlow: contexts by the GPU gather
(context.py), predictions by libpnn_hip.so (predict_by_batch_via_pnn), then the reference's own uint8 cast and
PSNR definitions.  predict_mask_vs_hevc_best_mode adds the paper's competitor, the best HEVC intra mode per block
(intraprediction.py: all 35 modes, their SSEs and the winner of every block in one GPU launch), and the reference's
dictionary_performance (indices and PSNRs of the best mode, PNN PSNRs, PNN's win frequency, its mean PSNR).
predict_mask_vs_hevc_best_mode_and_ipfcns adds the third column, IPFCN-S (ipfcns.py: line gather, the four layers and the
uint8 epilogue with the per-block SSE in one GPU call), as the reference does only when nothing is masked.
"""
import numpy as np

from . import context, intraprediction
from .prediction_neural_network import predict_by_batch_via_pnn


def cast_float_to_uint8(array_float):
    """tools/tools.py:12-49: clip to [0, 255], numpy.round (half to even), cast.  (HM itself rounds half away from zero,
    TComPrediction.cpp:632 -- the two differ only on exact .5 values.)"""
    if not np.issubdtype(array_float.dtype, np.floating):
        raise TypeError('`array_float.dtype` is not smaller than `numpy.float` in type hierarchy.')
    return np.round(array_float.clip(min=0., max=255.)).astype(np.uint8)


def compute_psnr(array_0_uint8, array_1_uint8):
    """tools/tools.py:364-401: 10 log10(255^2 / (mse + 1e-6)) in float64."""
    if array_0_uint8.dtype != np.uint8:
        raise TypeError('`array_0_uint8.dtype` is not equal to `numpy.uint8`.')
    if array_1_uint8.dtype != np.uint8:
        raise TypeError('`array_1_uint8.dtype` is not equal to `numpy.uint8`.')
    mse = np.mean((array_0_uint8.astype(np.float64) - array_1_uint8.astype(np.float64)) ** 2)
    return 10. * np.log10(255. ** 2 / (mse + 1.e-6))


def predict_mask(channels_uint8, width_target, row_1sts, col_1sts, predictor, batch_size, mean_training,
                 tuple_width_height_masks=(0, 0)):
    """Predicts the target patch of every (image, position) pair and scores it.

    Returns {'predictions_pnn_uint8': [N,w,w,1], 'targets_uint8': [N,w,w,1], 'psnrs_pnn': [N], 'mean_psnr_pnn': float}
    with N = images x positions, image-major (the order of sets/common.py:213-263)."""
    batches = context.extract_context_portions_targets_from_channels_plus_preprocessing(
        channels_uint8, width_target, row_1sts, col_1sts, mean_training, tuple_width_height_masks,
        predictor.is_fully_connected, predictor=predictor)
    n = batches[0].shape[0]
    if n % batch_size:
        raise ValueError('`numerator` is not divisible by `denominator`.')
    predictions_float32 = predict_by_batch_via_pnn(batches[0:-1], None, predictor, batch_size)
    targets_off = batches[-1] + np.float32(mean_training)
    if np.any(np.modf(targets_off)[0]):
        raise RuntimeError('The target patches have been altered.')      # comparing_pnn_...py:253-254
    targets_uint8 = cast_float_to_uint8(targets_off)
    predictions_uint8 = cast_float_to_uint8(predictions_float32 + np.float32(mean_training))
    psnrs = np.array([compute_psnr(targets_uint8[i], predictions_uint8[i]) for i in range(n)])
    return {'predictions_pnn_uint8': predictions_uint8, 'targets_uint8': targets_uint8, 'psnrs_pnn': psnrs,
            'mean_psnr_pnn': float(np.mean(psnrs))}


def compute_performance_neural_network_vs_hevc_best_mode(targets_uint8, predictions_nn_uint8, psnrs_hevc_best_mode):
    """comparing_pnn_ipfcns_hevc_best_mode.py:39-88: (PSNRs float64 [N] of the network's predictions, frequency with which
    they beat the best HEVC intra mode's)."""
    nb_targets = targets_uint8.shape[0]
    psnrs_nn = np.zeros(nb_targets)
    for i in range(nb_targets):
        psnrs_nn[i] = compute_psnr(np.squeeze(targets_uint8[i, :, :, :], axis=2), np.squeeze(predictions_nn_uint8[i, :, :, :], axis=2))
    frequency_win_nn = float(np.count_nonzero(psnrs_nn - psnrs_hevc_best_mode > 0.)) / nb_targets
    return (psnrs_nn, frequency_win_nn)


def predict_mask_vs_hevc_best_mode(channels_uint8, width_target, row_1sts, col_1sts, predictor, batch_size, mean_training,
                                   tuple_width_height_masks=(0, 0)):
    """predict_mask plus its competitor, as comparing_pnn_ipfcns_hevc_best_mode.py:162-322 scores them: the intra pattern of
    every target (its first row and column start one pixel above-left of the target, i.e. at (row_1st + w - 1,
    col_1st + w - 1)) predicted by the best HEVC intra mode on the GPU.

    Returns the reference's dictionary_performance -- 'indices_hevc_best_mode' [N] uint8, 'psnrs_hevc_best_mode' [N],
    'psnrs_pnn' [N], 'frequency_win_pnn', 'mean_psnr_pnn' -- plus 'predictions_pnn_uint8', 'predictions_hevc_best_mode_uint8'
    and 'targets_uint8' ([N,w,w,1] uint8), N = images x positions, image-major."""
    pnn = predict_mask(channels_uint8, width_target, row_1sts, col_1sts, predictor, batch_size, mean_training,
                       tuple_width_height_masks)
    intra_patterns_uint8 = intraprediction.extract_intra_patterns(channels_uint8, width_target, row_1sts + width_target - 1,
                                                                  col_1sts + width_target - 1, tuple_width_height_masks)
    indices, psnrs_hevc, predictions_hevc = intraprediction.predict_series_via_hevc_best_mode(
        intra_patterns_uint8, pnn['targets_uint8'], device=predictor.device)
    psnrs_pnn, frequency_win_pnn = compute_performance_neural_network_vs_hevc_best_mode(
        pnn['targets_uint8'], pnn['predictions_pnn_uint8'], psnrs_hevc)
    return {'indices_hevc_best_mode': indices, 'psnrs_hevc_best_mode': psnrs_hevc, 'psnrs_pnn': psnrs_pnn,
            'frequency_win_pnn': frequency_win_pnn, 'mean_psnr_pnn': np.mean(psnrs_pnn).item(),
            'predictions_pnn_uint8': pnn['predictions_pnn_uint8'], 'predictions_hevc_best_mode_uint8': predictions_hevc,
            'targets_uint8': pnn['targets_uint8']}


def predict_without_mask_via_ipfcns(channels_uint8, width_target, row_1sts, col_1sts, batch_size, net_ipfcns,
                                    dictionary_performance):
    """comparing_pnn_ipfcns_hevc_best_mode.py:633-711 on the GPU: the reference lines of every target (line origin
    (row_1st + w - 8, col_1st + w - 8)), IPFCN-S, pred = fl32(fc4 + mean), uint8 by rint (half to even) and the SSE against
    dictionary_performance['targets_uint8'] in one call.  FILLS dictionary_performance with 'psnrs_ipfcns' (float64 [N], from
    the integer SSEs by intraprediction.psnrs_from_sses, equal to compute_psnr), 'frequency_win_ipfcns' (against
    'psnrs_hevc_best_mode'), 'mean_psnr_ipfcns' and 'predictions_ipfcns_uint8' [N,w,w,1]."""
    import torch
    targets_uint8 = dictionary_performance['targets_uint8']
    nb_targets = targets_uint8.shape[0]
    if nb_targets % batch_size:
        raise ValueError('`numerator` is not divisible by `denominator`.')
    if net_ipfcns.width_target != width_target:
        raise ValueError('the net is the width-%d IPFCN-S, not the width-%d one' % (net_ipfcns.width_target, width_target))
    if channels_uint8.dtype != np.uint8 or channels_uint8.ndim != 4 or channels_uint8.shape[3] != 1:
        raise ValueError('`channels_uint8` must be uint8 [images, H, W, 1].')
    rows = np.ascontiguousarray(row_1sts + width_target - 8, dtype=np.int32)
    cols = np.ascontiguousarray(col_1sts + width_target - 8, dtype=np.int32)
    if channels_uint8.shape[0] * rows.size != nb_targets:
        raise ValueError('images x positions is not the number of targets.')
    dev = torch.device('cuda', net_ipfcns.device)
    d_channels = torch.from_numpy(np.ascontiguousarray(channels_uint8[..., 0])).to(dev)
    d_targets = torch.from_numpy(np.ascontiguousarray(targets_uint8[..., 0])).to(dev)
    pred_u8, _, _, sses = net_ipfcns.predict_from_channels_device(d_channels, torch.from_numpy(rows).to(dev),
                                                                  torch.from_numpy(cols).to(dev), d_targets)
    psnrs = intraprediction.psnrs_from_sses(sses, width_target)
    dictionary_performance['psnrs_ipfcns'] = psnrs
    dictionary_performance['frequency_win_ipfcns'] = \
        float(np.count_nonzero(psnrs - dictionary_performance['psnrs_hevc_best_mode'] > 0.)) / nb_targets
    dictionary_performance['mean_psnr_ipfcns'] = np.mean(psnrs).item()
    dictionary_performance['predictions_ipfcns_uint8'] = pred_u8[..., None]


def predict_mask_vs_hevc_best_mode_and_ipfcns(channels_uint8, width_target, row_1sts, col_1sts, predictor, batch_size,
                                              mean_training, net_ipfcns, tuple_width_height_masks=(0, 0)):
    """The three columns of the paper's table, as comparing_pnn_ipfcns_hevc_best_mode.py:162-322 fills them:
    predict_mask_vs_hevc_best_mode's dictionary plus, when net_ipfcns is given and nothing is masked (masks == (0, 0)), the
    IPFCN-S keys of predict_without_mask_via_ipfcns."""
    dictionary_performance = predict_mask_vs_hevc_best_mode(channels_uint8, width_target, row_1sts, col_1sts, predictor,
                                                            batch_size, mean_training, tuple_width_height_masks)
    if net_ipfcns is not None and tuple(tuple_width_height_masks) == (0, 0):
        predict_without_mask_via_ipfcns(channels_uint8, width_target, row_1sts, col_1sts, batch_size, net_ipfcns,
                                        dictionary_performance)
    return dictionary_performance
