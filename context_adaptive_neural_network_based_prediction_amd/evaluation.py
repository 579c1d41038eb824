"""Python-side evaluation of PNN predictions on images, mirroring the PNN half of the reference's
comparing_pnn_ipfcns_hevc_best_mode.py:162-322 (`predict_mask`) without TensorFlow: contexts by the GPU gather
(context.py), predictions by libpnn_hip.so (predict_by_batch_via_pnn), then the reference's own uint8 cast and
PSNR definitions.  predict_mask_vs_hevc_best_mode adds the paper's competitor, the best HEVC intra mode per block
(intraprediction.py: all 35 modes, their SSEs and the winner of every block in one GPU launch), and the reference's
dictionary_performance (indices and PSNRs of the best mode, PNN PSNRs, PNN's win frequency, its mean PSNR).
predict_mask_vs_hevc_best_mode_and_ipfcns adds the third column, IPFCN-S (ipfcns.py: line gather, the four layers and the
uint8 epilogue with the per-block SSE in one GPU call), as the reference does only when nothing is masked.
score_masks_from_pictures is the reference's loop over a list of masks (predict_masks, :324-452) on pictures that stay on the
GPU: per mask one pnn_score_pictures_device call (descriptors, PNN pass, uint8 epilogue with its SSE, best-mode search from
the pictures) and one download; the same dictionaries as predict_mask_vs_hevc_best_mode[_and_ipfcns], bit for bit.
score_masks_from_picture_pairs is the same loop on [images, H, W, 2] pairs (original, HEVC-decoded) for the pair models.
Both take first_pass=True for one more column per mask: the PNN and the 35 modes ranked by the Hadamard cost of HM's first intra
pass (pnn_first_pass_picture_pairs_hm_device: one more call per mask, the same download).
Every function with an HEVC column takes reference_smoothing (0, 1, 2: intraprediction's `smoothing`): 0, the default, is the reference's
extracted predictor; 2 makes the HEVC columns and the first-pass ranking those of HM's own predictor, with its reference-sample
smoothing.  A nonzero value adds the key 'reference_smoothing' to the dictionaries and changes nothing in the PNN's columns.
Both also take transform_qps, a list of 1 to 8 QPs, for the transform-domain column: what is left of the PNN's prediction and of the best
HEVC mode's after HM's residual path, RDOQ 0 or with transform_rdoq RDOQ 1 (intraprediction.transform_code; two more pnn_trquant_rdoq_device calls per mask, the
same download).
rd_pass=True (with first_pass and transform_qps) adds HM's second intra pass: the choice by D + lambda R among the first-pass candidates
and the PNN (pnn_rd_pass_rdoq_picture_pairs_device: one more call per mask, the same download).
Options travel as arguments: every call of the mask loop goes to the widest entry of its operation (*_hm_device, pnn_trquant_rdoq_device) with 0
or NULL for an option that is off; the narrower entries of include/pnn_hip.h forward to these with those values: the same kernel launch.
score_block_masks_from_pictures / _picture_pairs score every block under a mask of its OWN (the *_masks_device entries), and
coding_tree_from_pictures(availability='hm') gives each block of the tree the masks HM's coding order leaves it.
"""
import ctypes

import numpy as np

from . import _lib, context, intraprediction
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
                                   tuple_width_height_masks=(0, 0), reference_smoothing=0):
    """predict_mask plus its competitor, as comparing_pnn_ipfcns_hevc_best_mode.py:162-322 scores them: the intra pattern of
    every target (its first row and column start one pixel above-left of the target, i.e. at (row_1st + w - 1,
    col_1st + w - 1)) predicted by the best HEVC intra mode on the GPU.

    Returns the reference's dictionary_performance -- 'indices_hevc_best_mode' [N] uint8, 'psnrs_hevc_best_mode' [N],
    'psnrs_pnn' [N], 'frequency_win_pnn', 'mean_psnr_pnn' -- plus 'predictions_pnn_uint8', 'predictions_hevc_best_mode_uint8'
    and 'targets_uint8' ([N,w,w,1] uint8), N = images x positions, image-major.  reference_smoothing != 0: the HEVC modes predict with
    HM's reference-sample smoothing, and the dictionary says so in 'reference_smoothing'."""
    reference_smoothing = intraprediction._check_smoothing(reference_smoothing)
    pnn = predict_mask(channels_uint8, width_target, row_1sts, col_1sts, predictor, batch_size, mean_training,
                       tuple_width_height_masks)
    intra_patterns_uint8 = intraprediction.extract_intra_patterns(channels_uint8, width_target, row_1sts + width_target - 1,
                                                                  col_1sts + width_target - 1, tuple_width_height_masks)
    indices, psnrs_hevc, predictions_hevc = intraprediction.predict_series_via_hevc_best_mode(
        intra_patterns_uint8, pnn['targets_uint8'], device=predictor.device, smoothing=reference_smoothing)
    psnrs_pnn, frequency_win_pnn = compute_performance_neural_network_vs_hevc_best_mode(
        pnn['targets_uint8'], pnn['predictions_pnn_uint8'], psnrs_hevc)
    dictionary_performance = {
        'indices_hevc_best_mode': indices, 'psnrs_hevc_best_mode': psnrs_hevc, 'psnrs_pnn': psnrs_pnn,
        'frequency_win_pnn': frequency_win_pnn, 'mean_psnr_pnn': np.mean(psnrs_pnn).item(),
        'predictions_pnn_uint8': pnn['predictions_pnn_uint8'], 'predictions_hevc_best_mode_uint8': predictions_hevc,
        'targets_uint8': pnn['targets_uint8']}
    if reference_smoothing:
        dictionary_performance['reference_smoothing'] = reference_smoothing
    return dictionary_performance


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
    _fill_ipfcns_keys(dictionary_performance, sses, width_target, pred_u8)


def _fill_ipfcns_keys(dictionary_performance, sses, width_target, pred_u8):
    """The IPFCN-S keys from the integer SSEs of its uint8 predictions [N,w,w] (None: 'predictions_ipfcns_uint8' is left out)."""
    psnrs = intraprediction.psnrs_from_sses(sses, width_target)
    dictionary_performance['psnrs_ipfcns'] = psnrs
    dictionary_performance['frequency_win_ipfcns'] = \
        float(np.count_nonzero(psnrs - dictionary_performance['psnrs_hevc_best_mode'] > 0.)) / psnrs.size
    dictionary_performance['mean_psnr_ipfcns'] = np.mean(psnrs).item()
    if pred_u8 is not None:
        dictionary_performance['predictions_ipfcns_uint8'] = pred_u8[..., None]


def predict_mask_vs_hevc_best_mode_and_ipfcns(channels_uint8, width_target, row_1sts, col_1sts, predictor, batch_size,
                                              mean_training, net_ipfcns, tuple_width_height_masks=(0, 0), reference_smoothing=0):
    """The three columns of the paper's table, as comparing_pnn_ipfcns_hevc_best_mode.py:162-322 fills them:
    predict_mask_vs_hevc_best_mode's dictionary plus, when net_ipfcns is given and nothing is masked (masks == (0, 0)), the
    IPFCN-S keys of predict_without_mask_via_ipfcns.  reference_smoothing: as for predict_mask_vs_hevc_best_mode."""
    dictionary_performance = predict_mask_vs_hevc_best_mode(channels_uint8, width_target, row_1sts, col_1sts, predictor,
                                                            batch_size, mean_training, tuple_width_height_masks, reference_smoothing)
    if net_ipfcns is not None and tuple(tuple_width_height_masks) == (0, 0):
        predict_without_mask_via_ipfcns(channels_uint8, width_target, row_1sts, col_1sts, batch_size, net_ipfcns,
                                        dictionary_performance)
    return dictionary_performance


def context_descriptor_fields(width_target, height, width, index_image, row_1st, col_1st, tuple_width_height_masks):
    """The pnn_tb_dev fields of one block (context.py's descriptor loop; what the descriptor kernel of pnn_score_pictures_device
    writes): {'origin', 'stride', 'above_mask', 'left_units'} for the target whose context starts at (row_1st, col_1st) of image
    `index_image` in pictures of height x width.  With units = 2w / 4: origin = (index_image * height + row_1st + w) * width +
    col_1st + w, stride = width, above_mask = 2^(units - mask_w / 4) - 1 (0xFFFFFFFF at w = 64 without a mask: a 32-bit shift
    by 32 would not give that), left_units = units - mask_h / 4.  Raises context.py's ValueError for a mask outside {0, 4, ..., w}."""
    w = width_target
    (mask_w, mask_h) = tuple_width_height_masks
    if mask_w < 0 or mask_w > w or mask_w % 4 != 0:
        raise ValueError('`tuple_width_height_masks[0]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.')
    if mask_h < 0 or mask_h > w or mask_h % 4 != 0:
        raise ValueError('`tuple_width_height_masks[1]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.')
    units = 2 * w // 4
    return {'origin': (int(index_image) * int(height) + int(row_1st) + w) * int(width) + int(col_1st) + w, 'stride': int(width),
            'above_mask': (1 << (units - int(mask_w) // 4)) - 1, 'left_units': units - int(mask_h) // 4}


def score_masks_from_pictures(channels_uint8, width_target, row_1sts, col_1sts, predictor, mean_training,
                              tuples_width_height_masks, net_ipfcns=None, keep_predictions=True, first_pass=False, reference_smoothing=0,
                              transform_qps=(), transform_rate=False, transform_sign_hiding=False, rd_pass=False, transform_rdoq=False,
                              rd_pass_signalling=False, rd_pass_neighbour_modes=None, rd_pass_codec='switch', rd_pass_mode_stats=False,
                              transform_skip='off', rd_pass_transform_skip=False):
    """comparing_pnn_ipfcns_hevc_best_mode.py:324-452 (`predict_masks`) on the GPU: the dictionary_performance of
    predict_mask_vs_hevc_best_mode for every mask of `tuples_width_height_masks`, as {(mask_w, mask_h): dictionary}, same keys,
    dtypes and bits.  With `net_ipfcns` the mask (0, 0) also gets the IPFCN-S keys of predict_without_mask_via_ipfcns.

    channels_uint8 [images, H, W, 1], row_1sts / col_1sts (the contexts' top-left corners) are uploaded once.  Per mask ONE
    pnn_score_pictures_device call (made as pnn_score_picture_pairs_hm_device with one plane in both places) -- the descriptors of
    context_descriptor_fields, the PNN pass, the uint8 cast and its integer SSE, the best HEVC mode searched in the pictures
    themselves -- and ONE download; PSNRs from the SSEs by intraprediction.psnrs_from_sses (equal to compute_psnr), 0 dB where no
    HEVC mode beats the reference's start value.  keep_predictions=False leaves out (and never downloads) 'predictions_*_uint8' and
    'targets_uint8'.  Argument errors are those of context.extract_context_portions_targets_from_channels_plus_preprocessing, raised
    before anything touches the GPU.

    first_pass=True adds, per mask, the ranking of HM's first intra pass (TEncSearch.cpp:2376-2492) by ONE more call,
    pnn_first_pass_picture_pairs_hm_device, with the uint8 PNN predictions the score call left on the device as candidate 35; its results
    join the one download.  New keys: 'hads_pnn' uint32 [N] and 'hads_hevc_modes' uint32 [N, 35] (TComRdCost::xGetHADs of the
    predictions against the targets), 'first_pass_list' uint8 [N, K] and 'first_pass_costs' uint32 [N, K] (HM's sorted candidate list,
    K = 8 for w <= 8, else 3; ascending cost, the lower index first among equal costs, 35 = the PNN),
    'frequency_pnn_in_first_pass_list' and 'frequency_pnn_first_pass_best' (float: the share of blocks whose list contains 35 / starts
    with 35).  The costs leave out HM's modeBits * sqrtLambda term (include/pnn_hip.h); whose predictions they cost is
    reference_smoothing's choice.  With first_pass=False nothing changes: not a key, a call or a byte.

    reference_smoothing (0, 1, 2): HM's reference-sample smoothing in the HEVC modes, of the best-mode search and of the first pass alike
    (the `smoothing` argument of the *_hm entries of include/pnn_hip.h, which every call goes through).  0 reproduces the reference's
    extracted predictor, which has none -- the evaluator's competitor; 2 is HM's default, the predictor the encoders run.  A nonzero
    value adds the key 'reference_smoothing' (int) to every dictionary and leaves the PNN's and IPFCN-S's keys bit-identical.  With 0
    nothing changes: not a key, a call or a byte (the entries without _hm pass that 0 on: the same kernel launch under either name).

    transform_qps (1 to 8 integers in [0, 51]; ValueError otherwise, before anything touches the GPU) adds the transform-domain column,
    open-loop: per mask TWO more calls behind the score call (and the first-pass call), pnn_trquant_rdoq_device on the PNN's uint8 predictions
    and on the best HEVC mode's (the smoothed ones when reference_smoothing says so), both against the targets the first mask left on
    the device; HM's residual path as include/pnn_hip.h defines it, with RDOQ 0 unless transform_rdoq is set (no transform skip; sign-data hiding, the rate and RDOQ are the options below; at
    w = 64 the four 32 x 32 quadrants of the one prediction).  Their results join the one download.  New keys: 'transform_qps' (tuple),
    'sses_recon_pnn', 'nb_nonzero_levels_pnn', 'sum_abs_levels_pnn' (uint32 [nb_qps, N]), 'psnrs_recon_pnn' (float64 [nb_qps, N]), the same
    four with '_hevc_best_mode' in place of '_pnn', and 'frequency_recon_win_pnn' (one float per QP: the share of blocks whose PNN
    reconstruction PSNR is strictly higher).  Equal to intraprediction.transform_code on the dictionary's own predictions and targets.
    With transform_qps=() nothing changes: not a key, a call or a byte.

    transform_rate=True (with transform_qps; ValueError without, before anything touches the GPU) gives the two transform calls a rate
    pointer (NULL without it, as pnn_trquant_device passes): the CABAC rate of each residual's levels, the bits HM's counter reports
    from the I-slice initial contexts of the QP (include/pnn_hip.h, "the CABAC rate of the coded levels"; cbf, mode bits and any lambda
    left out).  The best mode's call gets the mode array the score call left on the device (the mode picks the scan at w = 4 and 8),
    the PNN's gets none: its blocks are coded under the diagonal scan, this project's definition.  The results join the one download.
    New keys: 'rate_bits_pnn', 'rate_bits_hevc_best_mode' (float64 [nb_qps, N], bits) and 'frequency_rate_win_pnn' (one float per QP:
    the share of blocks whose PNN residual costs strictly fewer bits).  Equal to intraprediction.transform_code(rate=True, modes=...)
    on the dictionary's own predictions, targets and modes.  With transform_rate=False nothing changes: not a key, a call or a byte.

    transform_sign_hiding=True (with transform_qps; ValueError without, before anything touches the GPU) sets the flag of the two
    transform calls (0 without it, as pnn_trquant_rate_device passes), whether or not transform_rate is set: HM's sign-data hiding as
    its quantiser does it with RDOQ 0 and SignHideFlag 1, HM's default (include/pnn_hip.h, "sign-data hiding").  The best mode's call
    gets the mode array the score call left on the device (the scan now shapes the levels), the PNN's gets none.  Same keys, computed
    from the levels after hiding ('sum_abs_levels_*' stays the sum before it; 'rate_bits_*' does not charge the hidden signs), plus
    'transform_sign_hiding': True.  Equal to intraprediction.transform_code(sign_data_hiding=True, modes=...) on the dictionary's own
    predictions, targets and modes.  With transform_sign_hiding=False nothing changes: not a key, a call or a byte.

    rd_pass=True (with first_pass=True and transform_qps; ValueError without either, before anything touches the GPU) adds HM's second
    intra pass (include/pnn_hip.h, "the second intra pass"; TEncSearch.cpp:2476-2605): per block and QP the choice by D + lambda R among
    the first-pass candidates and the PNN, which is appended as 35 where the list lacks it -- ONE more call per mask,
    pnn_rd_pass_rdoq_picture_pairs_device, behind the others, with the PNN's uint8 predictions on the device as the candidate, HM's lambda of
    each QP, reference_smoothing as the candidates' smoothing and transform_sign_hiding as its flag; its results join the one
    download, its scratch is allocated once.  New keys: 'rd_pass_candidates' uint8 [N, K + 1] (the slots' modes, 255 = unused),
    'rd_pass_costs' float64 [nb_qps, N, K + 1] (inf in an unused slot), 'rd_pass_modes' uint8, 'rd_pass_sses' uint32, 'rd_pass_rate_bits'
    float64 (bits), 'psnrs_recon_rd_pass' float64 (each [nb_qps, N], of the winner) and 'frequency_rd_pass_win_pnn' (one float per QP:
    the share of blocks whose winner is 35 -- how often the encoder would pick the PNN).  Equal to intraprediction.rd_pass on the
    dictionary's own patterns, targets and PNN predictions.  Mode bits and the missing most probable modes are left out, as the
    header says (RDOQ: the next option).  With rd_pass=False nothing changes: not a key, a call or a byte.
    rd_pass_signalling=True (needs rd_pass=True; ValueError otherwise, before anything touches the GPU) runs the second pass with the
    side information HM charges (include/pnn_hip.h, "mode signalling"; intraprediction.rd_pass(signalling=True)): the first pass on
    SATD + modeBits sqrt(lambda), the missing most probable modes appended in front of 35, mode bits and cbf_luma in every cost.
    rd_pass_neighbour_modes (needs rd_pass_signalling): None (no neighbour anywhere) or a pair (left, above) of integer [N] arrays in
    block order (image-major), each None or 0 .. 35 / 255; the same neighbours serve every mask.  The same rd_pass_* keys are written,
    'rd_pass_candidates' and 'rd_pass_costs' per QP with K + 3 slots ([nb_qps, N, K + 3]), plus 'rd_pass_side_rate_bits' float64
    [nb_qps, N] (the winner's mode bits and cbf bins); 'frequency_rd_pass_win_pnn' is computed from the new winners.  With the default
    nothing changes: not a key, a launch or a byte.
    rd_pass_codec='substitution' (needs rd_pass_signalling=True; ValueError otherwise, and for any other name than 'switch', before
    anything touches the GPU) runs the second pass of the reference's other codec (include/pnn_hip.h, "the substitution codec";
    intraprediction.rd_pass(codec='substitution')): HM's own search over modes 0 .. 34 with the PNN's prediction in the place of mode
    18's -- no flag bin, no mode 35, neighbours 0 .. 34 / 255.  The same rd_pass_* keys are written with K + 2 slots, and
    'frequency_rd_pass_win_pnn' is the share of winners equal to 18.  The call is pnn_rd_pass_codec_picture_pairs_device, which every
    second pass here goes through (codec 0 forwards to the entry it was).  With 'switch' nothing changes: not a key, a launch or a byte.
    rd_pass_mode_stats=True (needs rd_pass=True; ValueError otherwise), either codec: ONE more launch per mask,
    pnn_rd_pass_mode_stats_device, counts the tables the reference's codecs print per width from the slots and winners the second pass
    left on the device; they join the one download.  New keys: 'rd_pass_mode_fast_selections', 'rd_pass_mode_fast_wins',
    'rd_pass_mode_rd_wins' (uint32 [nb_qps, 36]: the mode occupies a used slot, is in slot 0, wins), 'rd_pass_modes_for_rd' (int64
    [nb_qps], the used slots: m_cumNbModesForRD) and 'rd_pass_runs' (N: m_nbFastRDRuns).  Equal to
    intraprediction.rd_pass_mode_stats on the dictionary's own 'rd_pass_candidates' and 'rd_pass_modes'.  With False nothing changes.

    transform_rdoq=True (with transform_qps; ValueError without, before anything touches the GPU) sets the option rdoq of the two
    transform calls and of the second-pass call (0 without it): HM's RDOQ under HM's lambda of each QP (include/pnn_hip.h,
    "rate-distortion optimised quantisation").  The transform-domain keys and the rd_pass_* keys are then those of RDOQ 1, and
    'transform_rdoq': True joins them.  Equal to intraprediction.transform_code(rdoq=True, modes=...) and rd_pass(rdoq=True) on the
    dictionary's own arrays.  With transform_rdoq=False nothing changes: not a key, a call or a byte.
    transform_skip='forced' or 'decide' (width 4 and transform_qps; ValueError otherwise, and for any other name than 'off', before
    anything touches the GPU; include/pnn_hip.h, "transform skip"; at width 4 'decide' is what the reference's configuration does): the two
    transform-coding calls go to pnn_trquant_tskip_device -- every 4 x 4 unit in its skipped form, or in the form HM's rule keeps under
    HM's lambda of each QP, no mode bits, the cbf bin charged; the scan of the best mode's column follows its mode.  The transform-domain
    keys are then the kept form's (the rate with the flag's bin), and new keys join them: 'transform_skip': the name,
    'transform_skip_flags_pnn' and 'transform_skip_flags_hevc_best_mode' (uint8 [nb_qps, N]: one per coded column, as every other
    transform-domain key) and 'frequency_transform_skip_pnn' / '_hevc_best_mode' (one float per QP: the share of units kept skipped).
    Equal to intraprediction.transform_code(transform_skip=..., modes=...) on the dictionary's own arrays.
    rd_pass_transform_skip=True (width 4 and rd_pass_signalling=True; ValueError otherwise, before anything touches the GPU): the second
    pass is pnn_rd_pass_tskip_picture_pairs_device's, either codec -- every slot keeps its cheaper form before the slots are compared, so
    'frequency_rd_pass_win_pnn' is computed against the competitor HM runs.  New keys: 'rd_pass_best_transform_skip' (uint8 [nb_qps, N],
    the winner's flag) and 'frequency_rd_pass_transform_skip' (one float per QP: the share of winners kept skipped).  Equal to
    intraprediction.rd_pass(transform_skip=True).  With the defaults nothing changes: not a key, a call or a byte."""
    return _score_masks(channels_uint8, 1, width_target, row_1sts, col_1sts, predictor, mean_training, tuples_width_height_masks,
                        net_ipfcns, keep_predictions, first_pass, reference_smoothing, transform_qps, transform_rate, transform_sign_hiding, rd_pass,
                        transform_rdoq, rd_pass_signalling, rd_pass_neighbour_modes, rd_pass_codec, rd_pass_mode_stats, transform_skip,
                        rd_pass_transform_skip)


def score_masks_from_picture_pairs(channels_pair_uint8, width_target, row_1sts, col_1sts, predictor, mean_training,
                                   tuples_width_height_masks, net_ipfcns=None, keep_predictions=True, first_pass=False, reference_smoothing=0,
                                   transform_qps=(), transform_rate=False, transform_sign_hiding=False, rd_pass=False, transform_rdoq=False,
                                   rd_pass_signalling=False, rd_pass_neighbour_modes=None, rd_pass_codec='switch', rd_pass_mode_stats=False,
                                   transform_skip='off', rd_pass_transform_skip=False):
    """score_masks_from_pictures for the "pair" models (trained on contexts of HEVC-decoded pictures with targets of the originals):
    channels_pair_uint8 [images, H, W, 2] as the reference carries such data, channel 0 the original, channel 1 the decoded picture.
    Same arguments otherwise, same dictionaries per mask, same `keep_predictions`, same errors before anything touches the GPU.

    Which plane feeds what (pnn_score_picture_pairs_hm_device):
      decoded (last channel):  the PNN's contexts (sets/common.py reads them there), the intra pattern of the HEVC search (this
                               project's definition -- the reference's extract_intra_patterns has no pair form; the decoded
                               neighbourhood is what an encoder holds), the reference lines of IPFCN-S (ipfcns.py:60-65)
      original (channel 0):    'targets_uint8' and the targets of every SSE, hence of every PSNR
    The pair is de-interleaved once on the host and uploaded once; per mask ONE call and ONE download, as for single pictures.
    first_pass=True: the keys of score_masks_from_pictures; reference samples from the decoded plane, targets of the costs from the
    original, as in the table above.  reference_smoothing: as for score_masks_from_pictures; the smoothed line is built from the decoded
    plane's samples, as the unsmoothed one is.  transform_qps: as for score_masks_from_pictures; the predictions that get coded are the
    ones made from the decoded plane, the residual's and the SSE's targets come from the original, as in the table above.
    transform_rate, transform_sign_hiding, transform_rdoq, rd_pass_signalling, rd_pass_neighbour_modes, rd_pass_codec, rd_pass_mode_stats,
    transform_skip, rd_pass_transform_skip: as for score_masks_from_pictures."""
    return _score_masks(channels_pair_uint8, 2, width_target, row_1sts, col_1sts, predictor, mean_training,
                        tuples_width_height_masks, net_ipfcns, keep_predictions, first_pass, reference_smoothing, transform_qps,
                        transform_rate, transform_sign_hiding, rd_pass, transform_rdoq, rd_pass_signalling, rd_pass_neighbour_modes, rd_pass_codec,
                        rd_pass_mode_stats, transform_skip, rd_pass_transform_skip)

def _check_block_masks(width_target, row_1sts, masks_w, masks_h, rd_pass, rd_pass_signalling):
    """The masks per block of score_block_masks_*: two integer arrays of row_1sts.size values in {0, 4, ..., width_target}; as uint8.
    Also the one option the per-block entries lack: a second pass without signalling (the entry it extends has none either)."""
    if rd_pass and not rd_pass_signalling:
        raise ValueError('masks per block: `rd_pass` needs `rd_pass_signalling` (pnn_rd_pass_picture_pairs_masks_device has no form without).')
    checked = []
    for masks, name in ((masks_w, 'masks_w'), (masks_h, 'masks_h')):
        masks = np.asarray(masks)
        if not np.issubdtype(masks.dtype, np.integer):
            raise TypeError('`%s.dtype` is not smaller than `numpy.integer` in type hierarchy.' % name)
        if masks.size != np.asarray(row_1sts).size:
            raise ValueError('`%s.size` is not equal to `row_1sts.size`.' % name)
        if masks.size and (masks.min() < 0 or masks.max() > width_target or np.any(masks % 4)):
            raise ValueError('`%s` has a value that does not belong to {0, 4, ..., `width_target`}.' % name)
        checked.append(np.ascontiguousarray(masks.ravel(), dtype=np.uint8))
    return tuple(checked)


def score_block_masks_from_pictures(channels_uint8, width_target, row_1sts, col_1sts, predictor, mean_training, masks_w, masks_h,
                                    keep_predictions=True, first_pass=False, reference_smoothing=0, transform_qps=(), transform_rate=False,
                                    transform_sign_hiding=False, rd_pass=False, transform_rdoq=False, rd_pass_signalling=False,
                                    rd_pass_neighbour_modes=None, rd_pass_codec='switch', rd_pass_mode_stats=False, transform_skip='off',
                                    rd_pass_transform_skip=False):
    """score_masks_from_pictures with a mask PER BLOCK instead of a list of masks for all blocks (include/pnn_hip.h, "masks per block"):
    masks_w / masks_h, integer arrays [positions] with values in {0, 4, ..., width_target}, give the masks of the blocks at each
    position, the same in every image -- intraprediction.hm_context_masks makes the ones HM's coding order leaves the blocks of a CTU
    grid.  Returns ONE dictionary with the keys a mask's dictionary has: block b's entries are those the mask
    (masks_w[pos], masks_h[pos]) gives it in score_masks_from_pictures, bit for bit; the frequencies and means run over the blocks as
    they are.  One upload (pictures, positions and masks), the same calls -- the score call, the first pass and the second pass as
    pnn_score_picture_pairs_masks_device, pnn_first_pass_picture_pairs_masks_device and pnn_rd_pass_picture_pairs_masks_device, the
    transform coding unchanged --, one download.  The options are score_masks_from_pictures' but two: there is no net_ipfcns (IPFCN-S
    has no masked form), and rd_pass=True needs rd_pass_signalling=True (ValueError otherwise: the second pass's entry has no form
    without).  Every argument is checked before anything touches the GPU."""
    w = width_target
    if w not in intraprediction.WIDTHS:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    block_masks = _check_block_masks(w, row_1sts, masks_w, masks_h, rd_pass, rd_pass_signalling)
    return _score_masks(channels_uint8, 1, w, row_1sts, col_1sts, predictor, mean_training, (), None, keep_predictions, first_pass,
                        reference_smoothing, transform_qps, transform_rate, transform_sign_hiding, rd_pass, transform_rdoq, rd_pass_signalling,
                        rd_pass_neighbour_modes, rd_pass_codec, rd_pass_mode_stats, transform_skip, rd_pass_transform_skip,
                        _block_masks=block_masks)[None]


def score_block_masks_from_picture_pairs(channels_pair_uint8, width_target, row_1sts, col_1sts, predictor, mean_training, masks_w, masks_h,
                                         keep_predictions=True, first_pass=False, reference_smoothing=0, transform_qps=(), transform_rate=False,
                                         transform_sign_hiding=False, rd_pass=False, transform_rdoq=False, rd_pass_signalling=False,
                                         rd_pass_neighbour_modes=None, rd_pass_codec='switch', rd_pass_mode_stats=False, transform_skip='off',
                                         rd_pass_transform_skip=False):
    """score_block_masks_from_pictures on [images, H, W, 2] pairs (original, decoded), the planes used as score_masks_from_picture_pairs
    uses them."""
    w = width_target
    if w not in intraprediction.WIDTHS:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    block_masks = _check_block_masks(w, row_1sts, masks_w, masks_h, rd_pass, rd_pass_signalling)
    return _score_masks(channels_pair_uint8, 2, w, row_1sts, col_1sts, predictor, mean_training, (), None, keep_predictions, first_pass,
                        reference_smoothing, transform_qps, transform_rate, transform_sign_hiding, rd_pass, transform_rdoq, rd_pass_signalling,
                        rd_pass_neighbour_modes, rd_pass_codec, rd_pass_mode_stats, transform_skip, rd_pass_transform_skip,
                        _block_masks=block_masks)[None]


def _check_score_masks_arguments(ch, nb_planes, w, row_1sts, col_1sts, predictor, mean_training, tuples_width_height_masks, net_ipfcns,
                                 reference_smoothing, transform_qps, transform_rate, transform_sign_hiding, rd_pass=False, transform_rdoq=False):
    """The argument checks of _score_masks, all before anything touches the GPU; the library is first used by the last, the predictor's mean.
    Returns (masks as int pairs, rows and cols as flat int64 arrays, reference_smoothing as int, transform_qps as a tuple of ints or ())."""
    if ch.dtype != np.uint8:
        raise TypeError('`channels_single_or_pair_uint8.dtype` is not equal to `numpy.uint8`.')
    if not np.issubdtype(row_1sts.dtype, np.integer):
        raise TypeError('`row_1sts.dtype` is not smaller than `numpy.integer` in type hierarchy.')
    if not np.issubdtype(col_1sts.dtype, np.integer):
        raise TypeError('`col_1sts.dtype` is not smaller than `numpy.integer` in type hierarchy.')
    if col_1sts.size != row_1sts.size:
        raise ValueError('`col_1sts.size` is not equal to `row_1sts.size`.')
    if ch.ndim != 4:
        raise ValueError('`channels_uint8.ndim` is not equal to 4.')
    nb_images, height, width, nb_channels = ch.shape
    if nb_channels not in (1, 2):
        raise ValueError('`channel_single_or_pair_uint8.shape[2]` does not belong to {1, 2}.')
    if nb_planes == 1 and nb_channels != 1:
        raise ValueError('`channels_uint8.shape[3]` is not equal to 1 (pairs of channels: context.py).')
    if nb_planes == 2 and nb_channels != 2:
        raise ValueError('`channels_pair_uint8.shape[3]` is not equal to 2 (single pictures: score_masks_from_pictures).')
    if w not in intraprediction.WIDTHS:
        raise ValueError('`width_target` does not belong to {4, 8, 16, 32, 64}.')
    if reference_smoothing not in intraprediction.SMOOTHINGS:
        raise ValueError('`reference_smoothing` does not belong to {0, 1, 2}.')
    if not (isinstance(transform_qps, (tuple, list)) and len(transform_qps) == 0):
        transform_qps = intraprediction._check_qps(transform_qps)
    if transform_rate and len(transform_qps) == 0:
        raise ValueError('`transform_rate` is set without `transform_qps`.')
    if transform_sign_hiding and len(transform_qps) == 0:
        raise ValueError('`transform_sign_hiding` is set without `transform_qps`.')
    if rd_pass and len(transform_qps) == 0:
        raise ValueError('`rd_pass` is set without `transform_qps`.')
    if transform_rdoq and len(transform_qps) == 0:
        raise ValueError('`transform_rdoq` is set without `transform_qps`.')
    masks = [(int(m[0]), int(m[1])) for m in tuples_width_height_masks]
    rows, cols = row_1sts.astype(np.int64).ravel(), col_1sts.astype(np.int64).ravel()
    if nb_images * rows.size == 0:
        raise ValueError('there is no target: no image or no position.')
    for mask in masks:
        context_descriptor_fields(w, height, width, nb_images - 1, rows[-1], cols[-1], mask)
    if rows.min() < 0 or cols.min() < 0:
        raise ValueError('`row_1st` / `col_1st` is not positive.')
    if rows.max() + 3 * w > height or cols.max() + 3 * w > width:
        raise ValueError('the context does not fit into the channel.')
    if predictor is None:
        raise ValueError("`predictor` (a PredictionNeuralNetwork holding the GPU context) is required")
    if predictor.width_target != w:
        raise ValueError('the predictor is for width %d, not %d' % (predictor.width_target, w))
    if net_ipfcns is not None and (0, 0) in masks:
        if net_ipfcns.width_target != w:
            raise ValueError('the net is the width-%d IPFCN-S, not the width-%d one' % (net_ipfcns.width_target, w))
        if net_ipfcns.device != predictor.device:
            raise ValueError('the IPFCN-S and the predictor are on different devices')
    ctx_mean = ctypes.c_float(_lib.lib().pnn_mean(predictor.ctx)).value
    if abs(ctx_mean - np.float32(mean_training)) > 1e-6:
        raise ValueError("`mean_training` differs from the predictor's mean")
    return masks, rows, cols, int(reference_smoothing), tuple(transform_qps)


_CODED_COLUMNS = (('pnn', 'predictions_pnn'), ('hevc_best_mode', 'predictions_hevc'))      # (key suffix, section) of what transform_qps codes
_COUNTS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels')                            # per coded column, uint32 [nb_qps, n]


_RD_PASS_SECTIONS = ('rd_pass_candidates', 'rd_pass_costs', 'rd_pass_modes', 'rd_pass_slots', 'rd_pass_best_costs', 'rd_pass_sses',
                     'rd_pass_rates')                                                      # intraprediction.RD_PASS_OUTPUTS, in the entry's order


def _output_layout(n, w, first_pass, nb_qps, transform_rate, rd_pass=False, rd_pass_signalling=False, rd_pass_codec='switch', rd_pass_mode_stats=False,
                   transform_skip=0, rd_pass_transform_skip=False):
    """Every output of a mask's calls in ONE buffer, described once as (name, dtype, shape): the small results first, then the uint8
    blocks of the PNN, of HEVC and the targets; a download is a prefix of it.  Each section starts at a multiple of its item size.
    Returns (sections, begin, end), the last two the byte offsets by name; end['targets'] is the size of the buffer."""
    sections = [('sses_pnn', np.uint32, (n,)), ('sses_hevc', np.uint32, (n,)), ('indices_hevc', np.uint8, (n,))]
    if first_pass:
        nb_list = intraprediction.first_pass_list_size(w)
        sections += [('hads_hevc_modes', np.uint32, (n, intraprediction.NB_MODES)), ('hads_pnn', np.uint32, (n,)),
                     ('first_pass_costs', np.uint32, (n, nb_list)), ('first_pass_list', np.uint8, (n, nb_list))]
    for column, _ in _CODED_COLUMNS if nb_qps else ():
        sections += [('%s_%s' % (name, column), np.uint32, (nb_qps, n)) for name in _COUNTS]
        if transform_rate:
            sections.append(('rate_' + column, np.uint64, (nb_qps, n)))
        if transform_skip:
            sections.append(('transform_skip_flags_' + column, np.uint8, (nb_qps, n)))
    if rd_pass and rd_pass_signalling:                    # per QP, K + 3 slots (K + 2: the substitution codec); the list's costs are not asked for
        shapes = intraprediction.rd_pass_signal_shapes(n, nb_qps, w, rd_pass_codec)
        sections += [(name, dtype, shape) for name, (_, dtype), shape in zip(_RD_PASS_SECTIONS, intraprediction.RD_PASS_OUTPUTS, shapes)]
        sections.append(('rd_pass_side_rates', np.uint64, shapes[-1]))
        if rd_pass_transform_skip:
            sections.append(('rd_pass_best_transform_skip', np.uint8, (nb_qps, n)))
    elif rd_pass:
        sections += [(name, dtype, shape) for name, (_, dtype), shape in zip(_RD_PASS_SECTIONS, intraprediction.RD_PASS_OUTPUTS,
                                                                             intraprediction.rd_pass_shapes(n, nb_qps, w))]
    if rd_pass_mode_stats:
        sections.append(('rd_pass_mode_stats', np.uint32, (nb_qps, 3, intraprediction.NB_STATS_BINS)))
    sections += [(name, np.uint8, (n, w, w, 1)) for name in ('predictions_pnn', 'predictions_hevc', 'targets')]
    begin, end, offset = {}, {}, 0
    for name, dtype, shape in sections:
        size = np.dtype(dtype).itemsize
        begin[name] = (offset + size - 1) // size * size
        end[name] = offset = begin[name] + size * int(np.prod(shape))
    return sections, begin, end


def _dictionary_of_download(view, n, w, first_pass, reference_smoothing, transform_qps, transform_rate, transform_sign_hiding, rd_pass=False,
                            transform_rdoq=False, rd_pass_signalling=False, rd_pass_codec='switch', rd_pass_mode_stats=False,
                            transform_skip='off', rd_pass_transform_skip=False):
    """One mask's dictionary_performance, but for the uint8 blocks, from `view`: the downloaded sections by name."""
    psnrs_pnn = intraprediction.psnrs_from_sses(view['sses_pnn'], w)
    psnrs_hevc = intraprediction.psnrs_from_sses(view['sses_hevc'], w)
    psnrs_hevc[view['sses_hevc'] == 65025 * w * w] = 0.   # the reference's start value, never beaten
    d = {'indices_hevc_best_mode': view['indices_hevc'].copy(), 'psnrs_hevc_best_mode': psnrs_hevc, 'psnrs_pnn': psnrs_pnn,
         'frequency_win_pnn': float(np.count_nonzero(psnrs_pnn - psnrs_hevc > 0.)) / n, 'mean_psnr_pnn': np.mean(psnrs_pnn).item()}
    if first_pass:
        d.update({key: view[key].copy() for key in ('hads_pnn', 'hads_hevc_modes', 'first_pass_list', 'first_pass_costs')})
        is_pnn = d['first_pass_list'] == intraprediction.NB_MODES
        d['frequency_pnn_in_first_pass_list'] = float(np.count_nonzero(is_pnn.any(axis=1))) / n
        d['frequency_pnn_first_pass_best'] = float(np.count_nonzero(is_pnn[:, 0])) / n
    if reference_smoothing:
        d['reference_smoothing'] = reference_smoothing
    if transform_qps:
        d['transform_qps'] = transform_qps
        for column, _ in _CODED_COLUMNS:
            d.update({key: view[key].copy() for key in ('%s_%s' % (name, column) for name in _COUNTS)})
            d['psnrs_recon_' + column] = intraprediction.psnrs_from_sses(view['sses_recon_' + column], w)
        d['frequency_recon_win_pnn'] = [float(np.count_nonzero(pnn - hevc > 0.)) / n                   # one float per QP
                                        for pnn, hevc in zip(d['psnrs_recon_pnn'], d['psnrs_recon_hevc_best_mode'])]
    if transform_rate:
        for column, _ in _CODED_COLUMNS:
            d['rate_bits_' + column] = view['rate_' + column].astype(np.float64) / 32768.
        d['frequency_rate_win_pnn'] = [float(np.count_nonzero(pnn < hevc)) / n
                                       for pnn, hevc in zip(d['rate_bits_pnn'], d['rate_bits_hevc_best_mode'])]
    if transform_sign_hiding:
        d['transform_sign_hiding'] = True
    if transform_rdoq:
        d['transform_rdoq'] = True
    if transform_skip != 'off':
        d['transform_skip'] = transform_skip
        for column, _ in _CODED_COLUMNS:
            d['transform_skip_flags_' + column] = view['transform_skip_flags_' + column].copy()
            d['frequency_transform_skip_' + column] = [float(np.count_nonzero(flags)) / n for flags in d['transform_skip_flags_' + column]]
    if rd_pass:
        d.update({key: view[key].copy() for key in ('rd_pass_candidates', 'rd_pass_costs', 'rd_pass_modes', 'rd_pass_sses')})
        d['rd_pass_rate_bits'] = view['rd_pass_rates'].astype(np.float64) / 32768.
        d['psnrs_recon_rd_pass'] = intraprediction.psnrs_from_sses(view['rd_pass_sses'], w)
        pnn_mode = intraprediction.SUBSTITUTED_MODE if intraprediction.CODECS[rd_pass_codec] else intraprediction.NB_MODES
        d['frequency_rd_pass_win_pnn'] = [float(np.count_nonzero(modes == pnn_mode)) / n for modes in d['rd_pass_modes']]
        if rd_pass_signalling:
            d['rd_pass_side_rate_bits'] = view['rd_pass_side_rates'].astype(np.float64) / 32768.
        if rd_pass_transform_skip:
            d['rd_pass_best_transform_skip'] = view['rd_pass_best_transform_skip'].copy()
            d['frequency_rd_pass_transform_skip'] = [float(np.count_nonzero(flags)) / n for flags in d['rd_pass_best_transform_skip']]
        if rd_pass_mode_stats:
            stats = intraprediction.mode_stats_dictionary(view['rd_pass_mode_stats'], n)
            d.update({'rd_pass_mode_fast_selections': stats['fast_selections'], 'rd_pass_mode_fast_wins': stats['fast_wins'],
                      'rd_pass_mode_rd_wins': stats['rd_wins'], 'rd_pass_modes_for_rd': stats['modes_for_rd'], 'rd_pass_runs': stats['runs']})
    return d


def _score_masks(ch, nb_planes, width_target, row_1sts, col_1sts, predictor, mean_training, tuples_width_height_masks, net_ipfcns,
                 keep_predictions, first_pass, reference_smoothing, transform_qps, transform_rate, transform_sign_hiding, rd_pass=False,
                 transform_rdoq=False, rd_pass_signalling=False, rd_pass_neighbour_modes=None, rd_pass_codec='switch', rd_pass_mode_stats=False,
                 transform_skip='off', rd_pass_transform_skip=False, _tree_leaves=None, _block_masks=None):
    """The body of score_masks_from_pictures (nb_planes = 1) and score_masks_from_picture_pairs (2): the targets come from channel 0,
    everything a predictor reads from the last channel; with one plane the two are the same device buffer.  Every option is an argument
    of the one entry its call has (the smoothing; the mode pointer, the rate pointer and the flag), 0 or NULL when off.
    _tree_leaves (private to coding_tree_from_pictures; None: nothing changes, call for call): {'dist', 'rate', 'mode': torch tensors
    on the predictor's device of [nb_qps, n] uint32 / uint64 / uint8 elements, 'keep': bool}.  Behind the second pass of each mask one
    more call, pnn_cu_tree_leaves_device, writes the width's leaves of the coding tree into them from the outputs the pass left on the
    device; with 'keep' False the mask's results are then neither downloaded nor returned (its value is None).
    _block_masks (private to score_block_masks_* and coding_tree_from_pictures; None: nothing changes, call for call): (masks_w, masks_h),
    checked uint8 [positions] arrays.  The loop then runs ONCE, under the key None (tuples_width_height_masks must be empty), and the score
    call, the first pass and the second pass go to the *_masks_device entries with the two arrays, uploaded once with everything else."""
    w = width_target
    if _block_masks is not None and len(tuples_width_height_masks):
        raise ValueError('`_block_masks` is given beside a list of masks.')
    if _tree_leaves is not None and not (rd_pass and rd_pass_signalling):
        raise ValueError('`_tree_leaves` is given without the second pass with signalling.')
    if rd_pass_signalling and not rd_pass:
        raise ValueError('`rd_pass_signalling` is set without `rd_pass`.')
    if rd_pass_neighbour_modes is not None and not rd_pass_signalling:
        raise ValueError('`rd_pass_neighbour_modes` is given without `rd_pass_signalling`.')
    if rd_pass_codec not in intraprediction.CODECS:
        raise ValueError("`rd_pass_codec` is not 'switch' or 'substitution'.")
    codec = intraprediction.CODECS[rd_pass_codec]
    if codec and not rd_pass_signalling:
        raise ValueError("`rd_pass_codec` 'substitution' is set without `rd_pass_signalling`.")
    if rd_pass_mode_stats and not rd_pass:
        raise ValueError('`rd_pass_mode_stats` is set without `rd_pass`.')
    if transform_skip not in intraprediction._TRANSFORM_SKIP:
        raise ValueError("`transform_skip` is not 'off', 'forced' or 'decide'.")
    skip = intraprediction._TRANSFORM_SKIP[transform_skip]
    if skip and len(transform_qps) == 0:
        raise ValueError('`transform_skip` is on without `transform_qps`.')
    if rd_pass_transform_skip and not rd_pass_signalling:
        raise ValueError('`rd_pass_transform_skip` is set without `rd_pass_signalling`.')
    if (skip or rd_pass_transform_skip) and w != 4:
        raise ValueError('`transform_skip` / `rd_pass_transform_skip` is on at a width other than 4.')
    rd_skip = int(bool(rd_pass_transform_skip))
    masks, rows, cols, reference_smoothing, transform_qps = _check_score_masks_arguments(
        ch, nb_planes, w, row_1sts, col_1sts, predictor, mean_training, tuples_width_height_masks, net_ipfcns, reference_smoothing,
        transform_qps, transform_rate, transform_sign_hiding, rd_pass, transform_rdoq)
    if rd_pass and not first_pass:
        raise ValueError('`rd_pass` is set without `first_pass`.')
    nb_images, height, width = ch.shape[:3]
    n_pos, nb_qps = rows.size, len(transform_qps)
    n = nb_images * n_pos
    L = _lib.lib()
    per_block = _block_masks is not None
    if per_block:                                         # one pass of the loop below, under the key None
        masks = [None]
    signalling = int(bool(rd_pass_signalling))
    left, above = (None, None) if rd_pass_neighbour_modes is None else rd_pass_neighbour_modes
    left = intraprediction._neighbour_array(left, n, not codec, 'rd_pass_neighbour_modes[0]')
    above = intraprediction._neighbour_array(above, n, not codec, 'rd_pass_neighbour_modes[1]')

    import torch
    dev = torch.device('cuda', predictor.device)
    d_planes = torch.from_numpy(np.ascontiguousarray(np.moveaxis(ch, 3, 0))).to(dev)      # [planes, images, H, W]: one copy, one upload
    d_target_channels, d_context_channels = d_planes[0], d_planes[nb_planes - 1]
    d_rows, d_cols = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (rows, cols))
    if per_block:                                         # both arrays in one upload, [2, positions]
        d_block_masks = torch.from_numpy(np.stack([np.asarray(a, np.uint8).ravel() for a in _block_masks])).to(dev)
    sections, begin, end = _output_layout(n, w, first_pass, nb_qps, transform_rate, rd_pass, rd_pass_signalling, rd_pass_codec, rd_pass_mode_stats,
                                          skip, rd_skip)
    d_out = torch.empty(end['targets'], dtype=torch.uint8, device=dev)       # the last section
    ptr = {name: d_out.data_ptr() + begin[name] for name in begin}
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    c_qps = (ctypes.c_int * max(nb_qps, 1))(*transform_qps)
    if rd_pass:                                           # the entry's scratch, the caller's: once for all masks
        nb_scratch = (L.pnn_rd_pass_tskip_workspace_bytes(w, n, nb_qps, signalling, codec, 1) if rd_skip else
                      L.pnn_rd_pass_codec_workspace_bytes(w, n, nb_qps, signalling, codec))
        d_scratch = torch.empty(nb_scratch, dtype=torch.uint8, device=dev)
        d_left, d_above = (None if a is None else torch.from_numpy(a).to(dev) for a in (left, above))
    if skip:                                              # the scratch of the two forms, the caller's: once for all masks and both columns
        nb_skip_scratch = L.pnn_trquant_tskip_workspace_bytes(w, n, nb_qps)
        d_skip_scratch = torch.empty(nb_skip_scratch, dtype=torch.uint8, device=dev)
    results, targets_uint8 = {}, None
    for i, mask in enumerate(masks):
        if mask in results:
            continue
        first = i == 0
        # the blocks of every picture entry: the mask's two ints, or (per block) the two arrays in their place for the *_masks_ entries
        blocks = (predictor.ctx, w, d_context_channels.data_ptr(), d_target_channels.data_ptr(), nb_images, height, width,
                  d_rows.data_ptr(), d_cols.data_ptr(), n_pos) + \
            ((d_block_masks[0].data_ptr(), d_block_masks[1].data_ptr()) if per_block else (mask[0], mask[1]))
        with torch.cuda.device(dev):
            _lib.check((L.pnn_score_picture_pairs_masks_device if per_block else L.pnn_score_picture_pairs_hm_device)(
                *blocks, reference_smoothing, ptr['targets'] if first else None,
                ptr['predictions_pnn'] if keep_predictions or first_pass or nb_qps else None, None, ptr['sses_pnn'], ptr['indices_hevc'],
                ptr['sses_hevc'], ptr['predictions_hevc'] if keep_predictions or nb_qps else None, stream), predictor.ctx)
            if first_pass:                                # the PNN's uint8 predictions are on the device: candidate 35
                _lib.check((L.pnn_first_pass_picture_pairs_masks_device if per_block else L.pnn_first_pass_picture_pairs_hm_device)(
                    *blocks, ptr['predictions_pnn'], reference_smoothing, ptr['hads_hevc_modes'], ptr['hads_pnn'], ptr['first_pass_list'],
                    ptr['first_pass_costs'], stream), predictor.ctx)
            for column, predictions in _CODED_COLUMNS if nb_qps else ():
                # both predictions and the first mask's targets are on the device.  Where the scan is read (by the rate, by the hiding), the
                # best mode's follows its mode, which the score call left there; the PNN has no mode: the diagonal scan
                modes = ptr['indices_hevc'] if column == 'hevc_best_mode' and (transform_rate or transform_sign_hiding or transform_rdoq or
                                                                               skip) else None
                if skip:                                  # (with the option off the call below is the one of before, argument for argument)
                    _lib.check(L.pnn_trquant_tskip_device(
                        predictor.ctx, w, ptr[predictions], ptr['targets'], n, modes, c_qps, nb_qps, ptr['sses_recon_' + column],
                        ptr['nb_nonzero_levels_' + column], ptr['sum_abs_levels_' + column], None, ptr['rate_' + column] if transform_rate else None,
                        int(bool(transform_sign_hiding)), int(bool(transform_rdoq)), None, skip, None, 1, ptr['transform_skip_flags_' + column],
                        d_skip_scratch.data_ptr(), nb_skip_scratch, stream), predictor.ctx)
                    continue
                _lib.check(L.pnn_trquant_rdoq_device(
                    predictor.ctx, w, ptr[predictions], ptr['targets'], n, modes, c_qps, nb_qps, ptr['sses_recon_' + column],
                    ptr['nb_nonzero_levels_' + column], ptr['sum_abs_levels_' + column], None, ptr['rate_' + column] if transform_rate else None,
                    int(bool(transform_sign_hiding)), int(bool(transform_rdoq)), None, stream), predictor.ctx)
            if rd_pass and per_block:                     # masks per block: the one entry, transform skip as its option (0: the codec entry's launches)
                _lib.check(L.pnn_rd_pass_picture_pairs_masks_device(
                    *blocks, ptr['predictions_pnn'], reference_smoothing, c_qps, nb_qps, None, int(bool(transform_sign_hiding)),
                    int(bool(transform_rdoq)), signalling, None if d_left is None else d_left.data_ptr(),
                    None if d_above is None else d_above.data_ptr(), codec, rd_skip, *[ptr[name] for name in _RD_PASS_SECTIONS], None,
                    ptr['rd_pass_side_rates'], ptr['rd_pass_best_transform_skip'] if rd_skip else None, d_scratch.data_ptr(), nb_scratch, stream),
                    predictor.ctx)
            elif rd_pass and rd_skip:                     # the second pass with transform skip: the codec entry's arguments and two more
                _lib.check(L.pnn_rd_pass_tskip_picture_pairs_device(
                    *blocks, ptr['predictions_pnn'], reference_smoothing, c_qps, nb_qps, None, int(bool(transform_sign_hiding)),
                    int(bool(transform_rdoq)), signalling, None if d_left is None else d_left.data_ptr(),
                    None if d_above is None else d_above.data_ptr(), codec, 1, *[ptr[name] for name in _RD_PASS_SECTIONS], None,
                    ptr['rd_pass_side_rates'], ptr['rd_pass_best_transform_skip'], d_scratch.data_ptr(), nb_scratch, stream), predictor.ctx)
            elif rd_pass:                                 # the candidate is the PNN's uint8 prediction; NULL lambdas: HM's of each QP
                # (the one entry of the second pass; codec 0 forwards to pnn_rd_pass_signal_picture_pairs_device, whose signalling 0 forwards
                # to pnn_rd_pass_rdoq_picture_pairs_device: the same launches)
                _lib.check(L.pnn_rd_pass_codec_picture_pairs_device(
                    *blocks, ptr['predictions_pnn'], reference_smoothing, c_qps, nb_qps, None, int(bool(transform_sign_hiding)),
                    int(bool(transform_rdoq)), signalling, None if d_left is None else d_left.data_ptr(),
                    None if d_above is None else d_above.data_ptr(), codec, *[ptr[name] for name in _RD_PASS_SECTIONS], None,
                    ptr['rd_pass_side_rates'] if signalling else None, d_scratch.data_ptr(), nb_scratch, stream), predictor.ctx)
            if rd_pass and rd_pass_mode_stats:            # from the slots and winners the call above left in the output buffer
                _lib.check(L.pnn_rd_pass_mode_stats_device(
                    predictor.ctx, ptr['rd_pass_candidates'], signalling, intraprediction.rd_pass_slot_count(w, signalling, rd_pass_codec),
                    ptr['rd_pass_modes'], n, nb_qps, ptr['rd_pass_mode_stats'], stream), predictor.ctx)
            if _tree_leaves is not None:                  # the coding tree's leaves of this width, device to device
                _lib.check(L.pnn_cu_tree_leaves_device(
                    predictor.ctx, w, n, nb_qps, ptr['rd_pass_sses'], ptr['rd_pass_rates'], ptr['rd_pass_side_rates'], ptr['rd_pass_modes'],
                    _tree_leaves['dist'].data_ptr(), _tree_leaves['rate'].data_ptr(), _tree_leaves['mode'].data_ptr(), stream), predictor.ctx)
        if _tree_leaves is not None and not _tree_leaves['keep']:
            # No download, hence NO wait for the stream: this function returns, and d_out, d_scratch, d_planes and the positions go
            # back to torch's caching allocator, while its launches may still be queued.  That is safe only because the allocator
            # is stream-ordered and everything that follows -- the next width's calls, the tree, its download -- is issued on the
            # SAME torch current stream of this device.  coding_tree_from_pictures must therefore run under one stream context from
            # its first width to its download; a caller that switched torch.cuda.stream between widths would break this.  (c_qps
            # and the other host arguments are read by the entries before they return.)
            results[mask] = None
            continue
        nb_down = (end['targets'] if first else begin['targets']) if keep_predictions else begin['predictions_pnn']
        out = d_out[:nb_down].cpu().numpy()               # (waits for the stream)
        view = {name: out[begin[name]:end[name]].view(dtype).reshape(shape) for name, dtype, shape in sections if end[name] <= out.size}
        dictionary_performance = _dictionary_of_download(view, n, w, first_pass, reference_smoothing, transform_qps, transform_rate,
                                                         transform_sign_hiding, rd_pass, transform_rdoq, rd_pass_signalling, rd_pass_codec,
                                                         rd_pass_mode_stats, transform_skip, rd_skip)
        if keep_predictions:
            if first:
                targets_uint8 = view['targets'].copy()
            dictionary_performance['predictions_pnn_uint8'] = view['predictions_pnn'].copy()
            dictionary_performance['predictions_hevc_best_mode_uint8'] = view['predictions_hevc'].copy()
            dictionary_performance['targets_uint8'] = targets_uint8
        results[mask] = dictionary_performance
    if net_ipfcns is not None and (0, 0) in results:
        # the reference lines' origin is (row_1st + w - 8, col_1st + w - 8), in the context plane; the targets (of the target plane)
        # are on the device already
        d_targets = d_out[begin['targets']:].view(n, w, w)
        pred_u8, _, _, sses = net_ipfcns.predict_from_channels_device(d_context_channels, d_rows + (w - 8), d_cols + (w - 8), d_targets,
                                                                      pred_u8=keep_predictions)
        _fill_ipfcns_keys(results[(0, 0)], sses, w, pred_u8)
    return results


def coding_tree_from_scores(scores_by_width, left_depths=None, above_depths=None, device=0):
    """The coding-tree pass (include/pnn_hip.h, "the coding tree"; intraprediction.cu_tree) over the second passes of the five widths:
    which of the blocks that `frequency_rd_pass_win_pnn` counts HM's recursion would actually code, per 64 x 64 CTU and QP.
    scores_by_width: {4: .., 8: .., 16: .., 32: .., 64: ..}, each the dictionary of mask (0, 0) -- or the {(0, 0): dictionary} a call
    returns -- of score_masks_from_pictures / _picture_pairs with rd_pass=True and rd_pass_signalling=True (either codec, the same for
    all five) on the positions intraprediction.ctu_block_positions gives that width for ONE list of CTUs, so that every width's blocks
    arrive in (image, CTU, z-order) order.  The five must share their QPs, their codec (told by the slots per block) and their number
    of CTUs; a mismatch is a ValueError before anything touches the GPU.  left_depths / above_depths: as for cu_tree, per (QP, CTU) with
    the CTUs counted image-major.  The leaves are rebuilt on the host from the dictionaries' own arrays -- 'rd_pass_sses' and the two
    rates, 12 bytes per block and QP -- uploaded, and decided by pnn_cu_tree_device on `device`; lambda is HM's of each QP, as in the
    second passes.  Returns cu_tree's dictionary; the mode that stands for the PNN is 35 under the switch codec, 18 under substitution."""
    if not isinstance(scores_by_width, dict) or sorted(scores_by_width) != list(intraprediction.WIDTHS):
        raise ValueError('`scores_by_width` is not a dictionary with the keys 4, 8, 16, 32 and 64.')
    needed = ('transform_qps', 'rd_pass_sses', 'rd_pass_rate_bits', 'rd_pass_side_rate_bits', 'rd_pass_modes', 'rd_pass_candidates')
    leaves, qps, codec, n_ctu = {}, None, None, None
    for w in intraprediction.WIDTHS:
        d = scores_by_width[w]
        if isinstance(d, dict) and (0, 0) in d:
            d = d[(0, 0)]
        if not isinstance(d, dict) or any(key not in d for key in needed):
            raise ValueError('the dictionary of width %d lacks the second pass with signalling (rd_pass=True, rd_pass_signalling=True).' % w)
        slots = d['rd_pass_candidates'].shape[-1]
        names = [name for name in intraprediction.CODECS if intraprediction.rd_pass_slot_count(w, True, name) == slots]
        if len(names) != 1:
            raise ValueError('the dictionary of width %d has %d slots per block: no codec with signalling has.' % (w, slots))
        count = (intraprediction.CTU_WIDTH // w) ** 2
        n = d['rd_pass_sses'].shape[1]
        if n == 0 or n % count:
            raise ValueError('the dictionary of width %d holds %d blocks: not whole CTUs of %d.' % (w, n, count))
        if qps is None:
            qps, codec, n_ctu = tuple(d['transform_qps']), names[0], n // count
        if tuple(d['transform_qps']) != qps:
            raise ValueError('the dictionaries differ in their QPs (width %d).' % w)
        if names[0] != codec:
            raise ValueError('the dictionaries differ in their codec (width %d).' % w)
        if n // count != n_ctu:
            raise ValueError('the dictionaries differ in their CTU list (width %d: %d CTUs, width 4: %d).' % (w, n // count, n_ctu))
        # the rates are whole numbers of 2^-15 bit below 2^53: the division that made the bits and this multiplication are exact
        leaves[w] = (d['rd_pass_sses'], (d['rd_pass_rate_bits'] * 32768.).astype(np.uint64), (d['rd_pass_side_rate_bits'] * 32768.).astype(np.uint64),
                     d['rd_pass_modes'])
    pnn_mode = intraprediction.SUBSTITUTED_MODE if intraprediction.CODECS[codec] else intraprediction.NB_MODES
    return intraprediction.cu_tree(leaves, qps, None, left_depths, above_depths, pnn_mode, device)


def coding_tree_from_pictures(channels_uint8, predictors_by_width, means_by_width, row_1st, col_1st, ctu_rows, ctu_cols, qps, codec='switch',
                              pairs=False, keep_scores=False, reference_smoothing=0, transform_rate=False, transform_sign_hiding=False,
                              transform_rdoq=False, rd_pass_transform_skip=False, availability='all'):
    """From pictures to the pictures' coding tree (include/pnn_hip.h, "the coding tree over a picture"; intraprediction.cu_tree_picture)
    without the leaves leaving the device: what a picture costs with the PNN in HM's search, per image and QP.
    channels_uint8 [images, H, W, 1], or [images, H, W, 2] with pairs=True (score_masks_from_picture_pairs' planes); predictors_by_width
    / means_by_width: {4: .., 8: .., 16: .., 32: .., 64: ..}, a PredictionNeuralNetwork and its training mean per width, all on one
    device; (row_1st, col_1st): the top-left sample of the first CTU of a grid of ctu_rows x ctu_cols whole CTUs, the same in every
    image -- at least 64 from the picture's top and left, and far enough from its bottom and right, for the 64-wide contexts; qps:
    1 to 8 integers in [0, 51]; codec 'switch' or 'substitution'.  The other options are score_masks_from_pictures', given to every
    width (rd_pass_transform_skip to width 4 alone, where it exists).  Everything is checked before anything touches the GPU.
    Per width the calls score_masks_* make for mask (0, 0) with first_pass, rd_pass and rd_pass_signalling on the positions
    ctu_block_positions(w, *ctu_grid(..)), then pnn_cu_tree_leaves_device from the second pass's device outputs into leaf buffers
    kept here; then ONE pnn_cu_tree_picture_device call and ONE download, of the tree's outputs.  No neighbour modes are given to the
    second passes (rd_pass_neighbour_modes None).  Returns cu_tree_picture's dictionary -- the mode that stands for the PNN is 35
    under the switch codec, 18 under substitution; with keep_scores=True (dictionary, {w: mask (0, 0)'s dictionary of the width}),
    the five also downloaded as score_masks_* would (without it nothing but the tree's outputs is).  Everything is issued on the
    torch current stream of the predictors' device as it is when the call begins; nothing waits for it before the one download.
    availability: 'all' -- every block reads its complete context, mask (0, 0), the calls above entry for entry -- or 'hm': every block
    reads what HM's coding order leaves it (include/pnn_hip.h, "context availability"), each width's masks from
    intraprediction.hm_context_masks(w, ctu_rows, ctu_cols) and its three picture calls the *_masks_device entries (score_block_masks_*'s
    calls); keep_scores=True then returns the per-width dictionaries as score_block_masks_* would.  ValueError for any other name."""
    if availability not in ('all', 'hm'):
        raise ValueError("`availability` is not 'all' or 'hm'.")
    if not isinstance(predictors_by_width, dict) or sorted(predictors_by_width) != list(intraprediction.WIDTHS):
        raise ValueError('`predictors_by_width` is not a dictionary with the keys 4, 8, 16, 32 and 64.')
    if not isinstance(means_by_width, dict) or sorted(means_by_width) != list(intraprediction.WIDTHS):
        raise ValueError('`means_by_width` is not a dictionary with the keys 4, 8, 16, 32 and 64.')
    if any(p is None for p in predictors_by_width.values()):
        raise ValueError('a predictor is None.')
    devices = {predictors_by_width[w].device for w in intraprediction.WIDTHS}
    if len(devices) != 1:
        raise ValueError('the five predictors are not on one device.')
    if codec not in intraprediction.CODECS:
        raise ValueError("`codec` is not 'switch' or 'substitution'.")
    qps = intraprediction._check_qps(qps)
    if not isinstance(channels_uint8, np.ndarray) or channels_uint8.ndim != 4 or channels_uint8.shape[3] != (2 if pairs else 1):
        raise ValueError('`channels_uint8` is not an array [images, H, W, %d].' % (2 if pairs else 1))
    n_images, height, width = channels_uint8.shape[:3]
    ctu_rows, ctu_cols, n_images = intraprediction._check_ctu_grid(ctu_rows, ctu_cols, n_images)
    ctu_row_1sts, ctu_col_1sts = intraprediction.ctu_grid(row_1st, col_1st, ctu_rows, ctu_cols)
    positions = {w: intraprediction.ctu_block_positions(w, ctu_row_1sts, ctu_col_1sts) for w in intraprediction.WIDTHS}
    for w in intraprediction.WIDTHS:
        if positions[w][0].max() + 3 * w > height or positions[w][1].max() + 3 * w > width:
            raise ValueError('the grid with its contexts of width %d does not lie inside the picture.' % w)
    device = devices.pop()
    nq, per_image = len(qps), ctu_rows * ctu_cols

    import torch
    dev = torch.device('cuda', device)
    nb_planes = 2 if pairs else 1
    held, scores = {}, {}
    for w in intraprediction.WIDTHS:
        n = n_images * per_image * (intraprediction.CTU_WIDTH // w) ** 2
        held[w] = {'dist': torch.empty(nq * n, dtype=torch.int32, device=dev), 'rate': torch.empty(nq * n, dtype=torch.int64, device=dev),
                   'mode': torch.empty(nq * n, dtype=torch.uint8, device=dev), 'keep': bool(keep_scores)}
        block_masks = intraprediction.hm_context_masks(w, ctu_rows, ctu_cols) if availability == 'hm' else None
        result = _score_masks(channels_uint8, nb_planes, w, positions[w][0], positions[w][1], predictors_by_width[w], means_by_width[w],
                              () if availability == 'hm' else ((0, 0),), None, False, True, reference_smoothing, qps, transform_rate, transform_sign_hiding, True,
                              transform_rdoq, True, None, codec, False, 'off', bool(rd_pass_transform_skip) and w == 4, _tree_leaves=held[w],
                              _block_masks=block_masks)
        scores[w] = result[None if availability == 'hm' else (0, 0)]
    pnn_mode = intraprediction.SUBSTITUTED_MODE if intraprediction.CODECS[codec] else intraprediction.NB_MODES
    wanted = [True] * len(intraprediction.CU_TREE_PICTURE_OUTPUTS)
    leaf_pointers = [[held[w][name].data_ptr() for w in intraprediction.WIDTHS] for name in ('dist', 'rate', 'mode')]
    outs = intraprediction._cu_tree_picture_device(device, leaf_pointers, True, qps, None, n_images, ctu_rows, ctu_cols, pnn_mode, wanted)
    tree = intraprediction._cu_tree_picture_dictionary(outs, wanted, True, qps, None, n_images, ctu_rows, ctu_cols)
    return (tree, scores) if keep_scores else tree
