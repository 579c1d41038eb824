"""GPU tests of the scoring path from PAIRS of pictures (pnn_score_picture_pairs_device, evaluation.score_masks_from_picture_pairs):
contexts, intra patterns and IPFCN-S lines from the decoded plane, targets and every SSE from the original.

Zero tolerance everywhere.  The yardstick is composed here from code the pair path does not touch: the context extraction on the
2-channel array (pinned on fixtures of the reference's sets/common.py), predict_by_batch_via_pnn, cast_float_to_uint8 and
compute_psnr for the PNN; extract_intra_patterns on the decoded plane and predict_series_via_hevc_best_mode with the original's
targets for HEVC; the line extraction on the pair and the net's forward for IPFCN-S.  Equality follows from the f32 order contract
(a block's bits depend neither on its batch nor on the entry point), one rounding rule and integer SSEs.

Pictures are (3w + 5) x (3w + 9), so the far position (5, 9) touches the last row and column; the decoded plane differs from the
original at EVERY pixel, so a plane read in the wrong place cannot go unnoticed."""

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, context, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
from context_adaptive_neural_network_based_prediction_amd.prediction_neural_network import predict_by_batch_via_pnn
from tests import util
from tests.util import PNN_E_ARG, POSITIONS, assert_same_dictionary, dev, ipfcns_params, picture_pairs, positions, ptr, untouched

pytestmark = pytest.mark.gpu

OUTPUTS = ("targets", "pnn_u8", "pnn_f32", "pnn_sse", "hevc_mode", "hevc_sse", "hevc_pred")


def make_net(w, kind, batch):
    return util.make_net(w, kind == "fc", batch)


def yardstick_outputs(pair, w, rows, cols, net, mask):
    """The seven outputs of the entry, from code it does not share: contexts (last channel) and targets (channel 0) by the context
    extraction, the net through the host-array path, the numpy cast, integer SSEs; the dense-pattern search on patterns of the
    decoded plane against those targets."""
    import torch
    n = pair.shape[0] * rows.size
    batches = context.extract_context_portions_targets_from_channels_plus_preprocessing(pair, w, rows, cols, util.MEAN, mask,
                                                                                        net.is_fully_connected, predictor=net)
    pnn_f32 = predict_by_batch_via_pnn(batches[0:-1], None, net, n)
    targets = evaluation.cast_float_to_uint8(batches[-1] + np.float32(util.MEAN))
    pnn_u8 = evaluation.cast_float_to_uint8(pnn_f32 + np.float32(util.MEAN))
    pnn_sse = ((pnn_u8.astype(np.int64) - targets) ** 2).sum(axis=(1, 2, 3)).astype(np.uint32)
    patterns = ip.extract_intra_patterns(pair[..., 1:2], w, rows + w - 1, cols + w - 1, mask)
    index, sse, pred, _ = ip.best_modes_device(dev(patterns[..., 0]), dev(targets[..., 0]), w)
    torch.cuda.synchronize()
    return [targets[..., 0], pnn_u8[..., 0], pnn_f32[..., 0], pnn_sse, index.cpu().numpy(), sse.cpu().numpy().view(np.uint32),
            pred.cpu().numpy()]


def yardstick_dictionary(pair, w, rows, cols, net, mask):
    """The reference's dictionary_performance of one mask for a pair, by the functions the evaluator has always scored with."""
    n = pair.shape[0] * rows.size
    batches = context.extract_context_portions_targets_from_channels_plus_preprocessing(pair, w, rows, cols, util.MEAN, mask,
                                                                                        net.is_fully_connected, predictor=net)
    predictions_float32 = predict_by_batch_via_pnn(batches[0:-1], None, net, n)
    targets_uint8 = evaluation.cast_float_to_uint8(batches[-1] + np.float32(util.MEAN))
    predictions_uint8 = evaluation.cast_float_to_uint8(predictions_float32 + np.float32(util.MEAN))
    patterns = ip.extract_intra_patterns(pair[..., 1:2], w, rows + w - 1, cols + w - 1, mask)
    indices, psnrs_hevc, predictions_hevc = ip.predict_series_via_hevc_best_mode(patterns, targets_uint8, device=net.device)
    psnrs_pnn = np.array([evaluation.compute_psnr(targets_uint8[i, :, :, 0], predictions_uint8[i, :, :, 0]) for i in range(n)])
    return {'indices_hevc_best_mode': indices, 'psnrs_hevc_best_mode': psnrs_hevc, 'psnrs_pnn': psnrs_pnn,
            'frequency_win_pnn': float(np.count_nonzero(psnrs_pnn - psnrs_hevc > 0.)) / n, 'mean_psnr_pnn': np.mean(psnrs_pnn).item(),
            'predictions_pnn_uint8': predictions_uint8, 'predictions_hevc_best_mode_uint8': predictions_hevc,
            'targets_uint8': targets_uint8}


def output_dtypes(n, w):
    return [(np.uint8, (n, w, w)), (np.uint8, (n, w, w)), (np.float32, (n, w, w)), (np.uint32, (n,)), (np.uint8, (n,)),
            (np.uint32, (n,)), (np.uint8, (n, w, w))]


def call(entry, ctx, w, planes, rows, cols, mask, wanted=(True,) * 7, shape=None, blocks=None):
    """Raw ABI call.  `planes`: the device tensors (or None) in the entry's order -- (context, target) for the pair entry, (picture,)
    for pnn_score_pictures_device.  Every output lies between guard bytes.  Returns (rc, the seven outputs as numpy -- None where
    one was not asked for --, whether every byte outside the asked-for outputs still is the guard)."""
    images, H, W = shape
    n = blocks if blocks is not None else images * len(rows)
    d_r, d_c = dev(np.asarray(rows, np.int32)), dev(np.asarray(cols, np.int32))
    front = (ctx, w, *[ptr(p) for p in planes], images, H, W, d_r.data_ptr(), d_c.data_ptr(), len(rows), mask[0], mask[1])
    return util.call(entry, front, (), output_dtypes(n, w), wanted)


def pair_call(ctx, w, pair, rows, cols, mask, **kw):
    kw.setdefault("shape", pair.shape[:3])
    return call("pnn_score_picture_pairs_device", ctx, w, (dev(pair[..., 1]), dev(pair[..., 0])), rows, cols, mask, **kw)


def assert_outputs_equal(got, want, label):
    for k, name in enumerate(OUTPUTS):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (label, name)
        assert got[k].tobytes() == want[k].tobytes(), "%s %s: %d differing values" % (label, name, (got[k] != want[k]).sum())


W4_MASKS, W16_MASKS = ((0, 0), (4, 0), (4, 4)), ((0, 0), (16, 0), (4, 16))          # (0, 0), (w, 0), (4, w)
CASES = [("fc", 4, W4_MASKS),                      # FC net: the separate gather
         ("conv", 16, W16_MASKS),                  # conv net: the gather fused into the first layer
         ("conv", 64, ((0, 0),))]                  # no mask at w = 64: all 32 bits of the above mask


@pytest.mark.parametrize("kind, w, masks", CASES, ids=["%s%d" % c[:2] for c in CASES])
def test_pairs_equal_the_composed_yardstick(kind, w, masks):
    pair = picture_pairs(2, w, 800 + w)
    rows, cols = positions()
    n = 2 * rows.size
    net = make_net(w, kind, n)
    got = evaluation.score_masks_from_picture_pairs(pair, w, rows, cols, net, util.MEAN, masks)
    assert list(got) == list(masks)
    for mask in masks:
        assert_same_dictionary(got[mask], yardstick_dictionary(pair, w, rows, cols, net, mask), "%s w %d mask %s" % (kind, w, mask))
        # the entry itself, every output (the floats and the integer SSEs are not in the dictionary)
        rc, out, intact = pair_call(net.ctx, w, pair, rows, cols, mask)
        assert rc == 0 and intact
        assert_outputs_equal(out, yardstick_outputs(pair, w, rows, cols, net, mask), "ABI %s w %d mask %s" % (kind, w, mask))
    lean = evaluation.score_masks_from_picture_pairs(pair, w, rows, cols, net, util.MEAN, masks[:1], keep_predictions=False)
    assert set(lean[masks[0]]) == {'indices_hevc_best_mode', 'psnrs_hevc_best_mode', 'psnrs_pnn', 'frequency_win_pnn', 'mean_psnr_pnn'}
    assert_same_dictionary(lean[masks[0]], {k: got[masks[0]][k] for k in lean[masks[0]]}, "lean")
    with pytest.raises(ValueError, match="`mean_training` differs from the predictor's mean"):
        evaluation.score_masks_from_picture_pairs(pair, w, rows, cols, net, util.MEAN + 1., masks)
    net.close()


def test_the_planes_are_not_interchangeable():
    """Right, swapped, decoded twice, original twice: each equals the yardstick on the pair so arranged, and against the right
    arrangement every output that reads a wrongly placed plane changes."""
    w, mask = 4, (0, 0)
    pair = picture_pairs(2, w, 810)
    rows, cols = positions()
    net = make_net(w, "fc", 6)
    original, decoded = pair[..., 0:1], pair[..., 1:2]
    arranged = {"right": pair, "swapped": np.concatenate([decoded, original], axis=3),
                "decoded twice": np.concatenate([decoded, decoded], axis=3), "original twice": np.concatenate([original, original], axis=3)}
    out = {}
    for name, a in arranged.items():
        rc, out[name], intact = pair_call(net.ctx, w, a, rows, cols, mask)
        assert rc == 0 and intact, name
        assert_outputs_equal(out[name], yardstick_outputs(a, w, rows, cols, net, mask), name)
    T, U8, F32, PSSE, MODE, HSSE, HPRED = range(7)
    # (changed, unchanged) against the right arrangement; the winning mode and, where only the targets move, its prediction may
    # survive, so nothing is claimed for them
    expect = {"swapped": ((T, U8, F32, PSSE, HSSE, HPRED), ()),                # both planes wrong
              "decoded twice": ((T, PSSE, HSSE), (U8, F32)),                    # targets from the wrong plane
              "original twice": ((U8, F32, PSSE, HSSE, HPRED), (T,))}           # contexts and intra patterns from the wrong plane
    for name, (changed, unchanged) in expect.items():
        for k in changed:
            assert out[name][k].tobytes() != out["right"][k].tobytes(), "%s: %s did not change" % (name, OUTPUTS[k])
        for k in unchanged:
            assert out[name][k].tobytes() == out["right"][k].tobytes(), "%s: %s changed" % (name, OUTPUTS[k])
    assert (out["swapped"][T] != out["right"][T]).all()                         # every pixel of every target
    net.close()


@pytest.mark.parametrize("kind, w, mask", [("fc", 4, (4, 0)), ("conv", 16, (4, 16))])
def test_equal_pointers_give_the_bytes_of_the_single_entry(kind, w, mask):
    pair = picture_pairs(2, w, 820 + w)
    rows, cols = positions()
    net = make_net(w, kind, 6)
    for plane in (pair[..., 0], pair[..., 1]):
        d_plane = dev(plane)
        rc, single, intact = call("pnn_score_pictures_device", net.ctx, w, (d_plane,), rows, cols, mask, shape=plane.shape)
        assert rc == 0 and intact
        rc, both, intact = call("pnn_score_picture_pairs_device", net.ctx, w, (d_plane, d_plane), rows, cols, mask, shape=plane.shape)
        assert rc == 0 and intact
        assert_outputs_equal(both, single, "equal pointers")
        # and two copies of one plane are that plane
        rc, copies, intact = call("pnn_score_picture_pairs_device", net.ctx, w, (d_plane, dev(plane)), rows, cols, mask, shape=plane.shape)
        assert rc == 0 and intact
        assert_outputs_equal(copies, single, "two copies")
    net.close()


def test_null_outputs_slices_and_empty_calls():
    w, mask = 4, (4, 4)
    pair = picture_pairs(2, w, 830)
    rows, cols = positions()
    n = 6
    net = make_net(w, "fc", n)
    rc, full, intact = pair_call(net.ctx, w, pair, rows, cols, mask)
    assert rc == 0 and intact
    # each output alone: its bits, nothing else written
    for k in range(7):
        wanted = tuple(j == k for j in range(7))
        rc, got, intact = pair_call(net.ctx, w, pair, rows, cols, mask, wanted=wanted)
        assert rc == 0 and intact, OUTPUTS[k]
        assert got[k].tobytes() == full[k].tobytes(), OUTPUTS[k]
    # the targets and the HEVC outputs alone need no model
    rc, got, intact = pair_call(ip._context(0), w, pair, rows, cols, mask, wanted=(True, False, False, False, True, True, True))
    assert rc == 0 and intact
    for k in (0, 4, 5, 6):
        assert got[k].tobytes() == full[k].tobytes(), OUTPUTS[k]
    # slices smaller than n (4 + 2, then one block each): the same bytes
    for chunk in (4, 1):
        net.set_option("max_chunk", chunk)
        rc, got, intact = pair_call(net.ctx, w, pair, rows, cols, mask)
        assert rc == 0 and intact
        assert_outputs_equal(got, full, "max_chunk %d" % chunk)
    net.set_option("max_chunk", 0)
    # n == 0 (no image, no position): nothing is written
    rc, got, intact = pair_call(net.ctx, w, pair[:0], rows, cols, mask, blocks=n)
    assert rc == 0 and intact and untouched(got)
    rc, got, intact = pair_call(net.ctx, w, pair, rows[:0], cols[:0], mask, blocks=n)
    assert rc == 0 and intact and untouched(got)
    net.close()


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    w, mask = 4, (0, 0)
    pair = picture_pairs(2, w, 840)
    rows, cols = positions()
    images, H, W = pair.shape[:3]
    net = make_net(w, "fc", 6)
    d_context, d_target = dev(pair[..., 1]), dev(pair[..., 0])

    def refused(planes=(d_context, d_target), rows=rows, cols=cols, shape=(images, H, W), mask=mask, wanted=(True,) * 7, w=w):
        rc, got, intact = call("pnn_score_picture_pairs_device", net.ctx, w, planes, rows, cols, mask, wanted=wanted, shape=shape, blocks=6)
        return rc == PNN_E_ARG and intact and untouched(got) and bool(L.pnn_last_error(net.ctx))

    assert refused(planes=(None, d_target)) and refused(planes=(d_context, None))                  # exactly one plane
    assert refused(planes=(None, d_target), shape=(0, H, W))                                          # ... also of an empty call
    assert refused(planes=(None, None))                                                               # no plane at all, n > 0
    assert refused(rows=[0, 6, 2]) and refused(cols=[0, 10, 5]) and refused(rows=[0, -1, 2]) and refused(cols=[-1, 9, 5])
    assert refused(shape=(images, H - 1, W)) and refused(shape=(images, H, W - 1))                  # the far context leaves the picture
    assert refused(mask=(8, 0)) and refused(mask=(0, 2)) and refused(w=12) and refused(wanted=(False,) * 7)
    rc, got, intact = call("pnn_score_picture_pairs_device", None, w, (d_context, d_target), rows, cols, mask, shape=(images, H, W))
    assert rc == PNN_E_ARG and intact and untouched(got)                                              # no context
    # and the same call with good arguments goes through
    rc, got, intact = call("pnn_score_picture_pairs_device", net.ctx, w, (d_context, d_target), rows, cols, mask, shape=(images, H, W))
    assert rc == 0 and intact
    net.close()


# the reference lines start at (row + w - 8, col + w - 8): at w = 4 the nearest corner a context may have is (4, 4), not (0, 0)
@pytest.mark.parametrize("kind, w, where", [("fc", 4, ((4, 4), (5, 9), (4, 7))), ("conv", 16, POSITIONS)])
def test_ipfcns_keys_lines_from_the_decoded_plane_sse_against_the_original(kind, w, where):
    pair = picture_pairs(2, w, 850 + w)
    rows, cols = positions(where)
    n = 2 * rows.size
    net = make_net(w, kind, n)
    ipf = I.NetIpfcns(w, ipfcns_params(w, 95 + w))
    masks = ((w, 0), (0, 0))
    got = evaluation.score_masks_from_picture_pairs(pair, w, rows, cols, net, util.MEAN, masks, net_ipfcns=ipf)
    want = yardstick_dictionary(pair, w, rows, cols, net, (0, 0))
    # the reference's IPFCN-S column: lines of the pair (its last channel), the net, + mean, the cast, the scores
    flattened, means = I.extract_pairs_groups_lines_from_channels_plus_preprocessing(pair, w, rows + w - 8, cols + w - 8)
    fc4 = I.predict_by_batch_via_ipfcns(flattened, ipf, w, n)
    predictions = evaluation.cast_float_to_uint8(fc4 + means[:, None, None, None])
    sses = ((predictions.astype(np.int64) - want['targets_uint8']) ** 2).sum(axis=(1, 2, 3))
    psnrs = ip.psnrs_from_sses(sses, w)
    want.update({'psnrs_ipfcns': psnrs, 'frequency_win_ipfcns': float(np.count_nonzero(psnrs - want['psnrs_hevc_best_mode'] > 0.)) / n,
                 'mean_psnr_ipfcns': np.mean(psnrs).item(), 'predictions_ipfcns_uint8': predictions})
    assert_same_dictionary(got[(0, 0)], want, "IPFCN-S w %d" % w)
    assert not any('ipfcns' in k for k in got[(w, 0)])
    assert_same_dictionary(got[(w, 0)], yardstick_dictionary(pair, w, rows, cols, net, (w, 0)), "(w, 0)")
    # lines from the original instead would have given other predictions; SSEs against the decoded targets other scores
    from_original, _ = I.extract_pairs_groups_lines_from_channels_plus_preprocessing(pair[..., 0:1], w, rows + w - 8, cols + w - 8)
    assert from_original.tobytes() != flattened.tobytes()
    net.close()
    ipf.close()
