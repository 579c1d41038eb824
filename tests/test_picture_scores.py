"""CPU tests of the evaluator's scoring path from pictures: the two C-ABI entries are exported and bound, the argument errors of
evaluation.score_masks_from_pictures are raised before anything touches the predictor's context, and the pure-Python twin of the
descriptor kernel gives context.py's fields (the full 32-bit mask at w = 64 without a mask included)."""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_symbols_resolve_and_are_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pnn_score_pictures_device", "pnn_score_f32_device"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pnn_score_pictures_device"][1]) == 19
    assert len(_lib.SIGNATURES["pnn_score_f32_device"][1]) == 13
    header = open(os.path.join(ROOT, "include", "pnn_hip.h")).read()
    assert "reads d_rows / d_cols back" in header.lower()


class UntouchablePredictor(object):
    """Stands in for a PredictionNeuralNetwork; any use of its context (the first step towards the GPU) fails the test."""
    width_target = 8
    is_fully_connected = False
    device = 0

    @property
    def ctx(self):
        raise AssertionError("the context was touched before the arguments were checked")


def call(**changes):
    w = 8
    args = dict(channels_uint8=np.zeros((2, 3 * w + 5, 3 * w + 7, 1), np.uint8), width_target=w,
                row_1sts=np.array([0, 5], np.int32), col_1sts=np.array([7, 0], np.int32), predictor=UntouchablePredictor(),
                mean_training=util.MEAN, tuples_width_height_masks=((0, 0), (4, 8)))
    args.update(changes)
    return evaluation.score_masks_from_pictures(**args)


@pytest.mark.parametrize("changes, error, text", [
    (dict(channels_uint8=np.zeros((2, 29, 31, 1), np.int32)), TypeError, '`channels_single_or_pair_uint8.dtype` is not equal to `numpy.uint8`.'),
    (dict(row_1sts=np.array([0., 5.])), TypeError, '`row_1sts.dtype` is not smaller than `numpy.integer` in type hierarchy.'),
    (dict(col_1sts=np.array([7., 0.])), TypeError, '`col_1sts.dtype` is not smaller than `numpy.integer` in type hierarchy.'),
    (dict(col_1sts=np.array([7], np.int32)), ValueError, '`col_1sts.size` is not equal to `row_1sts.size`.'),
    (dict(channels_uint8=np.zeros((2, 29, 31, 3), np.uint8)), ValueError, '`channel_single_or_pair_uint8.shape[2]` does not belong to {1, 2}.'),
    (dict(channels_uint8=np.zeros((2, 29, 31, 2), np.uint8)), ValueError, '`channels_uint8.shape[3]` is not equal to 1 (pairs of channels: context.py).'),
    (dict(tuples_width_height_masks=((0, 0), (12, 0))), ValueError, '`tuple_width_height_masks[0]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.'),
    (dict(tuples_width_height_masks=((-4, 0),)), ValueError, '`tuple_width_height_masks[0]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.'),
    (dict(tuples_width_height_masks=((0, 2),)), ValueError, '`tuple_width_height_masks[1]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.'),
    (dict(tuples_width_height_masks=((0, 0), (8, 16))), ValueError, '`tuple_width_height_masks[1]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.'),
    (dict(row_1sts=np.array([0, -1], np.int32)), ValueError, '`row_1st` / `col_1st` is not positive.'),
    (dict(col_1sts=np.array([-3, 0], np.int32)), ValueError, '`row_1st` / `col_1st` is not positive.'),
    (dict(row_1sts=np.array([0, 6], np.int32)), ValueError, 'the context does not fit into the channel.'),
    (dict(col_1sts=np.array([8, 0], np.int32)), ValueError, 'the context does not fit into the channel.'),
    (dict(predictor=None), ValueError, "`predictor` (a PredictionNeuralNetwork holding the GPU context) is required"),
])
def test_argument_errors_come_before_any_device_call(changes, error, text):
    with pytest.raises(error) as info:
        call(**changes)
    assert str(info.value) == text


def test_the_stub_predictor_is_reached_only_by_valid_arguments():
    with pytest.raises(AssertionError):
        call()


def test_the_shared_errors_are_those_of_the_context_extraction():
    """Same exception types and texts as context.extract_context_portions_targets_from_channels_plus_preprocessing."""
    from context_adaptive_neural_network_based_prediction_amd import context
    w = 8
    good = dict(channels=np.zeros((2, 29, 31, 1), np.uint8), rows=np.array([0, 5], np.int32), cols=np.array([7, 0], np.int32), mask=(0, 0))
    cases = [dict(channels=np.zeros((2, 29, 31, 1), np.int16)), dict(rows=np.array([0., 5.])), dict(cols=np.array([0., 5.])),
             dict(cols=np.array([7], np.int32)), dict(channels=np.zeros((2, 29, 31, 3), np.uint8)), dict(mask=(12, 0)), dict(mask=(0, 6)),
             dict(rows=np.array([-1, 5], np.int32)), dict(cols=np.array([7, 8], np.int32)), dict(predictor=None)]
    for case in cases:
        a = dict(good, predictor=UntouchablePredictor())
        a.update(case)
        with pytest.raises((TypeError, ValueError)) as old:
            context.extract_context_portions_targets_from_channels_plus_preprocessing(a["channels"], w, a["rows"], a["cols"], util.MEAN,
                                                                                      a["mask"], False, predictor=a["predictor"])
        with pytest.raises((TypeError, ValueError)) as new:
            evaluation.score_masks_from_pictures(a["channels"], w, a["rows"], a["cols"], a["predictor"], util.MEAN, (a["mask"],))
        assert type(new.value) is type(old.value) and str(new.value) == str(old.value), case


def test_descriptor_fields_equal_the_loop_of_the_context_extraction():
    """context.py:54-61 written out again for every width, some masks and positions; ctypes holds the fields as the kernel does."""
    for w in (4, 8, 16, 32, 64):
        units = 2 * w // 4
        H, W = 3 * w + 9, 3 * w + 14
        for mask in sorted({(0, 0), (w, w), (4, w // 8 * 4), (w, 0)}):
            for i, r, c in ((0, 0, 0), (1, 9, 14), (3, 5, 3)):
                got = evaluation.context_descriptor_fields(w, H, W, i, r, c, mask)
                d = _lib.TbDev()
                d.origin, d.stride = (i * H + r + w) * W + c + w, W
                d.above_mask, d.left_units = (1 << (units - mask[0] // 4)) - 1, units - mask[1] // 4
                assert got == {'origin': d.origin, 'stride': d.stride, 'above_mask': d.above_mask, 'left_units': d.left_units}


def test_descriptor_fields_at_width_64():
    full = evaluation.context_descriptor_fields(64, 300, 400, 2, 10, 20, (0, 0))
    assert full == {'origin': (2 * 300 + 10 + 64) * 400 + 20 + 64, 'stride': 400, 'above_mask': 0xFFFFFFFF, 'left_units': 32}
    masked = evaluation.context_descriptor_fields(64, 300, 400, 2, 10, 20, (64, 64))
    assert masked == {'origin': full['origin'], 'stride': 400, 'above_mask': 0xFFFF, 'left_units': 16}
    assert evaluation.context_descriptor_fields(64, 1 << 16, 1 << 16, 1 << 12, 0, 0, (0, 0))['origin'] > 1 << 40      # int64, not int32
