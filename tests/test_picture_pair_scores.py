"""CPU tests of the scoring path from PAIRS of pictures (original, HEVC-decoded): pnn_score_picture_pairs_device is exported and
bound, and the argument errors of evaluation.score_masks_from_picture_pairs are raised before anything touches the GPU, with the
messages of context.extract_context_portions_targets_from_channels_plus_preprocessing where that function has one."""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, context, evaluation
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pair_symbol_resolves_and_is_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "pnn_score_picture_pairs_device")
    res, args = _lib.SIGNATURES["pnn_score_picture_pairs_device"]
    assert res is ctypes.c_int and len(args) == 20
    # pnn_score_pictures_device's arguments with the one picture pointer doubled
    single = _lib.SIGNATURES["pnn_score_pictures_device"][1]
    assert args == single[:3] + [ctypes.c_void_p] + single[3:]
    header = open(os.path.join(ROOT, "include", "pnn_hip.h")).read()
    assert "pnn_score_picture_pairs_device(" in header
    assert "THIS PROJECT'S DEFINITION" in header            # which plane feeds the intra pattern is stated, and stated as ours


class UntouchablePredictor(object):
    """Stands in for a PredictionNeuralNetwork; any use of its context (the first step towards the GPU) fails the test."""
    width_target = 8
    is_fully_connected = False
    device = 0

    @property
    def ctx(self):
        raise AssertionError("the context was touched before the arguments were checked")


class MeanZeroPredictor(object):
    """A predictor without a context: pnn_mean(NULL) is 0 (pure host code), so any training mean but 0 differs from its mean."""
    width_target = 8
    is_fully_connected = False
    device = 0
    ctx = None


def call(**changes):
    w = 8
    args = dict(channels_pair_uint8=np.zeros((2, 3 * w + 5, 3 * w + 7, 2), np.uint8), width_target=w,
                row_1sts=np.array([0, 5], np.int32), col_1sts=np.array([7, 0], np.int32), predictor=UntouchablePredictor(),
                mean_training=util.MEAN, tuples_width_height_masks=((0, 0), (4, 8)))
    args.update(changes)
    return evaluation.score_masks_from_picture_pairs(**args)


@pytest.mark.parametrize("changes, error, text", [
    (dict(channels_pair_uint8=np.zeros((2, 29, 31, 2), np.int32)), TypeError, '`channels_single_or_pair_uint8.dtype` is not equal to `numpy.uint8`.'),
    (dict(channels_pair_uint8=np.zeros((2, 29, 31), np.uint8)), ValueError, '`channels_uint8.ndim` is not equal to 4.'),
    (dict(channels_pair_uint8=np.zeros((2, 29, 31, 2, 1), np.uint8)), ValueError, '`channels_uint8.ndim` is not equal to 4.'),
    (dict(channels_pair_uint8=np.zeros((2, 29, 31, 3), np.uint8)), ValueError, '`channel_single_or_pair_uint8.shape[2]` does not belong to {1, 2}.'),
    (dict(channels_pair_uint8=np.zeros((2, 29, 31, 1), np.uint8)), ValueError,
     '`channels_pair_uint8.shape[3]` is not equal to 2 (single pictures: score_masks_from_pictures).'),
    (dict(row_1sts=np.array([0., 5.])), TypeError, '`row_1sts.dtype` is not smaller than `numpy.integer` in type hierarchy.'),
    (dict(col_1sts=np.array([7], np.int32)), ValueError, '`col_1sts.size` is not equal to `row_1sts.size`.'),
    (dict(row_1sts=np.array([0, -1], np.int32)), ValueError, '`row_1st` / `col_1st` is not positive.'),
    (dict(row_1sts=np.array([0, 6], np.int32)), ValueError, 'the context does not fit into the channel.'),
    (dict(col_1sts=np.array([8, 0], np.int32)), ValueError, 'the context does not fit into the channel.'),
    (dict(tuples_width_height_masks=((0, 0), (12, 0))), ValueError, '`tuple_width_height_masks[0]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.'),
    (dict(tuples_width_height_masks=((0, 2),)), ValueError, '`tuple_width_height_masks[1]` does not belong to {0, 4, ..., `targets_uint8.shape[1]`}.'),
    (dict(predictor=None), ValueError, "`predictor` (a PredictionNeuralNetwork holding the GPU context) is required"),
    (dict(predictor=MeanZeroPredictor()), ValueError, "`mean_training` differs from the predictor's mean"),
])
def test_argument_errors_come_before_any_device_call(changes, error, text):
    with pytest.raises(error) as info:
        call(**changes)
    assert str(info.value) == text


def test_the_stub_predictor_is_reached_only_by_valid_arguments():
    with pytest.raises(AssertionError):
        call()


def test_the_shared_errors_are_those_of_the_context_extraction_on_the_same_pair():
    """Same exception types and texts as context.extract_context_portions_targets_from_channels_plus_preprocessing, which takes pairs."""
    w = 8
    good = dict(channels=np.zeros((2, 29, 31, 2), np.uint8), rows=np.array([0, 5], np.int32), cols=np.array([7, 0], np.int32), mask=(0, 0),
                predictor=UntouchablePredictor())
    cases = [dict(channels=np.zeros((2, 29, 31, 2), np.int16)), dict(rows=np.array([0., 5.])), dict(cols=np.array([0., 5.])),
             dict(cols=np.array([7], np.int32)), dict(channels=np.zeros((2, 29, 31, 3), np.uint8)), dict(mask=(12, 0)), dict(mask=(0, 6)),
             dict(rows=np.array([-1, 5], np.int32)), dict(cols=np.array([7, 8], np.int32)), dict(predictor=None)]
    for case in cases:
        a = dict(good)
        a.update(case)
        with pytest.raises((TypeError, ValueError)) as old:
            context.extract_context_portions_targets_from_channels_plus_preprocessing(a["channels"], w, a["rows"], a["cols"], util.MEAN,
                                                                                      a["mask"], False, predictor=a["predictor"])
        with pytest.raises((TypeError, ValueError)) as new:
            evaluation.score_masks_from_picture_pairs(a["channels"], w, a["rows"], a["cols"], a["predictor"], util.MEAN, (a["mask"],))
        assert type(new.value) is type(old.value) and str(new.value) == str(old.value), case
