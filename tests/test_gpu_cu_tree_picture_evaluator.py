"""GPU test of evaluation.coding_tree_from_pictures: from a seeded 256 x 256 picture (pair) to the tree of its
2 x 2 CTUs without the leaves leaving the device -- equal, byte for byte, to the chain it replaces: the five score_masks_* calls with
the same options, the leaves built as evaluation.coding_tree_from_scores builds them, intraprediction.cu_tree_picture(device=None).
For the switch codec from pictures and the substitution codec from pairs.  The per-width score calls made again afterwards return the
same bytes, and the chained tree differs from coding_tree_from_scores with edges absent in at least one CTU's map.

The picture, its grid, the options and the picture seeds (chosen on the host path; how to find them again) are
tests/cu_tree_picture_cases.py's, shared with tools/cu_tree_picture_rate.py."""
import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cu_tree_picture_cases as pc
from tests import util
from tests.util import assert_same_dictionary

pytestmark = pytest.mark.gpu

QPS, SEEDS, OPTIONS, POSITIONS = pc.EVALUATOR_QPS, pc.SEEDS, pc.OPTIONS, pc.POSITIONS
ROW_1ST, COL_1ST, CTU_ROWS, CTU_COLS, SIDE = pc.ROW_1ST, pc.COL_1ST, pc.CTU_ROWS, pc.CTU_COLS, pc.SIDE
leaves_of, channels_of = pc.leaves_of_scores, pc.evaluator_channels


@pytest.mark.parametrize("codec, pairs", (('switch', False), ('substitution', True)))
def test_coding_tree_from_pictures_equals_the_chain_through_the_host(codec, pairs):
    assert max(int(POSITIONS[w][0].max()) + 3 * w for w in ip.WIDTHS) == SIDE and max(int(POSITIONS[w][1].max()) + 3 * w for w in ip.WIDTHS) == SIDE
    channels = channels_of(pairs, SEEDS[codec])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    options = dict(OPTIONS, keep_predictions=False, first_pass=True, transform_qps=QPS, rd_pass=True, rd_pass_signalling=True, rd_pass_codec=codec)
    nets = {w: util.make_net(w, w <= 8, POSITIONS[w][0].size) for w in ip.WIDTHS}
    means = dict.fromkeys(ip.WIDTHS, util.MEAN)
    try:
        def all_widths():
            return {w: score(channels, w, POSITIONS[w][0], POSITIONS[w][1], nets[w], util.MEAN, ((0, 0),), **options) for w in ip.WIDTHS}

        before = all_widths()
        pnn_mode = 35 if codec == 'switch' else 18
        want = ip.cu_tree_picture(leaves_of(before), QPS, 1, CTU_ROWS, CTU_COLS, pnn_mode=pnn_mode)
        got = evaluation.coding_tree_from_pictures(channels, nets, means, ROW_1ST, COL_1ST, CTU_ROWS, CTU_COLS, QPS, codec, pairs, **OPTIONS)
        assert_same_dictionary(got, want, codec)
        assert got['cu_depths'].shape == (2, 4, 64) and got['image_dists'].shape == (2, 1) and int(got['selected'].sum()) > 0
        got, scores = evaluation.coding_tree_from_pictures(channels, nets, means, ROW_1ST, COL_1ST, CTU_ROWS, CTU_COLS, QPS, codec, pairs,
                                                           keep_scores=True, **OPTIONS)
        assert_same_dictionary(got, want, codec + " with the scores kept")
        after = all_widths()
        for w in ip.WIDTHS:
            assert_same_dictionary(scores[w], before[w][(0, 0)], "%s kept scores width %d" % (codec, w))
            assert_same_dictionary(after[w][(0, 0)], before[w][(0, 0)], "%s width %d" % (codec, w))
        unchained = evaluation.coding_tree_from_scores(before, device=0)
        differing = int((unchained['cu_depths'] != got['cu_depths']).any(axis=2).sum())
        print("%s: %d of 8 (QP, CTU) maps differ from the unchained tree" % (codec, differing))
        assert differing >= 1
    finally:
        for net in nets.values():
            net.close()


def test_arguments_are_checked_before_the_gpu():
    class Fake:                                           # stands for a predictor: only the device is read before the checks end
        def __init__(self, device):
            self.device = device

    nets = {w: Fake(99) for w in ip.WIDTHS}
    means = dict.fromkeys(ip.WIDTHS, util.MEAN)
    channels = np.zeros((1, SIDE, SIDE, 1), np.uint8)
    good = dict(channels_uint8=channels, predictors_by_width=nets, means_by_width=means, row_1st=64, col_1st=64, ctu_rows=2, ctu_cols=2, qps=QPS)
    for label, kwargs in (("four predictors", dict(predictors_by_width={w: nets[w] for w in (4, 8, 16, 32)})),
                          ("two devices", dict(predictors_by_width={**nets, 16: Fake(98)})),
                          ("a predictor missing", dict(predictors_by_width={**nets, 16: None})),
                          ("four means", dict(means_by_width={w: util.MEAN for w in (4, 8, 16, 32)})),
                          ("grid beyond the bottom", dict(ctu_rows=3)), ("grid beyond the right", dict(ctu_cols=3)),
                          ("no context above", dict(row_1st=63)), ("no context left", dict(col_1st=0)), ("grid moved out", dict(row_1st=65)),
                          ("no CTU", dict(ctu_rows=0)), ("QP 52", dict(qps=(22, 52))), ("no QP", dict(qps=())), ("a codec", dict(codec='other')),
                          ("pairs without the second plane", dict(pairs=True)), ("three dimensions", dict(channels_uint8=channels[0]))):
        arguments = dict(good)
        arguments.update(kwargs)
        with pytest.raises(ValueError):
            evaluation.coding_tree_from_pictures(**arguments)
