"""GPU test of evaluation.coding_tree_from_pictures: from a seeded 256 x 256 picture (pair) to the tree of its
2 x 2 CTUs without the leaves leaving the device -- equal, byte for byte, to the chain it replaces: the five score_masks_* calls with
the same options, the leaves built as evaluation.coding_tree_from_scores builds them, intraprediction.cu_tree_picture(device=None).
For the switch codec from pictures and the substitution codec from pairs.  The per-width score calls made again afterwards return the
same bytes, and the chained tree differs from coding_tree_from_scores with edges absent in at least one CTU's map.

The picture, its grid, the options and the picture seeds (chosen on the host path; how to find them again) are
tests/cu_tree_picture_cases.py's, shared with tools/cu_tree_picture_rate.py.

That test has one image and a square grid, and its yardstick's leaves come from the same GPU second passes in the same order.
test_coding_tree_from_pictures_equals_the_host_built_yardstick runs two images on a 1 x 2 and on a 2 x 1 grid, the switch codec from
pairs with transform skip and the substitution codec from pictures, and transform skip on the 2 x 2 grid, against a yardstick built
on the host image by image; the cases, the yardstick, the floors and the seeds tried are tests/cu_tree_picture_cases.py's."""
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


PER_CTU = ('cu_depths', 'part_nxn', 'node_costs', 'ctu_costs', 'ctu_dists', 'ctu_rates')


def assert_tree_is_the_yardstick(got, want, label):
    for key in pc.TREE_KEYS + ('image_dists',):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (label, key)
        assert got[key].tobytes() == want[key].tobytes(), "%s %s: %d differing values" % (label, key, (got[key] != want[key]).sum())
    # 'image_rates' leaves cu_tree_picture's dictionary as bits: whole numbers of 2^-15 bit below 2^53, so the product is exact
    rates = got['image_rate_bits'] * 32768.
    assert rates.shape == want['image_rates'].shape and np.array_equal(rates, want['image_rates'].astype(np.float64)), label
    assert np.array_equal(rates.astype(np.uint64), want['image_rates']), label


@pytest.mark.parametrize("name", ('A', 'B', 'crossing'))
def test_coding_tree_from_pictures_equals_the_host_built_yardstick(name):
    """Two images on a 1 x 2 grid (switch codec from pairs, transform skip at width 4) and on a 2 x 1 grid (substitution codec from
    pictures), and transform skip on the 2 x 2 grid: coding_tree_from_pictures against a yardstick that goes neither through a device
    call on more than one image nor through the second pass on the device nor through the picture entries of the tree
    (tests/cu_tree_picture_cases.py: host_leaves, yardstick), byte for byte; the kept scores; a batch against its images one at a
    time; and the floors that keep all this from passing vacuously, computed from the yardstick alone."""
    case = pc.EVALUATOR_CASES[name]
    n_images, rows, cols, codec, pairs = case['n_images'], case['ctu_rows'], case['ctu_cols'], case['codec'], case['pairs']
    positions = pc.case_positions(case)
    assert max(int(positions[w][0].max()) + 3 * w for w in ip.WIDTHS) == case['height']
    assert max(int(positions[w][1].max()) + 3 * w for w in ip.WIDTHS) == case['width']
    blocks = {w: n_images * positions[w][0].size for w in ip.WIDTHS}
    if n_images == 2:
        assert blocks[4] == 1024 and blocks[64] == 4
    channels = pc.case_channels(case)
    assert channels.shape == (n_images, case['height'], case['width'], 2 if pairs else 1)
    assert n_images == 1 or not np.array_equal(channels[0], channels[1])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    nets = {w: util.make_net(w, w <= 8, blocks[w]) for w in ip.WIDTHS}
    means = dict.fromkeys(ip.WIDTHS, util.MEAN)
    try:
        def tree(pictures, **options):
            return evaluation.coding_tree_from_pictures(pictures, nets, means, pc.ROW_1ST, pc.COL_1ST, rows, cols, QPS, codec, pairs,
                                                        rd_pass_transform_skip=case['transform_skip'], **dict(OPTIONS, **options))

        # the yardstick, and where it is built: one image alone and the same image in a batch give the same predictions
        host = pc.host_leaves(case, channels, nets)
        both = {w: score(channels, w, positions[w][0], positions[w][1], nets[w], util.MEAN, ((0, 0),), **pc.case_score_options(case, w, True))[(0, 0)]
                for w in ip.WIDTHS}
        for w in ip.WIDTHS:
            for key in ('predictions_pnn_uint8', 'targets_uint8'):
                assert both[w][key].shape == host[w][key].shape and both[w][key].tobytes() == host[w][key].tobytes(), \
                    "%s width %d %s: an image alone and in a batch of %d differ" % (name, w, key, n_images)
        leaves = pc.tree_leaves_of_host(host)
        want = pc.case_yardstick(case, leaves)

        got = tree(channels)
        assert_tree_is_the_yardstick(got, want, name)
        assert_same_dictionary(got, ip.cu_tree_picture({w: (d, r, np.zeros_like(r), m) for w, (d, r, m) in leaves.items()}, QPS, n_images, rows, cols,
                                                       pnn_mode=pc.case_pnn_mode(case)), name + " against the host twin")
        assert got['cu_depths'].shape == (2, n_images * rows * cols, 64) and got['image_dists'].shape == (2, n_images)

        # the scores kept: the same tree; each width's dictionary is score_masks_*'s on all images in one call, its leaves the host twin's
        kept_tree, scores = tree(channels, keep_scores=True)
        assert_same_dictionary(kept_tree, got, name + " with the scores kept")
        for w in ip.WIDTHS:
            plain = score(channels, w, positions[w][0], positions[w][1], nets[w], util.MEAN, ((0, 0),), **pc.case_score_options(case, w, False))[(0, 0)]
            assert_same_dictionary(scores[w], plain, "%s kept scores width %d" % (name, w))
            assert_same_dictionary({k: scores[w][k] for k in pc.LEAF_KEYS}, {k: host[w][v] for k, v in pc.LEAF_KEYS.items()},
                                   "%s leaves width %d" % (name, w))

        # a batch equals its images one at a time
        if n_images == 2:
            per_image = rows * cols
            singles = [tree(channels[i:i + 1]) for i in range(2)]
            for i, single in enumerate(singles):
                for key in PER_CTU:
                    part = got[key][:, i * per_image:(i + 1) * per_image]
                    assert single[key].shape == part.shape and single[key].tobytes() == np.ascontiguousarray(part).tobytes(), (name, i, key)
                for key in ('image_dists', 'image_rate_bits', 'psnr_images', 'bits_per_pixel_images'):
                    assert np.array_equal(single[key][:, 0], got[key][:, i]), (name, i, key)
            for key in ('selected', 'selected_pnn'):
                assert np.array_equal(singles[0][key] + singles[1][key], got[key]), (name, key)

        # the floors, from the yardstick alone
        floors = pc.evaluator_floors(case, leaves, want)
        print("%s: %s" % (name, floors))
        assert floors['edges'] >= 1 and floors['context_share'] > 0., floors
        if n_images == 2:                                 # (the crossing's grid is square: exchanged it is the same grid)
            assert floors['transposed'] >= 1, floors
            assert floors['first_of_image_1_alone'] and floors['stacked'], floors
            assert floors['depth_maps_differ'] and floors['image_dists_differ'], floors
        if case['transform_skip']:
            without = pc.host_leaves(case, channels, nets, transform_skip=False)[4]
            moved = sum(int((without[key] != host[4][key]).sum()) for key in pc.LEAF_KEYS.values())
            print("%s: %d width-4 leaf values differ between transform skip on and off" % (name, moved))
            assert moved >= 1
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
