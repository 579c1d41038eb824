"""GPU test of evaluation.coding_tree_from_scores: the second passes of the five widths over the blocks of two
CTUs of one small picture, then the coding tree over their winners on the GPU -- equal to intraprediction.cu_tree(device=None) on the
dictionaries' own arrays, for the switch codec from pictures and the substitution codec from pairs.  The tree changes nothing in the
per-width dictionaries: the same calls made again after it return the same bytes."""
import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cu_tree_cases
from tests import util
from tests.util import assert_same_dictionary

pytestmark = pytest.mark.gpu

QPS = (22, 37)
# Two CTUs side by side.  evaluation._check_score_masks_arguments wants every context corner (block position - w) at 0 or more and its
# 3w x 3w context inside the picture: the first CTU therefore starts at (64, 64), where the 64-wide block's corner is (0, 0), and the
# picture ends where the widest context of the second CTU does -- the smallest picture that holds both.
CTU_ROWS, CTU_COLS = np.array([64, 64]), np.array([64, 128])
POSITIONS = {w: ip.ctu_block_positions(w, CTU_ROWS, CTU_COLS) for w in ip.WIDTHS}
HEIGHT = max(int(POSITIONS[w][0].max()) + 3 * w for w in ip.WIDTHS)
WIDTH = max(int(POSITIONS[w][1].max()) + 3 * w for w in ip.WIDTHS)


def leaves_of(scores):
    out = {}
    for w, d in scores.items():
        d = d[(0, 0)]
        out[w] = (d['rd_pass_sses'], (d['rd_pass_rate_bits'] * 32768.).astype(np.uint64), (d['rd_pass_side_rate_bits'] * 32768.).astype(np.uint64),
                  d['rd_pass_modes'])
    return out


# For the substitution codec from pairs the tree on these real leaves is also held to the independent restatement of
# tests/cu_tree_cases.py, and the leaves themselves -- every width's rd_pass_sses, rd_pass_rate_bits, rd_pass_side_rate_bits and
# rd_pass_modes -- to the second pass's host twin on the dictionary's own targets and PNN predictions and host-extracted patterns, over
# all blocks of both CTUs (512 at w = 4: the twin takes a few hundredths of a second on them).
TREE_KEYS = ("cu_depths", "part_nxn", "node_costs", "ctu_costs", "ctu_dists", "ctu_rates", "selected", "selected_pnn")
LEAF_KEYS = {'rd_pass_sses': 'sses', 'rd_pass_rate_bits': 'rate_bits', 'rd_pass_side_rate_bits': 'side_rate_bits', 'rd_pass_modes': 'modes'}


def assert_tree_is_the_restatement(got, leaves, pnn_mode, label):
    """As tests/test_cu_tree.py holds the twin to the restatement, which takes rate plus side rate summed (cu_tree_cases.as_rd_pass_tuples
    in reverse)"""
    want = cu_tree_cases.restate({w: (d, r + side, m) for w, (d, r, side, m) in leaves.items()}, QPS, pnn_mode=pnn_mode)
    for key in TREE_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (label, key)
        assert got[key].tobytes() == want[key].tobytes(), "%s %s: %d differing values" % (label, key, (got[key] != want[key]).sum())


@pytest.mark.parametrize("codec, pairs", (('switch', False), ('substitution', True)))
def test_coding_tree_from_scores_equals_host_twin(codec, pairs):
    assert (HEIGHT, WIDTH) == (192, 256)
    pictures = util.pictures(2 if pairs else 1, HEIGHT, WIDTH, 5200)
    channels = np.ascontiguousarray(np.stack([pictures[0], pictures[1]], axis=-1)[None] if pairs else pictures[..., None])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    options = dict(keep_predictions=False, first_pass=True, reference_smoothing=2, transform_qps=QPS, transform_rate=True,
                   transform_sign_hiding=True, transform_rdoq=True, rd_pass=True, rd_pass_signalling=True, rd_pass_codec=codec)
    nets = {w: util.make_net(w, w <= 8, POSITIONS[w][0].size) for w in ip.WIDTHS}
    try:
        def all_widths():
            return {w: score(channels, w, POSITIONS[w][0], POSITIONS[w][1], nets[w], util.MEAN, ((0, 0),), **options) for w in ip.WIDTHS}

        before = all_widths()
        got = evaluation.coding_tree_from_scores(before, device=0)
        pnn_mode = 35 if codec == 'switch' else 18
        want = ip.cu_tree(leaves_of(before), QPS, pnn_mode=pnn_mode)
        assert_same_dictionary(got, want, codec)
        assert got['cu_depths'].shape == (2, 2, 64) and int(got['selected'].sum()) > 0
        rng = np.random.default_rng(3)
        left, above = (rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), size=(2, 2, 8)) for _ in range(2))
        assert_same_dictionary(evaluation.coding_tree_from_scores({w: d[(0, 0)] for w, d in before.items()}, left, above, device=0),
                               ip.cu_tree(leaves_of(before), QPS, None, left, above, pnn_mode), codec + " edges")
        after = all_widths()
        for w in ip.WIDTHS:
            assert_same_dictionary(after[w][(0, 0)], before[w][(0, 0)], "%s width %d" % (codec, w))
        if pairs:
            assert_tree_is_the_restatement(got, leaves_of(before), pnn_mode, codec + " restated")
            for w in ip.WIDTHS:                           # the tree's inputs: once more with the predictions kept, against the host twin
                rows, cols = POSITIONS[w]
                kept = score(channels, w, rows, cols, nets[w], util.MEAN, ((0, 0),), **dict(options, keep_predictions=True))[(0, 0)]
                patterns = ip.extract_intra_patterns(channels[..., -1:], w, rows + w - 1, cols + w - 1, (0, 0))[..., 0]
                host = ip.rd_pass(patterns, kept['targets_uint8'][..., 0], kept['predictions_pnn_uint8'][..., 0], QPS, reference_smoothing=2,
                                  sign_data_hiding=True, rdoq=True, signalling=True, codec=codec)
                assert_same_dictionary({k: kept[k] for k in LEAF_KEYS}, {k: host[v] for k, v in LEAF_KEYS.items()}, "%s leaves width %d" % (codec, w))
                assert_same_dictionary({k: before[w][(0, 0)][k] for k in LEAF_KEYS}, {k: kept[k] for k in LEAF_KEYS}, "%s kept width %d" % (codec, w))
    finally:
        for net in nets.values():
            net.close()


def test_mismatches_are_refused_before_the_gpu():
    def fake(w, qps=QPS, codec='switch', n_ctu=2):
        n = n_ctu * (64 // w) ** 2
        slots = ip.rd_pass_slot_count(w, True, codec)
        return {'transform_qps': qps, 'rd_pass_sses': np.zeros((len(qps), n), np.uint32), 'rd_pass_rate_bits': np.zeros((len(qps), n)),
                'rd_pass_side_rate_bits': np.zeros((len(qps), n)), 'rd_pass_modes': np.zeros((len(qps), n), np.uint8),
                'rd_pass_candidates': np.zeros((len(qps), n, slots), np.uint8)}

    good = {w: fake(w) for w in ip.WIDTHS}
    cases = {"QPs": fake(16, qps=(22, 38)), "codec": fake(16, codec='substitution'), "CTU list": fake(16, n_ctu=3)}
    for label, dictionary in cases.items():
        with pytest.raises(ValueError, match=label):
            evaluation.coding_tree_from_scores({w: dictionary if w == 16 else good[w] for w in ip.WIDTHS}, device=99)
    with pytest.raises(ValueError):
        evaluation.coding_tree_from_scores({w: good[w] for w in (4, 8, 16, 32)}, device=99)
    without = dict(good[8])
    del without['rd_pass_side_rate_bits']
    with pytest.raises(ValueError):
        evaluation.coding_tree_from_scores({w: without if w == 8 else good[w] for w in ip.WIDTHS}, device=99)
