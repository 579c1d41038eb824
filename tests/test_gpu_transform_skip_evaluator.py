"""GPU tests of the evaluator's transform-skip options: evaluation.score_masks_from_pictures / _picture_pairs with
transform_skip='forced' / 'decide' and rd_pass_transform_skip=True at width 4.  The new keys and the keys the options change equal the dense
Python entries (intraprediction.transform_code and rd_pass, host twins) on the dictionary's own patterns, targets, predictions and best
modes; every other key has the bytes of the call without the options; the defaults change no key and no byte."""
import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import util
from tests.util import assert_same_dictionary, picture_pairs

pytestmark = pytest.mark.gpu

W, QPS = 4, (22, 37)
COLUMNS = (('pnn', 'predictions_pnn_uint8'), ('hevc_best_mode', 'predictions_hevc_best_mode_uint8'))
TRANSFORM_KEYS = tuple('%s_%s' % (name, column) for column, _ in COLUMNS
                       for name in ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'psnrs_recon', 'rate_bits')) + \
    ('frequency_recon_win_pnn', 'frequency_rate_win_pnn')
RD_KEYS = ('rd_pass_candidates', 'rd_pass_costs', 'rd_pass_modes', 'rd_pass_sses', 'rd_pass_rate_bits', 'psnrs_recon_rd_pass',
           'frequency_rd_pass_win_pnn', 'rd_pass_side_rate_bits')


@pytest.mark.parametrize("codec", ('switch', 'substitution'))
def test_evaluator_keys_against_the_dense_python_entries(codec):
    pair = picture_pairs(2, W, 3100 + W)
    single = np.ascontiguousarray(pair[..., 0:1])
    rows, cols = np.array([0, 5, 2, 3, 1]), np.array([0, 9, 5, 2, 7])
    n = 2 * rows.size
    masks = ((0, 0), (4, W))
    rng = np.random.default_rng(31)
    left = rng.integers(0, 35, n).astype(np.uint8)
    above = np.where(rng.integers(0, 3, n) == 0, 255, rng.integers(0, 35, n)).astype(np.uint8)
    pnn_mode = 35 if codec == 'switch' else 18
    net = util.make_net(W, True, n)
    try:
        for name, channels, score in (("pictures", single, evaluation.score_masks_from_pictures),
                                      ("pairs", pair, evaluation.score_masks_from_picture_pairs)):
            options = dict(first_pass=True, reference_smoothing=2, transform_qps=QPS, transform_rate=True, transform_sign_hiding=True,
                           transform_rdoq=True, rd_pass=True, rd_pass_signalling=True, rd_pass_neighbour_modes=(left, above), rd_pass_codec=codec)
            plain = score(channels, W, rows, cols, net, util.MEAN, masks, **options)
            off = score(channels, W, rows, cols, net, util.MEAN, masks, transform_skip='off', rd_pass_transform_skip=False, **options)
            context = channels[..., -1:]
            for option in ('forced', 'decide'):
                got = score(channels, W, rows, cols, net, util.MEAN, masks, transform_skip=option, rd_pass_transform_skip=True, **options)
                for mask in masks:
                    label = "%s %s mask %s %s" % (name, codec, mask, option)
                    assert_same_dictionary(off[mask], plain[mask], label)                 # the defaults: no key and no byte differs
                    g = got[mask]
                    new = {'transform_skip', 'rd_pass_best_transform_skip', 'frequency_rd_pass_transform_skip'} | \
                        {'%s_%s' % (k, column) for column, _ in COLUMNS for k in ('transform_skip_flags', 'frequency_transform_skip')}
                    assert set(g) == set(plain[mask]) | new, label
                    changed = set(TRANSFORM_KEYS) | set(RD_KEYS) | new
                    assert_same_dictionary({k: v for k, v in g.items() if k not in changed},
                                           {k: v for k, v in plain[mask].items() if k not in changed}, label)
                    assert g['transform_skip'] == option
                    targets = g['targets_uint8'][..., 0]
                    for column, predictions in COLUMNS:                                   # the transform-domain column: transform_code's host twin
                        modes = g['indices_hevc_best_mode'] if column == 'hevc_best_mode' else None
                        host = ip.transform_code(g[predictions][..., 0], targets, QPS, modes=modes, rate=True, sign_data_hiding=True, rdoq=True,
                                                 transform_skip=option)
                        want = {'%s_%s' % (k, column): host[k] for k in ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'psnrs_recon', 'rate_bits')}
                        want['transform_skip_flags_' + column] = host['transform_skip_flags']
                        want['frequency_transform_skip_' + column] = [float(np.count_nonzero(f)) / n for f in host['transform_skip_flags']]
                        assert_same_dictionary({k: g[k] for k in want}, want, label + " " + column)
                    patterns = ip.extract_intra_patterns(context, W, rows + W - 1, cols + W - 1, mask)[..., 0]
                    host = ip.rd_pass(patterns, targets, g['predictions_pnn_uint8'][..., 0], QPS, reference_smoothing=2, sign_data_hiding=True, rdoq=True,
                                      signalling=True, neighbour_modes=(left, above), codec=codec, transform_skip=True)
                    want = {'rd_pass_candidates': host['candidates'], 'rd_pass_costs': host['costs'], 'rd_pass_modes': host['modes'],
                            'rd_pass_sses': host['sses'], 'rd_pass_rate_bits': host['rate_bits'], 'psnrs_recon_rd_pass': host['psnrs_recon'],
                            'frequency_rd_pass_win_pnn': [float(np.count_nonzero(m == pnn_mode)) / n for m in host['modes']],
                            'rd_pass_side_rate_bits': host['side_rate_bits'], 'rd_pass_best_transform_skip': host['best_transform_skip'],
                            'frequency_rd_pass_transform_skip': [float(np.count_nonzero(f)) / n for f in host['best_transform_skip']]}
                    assert_same_dictionary({k: g[k] for k in want}, want, label + " second pass")
    finally:
        net.close()
