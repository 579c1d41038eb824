"""GPU tests of the second intra pass read from picture planes at all five widths (stage_blocks<W, G, PIC = true> through
picture_corner, csrc/pnn_hevc_intra.hip; the masks as ph / pw from set_blocks, csrc/pnn_eval.cpp): the three picture-pair entries
against the host twin on blocks cut out on the host, single pictures as pairs with equal planes, a batch against its images one at a
time, and the evaluator's rd_pass_* keys at the widths its other tests leave out.  The cases, the yardstick and the conditions it
meets are tests/rd_pass_picture_cases.py's (tests/test_rd_pass_pictures.py asserts the conditions without a GPU).  Every comparison
is equality of bytes (doubles by bit pattern); every raw call lies between guard bytes and gets exactly the scratch its
*_workspace_bytes function names."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import rd_pass_picture_cases as cases
from tests import util
from tests.util import assert_same_dictionary, dev

pytestmark = pytest.mark.gpu

ENTRIES = {'plain': "pnn_rd_pass_rdoq_picture_pairs_device", 'switch': "pnn_rd_pass_signal_picture_pairs_device",
           'substitution': "pnn_rd_pass_codec_picture_pairs_device"}


def outputs_of(rung, w, n):
    """[(name, dtype, shape)] of the entry's outputs, in its order"""
    nq = len(cases.QPS)
    if rung == 'plain':
        return [(name, dtype, shape) for (name, dtype), shape in zip(ip.RD_PASS_OUTPUTS, ip.rd_pass_shapes(n, nq, w))]
    return [(name, dtype, shape) for (name, dtype), shape in zip(ip.RD_PASS_SIGNAL_OUTPUTS, ip.rd_pass_signal_shapes(n, nq, w, rung))]


def workspace_bytes(rung, w, n):
    L, nq = _lib.lib(), len(cases.QPS)
    return {'plain': lambda: L.pnn_rd_pass_workspace_bytes(w, n, nq), 'switch': lambda: L.pnn_rd_pass_signal_workspace_bytes(w, n, nq, 1),
            'substitution': lambda: L.pnn_rd_pass_codec_workspace_bytes(w, n, nq, 1, 1)}[rung]()


def picture_call(w, rung, mask, smoothing, context, target, rows, cols, candidates, left, above):
    """One raw call of the rung's picture-pair entry, all outputs asked for: RDOQ and sign-data hiding on, cases.QPS, HM's lambdas.
    context / target: [images, H, W] uint8 planes, or target None for the single-picture form (both pointers equal).
    -> {name: array}"""
    import torch
    images, height, width = context.shape
    n, nq = images * rows.size, len(cases.QPS)
    d_context = dev(np.array(context))                    # (copies: the shared cases are read-only)
    d_target = d_context if target is None else dev(np.array(target))
    d = [dev(a) for a in (rows.astype(np.int32), cols.astype(np.int32), np.array(candidates))]
    d_left, d_above = (None if a is None else dev(np.array(a)) for a in (left, above))
    nb = workspace_bytes(rung, w, n)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    front = (ip._context(0), w, d_context.data_ptr(), d_target.data_ptr(), images, height, width, d[0].data_ptr(), d[1].data_ptr(), rows.size,
             mask[0], mask[1], d[2].data_ptr(), smoothing, (ctypes.c_int * nq)(*cases.QPS), nq, None, 1, 1)
    if rung != 'plain':
        front += (1, util.ptr(d_left), util.ptr(d_above)) + ((1,) if rung == 'substitution' else ())
    outputs = outputs_of(rung, w, n)
    rc, outs, intact = util.call(ENTRIES[rung], front, (), [(dtype, shape) for _, dtype, shape in outputs], (True,) * len(outputs),
                                 after=(ws.data_ptr(), nb))
    assert rc == 0 and intact, _lib.lib().pnn_last_error(ip._context(0))
    return {name: out for (name, _, _), out in zip(outputs, outs)}


def check(got, want, label):
    for name, g in got.items():
        v = want[name]
        assert g.dtype == v.dtype and g.shape == v.shape, (label, name, g.dtype, g.shape, v.dtype, v.shape)
        assert g.tobytes() == v.tobytes(), "%s %s: %d differing values" % (label, name, (g != v).sum())


def raw_cases():
    """Every (width, rung, smoothing) -- the instantiations -- under the asymmetric mask; the other masks -- the geometry, which
    stage_blocks<W, G, PIC> shares among the instantiations of a width -- once per width, on the switch rung at its largest smoothing."""
    out = []
    for w in cases.WIDTHS:
        out += [(w, rung, cases.asymmetric(w), smoothing) for rung in cases.RUNGS for smoothing in cases.SMOOTHINGS[w]]
        out += [(w, 'switch', mask, cases.SMOOTHINGS[w][-1]) for mask in cases.masks(w) if mask != cases.asymmetric(w)]
    return out


@pytest.mark.parametrize("w, rung, mask, smoothing", raw_cases(),
                         ids=["w%d-%s-mask%dx%d-smoothing%d" % (w, r, m[0], m[1], s) for w, r, m, s in raw_cases()])
def test_pair_entries_against_host_twin(w, rung, mask, smoothing):
    """(a) One call of a picture-pair entry on 3 images and n = 2 G + 1 blocks: context plane = channel 1, target plane = channel 0.
    The case reaches rd_candidates_kernel<W = w, PIC = true, SMOOTH = (smoothing != 0), SLOTS = (rung != 'plain'), SUBST = (rung ==
    'substitution')> -- smoothing 1 and 2 are one instantiation and differ at w = 32 alone, in the strong filter's flag; w = 64 with
    slots takes the quadrant-major output loop -- behind hevc_mode_hads_kernel<W, true, SMOOTH>, which stages the same way."""
    context, target = cases.planes(w)
    rows, cols = cases.positions(w)
    left, above = cases.neighbours(w, rung)
    got = picture_call(w, rung, mask, smoothing, context, target, rows, cols, cases.blocks(w, mask)[2], left, above)
    check(got, cases.yardstick(w, rung, mask, smoothing), "w %d %s mask %s smoothing %d" % (w, rung, mask, smoothing))


@pytest.mark.parametrize("w", (4, 64))
def test_single_pictures_are_pairs_with_equal_planes(w):
    """(b) The signalling rung with both plane pointers equal against the yardstick built from that one plane"""
    context, _ = cases.planes(w, single=True)
    rows, cols = cases.positions(w)
    mask = cases.asymmetric(w)
    left, above = cases.neighbours(w, 'switch')
    got = picture_call(w, 'switch', mask, 0, context, None, rows, cols, cases.blocks(w, mask, True)[2], left, above)
    check(got, cases.yardstick(w, 'switch', mask, 0, True), "single w %d" % w)


@pytest.mark.parametrize("w", (4, 16))
def test_batch_equals_its_images_one_at_a_time(w):
    """(c) The 3-image call against three 1-image calls on the same positions, their outputs concatenated over the blocks: the image
    term of picture_corner apart from everything else"""
    context, target = cases.planes(w)
    rows, cols = cases.positions(w)
    mask, smoothing = cases.asymmetric(w), cases.SMOOTHINGS[w][-1]
    candidates = cases.blocks(w, mask)[2]
    left, above = cases.neighbours(w, 'switch')
    batch = picture_call(w, 'switch', mask, smoothing, context, target, rows, cols, candidates, left, above)
    per = rows.size
    singles = [picture_call(w, 'switch', mask, smoothing, context[i:i + 1], target[i:i + 1], rows, cols, candidates[i * per:(i + 1) * per],
                            left[i * per:(i + 1) * per], above[i * per:(i + 1) * per]) for i in range(cases.IMAGES)]
    check({name: np.concatenate([s[name] for s in singles], axis=1) for name in batch}, batch, "batch w %d" % w)


RD_KEYS = ('rd_pass_candidates', 'rd_pass_costs', 'rd_pass_modes', 'rd_pass_sses', 'rd_pass_rate_bits', 'psnrs_recon_rd_pass',
           'frequency_rd_pass_win_pnn', 'rd_pass_side_rate_bits')


def rd_keys_of_host_twin(host, pnn_mode):
    n = host['modes'].shape[1]
    return {'rd_pass_candidates': host['candidates'], 'rd_pass_costs': host['costs'], 'rd_pass_modes': host['modes'],
            'rd_pass_sses': host['sses'], 'rd_pass_rate_bits': host['rate_bits'], 'psnrs_recon_rd_pass': host['psnrs_recon'],
            'frequency_rd_pass_win_pnn': [float(np.count_nonzero(m == pnn_mode)) / n for m in host['modes']],
            'rd_pass_side_rate_bits': host['side_rate_bits']}


@pytest.mark.parametrize("is_fc, w", [(True, 4), (False, 32), (False, 64)], ids=["fc4", "conv32", "conv64"])
def test_evaluator_rd_pass_at_the_other_widths(is_fc, w):
    """(d) score_masks_from_pictures / _picture_pairs with the whole second pass on, both codecs: the rd_pass_* keys, psnrs_recon_rd_pass
    and frequency_rd_pass_win_pnn equal the host twin on the dictionary's own targets and PNN predictions and the host-extracted
    patterns; keep_predictions=False gives the same bytes for every key both calls have."""
    from context_adaptive_neural_network_based_prediction_amd import evaluation
    pair = np.array(cases.pictures(w))                    # (a copy: the shared pictures are read-only)
    single = np.ascontiguousarray(pair[..., 0:1])
    rows, cols = cases.positions(w)
    n = cases.blocks_per_call(w)
    masks = ((0, 0), (4, w))
    net = util.make_net(w, is_fc, n)
    try:
        for name, channels, score in (("pictures", single, evaluation.score_masks_from_pictures),
                                      ("pairs", pair, evaluation.score_masks_from_picture_pairs)):
            context = channels[..., -1:]
            for codec in ('switch', 'substitution'):
                neighbours = cases.neighbours(w, codec)
                options = dict(first_pass=True, reference_smoothing=2, transform_qps=cases.QPS, transform_rate=True, transform_sign_hiding=True,
                               transform_rdoq=True, rd_pass=True, rd_pass_signalling=True, rd_pass_neighbour_modes=neighbours, rd_pass_codec=codec)
                got = score(channels, w, rows, cols, net, util.MEAN, masks, keep_predictions=True, **options)
                lean = score(channels, w, rows, cols, net, util.MEAN, masks, keep_predictions=False, **options)
                for mask in masks:
                    label = "%s w %d %s mask %s" % (name, w, codec, mask)
                    patterns = ip.extract_intra_patterns(context, w, rows + w - 1, cols + w - 1, mask)[..., 0]
                    host = cases.host_twin(w, codec, patterns, got[mask]['targets_uint8'][..., 0], got[mask]['predictions_pnn_uint8'][..., 0], 2,
                                           neighbours)
                    assert_same_dictionary({k: got[mask][k] for k in RD_KEYS}, rd_keys_of_host_twin(host, cases.CANDIDATE_MODE[codec]), label)
                    assert set(lean[mask]) < set(got[mask]) and set(RD_KEYS) <= set(lean[mask]), label
                    assert_same_dictionary(lean[mask], {k: got[mask][k] for k in lean[mask]}, label + " lean")
    finally:
        net.close()
