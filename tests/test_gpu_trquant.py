"""GPU tests of the open-loop transform coding (trquant_kernel behind pnn_trquant_device, intraprediction.transform_code(device=0),
evaluation.score_masks_from_pictures / _picture_pairs(transform_qps=...)).  The yardstick is the host twin, which tests/test_trquant.py
pins to numpy and to HM's own transforms; every comparison is integer equality, every output lies between guard bytes."""
import ctypes
import itertools

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import trquant_cases as cases
from tests import util
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, make_net, picture_pairs, positions, stream, untouched

pytestmark = pytest.mark.gpu

QP_LISTS = {1: (27,), 4: (22, 27, 32, 37), 8: (0, 5, 17, 22, 30, 37, 46, 51)}
OUTPUTS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'reconstructions_uint8')


def device_call(w, predictions, targets, qps, wanted=(True,) * 4, n=None, ctx=None):
    """Raw ABI call; every output between guard bytes.  Returns (rc, the four outputs as numpy or None, guards intact)."""
    n = predictions.shape[0] if n is None else n
    nq = len(qps)
    d_p, d_t = dev(predictions), dev(targets)
    front = (ip._context(0) if ctx is None else ctx, w, d_p.data_ptr(), d_t.data_ptr(), n, (ctypes.c_int * max(nq, 1))(*qps), nq)
    return util.call("pnn_trquant_device", front, (), cases.specs_of(w, max(n, 0), nq)[:4], wanted)


@pytest.mark.parametrize("nb_qps", (1, 4, 8))
@pytest.mark.parametrize("w", cases.WIDTHS)
def test_kernel_against_host_twin(w, nb_qps):
    """n = 2 G + 1 blocks: two full workgroups and a ragged one; the extremes and a zero residual share the first with random blocks."""
    n = 2 * cases.blocks_per_workgroup(w) + 1
    qps = QP_LISTS[nb_qps]
    predictions, targets = cases.mixed_pairs(w, max(n, 4), 700 + w)
    predictions, targets = predictions[:n], targets[:n]
    if n < 4:                                           # one block per workgroup (w = 32, 64): the three QP lists share out the special blocks
        ep, et = cases.extreme_pairs(w)                 # + 255, - 255, the checkerboard, a zero residual
        for slot, k in enumerate({1: (0, 1, 2), 4: (2, 3), 8: (1, 3)}[nb_qps]):
            predictions[slot], targets[slot] = ep[k], et[k]
    host = ip.transform_code(predictions, targets, qps, keep_reconstructions=True)
    rc, outs, intact = device_call(w, predictions, targets, qps)
    assert rc == 0 and intact
    for name, got in zip(OUTPUTS, outs):
        assert np.array_equal(got, host[name]), "w %d, %d QPs, %s: %d differing values" % (w, nb_qps, name, (got != host[name]).sum())
    if nb_qps == 4:
        # each output left out in turn, and each asked for alone: the others do not change, nothing else is written
        for wanted in [tuple(i != k for i in range(4)) for k in range(4)] + [tuple(i == k for i in range(4)) for k in range(4)]:
            rc, part, intact = device_call(w, predictions, targets, qps, wanted=wanted)
            assert rc == 0 and intact, wanted
            for name, got, want in zip(OUTPUTS, part, wanted):
                assert (got is None) == (not want) and (got is None or np.array_equal(got, host[name])), (w, wanted, name)
        got = ip.transform_code(predictions, targets, qps, device=0, keep_reconstructions=True)
        assert_same_dictionary(got, host, "transform_code w %d" % w)


def test_width_64_quadrants():
    """Each quadrant of a 64 x 64 block carries another constant residual: per unit one level of |d| * 32 / 8 at QP 22 and an exact
    reconstruction (tests/test_trquant.py derives it), so a unit read, coded or stored in another quadrant's place shows."""
    ds = np.array([[3, -7], [20, -40]])
    predictions = np.full((3, 64, 64), 100, np.uint8)
    predictions[1] = 77
    targets = predictions.copy()
    for b in range(3):
        for qy, qx in itertools.product(range(2), range(2)):
            d = ds[qy, qx] if b < 2 else ds[1 - qy, 1 - qx]
            targets[b, 32 * qy:32 * qy + 32, 32 * qx:32 * qx + 32] = predictions[b, 0, 0] + d
    rc, (sse, nonzero, sum_abs, recon), intact = device_call(64, predictions, targets, (22, 51))
    assert rc == 0 and intact
    assert (nonzero[0] == 4).all() and (sum_abs[0] == 4 * np.abs(ds).sum()).all() and not sse[0].any()
    assert np.array_equal(recon[0], targets)
    host = ip.transform_code(predictions, targets, (22, 51), keep_reconstructions=True)
    for name, got in zip(OUTPUTS, (sse, nonzero, sum_abs, recon)):
        assert np.array_equal(got, host[name]), name


def test_device_argument_errors():
    """Every refusal comes before the launch: the guards and the outputs stay untouched, pnn_last_error names the argument."""
    L = _lib.lib()
    w = 8
    predictions, targets = cases.random_pairs(w, 3, 11)
    ctx = ip._context(0)
    for kwargs, word in ((dict(w=12), b"width"), (dict(n=-1), b"batch"), (dict(qps=()), b"QPs"), (dict(qps=(22,) * 9), b"QPs"),
                         (dict(qps=(52,)), b"QPs"), (dict(qps=(22, -1)), b"QPs"), (dict(wanted=(False,) * 4), b"NULL")):
        args = dict(w=w, qps=(22,), wanted=(True,) * 4, n=None)
        args.update(kwargs)
        rc, outs, intact = device_call(args['w'], predictions, targets, args['qps'], wanted=args['wanted'], n=args['n'])
        assert rc == PNN_E_ARG and intact, kwargs
        assert untouched(outs), kwargs
        assert word in L.pnn_last_error(ctx), (kwargs, L.pnn_last_error(ctx))
    out = dev(np.zeros(3, np.uint32))
    good = (ctypes.c_int * 1)(22)
    assert L.pnn_trquant_device(ctx, w, None, dev(targets).data_ptr(), 3, good, 1, out.data_ptr(), None, None, None, stream()) == PNN_E_ARG
    assert L.pnn_trquant_device(ctx, w, dev(predictions).data_ptr(), None, 3, good, 1, out.data_ptr(), None, None, None, stream()) == PNN_E_ARG
    assert L.pnn_trquant_device(ctx, w, dev(predictions).data_ptr(), dev(targets).data_ptr(), 3, None, 1, out.data_ptr(), None, None, None, stream()) == PNN_E_ARG
    assert L.pnn_trquant_device(ctx, w, None, None, 0, good, 1, out.data_ptr(), None, None, None, stream()) == 0       # n == 0 does nothing
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (52,), device=0)


TRANSFORM_KEYS = {'transform_qps', 'frequency_recon_win_pnn'} | {
    '%s_%s' % (name, column) for name in ('sses_recon', 'psnrs_recon', 'nb_nonzero_levels', 'sum_abs_levels') for column in ('pnn', 'hevc_best_mode')}


@pytest.mark.parametrize("pairs", (False, True), ids=("pictures", "pairs"))
@pytest.mark.parametrize("is_fc, w", [(True, 8), (False, 16)], ids=["fc8", "conv16"])
def test_evaluator_transform_qps(is_fc, w, pairs):
    """transform_qps=(22, 37): the new keys equal transform_code's host twin on the dictionary's own predictions and targets, every old
    key has the bytes of the call without the option, and () is that call."""
    pair = picture_pairs(2, w, 1300 + w)
    channels = pair if pairs else np.ascontiguousarray(pair[..., 0:1])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, w))
    qps = (22, 37)
    net = make_net(w, is_fc, n)
    try:
        for first_pass, smoothing in ((False, 0), (True, 2), (True, 0), (False, 2)):
            plain = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass, reference_smoothing=smoothing)
            empty = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass, reference_smoothing=smoothing, transform_qps=())
            coded = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass, reference_smoothing=smoothing, transform_qps=qps)
            lean = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass, reference_smoothing=smoothing, transform_qps=list(qps),
                         keep_predictions=False)
            lean_plain = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass, reference_smoothing=smoothing,
                               keep_predictions=False)
            for mask in masks:
                label = "w %d mask %s first_pass %s smoothing %d" % (w, mask, first_pass, smoothing)
                assert_same_dictionary(empty[mask], plain[mask], label)
                assert set(coded[mask]) == set(plain[mask]) | TRANSFORM_KEYS, label
                assert set(lean[mask]) == set(lean_plain[mask]) | TRANSFORM_KEYS, label
                assert_same_dictionary({k: v for k, v in coded[mask].items() if k not in TRANSFORM_KEYS}, plain[mask], label)
                assert_same_dictionary({k: v for k, v in lean[mask].items() if k not in TRANSFORM_KEYS}, lean_plain[mask], label)
                want = {'transform_qps': qps}
                for column in ('pnn', 'hevc_best_mode'):
                    host = ip.transform_code(coded[mask]['predictions_%s_uint8' % column], coded[mask]['targets_uint8'], qps)
                    assert host['sses_recon'].shape == (2, n)
                    want.update({'%s_%s' % (name, column): host[name] for name in host})
                want['frequency_recon_win_pnn'] = [
                    float(np.count_nonzero(want['psnrs_recon_pnn'][q] - want['psnrs_recon_hevc_best_mode'][q] > 0.)) / n for q in range(2)]
                for got in (coded[mask], lean[mask]):
                    assert_same_dictionary({k: got[k] for k in TRANSFORM_KEYS}, want, label)
        for bad in ((52,), (22,) * 9, (22.5,), 22):
            with pytest.raises(ValueError):
                score(channels, w, rows, cols, net, util.MEAN, masks, transform_qps=bad)
    finally:
        net.close()
