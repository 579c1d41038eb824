"""GPU tests of the CABAC rate of the coded levels (trquant_kernel<W, RATE = true> behind pnn_trquant_rate_device,
intraprediction.transform_code(device=0, rate=True), evaluation.score_masks_from_pictures / _picture_pairs(transform_rate=True)).  The
yardstick is the host twin pnn_trquant_rate_host, which tests/test_cabac_rate.py pins to a Python restatement and to HM's recorded
numbers; every comparison is integer equality, every output lies between guard bytes."""
import ctypes
import itertools

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import trquant_cases as cases
from tests import util
from tests.trquant_cases import MODES, blocks_per_workgroup, specs_of
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, make_net, picture_pairs, positions, ptr, untouched

pytestmark = pytest.mark.gpu

QP_LISTS = {1: (27,), 4: (0, 22, 37, 51), 8: (0, 5, 17, 22, 30, 37, 46, 51)}
OUTPUTS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'reconstructions_uint8', 'rate')


def host_call(w, predictions, targets, qps, modes):
    """pnn_trquant_rate_host, raw: the five outputs"""
    n, nq = predictions.shape[0], len(qps)
    outs = [np.zeros(s, t) for t, s in specs_of(w, n, nq)]
    rc = _lib.lib().pnn_trquant_rate_host(predictions.ctypes.data, targets.ctypes.data, w, n, None if modes is None else modes.ctypes.data,
                                          (ctypes.c_int * nq)(*qps), nq, *[o.ctypes.data for o in outs])
    assert rc == 0
    return outs


def device_call(w, predictions, targets, qps, modes, wanted=(True,) * 5, plain=False):
    """Raw ABI call of pnn_trquant_rate_device (plain: of pnn_trquant_device, which has neither modes nor rate: its four outputs, None
    for the rate); every output between guard bytes.  Returns (rc, the outputs as numpy or None, guards intact)."""
    n, nq = predictions.shape[0], len(qps)
    specs = specs_of(w, n, nq)
    d_p, d_t = dev(predictions), dev(targets)
    d_m = None if modes is None else dev(modes)
    blocks = (ip._context(0), w, d_p.data_ptr(), d_t.data_ptr(), n)
    c_qps = (ctypes.c_int * max(nq, 1))(*qps)
    if plain:
        rc, outs, intact = util.call("pnn_trquant_device", blocks + (c_qps, nq), (), specs[:4], wanted[:4])
        return rc, outs + [None], intact
    return util.call("pnn_trquant_rate_device", blocks + (ptr(d_m), c_qps, nq), (), specs, wanted)


def blocks_of(w, n, nb_qps):
    """n (prediction, target) pairs: the extremes -- the largest levels the path can make (about 13107 at QP 0; the clip at 32767 is out
    of its reach and is covered on the CPU through cabac_rate_of_levels) -- and a zero residual among random and smooth ones; at w = 64
    also a block with another constant residual per quadrant"""
    predictions, targets = cases.mixed_pairs(w, max(n, 4), 1700 + w)
    predictions, targets = predictions[:n].copy(), targets[:n].copy()
    if n < 4:                                             # one block per workgroup: the QP lists share out the special blocks
        ep, et = cases.extreme_pairs(w)
        for slot, k in enumerate({1: (0, 3), 4: (2, 3), 8: (1, 3)}[nb_qps]):
            predictions[slot], targets[slot] = ep[k], et[k]
    if w == 64:
        predictions[n - 1] = 100
        for (qy, qx), d in zip(itertools.product(range(2), range(2)), (3, -7, 20, -40)):
            targets[n - 1, 32 * qy:32 * qy + 32, 32 * qx:32 * qx + 32] = 100 + d
    return predictions, targets


@pytest.mark.parametrize("nb_qps", (1, 4, 8))
@pytest.mark.parametrize("w", cases.WIDTHS)
def test_kernel_against_host_twin(w, nb_qps):
    """n = 2 G + 1 blocks: two full workgroups and a ragged one; without modes and with a mode array that takes every scan."""
    n = 2 * blocks_per_workgroup(w) + 1
    qps = QP_LISTS[nb_qps]
    predictions, targets = blocks_of(w, n, nb_qps)
    mode_array = np.array([MODES[(b + nb_qps) % len(MODES)] for b in range(n)], np.uint8)
    for modes in (None, mode_array):
        host = host_call(w, predictions, targets, qps, modes)
        rc, outs, intact = device_call(w, predictions, targets, qps, modes)
        assert rc == 0 and intact
        for name, got, want in zip(OUTPUTS, outs, host):
            assert np.array_equal(got, want), "w %d, %d QPs, modes %s, %s: %d differing values" % (
                w, nb_qps, modes is not None, name, (got != want).sum())
        assert host[4].any() and (host[4][:, (predictions == targets).all(axis=(1, 2))] == 0).all()      # a zero residual costs 0
    if w <= 8:                                            # (the last `host` is the one with modes) the scan matters at these sizes
        assert not np.array_equal(host[4], host_call(w, predictions, targets, qps, None)[4])
    if nb_qps == 4:
        # the rate alone, and each other output left out in turn: nothing else is written, nothing changes
        for wanted in [tuple(i == 4 for i in range(5))] + [tuple(i != k for i in range(5)) for k in range(4)]:
            rc, part, intact = device_call(w, predictions, targets, qps, mode_array, wanted=wanted)
            assert rc == 0 and intact, wanted
            for name, got, want, full in zip(OUTPUTS, part, wanted, host):
                assert (got is None) == (not want) and (got is None or np.array_equal(got, full)), (w, wanted, name)
        # pnn_trquant_device, the call without the rate: the other outputs bit for bit
        rc, plain, intact = device_call(w, predictions, targets, qps, None, wanted=(True,) * 4 + (False,), plain=True)
        assert rc == 0 and intact
        for name, got, full in zip(OUTPUTS[:4], plain, host):
            assert np.array_equal(got, full), (w, name)
        got = ip.transform_code(predictions, targets, qps, device=0, keep_reconstructions=True, modes=mode_array, rate=True)
        want = ip.transform_code(predictions, targets, qps, keep_reconstructions=True, modes=mode_array, rate=True)
        assert_same_dictionary(got, want, "transform_code w %d" % w)
        assert np.array_equal(got['rate_bits'], host[4].astype(np.float64) / 32768.)


def test_device_argument_errors():
    """Every refusal comes before the launch: modes without a rate output, every output NULL; the guards stay untouched."""
    w = 8
    predictions, targets = cases.random_pairs(w, 3, 12)
    modes = np.array([0, 10, 26], np.uint8)
    for wanted, mode_array, word in (((True,) * 4 + (False,), modes, b"modes"), ((False,) * 5, None, b"NULL")):
        rc, outs, intact = device_call(w, predictions, targets, (22,), mode_array, wanted=wanted)
        assert rc == PNN_E_ARG and intact
        assert untouched(outs)
        assert word in _lib.lib().pnn_last_error(ip._context(0))
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (22,), device=0, modes=modes)
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (22,), device=0, modes=np.array([0, 35, 1]), rate=True)


RATE_KEYS = {'rate_bits_pnn', 'rate_bits_hevc_best_mode', 'frequency_rate_win_pnn'}


@pytest.mark.parametrize("pairs", (False, True), ids=("pictures", "pairs"))
@pytest.mark.parametrize("is_fc, w", [(True, 8), (False, 16)], ids=["fc8", "conv16"])
def test_evaluator_transform_rate(is_fc, w, pairs):
    """transform_rate=True: the new keys equal transform_code's host twin with the rate on the dictionary's own predictions, targets and
    modes; every old key has the bytes of the call without the option."""
    pair = picture_pairs(2, w, 1400 + w)
    channels = pair if pairs else np.ascontiguousarray(pair[..., 0:1])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, w))
    qps = (22, 37)
    net = make_net(w, is_fc, n)
    try:
        for smoothing in (0, 2):
            plain = score(channels, w, rows, cols, net, util.MEAN, masks, reference_smoothing=smoothing, transform_qps=qps)
            rated = score(channels, w, rows, cols, net, util.MEAN, masks, reference_smoothing=smoothing, transform_qps=qps, transform_rate=True)
            for mask in masks:
                label = "w %d mask %s smoothing %d" % (w, mask, smoothing)
                assert set(rated[mask]) == set(plain[mask]) | RATE_KEYS, label
                assert_same_dictionary({k: v for k, v in rated[mask].items() if k not in RATE_KEYS}, plain[mask], label)
                got = rated[mask]
                want = {}
                for column, modes in (('pnn', None), ('hevc_best_mode', got['indices_hevc_best_mode'])):
                    host = ip.transform_code(got['predictions_%s_uint8' % column], got['targets_uint8'], qps, modes=modes, rate=True)
                    assert host['rate_bits'].shape == (2, n) and host['rate_bits'].any()
                    want['rate_bits_' + column] = host['rate_bits']
                want['frequency_rate_win_pnn'] = [
                    float(np.count_nonzero(got['rate_bits_pnn'][q] < got['rate_bits_hevc_best_mode'][q])) / n for q in range(2)]
                assert_same_dictionary({k: got[k] for k in RATE_KEYS}, want, label)
        with pytest.raises(ValueError):
            score(channels, w, rows, cols, net, util.MEAN, masks, transform_rate=True)
    finally:
        net.close()
