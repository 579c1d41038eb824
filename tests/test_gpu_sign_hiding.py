"""GPU tests of HM's sign-data hiding in the transform-coding column (trquant_kernel<W, RATE, SDH = true> behind
pnn_trquant_sdh_device, intraprediction.transform_code(device=0, sign_data_hiding=True), evaluation.score_masks_from_pictures /
_picture_pairs(transform_sign_hiding=True)).  The yardstick is the host twin pnn_trquant_sdh_host, which tests/test_sign_hiding.py pins
to a Python restatement and to recorded calls of HM's own signBitHidingHDQ; every comparison is integer equality, every output lies
between guard bytes.

No case may pass because nothing was hidden: in every parametrised case the host twin's stages must show a changed level in at least a
quarter of the (unit, QP) pairs, and over the file every row of the cost table must have been met among the candidates of a group that
changed, every allowed row as a winner's (test_every_row_of_the_cost_table_was_taken, which runs last)."""
import ctypes
import itertools

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cabac_rate_cases as cabac
from tests import sign_hiding_cases as cases
from tests import util
from tests.trquant_cases import MODES, blocks_per_workgroup, specs_of
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, make_net, picture_pairs, positions, ptr, untouched

pytestmark = pytest.mark.gpu

# low QPs: dense levels, whose groups have the wrong parity about half the time
QP_LISTS = {1: (12,), 4: (0, 10, 22, 27), 8: (0, 4, 8, 12, 17, 22, 27, 32)}
OUTPUTS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'reconstructions_uint8', 'rate')
TAKEN = {}                                                # rows of the cost table the host twin took, over the whole file


def host_call(w, predictions, targets, qps, modes, flag=1, wanted=(True,) * 5):
    """pnn_trquant_sdh_host, raw: the five outputs (None where not wanted)"""
    n, nq = predictions.shape[0], len(qps)
    outs = [np.zeros(s, t) if want else None for (t, s), want in zip(specs_of(w, n, nq), wanted)]
    rc = _lib.lib().pnn_trquant_sdh_host(predictions.ctypes.data, targets.ctypes.data, w, n, None if modes is None else modes.ctypes.data,
                                         (ctypes.c_int * nq)(*qps), nq, *[None if o is None else o.ctypes.data for o in outs], flag)
    assert rc == 0
    return outs


def device_call(w, predictions, targets, qps, modes, flag=1, wanted=(True,) * 5, entry="sdh"):
    """Raw ABI call of pnn_trquant_sdh_device (entry "rate": of pnn_trquant_rate_device, which has no flag); every output between guard
    bytes.  Returns (rc, the outputs as numpy or None, guards intact)."""
    n, nq = predictions.shape[0], len(qps)
    d_p, d_t = dev(predictions), dev(targets)
    d_m = None if modes is None else dev(modes)
    front = (ip._context(0), w, d_p.data_ptr(), d_t.data_ptr(), n, ptr(d_m), (ctypes.c_int * max(nq, 1))(*qps), nq)
    if entry == "rate":
        return util.call("pnn_trquant_rate_device", front, (), specs_of(w, n, nq), wanted)
    return util.call("pnn_trquant_sdh_device", front, (), specs_of(w, n, nq), wanted, after=(flag,))


def blocks_of(w, n):
    """n dense (prediction, target) pairs, a zero residual among them; at w = 64 the last block has another constant residual per
    quadrant"""
    predictions, targets = cases.dense_pairs(w, n, 2300 + w)
    targets[1] = predictions[1]
    if w == 64:
        predictions[n - 1] = 100
        for (qy, qx), d in zip(itertools.product(range(2), range(2)), (3, -7, 20, -40)):
            targets[n - 1, 32 * qy:32 * qy + 32, 32 * qx:32 * qx + 32] = 100 + d
    return predictions, targets


def share_of_changed_units(w, predictions, targets, qps, modes):
    """From the host twin's stages: the share of (unit, QP) pairs in which hiding changed a level; the rows taken go to TAKEN."""
    t = min(w, 32)
    changed = total = 0
    for b in range(predictions.shape[0]):
        scan = cabac.scan_of_mode(t, None if modes is None else int(modes[b]))
        for qp in qps:
            s = ip.transform_stages(predictions[b], targets[b], qp, sign_data_hiding=True, scan=scan)
            for unit in cases.units_of(w):
                total += 1
                if not np.array_equal(s['levels'][unit], s['levels_hidden'][unit]):
                    changed += 1
                    assert cases.book_keeping(s['levels'][unit], s['levels_hidden'][unit], s['coeffs'][unit], s['delta_u'][unit], scan, TAKEN)
    return changed / total


@pytest.mark.parametrize("nb_qps", (1, 4, 8))
@pytest.mark.parametrize("w", (4, 8, 16, 32, 64))
def test_kernel_against_host_twin(w, nb_qps):
    """n = 2 G + 1 blocks: two full workgroups and a ragged one; without modes and with a mode array that takes every scan; the rate on
    and off."""
    n = 2 * blocks_per_workgroup(w) + 1
    qps = QP_LISTS[nb_qps]
    predictions, targets = blocks_of(w, n)
    mode_array = np.array([MODES[(b + nb_qps) % len(MODES)] for b in range(n)], np.uint8)
    no_rate = (True,) * 4 + (False,)
    for modes in (None, mode_array):
        assert share_of_changed_units(w, predictions, targets, qps, modes) >= 0.25, "too little was hidden for the case to show anything"
        host = host_call(w, predictions, targets, qps, modes)
        for wanted in ((True,) * 5, no_rate):
            rc, outs, intact = device_call(w, predictions, targets, qps, modes, wanted=wanted)
            assert rc == 0 and intact
            for name, got, want, full in zip(OUTPUTS, outs, wanted, host):
                assert (got is None) == (not want)
                assert got is None or np.array_equal(got, full), "w %d, %d QPs, modes %s, rate %s, %s: %d differing values" % (
                    w, nb_qps, modes is not None, wanted[4], name, (got != full).sum())
        zero = (predictions == targets).all(axis=(1, 2))
        assert zero.any() and host[4].any() and not host[4][:, zero].any() and not host[0][:, zero].any()
        unhidden = host_call(w, predictions, targets, qps, modes, flag=0)
        assert not np.array_equal(unhidden[3], host[3]) and (host[4] < unhidden[4]).any()    # hiding shows in the samples and in the bits
        assert np.array_equal(unhidden[2], host[2])                                          # sum_abs_levels is HM's uiAbsSum: before hiding
    if w == 8:            # (the last `host` is the one with modes) the scan shapes the levels; at w = 4 only through ties: every level is set
        assert not np.array_equal(host[3], host_call(w, predictions, targets, qps, None)[3])
    if w == 64:                                           # each quadrant of the last block is a unit of its own: one level each, nothing to hide
        assert (host[1][:, n - 1] == 4).all()
    if nb_qps == 4:
        # each output alone: nothing else is written, nothing changes
        for k in range(5):
            wanted = tuple(i == k for i in range(5))
            rc, part, intact = device_call(w, predictions, targets, qps, mode_array, wanted=wanted)
            assert rc == 0 and intact, wanted
            for name, got, want, full in zip(OUTPUTS, part, wanted, host):
                assert (got is None) == (not want) and (got is None or np.array_equal(got, full)), (w, wanted, name)
        # the flag 0: pnn_trquant_rate_device's outputs
        rc, off, intact = device_call(w, predictions, targets, qps, mode_array, flag=0)
        rc2, rated, intact2 = device_call(w, predictions, targets, qps, mode_array, entry="rate")
        assert rc == 0 and rc2 == 0 and intact and intact2
        for name, got, want, full in zip(OUTPUTS, off, rated, unhidden):
            assert np.array_equal(got, want) and np.array_equal(got, full), (w, name)
        for rate in (False, True):
            got = ip.transform_code(predictions, targets, qps, device=0, keep_reconstructions=True, modes=mode_array, rate=rate,
                                    sign_data_hiding=True)
            want = ip.transform_code(predictions, targets, qps, keep_reconstructions=True, modes=mode_array, rate=rate, sign_data_hiding=True)
            assert ('rate_bits' in got) == rate
            assert_same_dictionary(got, want, "transform_code w %d" % w)
        assert np.array_equal(got['rate_bits'], host[4].astype(np.float64) / 32768.)


def test_device_argument_errors():
    """Every refusal comes before the launch; with the flag a mode array needs no rate output, without it it still does."""
    w = 8
    predictions, targets = cases.dense_pairs(w, 3, 12)
    modes = np.array([0, 10, 26], np.uint8)
    no_rate = (True,) * 4 + (False,)
    for wanted, mode_array, flag, word in ((no_rate, modes, 0, b"modes"), ((False,) * 5, None, 1, b"NULL")):
        rc, outs, intact = device_call(w, predictions, targets, (22,), mode_array, flag=flag, wanted=wanted)
        assert rc == PNN_E_ARG and intact
        assert untouched(outs)
        assert word in _lib.lib().pnn_last_error(ip._context(0))
    rc, outs, intact = device_call(w, predictions, targets, (22,), modes, wanted=no_rate)
    assert rc == 0 and intact
    assert _lib.lib().pnn_trquant_sdh_device(None, w, None, None, 2, None, (ctypes.c_int * 1)(22), 1, None, None, None, None, None, 1,
                                             None) == PNN_E_ARG
    with pytest.raises(ValueError):
        ip.transform_code(predictions, targets, (22,), device=0, modes=np.array([0, 35, 1]), sign_data_hiding=True)


COLUMN_KEYS = ('sses_recon', 'nb_nonzero_levels', 'sum_abs_levels', 'psnrs_recon')


@pytest.mark.parametrize("pairs", (False, True), ids=("pictures", "pairs"))
@pytest.mark.parametrize("is_fc, w", [(True, 8), (False, 16)], ids=["fc8", "conv16"])
def test_evaluator_transform_sign_hiding(is_fc, w, pairs):
    """transform_sign_hiding=True, with and without transform_rate: the transform keys equal transform_code's host twin with the flag on
    the dictionary's own predictions, targets and modes; every other key has the bytes of the call without the option."""
    pair = picture_pairs(2, w, 1400 + w)
    channels = pair if pairs else np.ascontiguousarray(pair[..., 0:1])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, w))
    qps = (4, 17)
    net = make_net(w, is_fc, n)
    try:
        for rate in (False, True):
            plain = score(channels, w, rows, cols, net, util.MEAN, masks, transform_qps=qps, transform_rate=rate)
            hidden = score(channels, w, rows, cols, net, util.MEAN, masks, transform_qps=qps, transform_rate=rate, transform_sign_hiding=True)
            again = score(channels, w, rows, cols, net, util.MEAN, masks, transform_qps=qps, transform_rate=rate, transform_sign_hiding=False)
            transform_keys = {'%s_%s' % (name, column) for name in COLUMN_KEYS + (('rate_bits',) if rate else ())
                              for column in ('pnn', 'hevc_best_mode')} | {'frequency_recon_win_pnn'} | ({'frequency_rate_win_pnn'} if rate else set())
            for mask in masks:
                label = "w %d mask %s rate %s" % (w, mask, rate)
                assert_same_dictionary(again[mask], plain[mask], label)
                got = hidden[mask]
                assert set(got) == set(plain[mask]) | {'transform_sign_hiding'} and got['transform_sign_hiding'] is True, label
                assert_same_dictionary({k: v for k, v in got.items() if k not in transform_keys and k != 'transform_sign_hiding'},
                                       {k: v for k, v in plain[mask].items() if k not in transform_keys}, label)
                want = {}
                for column, modes in (('pnn', None), ('hevc_best_mode', got['indices_hevc_best_mode'])):
                    blocks = (got['predictions_%s_uint8' % column], got['targets_uint8'])
                    assert share_of_changed_units(w, blocks[0][..., 0], blocks[1][..., 0], qps, modes) >= 0.25, label
                    host = ip.transform_code(*blocks, qps, modes=modes, rate=rate, sign_data_hiding=True)
                    for name in COLUMN_KEYS + (('rate_bits',) if rate else ()):
                        want['%s_%s' % (name, column)] = host[name]
                    assert not np.array_equal(host['sses_recon'], plain[mask]['sses_recon_' + column]), label
                want['frequency_recon_win_pnn'] = [
                    float(np.count_nonzero(want['psnrs_recon_pnn'][q] - want['psnrs_recon_hevc_best_mode'][q] > 0.)) / n for q in range(2)]
                if rate:
                    want['frequency_rate_win_pnn'] = [
                        float(np.count_nonzero(want['rate_bits_pnn'][q] < want['rate_bits_hevc_best_mode'][q])) / n for q in range(2)]
                assert_same_dictionary({k: got[k] for k in transform_keys}, want, label)
        with pytest.raises(ValueError, match="transform_sign_hiding"):
            score(channels, w, rows, cols, net, util.MEAN, masks, transform_sign_hiding=True)
    finally:
        net.close()


def test_every_row_of_the_cost_table_was_taken():
    """Over the cases above (this test is the file's last): every row of the table among the candidates of groups that changed, every
    allowed row as the winner's."""
    if not TAKEN:                                         # run on its own: the host twin's part of the kernel cases, again
        for w, nb_qps in itertools.product((4, 8, 16, 32, 64), (1, 4, 8)):
            predictions, targets = blocks_of(w, 2 * blocks_per_workgroup(w) + 1)
            share_of_changed_units(w, predictions, targets, QP_LISTS[nb_qps], None)
    for row in cases.ROWS:
        assert TAKEN.get(row, 0) > 0, row
        if not row.endswith('forbidden'):
            assert TAKEN.get('won:' + row, 0) > 0, row
