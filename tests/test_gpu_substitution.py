"""GPU tests of the substitution codec's intra search as a column and of the mode statistics (substitution_list_kernel, the K + 2 slots
form of rd_candidates_kernel, the unchanged trquant_kernel launch per QP, the decision without the flag bin and mode_stats_kernel behind
pnn_rd_pass_codec_device / _picture_pairs_device and pnn_rd_pass_mode_stats_device; intraprediction.rd_pass(device=0,
codec='substitution'), the evaluator's rd_pass_codec and rd_pass_mode_stats).  The yardstick is the host twin pnn_rd_pass_codec_host,
which tests/test_substitution.py pins to a Python restatement; every comparison is equality of bytes (doubles by bit pattern), every
output lies between guard bytes.  The seeded blocks and neighbours are those on which test_substitution.py asserts the conditions."""
import ctypes
import itertools

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import mode_signal_cases as signal
from tests import rd_pass_cases
from tests import substitution_cases as cases
from tests import util
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, picture_pairs, positions, untouched

pytestmark = pytest.mark.gpu

NAMES = tuple(name for name, _ in ip.RD_PASS_SIGNAL_OUTPUTS)
ALL = (True,) * len(NAMES)
SUB = dict(signalling=True, codec='substitution')


def specs_of(w, n, nq, codec=1, signalling=1):
    if not signalling:
        return [(dtype, shape) for (_, dtype), shape in zip(ip.RD_PASS_OUTPUTS, ip.rd_pass_shapes(n, nq, w))] + [(np.float64, (1,)), (np.uint64, (1,))]
    shapes = ip.rd_pass_signal_shapes(n, nq, w, 'substitution' if codec == 1 else 'switch')
    return [(dtype, shape) for (_, dtype), shape in zip(ip.RD_PASS_SIGNAL_OUTPUTS, shapes)]


def device_call(w, patterns, targets, candidates, qps, left=None, above=None, smoothing=0, flag=0, rdoq=0, lambdas=None, wanted=ALL, short=0,
                signalling=1, codec=1, no_candidate=False, entry="pnn_rd_pass_codec_device"):
    """Raw ABI call of pnn_rd_pass_codec_device (or, without `codec`, of pnn_rd_pass_signal_device), every output between guard bytes, the
    workspace `short` bytes below what the entry asks for.  Returns (rc, the outputs as numpy or None, guards intact)."""
    import torch
    n, nq = targets.shape[0], len(qps)
    d_in = [dev(a) for a in (patterns, targets, candidates)]
    d_left, d_above = (None if a is None else dev(np.asarray(a, np.uint8)) for a in (left, above))
    L = _lib.lib()
    if codec is None:
        nb = L.pnn_rd_pass_signal_workspace_bytes(w, n, nq, signalling)
    elif codec == 0:
        nb = L.pnn_rd_pass_codec_workspace_bytes(w, n, nq, signalling, 0)
    else:                                                 # (a refused codec or signalling 0: the scratch of the accepted combination)
        nb = L.pnn_rd_pass_codec_workspace_bytes(w, n, nq, 1, 1)
    d_ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
    c_lambdas = None if lambdas is None else (ctypes.c_double * nq)(*lambdas)
    front = (ip._context(0), w, d_in[0].data_ptr(), patterns.shape[1], patterns.shape[2], d_in[1].data_ptr(), n,
             None if no_candidate else d_in[2].data_ptr(), smoothing, (ctypes.c_int * nq)(*qps), nq, c_lambdas, flag, rdoq, signalling,
             util.ptr(d_left), util.ptr(d_above)) + (() if codec is None else (codec,))
    specs = specs_of(w, n, nq, 0 if codec is None else codec if codec in (0, 1) else 1, signalling)
    return util.call(entry if codec is not None else "pnn_rd_pass_signal_device", front, (), specs, wanted, after=(d_ws.data_ptr(), nb - short))


def host_outputs(patterns, targets, candidates, qps, left=None, above=None, smoothing=0, flag=0, rdoq=0, lambdas=None):
    neighbour_modes = None if left is None and above is None else (left, above)
    result = ip.rd_pass(patterns, targets, candidates, qps, smoothing, bool(flag), lambdas, rdoq=bool(rdoq), neighbour_modes=neighbour_modes, **SUB)
    return result, [result[name] for name in NAMES]


def check(outs, host, wanted, label):
    for name, got, want, full in zip(NAMES, outs, wanted, host):
        assert (got is None) == (not want), (label, name)
        assert got is None or (got.dtype == full.dtype and got.tobytes() == full.tobytes()), "%s %s: %d differing values" % (
            label, name, (got != full).sum())


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_kernels_against_host_twin(w):
    """n = 2 G + 1 blocks and n = 1; QPs 22 / 37, smoothing 0 and 2, RDOQ off and (at w = 8 and 64) on, given neighbours and NULL, HM's
    lambdas and the caller's; each output alone and all together."""
    n = 2 * cases.BLOCKS_PER_WORKGROUP[w] + 1
    patterns, targets, candidates = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    own = (3.5, 180.25)
    qps = cases.QP_PAIRS[0]
    configs = [(0, 0, 0, None, True), (2, 1, 0, own, True), (2, 0, 0, own, False)]
    if w in (8, 64):
        configs.append((2, 1, 1, None, True))
    for smoothing, flag, rdoq, lambdas, given in configs:
        label = "w %d, smoothing %d, sdh %d, rdoq %d, lambdas %s, neighbours %s" % (w, smoothing, flag, rdoq, lambdas is not None, given)
        l, a = (left, above) if given else (None, None)
        result, host = host_outputs(patterns, targets, candidates, qps, l, a, smoothing, flag, rdoq, lambdas)
        rc, outs, intact = device_call(w, patterns, targets, candidates, qps, l, a, smoothing, flag, rdoq, lambdas)
        assert rc == 0 and intact, label
        check(outs, host, ALL, label)
        assert not (outs[0] == 35).any() and not (outs[2] == 35).any(), label
    _, host = host_outputs(patterns, targets, candidates, (37,), None, above)             # one neighbour array alone
    rc, outs, intact = device_call(w, patterns, targets, candidates, (37,), None, above)
    assert rc == 0 and intact
    check(outs, host, ALL, "w %d above alone" % w)
    rc, outs, intact = device_call(w, patterns[:1], targets[:1], candidates[:1], qps, left[:1], above[:1], 0, 1, 0, own)
    assert rc == 0 and intact
    check(outs, host_outputs(patterns[:1], targets[:1], candidates[:1], qps, left[:1], above[:1], 0, 1, 0, own)[1], ALL, "w %d n 1" % w)
    _, host = host_outputs(patterns, targets, candidates, qps, left, above, 2, 1, 0, own)
    for k in range(len(NAMES)):                           # each output alone: nothing else is written, nothing changes
        wanted = tuple(i == k for i in range(len(NAMES)))
        rc, part, intact = device_call(w, patterns, targets, candidates, qps, left, above, 2, 1, 0, own, wanted=wanted)
        assert rc == 0 and intact, wanted
        check(part, host, wanted, "w %d alone %s" % (w, NAMES[k]))
    assert_same_dictionary(ip.rd_pass(patterns, targets, candidates, (22, 37), 2, True, device=0, neighbour_modes=(left, above), **SUB),
                           ip.rd_pass(patterns, targets, candidates, (22, 37), 2, True, neighbour_modes=(left, above), **SUB), "rd_pass w %d" % w)


def test_quadrants_of_a_64_block():
    """w = 64: a block whose target differs from a constant candidate by another constant per quadrant, one quadrant not at all: every
    quadrant is a unit of its own with its own cbf bin; 18 is coded as an appended most probable mode."""
    w, n = 64, 2
    patterns, targets, candidates = rd_pass_cases.seeded(w, n)
    candidates[1] = 100
    for (qy, qx), d in zip(itertools.product(range(2), range(2)), (3, 0, 20, -40)):
        targets[1, 32 * qy:32 * qy + 32, 32 * qx:32 * qx + 32] = 100 + d
    left, above = np.array([18, 18], np.uint8), np.array([255, 10], np.uint8)
    for rdoq in (0, 1):
        result, host = host_outputs(patterns, targets, candidates, cases.QP_PAIRS[0], left, above, 0, 1, rdoq)
        rc, outs, intact = device_call(w, patterns, targets, candidates, cases.QP_PAIRS[0], left, above, 0, 1, rdoq)
        assert rc == 0 and intact
        check(outs, host, ALL, "quadrants rdoq %d" % rdoq)
    slot = int(np.argmax(result['candidates'][0, 1] == cases.PNN_MODE))
    assert result['candidates'][0, 1, slot] == cases.PNN_MODE and np.isfinite(result['costs'][0, 1, slot])


def test_picture_pairs_form():
    """pnn_rd_pass_codec_picture_pairs_device equals the host twin on the dense patterns and targets of the same blocks."""
    import torch
    w, qps = 8, (22, 37)
    pair = picture_pairs(2, w, 2900 + w)
    rows, cols = positions()
    n = 2 * rows.size
    mask = (4, w)
    context, target = np.ascontiguousarray(pair[..., 1]), np.ascontiguousarray(pair[..., 0])
    patterns = ip.extract_intra_patterns(pair[..., 1:2], w, rows + w - 1, cols + w - 1, mask)[..., 0]
    targets = np.array([target[i, r + w:r + 2 * w, c + w:c + 2 * w] for i in range(2) for r, c in zip(rows, cols)])
    candidates = np.clip(targets.astype(np.int64) + np.random.default_rng(11).integers(-9, 10, targets.shape), 0, 255).astype(np.uint8)
    left, above = cases.neighbours(w, n)
    result, host = host_outputs(patterns, targets, candidates, qps, left, above, 2, 1)
    d = [dev(a) for a in (context, target, rows.astype(np.int32), cols.astype(np.int32), candidates, left, above)]
    nb = _lib.lib().pnn_rd_pass_codec_workspace_bytes(w, n, len(qps), 1, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    front = (ip._context(0), w, d[0].data_ptr(), d[1].data_ptr(), 2, pair.shape[1], pair.shape[2], d[2].data_ptr(), d[3].data_ptr(), rows.size,
             mask[0], mask[1], d[4].data_ptr(), 2, (ctypes.c_int * 2)(*qps), 2, None, 1, 0, 1, d[5].data_ptr(), d[6].data_ptr(), 1)
    rc, outs, intact = util.call("pnn_rd_pass_codec_picture_pairs_device", front, (), specs_of(w, n, 2), ALL, after=(ws.data_ptr(), nb))
    assert rc == 0 and intact, _lib.lib().pnn_last_error(ip._context(0))
    check(outs, host, ALL, "picture pairs")


def test_codec_0_is_the_signal_entry():
    w, n, qps = 8, 33, (22, 37)
    patterns, targets, candidates = rd_pass_cases.seeded(w, n)
    left, above = signal.neighbours(w, n)
    for signalling, wanted in ((1, ALL), (0, (True,) * 7 + (False,) * 2)):
        l, a = (left, above) if signalling else (None, None)
        rc, old, intact = device_call(w, patterns, targets, candidates, qps, l, a, 2, 1, signalling=signalling, codec=None, wanted=wanted)
        assert rc == 0 and intact
        rc, new, intact = device_call(w, patterns, targets, candidates, qps, l, a, 2, 1, signalling=signalling, codec=0, wanted=wanted)
        assert rc == 0 and intact
        for x, y in zip(old, new):
            assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes())
    L = _lib.lib()
    assert L.pnn_rd_pass_codec_workspace_bytes(w, n, 2, 1, 0) == L.pnn_rd_pass_signal_workspace_bytes(w, n, 2, 1)


def stats_device(candidates, modes):
    """Raw ABI call of pnn_rd_pass_mode_stats_device, the output between guard bytes"""
    nq, n = modes.shape
    d_c, d_m = dev(candidates), dev(modes)
    front = (ip._context(0), d_c.data_ptr() if n else None, int(candidates.ndim == 3), candidates.shape[-1], d_m.data_ptr() if n else None, n, nq)
    return util.call("pnn_rd_pass_mode_stats_device", front, (), [(np.uint32, (nq, 3, 36))], (True,))


@pytest.mark.parametrize("n", (1, 257))
def test_mode_stats_against_host_twin(n):
    """Both layouts, 3 QPs; n = 257 is two workgroups and a ragged tail.  The slots and winners are drawn, not computed: every mode 0 .. 35
    and 255 occurs."""
    rng = np.random.default_rng(40 + n)
    L = _lib.lib()
    for shape in ((n, 4), (3, n, 11), (3, n, 10)):
        candidates = rng.integers(0, 36, shape).astype(np.uint8)
        candidates[rng.random(shape) < 0.2] = 255
        modes = rng.integers(0, 36, (3, n)).astype(np.uint8)
        modes[rng.random((3, n)) < 0.1] = 255
        want = np.zeros((3, 3, 36), np.uint32)
        assert L.pnn_rd_pass_mode_stats_host(candidates.ctypes.data, int(len(shape) == 3), shape[-1], modes.ctypes.data, n, 3, want.ctypes.data) == 0
        assert np.array_equal(want, cases.stats_of(candidates, modes))
        rc, outs, intact = stats_device(candidates, modes)
        assert rc == 0 and intact, shape
        assert outs[0].tobytes() == want.tobytes(), shape
        got = ip.rd_pass_mode_stats(candidates, modes, device=0)
        assert_same_dictionary(got, ip.rd_pass_mode_stats(candidates, modes), "stats %s" % (shape,))


@pytest.mark.parametrize("is_fc, w", [(True, 8), (False, 16)], ids=["fc8", "conv16"])
def test_evaluator_substitution_and_stats(is_fc, w):
    """rd_pass_codec='substitution' on pictures and on pairs: the rd_pass_* keys equal the dense Python entry's host twin on the
    dictionary's own patterns, targets and PNN predictions, every other key has the bytes of the call without the option; the stats
    keys equal rd_pass_mode_stats on the dictionary's own slots and winners, for both codecs; the defaults change no key and no byte."""
    from context_adaptive_neural_network_based_prediction_amd import evaluation
    pair = picture_pairs(2, w, 2950 + w)
    single = np.ascontiguousarray(pair[..., 0:1])
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, w))
    qps = (22, 37)
    left, above = cases.neighbours(w, n, 78)
    keys = ('rd_pass_candidates', 'rd_pass_costs', 'rd_pass_modes', 'rd_pass_sses', 'rd_pass_rate_bits', 'psnrs_recon_rd_pass',
            'frequency_rd_pass_win_pnn', 'rd_pass_side_rate_bits')
    stats_keys = {'rd_pass_mode_fast_selections': 'fast_selections', 'rd_pass_mode_fast_wins': 'fast_wins', 'rd_pass_mode_rd_wins': 'rd_wins',
                  'rd_pass_modes_for_rd': 'modes_for_rd', 'rd_pass_runs': 'runs'}
    net = util.make_net(w, is_fc, n)
    try:
        for name, channels, score in (("pictures", single, evaluation.score_masks_from_pictures),
                                      ("pairs", pair, evaluation.score_masks_from_picture_pairs)):
            options = dict(first_pass=True, reference_smoothing=2, transform_qps=qps, transform_rate=True, transform_sign_hiding=True, rd_pass=True)
            plain = score(channels, w, rows, cols, net, util.MEAN, masks, **options)
            off = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass_codec='switch', rd_pass_mode_stats=False, **options)
            switch = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass_signalling=True, rd_pass_neighbour_modes=(left, above), **options)
            got = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass_signalling=True, rd_pass_neighbour_modes=(left, above),
                        rd_pass_codec='substitution', rd_pass_mode_stats=True, **options)
            counted = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass_mode_stats=True, **options)
            context = channels[..., -1:]
            for mask in masks:
                label = "%s w %d mask %s" % (name, w, mask)
                assert_same_dictionary(off[mask], plain[mask], label)
                assert set(got[mask]) == set(switch[mask]) | set(stats_keys), label
                assert_same_dictionary({k: v for k, v in got[mask].items() if k not in keys and k not in stats_keys},
                                       {k: v for k, v in plain[mask].items() if k not in keys}, label)
                patterns = ip.extract_intra_patterns(context, w, rows + w - 1, cols + w - 1, mask)[..., 0]
                host = ip.rd_pass(patterns, got[mask]['targets_uint8'][..., 0], got[mask]['predictions_pnn_uint8'][..., 0], qps,
                                  reference_smoothing=2, sign_data_hiding=True, neighbour_modes=(left, above), **SUB)
                want = {'rd_pass_candidates': host['candidates'], 'rd_pass_costs': host['costs'], 'rd_pass_modes': host['modes'],
                        'rd_pass_sses': host['sses'], 'rd_pass_rate_bits': host['rate_bits'], 'psnrs_recon_rd_pass': host['psnrs_recon'],
                        'frequency_rd_pass_win_pnn': [float(np.count_nonzero(m == cases.PNN_MODE)) / n for m in host['modes']],
                        'rd_pass_side_rate_bits': host['side_rate_bits']}
                assert_same_dictionary({k: got[mask][k] for k in keys}, want, label)
                assert host['candidates'].shape[2] == ip.first_pass_list_size(w) + 2
                for result in (got[mask], counted[mask]):
                    stats = ip.rd_pass_mode_stats(result['rd_pass_candidates'], result['rd_pass_modes'])
                    assert_same_dictionary({k: result[k] for k in stats_keys}, {k: stats[v] for k, v in stats_keys.items()}, label)
                assert_same_dictionary({k: v for k, v in counted[mask].items() if k not in stats_keys}, plain[mask], label)
                assert counted[mask]['rd_pass_runs'] == n and (counted[mask]['rd_pass_mode_rd_wins'].sum(axis=1) == n).all()
                assert not got[mask]['rd_pass_mode_fast_selections'][:, 35].any()
    finally:
        net.close()


def test_device_argument_errors():
    """Every refusal comes before any launch: no output is written; a bad codec, a neighbour 35, signalling 0, a missing candidate and a
    workspace one byte short among them."""
    w = 8
    patterns, targets, candidates = rd_pass_cases.seeded(w, 3)
    L = _lib.lib()
    for kwargs, word in ((dict(short=1), b"workspace"), (dict(wanted=(False,) * len(NAMES)), b"NULL"), (dict(smoothing=3), b"smoothing"),
                         (dict(lambdas=(-1.,)), b"lambda"), (dict(lambdas=(0.,), rdoq=1), b"lambda"), (dict(qps=(52,)), b"QP"),
                         (dict(left=(0, 35, 0)), b"neighbour"), (dict(above=(254, 0, 0)), b"neighbour"), (dict(codec=2), b"codec"),
                         (dict(codec=-1), b"codec"), (dict(signalling=0, wanted=(True,) * 7 + (False,) * 2), b"signalling"),
                         (dict(no_candidate=True), b"cand_pred")):
        call = dict(qps=(22,))
        call.update(kwargs)
        rc, outs, intact = device_call(w, patterns, targets, candidates, **call)
        assert rc == PNN_E_ARG and intact, kwargs
        assert untouched(outs), kwargs
        assert word in L.pnn_last_error(ip._context(0)), (kwargs, L.pnn_last_error(ip._context(0)))
    rc, outs, intact = device_call(64, *rd_pass_cases.seeded(64, 1), (22,), short=1)
    assert rc == PNN_E_ARG and intact and untouched(outs)
    rc, outs, intact = device_call(w, patterns, targets, candidates, (22,))
    assert rc == 0 and intact
    slots, modes = np.zeros((3, 4), np.uint8), np.zeros((1, 3), np.uint8)
    d_s, d_m = dev(slots), dev(modes)
    for front in ((None, 0, 4, d_m.data_ptr(), 3, 1), (d_s.data_ptr(), 0, 0, d_m.data_ptr(), 3, 1), (d_s.data_ptr(), 0, 17, d_m.data_ptr(), 3, 1),
                  (d_s.data_ptr(), 0, 4, None, 3, 1), (d_s.data_ptr(), 0, 4, d_m.data_ptr(), -1, 1), (d_s.data_ptr(), 0, 4, d_m.data_ptr(), 3, 9)):
        rc, outs, intact = util.call("pnn_rd_pass_mode_stats_device", (ip._context(0),) + front, (), [(np.uint32, (1, 3, 36))], (True,))
        assert rc == PNN_E_ARG and intact and untouched(outs), front
    rc, outs, intact = util.call("pnn_rd_pass_mode_stats_device", (ip._context(0), d_s.data_ptr(), 0, 4, d_m.data_ptr(), 3, 1), (), [(np.uint32, (1, 3, 36))],
                                 (False,))
    assert rc == PNN_E_ARG and intact
