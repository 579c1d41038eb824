"""GPU tests of the second pass with mode signalling (signal_list_kernel, the slots form of rd_candidates_kernel, the unchanged
trquant_kernel launch per QP and rd_decide_signal_kernel behind pnn_rd_pass_signal_device / _picture_pairs_device,
intraprediction.rd_pass(device=0, signalling=True)).  The yardstick is the host twin pnn_rd_pass_signal_host, which
tests/test_mode_signal.py pins to a Python restatement; every comparison is equality of bytes (doubles by bit pattern), every output
lies between guard bytes.  The seeded blocks and neighbours are those on which test_mode_signal.py asserts the conditions."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import mode_signal_cases as cases
from tests import rd_pass_cases
from tests import util
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, picture_pairs, positions, untouched

pytestmark = pytest.mark.gpu

NAMES = tuple(name for name, _ in ip.RD_PASS_SIGNAL_OUTPUTS)
ALL = (True,) * len(NAMES)


def specs_of(w, n, nq, signalling=1):
    if not signalling:
        return [(dtype, shape) for (_, dtype), shape in zip(ip.RD_PASS_OUTPUTS, ip.rd_pass_shapes(n, nq, w))] + [(np.float64, (1,)), (np.uint64, (1,))]
    return [(dtype, shape) for (_, dtype), shape in zip(ip.RD_PASS_SIGNAL_OUTPUTS, ip.rd_pass_signal_shapes(n, nq, w))]


def device_call(w, patterns, targets, candidates, qps, left=None, above=None, smoothing=0, flag=0, rdoq=0, lambdas=None, wanted=ALL, short=0,
                signalling=1):
    """Raw ABI call of pnn_rd_pass_signal_device, every output between guard bytes, the workspace `short` bytes below what the entry asks
    for.  Returns (rc, the outputs as numpy or None, guards intact)."""
    import torch
    n, nq = targets.shape[0], len(qps)
    d_in = [dev(a) for a in (patterns, targets, candidates)]
    d_left, d_above = (None if a is None else dev(np.asarray(a, np.uint8)) for a in (left, above))
    nb = _lib.lib().pnn_rd_pass_signal_workspace_bytes(w, n, nq, signalling)
    d_ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
    c_lambdas = None if lambdas is None else (ctypes.c_double * nq)(*lambdas)
    front = (ip._context(0), w, d_in[0].data_ptr(), patterns.shape[1], patterns.shape[2], d_in[1].data_ptr(), n, d_in[2].data_ptr(), smoothing,
             (ctypes.c_int * nq)(*qps), nq, c_lambdas, flag, rdoq, signalling, util.ptr(d_left), util.ptr(d_above))
    return util.call("pnn_rd_pass_signal_device", front, (), specs_of(w, n, nq, signalling), wanted, after=(d_ws.data_ptr(), nb - short))


def host_outputs(patterns, targets, candidates, qps, left=None, above=None, smoothing=0, flag=0, rdoq=0, lambdas=None):
    neighbour_modes = None if left is None and above is None else (left, above)
    result = ip.rd_pass(patterns, targets, candidates, qps, smoothing, bool(flag), lambdas, rdoq=bool(rdoq), signalling=True,
                        neighbour_modes=neighbour_modes)
    return result, [result[name] for name in NAMES]


def check(outs, host, wanted, label):
    for name, got, want, full in zip(NAMES, outs, wanted, host):
        assert (got is None) == (not want), (label, name)
        assert got is None or (got.dtype == full.dtype and got.tobytes() == full.tobytes()), "%s %s: %d differing values" % (
            label, name, (got != full).sum())


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_kernels_against_host_twin(w):
    """n = 2 G + 1 blocks and n = 1; QPs 22 / 37 and 0 / 51, smoothing 0 and 2, RDOQ off and (to w = 16) on, given neighbours and NULL,
    HM's lambdas and the caller's; each output alone."""
    n = 2 * cases.BLOCKS_PER_WORKGROUP[w] + 1
    patterns, targets, candidates = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    own = (3.5, 180.25)
    configs = [(cases.QP_PAIRS[0], 0, 0, 0, None, True), (cases.QP_PAIRS[1], 2, 1, 0, own, True), (cases.QP_PAIRS[0], 2, 0, 0, own, False)]
    if w <= 16 or w == 64:                                 # (at 64 RDOQ runs the quadrants under cbf context 0: n = 3 blocks)
        configs.append((cases.QP_PAIRS[0], 2, 1, 1, None, True))
    for qps, smoothing, flag, rdoq, lambdas, given in configs:
        label = "w %d, QPs %s, smoothing %d, sdh %d, rdoq %d, lambdas %s, neighbours %s" % (w, qps, smoothing, flag, rdoq, lambdas is not None, given)
        l, a = (left, above) if given else (None, None)
        result, host = host_outputs(patterns, targets, candidates, qps, l, a, smoothing, flag, rdoq, lambdas)
        rc, outs, intact = device_call(w, patterns, targets, candidates, qps, l, a, smoothing, flag, rdoq, lambdas)
        assert rc == 0 and intact, label
        check(outs, host, ALL, label)
    # one neighbour array alone
    _, host = host_outputs(patterns, targets, candidates, (37,), None, above)
    rc, outs, intact = device_call(w, patterns, targets, candidates, (37,), None, above)
    assert rc == 0 and intact
    check(outs, host, ALL, "w %d above alone" % w)
    rc, outs, intact = device_call(w, patterns[:1], targets[:1], candidates[:1], cases.QP_PAIRS[1], left[:1], above[:1], 0, 1, 0, own)
    assert rc == 0 and intact
    check(outs, host_outputs(patterns[:1], targets[:1], candidates[:1], cases.QP_PAIRS[1], left[:1], above[:1], 0, 1, 0, own)[1], ALL, "w %d n 1" % w)
    _, host = host_outputs(patterns, targets, candidates, cases.QP_PAIRS[0], left, above, 2, 1, 0, own)
    for k in range(len(NAMES)):                           # each output alone: nothing else is written, nothing changes
        wanted = tuple(i == k for i in range(len(NAMES)))
        rc, part, intact = device_call(w, patterns, targets, candidates, cases.QP_PAIRS[0], left, above, 2, 1, 0, own, wanted=wanted)
        assert rc == 0 and intact, wanted
        check(part, host, wanted, "w %d alone %s" % (w, NAMES[k]))
    assert_same_dictionary(ip.rd_pass(patterns, targets, candidates, (22, 37), 2, True, device=0, signalling=True, neighbour_modes=(left, above)),
                           ip.rd_pass(patterns, targets, candidates, (22, 37), 2, True, signalling=True, neighbour_modes=(left, above)),
                           "rd_pass w %d" % w)


def test_side_bits_follow_the_restatement():
    """The kernels' side bits looked up in the Python restatement directly: the winner's side rate is its mode's bits plus the cbf bin."""
    w, n, qps = 8, 33, (22, 37)
    patterns, targets, candidates = rd_pass_cases.seeded(w, n)
    left, above = cases.neighbours(w, n)
    rc, outs, intact = device_call(w, patterns, targets, candidates, qps, left, above)
    assert rc == 0 and intact
    got = dict(zip(NAMES, outs))
    for qi, qp in enumerate(qps):
        cbf = cases.cbf_bits(qp)[1]
        for b in range(n):
            mpm, _ = cases.mpm_of(left[b], above[b])
            bits = cases.mode_bits(int(got['modes'][qi, b]), mpm, qp)
            assert int(got['side_rates'][qi, b]) - bits in cbf, (qp, b)
            assert (int(got['side_rates'][qi, b]) - bits == cbf[0]) == (got['rates'][qi, b] == 0)
    # ... and in HM's own records (tests/golden/hm_mode_signal.npz, the regular tree): a regular winner's side bits are the PNN flag's
    # bin for 0 (the switch codec's addition, the restatement's) plus what HM's encodeIntraDirModeLuma and codeQtCbf (depth 0) counted
    import os
    hm = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hm_mode_signal.npz"))
    triples = [tuple(int(x) for x in t) for t in hm['regular_triples']]
    looked_up = 0
    for qi, qp in enumerate(qps):
        q = list(hm['qps']).index(qp)
        flag0 = cases.bin_bits(cases.INIT_PNN_FLAG, qp)[0]
        for b in range(n):
            mode = int(got['modes'][qi, b])
            mpm, _ = cases.mpm_of(left[b], above[b])
            if mode == cases.PNN or tuple(mpm) not in triples:
                continue
            coded = int(got['rates'][qi, b] != 0)
            want = flag0 + int(hm['regular_bits'][triples.index(tuple(mpm)), q, mode]) + int(hm['regular_cbf'][q, 0, coded])
            assert int(got['side_rates'][qi, b]) == want, (qp, b)
            looked_up += 1
    assert looked_up > 0


def test_signalling_off_is_the_rdoq_entry():
    w, n, qps = 8, 33, (22, 37)
    patterns, targets, candidates = rd_pass_cases.seeded(w, n)
    for rdoq in (0, 1):
        plain = ip.rd_pass(patterns, targets, candidates, qps, 2, True, rdoq=bool(rdoq), device=0)
        rc, outs, intact = device_call(w, patterns, targets, candidates, qps, None, None, 2, 1, rdoq, signalling=0, wanted=(True,) * 7 + (False,) * 2)
        assert rc == 0 and intact
        for (name, _), got in zip(ip.RD_PASS_OUTPUTS, outs):
            assert got.tobytes() == plain[name].tobytes(), name


def test_picture_pairs_form():
    """pnn_rd_pass_signal_picture_pairs_device equals the host twin on the dense patterns and targets of the same blocks."""
    import torch
    w, qps = 8, (22, 37)
    pair = picture_pairs(2, w, 2700 + w)
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
    nb = _lib.lib().pnn_rd_pass_signal_workspace_bytes(w, n, len(qps), 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    front = (ip._context(0), w, d[0].data_ptr(), d[1].data_ptr(), 2, pair.shape[1], pair.shape[2], d[2].data_ptr(), d[3].data_ptr(), rows.size,
             mask[0], mask[1], d[4].data_ptr(), 2, (ctypes.c_int * 2)(*qps), 2, None, 1, 0, 1, d[5].data_ptr(), d[6].data_ptr())
    rc, outs, intact = util.call("pnn_rd_pass_signal_picture_pairs_device", front, (), specs_of(w, n, 2), ALL, after=(ws.data_ptr(), nb))
    assert rc == 0 and intact, _lib.lib().pnn_last_error(ip._context(0))
    check(outs, host, ALL, "picture pairs")


def test_device_argument_errors():
    """Every refusal comes before any launch: no output is written; a workspace one byte short, a bad neighbour and width 64 among them."""
    w = 8
    patterns, targets, candidates = rd_pass_cases.seeded(w, 3)
    L = _lib.lib()
    for kwargs, word in ((dict(short=1), b"workspace"), (dict(wanted=(False,) * len(NAMES)), b"NULL"), (dict(smoothing=3), b"smoothing"),
                         (dict(lambdas=(-1.,)), b"lambda"), (dict(lambdas=(0.,), rdoq=1), b"lambda"), (dict(qps=(52,)), b"QP"),
                         (dict(left=(0, 36, 0)), b"neighbour"), (dict(above=(254, 0, 0)), b"neighbour")):
        call = dict(qps=(22,))
        call.update(kwargs)
        rc, outs, intact = device_call(w, patterns, targets, candidates, **call)
        assert rc == PNN_E_ARG and intact, kwargs
        assert untouched(outs), kwargs
        assert word in L.pnn_last_error(ip._context(0)), (kwargs, L.pnn_last_error(ip._context(0)))
    rc, outs, intact = device_call(64, *rd_pass_cases.seeded(64, 1), (22,), short=1)
    assert rc == PNN_E_ARG and intact and untouched(outs)
    assert L.pnn_rd_pass_signal_workspace_bytes(64, 1, 1, 0) == L.pnn_rd_pass_workspace_bytes(64, 1, 1)
    rc, outs, intact = device_call(w, patterns, targets, candidates, (22,), signalling=0, wanted=(True,) * 9)
    assert rc == PNN_E_ARG and intact and untouched(outs)                 # the added outputs without signalling
    rc, outs, intact = device_call(w, patterns, targets, candidates, (22,))
    assert rc == 0 and intact


def test_quadrants_of_a_64_block():
    """w = 64: a block whose target differs from a constant candidate by another constant per quadrant, one quadrant not at all: every
    quadrant is a unit of its own with its own cbf bin."""
    import itertools
    w, n = 64, 2
    patterns, targets, candidates = rd_pass_cases.seeded(w, n)
    candidates[1] = 100
    for (qy, qx), d in zip(itertools.product(range(2), range(2)), (3, 0, 20, -40)):
        targets[1, 32 * qy:32 * qy + 32, 32 * qx:32 * qx + 32] = 100 + d
    left, above = np.array([35, 10], np.uint8), np.array([255, 10], np.uint8)
    for rdoq in (0, 1):
        result, host = host_outputs(patterns, targets, candidates, cases.QP_PAIRS[0], left, above, 0, 1, rdoq)
        rc, outs, intact = device_call(w, patterns, targets, candidates, cases.QP_PAIRS[0], left, above, 0, 1, rdoq)
        assert rc == 0 and intact
        check(outs, host, ALL, "quadrants rdoq %d" % rdoq)
    slot = int(np.argmax(result['candidates'][0, 1] == cases.PNN))
    assert np.isfinite(result['costs'][0, 1, slot])


@pytest.mark.parametrize("is_fc, w", [(True, 8), (False, 16)], ids=["fc8", "conv16"])
def test_evaluator_rd_pass_signalling(is_fc, w):
    """rd_pass_signalling=True on pictures and on pairs: the rd_pass_* keys equal rd_pass(signalling=True)'s host twin on the dictionary's
    own patterns, targets and PNN predictions; every other key has the bytes of the call without the option; the default changes no key
    and no byte."""
    from context_adaptive_neural_network_based_prediction_amd import evaluation
    pair = picture_pairs(2, w, 2800 + w)
    single = np.ascontiguousarray(pair[..., 0:1])
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, w))
    qps = (22, 37)
    left, above = cases.neighbours(w, n, 77)
    keys = ('rd_pass_candidates', 'rd_pass_costs', 'rd_pass_modes', 'rd_pass_sses', 'rd_pass_rate_bits', 'psnrs_recon_rd_pass',
            'frequency_rd_pass_win_pnn', 'rd_pass_side_rate_bits')
    net = util.make_net(w, is_fc, n)
    try:
        for name, channels, score in (("pictures", single, evaluation.score_masks_from_pictures),
                                      ("pairs", pair, evaluation.score_masks_from_picture_pairs)):
            options = dict(first_pass=True, reference_smoothing=2, transform_qps=qps, transform_rate=True, transform_sign_hiding=True, rd_pass=True)
            plain = score(channels, w, rows, cols, net, util.MEAN, masks, **options)
            off = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass_signalling=False, rd_pass_neighbour_modes=None, **options)
            got = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass_signalling=True, rd_pass_neighbour_modes=(left, above), **options)
            context = channels[..., -1:]
            for mask in masks:
                label = "%s w %d mask %s" % (name, w, mask)
                assert_same_dictionary(off[mask], plain[mask], label)
                assert set(got[mask]) == set(plain[mask]) | {'rd_pass_side_rate_bits'}, label
                assert_same_dictionary({k: v for k, v in got[mask].items() if k not in keys},
                                       {k: v for k, v in plain[mask].items() if k not in keys}, label)
                patterns = ip.extract_intra_patterns(context, w, rows + w - 1, cols + w - 1, mask)[..., 0]
                host = ip.rd_pass(patterns, got[mask]['targets_uint8'][..., 0], got[mask]['predictions_pnn_uint8'][..., 0], qps,
                                  reference_smoothing=2, sign_data_hiding=True, signalling=True, neighbour_modes=(left, above))
                want = {'rd_pass_candidates': host['candidates'], 'rd_pass_costs': host['costs'], 'rd_pass_modes': host['modes'],
                        'rd_pass_sses': host['sses'], 'rd_pass_rate_bits': host['rate_bits'], 'psnrs_recon_rd_pass': host['psnrs_recon'],
                        'frequency_rd_pass_win_pnn': [float(np.count_nonzero(m == cases.PNN)) / n for m in host['modes']],
                        'rd_pass_side_rate_bits': host['side_rate_bits']}
                assert_same_dictionary({k: got[mask][k] for k in keys}, want, label)
    finally:
        net.close()
