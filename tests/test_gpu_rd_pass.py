"""GPU tests of HM's second intra pass as a column (rd_candidates_kernel, the unchanged trquant_kernel launch and rd_decide_kernel behind
pnn_rd_pass_device / pnn_rd_pass_picture_pairs_device, intraprediction.rd_pass(device=0), evaluation.score_masks_from_pictures /
_picture_pairs(rd_pass=True)).  The yardstick is the host twin pnn_rd_pass_host, which tests/test_rd_pass.py pins to a Python
restatement; every comparison is equality of bytes (doubles by bit pattern), every output lies between guard bytes.  The seeded blocks
are those on which test_rd_pass.py asserts that something is decided (rd_pass_cases.assert_conditions)."""
import ctypes
import itertools

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import rd_pass_cases as cases
from tests import util
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, make_net, picture_pairs, positions, untouched

pytestmark = pytest.mark.gpu

NAMES = tuple(name for name, _ in ip.RD_PASS_OUTPUTS)
ALL = (True,) * len(NAMES)


def specs_of(w, n, nq):
    return [(dtype, shape) for (_, dtype), shape in zip(ip.RD_PASS_OUTPUTS, ip.rd_pass_shapes(n, nq, w))]


def device_call(w, patterns, targets, candidates, qps, smoothing=0, flag=0, lambdas=None, wanted=ALL, short=0):
    """Raw ABI call of pnn_rd_pass_device, every output between guard bytes, the workspace `short` bytes below what the entry asks for.
    Returns (rc, the outputs as numpy or None, guards intact)."""
    import torch
    n, nq = targets.shape[0], len(qps)
    d_in = [dev(a) for a in (patterns, targets, candidates)]
    nb = _lib.lib().pnn_rd_pass_workspace_bytes(w, n, nq)
    d_ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    c_lambdas = None if lambdas is None else (ctypes.c_double * nq)(*lambdas)
    front = (ip._context(0), w, d_in[0].data_ptr(), patterns.shape[1], patterns.shape[2], d_in[1].data_ptr(), n, d_in[2].data_ptr(), smoothing,
             (ctypes.c_int * nq)(*qps), nq, c_lambdas, flag)
    return util.call("pnn_rd_pass_device", front, (), specs_of(w, n, nq), wanted, after=(d_ws.data_ptr(), nb - short))


def host_outputs(patterns, targets, candidates, qps, smoothing=0, flag=0, lambdas=None):
    result = ip.rd_pass(patterns, targets, candidates, qps, smoothing, bool(flag), lambdas)
    return result, [result[name] for name in NAMES]


def check(outs, host, wanted, label):
    for name, got, want, full in zip(NAMES, outs, wanted, host):
        assert (got is None) == (not want), (label, name)
        assert got is None or (got.dtype == full.dtype and got.tobytes() == full.tobytes()), "%s %s: %d differing values" % (
            label, name, (got != full).sum())


@pytest.mark.parametrize("nb_qps", (1, 4, 8))
@pytest.mark.parametrize("w", cases.WIDTHS)
def test_kernels_against_host_twin(w, nb_qps):
    """n = 2 G + 1 blocks (two full workgroups of rd_candidates_kernel and a ragged one) and n = 1; smoothing 0 and 2, sign hiding off and
    on, HM's lambdas and the caller's."""
    n = 2 * cases.BLOCKS_PER_WORKGROUP[w] + 1
    qps = cases.QP_LISTS[nb_qps]
    patterns, targets, candidates = cases.seeded(w, n)
    own = [0.5 + 3.25 * i for i in range(nb_qps)]
    for smoothing, flag, lambdas in ((0, 0, None), (2, 1, own), (2, 0, None), (0, 1, own)):
        label = "w %d, %d QPs, smoothing %d, sdh %d, lambdas %s" % (w, nb_qps, smoothing, flag, lambdas is not None)
        result, host = host_outputs(patterns, targets, candidates, qps, smoothing, flag, lambdas)
        if nb_qps == 4:
            cases.assert_conditions(result, label)
        rc, outs, intact = device_call(w, patterns, targets, candidates, qps, smoothing, flag, lambdas)
        assert rc == 0 and intact, label
        check(outs, host, ALL, label)
    # (the last case: smoothing 0, sign hiding, the caller's lambdas)
    rc, outs, intact = device_call(w, patterns[:1], targets[:1], candidates[:1], qps, 0, 1, own)
    assert rc == 0 and intact
    check(outs, host_outputs(patterns[:1], targets[:1], candidates[:1], qps, 0, 1, own)[1], ALL, "w %d n 1" % w)
    if nb_qps == 4:
        for k in range(len(NAMES)):                       # each output alone: nothing else is written, nothing changes
            wanted = tuple(i == k for i in range(len(NAMES)))
            rc, part, intact = device_call(w, patterns, targets, candidates, qps, 0, 1, own, wanted=wanted)
            assert rc == 0 and intact, wanted
            check(part, host, wanted, "w %d alone %s" % (w, NAMES[k]))
        assert_same_dictionary(ip.rd_pass(patterns, targets, candidates, qps, 2, True, device=0),
                               ip.rd_pass(patterns, targets, candidates, qps, 2, True), "rd_pass w %d" % w)


def test_quadrants_of_a_64_block():
    """w = 64: a block whose target differs from a constant prediction by another constant per quadrant, each quadrant a unit of its own."""
    w, n = 64, 2
    patterns, targets, candidates = cases.seeded(w, n)
    candidates[1] = 100
    for (qy, qx), d in zip(itertools.product(range(2), range(2)), (3, -7, 20, -40)):
        targets[1, 32 * qy:32 * qy + 32, 32 * qx:32 * qx + 32] = 100 + d
    qps = cases.QP_LISTS[4]
    result, host = host_outputs(patterns, targets, candidates, qps, 0, 1)
    rc, outs, intact = device_call(w, patterns, targets, candidates, qps, 0, 1)
    assert rc == 0 and intact
    check(outs, host, ALL, "quadrants")
    slot = int(np.argmax(result['candidates'][1] == cases.CANDIDATE))
    coded = ip.transform_code(candidates[1:], targets[1:], qps, rate=True, sign_data_hiding=True)
    assert (coded['nb_nonzero_levels'][0] == 4).all()     # at the lowest QP one level per quadrant: each is a unit of its own
    want = coded['sses_recon'][:, 0] + result['lambdas'] * np.floor(coded['rate_bits'][:, 0])
    assert np.array_equal(result['costs'][:, 1, slot], want)


def test_device_argument_errors():
    """Every refusal comes before any launch: no output is written; a workspace one byte short among them."""
    w = 8
    patterns, targets, candidates = cases.seeded(w, 3)
    L = _lib.lib()
    for kwargs, word in ((dict(short=1), b"workspace"), (dict(wanted=(False,) * len(NAMES)), b"NULL"), (dict(smoothing=3), b"smoothing"),
                         (dict(lambdas=(-1.,)), b"lambda"), (dict(lambdas=(float('nan'),)), b"lambda"), (dict(lambdas=(float('inf'),)), b"lambda"),
                         (dict(qps=(52,)), b"QP")):
        call = dict(qps=(22,))
        call.update(kwargs)
        rc, outs, intact = device_call(w, patterns, targets, candidates, **call)
        assert rc == PNN_E_ARG and intact, kwargs
        assert untouched(outs), kwargs
        assert word in L.pnn_last_error(ip._context(0)), (kwargs, L.pnn_last_error(ip._context(0)))
    rc, outs, intact = device_call(w, patterns, targets, candidates, (22,))
    assert rc == 0 and intact
    import torch
    d = [dev(a) for a in (patterns, targets, candidates)]
    nb = L.pnn_rd_pass_workspace_bytes(w, 3, 1)
    ws, out = torch.empty(nb + 8, dtype=torch.uint8, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda")
    qps = (ctypes.c_int * 1)(22)
    tail = (None, None, out.data_ptr(), None, None, None, None)
    for args in ((ip._context(0), w, d[0].data_ptr(), 17, 17, d[1].data_ptr(), 3, None, 0, qps, 1, None, 0, *tail, ws.data_ptr(), nb),
                 (ip._context(0), w, d[0].data_ptr(), 17, 17, d[1].data_ptr(), 3, d[2].data_ptr(), 0, qps, 1, None, 0, *tail, None, nb),
                 (ip._context(0), w, d[0].data_ptr(), 17, 17, d[1].data_ptr(), 3, d[2].data_ptr(), 0, qps, 1, None, 0, *tail, ws.data_ptr() + 4, nb),
                 (ip._context(0), w, d[0].data_ptr(), 8, 17, d[1].data_ptr(), 3, d[2].data_ptr(), 0, qps, 1, None, 0, *tail, ws.data_ptr(), nb),
                 (None, w, d[0].data_ptr(), 17, 17, d[1].data_ptr(), 3, d[2].data_ptr(), 0, qps, 1, None, 0, *tail, ws.data_ptr(), nb)):
        assert L.pnn_rd_pass_device(*args, util.stream()) == PNN_E_ARG
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


RD_KEYS = ('rd_pass_candidates', 'rd_pass_costs', 'rd_pass_modes', 'rd_pass_sses', 'rd_pass_rate_bits', 'psnrs_recon_rd_pass',
           'frequency_rd_pass_win_pnn')


@pytest.mark.parametrize("is_fc, w", [(True, 8), (False, 16)], ids=["fc8", "conv16"])
def test_evaluator_rd_pass(is_fc, w):
    """rd_pass=True on pictures and on pairs: the new keys equal rd_pass's host twin on the dictionary's own patterns, targets and PNN
    predictions; every old key has the bytes of the call without the option; the pair form with both planes equal gives the
    single-picture bits; the option without first_pass or transform_qps is refused."""
    pair = picture_pairs(2, w, 2600 + w)
    single = np.ascontiguousarray(pair[..., 0:1])
    twice = np.ascontiguousarray(np.concatenate([single, single], axis=3))
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, w))
    qps = (22, 37)
    net = make_net(w, is_fc, n)
    try:
        results = {}
        for name, channels, score in (("pictures", single, evaluation.score_masks_from_pictures),
                                      ("pairs", pair, evaluation.score_masks_from_picture_pairs),
                                      ("twice", twice, evaluation.score_masks_from_picture_pairs)):
            options = dict(first_pass=True, reference_smoothing=2, transform_qps=qps, transform_rate=True, transform_sign_hiding=True)
            plain = score(channels, w, rows, cols, net, util.MEAN, masks, **options)
            off = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass=False, **options)
            got = results[name] = score(channels, w, rows, cols, net, util.MEAN, masks, rd_pass=True, **options)
            context = channels[..., -1:]
            for mask in masks:
                label = "%s w %d mask %s" % (name, w, mask)
                assert_same_dictionary(off[mask], plain[mask], label)
                assert set(got[mask]) == set(plain[mask]) | set(RD_KEYS), label
                assert_same_dictionary({k: v for k, v in got[mask].items() if k not in RD_KEYS}, plain[mask], label)
                patterns = ip.extract_intra_patterns(context, w, rows + w - 1, cols + w - 1, mask)[..., 0]
                host = ip.rd_pass(patterns, got[mask]['targets_uint8'][..., 0], got[mask]['predictions_pnn_uint8'][..., 0], qps,
                                  reference_smoothing=2, sign_data_hiding=True)
                want = {'rd_pass_candidates': host['candidates'], 'rd_pass_costs': host['costs'], 'rd_pass_modes': host['modes'],
                        'rd_pass_sses': host['sses'], 'rd_pass_rate_bits': host['rate_bits'], 'psnrs_recon_rd_pass': host['psnrs_recon'],
                        'frequency_rd_pass_win_pnn': [float(np.count_nonzero(m == cases.CANDIDATE)) / n for m in host['modes']]}
                assert_same_dictionary({k: got[mask][k] for k in RD_KEYS}, want, label)
                assert np.array_equal(got[mask]['rd_pass_candidates'][:, :-1], got[mask]['first_pass_list']), label
        for mask in masks:
            assert_same_dictionary(results["twice"][mask], results["pictures"][mask], "both planes equal, mask %s" % (mask,))
        for options in (dict(transform_qps=qps), dict(first_pass=True)):
            with pytest.raises(ValueError, match="rd_pass"):
                evaluation.score_masks_from_pictures(single, w, rows, cols, net, util.MEAN, masks, rd_pass=True, **options)
    finally:
        net.close()
