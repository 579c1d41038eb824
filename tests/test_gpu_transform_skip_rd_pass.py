"""GPU tests of transform skip in the second intra pass (include/pnn_hip.h, "transform skip"): pnn_rd_pass_tskip_device
/ _picture_pairs_device (per QP the unchanged transform-coding launch, tskip4_kernel, the slots' mode bits, tskip_decide_kernel in place, the
unchanged decision, the winners' flags) against the host twin pnn_rd_pass_tskip_host, which tests/test_transform_skip_rd_pass.py pins to a
composition: both codecs, dense at n = 1 and 2 * 64 + 1 and from picture pairs, equality of bytes, the raw picture-pairs call between guard
bytes; the option off; every refusal before a launch."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import util
from tests.test_transform_skip_rd_pass import seeded
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, picture_pairs, positions, untouched

pytestmark = pytest.mark.gpu

OUTPUTS = tuple(ip.RD_PASS_SIGNAL_OUTPUTS) + (('best_transform_skip', np.uint8),)


def specs_of(n, nq, codec):
    return [(dtype, shape) for (_, dtype), shape in zip(OUTPUTS, tuple(ip.rd_pass_signal_shapes(n, nq, 4, codec)) + ((nq, n),))]


@pytest.mark.parametrize("codec", ('switch', 'substitution'))
def test_dense_entry_against_host_twin(codec):
    patterns, targets, candidates, left, above = seeded(codec)
    for n in (1, 129):
        for sdh, rdoq, lambdas in ((0, 0, None), (1, 1, None), (1, 1, [3.5, 40.])):
            kwargs = dict(reference_smoothing=2, sign_data_hiding=bool(sdh), rdoq=bool(rdoq), signalling=True, lambdas=lambdas,
                          neighbour_modes=(left[:n], above[:n]), codec=codec, transform_skip=True)
            got = ip.rd_pass(patterns[:n], targets[:n], candidates[:n], (22, 37), device=0, **kwargs)
            want = ip.rd_pass(patterns[:n], targets[:n], candidates[:n], (22, 37), **kwargs)
            assert_same_dictionary(got, want, "%s n %d sdh %d rdoq %d" % (codec, n, sdh, rdoq))
            if n == 129:
                assert 0 < want['best_transform_skip'].sum() < want['best_transform_skip'].size
    kwargs = dict(reference_smoothing=2, signalling=True, neighbour_modes=(left, above), codec=codec)     # the option off: today's bytes
    assert_same_dictionary(ip.rd_pass(patterns, targets, candidates, (22, 37), device=0, transform_skip=False, **kwargs),
                           ip.rd_pass(patterns, targets, candidates, (22, 37), **kwargs), "option off")


def pair_call(codec, option, short=0, width=4, lambdas=None, qps=(22, 37), signalling=1, wanted=None, images=2, per_image=None):
    """Raw call of pnn_rd_pass_tskip_picture_pairs_device between guard bytes: (rc, outputs, intact, host dictionary or None).  n =
    images x per_image blocks: the first per_image positions of the picture's grid (util's three positions when None)"""
    import torch
    w = width
    pair = picture_pairs(images, w, 2900 + w)
    rows, cols = positions()
    if per_image is not None:                             # every position a (3w + 5) x (3w + 9) picture has, row-major
        grid = [(r, c) for r in range(6) for c in range(10)][:per_image]
        rows, cols = positions(grid)
    n, nq = images * rows.size, len(qps)
    mask = (4, w)
    context, target = np.ascontiguousarray(pair[..., 1]), np.ascontiguousarray(pair[..., 0])
    patterns = ip.extract_intra_patterns(pair[..., 1:2], w, rows + w - 1, cols + w - 1, mask)[..., 0]
    targets = np.array([target[i, r + w:r + 2 * w, c + w:c + 2 * w] for i in range(images) for r, c in zip(rows, cols)])
    rng = np.random.default_rng(11)
    candidates = np.clip(targets.astype(np.int64) - np.where(rng.integers(0, 2, targets.shape) == 1, 25, 0), 0, 255).astype(np.uint8)
    left = rng.integers(0, 35, n).astype(np.uint8)
    above = np.where(rng.integers(0, 3, n) == 0, 255, rng.integers(0, 35, n)).astype(np.uint8)
    number = ip.CODECS[codec]
    d = [dev(a) for a in (context, target, rows.astype(np.int32), cols.astype(np.int32), candidates, left, above)]
    L = _lib.lib()
    nb = L.pnn_rd_pass_tskip_workspace_bytes(4, n, len(qps), 1, number, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    c_lambdas = None if lambdas is None else (ctypes.c_double * nq)(*lambdas)
    front = (ip._context(0), w, d[0].data_ptr(), d[1].data_ptr(), images, pair.shape[1], pair.shape[2], d[2].data_ptr(), d[3].data_ptr(), rows.size,
             mask[0], mask[1], d[4].data_ptr(), 2, (ctypes.c_int * nq)(*qps), nq, c_lambdas, 1, 1, signalling, d[5].data_ptr(), d[6].data_ptr(),
             number, option)
    specs = specs_of(n, nq, codec) if w == 4 else [(np.uint8, (4,))] * len(OUTPUTS)
    wanted = (True,) * len(OUTPUTS) if wanted is None else wanted
    rc, outs, intact = util.call("pnn_rd_pass_tskip_picture_pairs_device", front, (), specs, wanted, after=(ws.data_ptr(), nb - short))
    host = None
    if rc == 0:
        host = ip.rd_pass(patterns, targets, candidates, qps, reference_smoothing=2, sign_data_hiding=True, rdoq=True, signalling=True,
                          neighbour_modes=(left, above), codec=codec, transform_skip=bool(option))
    return rc, outs, intact, host


@pytest.mark.parametrize("codec", ('switch', 'substitution'))
def test_picture_pairs_entry_against_host_twin(codec):
    for images, per_image in ((2, None), (1, 1), (3, 43)):                # n = 6, 1 and 2 * 64 + 1
        rc, outs, intact, host = pair_call(codec, 1, images=images, per_image=per_image)
        assert rc == 0 and intact, _lib.lib().pnn_last_error(ip._context(0))
        assert host['modes'].shape[1] == (6, 1, 129)[(2, 1, 3).index(images)]
        for (name, _), got in zip(OUTPUTS, outs):
            assert got.tobytes() == host[name].tobytes(), (name, images)
        assert images == 1 or host['best_transform_skip'].any()
    rc, outs, intact, host = pair_call(codec, 0)                          # the option off: the pass of today, the flags zeroed
    assert rc == 0 and intact
    for (name, _), got in zip(OUTPUTS[:-1], outs):
        assert got.tobytes() == host[name].tobytes(), name
    assert not outs[-1].any()


def test_every_refusal_comes_before_a_launch():
    L, ctx = _lib.lib(), ip._context(0)
    rc, outs, intact, _ = pair_call('switch', 1)
    assert rc == 0 and intact
    good = ctypes.c_int(-1)
    assert L.pnn_last_call_stats(ctx, None, None, ctypes.byref(good)) == 0 and good.value == 2 + 2 * 7
    for kwargs in (dict(option=2), dict(option=-1), dict(option=1, width=8), dict(option=1, short=1), dict(option=1, lambdas=[1., 0.]),
                   dict(option=1, signalling=0), dict(option=0, signalling=0), dict(option=1, qps=(22, 52)),
                   dict(option=1, wanted=(False,) * len(OUTPUTS))):
        option = kwargs.pop('option')
        rc, outs, intact, _ = pair_call('switch', option, **kwargs)
        launches = ctypes.c_int(-1)
        assert L.pnn_last_call_stats(ctx, None, None, ctypes.byref(launches)) == 0
        assert rc == PNN_E_ARG and intact and untouched(outs) and launches.value == good.value, (option, kwargs)
