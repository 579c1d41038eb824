"""GPU tests of transform skip in the transform-coding column (include/pnn_hip.h, "transform skip"): tskip4_kernel
and tskip_decide_kernel behind pnn_trquant_tskip_device and intraprediction.transform_code(device=0, transform_skip=...).  The yardstick
is the host twin (pnn_trquant_tskip_host), which tests/test_hm_transform_skip.py pins to HM's own output and tests/test_transform_skip.py
to a restatement.  Everything at zero tolerance, every raw call between guard bytes."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import transform_skip_cases as tc
from tests import util
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, ptr, untouched

pytestmark = pytest.mark.gpu

QP_LISTS = {1: (27,), 8: (0, 10, 17, 22, 27, 32, 37, 51)}
ALL = (True,) * 6


def specs_of(n, nq):
    return [(np.uint32, (nq, n))] * 3 + [(np.uint8, (nq, n, 4, 4)), (np.uint64, (nq, n)), (np.uint8, (nq, n))]


def device_call(predictions, targets, modes, qps, sdh, rdoq, lambdas, option, mode_bits, charge_cbf, wanted=ALL, width=4, short=0,
                entry="pnn_trquant_tskip_device"):
    """Raw ABI call, every output between guard bytes: (rc, outputs or None, guards intact).  The ts_flag pointer travels behind the
    options, so the call is spelled out here with util's guarded buffers."""
    import torch
    n, nq = predictions.shape[0], len(qps)
    d_p, d_t = dev(predictions), dev(targets)
    d_m = None if modes is None else dev(modes)
    d_b = None if mode_bits is None else dev(mode_bits.view(np.int32))
    L = _lib.lib()
    need = L.pnn_trquant_tskip_workspace_bytes(4, n, nq) if option in (1, 2) else 0
    d_ws = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")
    specs = specs_of(n, nq)
    bufs = util.guarded(specs)
    out = [b.data_ptr() + util.PAD if want else None for b, want in zip(bufs, wanted)]
    c_lambdas = None if lambdas is None else (ctypes.c_double * nq)(*lambdas)
    front = (ip._context(0), width, d_p.data_ptr(), d_t.data_ptr(), n, ptr(d_m), (ctypes.c_int * max(nq, 1))(*qps), nq)
    if entry == "pnn_trquant_rdoq_device":
        rc = L.pnn_trquant_rdoq_device(*front, *out[:5], sdh, rdoq, c_lambdas, util.stream())
    else:
        rc = L.pnn_trquant_tskip_device(*front, *out[:5], sdh, rdoq, c_lambdas, option, ptr(d_b), charge_cbf, out[5],
                                        d_ws.data_ptr() if need else None, max(need - short, 0), util.stream())
    outs, intact = util.collect(bufs, wanted, specs)
    return rc, outs, intact


def same(outs, host, wanted, label):
    for name, got, want, full in zip(tc.KEYS, outs, wanted, host):
        assert (got is None) == (not want), (label, name)
        assert got is None or np.array_equal(got, full), "%s %s: %d differing values" % (label, name, (got != full).sum())


@pytest.mark.parametrize("nb_qps", (1, 8))
@pytest.mark.parametrize("rdoq", (0, 1))
@pytest.mark.parametrize("sdh", (0, 1))
def test_kernels_against_host_twin(nb_qps, rdoq, sdh):
    """n = 1, 65 (one workgroup plus one unit) and 129; forced and decide; mode_bits and lambdas given and NULL; modes given and NULL;
    charge_cbf 0 and 1"""
    qps = QP_LISTS[nb_qps]
    own = [ip.hm_intra_lambda(q) * (0.4 + 0.3 * k) for k, q in enumerate(qps)]
    for n in (1, 65, 129):
        predictions, targets, modes = tc.blocks(n)
        mode_bits = tc.seeded_mode_bits(nb_qps, n)
        for option, m, bits, cbf, lambdas in ((1, modes, None, 1, None), (2, modes, mode_bits, 1, None), (2, None, None, 0, own)):
            label = "n %d, %d QPs, rdoq %d, sdh %d, option %d, modes %s" % (n, nb_qps, rdoq, sdh, option, m is not None)
            rc, host = tc.host_entry(predictions, targets, m, qps, sdh, rdoq, lambdas, option, bits, cbf)
            assert rc == 0, label
            rc, outs, intact = device_call(predictions, targets, m, qps, sdh, rdoq, lambdas, option, bits, cbf)
            assert rc == 0 and intact, label
            same(outs, host, ALL, label)
            if option == 2 and n == 129:
                assert 0 < host[5].sum() < host[5].size, label           # both forms are kept somewhere


def test_each_output_alone_and_the_option_off():
    qps = (22, 37)
    predictions, targets, modes = tc.blocks(65)
    mode_bits = tc.seeded_mode_bits(2, 65)
    rc, host = tc.host_entry(predictions, targets, modes, qps, 1, 1, None, 2, mode_bits, 1)
    assert rc == 0
    for k in range(6):
        wanted = tuple(i == k for i in range(6))
        rc, part, intact = device_call(predictions, targets, modes, qps, 1, 1, None, 2, mode_bits, 1, wanted=wanted)
        assert rc == 0 and intact, wanted
        same(part, host, wanted, "alone %d" % k)
    for sdh, rdoq in ((0, 0), (1, 0), (1, 1)):                            # transform_skip 0 against pnn_trquant_rdoq_device
        rc, off, intact = device_call(predictions, targets, modes, qps, sdh, rdoq, None, 0, None, 1)
        assert rc == 0 and intact
        rc, old, intact = device_call(predictions, targets, modes, qps, sdh, rdoq, None, 0, None, 1, wanted=(True,) * 5 + (False,),
                                      entry="pnn_trquant_rdoq_device")
        assert rc == 0 and intact
        for got, want in zip(off[:5], old[:5]):
            assert got.tobytes() == want.tobytes()
        assert not off[5].any()


def test_transform_code_on_the_device():
    predictions, targets, modes = tc.blocks(129)
    mode_bits = tc.seeded_mode_bits(2, 129)
    for option, bits in (('forced', None), ('decide', mode_bits), ('decide', None)):
        kwargs = dict(keep_reconstructions=True, modes=modes, rate=True, sign_data_hiding=True, rdoq=True, transform_skip=option, mode_bits=bits)
        assert_same_dictionary(ip.transform_code(predictions, targets, (22, 37), device=0, **kwargs),
                               ip.transform_code(predictions, targets, (22, 37), **kwargs), "transform_code %s" % option)
    # the defaults: no key and no byte differs from the call without the argument
    kwargs = dict(keep_reconstructions=True, modes=modes, rate=True, sign_data_hiding=True)
    assert_same_dictionary(ip.transform_code(predictions, targets, (22, 37), device=0, transform_skip='off', **kwargs),
                           ip.transform_code(predictions, targets, (22, 37), **kwargs), "transform_code off")


def test_every_refusal_comes_before_a_launch():
    predictions, targets, modes = tc.blocks(65)
    qps = (22, 37)
    eight = np.zeros((3, 8, 8), np.uint8)
    L = _lib.lib()
    ctx = ip._context(0)

    def refused(*args, **kwargs):
        rc, outs, intact = device_call(*args, **kwargs)
        launches = ctypes.c_int(-1)
        assert L.pnn_last_call_stats(ctx, None, None, ctypes.byref(launches)) == 0
        return rc == PNN_E_ARG and intact and untouched(outs), launches

    rc, outs, intact = device_call(predictions, targets, modes, qps, 0, 0, None, 2, None, 1)     # a good call first: its launches are counted
    assert rc == 0 and intact
    good = ctypes.c_int(-1)
    assert L.pnn_last_call_stats(ctx, None, None, ctypes.byref(good)) == 0 and good.value == 3
    for args, kwargs in (((eight, eight, None, qps, 0, 0, None, 1, None, 1), dict(width=8)),           # width 8 with the option on
                         ((eight, eight, None, qps, 0, 0, None, 2, None, 1), dict(width=8)),
                         ((predictions, targets, modes, qps, 0, 0, None, 3, None, 1), {}),            # a bad option value
                         ((predictions, targets, modes, qps, 0, 0, None, -1, None, 1), {}),
                         ((predictions, targets, modes, qps, 0, 0, None, 2, None, 2), {}),            # charge_cbf
                         ((predictions, targets, modes, qps, 0, 0, [1., 0.], 2, None, 1), {}),        # decide without a usable lambda
                         ((predictions, targets, modes, qps, 0, 0, [1., float('inf')], 2, None, 1), {}),
                         ((predictions, targets, modes, qps, 0, 0, None, 2, None, 1), dict(short=1)),  # a workspace one byte short
                         ((predictions, targets, modes, qps, 0, 0, None, 1, None, 1), dict(short=1)),
                         ((predictions, targets, modes, (22, 52), 0, 0, None, 1, None, 1), {}),
                         ((predictions, targets, modes, qps, 0, 0, None, 1, None, 1), dict(wanted=(False,) * 6))):
        ok, launches = refused(*args, **kwargs)
        assert ok, (args[3:], kwargs)
        assert launches.value == good.value, "a refused call reset or added to the launch count"
