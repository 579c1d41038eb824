"""The exact-f32 mode ("precision" 0) against the bit-exact CPU model of its summation order (oracle/pnn_order.c, written from
INTEGRATION.md section 4 "Exact-f32 summation order, revision 6") -- at ZERO tolerance: every float bit, every Pel value, for every
architecture, every kernel family a batch size or a launch option selects, from host arrays and from the picture plane.  And the
split-f16 mode ("precision" 1), which has no bit-level model, against float64 with a tie-aware per-pixel Pel rule.

Floats are compared with np.array_equal (+0 == -0).  The autouse `precision` fixture of test_gpu_parity.py does not apply here:
every net sets its precision itself.
"""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import weights as wts
from tests import torch_formulation as TF
from tests import util

pytestmark = pytest.mark.gpu

FLOAT_ATOL = 2e-3                                     # test_gpu_parity.py: the split mode's float bound
TIE_MARGIN = 2e-3                                     # split mode: Pel must equal float64's rounding unless p + mean is this close to k + .5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARCHS = [(True, 4), (True, 8), (True, 16), (False, 4), (False, 8), (False, 16), (False, 32), (False, 64)]
ARCH_IDS = ["%s%d" % ("fc" if f else "conv", w) for f, w in ARCHS]
# batch sizes past the small kernels: FC -- fc_out_f32 (below 1024 blocks), the output layer from stored activations and the fused
# output layer (2048); conv -- tapgemm_f32_kernel tiles, position-major tiles, two streams
BIG = {(True, 4): (300, 700, 2048), (True, 8): (300, 700, 2048), (True, 16): (300, 700, 2048),
       (False, 4): (130,), (False, 8): (130,), (False, 16): (130, 384), (False, 32): (130,), (False, 64): (36,)}
SMALL = (1, 2, 3, 17)


@pytest.fixture(scope="module")
def pnn():
    import context_adaptive_neural_network_based_prediction_amd as P
    return P


def _net(pnn, n, w, is_fc, params, precision=0):
    net = pnn.PredictionNeuralNetwork(n, w, is_fc, params=params)
    net.set_option("precision", precision)
    return net


def _ins(is_fc, above, left):
    return (util.flatten_fc(above, left),) if is_fc else (above, left)


def _model(oracle, params, w, is_fc, above, left, variant=0):
    if is_fc:
        return oracle.order_fc_forward(params, w, util.flatten_fc(above, left), variant)
    return oracle.order_conv_forward(params, w, above, left, variant)


def _same_bits(got, want, what, oracle=None, model_args=None):
    """np.array_equal, with a report that names the parts of the order a mismatch is consistent with (the ladder of the issue:
    which single departure from the order, if any, reproduces the GPU's bits)."""
    got = np.asarray(got).reshape(want.shape)
    if np.array_equal(got, want):
        return
    diff = got != want
    msg = "%s: %d of %d values differ from the order model, max |delta| %.3g" % (
        what, int(diff.sum()), diff.size, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
    if oracle is not None and model_args is not None:
        hits = [name for name, (bit, _, _) in oracle.ORDER_VARIANTS.items()
                if np.array_equal(got, _model(oracle, *model_args, variant=bit).reshape(want.shape))]
        msg += "; departures that reproduce the GPU: %s" % (hits or "none")
    raise AssertionError(msg)


def _check_net(net, oracle, params, w, is_fc, above, left, what):
    want = _model(oracle, params, w, is_fc, above, left)
    got = net.predict(*_ins(is_fc, above, left))
    _same_bits(got[..., 0] if got.ndim == 4 else got, want, what + " (float)", oracle, (params, w, is_fc, above, left))
    assert np.array_equal(net.predict_pel(*_ins(is_fc, above, left)), oracle.epilogue(want, util.MEAN)), what + " (Pel)"
    return want


def test_library_tag_is_the_models(pnn, oracle):
    """The f32 mode reports the order the model implements; the model refuses any other tag (the split mode's, a later revision's)."""
    net = _net(pnn, 1, 8, True, util.make_params(8, True, 1))
    tag = net.arithmetic_tag()
    assert tag == oracle.order_tag()
    oracle.require_order_tag(tag)
    net.set_option("precision", 1)
    with pytest.raises(ValueError):
        oracle.require_order_tag(net.arithmetic_tag())
    with pytest.raises(ValueError):
        oracle.require_order_tag(tag.replace("pnn-order-6", "pnn-order-7"))
    net.close()


@pytest.mark.parametrize("is_fc,w", ARCHS, ids=ARCH_IDS)
def test_every_batch_size_matches_the_order_model(pnn, oracle, is_fc, w):
    """Small kernels and tails (1, 2, 3, 17 blocks) and the batch kernels (BIG): float and Pel predictions = the model's, bit for bit.
    Seeded weights with out_gain (x 3 on conv: both clamps of the epilogue with half the contexts masked), contexts with masked units."""
    params = util.make_params(w, is_fc, 601 + w, out_gain=util.out_gain(w, is_fc) * (1 if is_fc else 3))
    n_max = max(SMALL + BIG[(is_fc, w)])
    above, left = util.make_contexts(w, n_max, 602 + w, masked_fraction=0.5)
    want = _model(oracle, params, w, is_fc, above, left)
    pel_want = oracle.epilogue(want, util.MEAN)
    assert pel_want.min() == 0 and pel_want.max() == 255, "the inputs must exercise both clamps"
    net = _net(pnn, n_max, w, is_fc, params)
    for n in SMALL + BIG[(is_fc, w)]:
        lo = n_max - n if n in SMALL else 0                          # the small calls take the END of the batch: other blocks
        a, l = above[lo:lo + n], left[lo:lo + n]
        got = net.predict(*_ins(is_fc, a, l))[..., 0]
        _same_bits(got, want[lo:lo + n], "%d blocks" % n, oracle, (params, w, is_fc, a, l))
        assert np.array_equal(net.predict_pel(*_ins(is_fc, a, l)), pel_want[lo:lo + n]), "%d blocks (Pel)" % n
    net.close()


# (option, values in the order they are set; the last one is the default)
OPTIONS = [("f32_small", (0, 1)), ("seg_fold", (0, 1)), ("tails", (0, 1)), ("chain_io", (0, 1)), ("fc_out_f32", (0, 1)),
           ("fuse_last", (0, 1)), ("pair", (0, 1)), ("f32_small_deep", (0, 2, 1))]


@pytest.mark.parametrize("is_fc,w", ARCHS, ids=ARCH_IDS)
def test_launch_options_keep_the_model_bits(pnn, oracle, is_fc, w):
    """Every option that restructures the launches of a pass and claims the same bits, against the model itself on 1 and 5 blocks;
    option "graphs": the first (plain), second (captured) and third (replayed) call of a shape, new inputs each time."""
    params = util.make_params(w, is_fc, 611 + w, out_gain=util.out_gain(w, is_fc))
    above, left = util.make_contexts(w, 5, 612 + w)
    want = _model(oracle, params, w, is_fc, above, left)
    net = _net(pnn, 8, w, is_fc, params)
    for name, values in OPTIONS:
        for v in values:
            net.set_option(name, v)
            got = net.predict(*_ins(is_fc, above, left))[..., 0]
            _same_bits(got, want, "%s = %d, 5 blocks" % (name, v), oracle, (params, w, is_fc, above, left))
            got1 = net.predict(*_ins(is_fc, above[2:3], left[2:3]))[..., 0]
            _same_bits(got1, want[2:3], "%s = %d, 1 block" % (name, v))
    net.set_option("graphs", 1)
    for call in range(3):
        a, l = util.make_contexts(w, 3, 613 + 10 * w + call)
        _check_net(net, oracle, params, w, is_fc, a, l, "graphs = 1, call %d" % (call + 1))
    net.set_option("graphs", 0)
    net.close()


@pytest.mark.parametrize("is_fc,w,n", [(True, 8, 700), (False, 16, 130), (False, 32, 130)])
def test_f32_tile_configurations_match_the_model(pnn, oracle, is_fc, w, n):
    """The f32_cfg sweep (every tapgemm_f32 tile configuration) at a mid size; f32_persist (persistent workgroups) on conv."""
    from context_adaptive_neural_network_based_prediction_amd import _lib
    params = util.make_params(w, is_fc, 621 + w, out_gain=util.out_gain(w, is_fc))
    above, left = util.make_contexts(w, n, 622 + w)
    want = _model(oracle, params, w, is_fc, above, left)
    net = _net(pnn, n, w, is_fc, params)
    net.set_option("autotune", 0)
    for cfg in range(-1, _lib.lib().pnn_num_f32_configs()):
        net.set_option("f32_cfg", cfg)
        _same_bits(net.predict(*_ins(is_fc, above, left))[..., 0], want, "f32_cfg = %d" % cfg)
    net.set_option("f32_cfg", -1)
    if not is_fc:
        for persist in (0, 1, 2, 3):
            net.set_option("f32_persist", persist)
            _same_bits(net.predict(above, left)[..., 0], want, "f32_persist = %d" % persist)
        net.set_option("f32_persist", -1)
    net.close()


@pytest.mark.parametrize("is_fc,w,slice_blocks", [(True, 8, 64), (False, 16, 16), (False, 4, 32)])
def test_multi_slice_host_call_matches_the_model(pnn, oracle, is_fc, w, slice_blocks):
    n = 3 * slice_blocks + 5
    params = util.make_params(w, is_fc, 631 + w, out_gain=util.out_gain(w, is_fc))
    above, left = util.make_contexts(w, n, 632 + w)
    net = _net(pnn, slice_blocks, w, is_fc, params)
    net.set_option("host_slice", slice_blocks)
    _check_net(net, oracle, params, w, is_fc, above, left, "%d blocks in slices of %d" % (n, slice_blocks))
    net.close()


def _device_tbs(xs, ys, flags, stride, w):
    from context_adaptive_neural_network_based_prediction_amd import _lib
    L = _lib.lib()
    units = 2 * w // 4
    arr = (_lib.TbDev * len(xs))()
    for i in range(len(xs)):
        assert L.pnn_make_tb_desc(ctypes.byref(arr[i]), int(ys[i]) * stride + int(xs[i]), stride,
                                  flags[i].ctypes.data_as(_lib.u8p), int(flags[i].sum()), units, units) == 0
    return np.frombuffer(arr, dtype=np.uint8).copy()


@pytest.mark.parametrize("is_fc,w,n", [(True, 4, 300), (True, 8, 64), (True, 16, 40), (False, 4, 64), (False, 8, 64),
                                       (False, 16, 48), (False, 32, 12), (False, 64, 4)], ids=ARCH_IDS)
def test_picture_plane_path_matches_the_model(pnn, oracle, is_fc, w, n):
    """pnn_predict_tbs_device with the gather fused into the first layer and as its own launch: the reference gather (oracle) ->
    model -> epilogue, exactly, float and Pel."""
    import torch
    from context_adaptive_neural_network_based_prediction_amd import _lib
    L = _lib.lib()
    params = util.make_params(w, is_fc, 641 + w, out_gain=util.out_gain(w, is_fc))
    plane = util.make_plane(288, 448, seed=642 + w, pad=16)
    xs, ys, flags = util.make_tbs(288, 448, w, n, seed=643 + w, partial_fraction=0.5)
    above = np.empty((n, w, 3 * w), np.float32)
    left = np.empty((n, 2 * w, w), np.float32)
    for i in range(n):
        rc, above[i], left[i] = oracle.extract_context(plane, int(xs[i]), int(ys[i]), w, flags[i], util.MEAN)
        assert rc == 0
    want = _model(oracle, params, w, is_fc, above, left)
    net = _net(pnn, n, w, is_fc, params)
    d_plane = torch.from_numpy(plane).cuda()
    d_tbs = torch.from_numpy(_device_tbs(xs, ys, flags, plane.shape[1], w)).cuda()
    for fuse in (1, 0):
        net.set_option("fuse_gather", fuse)
        d_dst = torch.full((n, w, w), -1, dtype=torch.int32, device="cuda")
        d_f32 = torch.full((n, w, w), float("nan"), dtype=torch.float32, device="cuda")
        rc = L.pnn_predict_tbs_device(net.ctx, w, d_plane.data_ptr(), 4, d_tbs.data_ptr(), n, d_dst.data_ptr(), d_f32.data_ptr(), None)
        assert rc == 0, L.pnn_last_error(net.ctx)
        torch.cuda.synchronize()
        _same_bits(d_f32.cpu().numpy(), want, "fuse_gather = %d (float)" % fuse, oracle, (params, w, is_fc, above, left))
        assert np.array_equal(d_dst.cpu().numpy(), oracle.epilogue(want, util.MEAN)), "fuse_gather = %d (Pel)" % fuse
    net.close()


@pytest.mark.parametrize("w", [4, 8])
def test_trained_checkpoints_match_the_model(pnn, oracle, w):
    """The two trained conv checkpoints on the recorded real contexts of nets.npz, on synthetic ones, and on natural pictures when
    the fixture exists (built from the reference checkout)."""
    flat, _, _ = wts.load_pnnw(os.path.join(GOLD, "conv%d_single.pnnw" % w))
    g = np.load(os.path.join(GOLD, "nets.npz"))
    sets = [("nets.npz real contexts", g["real%d_above" % w], g["real%d_left" % w]),
            ("synthetic contexts", *util.make_contexts(w, 64, 651 + w))]
    from tests.test_natural import NATURAL, natural_contexts
    if os.path.exists(NATURAL):
        a, l, _ = natural_contexts(w, 256)
        sets.append(("natural contexts", a.astype(np.float32) - np.float32(util.MEAN), l.astype(np.float32) - np.float32(util.MEAN)))
    net = _net(pnn, 256, w, False, flat)
    for what, a, l in sets:
        for lo, hi in ((0, 1), (0, len(a))):
            _check_net(net, oracle, flat, w, False, np.ascontiguousarray(a[lo:hi]), np.ascontiguousarray(l[lo:hi]),
                       "%s, %d blocks" % (what, hi - lo))
    net.close()


def _subnormal_params(w, is_fc):
    """Zero biases, first layer scaled down by 1e-38 and the last one up by 1e38: the hidden activations of the first layers are
    (partly) subnormal, and the predictions still depend on them."""
    flat = util.make_params(w, is_fc, 661 + w, bias_std=0.0)
    specs = wts.tensor_specs(w, is_fc)
    offs = np.concatenate([[0], np.cumsum([int(np.prod(sh)) for _, sh, _ in specs])])
    if is_fc:
        flat[offs[0]:offs[1]] *= np.float32(1e-38)
    else:
        nl = len(wts.STRIDES_BRANCH[w])
        for t in (0, 2 * nl):                                       # both branches' first convolutions
            flat[offs[t]:offs[t + 1]] *= np.float32(1e-38)
    flat[offs[-3]:offs[-2]] *= np.float32(1e38)
    return flat, offs


@pytest.mark.parametrize("is_fc,w,n", [(True, 4, 1), (True, 8, 17), (True, 16, 300), (False, 4, 3), (False, 8, 17), (False, 16, 130),
                                       (False, 32, 2)])
def test_edges_match_the_model(pnn, oracle, is_fc, w, n):
    """A fully masked (all-zero) context, contexts all at -mean and all at 255 - mean, contexts scaled to ~1e4 (the f32 mode has no
    range bound), and weights that make hidden activations subnormal (kept by the kernels, as by the model)."""
    params = util.make_params(w, is_fc, 671 + w, out_gain=util.out_gain(w, is_fc))
    above, left = util.make_contexts(w, n, 672 + w)
    net = _net(pnn, n, w, is_fc, params)
    cases = [("all-zero context", np.zeros_like(above), np.zeros_like(left)),
             ("contexts at -mean", np.full_like(above, -np.float32(util.MEAN)), np.full_like(left, -np.float32(util.MEAN))),
             ("contexts at 255 - mean", np.full_like(above, 255 - np.float32(util.MEAN)), np.full_like(left, 255 - np.float32(util.MEAN))),
             ("contexts x 80", above * np.float32(80), left * np.float32(80))]
    for what, a, l in cases:
        _check_net(net, oracle, params, w, is_fc, a, l, what)
    net.close()
    flat, offs = _subnormal_params(w, is_fc)
    if is_fc:
        h = util.flatten_fc(above, left) @ flat[offs[0]:offs[1]].reshape(5 * w * w, -1)
    else:
        h = flat[offs[0]:offs[1]] * np.float32(100)                   # |taps| x |pixels| of the first convolution
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(h) < tiny) & (h != 0)).any(), "the first layer must produce subnormal values"
    net = _net(pnn, n, w, is_fc, flat)
    want = _check_net(net, oracle, flat, w, is_fc, above, left, "subnormal hidden activations")
    assert np.abs(want).max() > 1e-3, "the subnormal activations must reach the predictions"
    net.close()


@pytest.mark.parametrize("is_fc,w,n", [(True, 8, 9), (False, 16, 7)])
def test_split_mode_range_fallback_is_the_f32_order(pnn, oracle, is_fc, w, n):
    """A split-mode call where one block leaves the f16 range: that block is recomputed on the exact-f32 kernels
    (include/pnn_hip.h, "Input-range contract") -- its bits are the order model's."""
    params = util.make_params(w, is_fc, 91, out_gain=util.out_gain(w, is_fc)).copy()
    specs = wts.tensor_specs(w, is_fc)
    offs = np.concatenate([[0], np.cumsum([int(np.prod(sh)) for _, sh, _ in specs])])
    gain = 300.0 if is_fc else 1000.0
    params[offs[0]:offs[2]] *= gain
    params[offs[-3]:offs[-2]] /= gain
    above, left = util.make_contexts(w, n, 92, masked_fraction=0.0)
    bad = n // 2
    above[bad] *= 40.0
    left[bad] *= 40.0
    net = _net(pnn, n, w, is_fc, params, precision=1)
    got = net.predict(*_ins(is_fc, above, left))[..., 0]
    want = _model(oracle, params, w, is_fc, above[bad:bad + 1], left[bad:bad + 1])
    _same_bits(got[bad:bad + 1], want, "the overflowing block", oracle, (params, w, is_fc, above[bad:bad + 1], left[bad:bad + 1]))
    net.close()


def _check_pel_tie_aware(got, p64, what):
    """Every pixel whose float64 p + mean lies more than TIE_MARGIN from a rounding boundary k + .5 equals float64's rounding; the
    others differ by at most 1."""
    v = np.clip(p64 + util.MEAN, 0.0, 255.0)
    exact = np.floor(v + 0.5)
    near = np.abs(v - np.floor(v) - 0.5) <= TIE_MARGIN
    d = np.abs(got.astype(np.int64) - exact.astype(np.int64))
    assert d.max() <= 1, "%s: max |delta| = %d LSB" % (what, d.max())
    assert not (d[~near] != 0).any(), "%s: %d pixels away from a .5 boundary round differently from float64" % (what, int((d[~near] != 0).sum()))


SPLIT_BATCH = {(True, 4): 700, (True, 8): 700, (True, 16): 700, (False, 4): 130, (False, 8): 130, (False, 16): 130, (False, 32): 48,
               (False, 64): 16}


@pytest.mark.parametrize("is_fc,w", ARCHS, ids=ARCH_IDS)
def test_split_mode_against_float64(pnn, oracle, is_fc, w):
    """The split-f16 mode cannot be modelled bit for bit (the f16 MFMA's internal accumulation is not specified): float predictions
    within FLOAT_ATOL of float64, Pel equal to float64's rounding wherever float64 is not within TIE_MARGIN of a .5 boundary."""
    n_max = SPLIT_BATCH[(is_fc, w)]
    params = util.make_params(w, is_fc, 681 + w, out_gain=util.out_gain(w, is_fc))
    above, left = util.make_contexts(w, n_max, 682 + w)
    p64 = TF.fc_forward(params, w, util.flatten_fc(above, left), np.float64) if is_fc else TF.conv_forward(params, w, above, left, np.float64)
    net = _net(pnn, n_max, w, is_fc, params, precision=1)
    for n in (1, 17, n_max):
        got = net.predict(*_ins(is_fc, above[:n], left[:n]))[..., 0]
        np.testing.assert_allclose(got, p64[:n], rtol=0, atol=FLOAT_ATOL, err_msg="%d blocks" % n)
        _check_pel_tie_aware(net.predict_pel(*_ins(is_fc, above[:n], left[:n])), p64[:n], "%d blocks" % n)
    net.close()
