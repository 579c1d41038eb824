"""GPU tests of IPFCN-S (pnn_ipfcns_forward_device / pnn_ipfcns_predict_device, csrc/pnn_ipfcns.hip over the exact-f32 tap-GEMM
family): bit for bit against the host twin pnn_ipfcns_forward_host at every width, batch size, tile configuration and slice
size; the fused path from pictures against the twin and numpy; the uint8 epilogue's half-to-even rounding and clipping; NULL
outputs, empty calls and argument errors; and the evaluator's three-way dictionary.  Seeded weights only."""
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
from tests import util
from tests.util import dev, ipfcns_params, pictures, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NATURAL = os.path.join(ROOT, "oracle", "_ref", "natural_luma.npz")
PNN_E_ARG = -1


def rows_for(w, n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 40, (n, I.input_size(w))).astype(np.float32)


@pytest.mark.parametrize("w", I.WIDTHS)
def test_forward_device_equals_the_twin_bit_for_bit(w):
    params = ipfcns_params(w, 10 + w)
    net = I.NetIpfcns(w, params)
    sizes = (1, 7, 64, 1000, 2048 if w == 32 else 8192)
    x = rows_for(w, sizes[-1], 20 + w)
    want = I.forward_host(params, w, x)
    for n in sizes:
        got = net.forward(x[:n])
        assert got.tobytes() == want[:n].tobytes(), "w %d n %d: %d differing values" % (w, n, (got != want[:n]).sum())
    net.close()


@pytest.mark.parametrize("w", I.WIDTHS)
def test_every_tile_configuration_and_slice_size_gives_the_twin_bits(w):
    params = ipfcns_params(w, 30 + w)
    net = I.NetIpfcns(w, params)
    net.set_option("autotune", 0)
    x = rows_for(w, 300, 40 + w)
    want = I.forward_host(params, w, x)
    for cfg in range(-1, _lib.lib().pnn_num_f32_configs()):
        net.set_option("f32_cfg", cfg)
        for n in (5, 300):
            assert net.forward(x[:n]).tobytes() == want[:n].tobytes(), "w %d f32_cfg %d n %d" % (w, cfg, n)
    net.set_option("f32_cfg", -1)
    for chunk in (1, 7, 64):
        net.set_option("max_chunk", chunk)
        assert net.forward(x).tobytes() == want.tobytes(), "w %d max_chunk %d" % (w, chunk)
    net.close()


def twin_predict(params, w, imgs, rows, cols, targets=None):
    x, means = I.extract_pairs_groups_lines_from_channels_plus_preprocessing(imgs[..., None], w, rows, cols)
    pred = (I.forward_host(params, w, x) + means[:, None]).astype(np.float32)
    u8 = evaluation.cast_float_to_uint8(pred).reshape(-1, w, w)
    sse = None
    if targets is not None:
        sse = ((u8.astype(np.int64) - targets.astype(np.int64)) ** 2).reshape(len(u8), -1).sum(1)
    return u8, pred.reshape(-1, w, w), means, sse


@pytest.mark.parametrize("w", I.WIDTHS)
def test_fused_path_equals_twin_and_numpy(w):
    """>= 65 536 positions per width over several pictures, edge origins included, plus constant pictures 0 .. 255."""
    params = ipfcns_params(w, 50 + w)
    net = I.NetIpfcns(w, params)
    span = 2 * w + 8
    imgs = pictures(4, 3 * span + 13, 4 * span + 9, 60 + w)
    H, W = imgs.shape[1:]
    rng = np.random.default_rng(70 + w)
    npos = 16384
    rows = rng.integers(0, H - span + 1, npos).astype(np.int32)
    cols = rng.integers(0, W - span + 1, npos).astype(np.int32)
    rows[:4] = [0, 0, H - span, H - span]
    cols[:4] = [0, W - span, 0, W - span]
    targets = rng.integers(0, 256, (4 * npos, w, w)).astype(np.uint8)
    u8, f32, means, sse = net.predict_from_channels_device(dev(imgs), dev(rows), dev(cols), dev(targets), True, True, True)
    tu8, tf32, tmeans, tsse = twin_predict(params, w, imgs, rows, cols, targets)
    assert means.tobytes() == tmeans.tobytes()
    assert f32.tobytes() == tf32.tobytes()
    np.testing.assert_array_equal(u8, tu8)
    np.testing.assert_array_equal(sse, tsse)
    const = np.repeat(np.arange(256, dtype=np.uint8), span * span).reshape(256, span, span)
    z = np.zeros(1, dtype=np.int32)
    u8c, f32c, meansc, _ = net.predict_from_channels_device(dev(const), dev(z), dev(z), None, True, True, True)
    tu8c, tf32c, tmc, _ = twin_predict(params, w, const, z, z)
    assert meansc.tobytes() == np.arange(256, dtype=np.float32).tobytes() == tmc.tobytes()
    assert f32c.tobytes() == tf32c.tobytes()
    np.testing.assert_array_equal(u8c, tu8c)
    net.close()


def raw_predict(net, w, imgs, rows, cols, targets, outs, n_override=None):
    import torch
    images, H, W = imgs.shape
    n = images * rows.shape[0]
    bufs = [torch.zeros((n, w, w), dtype=torch.uint8, device="cuda") if outs[0] else None,
            torch.zeros((n, w, w), dtype=torch.float32, device="cuda") if outs[1] else None,
            torch.zeros(n, dtype=torch.float32, device="cuda") if outs[2] else None,
            torch.zeros(n, dtype=torch.int32, device="cuda") if outs[3] else None]
    ptr = (lambda t: None if t is None else t.data_ptr())
    rc = _lib.lib().pnn_ipfcns_predict_device(net.ctx, w, ptr(imgs), images, H, W, ptr(rows), ptr(cols),
                                              rows.shape[0] if n_override is None else n_override, ptr(targets),
                                              *[ptr(b) for b in bufs], stream())
    import torch as T
    T.cuda.synchronize()
    return rc, [None if b is None else b.cpu().numpy() for b in bufs]


def test_null_outputs_empty_calls_and_bad_arguments():
    import torch
    w = 8
    params = ipfcns_params(w, 80)
    net = I.NetIpfcns(w, params)
    span = 2 * w + 8
    imgs = dev(pictures(2, 50, 60, 81))
    rng = np.random.default_rng(82)
    rows = dev(rng.integers(0, 50 - span + 1, 33).astype(np.int32))
    cols = dev(rng.integers(0, 60 - span + 1, 33).astype(np.int32))
    tg = dev(rng.integers(0, 256, (66, w, w)).astype(np.uint8))
    rc, full = raw_predict(net, w, imgs, rows, cols, tg, (1, 1, 1, 1))
    assert rc == 0
    for mask in range(16):
        outs = tuple((mask >> i) & 1 for i in range(4))
        rc, got = raw_predict(net, w, imgs, rows, cols, tg if outs[3] else None, outs)
        assert rc == 0
        for g, f in zip(got, full):
            if g is not None:
                assert g.tobytes() == f.tobytes()
    L = _lib.lib()
    # n = 0 does nothing
    assert L.pnn_ipfcns_predict_device(net.ctx, w, None, 0, 50, 60, None, None, 0, None, None, None, None, None, stream()) == 0
    assert L.pnn_ipfcns_forward_device(net.ctx, w, None, 0, None, stream()) == 0
    # d_sse without targets
    rc, _ = raw_predict(net, w, imgs, rows, cols, None, (1, 0, 0, 1))
    assert rc == PNN_E_ARG
    # out-of-picture origins: every side
    for r, c in ((-1, 0), (0, -1), (50 - span + 1, 0), (0, 60 - span + 1)):
        bad_r = rows.clone(); bad_c = cols.clone()
        bad_r[5] = r; bad_c[5] = c
        out = torch.full((66, w, w), 7, dtype=torch.uint8, device="cuda")
        rc = L.pnn_ipfcns_predict_device(net.ctx, w, imgs.data_ptr(), 2, 50, 60, bad_r.data_ptr(), bad_c.data_ptr(), 33, None,
                                         out.data_ptr(), None, None, None, stream())
        torch.cuda.synchronize()
        assert rc == PNN_E_ARG
        assert (out == 7).all()                          # nothing launched
    # widths without a net / without an architecture; a model-less context
    for bad_w in (64, 5, 16):
        assert L.pnn_ipfcns_predict_device(net.ctx, bad_w, imgs.data_ptr(), 2, 50, 60, rows.data_ptr(), cols.data_ptr(), 33,
                                           None, tg.data_ptr(), None, None, None, stream()) == PNN_E_ARG
        assert L.pnn_ipfcns_forward_device(net.ctx, bad_w, tg.data_ptr(), 1, tg.data_ptr(), stream()) == PNN_E_ARG
    # loader: wrong count, wrong width; a later load replaces the net
    p = np.ascontiguousarray(params)
    assert L.pnn_ipfcns_load(net.ctx, w, p.ctypes.data_as(_lib.f32p), p.size - 1) == PNN_E_ARG
    assert L.pnn_ipfcns_load(net.ctx, 64, p.ctypes.data_as(_lib.f32p), p.size) == PNN_E_ARG
    assert L.pnn_ipfcns_load(net.ctx, 16, p.ctypes.data_as(_lib.f32p), p.size) == PNN_E_ARG
    x = rows_for(w, 9, 83)
    before = net.forward(x)
    p2 = ipfcns_params(w, 84)
    net.load(p2)
    assert net.forward(x).tobytes() == I.forward_host(p2, w, x).tobytes() != before.tobytes()
    net.close()


def test_epilogue_rounds_half_to_even_and_clips():
    """Zero weights and fc4 bias k + 0.5 on integer means: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ...; large gains clip at both ends."""
    w = 4
    K, H, O = I.layer_dims(w)
    span = 2 * w + 8
    const = np.repeat(np.arange(0, 256, 5, dtype=np.uint8), span * span).reshape(-1, span, span)   # integer means
    z = np.zeros(1, dtype=np.int32)
    p = np.zeros(I.n_params(w), dtype=np.float32)
    b4 = np.arange(O, dtype=np.float32) - 7.5             # -7.5 .. 7.5: every mean + b4 is k + 0.5
    p[-O:] = b4
    net = I.NetIpfcns(w, p)
    u8, f32, means, _ = net.predict_from_channels_device(dev(const), dev(z), dev(z), None, True, True, True)
    want = (means[:, None] + b4[None, :]).astype(np.float32)
    assert f32.reshape(-1, O).tobytes() == want.tobytes()
    np.testing.assert_array_equal(u8.reshape(-1, O), np.round(np.clip(want, 0, 255)).astype(np.uint8))
    assert u8.reshape(-1, O)[0, 8] == 0 and u8.reshape(-1, O)[0, 10] == 2        # 0.5 -> 0, 2.5 -> 2
    # clipping: fc4 bias of +-1000
    p[-O:] = np.where(np.arange(O) % 2, 1000.0, -1000.0).astype(np.float32)
    net.load(p)
    u8, _, _, _ = net.predict_from_channels_device(dev(const), dev(z), dev(z), None, True, False, False)
    assert (u8.reshape(-1, O)[:, 1::2] == 255).all() and (u8.reshape(-1, O)[:, 0::2] == 0).all()
    net.close()


def check_three_way(img, w, rows, cols):
    import context_adaptive_neural_network_based_prediction_amd as P
    net = P.PredictionNeuralNetwork(4, w, False, path_to_model=os.path.join(GOLD, "conv%d_single.pnnw" % w))
    params = ipfcns_params(w, 90 + w)
    ipf = I.NetIpfcns(w, params)
    res = evaluation.predict_mask_vs_hevc_best_mode_and_ipfcns(img, w, rows, cols, net, 4, util.MEAN, ipf)
    base = evaluation.predict_mask_vs_hevc_best_mode(img, w, rows, cols, net, 4, util.MEAN)
    n = img.shape[0] * rows.size
    for k in base:
        np.testing.assert_array_equal(res[k], base[k])
    tg = res['targets_uint8']
    psnrs = np.array([evaluation.compute_psnr(tg[i, :, :, 0], res['predictions_ipfcns_uint8'][i, :, :, 0]) for i in range(n)])
    assert res['psnrs_ipfcns'].tobytes() == psnrs.tobytes()
    tu8, _, _, _ = twin_predict(params, w, img[..., 0], (rows + w - 8).astype(np.int32), (cols + w - 8).astype(np.int32))
    np.testing.assert_array_equal(res['predictions_ipfcns_uint8'][..., 0], tu8)
    ref_psnrs, ref_freq = evaluation.compute_performance_neural_network_vs_hevc_best_mode(tg, tu8[..., None], res['psnrs_hevc_best_mode'])
    assert res['psnrs_ipfcns'].tobytes() == ref_psnrs.tobytes()
    assert res['frequency_win_ipfcns'] == ref_freq == np.count_nonzero(psnrs - res['psnrs_hevc_best_mode'] > 0.) / n
    assert res['mean_psnr_ipfcns'] == float(np.mean(psnrs))
    masked = evaluation.predict_mask_vs_hevc_best_mode_and_ipfcns(img, w, rows, cols, net, 4, util.MEAN, ipf, (4, 4))
    assert not any('ipfcns' in k for k in masked)
    net.close()
    ipf.close()


def test_evaluator_three_way_dictionary():
    rng = np.random.RandomState(5)
    if os.path.exists(NATURAL):
        pics = np.load(NATURAL)
        imgs = [pics[k] for k in sorted(pics.files)[:2]]
    else:
        imgs = list(pictures(2, 256, 320, 6))
    for w in (4, 8):                                  # the widths of the committed conv nets
        for img in imgs:
            H, W = img.shape
            rows = (w * rng.randint(1, (H - 3 * w) // w, 16)).astype(np.int64)
            cols = (w * rng.randint(1, (W - 3 * w) // w, 16)).astype(np.int64)
            check_three_way(img[None, :, :, None], w, rows, cols)
