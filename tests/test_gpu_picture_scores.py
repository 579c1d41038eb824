"""GPU tests of the scoring path from pictures (pnn_score_pictures_device, pnn_score_f32_device, evaluation.score_masks_from_pictures):
every value of the mask loop's dictionaries against the existing evaluator, bit for bit, on every width and kind of net; the
search from pictures against the dense-pattern search across a workgroup boundary; the rounding rule; NULL outputs; argument
errors; the split-precision mode; the IPFCN-S keys.  Zero tolerance everywhere: equality follows from the f32 order contract
(a block's bits depend neither on its batch nor on the entry point), the identical rounding rule and integer SSEs."""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from context_adaptive_neural_network_based_prediction_amd import ipfcns as I
from tests import util
from tests.util import PNN_E_ARG, assert_same_dictionary, dev, ipfcns_params, pictures, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OUTPUTS = ("targets", "pnn_u8", "pnn_f32", "pnn_sse", "hevc_mode", "hevc_sse", "hevc_pred")
POSITIONS = ((0, 0), (9, 14), (5, 3))              # the near corner, the far one (odd, no multiple of 4), one in between


def guarded(n, w):
    """One guard-filled device buffer per output of pnn_score_pictures_device, in the order of OUTPUTS."""
    import torch
    u8 = lambda fill: torch.full((n, w, w), fill, dtype=torch.uint8, device="cuda")
    return [u8(0xA1), u8(0xA2), torch.full((n, w, w), -777., dtype=torch.float32, device="cuda"),
            torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda"),
            torch.full((n,), -7, dtype=torch.int32, device="cuda"), u8(0xA3)]


def score(ctx, w, imgs, rows, cols, mask, wanted=(True,) * 7, bufs=None, shape=None):
    """Raw ABI call on pictures [images, H, W]; returns (rc, the seven outputs as numpy -- the guards where one was not asked for)."""
    import torch
    images, H, W = shape or imgs.shape
    positions = len(rows)
    n = imgs.shape[0] * positions
    bufs = bufs or guarded(n, w)
    d_i, d_r, d_c = dev(imgs), dev(np.asarray(rows, np.int32)), dev(np.asarray(cols, np.int32))
    rc = _lib.lib().pnn_score_pictures_device(ctx, w, d_i.data_ptr(), images, H, W, d_r.data_ptr(), d_c.data_ptr(), positions, mask[0],
                                              mask[1], *[b.data_ptr() if want else None for b, want in zip(bufs, wanted)], stream())
    torch.cuda.synchronize()
    out = [b.cpu().numpy() for b in bufs]
    for k in (3, 5):
        out[k] = out[k].view(np.uint32)
    return rc, out


def untouched(out, n, w, which=range(7)):
    want = [b.cpu().numpy() for b in guarded(n, w)]
    return all(out[k].tobytes() == want[k].tobytes() for k in which)


def targets_of(imgs, w, rows, cols):
    return np.array([img[r + w:r + 2 * w, c + w:c + 2 * w] for img in imgs for r, c in zip(rows, cols)])


def make_net(w, kind, batch):
    import context_adaptive_neural_network_based_prediction_amd as P
    if kind == "trained":
        return P.PredictionNeuralNetwork(batch, w, False, path_to_model=os.path.join(GOLD, "conv%d_single.pnnw" % w))
    return util.make_net(w, kind == "fc", batch, seed=40 + w)


CASES = [("trained", 4, ((0, 0), (4, 0), (0, 4), (4, 4))),
         ("trained", 8, tuple((a, b) for a in (0, 4, 8) for b in (0, 4, 8))),
         ("fc", 4, ((0, 0), (4, 0), (0, 4), (4, 4))),
         ("fc", 8, tuple((a, b) for a in (0, 4, 8) for b in (0, 4, 8))),
         ("conv", 16, ((0, 0), (16, 16), (4, 8))),
         ("conv", 32, ((0, 0), (32, 32), (4, 16))),
         ("conv", 64, ((0, 0), (32, 64)))]             # (0, 0) at w = 64: the descriptor's shift by 32


@pytest.mark.parametrize("kind, w, masks", CASES, ids=["%s%d" % c[:2] for c in CASES])
def test_whole_dictionary_equals_the_existing_evaluator(kind, w, masks):
    imgs = pictures(2, 3 * w + 9, 3 * w + 14, 100 + w)[..., None]
    rows = np.array([p[0] for p in POSITIONS], np.int64)
    cols = np.array([p[1] for p in POSITIONS], np.int64)
    n = 2 * len(POSITIONS)
    net = make_net(w, kind, n)
    got = evaluation.score_masks_from_pictures(imgs, w, rows, cols, net, util.MEAN, masks)
    assert list(got) == list(masks)
    for mask in masks:
        want = evaluation.predict_mask_vs_hevc_best_mode(imgs, w, rows, cols, net, n, util.MEAN, mask)
        assert_same_dictionary(got[mask], want, "%s w %d mask %s" % (kind, w, mask))
        assert got[mask]['targets_uint8'].tobytes() == targets_of(imgs[..., 0], w, rows, cols).tobytes()
    # without the predictions only the scores come back, and they are the same
    lean = evaluation.score_masks_from_pictures(imgs, w, rows, cols, net, util.MEAN, masks[:2], keep_predictions=False)
    for mask in masks[:2]:
        assert set(lean[mask]) == {'indices_hevc_best_mode', 'psnrs_hevc_best_mode', 'psnrs_pnn', 'frequency_win_pnn', 'mean_psnr_pnn'}
        assert_same_dictionary(lean[mask], {k: got[mask][k] for k in lean[mask]}, "lean %s" % (mask,))
    with pytest.raises(ValueError, match="`mean_training` differs from the predictor's mean"):
        evaluation.score_masks_from_pictures(imgs, w, rows, cols, net, util.MEAN + 1., masks)
    net.close()


def dense_search(w, imgs, rows, cols, mask):
    """pnn_hevc_best_mode_device on the dense patterns and target copies of the same blocks: (index, SSE, prediction)."""
    import torch
    pats = ip.extract_intra_patterns(imgs[..., None], w, np.asarray(rows) + w - 1, np.asarray(cols) + w - 1, mask)[..., 0]
    tg = targets_of(imgs, w, rows, cols)
    idx, sse, pred, _ = ip.best_modes_device(dev(pats), dev(tg), w)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sse.cpu().numpy().view(np.uint32), pred.cpu().numpy(), tg


@pytest.mark.parametrize("w, images, positions", [(4, 5, 13), (16, 1, 17)])       # 65 and 17 blocks: one more than a workgroup takes
def test_search_from_pictures_equals_the_dense_search_across_a_workgroup(w, images, positions):
    H, W = 3 * w + 9, 3 * w + 14
    imgs = pictures(images, H, W, 200 + w)
    rng = np.random.default_rng(210 + w)
    rows, cols = rng.integers(0, 10, positions), rng.integers(0, 15, positions)
    rows[-1], cols[-1] = 9, 14
    # block 0: reference samples all 0 against a target of 255 -- no mode beats 0 dB: index 0, all-zero prediction
    imgs[0] = 0
    imgs[0, rows[0] + w:rows[0] + 2 * w, cols[0] + w:cols[0] + 2 * w] = 255
    n = images * positions
    for mask in ((0, 0), (w, w)):
        rc, out = score(ip._context(0), w, imgs, rows, cols, mask, (True, False, False, False, True, True, True))
        assert rc == 0
        idx, sse, pred, tg = dense_search(w, imgs, rows, cols, mask)
        assert out[0].tobytes() == tg.tobytes()
        np.testing.assert_array_equal(out[4], idx)
        np.testing.assert_array_equal(out[5], sse)
        np.testing.assert_array_equal(out[6], pred)
        assert out[4][0] == 0 and out[5][0] == 65025 * w * w and not out[6][0].any()
        assert untouched(out, n, w, (1, 2, 3))


def score_f32(ctx, w, pred, imgs, rows, cols, wanted=(True, True), guard_blocks=None):
    """Raw call of the epilogue entry into guard-filled buffers of n blocks (guard_blocks of them for an empty call)."""
    import torch
    n = guard_blocks or imgs.shape[0] * len(rows)
    u8 = torch.full((n, w, w), 0xA2, dtype=torch.uint8, device="cuda")
    sse = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_p, d_i, d_r, d_c = dev(pred), dev(imgs), dev(np.asarray(rows, np.int32)), dev(np.asarray(cols, np.int32))
    rc = _lib.lib().pnn_score_f32_device(ctx, w, d_p.data_ptr(), d_i.data_ptr(), imgs.shape[0], imgs.shape[1], imgs.shape[2], d_r.data_ptr(),
                                         d_c.data_ptr(), len(rows), u8.data_ptr() if wanted[0] else None,
                                         sse.data_ptr() if wanted[1] else None, stream())
    torch.cuda.synchronize()
    return rc, u8.cpu().numpy(), sse.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def contexts():
    """Model-less contexts of mean 0 and of the training mean."""
    L = _lib.lib()
    made = []
    for mean in (0., util.MEAN):
        ctx = ctypes.c_void_p()
        _lib.check(L.pnn_create_empty(ctypes.byref(ctx), ctypes.c_float(mean), 0))
        made.append(ctx)
    yield made
    for ctx in made:
        L.pnn_destroy(ctx)


def test_rounding_rule_half_to_even_and_both_clamps(contexts):
    w = 4
    imgs = pictures(1, 3 * w, 3 * w, 300)
    pred = np.zeros((1, w, w), np.float32)
    pred.ravel()[:8] = [-1., -0.5, 0.5, 1.5, 2.5, 254.5, 255.5, 300.]
    rc, u8, sse = score_f32(contexts[0], w, pred, imgs, [0], [0])
    assert rc == 0
    assert list(u8.ravel()[:8]) == [0, 0, 0, 2, 2, 254, 255, 255] and not u8.ravel()[8:].any()
    tg = targets_of(imgs, w, [0], [0])
    assert sse[0] == ((u8.astype(np.int64) - tg) ** 2).sum()


@pytest.mark.parametrize("w", (4, 64))
def test_random_floats_equal_the_numpy_cast_and_sse(contexts, w):
    imgs = pictures(2, 3 * w + 9, 3 * w + 14, 310 + w)
    rows, cols = [p[0] for p in POSITIONS], [p[1] for p in POSITIONS]
    rng = np.random.default_rng(320 + w)
    pred = rng.uniform(-300., 300., (6, w, w)).astype(np.float32)
    halves = rng.random(pred.shape) < 0.25                # exact ties around both means
    pred[halves] = (rng.integers(-130, 260, pred.shape)[halves] + 0.5).astype(np.float32)
    tg = targets_of(imgs, w, rows, cols)
    for ctx, mean in zip(contexts, (0., util.MEAN)):
        rc, u8, sse = score_f32(ctx, w, pred, imgs, rows, cols)
        assert rc == 0
        want = evaluation.cast_float_to_uint8(pred + np.float32(mean))
        np.testing.assert_array_equal(u8, want)
        np.testing.assert_array_equal(sse, ((want.astype(np.int64) - tg) ** 2).sum(axis=(1, 2)))
        for wanted in ((True, False), (False, True)):
            rc, u8_1, sse_1 = score_f32(ctx, w, pred, imgs, rows, cols, wanted)
            assert rc == 0
            assert (u8_1.tobytes() == u8.tobytes()) if wanted[0] else (u8_1 == 0xA2).all()
            assert (sse_1.tobytes() == sse.tobytes()) if wanted[1] else (sse_1.view(np.int32) == -7).all()


def test_each_output_alone_gives_the_bits_of_all_together():
    w = 8
    imgs = pictures(2, 3 * w + 9, 3 * w + 14, 400)
    rows, cols = [p[0] for p in POSITIONS], [p[1] for p in POSITIONS]
    net = make_net(w, "trained", 6)
    rc, full = score(net.ctx, w, imgs, rows, cols, (4, 0))
    assert rc == 0
    for k in range(7):
        wanted = tuple(j == k for j in range(7))
        rc, got = score(net.ctx, w, imgs, rows, cols, (4, 0), wanted)
        assert rc == 0, OUTPUTS[k]
        assert got[k].tobytes() == full[k].tobytes(), OUTPUTS[k]
        assert untouched(got, 6, w, [j for j in range(7) if j != k]), OUTPUTS[k]
    net.close()


def test_empty_calls_and_bad_arguments_leave_the_outputs_untouched():
    L = _lib.lib()
    w = 8
    H, W = 3 * w + 9, 3 * w + 14
    imgs = pictures(2, H, W, 500)
    rows, cols = [p[0] for p in POSITIONS], [p[1] for p in POSITIONS]
    net = make_net(w, "trained", 6)
    bare = ip._context(0)
    # n == 0: no image, no position
    rc, out = score(net.ctx, w, imgs[:0], rows, cols, (0, 0), bufs=guarded(6, w))
    assert rc == 0 and untouched(out, 6, w)
    rc, out = score(net.ctx, w, imgs, [], [], (0, 0), bufs=guarded(6, w))
    assert rc == 0 and untouched(out, 6, w)
    assert L.pnn_score_pictures_device(net.ctx, w, None, 0, H, W, None, None, 3, 0, 0, None, None, None, None, dev(np.zeros(1, np.uint8)).data_ptr(),
                                       None, None, stream()) == 0
    bad = [dict(w=12), dict(w=0), dict(mask=(12, 0)), dict(mask=(0, 12)), dict(mask=(-4, 0)), dict(mask=(2, 0)), dict(mask=(0, 6)),
           dict(rows=[0, -1, 5]), dict(cols=[0, 14, -3]), dict(rows=[0, 10, 5]), dict(cols=[0, 15, 3]),
           dict(shape=(2, H - 1, W)), dict(shape=(2, H, W - 1)), dict(wanted=(False,) * 7),
           dict(ctx=bare, wanted=(False, True, False, False, False, False, False)),
           dict(ctx=bare, wanted=(True, False, True, False, True, True, True)),
           dict(ctx=bare, wanted=(False, False, False, True, False, False, False))]
    for case in bad:
        a = dict(ctx=net.ctx, w=w, rows=rows, cols=cols, mask=(0, 0), wanted=(True,) * 7, shape=None)
        a.update(case)
        rc, out = score(a["ctx"], a["w"], imgs, a["rows"], a["cols"], a["mask"], a["wanted"], bufs=guarded(6, w), shape=a["shape"])
        assert rc == PNN_E_ARG, case
        assert L.pnn_last_error(a["ctx"]), case
        assert untouched(out, 6, w), case
    assert L.pnn_score_pictures_device(None, w, None, 0, H, W, None, None, 0, 0, 0, None, None, None, None, None, None, None, stream()) == PNN_E_ARG
    # the targets and the HEVC outputs alone need no model
    rc, out = score(bare, w, imgs, rows, cols, (0, 0), (True, False, False, False, True, True, True))
    assert rc == 0 and not untouched(out, 6, w, [0]) and untouched(out, 6, w, (1, 2, 3))
    # the epilogue entry: same checks
    pred = np.zeros((6, w, w), np.float32)
    for case in (dict(w=12), dict(rows=[0, -1, 5]), dict(cols=[0, 15, 3]), dict(wanted=(False, False))):
        a = dict(w=w, rows=rows, cols=cols, wanted=(True, True))
        a.update(case)
        rc, u8, sse = score_f32(bare, a["w"], pred, imgs, a["rows"], a["cols"], a["wanted"])
        assert rc == PNN_E_ARG and (u8 == 0xA2).all() and (sse.view(np.int32) == -7).all(), case
    rc, u8, sse = score_f32(bare, w, pred[:0], imgs[:0], rows, cols, guard_blocks=6)      # n == 0 with real output buffers
    assert rc == 0 and (u8 == 0xA2).all() and (sse.view(np.int32) == -7).all()
    net.close()


def test_split_precision_mode():
    """precision = 1: targets and HEVC outputs are those of float32; the uint8 predictions and SSEs are the numpy epilogue of the
    same call's floats.  (No claim against the host-array path in that mode.)"""
    w = 8
    imgs = pictures(2, 3 * w + 9, 3 * w + 14, 600)
    rows, cols = [p[0] for p in POSITIONS], [p[1] for p in POSITIONS]
    net = make_net(w, "trained", 6)
    rc, f32 = score(net.ctx, w, imgs, rows, cols, (0, 4))
    assert rc == 0
    net.set_option("precision", 1)
    rc, sp = score(net.ctx, w, imgs, rows, cols, (0, 4))
    assert rc == 0
    assert _lib.lib().pnn_check_range(net.ctx, stream(), None) == 0
    for k in (0, 4, 5, 6):
        assert sp[k].tobytes() == f32[k].tobytes(), OUTPUTS[k]
    want = evaluation.cast_float_to_uint8(sp[2] + np.float32(util.MEAN))
    np.testing.assert_array_equal(sp[1], want)
    np.testing.assert_array_equal(sp[3], ((want.astype(np.int64) - sp[0]) ** 2).sum(axis=(1, 2)))
    net.close()


def test_ipfcns_keys_at_no_mask_only():
    w = 4
    imgs = pictures(2, 3 * w + 9, 3 * w + 14, 700)[..., None]
    rows, cols = np.array([4, 9, 5], np.int64), np.array([6, 14, 4], np.int64)     # the reference lines start 4 above-left of the context
    net = make_net(w, "trained", 6)
    ipf = I.NetIpfcns(w, ipfcns_params(w, 94))
    got = evaluation.score_masks_from_pictures(imgs, w, rows, cols, net, util.MEAN, ((4, 4), (0, 0)), net_ipfcns=ipf)
    want = evaluation.predict_mask_vs_hevc_best_mode_and_ipfcns(imgs, w, rows, cols, net, 6, util.MEAN, ipf)
    assert 'psnrs_ipfcns' in want and 'predictions_ipfcns_uint8' in want
    assert_same_dictionary(got[(0, 0)], want, "IPFCN-S (0, 0)")
    assert not any('ipfcns' in k for k in got[(4, 4)])
    assert_same_dictionary(got[(4, 4)], evaluation.predict_mask_vs_hevc_best_mode(imgs, w, rows, cols, net, 6, util.MEAN, (4, 4)), "(4, 4)")
    without = evaluation.score_masks_from_pictures(imgs, w, rows, cols, net, util.MEAN, ((0, 0),))
    assert not any('ipfcns' in k for k in without[(0, 0)])
    net.close()
    ipf.close()
