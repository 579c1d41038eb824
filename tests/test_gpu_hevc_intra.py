"""GPU tests of the HEVC best-intra-mode search (pnn_hevc_best_mode_device, csrc/pnn_hevc_intra.hip) and of the evaluator
that scores PNN against it: bit-exact against the reference's records (tests/golden/hevc_intra_ref.npz) and against the host
twin pnn_hevc_intra_predict on random blocks of every width and mask, edge cases, NULL outputs, argument errors, and
evaluation.predict_mask_vs_hevc_best_mode with the reference's trained conv-8 net."""
import ctypes
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import util
from tests.util import PNN_E_ARG, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NATURAL = os.path.join(ROOT, "oracle", "_ref", "natural_luma.npz")
WIDTHS = (4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLD, "hevc_intra_ref.npz"))


def run(w, pats, tgts, outputs=(True, True, True, True)):
    """Raw ABI call on [n, h, w'] patterns and [n, w, w] targets; returns (rc, index, sse, pred, mode_sse) as numpy (None where
    the output was not asked for)."""
    import torch
    n = len(tgts)
    bufs = [torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda"),
            torch.full((n, w, w), 0xCD, dtype=torch.uint8, device="cuda"), torch.full((n, 35), -7, dtype=torch.int32, device="cuda")]
    ptrs = [b.data_ptr() if want else None for b, want in zip(bufs, outputs)]
    d_p, d_t = dev(pats), dev(tgts)
    rc = _lib.lib().pnn_hevc_best_mode_device(ip._context(0), w, d_p.data_ptr(), pats.shape[1], pats.shape[2], d_t.data_ptr(),
                                              n, *ptrs, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = [b.cpu().numpy() if want else None for b, want in zip(bufs, outputs)]
    for k in (1, 3):
        if out[k] is not None:
            out[k] = out[k].view(np.uint32)
    return [rc] + out


def twin_all(pats, w):
    return np.array([[ip.predict_via_hevc_mode(np.ascontiguousarray(p[..., None]), w, m)[..., 0] for m in range(35)]
                     for p in pats], np.uint8)


def random_patterns(rng, n, w, mask):
    return rng.integers(0, 256, (n, 2 * w + 1 - mask[1], 2 * w + 1 - mask[0])).astype(np.uint8)


@pytest.mark.parametrize("w", WIDTHS)
def test_kernel_equals_the_reference_records(ref, w):
    for tag in ("", "_masked", "_random"):
        key = "best_w%d%s" % (w, tag)
        pats, tgts = ref[key + "_patterns"], ref[key + "_targets"]
        rc, idx, sse, pred, mode_sse = run(w, pats, tgts)
        assert rc == 0
        np.testing.assert_array_equal(idx, ref[key + "_index"])
        np.testing.assert_array_equal(pred, ref[key + "_pred"])
        assert (mode_sse.min(axis=1) == sse).all()
        psnr = ip.psnrs_from_sses(sse, w)
        psnr[sse == 65025 * w * w] = 0.
        assert psnr.tobytes() == ref[key + "_psnr"].tobytes(), key
        # the public function gives the same three arrays
        i2, p2, pr2 = ip.predict_series_via_hevc_best_mode(pats[..., None], tgts[..., None])
        assert i2.dtype == np.uint8 and p2.dtype == np.float64 and pr2.shape == tgts.shape + (1,)
        np.testing.assert_array_equal(i2, ref[key + "_index"])
        assert p2.tobytes() == ref[key + "_psnr"].tobytes()
        np.testing.assert_array_equal(pr2[..., 0], ref[key + "_pred"])


@pytest.mark.parametrize("w", WIDTHS)
def test_mode_sses_equal_the_host_twin_on_random_blocks(w):
    rng = np.random.default_rng(w)
    sizes = [1, 3, 69] + ([4096] if w <= 8 else [300] if w == 64 else [])
    for mask in sorted({(0, 0), (w, 0), (0, w), (4, 4), (w, w)}):
        for n in sizes:
            pats = random_patterns(rng, n, w, mask)
            tgts = rng.integers(0, 256, (n, w, w)).astype(np.uint8)
            rc, idx, sse, pred, mode_sse = run(w, pats, tgts)
            assert rc == 0
            check = np.arange(n) if n <= 300 else rng.choice(n, 200, replace=False)    # the host twin is slow in Python
            preds = twin_all(pats[check], w)
            want = ((preds.astype(np.int64) - tgts[check][:, None].astype(np.int64)) ** 2).sum(axis=(2, 3))
            np.testing.assert_array_equal(mode_sse[check], want, err_msg="w=%d mask=%s n=%d" % (w, mask, n))
            np.testing.assert_array_equal(idx, np.argmin(mode_sse, axis=1))
            np.testing.assert_array_equal(pred[check], preds[np.arange(len(check)), idx[check]])


@pytest.mark.parametrize("w", WIDTHS)
def test_ties_and_the_zero_db_case(w):
    pats = np.stack([np.full((2 * w + 1, 2 * w + 1), v, np.uint8) for v in (140, 0, 255)])
    tgts = np.stack([np.full((w, w), v, np.uint8) for v in (140, 255, 0)])
    rc, idx, sse, pred, mode_sse = run(w, pats, tgts)
    assert rc == 0
    assert (mode_sse[0] == 0).all() and idx[0] == 0 and (pred[0] == 140).all()
    assert list(idx[1:]) == [0, 0] and list(sse[1:]) == [65025 * w * w] * 2 and not pred[1:].any()
    i2, p2, _ = ip.predict_series_via_hevc_best_mode(pats[..., None], tgts[..., None])
    assert list(p2[1:]) == [0., 0.]


def test_every_null_output_combination_gives_the_same_bits():
    rng = np.random.default_rng(11)
    for w in (8, 32):
        pats, tgts = random_patterns(rng, 37, w, (4, 0)), rng.integers(0, 256, (37, w, w)).astype(np.uint8)
        full = run(w, pats, tgts)
        for combo in range(1, 16):
            outputs = tuple(bool(combo >> k & 1) for k in range(4))
            got = run(w, pats, tgts, outputs)
            assert got[0] == 0
            for k in range(4):
                if outputs[k]:
                    np.testing.assert_array_equal(got[k + 1], full[k + 1], err_msg="outputs %s" % (outputs,))


def test_zero_blocks_and_bad_arguments():
    import torch
    L = _lib.lib()
    ctx = ip._context(0)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = 8
    p, t = dev(np.zeros((4, 17, 17), np.uint8)), dev(np.zeros((4, 8, 8), np.uint8))
    idx = torch.full((4,), 9, dtype=torch.uint8, device="cuda")
    sse = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    assert L.pnn_hevc_best_mode_device(ctx, w, p.data_ptr(), 17, 17, t.data_ptr(), 0, idx.data_ptr(), sse.data_ptr(), None, None, s) == 0
    assert L.pnn_hevc_best_mode_device(ctx, w, None, 17, 17, None, 0, idx.data_ptr(), None, None, None, s) == 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == 9).all() and (sse.cpu().numpy() == 9).all()          # n = 0 wrote nothing
    bad = [(ctx, 12, p.data_ptr(), 25, 25, t.data_ptr(), 4, idx.data_ptr()),        # width
           (ctx, w, p.data_ptr(), 8, 17, t.data_ptr(), 4, idx.data_ptr()),          # pattern too short
           (ctx, w, p.data_ptr(), 17, 18, t.data_ptr(), 4, idx.data_ptr()),         # pattern too wide
           (ctx, w, p.data_ptr(), 17, 17, t.data_ptr(), -1, idx.data_ptr()),        # n
           (ctx, w, None, 17, 17, t.data_ptr(), 4, idx.data_ptr()),                 # no patterns
           (ctx, w, p.data_ptr(), 17, 17, None, 4, idx.data_ptr()),                 # no targets
           (ctx, w, p.data_ptr(), 17, 17, t.data_ptr(), 4, None)]                   # no output at all
    for args in bad:
        assert L.pnn_hevc_best_mode_device(*args, None, None, None, s) == PNN_E_ARG, args[1:7]
        assert L.pnn_last_error(ctx)
    assert L.pnn_hevc_best_mode_device(None, w, p.data_ptr(), 17, 17, t.data_ptr(), 4, idx.data_ptr(), None, None, None, s) == PNN_E_ARG
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == 9).all()


def test_a_batch_equals_its_blocks_one_at_a_time():
    rng = np.random.default_rng(5)
    for w in WIDTHS:
        pats, tgts = random_patterns(rng, 70, w, (0, w)), rng.integers(0, 256, (70, w, w)).astype(np.uint8)
        rc, idx, sse, pred, mode_sse = run(w, pats, tgts)
        for i in range(0, 70, 7):
            _, i1, s1, p1, m1 = run(w, pats[i:i + 1], tgts[i:i + 1])
            assert i1[0] == idx[i] and s1[0] == sse[i] and (p1[0] == pred[i]).all() and (m1[0] == mode_sse[i]).all()
            j, psnr, pr = ip.predict_via_hevc_best_mode(pats[i][..., None], tgts[i][..., None])
            assert j == idx[i] and pr.shape == (w, w, 1) and (pr[..., 0] == pred[i]).all()
            assert psnr == evaluation.compute_psnr(tgts[i], pred[i])


def check_evaluator(img, w, rows, cols, mask=(0, 0)):
    """predict_mask_vs_hevc_best_mode against the unchanged predict_mask, the host twin and the definition of the win rate."""
    import context_adaptive_neural_network_based_prediction_amd as P
    net = P.PredictionNeuralNetwork(4, w, False, path_to_model=os.path.join(GOLD, "conv%d_single.pnnw" % w))
    res = evaluation.predict_mask_vs_hevc_best_mode(img, w, rows, cols, net, 4, util.MEAN, mask)
    base = evaluation.predict_mask(img, w, rows, cols, net, 4, util.MEAN, mask)
    net.close()
    n = img.shape[0] * rows.size
    assert set(res) >= {'indices_hevc_best_mode', 'psnrs_hevc_best_mode', 'psnrs_pnn', 'frequency_win_pnn', 'mean_psnr_pnn'}
    assert res['psnrs_pnn'].tobytes() == base['psnrs_pnn'].tobytes()
    np.testing.assert_array_equal(res['predictions_pnn_uint8'], base['predictions_pnn_uint8'])
    np.testing.assert_array_equal(res['targets_uint8'], base['targets_uint8'])
    assert res['mean_psnr_pnn'] == float(np.mean(base['psnrs_pnn']))
    pats = ip.extract_intra_patterns(img, w, rows + w - 1, cols + w - 1, mask)
    tg = res['targets_uint8']
    for i in range(n):
        per_mode = np.array([evaluation.compute_psnr(tg[i, :, :, 0], ip.predict_via_hevc_mode(pats[i], w, m)[..., 0])
                             for m in range(35)])
        assert res['psnrs_hevc_best_mode'][i] == max(per_mode.max(), 0.)
        assert (res['psnrs_hevc_best_mode'][i] >= per_mode).all()
        assert res['indices_hevc_best_mode'][i] == (np.argmax(per_mode) if per_mode.max() > 0 else 0)
        np.testing.assert_array_equal(res['predictions_hevc_best_mode_uint8'][i],
                                      ip.predict_via_hevc_mode(pats[i], w, int(res['indices_hevc_best_mode'][i])))
    diff = res['psnrs_pnn'] - res['psnrs_hevc_best_mode']
    assert res['frequency_win_pnn'] == np.count_nonzero(diff > 0.) / n
    return res


def test_evaluator_on_the_smooth_synthetic_image():
    w = 8
    yy, xx = np.mgrid[0:64, 0:96]
    img = np.clip(90 + 0.9 * xx + 0.5 * yy + 12 * np.sin(xx / 7.0), 0, 255).astype(np.uint8)[None, :, :, None]
    rows = np.array([0, 8, 24, 40], dtype=np.int32)
    cols = np.array([4, 32, 60, 72], dtype=np.int32)
    res = check_evaluator(img, w, rows, cols)
    assert res['psnrs_hevc_best_mode'].min() > 20.0
    check_evaluator(img, w, rows, cols, (4, 8))


def test_evaluator_on_natural_pictures():
    if not os.path.exists(NATURAL):
        pytest.skip("oracle/_ref/natural_luma.npz is generated from the reference checkout by __graft_entry__.build() (tests/golden/make_natural.py)")
    pics = np.load(NATURAL)
    rng = np.random.RandomState(3)
    for w in (4, 8):
        img = pics[sorted(pics.files)[0]]
        H, W = img.shape
        rows = (w * rng.randint(0, (H - 3 * w) // w, 24)).astype(np.int64)
        cols = (w * rng.randint(0, (W - 3 * w) // w, 24)).astype(np.int64)
        check_evaluator(img[None, :, :, None], w, rows, cols)
