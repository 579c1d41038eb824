"""GPU tests of HM's reference-sample smoothing in the two 35-mode kernels (the SMOOTH instantiations of hevc_best_mode_kernel and
hevc_mode_hads_kernel) behind the four *_hm device entries, and of the evaluator's reference_smoothing option.

Every comparison has zero tolerance, against the host twin (pnn_hevc_intra_predict_hm, pnn_hevc_mode_hads_hm_host), which
tests/test_hevc_smoothing.py pins to a numpy restatement of the filter.  The dense shapes cross one workgroup boundary with a ragged
last group (the SATD kernel takes 64, 64, 16, 4, 1 blocks per workgroup at w = 4 .. 64, the SSE search 64, 64, 16, 8, 4): the smallest at
which the per-block strong flag, the ref / ref_s select per wave, the LDS atomics and the winner's write-back can each go wrong.  At
w = 32 the blocks include the crafted strong, half-flat and threshold lines of the CPU test, a strong and a non-strong one in one
workgroup.  Guard bytes surround every output."""
import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import hevc_smoothing_cases as cases
from tests import test_gpu_mode_hads as base
from tests import util
from tests.util import PNN_E_ARG, call, dev, picture_pairs, positions, ptr, untouched

pytestmark = pytest.mark.gpu

WIDTHS = (4, 8, 16, 32, 64)
HADS_N = {4: 64 + 3, 8: 64 + 3, 16: 16 + 3, 32: 4 + 3, 64: 3}        # the SATD kernel's G + 3 (1 + 2 at w = 64)
SSE_N = {4: 64 + 3, 8: 64 + 3, 16: 16 + 3, 32: 8 + 3, 64: 4 + 3}     # the SSE search groups 64 / (w / rows per lane) blocks: its own G + 3
HOST_KEYS = base.HOST_KEYS


def hads_specs(n, w):
    return base.output_specs(n, w)


def sse_specs(n, w):
    return [(np.uint8, (n,)), (np.uint32, (n,)), (np.uint8, (n, w, w)), (np.uint32, (n, 35))]


def hads_dense(ctx, w, d_patterns, sides, d_targets, n, d_cand, smoothing, wanted=(True,) * 4, blocks=None):
    front = (ctx, w, ptr(d_patterns), sides[0], sides[1], ptr(d_targets), n, ptr(d_cand))
    specs = hads_specs(blocks if blocks is not None else n, w)
    if smoothing is None:
        return call("pnn_hevc_mode_hads_device", front, (), specs, wanted)
    return call("pnn_hevc_mode_hads_hm_device", front, (smoothing,), specs, wanted)


def sse_dense(ctx, w, d_patterns, sides, d_targets, n, smoothing, wanted=(True,) * 4, blocks=None):
    front = (ctx, w, ptr(d_patterns), sides[0], sides[1], ptr(d_targets), n)
    specs = sse_specs(blocks if blocks is not None else n, w)
    if smoothing is None:
        return call("pnn_hevc_best_mode_device", front, (), specs, wanted)
    return call("pnn_hevc_best_mode_hm_device", front, (smoothing,), specs, wanted)


def picture_front(ctx, w, planes, rows, cols, mask, shape):
    images, H, W = shape
    d_r, d_c = dev(np.asarray(rows, np.int32)), dev(np.asarray(cols, np.int32))
    return (ctx, w, ptr(planes[0]), ptr(planes[1]), images, H, W, d_r.data_ptr(), d_c.data_ptr(), len(rows), mask[0], mask[1]), (d_r, d_c)


def hads_pictures(ctx, w, planes, rows, cols, mask, d_cand, shape, smoothing, wanted=(True,) * 4, blocks=None):
    front, keep = picture_front(ctx, w, planes, rows, cols, mask, shape)
    specs = hads_specs(blocks if blocks is not None else shape[0] * len(rows), w)
    return call("pnn_first_pass_picture_pairs_hm_device", front + (ptr(d_cand),), (smoothing,), specs, wanted)


def score_specs(n, w):
    """d_targets, d_pnn_u8, d_pnn_f32, d_pnn_sse, d_hevc_mode, d_hevc_sse, d_hevc_pred"""
    return [(np.uint8, (n, w, w)), (np.uint8, (n, w, w)), (np.float32, (n, w, w)), (np.uint32, (n,)), (np.uint8, (n,)), (np.uint32, (n,)),
            (np.uint8, (n, w, w))]


HEVC_ONLY = (False, False, False, False, True, True, True)


def score_pictures(ctx, w, planes, rows, cols, mask, shape, smoothing, wanted=HEVC_ONLY, blocks=None):
    front, keep = picture_front(ctx, w, planes, rows, cols, mask, shape)
    specs = score_specs(blocks if blocks is not None else shape[0] * len(rows), w)
    return call("pnn_score_picture_pairs_hm_device", front, (smoothing,), specs, wanted)


def host_best(patterns, targets, w, smoothing):
    """(mode uint8 [n], SSE uint32 [n], prediction uint8 [n, w, w], SSE of every mode uint32 [n, 35]) by the host twin and numpy"""
    preds = np.array([[ip.predict_via_hevc_mode(np.ascontiguousarray(p[..., None]), w, m, smoothing=smoothing)[..., 0] for m in range(35)]
                      for p in patterns], np.uint8)
    sse = ((preds.astype(np.int64) - targets[:, None].astype(np.int64)) ** 2).sum(axis=(2, 3)).astype(np.uint32)
    mode = np.argmin(sse, axis=1).astype(np.uint8)                         # the first of the smallest
    rows = np.arange(len(patterns))
    assert (sse[rows, mode] < 65025 * w * w).all()                         # (the 0 dB case is not among these blocks)
    return mode, sse[rows, mode], preds[rows, mode], sse


def blocks_with_crafted_lines(w, n, sides, seed):
    """base.dense_blocks; at w = 32 the first blocks carry the crafted lines, cut to `sides` (a cut line pads its last sample)."""
    patterns, targets, candidate = base.dense_blocks(w, n, sides, seed)
    if w == 32:
        crafted = [p for _, p, _ in cases.crafted_blocks()]
        if sides[0] == w + 1 and sides[1] == w + 1:
            crafted = crafted[-1:] + crafted[:-1]                          # the masked block as it is, first
        for b, p in enumerate(crafted[:n]):
            patterns[b] = 255
            patterns[b, :, 0] = cases.padded(p, w)[:sides[0], 0]
            patterns[b, 0, :] = cases.padded(p, w)[0, :sides[1]]
    return patterns, targets, candidate


def assert_same(got, want, label):
    for k, (g, v) in enumerate(zip(got, want)):
        assert (g is None and v is None) or (g.dtype == v.dtype and g.shape == v.shape and g.tobytes() == v.tobytes()), (label, k)


@pytest.mark.parametrize("w", WIDTHS)
def test_satd_kernel_dense_form_equals_the_host_twin(w):
    n = HADS_N[w]
    ctx = ip._context(0)
    for sides in ((2 * w + 1, 2 * w + 1), (w + 1, w + 1), (w + 1, 2 * w + 1)):
        patterns, targets, candidate = blocks_with_crafted_lines(w, n, sides, 800 + w)
        d_patterns, d_targets, d_cand = dev(patterns), dev(targets), dev(candidate)
        if w == 32 and sides[0] == sides[1]:                               # a strong and a non-strong block in the first workgroup (G = 4)
            flags = [ip.smoothed_reference(p, w, 2)[1] for p in patterns[:4]]
            assert any(flags) and not all(flags), (sides, flags)
        for cand in (candidate, None):
            d_c = d_cand if cand is not None else None
            wanted = (True, cand is not None, True, True)
            rc, old, intact = hads_dense(ctx, w, d_patterns, sides, d_targets, n, d_c, None, wanted)
            assert rc == 0 and intact
            rc, zero, intact = hads_dense(ctx, w, d_patterns, sides, d_targets, n, d_c, 0, wanted)
            assert rc == 0 and intact
            assert_same(zero, old, "smoothing 0, w %d sides %s" % (w, sides))                          # 0 through the new entry: the old entry's bits
            for smoothing in (1, 2):
                label = "w %d sides %s candidate %s smoothing %d" % (w, sides, cand is not None, smoothing)
                rc, got, intact = hads_dense(ctx, w, d_patterns, sides, d_targets, n, d_c, smoothing, wanted)
                assert rc == 0 and intact, label
                host = ip.mode_hads_host(patterns, targets, w, cand, smoothing=smoothing)
                base.assert_equal_host(got, host, wanted, label)
                if w in (4, 64):
                    assert_same(got, old, label)                                                        # no mode smooths: the old entry's bits
                else:
                    assert got[0].tobytes() != old[0].tobytes(), label
                public = ip.mode_hads_device(d_patterns, d_targets, w, d_c, smoothing=smoothing)         # the Python interface
                for key in HOST_KEYS:
                    assert (public[key] is None and host[key] is None) or public[key].tobytes() == host[key].tobytes(), (label, key)


@pytest.mark.parametrize("w", WIDTHS)
def test_sse_search_dense_form_equals_the_host_twin(w):
    n = SSE_N[w]
    ctx = ip._context(0)
    for sides in ((2 * w + 1, 2 * w + 1), (w + 1, w + 1), (w + 1, 2 * w + 1)):
        patterns, targets, _ = blocks_with_crafted_lines(w, n, sides, 900 + w)
        m = n
        d_patterns, d_targets = dev(patterns), dev(targets)
        if w == 32 and sides[0] == sides[1]:                               # a strong and a non-strong block in the first workgroup (G = 8)
            flags = [ip.smoothed_reference(p, w, 2)[1] for p in patterns[:8]]
            assert any(flags) and not all(flags), (sides, flags)
        rc, old, intact = sse_dense(ctx, w, d_patterns, sides, d_targets, m, None)
        assert rc == 0 and intact
        rc, zero, intact = sse_dense(ctx, w, d_patterns, sides, d_targets, m, 0)
        assert rc == 0 and intact
        assert_same(zero, old, "smoothing 0, w %d sides %s" % (w, sides))
        for smoothing in (1, 2):
            label = "w %d sides %s smoothing %d" % (w, sides, smoothing)
            rc, got, intact = sse_dense(ctx, w, d_patterns, sides, d_targets, m, smoothing)
            assert rc == 0 and intact, label
            assert_same(got, list(host_best(patterns, targets, w, smoothing)), label)
            for b in range(m):                                             # the best prediction is the _hm predictor's of the reported mode
                want = ip.predict_via_hevc_mode(np.ascontiguousarray(patterns[b][..., None]), w, int(got[0][b]), smoothing=smoothing)[..., 0]
                assert got[2][b].tobytes() == want.tobytes(), (label, b)
            if w in (4, 64):
                assert_same(got, old, label)
            else:
                assert got[3].tobytes() != old[3].tobytes(), label
            rc, lean, intact = sse_dense(ctx, w, d_patterns, sides, d_targets, m, smoothing, wanted=(False, False, True, False))
            assert rc == 0 and intact and lean[2].tobytes() == got[2].tobytes(), label                   # the write-back alone
            index, sse, pred, all_sse = ip.best_modes_device(d_patterns, d_targets, w, mode_sse=True, smoothing=smoothing)
            public = [index.cpu().numpy(), sse.cpu().numpy().view(np.uint32), pred.cpu().numpy(), all_sse.cpu().numpy().view(np.uint32)]
            assert_same(public, got, label + " (Python)")


@pytest.mark.parametrize("w", WIDTHS)
def test_picture_and_pair_forms_equal_the_dense_form(w):
    pair = picture_pairs(2, w, 1000 + w)
    rows, cols = positions()
    n = 2 * rows.size
    ctx = ip._context(0)
    original, decoded = np.ascontiguousarray(pair[..., 0]), np.ascontiguousarray(pair[..., 1])
    d_original, d_decoded = dev(original), dev(decoded)
    rng = np.random.RandomState(w)
    for mask in ((0, 0), (4, 0), (w, w)):
        for smoothing in (1, 2) if w == 32 else (2,):
            label = "w %d mask %s smoothing %d" % (w, mask, smoothing)
            patterns, targets = base.dense_inputs_of_pictures(decoded, original, w, rows, cols, mask)
            candidate = np.clip(targets.astype(np.int64) + rng.randint(-25, 26, targets.shape), 0, 255).astype(np.uint8)
            d_cand = dev(candidate)
            host = ip.mode_hads_host(patterns, targets, w, candidate, smoothing=smoothing)
            # the first-pass ranking
            rc, dense, intact = hads_dense(ctx, w, dev(patterns), patterns.shape[1:], dev(targets), n, d_cand, smoothing)
            assert rc == 0 and intact
            base.assert_equal_host(dense, host, (True,) * 4, "dense " + label)
            rc, got, intact = hads_pictures(ctx, w, (d_decoded, d_original), rows, cols, mask, d_cand, original.shape, smoothing)
            assert rc == 0 and intact
            assert_same(got, dense, "first pass " + label)
            rc, swapped, intact = hads_pictures(ctx, w, (d_original, d_decoded), rows, cols, mask, d_cand, original.shape, smoothing)
            assert rc == 0 and intact
            p2, t2 = base.dense_inputs_of_pictures(original, decoded, w, rows, cols, mask)
            base.assert_equal_host(swapped, ip.mode_hads_host(p2, t2, w, candidate, smoothing=smoothing), (True,) * 4, "swapped " + label)
            assert swapped[0].tobytes() != got[0].tobytes()
            # the best-mode search of the score entry
            want = host_best(patterns, targets, w, smoothing)
            rc, dense, intact = sse_dense(ctx, w, dev(patterns), patterns.shape[1:], dev(targets), n, smoothing)
            assert rc == 0 and intact
            assert_same(dense, list(want), "dense search " + label)
            rc, got, intact = score_pictures(ctx, w, (d_decoded, d_original), rows, cols, mask, original.shape, smoothing)
            assert rc == 0 and intact
            assert_same(got[4:], list(want[:3]), "score " + label)
            rc, swapped, intact = score_pictures(ctx, w, (d_original, d_decoded), rows, cols, mask, original.shape, smoothing)
            assert rc == 0 and intact
            assert_same(swapped[4:], list(host_best(p2, t2, w, smoothing)[:3]), "swapped score " + label)
            assert swapped[5].tobytes() != got[5].tobytes()
            # the single-picture form: both pointers equal
            rc, single, intact = score_pictures(ctx, w, (d_decoded, d_decoded), rows, cols, mask, decoded.shape, smoothing)
            assert rc == 0 and intact
            p1, t1 = base.dense_inputs_of_pictures(decoded, decoded, w, rows, cols, mask)
            assert_same(single[4:], list(host_best(p1, t1, w, smoothing)[:3]), "single " + label)


PNN_KEYS = ('psnrs_pnn', 'mean_psnr_pnn', 'predictions_pnn_uint8', 'targets_uint8', 'hads_pnn')


@pytest.mark.parametrize("is_fc, w, pairs", [(True, 8, False), (False, 16, True), (True, 8, True)], ids=["fc8", "conv16-pairs", "fc8-pairs"])
def test_evaluator_reference_smoothing(is_fc, w, pairs):
    """reference_smoothing=2 against a yardstick of untouched code and the host twin: the default call for every PNN key, the host twin
    for the HEVC and first-pass keys, numpy for the frequencies; reference_smoothing=0 is today's call, key for key and byte for byte."""
    pair = picture_pairs(2, w, 1100 + w)
    channels = pair if pairs else np.ascontiguousarray(pair[..., 0:1])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, 0), (w, w))
    net = base.golden_net(w, is_fc, n)
    for first_pass in (True, False):
        default = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass)
        zero = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass, reference_smoothing=0)
        got = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=first_pass, reference_smoothing=2)
        lean = score(channels, w, rows, cols, net, util.MEAN, masks, keep_predictions=False, first_pass=first_pass, reference_smoothing=2)
        assert list(got) == list(masks)
        for mask in masks:
            util.assert_same_dictionary(zero[mask], default[mask], "reference_smoothing=0 %s" % (mask,))
            assert 'reference_smoothing' not in default[mask]
            assert set(got[mask]) == set(default[mask]) | {'reference_smoothing'}
            assert got[mask]['reference_smoothing'] == 2 and type(got[mask]['reference_smoothing']) is int
            assert lean[mask]['reference_smoothing'] == 2 and 'predictions_hevc_best_mode_uint8' not in lean[mask]
            for key in PNN_KEYS:                                           # the PNN's keys: bit-identical to the default call
                if key in default[mask]:
                    g, v = got[mask][key], default[mask][key]
                    assert (g.tobytes() == v.tobytes() and g.dtype == v.dtype) if isinstance(v, np.ndarray) else (type(g) is type(v) and g == v), (mask, key)
            patterns = np.ascontiguousarray(ip.extract_intra_patterns(channels[..., -1:], w, rows + w - 1, cols + w - 1, mask)[..., 0])
            targets = np.ascontiguousarray(default[mask]['targets_uint8'][..., 0])
            mode, sse, pred, _ = host_best(patterns, targets, w, 2)
            psnrs = ip.psnrs_from_sses(sse, w)
            want = {'indices_hevc_best_mode': mode, 'psnrs_hevc_best_mode': psnrs, 'predictions_hevc_best_mode_uint8': pred[..., None],
                    'frequency_win_pnn': float(np.count_nonzero(default[mask]['psnrs_pnn'] - psnrs > 0.)) / n}
            if first_pass:
                host = ip.mode_hads_host(patterns, targets, w, np.ascontiguousarray(default[mask]['predictions_pnn_uint8'][..., 0]), smoothing=2)
                want.update({'hads_hevc_modes': host['hads_modes'], 'first_pass_list': host['list_modes'], 'first_pass_costs': host['list_costs'],
                             'frequency_pnn_in_first_pass_list': float(np.mean((host['list_modes'] == 35).any(axis=1))),
                             'frequency_pnn_first_pass_best': float(np.mean(host['list_modes'][:, 0] == 35))})
                assert got[mask]['hads_hevc_modes'].tobytes() != default[mask]['hads_hevc_modes'].tobytes()
            for new in (got[mask], lean[mask]):
                for key, v in want.items():
                    if key not in new:
                        assert new is lean[mask] and key == 'predictions_hevc_best_mode_uint8'
                        continue
                    g = new[key]
                    if isinstance(v, np.ndarray):
                        assert g.dtype == v.dtype and g.shape == v.shape and g.tobytes() == v.tobytes(), (mask, key)
                    else:
                        assert type(g) is float and g == v, (mask, key)
    if not pairs:                                                          # the path through dense patterns gives the same dictionary
        for mask in masks[:2]:
            dense = evaluation.predict_mask_vs_hevc_best_mode(channels, w, rows, cols, net, n, util.MEAN, mask, reference_smoothing=2)
            reference = score(channels, w, rows, cols, net, util.MEAN, (mask,), reference_smoothing=2)[mask]
            util.assert_same_dictionary(dense, reference, "dense path %s" % (mask,))
            plain = evaluation.predict_mask_vs_hevc_best_mode(channels, w, rows, cols, net, n, util.MEAN, mask)
            assert 'reference_smoothing' not in plain
    net.close()


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    w, mask = 8, (0, 0)
    pair = picture_pairs(2, w, 1200)
    rows, cols = positions()
    images, H, W = pair.shape[:3]
    ctx = ip._context(0)
    d_context, d_target = dev(pair[..., 1]), dev(pair[..., 0])
    d_cand = dev(np.zeros((6, w, w), np.uint8))

    def first_pass_refused(planes=(d_context, d_target), rows=rows, cols=cols, shape=(images, H, W), mask=mask, wanted=(True,) * 4, w=w, cand=d_cand,
                           smoothing=2, ctx=ctx):
        rc, got, intact = hads_pictures(ctx, w, planes, rows, cols, mask, cand, shape, smoothing, wanted=wanted, blocks=6)
        return rc == PNN_E_ARG and intact and untouched(got) and (ctx is None or bool(L.pnn_last_error(ctx)))

    def score_refused(planes=(d_context, d_target), rows=rows, cols=cols, shape=(images, H, W), mask=mask, wanted=HEVC_ONLY, w=w, smoothing=2, ctx=ctx):
        rc, got, intact = score_pictures(ctx, w, planes, rows, cols, mask, shape, smoothing, wanted=wanted, blocks=6)
        return rc == PNN_E_ARG and intact and untouched(got) and (ctx is None or bool(L.pnn_last_error(ctx)))

    for refused in (first_pass_refused, score_refused):
        assert refused(smoothing=-1) and refused(smoothing=3)
        assert b"smoothing" in L.pnn_last_error(ctx)
        assert refused(planes=(None, d_target)) and refused(planes=(d_context, None)) and refused(planes=(None, None))
        assert refused(planes=(None, d_target), shape=(0, H, W))
        assert refused(rows=[0, 6, 2]) and refused(cols=[0, 10, 5]) and refused(rows=[0, -1, 2]) and refused(cols=[-1, 9, 5])
        assert refused(shape=(images, H - 1, W)) and refused(shape=(images, H, W - 1))
        assert refused(mask=(12, 0)) and refused(mask=(0, 2)) and refused(w=12) and refused(wanted=(False,) * (4 if refused is first_pass_refused else 7))
        assert refused(ctx=None)
    assert first_pass_refused(cand=None) and first_pass_refused(cand=None, wanted=(False, True, False, False))
    assert score_refused(wanted=(False, True, False, False, True, True, True))             # a PNN output without a model on the context
    for shape, r, c in (((0, H, W), rows, cols), ((images, H, W), rows[:0], cols[:0])):     # n == 0 does nothing
        rc, got, intact = hads_pictures(ctx, w, (d_context, d_target), r, c, mask, d_cand, shape, 2, blocks=6)
        assert rc == 0 and intact and untouched(got)
        rc, got, intact = score_pictures(ctx, w, (d_context, d_target), r, c, mask, shape, 2, blocks=6)
        assert rc == 0 and intact and untouched(got)
    rc, got, intact = hads_pictures(ctx, w, (d_context, d_target), rows, cols, mask, d_cand, (images, H, W), 2)
    assert rc == 0 and intact
    rc, got, intact = score_pictures(ctx, w, (d_context, d_target), rows, cols, mask, (images, H, W), 2)
    assert rc == 0 and intact

    # the dense entries
    n = 5
    full = (2 * w + 1, 2 * w + 1)
    patterns, targets, candidate = base.dense_blocks(w, n, full, 1250)
    d_patterns, d_targets, d_cand = dev(patterns), dev(targets), dev(candidate)

    def hads_refused(ctx=ctx, w=w, patterns=d_patterns, sides=full, targets=d_targets, n=n, cand=d_cand, wanted=(True,) * 4, smoothing=2):
        rc, got, intact = hads_dense(ctx, w, patterns, sides, targets, n, cand, smoothing, wanted=wanted, blocks=5)
        return rc == PNN_E_ARG and intact and untouched(got)

    def sse_refused(ctx=ctx, w=w, patterns=d_patterns, sides=full, targets=d_targets, n=n, wanted=(True,) * 4, smoothing=2):
        rc, got, intact = sse_dense(ctx, w, patterns, sides, targets, n, smoothing, wanted=wanted, blocks=5)
        return rc == PNN_E_ARG and intact and untouched(got)

    for refused in (hads_refused, sse_refused):
        assert refused(smoothing=-1) and refused(smoothing=3)
        assert b"smoothing" in L.pnn_last_error(ctx)
        assert refused(w=12) and refused(sides=(w, 2 * w + 1)) and refused(sides=(2 * w + 1, 2 * w + 2))
        assert refused(n=-1) and refused(patterns=None) and refused(targets=None) and refused(wanted=(False,) * 4) and refused(ctx=None)
    assert hads_refused(cand=None)
    rc, got, intact = hads_dense(ctx, w, d_patterns, full, d_targets, 0, d_cand, 2, blocks=5)
    assert rc == 0 and intact and untouched(got)
    rc, got, intact = sse_dense(ctx, w, d_patterns, full, d_targets, 0, 2, blocks=5)
    assert rc == 0 and intact and untouched(got)
    rc, got, intact = hads_dense(ctx, w, d_patterns, full, d_targets, n, d_cand, 2)
    assert rc == 0 and intact
    rc, got, intact = sse_dense(ctx, w, d_patterns, full, d_targets, n, 2)
    assert rc == 0 and intact
    with pytest.raises(ValueError):
        ip.mode_hads_device(d_patterns, d_targets, w, smoothing=3)
    with pytest.raises(ValueError):
        ip.best_modes_device(d_patterns, d_targets, w, smoothing=-1)
