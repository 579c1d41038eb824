"""GPU tests of the first-pass ranking: hevc_mode_hads_kernel behind pnn_hevc_mode_hads_device (dense patterns) and
pnn_first_pass_picture_pairs_device (the evaluator's pictures and pairs), and the evaluator's first_pass=True keys.

Every comparison has zero tolerance, against the host twin pnn_hevc_mode_hads_host (tests/test_mode_hads.py pins it to independent
code): the costs are integers, exact in any order.  The dense shapes cross one workgroup boundary with a ragged last group (a
workgroup takes 64, 64, 16, 4, 1 blocks at w = 4 .. 64): the smallest at which the sub-block-to-lane mapping, the LDS atomics
(w >= 16), the one-block workgroup (w = 64) and the tie rule can each go wrong."""
import itertools
import os

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import util
from tests.util import PNN_E_ARG, call, dev, picture_pairs, positions, ptr, untouched

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DENSE_N = {4: 64 + 3, 8: 64 + 3, 16: 16 + 3, 32: 4 + 3, 64: 3}
OUTPUTS = ("mode_hads", "cand_hads", "list_modes", "list_costs")
HOST_KEYS = ("hads_modes", "hads_candidate", "list_modes", "list_costs")


def dense_blocks(w, n, sides, seed):
    """n blocks with pattern sides `sides` = (height, width): seeded random ones, block 1 from a constant picture (all ties), block
    2 from a horizontal ramp (many equal costs across neighbouring angles); a candidate near the target, exact for the constant block."""
    rng = np.random.RandomState(seed)
    imgs = rng.randint(0, 256, (n, 3 * w, 3 * w)).astype(np.uint8)
    imgs[1] = 97
    imgs[2] = np.tile(np.linspace(10, 240, 3 * w).astype(np.uint8), (3 * w, 1))
    mask = (2 * w + 1 - sides[1], 2 * w + 1 - sides[0])
    at = np.array([w - 1], np.int64)
    patterns = ip.extract_intra_patterns(imgs[..., None], w, at, at, mask)[..., 0]
    patterns[:, 1:, 1:] = rng.randint(0, 256, patterns[:, 1:, 1:].shape)       # the inside of a dense pattern is never read
    targets = np.ascontiguousarray(imgs[:, w:2 * w, w:2 * w])
    candidate = np.clip(targets.astype(np.int64) + rng.randint(-25, 26, targets.shape), 0, 255).astype(np.uint8)
    candidate[1] = targets[1]
    assert patterns.shape == (n,) + tuple(sides)
    return np.ascontiguousarray(patterns), targets, candidate


def output_specs(n, w):
    k = 8 if w <= 8 else 3                          # (also for the widths the entries refuse)
    return [(np.uint32, (n, 35)), (np.uint32, (n,)), (np.uint8, (n, k)), (np.uint32, (n, k))]


def dense_call(ctx, w, d_patterns, sides, d_targets, n, d_cand, wanted=(True,) * 4, blocks=None):
    """Raw call of pnn_hevc_mode_hads_device, every output between guard bytes: (rc, the four outputs or None, guards intact)."""
    front = (ctx, w, ptr(d_patterns), sides[0], sides[1], ptr(d_targets), n, ptr(d_cand))
    return call("pnn_hevc_mode_hads_device", front, (), output_specs(blocks if blocks is not None else n, w), wanted)


def picture_call(ctx, w, planes, rows, cols, mask, d_cand, shape, wanted=(True,) * 4, blocks=None):
    """Raw call of pnn_first_pass_picture_pairs_device; `planes` = (context, target) device tensors or None."""
    images, H, W = shape
    n = blocks if blocks is not None else images * len(rows)
    d_r, d_c = dev(np.asarray(rows, np.int32)), dev(np.asarray(cols, np.int32))
    front = (ctx, w, ptr(planes[0]), ptr(planes[1]), images, H, W, d_r.data_ptr(), d_c.data_ptr(), len(rows), mask[0], mask[1], ptr(d_cand))
    return call("pnn_first_pass_picture_pairs_device", front, (), output_specs(n, w), wanted)


def assert_equal_host(got, host, wanted, label):
    for k, want in enumerate(wanted):
        if want:
            ref = host[HOST_KEYS[k]]
            assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, (label, OUTPUTS[k])
            assert got[k].tobytes() == ref.tobytes(), "%s %s: %d differing values" % (label, OUTPUTS[k], (got[k] != ref).sum())


@pytest.mark.parametrize("w", sorted(DENSE_N))
def test_dense_form_equals_the_host_twin(w):
    n = DENSE_N[w]
    ctx = ip._context(0)
    for sides in ((2 * w + 1, 2 * w + 1), (w + 1, w + 1), (w + 1, 2 * w + 1)):
        patterns, targets, candidate = dense_blocks(w, n, sides, 500 + w)
        d_patterns, d_targets, d_cand = dev(patterns), dev(targets), dev(candidate)
        for cand in (candidate, None):
            host = ip.mode_hads_host(patterns, targets, w, cand)
            if cand is not None:                                     # the constant block: all ties, the candidate (cost 0 too) stays out
                k = ip.first_pass_list_size(w)
                assert host['list_modes'][1].tolist() == list(range(k)) and not host['hads_modes'][1].any()
                assert (host['list_modes'] == 35).any()              # ... and elsewhere it is in the list
            full = sides == (2 * w + 1, 2 * w + 1)
            combos = [c for c in itertools.product((True, False), repeat=4) if any(c) and (cand is not None or not c[1])]
            for wanted in combos if full else combos[:1]:            # every legal combination of NULL outputs
                rc, got, intact = dense_call(ctx, w, d_patterns, sides, d_targets, n, d_cand if cand is not None else None, wanted=wanted)
                assert rc == 0 and intact, (w, sides, wanted)
                assert_equal_host(got, host, wanted, "w %d sides %s candidate %s outputs %s" % (w, sides, cand is not None, wanted))
            # the Python interface
            got = ip.mode_hads_device(d_patterns, d_targets, w, d_cand if cand is not None else None)
            for key in HOST_KEYS:
                assert (got[key] is None and host[key] is None) or got[key].tobytes() == host[key].tobytes(), (w, sides, key)


def dense_inputs_of_pictures(context_plane, target_plane, w, rows, cols, mask):
    patterns = ip.extract_intra_patterns(context_plane[..., None], w, rows + w - 1, cols + w - 1, mask)[..., 0]
    targets = np.stack([target_plane[i, r + w:r + 2 * w, c + w:c + 2 * w] for i in range(target_plane.shape[0]) for r, c in zip(rows, cols)])
    return np.ascontiguousarray(patterns), np.ascontiguousarray(targets)


@pytest.mark.parametrize("w", sorted(DENSE_N))
def test_picture_form_equals_the_dense_form(w):
    pair = picture_pairs(2, w, 600 + w)
    rows, cols = positions()
    n = 2 * rows.size
    ctx = ip._context(0)
    original, decoded = np.ascontiguousarray(pair[..., 0]), np.ascontiguousarray(pair[..., 1])
    d_original, d_decoded = dev(original), dev(decoded)
    rng = np.random.RandomState(w)
    for mask in ((0, 0), (4, 0), (w, w)):
        patterns, targets = dense_inputs_of_pictures(decoded, original, w, rows, cols, mask)
        candidate = np.clip(targets.astype(np.int64) + rng.randint(-25, 26, targets.shape), 0, 255).astype(np.uint8)
        d_cand = dev(candidate)
        rc, dense, intact = dense_call(ctx, w, dev(patterns), patterns.shape[1:], dev(targets), n, d_cand)
        assert rc == 0 and intact
        host = ip.mode_hads_host(patterns, targets, w, candidate)
        assert_equal_host(dense, host, (True,) * 4, "dense w %d mask %s" % (w, mask))
        rc, got, intact = picture_call(ctx, w, (d_decoded, d_original), rows, cols, mask, d_cand, original.shape)
        assert rc == 0 and intact
        for k in range(4):
            assert got[k].tobytes() == dense[k].tobytes(), "w %d mask %s %s" % (w, mask, OUTPUTS[k])
        # the planes are not interchangeable: swapped, the costs are those of the swapped dense inputs, and they differ
        rc, swapped, intact = picture_call(ctx, w, (d_original, d_decoded), rows, cols, mask, d_cand, original.shape)
        assert rc == 0 and intact
        p2, t2 = dense_inputs_of_pictures(original, decoded, w, rows, cols, mask)
        assert_equal_host(swapped, ip.mode_hads_host(p2, t2, w, candidate), (True,) * 4, "swapped w %d mask %s" % (w, mask))
        assert swapped[0].tobytes() != got[0].tobytes()
    # both pointers equal: the bits of the two-plane call on identical planes, and of the dense form on that one plane
    mask = (4, 0)
    patterns, targets = dense_inputs_of_pictures(decoded, decoded, w, rows, cols, mask)
    rc, single, intact = picture_call(ctx, w, (d_decoded, d_decoded), rows, cols, mask, None, decoded.shape, wanted=(True, False, True, True))
    assert rc == 0 and intact
    rc, copies, intact = picture_call(ctx, w, (d_decoded, dev(decoded)), rows, cols, mask, None, decoded.shape, wanted=(True, False, True, True))
    assert rc == 0 and intact
    host = ip.mode_hads_host(patterns, targets, w)
    for k in (0, 2, 3):
        assert single[k].tobytes() == copies[k].tobytes() == host[HOST_KEYS[k]].tobytes(), OUTPUTS[k]


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    w, mask = 8, (0, 0)
    pair = picture_pairs(2, w, 640)
    rows, cols = positions()
    images, H, W = pair.shape[:3]
    ctx = ip._context(0)
    d_context, d_target = dev(pair[..., 1]), dev(pair[..., 0])
    d_cand = dev(np.zeros((6, w, w), np.uint8))

    def refused(planes=(d_context, d_target), rows=rows, cols=cols, shape=(images, H, W), mask=mask, wanted=(True,) * 4, w=w, cand=d_cand):
        rc, got, intact = picture_call(ctx, w, planes, rows, cols, mask, cand, shape, wanted=wanted, blocks=6)
        return rc == PNN_E_ARG and intact and untouched(got) and bool(L.pnn_last_error(ctx))

    assert refused(planes=(None, d_target)) and refused(planes=(d_context, None))                  # exactly one plane
    assert refused(planes=(None, d_target), shape=(0, H, W))                                          # ... also of an empty call
    assert refused(planes=(None, None))                                                               # no plane at all, n > 0
    assert refused(rows=[0, 6, 2]) and refused(cols=[0, 10, 5]) and refused(rows=[0, -1, 2]) and refused(cols=[-1, 9, 5])
    assert refused(shape=(images, H - 1, W)) and refused(shape=(images, H, W - 1))                  # the far context leaves the picture
    assert refused(mask=(12, 0)) and refused(mask=(0, 2)) and refused(w=12) and refused(wanted=(False,) * 4)
    assert refused(cand=None) and refused(cand=None, wanted=(False, True, False, False))              # d_cand_hads needs d_cand_pred
    rc, got, intact = picture_call(None, w, (d_context, d_target), rows, cols, mask, d_cand, (images, H, W))
    assert rc == PNN_E_ARG and intact and untouched(got)                                              # no context
    # n == 0 (no image, no position) does nothing, with real buffers
    rc, got, intact = picture_call(ctx, w, (d_context, d_target), rows, cols, mask, d_cand, (0, H, W), blocks=6)
    assert rc == 0 and intact and untouched(got)
    rc, got, intact = picture_call(ctx, w, (d_context, d_target), rows[:0], cols[:0], mask, d_cand, (images, H, W), blocks=6)
    assert rc == 0 and intact and untouched(got)
    # the same call with good arguments goes through
    rc, got, intact = picture_call(ctx, w, (d_context, d_target), rows, cols, mask, d_cand, (images, H, W))
    assert rc == 0 and intact

    # the dense entry
    n = 5
    patterns, targets, candidate = dense_blocks(w, n, (2 * w + 1, 2 * w + 1), 650)
    d_patterns, d_targets, d_cand = dev(patterns), dev(targets), dev(candidate)

    def dense_refused(ctx=ctx, w=w, patterns=d_patterns, sides=(2 * w + 1, 2 * w + 1), targets=d_targets, n=n, cand=d_cand, wanted=(True,) * 4):
        rc, got, intact = dense_call(ctx, w, patterns, sides, targets, n, cand, wanted=wanted, blocks=5)
        return rc == PNN_E_ARG and intact and untouched(got)

    assert dense_refused(w=12) and dense_refused(sides=(w, 2 * w + 1)) and dense_refused(sides=(2 * w + 1, 2 * w + 2))
    assert dense_refused(n=-1) and dense_refused(patterns=None) and dense_refused(targets=None) and dense_refused(wanted=(False,) * 4)
    assert dense_refused(cand=None) and dense_refused(ctx=None)
    rc, got, intact = dense_call(ctx, w, d_patterns, (2 * w + 1, 2 * w + 1), d_targets, 0, d_cand, blocks=5)
    assert rc == 0 and intact and untouched(got)
    rc, got, intact = dense_call(ctx, w, d_patterns, (2 * w + 1, 2 * w + 1), d_targets, n, d_cand)
    assert rc == 0 and intact


def golden_net(w, is_fc, batch):
    """The seeded net of tests/golden/nets.npz for this architecture (tests/test_gpu_parity.py::test_golden_nets pins its output)."""
    import context_adaptive_neural_network_based_prediction_amd as P
    g = np.load(os.path.join(GOLD, "nets.npz"))
    seed = int(g["%s%d_seed" % ("fc" if is_fc else "conv", w)])
    return P.PredictionNeuralNetwork(batch, w, is_fc, params=util.make_params(w, is_fc, seed, out_gain=util.out_gain(w, is_fc)))


NEW_KEYS = ('hads_pnn', 'hads_hevc_modes', 'first_pass_list', 'first_pass_costs', 'frequency_pnn_in_first_pass_list',
            'frequency_pnn_first_pass_best')


@pytest.mark.parametrize("is_fc, w, pairs", [(True, 8, False), (False, 16, True), (True, 8, True)], ids=["fc8", "conv16-pairs", "fc8-pairs"])
def test_evaluator_first_pass_keys(is_fc, w, pairs):
    """The new keys against a yardstick of untouched code: the first_pass=False call for the uint8 PNN predictions and the targets,
    the host twin for costs and list, numpy for the two frequencies; every other key bit-identical to the first_pass=False call."""
    pair = picture_pairs(2, w, 700 + w)
    channels = pair if pairs else np.ascontiguousarray(pair[..., 0:1])
    score = evaluation.score_masks_from_picture_pairs if pairs else evaluation.score_masks_from_pictures
    rows, cols = positions()
    n = 2 * rows.size
    masks = ((0, 0), (4, 0), (w, w))
    net = golden_net(w, is_fc, n)
    base = score(channels, w, rows, cols, net, util.MEAN, masks)
    got = score(channels, w, rows, cols, net, util.MEAN, masks, first_pass=True)
    lean = score(channels, w, rows, cols, net, util.MEAN, masks, keep_predictions=False, first_pass=True)
    lean_base = score(channels, w, rows, cols, net, util.MEAN, masks, keep_predictions=False)
    assert list(got) == list(masks)
    k = ip.first_pass_list_size(w)
    for mask in masks:
        assert set(got[mask]) == set(base[mask]) | set(NEW_KEYS) and set(lean[mask]) == set(lean_base[mask]) | set(NEW_KEYS)
        for old, new in ((base[mask], got[mask]), (lean_base[mask], lean[mask])):
            for key, v in old.items():                               # every pre-existing key: the same bits
                g = new[key]
                if isinstance(v, np.ndarray):
                    assert g.dtype == v.dtype and g.shape == v.shape and g.tobytes() == v.tobytes(), (mask, key)
                else:
                    assert type(g) is type(v) and g == v, (mask, key)
        patterns = ip.extract_intra_patterns(channels[..., -1:], w, rows + w - 1, cols + w - 1, mask)[..., 0]
        host = ip.mode_hads_host(np.ascontiguousarray(patterns), np.ascontiguousarray(base[mask]['targets_uint8'][..., 0]), w,
                                 np.ascontiguousarray(base[mask]['predictions_pnn_uint8'][..., 0]))
        want = {'hads_pnn': host['hads_candidate'], 'hads_hevc_modes': host['hads_modes'], 'first_pass_list': host['list_modes'],
                'first_pass_costs': host['list_costs'],
                'frequency_pnn_in_first_pass_list': float(np.mean((host['list_modes'] == 35).any(axis=1))),
                'frequency_pnn_first_pass_best': float(np.mean(host['list_modes'][:, 0] == 35))}
        assert want['first_pass_list'].shape == (n, k)
        for new in (got[mask], lean[mask]):
            for key, v in want.items():
                g = new[key]
                if isinstance(v, np.ndarray):
                    assert g.dtype == v.dtype and g.shape == v.shape and g.tobytes() == v.tobytes(), (mask, key)
                else:
                    assert type(g) is float and g == v, (mask, key)
    net.close()
