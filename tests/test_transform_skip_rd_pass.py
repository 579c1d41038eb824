"""CPU tests of transform skip in the second intra pass (include/pnn_hip.h, "transform skip"): pnn_rd_pass_tskip_host
behind intraprediction.rd_pass(transform_skip=True) against a composition written here -- the slots the pass without the option reports,
each coded by pnn_trquant_tskip_host in 'decide' mode under the slot's mode bits (tests/mode_signal_cases.py's restatement), then J = D +
lambda ((side + R) >> 15) and the first minimum in slot order -- for both codecs; the option off byte for byte; the batch entry tied to
the HM-pinned unit entry; the conditions on the winners with the shares written down; the refusals."""
import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import mode_signal_cases as signal
from tests import transform_skip_cases as tc
from tests.util import assert_same_dictionary

W, N = 4, 129


def seeded(codec):
    """the blocks of mode_signal_cases at width 4; half of the candidates (the PNN's predictions) replaced by ones that leave a
    two-valued or single-edge residual, as transform_skip_cases.blocks makes them"""
    patterns, targets, candidates = signal.blocks(W, N)
    rng = np.random.RandomState(4413)                    # (4411 and 4412 left one cell below 5 %: found on the CPU)
    for b in range(1, N, 2):
        a = int(rng.choice((12, 25, 60, 120)))
        residual = np.where(rng.randint(2, size=(4, 4)) == 1, a, 0) if rng.randint(2) else np.pad(np.full((4, rng.randint(1, 4)), a), ((0, 0), (0, 0)))
        full = np.zeros((4, 4), np.int64)
        full[:, :residual.shape[1]] = residual
        candidates[b] = np.clip(targets[b].astype(np.int64) - full * (1 if rng.randint(2) else -1), 0, 255)
    left, above = signal.neighbours(W, N)
    if codec == 'substitution':
        left, above = (np.where(a == 35, 255, a).astype(np.uint8) for a in (left, above))
    return patterns, targets, candidates, left, above


def composed(patterns, targets, candidates, left, above, qps, codec, off, sdh, rdoq):
    """The winners with the option on, from the option-off pass's slots: every slot coded in both forms and decided, then compared"""
    n, nq = len(targets), len(qps)
    s = off['candidates'].shape[2]
    pnn_mode = 35 if codec == 'switch' else 18
    out = {k: np.zeros((nq, n), off[k].dtype) for k in ('modes', 'slots', 'best_costs', 'sses', 'rates', 'side_rates')}
    out['best_transform_skip'] = np.zeros((nq, n), np.uint8)
    out['costs'] = np.full((nq, n, s), np.inf)
    for qi, qp in enumerate(qps):
        lam = float(off['lambdas'][qi])
        cbf = tc.cbf_bins(qp)
        pred, tgt, modes, bits = [], [], [], []
        for b in range(n):
            mpm = signal.mpm_of(int(left[b]), int(above[b]))[0]
            for j in range(s):
                m = int(off['candidates'][qi, b, j])
                tgt.append(targets[b])
                pred.append(candidates[b] if m == pnn_mode else targets[b] if m == 255 else
                            ip.predict_via_hevc_mode(patterns[b][..., None], W, m, smoothing=2)[..., 0])
                modes.append(0 if m > 34 else m)
                bits.append(0 if m == 255 else signal.mode_bits(m, mpm, qp, pnn_flag=codec == 'switch'))
        rc, outs = tc.host_entry(np.ascontiguousarray(np.array(pred, np.uint8)), np.ascontiguousarray(np.array(tgt, np.uint8)),
                                 np.array(modes, np.uint8), (qp,), sdh, rdoq, [lam], 2, np.array(bits, np.uint32).reshape(1, -1), 1)
        assert rc == 0
        sse, nonzero, rate, flags = (outs[i][0].reshape(n, s) for i in (0, 1, 4, 5))
        for b in range(n):
            best = np.inf
            for j in range(s):
                m = int(off['candidates'][qi, b, j])
                if m == 255:
                    continue
                side = bits[b * s + j] + cbf[1 if nonzero[b, j] else 0]
                cost = float(sse[b, j]) + lam * float((side + int(rate[b, j])) >> 15)
                out['costs'][qi, b, j] = cost
                if cost < best:
                    best = cost
                    for key, value in (('modes', m), ('slots', j), ('best_costs', cost), ('sses', sse[b, j]), ('rates', rate[b, j]),
                                       ('side_rates', side), ('best_transform_skip', flags[b, j])):
                        out[key][qi, b] = value
    return out


@pytest.mark.parametrize("codec", ('switch', 'substitution'))
@pytest.mark.parametrize("sdh,rdoq", ((0, 0), (1, 1)))
def test_host_twin_against_the_composition_and_the_option_off(codec, sdh, rdoq):
    patterns, targets, candidates, left, above = seeded(codec)
    qps = (22, 37)
    kwargs = dict(reference_smoothing=2, sign_data_hiding=bool(sdh), rdoq=bool(rdoq), signalling=True, neighbour_modes=(left, above), codec=codec)
    off = ip.rd_pass(patterns, targets, candidates, qps, **kwargs)
    again = ip.rd_pass(patterns, targets, candidates, qps, transform_skip=False, **kwargs)
    assert_same_dictionary(again, off, "transform_skip=False")                       # the option off: no key and no byte differs
    on = ip.rd_pass(patterns, targets, candidates, qps, transform_skip=True, **kwargs)
    assert set(on) == set(off) | {'best_transform_skip'}
    assert np.array_equal(on['candidates'], off['candidates']) and on['first_pass_costs'].tobytes() == off['first_pass_costs'].tobytes()
    want = composed(patterns, targets, candidates, left, above, qps, codec, off, sdh, rdoq)
    for key, value in want.items():
        assert on[key].tobytes() == value.astype(on[key].dtype).tobytes(), (key, int((on[key] != value).sum()))
    # the conditions, each on at least 5 % of the (QP, block) winners: the winner changes against the option off; the PNN's slot wins
    # skipped.  Shares found
    pnn_mode = 35 if codec == 'switch' else 18
    shares = {"winner changes": float((on['slots'] != off['slots']).mean()),
              "PNN wins skipped": float(((on['modes'] == pnn_mode) & (on['best_transform_skip'] == 1)).mean())}
    print(codec, sdh, rdoq, shares)
    for name, share in shares.items():
        assert share >= 0.05, (name, share)
    one = ip.rd_pass(patterns[:1], targets[:1], candidates[:1], qps, transform_skip=True, **dict(kwargs, neighbour_modes=(left[:1], above[:1])))
    for key in want:
        assert one[key].tobytes() == on[key][:, :1].tobytes(), key


def test_the_batch_entry_agrees_with_the_hm_pinned_unit_entry():
    """pnn_trquant_tskip_host, forced, against pnn_tskip_unit_host per unit: levels' count, uiAbsSum, the bits with the flag and the
    reconstruction, under RDOQ and the hiding and HM's lambda -- ties the batch entry's cbf context and lambda to the unit entry's."""
    import ctypes
    predictions, targets, modes = tc.blocks(60)
    for sdh, rdoq in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for qp in (0, 22, 37, 51):
            rc, outs = tc.host_entry(predictions, targets, modes, (qp,), sdh, rdoq, None, 1, None, 1)
            assert rc == 0
            for b in range(len(predictions)):
                residual = np.ascontiguousarray(targets[b].astype(np.int32) - predictions[b].astype(np.int32))
                levels, back = np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int32)
                abs_sum, bits = ctypes.c_int32(-1), np.zeros(1, np.uint64)
                assert _lib.lib().pnn_tskip_unit_host(residual.ctypes.data, tc.scan_of_mode(int(modes[b])), qp, sdh, rdoq, ip.hm_intra_lambda(qp), 1, None,
                                                      levels.ctypes.data, ctypes.byref(abs_sum), back.ctypes.data, bits.ctypes.data, None) == 0
                recon = np.clip(predictions[b].astype(np.int32) + back, 0, 255)
                assert outs[1][0, b] == (levels != 0).sum() and outs[2][0, b] == abs_sum.value and outs[4][0, b] == bits[0]
                assert np.array_equal(outs[3][0, b], recon)


def test_option_conflicts_are_value_errors():
    patterns, targets, candidates, left, above = seeded('switch')
    with pytest.raises(ValueError):
        ip.rd_pass(patterns, targets, candidates, (22,), transform_skip=True)                                  # without signalling
    with pytest.raises(ValueError):
        ip.rd_pass(patterns, targets, candidates, (22,), signalling=True, transform_skip=True, lambdas=[0.])   # a lambda of 0
    p8, t8, c8 = signal.blocks(8, 3)
    with pytest.raises(ValueError):
        ip.rd_pass(p8, t8, c8, (22,), signalling=True, transform_skip=True)                                    # width 8
    L = _lib.lib()
    assert L.pnn_rd_pass_tskip_workspace_bytes(8, 10, 2, 1, 0, 1) == 0
    assert L.pnn_rd_pass_tskip_workspace_bytes(4, 10, 2, 1, 0, 0) == L.pnn_rd_pass_codec_workspace_bytes(4, 10, 2, 1, 0)
    assert L.pnn_rd_pass_tskip_workspace_bytes(4, 10, 2, 1, 1, 1) > L.pnn_rd_pass_codec_workspace_bytes(4, 10, 2, 1, 1)


def test_the_evaluator_refuses_option_conflicts_before_anything_touches_the_gpu():
    from context_adaptive_neural_network_based_prediction_amd import evaluation
    rows = cols = np.zeros(1, np.int64)
    four, eight = np.zeros((1, 17, 21, 1), np.uint8), np.zeros((1, 29, 33, 1), np.uint8)
    for score in (evaluation.score_masks_from_pictures, evaluation.score_masks_from_picture_pairs):
        with pytest.raises(ValueError, match="rd_pass_transform_skip"):                   # without rd_pass_signalling
            score(four, 4, rows, cols, None, 0., [(0, 0)], first_pass=True, transform_qps=(22,), rd_pass=True, rd_pass_transform_skip=True)
        with pytest.raises(ValueError, match="width other than 4"):
            score(eight, 8, rows, cols, None, 0., [(0, 0)], first_pass=True, transform_qps=(22,), rd_pass=True, rd_pass_signalling=True,
                  rd_pass_transform_skip=True)
        with pytest.raises(ValueError, match="width other than 4"):
            score(eight, 8, rows, cols, None, 0., [(0, 0)], transform_qps=(22,), transform_skip='decide')
        with pytest.raises(ValueError, match="transform_skip"):
            score(four, 4, rows, cols, None, 0., [(0, 0)], transform_qps=(22,), transform_skip='on')
        with pytest.raises(ValueError, match="transform_qps"):
            score(four, 4, rows, cols, None, 0., [(0, 0)], transform_skip='forced')
