"""CPU tests of the substitution codec's intra search as a column (include/pnn_hip.h, "the substitution codec") and
of the mode statistics: the host twin pnn_rd_pass_codec_host and the first-pass entry pnn_first_pass_codec_host against the Python
restatement of tests/substitution_cases.py, doubles by bit pattern; known answers derived here; the side bits against HM's own records
(tests/golden/hm_mode_signal.npz, the regular tree, whose getIntraDirPredictor and codeIntraDirLumaAng the substitution tree keeps);
codec 0 as the entries it forwards to; the conditions on the seeded cases; pnn_rd_pass_mode_stats_host against numpy.bincount; the
refusals; a sanitizer build of the host entries."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import mode_signal_cases as signal
from tests import rd_pass_cases
from tests import substitution_cases as cases

NAMES = tuple(name for name, _ in ip.RD_PASS_SIGNAL_OUTPUTS)
SUB = dict(signalling=True, codec='substitution')


def same_bits(got, want, label):
    for name in NAMES + ('rate_bits', 'side_rate_bits', 'lambdas'):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape, (label, name, a.shape, b.shape)
        assert a.astype(b.dtype).tobytes() == b.tobytes(), "%s %s: %d differing values" % (label, name, (a != b).sum())


def first_pass_codec(patterns, targets, candidates, qps, left, above, smoothing=0, lambdas=None, codec=1):
    n, w, nq = targets.shape[0], targets.shape[1], len(qps)
    k, s = ip.first_pass_list_size(w), ip.rd_pass_slot_count(w, True, 'substitution' if codec else 'switch')
    modes, costs, slots = np.zeros((nq, n, k), np.uint8), np.zeros((nq, n, k)), np.zeros((nq, n, s), np.uint8)
    c_lambdas = None if lambdas is None else (ctypes.c_double * nq)(*lambdas)
    rc = _lib.lib().pnn_first_pass_codec_host(patterns.ctypes.data, patterns.shape[1], patterns.shape[2], targets.ctypes.data, w, n,
                                              candidates.ctypes.data, smoothing, (ctypes.c_int * nq)(*qps), nq, c_lambdas, left.ctypes.data,
                                              above.ctypes.data, codec, modes.ctypes.data, costs.ctypes.data, slots.ctypes.data)
    assert rc == 0
    return modes, costs, slots


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_host_twin_equals_restatement(w):
    """n = max(2 G + 1, 25) and n = 1; QPs 22 / 37 and 0 / 51; smoothing 0 and 2; RDOQ off and -- to w = 16 -- on; sign hiding off and on."""
    n = cases.CONDITION_BLOCKS[w]
    patterns, targets, candidates = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    assert ip.rd_pass_slot_count(w, True, 'substitution') == ip.first_pass_list_size(w) + 2
    for qps, smoothing, rdoq, hiding in ((cases.QP_PAIRS[0], 0, False, False), (cases.QP_PAIRS[1], 2, False, True),
                                         (cases.QP_PAIRS[0], 2, True, True), (cases.QP_PAIRS[1], 0, True, False)):
        if rdoq and w > 16:
            continue
        label = "w %d qps %s smoothing %d rdoq %s hiding %s" % (w, qps, smoothing, rdoq, hiding)
        got = ip.rd_pass(patterns, targets, candidates, qps, smoothing, sign_data_hiding=hiding, rdoq=rdoq, neighbour_modes=(left, above), **SUB)
        want = cases.restatement(patterns, targets, candidates, qps, left, above, smoothing, sign_data_hiding=hiding, rdoq=rdoq)
        same_bits(got, want, label)
        assert not (got['candidates'] == 35).any() and not (got['modes'] == 35).any(), label
        # the first-pass entry: the list, its costs and the slots
        first = ip.mode_hads_host(patterns, targets, w, candidates, smoothing=smoothing)
        modes, costs, slots = first_pass_codec(patterns, targets, candidates, qps, left, above, smoothing)
        for qi, qp in enumerate(qps):
            v = cases.first_pass(first['hads_modes'], first['hads_candidate'], left, above, qp, ip.hm_intra_lambda(qp), modes.shape[2])
            for a, b in zip((modes[qi], costs[qi], slots[qi]), v):
                assert a.tobytes() == b.tobytes(), label
            assert costs[qi].tobytes() == got['first_pass_costs'][qi].tobytes() and slots[qi].tobytes() == got['candidates'][qi].tobytes()
    own = (3.5, 180.25)
    one = ip.rd_pass(patterns[:1], targets[:1], candidates[:1], (22, 37), 2, True, own, neighbour_modes=(left[:1], above[:1]), **SUB)
    same_bits(one, cases.restatement(patterns[:1], targets[:1], candidates[:1], (22, 37), left[:1], above[:1], 2, True, own), "w %d n 1" % w)
    none = ip.rd_pass(patterns[:3], targets[:3], candidates[:3], (37,), **SUB)
    unavailable = np.full(3, cases.NONE, np.uint8)
    same_bits(none, cases.restatement(patterns[:3], targets[:3], candidates[:3], (37,), unavailable, unavailable), "w %d no neighbours" % w)


@pytest.mark.parametrize("w", (4, 8, 16, 32))
def test_with_mode_18_as_the_candidate_it_is_the_regular_search(w):
    """The candidate equal to pnn_hevc_intra_predict_hm(mode 18): every output equals the restatement fed the plain mode_hads[18]."""
    n, qps, smoothing = 7, (22, 37), 2
    patterns, targets, _ = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    regular = np.array([ip.predict_via_hevc_mode(np.ascontiguousarray(patterns[b][..., None]), w, 18, smoothing)[..., 0] for b in range(n)])
    hads = ip.mode_hads_host(patterns, targets, w, regular, smoothing=smoothing)
    assert np.array_equal(hads['hads_candidate'], hads['hads_modes'][:, 18])
    got = ip.rd_pass(patterns, targets, regular, qps, smoothing, neighbour_modes=(left, above), **SUB)
    same_bits(got, cases.restatement(patterns, targets, regular, qps, left, above, smoothing, cand_hads=hads['hads_modes'][:, 18]), "regular w %d" % w)


def test_known_answers_of_the_first_pass():
    w, n, qps = 8, 33, (22, 37)
    patterns, targets, candidates = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    got = ip.rd_pass(patterns, targets, candidates, qps, neighbour_modes=(left, above), **SUB)
    hads = ip.mode_hads_host(patterns, targets, w, candidates)
    k = ip.first_pass_list_size(w)
    seen = 0
    for qi, qp in enumerate(qps):
        root = math.sqrt(ip.hm_intra_lambda(qp))
        for b in range(n):
            mpm, _ = signal.mpm_of(left[b], above[b])
            where = np.flatnonzero(got['candidates'][qi, b, :k] == 18)
            if where.size:                                # mode 18's cost: the candidate's Hadamard cost and the bits of 18's MPM position
                bits = signal.mode_bits(18, mpm, qp, pnn_flag=False)
                position = mpm.index(18) if 18 in mpm else None
                prev = signal.bin_bits(signal.INIT_PREV_INTRA_PRED, qp)
                assert bits == (prev[0] + 5 * 32768 if position is None else prev[1] + 32768 * (1 if position == 0 else 2))
                assert got['first_pass_costs'][qi, b, where[0]] == float(int(hads['hads_candidate'][b])) + float(bits >> 15) * root
                seen += 1
    assert seen > 10
    # equal neighbours 18: MPMs 18, 17, 19, one of them appended
    unit = ip.intra_mode_signal([18], [18], 30, pnn_flag=False)
    assert tuple(unit['mpm'][0]) == (18, 17, 19) and unit['num_append'][0] == 1
    poor = np.clip(targets[:1].astype(np.int64) + np.random.default_rng(3).integers(-90, 91, targets[:1].shape), 0, 255).astype(np.uint8)
    both = np.array([18], np.uint8)
    r = ip.rd_pass(patterns[:1], targets[:1], poor, (30,), neighbour_modes=(both, both), **SUB)
    assert 18 not in r['candidates'][0, 0, :k] and tuple(r['candidates'][0, 0, k:]) == (18, 255)
    # lambda 0: the list is the SATD order of the 35 costs, the candidate's in 18's place (ties: the lower mode first)
    zero = first_pass_codec(patterns, targets, candidates, qps, left, above, lambdas=(0., 0.))
    costs = hads['hads_modes'].astype(np.int64).copy()
    costs[:, 18] = hads['hads_candidate']
    order = np.argsort(costs, axis=1, kind='stable')[:, :k]
    for qi in range(2):
        assert np.array_equal(zero[0][qi], order) and np.array_equal(zero[1][qi], np.take_along_axis(costs, order, 1).astype(np.float64))


def test_side_bits_equal_hm_records():
    """Every winner's side bits, and all mode bits the unit entry returns with pnn_flag 0, equal hm_16_15_regular's own counts."""
    hm = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hm_mode_signal.npz"))
    triples = [tuple(int(x) for x in t) for t in hm['regular_triples']]
    pairs = hm['regular_triple_pair']
    as_ours = lambda v: np.where(v >= 254, 255, v).astype(np.uint8)
    for q, qp in enumerate(hm['qps']):
        unit = ip.intra_mode_signal(as_ours(pairs[:, 0]), as_ours(pairs[:, 1]), int(qp), pnn_flag=False)
        assert np.array_equal(unit['mode_frac_bits'][:, :35], hm['regular_bits'][:, q]) and not unit['mode_frac_bits'][:, 35].any()
    w, n, qps = 8, 33, (22, 37)
    patterns, targets, candidates = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    got = ip.rd_pass(patterns, targets, candidates, qps, 2, True, neighbour_modes=(left, above), **SUB)
    looked_up = 0
    for qi, qp in enumerate(qps):
        q = list(hm['qps']).index(qp)
        for b in range(n):
            mpm, _ = signal.mpm_of(left[b], above[b])
            if tuple(mpm) not in triples:
                continue
            coded = int(got['rates'][qi, b] != 0)
            want = int(hm['regular_bits'][triples.index(tuple(mpm)), q, int(got['modes'][qi, b])]) + int(hm['regular_cbf'][q, 0, coded])
            assert int(got['side_rates'][qi, b]) == want, (qp, b)
            looked_up += 1
    assert looked_up > n


def outputs(n, nq, w, codec):
    shapes = ip.rd_pass_signal_shapes(n, nq, w, codec)
    return [np.zeros(shape, dtype) for (_, dtype), shape in zip(ip.RD_PASS_SIGNAL_OUTPUTS, shapes)]


def test_codec_0_is_the_signal_entry():
    w, n, qps = 8, 5, (22, 37)
    patterns, targets, candidates = rd_pass_cases.seeded(w, n)
    left, above = signal.neighbours(w, n)
    L = _lib.lib()
    front = (patterns.ctypes.data, 17, 17, targets.ctypes.data, w, n, candidates.ctypes.data, 2, (ctypes.c_int * 2)(*qps), 2, None, 1, 0)
    a, b = outputs(n, 2, w, 'switch'), outputs(n, 2, w, 'switch')
    assert L.pnn_rd_pass_signal_host(*front, 1, left.ctypes.data, above.ctypes.data, *[o.ctypes.data for o in a]) == 0
    assert L.pnn_rd_pass_codec_host(*front, 1, left.ctypes.data, above.ctypes.data, 0, *[o.ctypes.data for o in b]) == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and (a[0] == 35).any()
    shapes = ip.rd_pass_shapes(n, 2, w)
    a, b = ([np.zeros(shape, dtype) for (_, dtype), shape in zip(ip.RD_PASS_OUTPUTS, shapes)] for _ in range(2))
    assert L.pnn_rd_pass_signal_host(*front, 0, None, None, *[o.ctypes.data for o in a], None, None) == 0
    assert L.pnn_rd_pass_codec_host(*front, 0, None, None, 0, *[o.ctypes.data for o in b], None, None) == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    plain = first_pass_codec(patterns, targets, candidates, qps, left, above, 2, codec=0)
    k, s = ip.first_pass_list_size(w), ip.rd_pass_slot_count(w, True)
    want = np.zeros((2, n, k), np.uint8), np.zeros((2, n, k)), np.zeros((2, n, s), np.uint8)
    assert L.pnn_first_pass_signal_host(*front[:11], left.ctypes.data, above.ctypes.data, *[o.ctypes.data for o in want]) == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, want))
    for width in cases.WIDTHS:
        for signalling in (0, 1):
            assert L.pnn_rd_pass_codec_slot_count(width, signalling, 0) == L.pnn_rd_pass_slot_count(width, signalling)
            assert L.pnn_rd_pass_codec_workspace_bytes(width, 7, 2, signalling, 0) == L.pnn_rd_pass_signal_workspace_bytes(width, 7, 2, signalling)


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_conditions_on_the_seeded_cases(w):
    """Each condition holds in at least 5 % of the (QP, block) pairs of the seeded cases, at every w, by the restatement alone: 18 is in
    the list, 18 is appended as a missing MPM, 18 wins, another mode wins, the winner is off slot 0, the mode bits reorder the list."""
    n = cases.CONDITION_BLOCKS[w]
    patterns, targets, candidates = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    assert {18, 17, 19, 255} <= set(left.tolist()) | set(above.tolist())
    found = []
    for qps, smoothing in cases.CONDITIONS:
        want = cases.restatement(patterns, targets, candidates, qps, left, above, smoothing)
        first = ip.mode_hads_host(patterns, targets, w, candidates, smoothing=smoothing)
        k = first['list_modes'].shape[1]
        satd = np.array([cases.first_pass(first['hads_modes'], first['hads_candidate'], left, above, qp, 0., k)[0] for qp in qps])
        found.append(cases.shares(want, satd))
    pooled = {key: float(np.mean([f[key] for f in found])) for key in found[0]}       # (equally many pairs in both)
    print("shares w %d: %s" % (w, {key: round(v, 4) for key, v in pooled.items()}))
    for key, share in pooled.items():
        assert share >= 0.05, (w, key, pooled)
        assert abs(share - cases.SHARES_FOUND[w][key]) < 5e-5, (w, key, share)        # the figures written down are these


@pytest.mark.parametrize("codec", ("switch", "substitution"))
def test_mode_stats_equal_bincount(codec):
    w, n, qps = 8, 33, (22, 37, 51)
    patterns, targets, candidates = cases.blocks(w, n)
    left, above = cases.neighbours(w, n)
    huge = (ip.hm_intra_lambda(22), ip.hm_intra_lambda(37), 1.7e308)                  # a caller's huge lambda: blocks without a winner
    runs = [ip.rd_pass(patterns, targets, candidates, qps, 2, lambdas=huge, signalling=True, neighbour_modes=(left, above), codec=codec)]
    if codec == "switch":
        runs.append(ip.rd_pass(patterns, targets, candidates, qps, 2, lambdas=huge))      # the K + 1 form: one [n][S] for all QPs
    for r in runs:
        got = ip.rd_pass_mode_stats(r['candidates'], r['modes'])
        want = cases.stats_of(r['candidates'], r['modes'])
        assert np.array_equal(got['fast_selections'], want[:, 0]) and np.array_equal(got['fast_wins'], want[:, 1])
        assert np.array_equal(got['rd_wins'], want[:, 2])
        used = (r['candidates'] != 255).reshape(-1, n, r['candidates'].shape[-1]).sum(axis=(1, 2))
        assert np.array_equal(got['modes_for_rd'], np.broadcast_to(used, (3,))) and got['runs'] == n
        assert (got['fast_wins'].sum(axis=1) == n).all() and (got['rd_wins'][:2].sum(axis=1) == n).all()
        no_winner = r['modes'][2] == 255                  # lambda R overflows wherever R > 1 whole bit: every J of such a block is +inf
        assert no_winner.any() and got['rd_wins'][2].sum() == n - no_winner.sum()     # a block without a winner counts nowhere
        assert codec == "switch" or not (got['fast_selections'][:, 35].any() or got['rd_wins'][:, 35].any())
    assert ip.rd_pass_mode_stats(np.zeros((0, 4), np.uint8), np.zeros((2, 0), np.uint8))['runs'] == 0


def test_refusals():
    L = _lib.lib()
    w, n = 8, 2
    patterns, targets, candidates = rd_pass_cases.seeded(w, n)
    qp = (ctypes.c_int * 1)(22)
    best = np.full((1, n), 0xA5, np.uint8)

    def host(codec=1, signalling=1, left=None, cand=candidates, out=best, width=w, lambdas=None, rdoq=0):
        l = None if left is None else np.array(left, np.uint8)
        return L.pnn_rd_pass_codec_host(patterns.ctypes.data, 17, 17, targets.ctypes.data, width, n, None if cand is None else cand.ctypes.data, 0, qp, 1,
                                        None if lambdas is None else (ctypes.c_double * 1)(*lambdas), 0, rdoq, signalling,
                                        None if l is None else l.ctypes.data, None, codec, None, None, None if out is None else out.ctypes.data,
                                        None, None, None, None, None, None)

    for bad in (dict(codec=2), dict(codec=-1), dict(signalling=0), dict(left=(35, 0)), dict(left=(0, 254)), dict(cand=None), dict(out=None),
                dict(width=12), dict(lambdas=(-1.,)), dict(lambdas=(0.,), rdoq=1)):
        assert host(**bad) != 0 and (best == 0xA5).all(), bad
    assert host() == 0 and not (best == 0xA5).all()
    slots = np.zeros((1, n, 10), np.uint8)
    bad_left = np.array([35, 0], np.uint8)
    front = (patterns.ctypes.data, 17, 17, targets.ctypes.data, w, n, candidates.ctypes.data, 0, qp, 1, None)
    assert L.pnn_first_pass_codec_host(*front, bad_left.ctypes.data, None, 1, None, None, slots.ctypes.data) != 0
    assert L.pnn_first_pass_codec_host(*front, None, None, 2, None, None, slots.ctypes.data) != 0
    assert L.pnn_first_pass_codec_host(*front, None, None, 1, None, None, None) != 0
    assert not slots.any()
    for width in cases.WIDTHS:
        assert L.pnn_rd_pass_codec_slot_count(width, 0, 1) == -1 and L.pnn_rd_pass_codec_slot_count(width, 1, 2) == -1
        assert L.pnn_rd_pass_codec_workspace_bytes(width, 3, 1, 0, 1) == 0 and L.pnn_rd_pass_codec_workspace_bytes(width, 3, 1, 1, 2) == 0
        assert L.pnn_rd_pass_codec_workspace_bytes(width, 3, 1, 1, 1) > 0
    assert L.pnn_rd_pass_codec_slot_count(12, 1, 1) == -1
    stats = np.full((1, 3, 36), 7, np.uint32)
    modes = np.zeros((1, n), np.uint8)
    for args in ((None, 0, 4, modes.ctypes.data, n, 1), (slots.ctypes.data, 0, 0, modes.ctypes.data, n, 1), (slots.ctypes.data, 0, 17, modes.ctypes.data, n, 1),
                 (slots.ctypes.data, 0, 4, None, n, 1), (slots.ctypes.data, 0, 4, modes.ctypes.data, -1, 1), (slots.ctypes.data, 0, 4, modes.ctypes.data, n, 0),
                 (slots.ctypes.data, 0, 4, modes.ctypes.data, n, 9)):
        assert L.pnn_rd_pass_mode_stats_host(*args, stats.ctypes.data) != 0 and (stats == 7).all(), args
    assert L.pnn_rd_pass_mode_stats_host(slots.ctypes.data, 0, 4, modes.ctypes.data, n, 1, None) != 0
    with pytest.raises(ValueError):
        ip.rd_pass(patterns, targets, candidates, (22,), codec='substitution')                       # without signalling
    with pytest.raises(ValueError):
        ip.rd_pass(patterns, targets, candidates, (22,), signalling=True, codec='other')
    with pytest.raises(ValueError):
        ip.rd_pass(patterns, targets, candidates, (22,), neighbour_modes=([35, 0], None), **SUB)
    with pytest.raises(ValueError):
        ip.rd_pass_slot_count(8, False, 'substitution')
    with pytest.raises(ValueError):
        ip.rd_pass_mode_stats(np.zeros((3, 4), np.uint8), np.zeros((2, 5), np.uint8))
    from context_adaptive_neural_network_based_prediction_amd import evaluation
    rows = cols = np.zeros(1, np.int64)
    for score in (evaluation.score_masks_from_pictures, evaluation.score_masks_from_picture_pairs):     # before anything touches the GPU
        with pytest.raises(ValueError, match="rd_pass_codec"):
            score(np.zeros((1, 24, 24, 1), np.uint8), 8, rows, cols, None, 0., [(0, 0)], rd_pass=True, rd_pass_codec='substitution')
        with pytest.raises(ValueError, match="rd_pass_codec"):
            score(np.zeros((1, 24, 24, 1), np.uint8), 8, rows, cols, None, 0., [(0, 0)], rd_pass=True, rd_pass_signalling=True, rd_pass_codec='hm')
        with pytest.raises(ValueError, match="rd_pass_mode_stats"):
            score(np.zeros((1, 24, 24, 1), np.uint8), 8, rows, cols, None, 0., [(0, 0)], rd_pass_mode_stats=True)


def test_sanitizer_program(tmp_path):
    """tests/sanitize_substitution.cpp, a stand-alone program over the new host entries, under AddressSanitizer + UBSan"""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    csrc = os.path.join(root, "context_adaptive_neural_network_based_prediction_amd", "csrc")
    exe = str(tmp_path / "sanitize_substitution")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                        "-Wall", "-Wextra", "-I" + os.path.join(root, "include"), os.path.join(here, "sanitize_substitution.cpp"),
                        os.path.join(csrc, "pnn_rd_pass.cpp"), os.path.join(csrc, "pnn_hevc_intra.cpp"), os.path.join(csrc, "pnn_trquant.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sanitize_substitution: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
