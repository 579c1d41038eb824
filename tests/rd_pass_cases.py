"""What tests/test_rd_pass.py and tests/test_gpu_rd_pass.py share: the seeded blocks of the second intra pass (include/pnn_hip.h, "the
second intra pass"), the Python restatement that pins the host twin, and the conditions the seeded cases must meet so that no case can
pass because nothing was decided.

The restatement calls the existing Python entries per candidate -- the first-pass list, the predictor, the transform coding with its
rate -- and decides in Python floats; it shares no line with csrc/pnn_rd_pass.cpp."""
import numpy as np

from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip

WIDTHS = (4, 8, 16, 32, 64)
CANDIDATE, UNUSED = 35, 255
QP_LISTS = {1: (27,), 4: (22, 27, 32, 37), 8: (0, 12, 22, 27, 32, 37, 45, 51)}
BLOCKS_PER_WORKGROUP = {4: 64, 8: 16, 16: 4, 32: 1, 64: 1}       # rd_candidates_kernel's G (csrc/pnn_hevc_intra.hip), trquant_kernel's too
# the candidate is the target plus noise of these amplitudes, block b taking NOISE[b % 4]: a candidate that enters the list and wins, one
# that does neither, and two in between
NOISE = (2, 120, 8, 30)
SEEDS = {4: 4104, 8: 4108, 16: 4116, 32: 4132, 64: 4164}

# What the host twin finds on seeded(w, 2 G + 1) at QP_LISTS[4] without smoothing or sign hiding, over the (QP, block) pairs (the first
# three) and over the blocks (the last two): shares of winners that are not slot 0, of wins of 35, of blocks whose list lacks 35.
# test_rd_pass.py asserts the conditions, not these figures.
SHARES_FOUND = {
    4: {'not_slot_0': 0.3450, 'pnn_wins': 0.5446, 'appended': 0.2481},
    8: {'not_slot_0': 0.3182, 'pnn_wins': 0.5000, 'appended': 0.2424},
    16: {'not_slot_0': 0.1667, 'pnn_wins': 0.5556, 'appended': 0.2222},
    32: {'not_slot_0': 0.2500, 'pnn_wins': 0.5000, 'appended': 0.3333},
    64: {'not_slot_0': 0.3333, 'pnn_wins': 0.5000, 'appended': 0.3333},
}


def seeded(w, n, seed=None):
    """(patterns [n, 2w + 1, 2w + 1], targets [n, w, w], candidates [n, w, w]) uint8: each block cut from a structured picture with a
    little noise (the modes differ, no two blocks agree), the pattern's first row and column the samples above and left of the target,
    the rest 255 as extract_intra_pattern leaves it; the candidate as NOISE says."""
    rng = np.random.default_rng(SEEDS[w] if seed is None else seed)
    side = 2 * w + 1
    yy, xx = np.mgrid[0:side, 0:side]
    patterns, targets, candidates = (np.full((n, side, side), 255, np.uint8), np.zeros((n, w, w), np.uint8), np.zeros((n, w, w), np.uint8))
    for b in range(n):
        f = rng.uniform(0.02, 0.4, 4) * 8 / w ** 0.5
        img = 128 + 60 * np.sin(f[0] * xx + f[1] * yy) + 40 * np.cos(f[2] * xx - f[3] * yy) + rng.normal(0, 3, (side, side))
        img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        patterns[b, 0, :], patterns[b, :, 0] = img[0, :], img[:, 0]
        targets[b] = img[1:w + 1, 1:w + 1]
        amplitude = NOISE[b % len(NOISE)]
        candidates[b] = np.clip(targets[b].astype(np.int64) + rng.integers(-amplitude, amplitude + 1, (w, w)), 0, 255)
    return patterns, targets, candidates


def restatement(patterns, targets, candidates, qps, smoothing=0, sign_data_hiding=False, lambdas=None):
    """rd_pass's dictionary (but 'psnrs_recon') from the existing Python entries and Python floats."""
    n, w = targets.shape[0], targets.shape[1]
    lists = ip.mode_hads_host(patterns, targets, w, candidates, smoothing=smoothing)['list_modes']
    k1 = lists.shape[1] + 1
    slots = np.full((n, k1), UNUSED, np.uint8)
    slots[:, :k1 - 1] = lists
    slots[(lists != CANDIDATE).all(axis=1), k1 - 1] = CANDIDATE
    sses, rates = np.zeros((len(qps), n, k1), np.uint32), np.zeros((len(qps), n, k1), np.uint64)
    where_mode, where_pnn = np.argwhere(slots < CANDIDATE), np.argwhere(slots == CANDIDATE)
    predictions = np.array([ip.predict_via_hevc_mode(np.ascontiguousarray(patterns[b][..., None]), w, int(slots[b, s]), smoothing)[..., 0]
                            for b, s in where_mode])
    for where, preds, modes in ((where_mode, predictions, slots[slots < CANDIDATE]), (where_pnn, candidates[where_pnn[:, 0]], None)):
        if len(where):                                    # the modes' scans follow them; 35 has no mode: the diagonal scan
            coded = ip.transform_code(preds, targets[where[:, 0]], qps, modes=modes, rate=True, sign_data_hiding=sign_data_hiding)
            sses[:, where[:, 0], where[:, 1]] = coded['sses_recon']
            rates[:, where[:, 0], where[:, 1]] = np.rint(coded['rate_bits'] * 32768.).astype(np.uint64)
    lams = [ip.hm_intra_lambda(q) for q in qps] if lambdas is None else [float(v) for v in lambdas]
    res = {'candidates': slots, 'costs': np.full((len(qps), n, k1), np.inf), 'modes': np.full((len(qps), n), UNUSED, np.uint8),
           'slots': np.full((len(qps), n), UNUSED, np.uint8), 'best_costs': np.full((len(qps), n), np.inf),
           'sses': np.zeros((len(qps), n), np.uint32), 'rates': np.zeros((len(qps), n), np.uint64), 'lambdas': np.array(lams)}
    for qi in range(len(qps)):
        for b in range(n):
            best = float('inf')
            for s in range(k1):
                if slots[b, s] == UNUSED:
                    continue
                bits = lams[qi] * float(int(rates[qi, b, s]) >> 15)
                cost = float(int(sses[qi, b, s])) + bits
                res['costs'][qi, b, s] = cost
                if cost < best:
                    best = cost
                    res['modes'][qi, b], res['slots'][qi, b], res['best_costs'][qi, b] = slots[b, s], s, cost
                    res['sses'][qi, b], res['rates'][qi, b] = sses[qi, b, s], rates[qi, b, s]
    res['rate_bits'] = res['rates'].astype(np.float64) / 32768.
    return res


def same_bits(got, want, label, keys=None):
    """Equal in dtype, shape and bytes (doubles by bit pattern), key by key."""
    for key in keys or want:
        g, v = got[key], want[key]
        assert g.dtype == v.dtype and g.shape == v.shape, (label, key, g.dtype, g.shape, v.dtype, v.shape)
        assert g.tobytes() == v.tobytes(), "%s %s: %d differing values" % (label, key, (g != v).sum())


def shares(result):
    """The figures of SHARES_FOUND from an rd_pass dictionary."""
    appended = result['candidates'][:, -1] == CANDIDATE
    return {'not_slot_0': float((result['slots'] != 0).mean()), 'pnn_wins': float((result['modes'] == CANDIDATE).mean()),
            'appended': float(appended.mean())}


def assert_conditions(result, label):
    """At least a tenth of the winners are not slot 0; 35 wins at least once and loses at least once; 35 is appended at least once and
    already listed at least once."""
    found = shares(result)
    assert found['not_slot_0'] >= 0.1, (label, found)
    assert 0. < found['pnn_wins'] < 1., (label, found)
    assert 0. < found['appended'] < 1., (label, found)
