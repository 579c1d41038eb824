"""What tests/test_substitution.py and tests/test_gpu_substitution.py share: a Python restatement of the substitution codec's intra
search as a column (include/pnn_hip.h, "the substitution codec"), written from the text of hm_16_15_substitution's
estIntraPredLumaQT (TEncSearch.cpp:2325-2584) and predIntraAng (TComPrediction.cpp:506-556): HM's own loop over modes 0 .. 34 with the
PNN's block returned for mode 18.  Also the seeded blocks, neighbours and candidates, and the conditions they must meet.

The restatement calls the existing Python entries per slot -- the Hadamard costs, the predictor, the transform coding with its rate at
one QP -- and decides in Python floats; the MPMs, the mode bits (pnn_flag off) and the cbf bins are tests/mode_signal_cases.py's, which
tests/golden/hm_mode_signal.npz pins to hm_16_15_regular's own output.  It shares no line with csrc/pnn_rd_pass.cpp or
csrc/pnn_mode_signal.h."""
import math

import numpy as np

from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import mode_signal_cases as signal
from tests import rd_pass_cases

WIDTHS = signal.WIDTHS
PNN_MODE, NONE, UNUSED = 18, 255, 255
BLOCKS_PER_WORKGROUP = rd_pass_cases.BLOCKS_PER_WORKGROUP
QP_PAIRS = signal.QP_PAIRS
CONDITION_BLOCKS = {w: max(2 * g + 1, 25) for w, g in BLOCKS_PER_WORKGROUP.items()}
CONDITIONS = ((QP_PAIRS[0], 0), (QP_PAIRS[1], 2))                       # (QPs, smoothing), RDOQ off
NEIGHBOUR_SEEDS = {4: 7004, 8: 7008, 16: 7016, 32: 7032, 64: 7064}
POOR_CANDIDATE_EVERY = 3                                               # every third block's candidate is far from its target

# What the restatement finds on blocks(w, CONDITION_BLOCKS[w]) with neighbours(w, CONDITION_BLOCKS[w]), as shares of the (QP, block)
# pairs of both configurations of CONDITIONS.  test_substitution.py asserts that each is at least 5 %, not these figures.
SHARES_FOUND = {
    4: {'pnn_listed': 0.7267, 'pnn_appended': 0.1047, 'pnn_wins': 0.4264, 'other_wins': 0.5736, 'winner_off_slot_0': 0.4128,
        'list_reordered': 0.3818},
    8: {'pnn_listed': 0.5985, 'pnn_appended': 0.2197, 'pnn_wins': 0.4091, 'other_wins': 0.5909, 'winner_off_slot_0': 0.3485,
        'list_reordered': 0.2576},
    16: {'pnn_listed': 0.37, 'pnn_appended': 0.23, 'pnn_wins': 0.37, 'other_wins': 0.63, 'winner_off_slot_0': 0.3, 'list_reordered': 0.14},
    32: {'pnn_listed': 0.36, 'pnn_appended': 0.2, 'pnn_wins': 0.32, 'other_wins': 0.68, 'winner_off_slot_0': 0.25, 'list_reordered': 0.16},
    64: {'pnn_listed': 0.36, 'pnn_appended': 0.28, 'pnn_wins': 0.32, 'other_wins': 0.68, 'winner_off_slot_0': 0.26, 'list_reordered': 0.06},
}


def blocks(w, n):
    """mode_signal_cases.blocks(w, n) -- structured blocks and, from w = 16 on, nearly flat ones, on which the mode-bit term reorders the
    list -- with every third candidate replaced by a poor one (the target under heavy noise): such a candidate's Hadamard cost keeps 18
    out of the list, so that 18 is coded only where it is a most probable mode the search appends."""
    patterns, targets, candidates = signal.blocks(w, n)
    rng = np.random.default_rng(7100 + w)
    for b in range(2, n, POOR_CANDIDATE_EVERY):
        candidates[b] = np.clip(targets[b].astype(np.int64) + rng.integers(-70, 71, (w, w)), 0, 255)
    return patterns, targets, candidates


def neighbours(w, n, seed=None):
    """(left, above) uint8 [n], each 0 .. 34 or 255: no neighbour, 18 on one side, equal angular modes (18, 17, 19 and the wrap-arounds 2
    and 34 among them), planar / DC, anything; a block with a poor candidate has 18 to its left more often than not, so that 18 is a
    most probable mode the list lacks."""
    rng = np.random.default_rng(NEIGHBOUR_SEEDS[w] if seed is None else seed)
    wanted, n = n, max(n, CONDITION_BLOCKS[w])            # (always the same draw: fewer blocks are the first of them)
    kinds = rng.integers(0, 8, n)
    left, above = rng.integers(0, 35, n), rng.integers(0, 35, n)
    left[kinds == 0] = NONE
    above[kinds == 1] = NONE
    left[kinds == 2] = PNN_MODE
    above[kinds == 3] = PNN_MODE
    same = kinds == 4
    above[same] = left[same]
    left[kinds == 5] = rng.choice((0, 1), int((kinds == 5).sum()))
    edge = kinds == 6
    left[edge] = above[edge] = rng.choice((18, 17, 19, 2, 34), int(edge.sum()))
    poor = np.arange(n) % POOR_CANDIDATE_EVERY == 2
    left[poor & (kinds % 2 == 0)] = PNN_MODE
    left[0], above[0] = PNN_MODE, PNN_MODE                # the first blocks, deliberately: 18 twice (MPMs 18, 17, 19), 17, 19 and 255
    left[1], above[1] = 17, NONE
    left[3], above[3] = NONE, 19
    return left.astype(np.uint8)[:wanted], above.astype(np.uint8)[:wanted]


def mode_bits(mode, mpm, qp):
    """codeIntraDirLumaAng of the substitution tree: hm_16_15_regular's, no flag bin"""
    assert 0 <= mode <= 34
    return signal.mode_bits(mode, mpm, qp, pnn_flag=False)


def first_pass(hads, cand_hads, left, above, qp, lam, k):
    """(list modes [n][k], list costs [n][k], slots [n][k + 2]) from the Hadamard costs: xUpdateCandList over 0 .. 34 on Python floats,
    mode 18's cost being the candidate's; then uiPreds[0 .. numCand - 1] where the list lacks them"""
    n = len(cand_hads)
    root = math.sqrt(lam)
    modes, costs, slots = np.zeros((n, k), np.uint8), np.zeros((n, k)), np.full((n, k + 2), UNUSED, np.uint8)
    for b in range(n):
        mpm, num = signal.mpm_of(left[b], above[b])
        lm, lc = [UNUSED] * k, [float('inf')] * k
        for i in range(35):
            satd = int(cand_hads[b]) if i == PNN_MODE else int(hads[b, i])
            bits = float(mode_bits(i, mpm, qp) >> 15) * root
            cost = float(satd) + bits
            shift = 0
            while shift < k and cost < lc[k - 1 - shift]:
                shift += 1
            if shift:
                at = k - shift
                lm[at + 1:], lc[at + 1:] = lm[at:k - 1], lc[at:k - 1]
                lm[at], lc[at] = i, cost
        rd_list = list(lm)
        for m in mpm[:num]:
            if m not in rd_list:
                rd_list.append(m)
        modes[b], costs[b] = lm, lc
        slots[b, :len(rd_list)] = rd_list
    return modes, costs, slots


def restatement(patterns, targets, candidates, qps, left, above, smoothing=0, sign_data_hiding=False, lambdas=None, rdoq=False,
                cand_hads=None):
    """rd_pass(signalling=True, codec='substitution')'s dictionary (but 'psnrs_recon') from the existing Python entries and Python floats.
    cand_hads: the Hadamard cost that stands for mode 18 (None: the candidate's own)."""
    n, w = targets.shape[0], targets.shape[1]
    nq = len(qps)
    first = ip.mode_hads_host(patterns, targets, w, candidates, smoothing=smoothing)
    if cand_hads is None:
        cand_hads = first['hads_candidate']
    k = first['list_modes'].shape[1]
    s = k + 2
    lams = [ip.hm_intra_lambda(q) for q in qps] if lambdas is None else [float(v) for v in lambdas]
    ctx = 1 if w in (8, 16, 32) else 0
    res = {'candidates': np.zeros((nq, n, s), np.uint8), 'costs': np.full((nq, n, s), np.inf), 'modes': np.full((nq, n), UNUSED, np.uint8),
           'slots': np.full((nq, n), UNUSED, np.uint8), 'best_costs': np.full((nq, n), np.inf), 'sses': np.zeros((nq, n), np.uint32),
           'rates': np.zeros((nq, n), np.uint64), 'first_pass_costs': np.zeros((nq, n, k)), 'side_rates': np.zeros((nq, n), np.uint64),
           'lambdas': np.array(lams)}
    units = 4 if w == 64 else 1
    for qi, qp in enumerate(qps):
        _, res['first_pass_costs'][qi], slots = first_pass(first['hads_modes'], cand_hads, left, above, qp, lams[qi], k)
        res['candidates'][qi] = slots
        sses, rates, nonzero = (np.zeros((n, s), np.int64) for _ in range(3))
        where = np.argwhere(slots != UNUSED)
        preds = np.array([candidates[b] if slots[b, j] == PNN_MODE else
                          ip.predict_via_hevc_mode(np.ascontiguousarray(patterns[b][..., None]), w, int(slots[b, j]), smoothing)[..., 0]
                          for b, j in where])
        tg = targets[where[:, 0]]
        modes = slots[slots != UNUSED]                    # the scan follows the slot's mode, 18 included (diagonal)
        if w == 64:                                       # the four quadrants as 32 x 32 blocks of their own, diagonal scan
            assert not rdoq                               # (its cbf context differs there: the twin is checked against the kernels instead)
            preds, tg = (np.ascontiguousarray(a.reshape(-1, 2, 32, 2, 32).transpose(0, 1, 3, 2, 4).reshape(-1, 32, 32)) for a in (preds, tg))
            modes = None
        coded = ip.transform_code(preds, tg, (qp,), modes=modes, rate=True, sign_data_hiding=sign_data_hiding, rdoq=rdoq,
                                  lambdas=(lams[qi],) if rdoq else None)
        sses[where[:, 0], where[:, 1]] = coded['sses_recon'][0].astype(np.int64).reshape(-1, units).sum(axis=1)
        rates[where[:, 0], where[:, 1]] = np.rint(coded['rate_bits'][0] * 32768.).astype(np.int64).reshape(-1, units).sum(axis=1)
        nonzero[where[:, 0], where[:, 1]] = (coded['nb_nonzero_levels'][0].reshape(-1, units) != 0).sum(axis=1)     # coded units
        cbf = signal.cbf_bits(qp)[ctx]
        for b in range(n):
            mpm, _ = signal.mpm_of(left[b], above[b])
            best = float('inf')
            for j in range(s):
                if slots[b, j] == UNUSED:
                    continue
                side = mode_bits(int(slots[b, j]), mpm, qp) + int(nonzero[b, j]) * cbf[1] + (units - int(nonzero[b, j])) * cbf[0]
                coefficient = int(rates[b, j]) if nonzero[b, j] else 0
                bits = lams[qi] * float((side + coefficient) >> 15)
                cost = float(int(sses[b, j])) + bits
                res['costs'][qi, b, j] = cost
                if cost < best:
                    best = cost
                    res['modes'][qi, b], res['slots'][qi, b], res['best_costs'][qi, b] = slots[b, j], j, cost
                    res['sses'][qi, b], res['rates'][qi, b], res['side_rates'][qi, b] = sses[b, j], rates[b, j], side
    res['rate_bits'] = res['rates'].astype(np.float64) / 32768.
    res['side_rate_bits'] = res['side_rates'].astype(np.float64) / 32768.
    return res


def shares(result, satd_lists):
    """The shares of the (QP, block) pairs that meet each condition: `result` a dictionary of the column, satd_lists [nb_qps][n][K] the
    lists of the same blocks under lambda 0 (plain SATD order)."""
    k = satd_lists.shape[2]
    lists, extra = result['candidates'][:, :, :k], result['candidates'][:, :, k:]
    return {'pnn_listed': float((lists == PNN_MODE).any(axis=2).mean()), 'pnn_appended': float((extra == PNN_MODE).any(axis=2).mean()),
            'pnn_wins': float((result['modes'] == PNN_MODE).mean()), 'other_wins': float((result['modes'] != PNN_MODE).mean()),
            'winner_off_slot_0': float((result['slots'] != 0).mean()), 'list_reordered': float((lists != satd_lists).any(axis=2).mean())}


def stats_of(candidates, modes):
    """numpy.bincount of a column's slots and winners: uint32 [nb_qps][3][36]"""
    nq = modes.shape[0]
    per_qp = candidates.ndim == 3
    out = np.zeros((nq, 3, 36), np.uint32)
    for qi in range(nq):
        slots = candidates[qi] if per_qp else candidates
        out[qi, 0] = np.bincount(slots[slots <= 35], minlength=36)
        out[qi, 1] = np.bincount(slots[:, 0][slots[:, 0] <= 35], minlength=36)
        out[qi, 2] = np.bincount(modes[qi][modes[qi] <= 35], minlength=36)
    return out
