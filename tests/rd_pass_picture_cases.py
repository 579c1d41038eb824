"""What tests/test_rd_pass_pictures.py (CPU) and tests/test_gpu_rd_pass_pictures.py (GPU) share: the second intra pass read from picture
planes (stage_blocks<W, G, PIC = true> through picture_corner in csrc/pnn_hevc_intra.hip, the masks turned into ph / pw by set_blocks in
csrc/pnn_eval.cpp) at all five widths -- seeded picture pairs, positions, masks, candidates and neighbours, and the yardstick, which is
built on the host without a kernel: the patterns by intraprediction.extract_intra_patterns from the context plane, the targets by numpy
slices of the target plane, blocks in (image, position) order, then the host twin intraprediction.rd_pass(device=None).

Shapes.  Per width IMAGES = 3 pictures of [3w + 5, 3w + 9] pixels, which admit the 6 x 10 corners rows 0 .. 5, cols 0 .. 9, and as many
positions as make n = IMAGES * positions = 2 G + 1, G being rd_candidates_kernel's blocks per workgroup:
    w    G   positions   n     what the shape forces
    4   64      43      129    two full workgroups and a ragged one; the image boundaries (blocks 43 and 86) fall inside workgroups
    8   16      11       33    the same, boundaries at 11 and 22
   16    4       3        9    the same, boundaries at 3 and 6
   32    1       1        3    one block per workgroup, three images
   64    1       1        3    the same; the largest picture is 197 x 201
The positions are a seeded choice without repetition that always holds the near corner (0, 0) and the far one (5, 9); where one position
is asked for it is the far corner, whose context square ends on the picture's last row and column.

At w = 32 the second picture is a faint ramp under noise of one level (its decoded version the same plus 4): its reference line is flat
enough on both arms for HM's strong filter (|p[-64] + p[0] - 2 p[-32]| < 8), the structured pictures' lines are not, so smoothing 1 and
2 differ on a line staged from the plane.

Rungs: 'plain' (no signalling), 'switch' (signalling, the switch codec), 'substitution' (signalling, the substitution codec); each with
RDOQ and sign-data hiding on at QPs (22, 37).  The neighbours are mode_signal_cases.neighbours; the substitution codec knows no mode 35,
so there a neighbour 35 becomes 18, the mode the PNN's block carries under that codec.

The conditions (assert_conditions; tests/test_rd_pass_pictures.py asserts them for every width, rung and smoothing of SMOOTHINGS on mask
(0, 0) and on the asymmetric one) are floors against a vacuous pass, not measurements.  What the host twin alone found with the seeds below, chosen on the CPU
before any GPU run -- shares of the (QP, block) pairs at the largest smoothing of the width: the candidate's mode wins / the winner is
off slot 0 / the largest number of distinct winning modes among the blocks of one QP:
    w     plain                switch               substitution
    4     0.465 / 0.368 / 26   0.492 / 0.302 / 25   0.434 / 0.368 / 27
    8     0.500 / 0.227 / 12   0.515 / 0.273 / 11   0.485 / 0.273 / 11
   16     0.556 / 0.222 /  5   0.556 / 0.222 /  5   0.556 / 0.222 /  5
   32     0.667 / 0.333 /  2   0.667 / 0.333 /  2   0.667 / 0.167 /  2
   64     0.667 / 0.333 /  2   0.667 / 0.333 /  2   0.667 / 0.333 /  2
At w = 32 the strong-filter flags of the three blocks are (False, True, False).
The host twin takes under 0.01 s at w = 4 (129 blocks, 11 slots, RDOQ, two QPs) and 0.03 s at w = 64 per call on one CPU core, so the
w = 4 case stays at n = 2 G + 1 = 129."""
import functools

import numpy as np

from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import mode_signal_cases
from tests import rd_pass_cases
from tests import util

WIDTHS = rd_pass_cases.WIDTHS
IMAGES = 3
POSITIONS_PER_IMAGE = {4: 43, 8: 11, 16: 3, 32: 1, 64: 1}
NEAR, FAR = (0, 0), (5, 9)                       # of a [3w + 5, 3w + 9] picture: rows 0 .. 5, cols 0 .. 9
QPS = (22, 37)
RUNGS = ('plain', 'switch', 'substitution')
RUNG_OPTIONS = {'plain': dict(signalling=False), 'switch': dict(signalling=True, codec='switch'),
                'substitution': dict(signalling=True, codec='substitution')}
CANDIDATE_MODE = {'plain': 35, 'switch': 35, 'substitution': 18}
# no mode smooths at w = 4 and 64 (rd_candidates_kernel asserts it); 1 and 2 differ at w = 32 only (the strong filter)
SMOOTHINGS = {4: (0,), 8: (0, 2), 16: (0, 2), 32: (0, 1, 2), 64: (0,)}
PICTURE_SEEDS = {4: 3304, 8: 3308, 16: 3316, 32: 5232, 64: 3564}      # (raised in steps of 100 until the host twin alone met the conditions)
FLAT_IMAGE = 1                                   # of the w = 32 pictures


def asymmetric(w):
    """The mask under which mask_w and mask_h cannot be exchanged unnoticed: (4, w); at w = 4 that one is the full mask, hence (0, 4)"""
    return (4, w) if w > 4 else (0, 4)


def masks(w):
    """The masks of the existing picture tests -- none, (4, w), the full one -- and at w = 4, where the last two are one, (0, 4)"""
    return ((0, 0), (4, w), (w, w)) if w > 4 else ((0, 0), (4, 4), (0, 4))


def blocks_per_call(w):
    return IMAGES * POSITIONS_PER_IMAGE[w]


@functools.lru_cache(maxsize=None)
def pictures(w):
    """[IMAGES, 3w + 5, 3w + 9, 2] uint8, read-only: util.picture_pairs -- channel 0 the original (the target plane), channel 1 its
    decoded version (the context plane) -- with the flat second picture at w = 32."""
    pair = util.picture_pairs(IMAGES, w, PICTURE_SEEDS[w])
    if w == 32:
        rng = np.random.default_rng(PICTURE_SEEDS[w] + 1)
        height, width = pair.shape[1:3]
        yy, xx = np.mgrid[0:height, 0:width]
        flat = np.clip(np.rint(120 + 0.04 * xx - 0.03 * yy + rng.normal(0, 1.0, (height, width))), 0, 251).astype(np.uint8)
        pair[FLAT_IMAGE, :, :, 0], pair[FLAT_IMAGE, :, :, 1] = flat, flat + 4
    pair.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def positions(w):
    """(rows, cols) int64 [POSITIONS_PER_IMAGE[w]], read-only"""
    count = POSITIONS_PER_IMAGE[w]
    corners = [(r, c) for r in range(FAR[0] + 1) for c in range(FAR[1] + 1) if (r, c) not in (NEAR, FAR)]
    order = np.random.default_rng(PICTURE_SEEDS[w] + 2).permutation(len(corners))
    chosen = ([FAR] if count == 1 else [NEAR, FAR] + [corners[i] for i in order[:count - 2]])
    rows, cols = np.array([p[0] for p in chosen], np.int64), np.array([p[1] for p in chosen], np.int64)
    rows.setflags(write=False)
    cols.setflags(write=False)
    return rows, cols


def planes(w, single=False):
    """(context plane, target plane) [IMAGES, H, W] uint8, contiguous; single: the one-picture form, both the original"""
    pair = pictures(w)
    target = np.ascontiguousarray(pair[..., 0])
    return (target if single else np.ascontiguousarray(pair[..., 1])), target


@functools.lru_cache(maxsize=None)
def blocks(w, mask, single=False):
    """(patterns [n, 2w + 1 - mask_h, 2w + 1 - mask_w], targets [n, w, w], candidates [n, w, w]) uint8, read-only, n = blocks_per_call(w),
    in (image, position) order -- made on the host, independently of the kernels.  The candidate is the target plus noise of amplitude
    rd_pass_cases.NOISE[b % 4], clipped: one that enters the list and wins, one that does neither, two in between."""
    context, target = planes(w, single)
    rows, cols = positions(w)
    patterns = ip.extract_intra_patterns(context[..., None], w, rows + w - 1, cols + w - 1, mask)[..., 0]
    targets = np.array([target[i, r + w:r + 2 * w, c + w:c + 2 * w] for i in range(IMAGES) for r, c in zip(rows, cols)])
    rng = np.random.default_rng(PICTURE_SEEDS[w] + 3)
    candidates = np.zeros_like(targets)
    for b in range(targets.shape[0]):
        amplitude = rd_pass_cases.NOISE[b % len(rd_pass_cases.NOISE)]
        candidates[b] = np.clip(targets[b].astype(np.int64) + rng.integers(-amplitude, amplitude + 1, (w, w)), 0, 255)
    out = (np.ascontiguousarray(patterns), np.ascontiguousarray(targets), candidates)
    for a in out:
        a.setflags(write=False)
    return out


def neighbours(w, rung, seed=None):
    """(left, above) uint8 [n] of a signalling rung, (None, None) of 'plain'"""
    if rung == 'plain':
        return None, None
    left, above = mode_signal_cases.neighbours(w, blocks_per_call(w), seed)
    if rung == 'substitution':
        left, above = (np.where(a == mode_signal_cases.PNN, CANDIDATE_MODE[rung], a).astype(np.uint8) for a in (left, above))
    return left, above


def host_twin(w, rung, patterns, targets, candidates, smoothing, neighbour_modes):
    """One rung on dense blocks through the host twin: RDOQ and sign-data hiding on, QPS, HM's lambdas"""
    return ip.rd_pass(np.ascontiguousarray(patterns), np.ascontiguousarray(targets), np.ascontiguousarray(candidates), QPS, smoothing, True, None,
                      device=None, rdoq=True, neighbour_modes=None if rung == 'plain' else neighbour_modes, **RUNG_OPTIONS[rung])


@functools.lru_cache(maxsize=None)
def yardstick(w, rung, mask, smoothing, single=False):
    """The host twin's dictionary of one rung on blocks(w, mask, single); computed once, shared, left unchanged"""
    result = host_twin(w, rung, *blocks(w, mask, single), smoothing, neighbours(w, rung))
    for value in result.values():
        value.setflags(write=False)
    return result


def strong_flags(w):
    """Per block of mask (0, 0): would HM's strong filter take its reference line under smoothing 2?  From the pattern, in numpy: p[j] the
    first row, p[-j] the first column."""
    patterns = blocks(w, (0, 0))[0].astype(np.int64)
    row, col = patterns[:, 0, :], patterns[:, :, 0]
    return (np.abs(col[:, 2 * w] + row[:, 0] - 2 * col[:, w]) < 8) & (np.abs(row[:, 0] + row[:, 2 * w] - 2 * row[:, w]) < 8)


def shares(result, rung):
    """(share of the (QP, block) pairs the candidate's mode wins, share of winners off slot 0, the largest number of distinct winning
    modes among the blocks of one QP)"""
    return (float((result['modes'] == CANDIDATE_MODE[rung]).mean()), float((result['slots'] != 0).mean()),
            max(int(np.unique(row).size) for row in result['modes']))


def assert_conditions(w, rung, result, label):
    wins, off_slot_0, distinct = shares(result, rung)
    if w <= 16:
        assert 0.1 <= wins <= 0.9, (label, wins)
    else:                                                 # three blocks, two QPs: the candidate wins at least once and loses at least once
        assert 0. < wins < 1., (label, wins)
    assert off_slot_0 > 0., label
    assert distinct >= 2, label
