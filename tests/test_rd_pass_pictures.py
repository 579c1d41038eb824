"""The conditions on the cases of tests/rd_pass_picture_cases.py, from the host twin alone (no GPU): what
tests/test_gpu_rd_pass_pictures.py compares the picture form of the second intra pass with decides something in every width and rung,
the 2 G + 1 table is the library's, and the seeded pictures are the ones the existing picture tests get."""
import hashlib

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import rd_pass_cases
from tests import rd_pass_picture_cases as cases
from tests import util


def test_picture_pairs_are_the_recorded_ones():
    """util.picture_pairs as the existing picture tests call it: the digest recorded from the parent commit"""
    pair = util.picture_pairs(2, 8, 2700 + 8)
    assert pair.shape == (2, 29, 33, 2) and pair.dtype == np.uint8
    assert hashlib.sha256(pair.tobytes()).hexdigest() == "6c646de53cd711ac2c22ed01e32218352aced6152914e476be507ad21ac06d1f"


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_shapes_force_what_the_table_says(w):
    g = rd_pass_cases.BLOCKS_PER_WORKGROUP[w]
    n = cases.blocks_per_call(w)
    assert n == 2 * g + 1 and n == cases.IMAGES * cases.POSITIONS_PER_IMAGE[w]
    pair = cases.pictures(w)
    assert pair.shape == (cases.IMAGES, 3 * w + 5, 3 * w + 9, 2)
    assert (pair[..., 0] != pair[..., 1]).all()           # a read from the wrong plane shows at every pixel
    rows, cols = cases.positions(w)
    chosen = list(zip(rows.tolist(), cols.tolist()))
    assert len(set(chosen)) == len(chosen) == cases.POSITIONS_PER_IMAGE[w]
    assert cases.FAR in chosen and (cases.NEAR in chosen or len(chosen) == 1)
    assert rows.min() >= 0 and cols.min() >= 0 and rows.max() + 3 * w <= pair.shape[1] and cols.max() + 3 * w <= pair.shape[2]
    assert rows.max() + 3 * w == pair.shape[1] and cols.max() + 3 * w == pair.shape[2]           # the far corner touches both edges
    if g > 1:                                             # an image boundary inside a workgroup
        assert any((i * cases.POSITIONS_PER_IMAGE[w]) % g for i in range(1, cases.IMAGES))
    # no two images give the same blocks at one position: an image term left out of the corner shows
    patterns, targets, _ = cases.blocks(w, (0, 0))
    per = cases.POSITIONS_PER_IMAGE[w]
    for i in range(1, cases.IMAGES):
        assert (patterns[i * per:(i + 1) * per, 0] != patterns[:per, 0]).any(axis=1).all()
        assert (targets[i * per:(i + 1) * per] != targets[:per]).any(axis=(1, 2)).all()
    # the asymmetric mask's patterns are not the exchanged mask's: [n, 2w + 1 - mask_h, 2w + 1 - mask_w]
    mask = cases.asymmetric(w)
    assert cases.blocks(w, mask)[0].shape[1:] == (2 * w + 1 - mask[1], 2 * w + 1 - mask[0])
    L = _lib.lib()
    for rung in cases.RUNGS:
        options = cases.RUNG_OPTIONS[rung]
        signalling, codec = int(options['signalling']), ip.CODECS[options.get('codec', 'switch')]
        for count in (n, cases.POSITIONS_PER_IMAGE[w]):   # the batch and one image of it
            assert L.pnn_rd_pass_codec_workspace_bytes(w, count, len(cases.QPS), signalling, codec) > 0, (w, rung, count)
        if rung == 'plain':
            assert L.pnn_rd_pass_workspace_bytes(w, n, len(cases.QPS)) > 0
        if rung == 'switch':
            assert L.pnn_rd_pass_signal_workspace_bytes(w, n, len(cases.QPS), 1) > 0


@pytest.mark.parametrize("rung", cases.RUNGS)
@pytest.mark.parametrize("w", cases.WIDTHS)
def test_every_rung_decides_something(w, rung):
    for smoothing in cases.SMOOTHINGS[w]:
        for mask in ((0, 0), cases.asymmetric(w)):
            result = cases.yardstick(w, rung, mask, smoothing)
            found = cases.shares(result, rung)
            print("w %d %s mask %s smoothing %d: candidate wins %.3f, off slot 0 %.3f, distinct winners %d" % ((w, rung, mask, smoothing) + found))
            cases.assert_conditions(w, rung, result, "w %d %s mask %s smoothing %d" % (w, rung, mask, smoothing))
            assert result['modes'].shape == (len(cases.QPS), cases.blocks_per_call(w))
            if rung == 'substitution':
                assert not (result['candidates'] == 35).any()


def test_strong_filter_is_taken_and_left_at_32():
    flags = cases.strong_flags(32)
    print("strong filter at w = 32:", flags.tolist())
    assert flags.any() and not flags.all()
    assert flags[cases.FLAT_IMAGE]
    # ... and it decides something: the smoothed line of the flat block differs between smoothing 1 and 2
    pattern = np.ascontiguousarray(cases.blocks(32, (0, 0))[0][cases.FLAT_IMAGE][..., None])
    assert not np.array_equal(ip.smoothed_reference(pattern, 32, 1), ip.smoothed_reference(pattern, 32, 2))
    for rung in cases.RUNGS:
        one, two = (cases.yardstick(32, rung, (0, 0), s) for s in (1, 2))
        assert one['costs'].tobytes() != two['costs'].tobytes(), rung


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_masks_and_planes_change_the_answer(w):
    """What a mistake in the geometry would have to change: the asymmetric mask's answer is neither the unmasked one nor the exchanged
    mask's, and the single-picture form's is not the pair's"""
    smoothing = cases.SMOOTHINGS[w][-1]
    mask = cases.asymmetric(w)
    assert mask[0] != mask[1] and mask in cases.masks(w) and (0, 0) in cases.masks(w)
    base = cases.yardstick(w, 'switch', mask, smoothing)
    assert base['costs'].tobytes() != cases.yardstick(w, 'switch', (0, 0), smoothing)['costs'].tobytes()
    patterns, targets, candidates = cases.blocks(w, mask)
    rows, cols = cases.positions(w)
    exchanged = ip.extract_intra_patterns(cases.planes(w)[0][..., None], w, rows + w - 1, cols + w - 1, mask[::-1])[..., 0]
    other = cases.host_twin(w, 'switch', exchanged, targets, candidates, smoothing, cases.neighbours(w, 'switch'))
    assert base['costs'].tobytes() != other['costs'].tobytes()
    assert base['costs'].tobytes() != cases.yardstick(w, 'switch', mask, smoothing, True)['costs'].tobytes()
