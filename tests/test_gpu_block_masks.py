"""Masks per block through the picture entries on the GPU (include/pnn_hip.h, "masks per block"):
pnn_score_picture_pairs_masks_device, pnn_first_pass_picture_pairs_masks_device and pnn_rd_pass_picture_pairs_masks_device, called raw
between guard bytes (tests/util.py), byte for byte and block by block against the EXISTING entry of each -- pnn_score_picture_pairs_hm_device,
pnn_first_pass_picture_pairs_hm_device, pnn_rd_pass_tskip_picture_pairs_device -- called once per distinct mask (and image) on the
positions that carry it, with the outputs scattered back.  The picture is a seeded 256 x 256 pair, the blocks those of 2 x 2 CTUs from
(64, 64), the masks intraprediction.hm_context_masks': at width 4 that is 1024 blocks whose groups of one workgroup mix all four masks.
Also: two images (masks by POSITION, not by block), sliced passes (max_chunk), all masks (0, 0) against the scalar entry, every refusal
before a launch, and evaluation.score_block_masks_from_picture_pairs against score_masks_from_picture_pairs per mask on subsets."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib, evaluation
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cu_tree_picture_cases as pc
from tests import util
from tests.util import PNN_E_ARG, dev, untouched

pytestmark = pytest.mark.gpu

QPS = (22, 37)
SIDE, SEED = 256, 6100
KINDS = ("score", "first_pass", "rd_pass")
ENTRIES = {"score": ("pnn_score_picture_pairs_hm_device", "pnn_score_picture_pairs_masks_device"),
           "first_pass": ("pnn_first_pass_picture_pairs_hm_device", "pnn_first_pass_picture_pairs_masks_device"),
           "rd_pass": ("pnn_rd_pass_tskip_picture_pairs_device", "pnn_rd_pass_picture_pairs_masks_device")}
RD_OUTPUTS = tuple(ip.RD_PASS_SIGNAL_OUTPUTS) + (('best_transform_skip', np.uint8),)


@pytest.fixture(scope="module")
def nets():
    made = {w: util.make_net(w, w <= 8, 2 * pc.POSITIONS[w][0].size) for w in ip.WIDTHS}
    yield made
    for net in made.values():
        net.close()


def pair(images):
    """[images, 256, 256, 2]: seeded pictures as the originals, further seeded pictures as the decoded planes"""
    pictures = util.pictures(2 * images, SIDE, SIDE, SEED)
    return np.ascontiguousarray(np.stack([pictures[:images], pictures[images:]], axis=-1))


def candidates(images, w):
    """a candidate prediction per block [images, positions, w, w], seeded; what the first and second passes take as mode 35"""
    return np.random.default_rng(SEED + w).integers(60, 200, (images, pc.POSITIONS[w][0].size, w, w)).astype(np.uint8)


def specs_of(kind, w, n, codec):
    """(dtype, shape) of the kind's outputs and the axis their blocks lie on"""
    if kind == "score":
        return [(np.uint8, (n, w, w)), (np.uint8, (n, w, w)), (np.float32, (n, w, w)), (np.uint32, (n,)), (np.uint8, (n,)), (np.uint32, (n,)),
                (np.uint8, (n, w, w))], 0
    if kind == "first_pass":
        k = ip.first_pass_list_size(w)
        return [(np.uint32, (n, 35)), (np.uint32, (n,)), (np.uint8, (n, k)), (np.uint32, (n, k))], 0
    return [(dtype, shape) for (_, dtype), shape in zip(RD_OUTPUTS, tuple(ip.rd_pass_signal_shapes(n, len(QPS), w, codec)) + ((len(QPS), n),))], 1


def launches(ctx):
    count = ctypes.c_int(-1)
    assert _lib.lib().pnn_last_call_stats(ctx, None, None, ctypes.byref(count)) == 0
    return count.value


def entry_call(kind, net, w, channels, rows, cols, masks, cand, codec='switch', tskip=0, wanted=None):
    """One raw guarded call.  masks: (int, int) -- the existing entry -- or two device tensors / None -- the new one.  channels
    [images, H, W, 2]; rows, cols: the positions; cand [images * positions, w, w].  Returns (rc, outputs, intact)."""
    import torch
    images, n_pos = channels.shape[0], rows.size
    n = images * n_pos
    per_block = not isinstance(masks[0], (int, np.integer))
    held = [dev(np.ascontiguousarray(channels[..., 1])), dev(np.ascontiguousarray(channels[..., 0])), dev(rows.astype(np.int32)),
            dev(cols.astype(np.int32)), dev(cand)]
    mask_arguments = tuple(util.ptr(m) for m in masks) if per_block else (int(masks[0]), int(masks[1]))
    blocks = (net.ctx, w, held[0].data_ptr(), held[1].data_ptr(), images, SIDE, SIDE, held[2].data_ptr(), held[3].data_ptr(), n_pos) + mask_arguments
    specs, _ = specs_of(kind, w, n, codec)
    wanted = (True,) * len(specs) if wanted is None else wanted
    entry = ENTRIES[kind][per_block]
    if kind == "score":
        return util.call(entry, blocks, (2,), specs, wanted)
    if kind == "first_pass":
        return util.call(entry, blocks + (held[4].data_ptr(),), (2,), specs, wanted)
    number = ip.CODECS[codec]
    nb = _lib.lib().pnn_rd_pass_tskip_workspace_bytes(w, n, len(QPS), 1, number, tskip)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    front = blocks + (held[4].data_ptr(), 2, (ctypes.c_int * len(QPS))(*QPS), len(QPS), None, 1, 1, 1, None, None, number, tskip)
    return util.call(entry, front, (), specs, wanted, after=(ws.data_ptr(), nb))


def new_entry(kind, net, w, channels, masks_w, masks_h, cand, **options):
    """The new entry on every position of width w with masks per position (numpy [positions]; held on the device past the call)"""
    rows, cols = pc.POSITIONS[w]
    held = (dev(masks_w), dev(masks_h))
    rc, outs, intact = entry_call(kind, net, w, channels, rows, cols, held, cand.reshape(-1, w, w), **options)
    assert rc == 0 and intact, _lib.lib().pnn_last_error(net.ctx)
    return outs


def by_subsets(kind, net, w, channels, masks_w, masks_h, cand, **options):
    """The yardstick, from the EXISTING entry alone: per image and per distinct mask ONE call with the scalar mask on the positions that
    carry it in that image, scattered back.  masks_w / masks_h: [images, positions], the mask each BLOCK is to be read with."""
    rows, cols = pc.POSITIONS[w]
    images, n_pos = masks_w.shape
    specs, axis = specs_of(kind, w, images * n_pos, options.get('codec', 'switch'))
    full = [np.zeros(shape, dtype) for dtype, shape in specs]
    filled = np.zeros(images * n_pos, bool)
    for i in range(images):
        for mask in sorted({(int(a), int(b)) for a, b in zip(masks_w[i], masks_h[i])}):
            idx = np.flatnonzero((masks_w[i] == mask[0]) & (masks_h[i] == mask[1]))
            rc, outs, intact = entry_call(kind, net, w, channels[i:i + 1], rows[idx], cols[idx], mask, cand[i, idx], **options)
            assert rc == 0 and intact, _lib.lib().pnn_last_error(net.ctx)
            for out, whole in zip(outs, full):
                whole[(slice(None),) * axis + (i * n_pos + idx,)] = out
            filled[i * n_pos + idx] = True
    assert filled.all()
    return full


def assert_blocks_equal(got, want, label):
    for k, (g, v) in enumerate(zip(got, want)):
        assert g.dtype == v.dtype and g.shape == v.shape, (label, k)
        assert g.tobytes() == v.tobytes(), "%s output %d: %d differing values" % (label, k, (g != v).sum())


def rd_options(w):
    """both codecs; at width 4 with and without transform skip"""
    return [dict(codec=codec, tskip=tskip) for codec in ('switch', 'substitution') for tskip in ((0, 1) if w == 4 else (0,))]


@pytest.mark.parametrize("w", ip.WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_new_entry_equals_the_existing_one_per_mask(nets, kind, w):
    """All 341 x 4 blocks of the 2 x 2 grid, width by width (1024 at width 4, where the blocks one workgroup stages mix all four masks),
    masks of hm_context_masks; QPs 22 and 37, both codecs, transform skip at width 4."""
    channels, cand = pair(1), candidates(1, w)
    masks_w, masks_h = ip.hm_context_masks(w, 2, 2)
    if w < 64:
        assert {(int(a), int(b)) for a, b in zip(masks_w, masks_h)} == {(0, 0), (0, w), (w, 0), (w, w)}
    for options in rd_options(w) if kind == "rd_pass" else [{}]:
        got = new_entry(kind, nets[w], w, channels, masks_w, masks_h, cand, **options)
        want = by_subsets(kind, nets[w], w, channels, masks_w[None], masks_h[None], cand, **options)
        assert_blocks_equal(got, want, "%s width %d %s" % (kind, w, options))


@pytest.mark.parametrize("kind", KINDS)
def test_partial_last_group(nets, kind):
    """1024 blocks fill every workgroup's group of blocks; with the first 1023 positions the last workgroup of every kernel is partial,
    and its blocks still mix masks.  A block's bytes do not depend on the other blocks of the call: they equal the whole call's."""
    w = 4
    channels, cand = pair(1), candidates(1, w)
    masks_w, masks_h = ip.hm_context_masks(w, 2, 2)
    rows, cols = pc.POSITIONS[w]
    keep = np.arange(1023)
    held = (dev(masks_w[keep]), dev(masks_h[keep]))
    for options in rd_options(w) if kind == "rd_pass" else [{}]:
        rc, got, intact = entry_call(kind, nets[w], w, channels, rows[keep], cols[keep], held, cand[0, keep], **options)
        assert rc == 0 and intact
        whole = new_entry(kind, nets[w], w, channels, masks_w, masks_h, cand, **options)
        _, axis = specs_of(kind, w, 1024, options.get('codec', 'switch'))
        assert_blocks_equal(got, [np.ascontiguousarray(a[(slice(None),) * axis + (keep,)]) for a in whole], "%s %s" % (kind, options))


@pytest.mark.parametrize("kind", KINDS)
def test_two_images_read_their_masks_by_position(nets, kind):
    """Two images at width 8.  The device arrays hold 2 x positions masks, the second half the first half reversed: an entry that
    indexed by BLOCK would read the second half for image 1.  From the existing entry alone the two readings differ; the new entry
    gives the reading by position."""
    w = 8
    channels, cand = pair(2), candidates(2, w)
    masks_w, masks_h = ip.hm_context_masks(w, 2, 2)
    n_pos = masks_w.size
    both_w, both_h = np.concatenate([masks_w, masks_w[::-1]]), np.concatenate([masks_h, masks_h[::-1]])
    options = dict(codec='switch', tskip=0) if kind == "rd_pass" else {}
    by_position = by_subsets(kind, nets[w], w, channels, np.stack([masks_w, masks_w]), np.stack([masks_h, masks_h]), cand, **options)
    by_block = by_subsets(kind, nets[w], w, channels, both_w.reshape(2, n_pos), both_h.reshape(2, n_pos), cand, **options)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(by_position, by_block)), "the two readings give the same bytes: the test shows nothing"
    rows, cols = pc.POSITIONS[w]
    held = (dev(both_w), dev(both_h))
    rc, got, intact = entry_call(kind, nets[w], w, channels, rows, cols, held, cand.reshape(-1, w, w), **options)
    assert rc == 0 and intact
    assert_blocks_equal(got, by_position, kind)


def test_sliced_passes_reach_their_masks(nets):
    """max_chunk below n: the PNN half of the score call runs in slices, and the descriptor kernel's block offset must reach the masks."""
    w = 8
    channels, cand = pair(1), candidates(1, w)
    masks_w, masks_h = ip.hm_context_masks(w, 2, 2)
    want = by_subsets("score", nets[w], w, channels, masks_w[None], masks_h[None], cand)
    try:
        for chunk in (100, 7):
            nets[w].set_option("max_chunk", chunk)
            got = new_entry("score", nets[w], w, channels, masks_w, masks_h, cand)
            assert launches(nets[w].ctx) > 2 * (masks_w.size // chunk), "the pass did not run in slices"
            assert_blocks_equal(got, want, "max_chunk %d" % chunk)
    finally:
        nets[w].set_option("max_chunk", 0)


@pytest.mark.parametrize("w", (4, 32))
@pytest.mark.parametrize("kind", KINDS)
def test_all_masks_zero_is_the_scalar_entry(nets, kind, w):
    channels, cand = pair(1), candidates(1, w)
    rows, cols = pc.POSITIONS[w]
    zeros = np.zeros(rows.size, np.uint8)
    for options in rd_options(w) if kind == "rd_pass" else [{}]:
        rc, want, intact = entry_call(kind, nets[w], w, channels, rows, cols, (0, 0), cand[0], **options)
        assert rc == 0 and intact
        assert_blocks_equal(new_entry(kind, nets[w], w, channels, zeros, zeros, cand, **options), want, "%s width %d arrays of zeros" % (kind, w))
        rc, got, intact = entry_call(kind, nets[w], w, channels, rows, cols, (None, None), cand[0], **options)     # both NULL: nothing masked
        assert rc == 0 and intact
        assert_blocks_equal(got, want, "%s width %d both NULL" % (kind, w))


@pytest.mark.parametrize("kind", KINDS)
def test_every_refusal_comes_before_a_launch(nets, kind):
    w = 8
    channels, cand = pair(1), candidates(1, w)
    rows, cols = pc.POSITIONS[w]
    masks_w, masks_h = ip.hm_context_masks(w, 2, 2)
    options = dict(codec='switch', tskip=0) if kind == "rd_pass" else {}
    new_entry(kind, nets[w], w, channels, masks_w, masks_h, cand, **options)      # a good call first: its launches are counted
    counted = launches(nets[w].ctx)
    assert counted >= 1

    def changed(at, value):
        out = masks_w.copy()
        out[at] = value
        return out

    good_h = dev(masks_h)
    for label, held in (("a mask of 3", (dev(changed(5, 3)), good_h)), ("a mask of w + 4", (dev(changed(200, w + 4)), good_h)),
                        ("a mask of 255 in the last place", (dev(masks_w), dev(np.where(np.arange(masks_h.size) == masks_h.size - 1, 255, masks_h)
                                                                                 .astype(np.uint8)))),
                        ("d_mask_w alone NULL", (None, good_h)), ("d_mask_h alone NULL", (dev(masks_w), None))):
        rc, outs, intact = entry_call(kind, nets[w], w, channels, rows, cols, held, cand[0], **options)
        assert rc == PNN_E_ARG and intact and untouched(outs), label
        assert launches(nets[w].ctx) == counted, "%s: a refused call reset or added to the launch count" % label
    # the geometry check stays: a masked portion outside the picture is still refused
    rc, outs, intact = entry_call(kind, nets[w], w, channels, rows + (SIDE - 3 * w - rows.max() + 1), cols, (dev(masks_w), good_h), cand[0], **options)
    assert rc == PNN_E_ARG and intact and untouched(outs)
    assert launches(nets[w].ctx) == counted


@pytest.mark.parametrize("w", (4, 16))
def test_python_layer_equals_score_masks_per_mask(nets, w):
    """evaluation.score_block_masks_from_picture_pairs against score_masks_from_picture_pairs, per mask on the positions that carry it"""
    channels = pair(2)
    rows, cols = pc.POSITIONS[w]
    masks_w, masks_h = ip.hm_context_masks(w, 2, 2)
    options = dict(pc.OPTIONS, first_pass=True, transform_qps=QPS, rd_pass=True, rd_pass_signalling=True, rd_pass_transform_skip=w == 4)
    got = evaluation.score_block_masks_from_picture_pairs(channels, w, rows, cols, nets[w], util.MEAN, masks_w, masks_h, **options)
    n_pos, n = rows.size, 2 * rows.size
    compared = 0
    for mask in sorted({(int(a), int(b)) for a, b in zip(masks_w, masks_h)}):
        idx = np.flatnonzero((masks_w == mask[0]) & (masks_h == mask[1]))
        want = evaluation.score_masks_from_picture_pairs(channels, w, rows[idx], cols[idx], nets[w], util.MEAN, (mask,), **options)[mask]
        assert set(want) == set(got)
        blocks = (np.arange(2)[:, None] * n_pos + idx[None, :]).ravel()
        for key, value in want.items():
            if not isinstance(value, np.ndarray):
                continue
            axis = 0 if value.shape[0] == blocks.size else 1
            assert value.shape[axis] == blocks.size and got[key].shape[axis] == n, key
            part = np.ascontiguousarray(got[key][(slice(None),) * axis + (blocks,)])
            assert part.dtype == value.dtype and part.tobytes() == value.tobytes(), "width %d mask %s %s" % (w, mask, key)
            compared += 1
    assert compared >= 4 * 20
    assert got['mean_psnr_pnn'] == np.mean(got['psnrs_pnn']).item()


def test_python_layer_checks_its_arguments_before_the_gpu():
    class Fake:
        device, width_target = 99, 8

    channels = np.zeros((1, SIDE, SIDE, 2), np.uint8)
    rows, cols = pc.POSITIONS[8]
    masks_w, masks_h = ip.hm_context_masks(8, 2, 2)
    good = dict(channels_pair_uint8=channels, width_target=8, row_1sts=rows, col_1sts=cols, predictor=Fake(), mean_training=util.MEAN,
                masks_w=masks_w, masks_h=masks_h)
    for label, kwargs, error in (("a width", dict(width_target=12), ValueError), ("float masks", dict(masks_w=masks_w.astype(np.float32)), TypeError),
                                 ("too few masks", dict(masks_h=masks_h[:-1]), ValueError), ("a mask of 3", dict(masks_w=masks_w + 3), ValueError),
                                 ("a mask of 12", dict(masks_h=np.full_like(masks_h, 12)), ValueError),
                                 ("a negative mask", dict(masks_w=masks_w.astype(np.int64) - 4), ValueError),
                                 ("one plane", dict(channels_pair_uint8=channels[..., :1]), ValueError),
                                 ("rd_pass without signalling", dict(first_pass=True, transform_qps=QPS, rd_pass=True), ValueError)):
        arguments = dict(good)
        arguments.update(kwargs)
        with pytest.raises(error):
            evaluation.score_block_masks_from_picture_pairs(**arguments)
