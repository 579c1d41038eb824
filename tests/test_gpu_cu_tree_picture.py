"""The coding tree over whole pictures on the GPU: cu_tree_picture_kernel behind pnn_cu_tree_picture_device,
called raw with every output and the workspace between guard bytes, at zero tolerance against the host twin pnn_cu_tree_picture_host
(which tests/test_cu_tree_picture.py holds to the existing entry called CTU by CTU), over CASES and EXTRA_CASES (anti-diagonals of up
to three CTUs, one row and one column of five, three images); cu_depths NULL (the maps in the workspace) and given; the launch count of an accepted call; every refusal before a launch, by the launch count, with outputs and workspace untouched;
intraprediction.cu_tree_picture(device=0) against device=None; cu_tree_leaves_kernel behind pnn_cu_tree_leaves_device against the numpy
expression evaluation.coding_tree_from_scores builds its leaves with."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cu_tree_cases as cc
from tests import cu_tree_picture_cases as pc
from tests import util
from tests.util import GUARD, PAD, PNN_E_ARG, untouched

pytestmark = pytest.mark.gpu

WIDTHS = pc.WIDTHS
EIGHT = pc.EIGHT_QPS
POINTERS = ctypes.c_void_p * 5
NAMES = [name for name, _ in ip.CU_TREE_PICTURE_OUTPUTS]
ALL = (True,) * 10
NO_PNN = (True,) * 7 + (False, True, True)


def launches():
    count = ctypes.c_int(-1)
    assert _lib.lib().pnn_last_call_stats(ip._context(0), None, None, ctypes.byref(count)) == 0
    return count.value


def host_call(leaves, qps, lambdas, n_images, rows, cols, modes, pnn_mode):
    """pnn_cu_tree_picture_host, every output (selected_pnn only with modes): the yardstick of this file"""
    nq = len(qps)
    outs = [np.zeros(shape, dtype) for (_, dtype), shape in zip(ip.CU_TREE_PICTURE_OUTPUTS, ip.cu_tree_picture_shapes(nq, n_images, rows, cols))]
    c_lambdas = None if lambdas is None else (ctypes.c_double * nq)(*lambdas)
    rc = _lib.lib().pnn_cu_tree_picture_host(
        (ctypes.c_int * nq)(*qps), nq, c_lambdas, n_images, rows, cols, POINTERS(*[leaves[w][0].ctypes.data for w in WIDTHS]),
        POINTERS(*[leaves[w][1].ctypes.data for w in WIDTHS]), POINTERS(*[leaves[w][2].ctypes.data for w in WIDTHS]) if modes else None,
        pnn_mode, *[o.ctypes.data if modes or i != 7 else None for i, o in enumerate(outs)])
    assert rc == 0
    return outs


def device_call(leaves, qps, lambdas, n_images, rows, cols, modes, pnn_mode, wanted, nq=None, drop=None, shift=None, workspace="exact"):
    """Raw ABI call of pnn_cu_tree_picture_device through the guarded call of tests/util.py, the workspace between guard bytes too.
    drop = (0 dists / 1 rates / 2 modes, width index or None): a NULL in its place; shift = (kind, width index, bytes): a misaligned
    leaf array; workspace: "exact", "short" (one byte less), "misaligned" (8 bytes on) or "null".  Returns (rc, outputs, intact,
    whether the workspace between its guards was left untouched)."""
    import torch
    nq = len(qps) if nq is None else nq
    shapes_nq, n_ctu = len(qps), leaves[64][0].shape[1]
    held = {w: [None if a is None else util.dev(a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int64) if a.dtype == np.uint64 else a)
                for a in leaves[w]] for w in WIDTHS}
    tables = [[util.ptr(held[w][k]) for w in WIDTHS] for k in range(3)]
    if drop is not None and drop[1] is not None:
        tables[drop[0]][drop[1]] = None
    if shift is not None:
        tables[shift[0]][shift[1]] += shift[2]
    tables = [None if (drop is not None and drop[0] == k and drop[1] is None) or (k == 2 and not modes) else POINTERS(*t) for k, t in enumerate(tables)]
    c_lambdas = None if lambdas is None else (ctypes.c_double * len(lambdas))(*lambdas)
    front = (ip._context(0), (ctypes.c_int * len(qps))(*qps), nq, c_lambdas, n_images, rows, cols, *tables, pnn_mode)
    specs = [(dtype, shape) for (_, dtype), shape in zip(ip.CU_TREE_PICTURE_OUTPUTS,
                                                         ip.cu_tree_shapes(shapes_nq, n_ctu) + ((shapes_nq, max(n_images, 1)),) * 2)]
    need = shapes_nq * n_ctu * 64
    d_workspace = torch.full((2 * PAD + need,), GUARD, dtype=torch.uint8, device="cuda")
    address = {"exact": d_workspace.data_ptr() + PAD, "short": d_workspace.data_ptr() + PAD, "misaligned": d_workspace.data_ptr() + PAD + 8,
               "null": None}[workspace]
    nbytes = {"exact": need, "short": need - 1, "misaligned": need + 8, "null": need}[workspace]
    rc, outs, intact = util.call("pnn_cu_tree_picture_device", front, (), specs, wanted, after=(address, nbytes))
    torch.cuda.synchronize()
    raw = d_workspace.cpu().numpy()
    intact = intact and bool((raw[:PAD] == GUARD).all() and (raw[-PAD:] == GUARD).all())
    return rc, outs, intact, bool((raw == GUARD).all())


# every grid of the CPU cases, both image counts, 1 and 8 QPs, HM's lambda and the caller's, modes present and absent; the extra cases
# add anti-diagonals of 1, 2, 3, 3, 2, 1 CTUs under three images, and one row and one column of five CTUs
@pytest.mark.parametrize("case", pc.CASES + pc.EXTRA_CASES, ids=[c[0] for c in pc.CASES + pc.EXTRA_CASES])
@pytest.mark.parametrize("maps_given", [True, False], ids=["cu_depths given", "cu_depths NULL"])
def test_device_entry_equals_host_twin(case, maps_given):
    name, n_images, rows, cols, qps, lambdas, modes = case
    leaves = pc.case_leaves(case)
    pnn_mode = 35 if len(name) % 2 else 18
    want = host_call(leaves, qps, lambdas, n_images, rows, cols, modes, pnn_mode)
    wanted = tuple(w and (maps_given or i != 0) for i, w in enumerate(ALL if modes else NO_PNN))
    rc, outs, intact, workspace_untouched = device_call(leaves, qps, lambdas, n_images, rows, cols, modes, pnn_mode, wanted)
    assert rc == 0 and intact
    assert launches() == rows + cols - 1
    assert workspace_untouched == maps_given, "the maps live in the workspace exactly when cu_depths is NULL"
    for key, g, w, asked in zip(NAMES, outs, want, wanted):
        if asked:
            assert g.tobytes() == w.tobytes(), "%s %s: %d differing values" % (name, key, (g != w).sum())
    assert int(outs[6].sum()) > 0


def test_each_output_alone():
    case = pc.CASES[5]                                    # 2x3, two images, eight QPs, own lambdas
    name, n_images, rows, cols, qps, lambdas, modes = case
    leaves = pc.case_leaves(case)
    want = host_call(leaves, qps, lambdas, n_images, rows, cols, True, 35)
    for i, key in enumerate(NAMES):
        wanted = tuple(k == i for k in range(10))
        rc, outs, intact, _ = device_call(leaves, qps, lambdas, n_images, rows, cols, True, 35, wanted)
        assert rc == 0 and intact, key
        assert outs[i].tobytes() == want[i].tobytes(), key


def test_python_layer_device_equals_host():
    for case in (pc.CASES[2], pc.CASES[6]):
        name, n_images, rows, cols, qps, lambdas, modes = case
        tuples = cc.as_rd_pass_tuples(pc.case_leaves(case))
        util.assert_same_dictionary(ip.cu_tree_picture(tuples, qps, n_images, rows, cols, lambdas, device=0),
                                    ip.cu_tree_picture(tuples, qps, n_images, rows, cols, lambdas), name)
    bare = {w: t[:3] + (None,) for w, t in tuples.items()}
    util.assert_same_dictionary(ip.cu_tree_picture(bare, qps, n_images, rows, cols, lambdas, pnn_mode=18, device=0),
                                ip.cu_tree_picture(bare, qps, n_images, rows, cols, lambdas, pnn_mode=18), "no modes")


def test_every_refusal_comes_before_a_launch():
    qps = (22, 37)
    leaves = pc.near_tie_leaves(6, qps, None, 9)
    good = dict(leaves=leaves, qps=qps, lambdas=None, n_images=1, rows=2, cols=3, modes=True, pnn_mode=35, wanted=ALL)
    rc, outs, intact, _ = device_call(**good)             # a good call first: its launches are counted
    assert rc == 0 and intact and launches() == 4
    nan = (float("nan"), 1.)
    for label, kwargs in (("no QP", dict(nq=0)), ("nine QPs", dict(nq=9)), ("QP 52", dict(qps=(22, 52))), ("no image", dict(n_images=0)),
                          ("no CTU row", dict(rows=0)), ("negative CTU columns", dict(cols=-3)),
                          ("n_ctu beyond an int", dict(n_images=65536, rows=65536, cols=1)), ("no dists", dict(drop=(0, None))),
                          ("no rates", dict(drop=(1, None))), ("a dist array missing", dict(drop=(0, 3))), ("a rate array missing", dict(drop=(1, 0))),
                          ("a mode array missing", dict(drop=(2, 4))), ("lambda nan", dict(lambdas=nan)), ("lambda inf", dict(lambdas=(1., float("inf")))),
                          ("lambda below 0", dict(lambdas=(-1e-9, 1.))), ("selected_pnn without modes", dict(modes=False)),
                          ("no output", dict(wanted=(False,) * 10)), ("pnn_mode 256", dict(pnn_mode=256)),
                          ("a misaligned dist array", dict(shift=(0, 2, 2))), ("a misaligned rate array", dict(shift=(1, 4, 4))),
                          ("workspace one byte short", dict(workspace="short")), ("workspace misaligned", dict(workspace="misaligned")),
                          ("workspace NULL", dict(workspace="null"))):
        arguments = dict(good)
        arguments.update(kwargs)
        rc, outs, intact, workspace_untouched = device_call(**arguments)
        assert rc == PNN_E_ARG and intact and untouched(outs) and workspace_untouched, label
        assert launches() == 4, "%s: a refused call reset or added to the launch count" % label


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("nq", [1, 8])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one element on"])
def test_leaves_entry_equals_the_numpy_expression(w, nq, offset):
    """n = one CTU's blocks.  `offset` moves every input one element on, off the 16-byte alignment of the vector path; at w = 64 and
    one QP the single element goes through the partial group."""
    leaves_entry_equals_the_numpy_expression(w, nq, offset, (64 // w) ** 2)


@pytest.mark.parametrize("w, nq", [(4, 8), (64, 1)])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one element on"])
def test_leaves_entry_over_three_ctus(w, nq, offset):
    """n = three CTUs' blocks, as coding_tree_from_pictures calls the entry with every image's blocks at once: 768 blocks x 8 QPs at
    w = 4 (6144 elements: six whole workgroups of 256 lanes x 4 elements) and 3 blocks x 1 QP at w = 64 (one partial group of three)."""
    leaves_entry_equals_the_numpy_expression(w, nq, offset, 3 * (64 // w) ** 2)


def leaves_entry_equals_the_numpy_expression(w, nq, offset, n):
    import torch
    rng = np.random.default_rng(100 * w + nq)
    sses = rng.integers(0, 2 ** 32, nq * n + 1, dtype=np.uint64).astype(np.uint32)
    rates = rng.integers(0, 2 ** 40, nq * n + 1, dtype=np.uint64)
    side_rates = rng.integers(0, 2 ** 20, nq * n + 1, dtype=np.uint64)
    modes = rng.integers(0, 36, nq * n + 4).astype(np.uint8)
    held = [util.dev(sses.view(np.int32)), util.dev(rates.view(np.int64)), util.dev(side_rates.view(np.int64)), util.dev(modes)]
    front = (ip._context(0), w, n, nq, held[0].data_ptr() + 4 * offset, held[1].data_ptr() + 8 * offset, held[2].data_ptr() + 8 * offset,
             held[3].data_ptr() + 4 * offset)
    specs = [(np.uint32, (nq, n)), (np.uint64, (nq, n)), (np.uint8, (nq, n))]
    rc, outs, intact = util.call("pnn_cu_tree_leaves_device", front, (), specs, (True,) * 3)
    torch.cuda.synchronize()
    assert rc == 0 and intact and launches() == 1
    sl = slice(offset, offset + nq * n)
    assert np.array_equal(outs[0], sses[sl].reshape(nq, n))
    assert np.array_equal(outs[1], (rates[sl] + side_rates[sl]).reshape(nq, n))                 # coding_tree_from_scores: rate + side rate
    assert np.array_equal(outs[2], modes[4 * offset:4 * offset + nq * n].reshape(nq, n))


def test_leaves_entry_refusals():
    import torch
    held = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(4)]
    good = dict(w=64, n=1, nq=1, pointers=[t.data_ptr() for t in held])
    specs = [(np.uint32, (1, 1)), (np.uint64, (1, 1)), (np.uint8, (1, 1))]
    for label, kwargs, wanted in (("width 12", dict(w=12), (True,) * 3), ("no block", dict(n=0), (True,) * 3), ("half a CTU", dict(w=8, n=32), (True,) * 3),
                                  ("no QP", dict(nq=0), (True,) * 3), ("nine QPs", dict(nq=9), (True,) * 3),
                                  ("a NULL input", dict(pointers=[held[0].data_ptr(), None, held[2].data_ptr(), held[3].data_ptr()]), (True,) * 3),
                                  ("a misaligned input", dict(pointers=[held[0].data_ptr() + 2] + [t.data_ptr() for t in held[1:]]), (True,) * 3),
                                  ("a NULL output", dict(), (True, False, True))):
        arguments = dict(good)
        arguments.update(kwargs)
        rc, outs, intact = util.call("pnn_cu_tree_leaves_device", (ip._context(0), arguments["w"], arguments["n"], arguments["nq"],
                                                                   *arguments["pointers"]), (), specs, wanted)
        assert rc == PNN_E_ARG and intact and untouched(outs), label
