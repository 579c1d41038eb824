"""The coding-tree pass on the CPU (include/pnn_hip.h, "the coding tree"): the host twin pnn_cu_tree_host through
intraprediction.cu_tree against the recursive restatement of tests/cu_tree_cases.py (doubles by bit pattern), the conditions on the
seeded leaves, the known answers, every refusal, and ctu_block_positions against a brute-force z-order."""
import ctypes

import numpy as np
import pytest

from context_adaptive_neural_network_based_prediction_amd import _lib
from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cu_tree_cases as cc

WIDTHS = cc.WIDTHS
KEYS = ("cu_depths", "part_nxn", "node_costs", "ctu_costs", "ctu_dists", "ctu_rates", "selected", "selected_pnn")


@pytest.fixture(scope="module")
def restated():
    """The restatement's answer to every case, computed once"""
    return {case[0]: cc.restate(*cc.case_inputs(case)) for case in cc.CASES}


def assert_equal_outputs(got, want, label):
    for key in KEYS:
        if key not in want:
            assert key not in got, (label, key)
            continue
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (label, key)
        assert got[key].tobytes() == want[key].tobytes(), "%s %s: %d differing values" % (label, key, (got[key] != want[key]).sum())


@pytest.mark.parametrize("case", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_host_twin_equals_the_restatement(case, restated):
    leaves, qps, lambdas, left, above = cc.case_inputs(case)
    got = ip.cu_tree(cc.as_rd_pass_tuples(leaves), qps, lambdas, left, above)
    assert_equal_outputs(got, restated[case[0]], case[0])
    selected = got["selected"].astype(np.float64)
    assert np.array_equal(got["area_share"], selected * np.array([w * w for w in WIDTHS]) / (case[1] * 4096.0))
    assert np.allclose(got["area_share"].sum(axis=1), 1.0)
    nan = selected == 0
    assert np.isnan(got["frequency_selected_pnn"][nan]).all()
    assert np.array_equal(got["frequency_selected_pnn"][~nan], (got["selected_pnn"] / np.where(nan, 1, selected))[~nan])
    want_lambdas = [cc.hm_lambda(q) for q in qps] if lambdas is None else list(lambdas)
    assert np.array_equal(got["lambdas"], np.array(want_lambdas))


def test_other_pnn_mode_and_no_modes(restated):
    case = cc.CASES[2]
    leaves, qps, lambdas, left, above = cc.case_inputs(case)
    got = ip.cu_tree(cc.as_rd_pass_tuples(leaves), qps, lambdas, left, above, pnn_mode=18)
    assert_equal_outputs(got, cc.restate(leaves, qps, lambdas, left, above, pnn_mode=18), "pnn_mode 18")
    assert not np.array_equal(got["selected_pnn"], restated[case[0]]["selected_pnn"])
    bare = {w: (d, r, None) for w, (d, r, m) in leaves.items()}
    got = ip.cu_tree(cc.as_rd_pass_tuples(bare), qps, lambdas, left, above)
    assert "selected_pnn" not in got and "frequency_selected_pnn" not in got
    assert_equal_outputs(got, cc.restate(bare, qps, lambdas, left, above), "no modes")


def test_rd_pass_dictionaries_are_accepted(restated):
    case = cc.CASES[0]
    leaves, qps, lambdas, left, above = cc.case_inputs(case)
    as_dicts = {w: dict(zip(("sses", "rates", "side_rates", "modes"), t), costs=None) for w, t in cc.as_rd_pass_tuples(leaves).items()}
    assert_equal_outputs(ip.cu_tree(as_dicts, qps, lambdas, left, above), restated[case[0]], "dictionaries")


def test_every_alternative_has_its_share(restated):
    """The conditions on the seeded leaves, from the restatement alone (the figures are written in tests/cu_tree_cases.py)"""
    area, nxn_wins, nxn_loses, contexts = cc.shares(list(restated.values()))
    print("area %s, N x N wins %.3f loses %.3f, contexts %s" % (area, nxn_wins, nxn_loses, contexts))
    assert (area >= 0.05).all(), area
    assert nxn_wins >= 0.05 and nxn_loses >= 0.05
    assert (contexts >= 0.05).all(), contexts


def constant_leaves(n_ctu, nq, dist, rate):
    """{w: (dist, rate, None)} with one value per width (dictionaries by width)"""
    return {w: (np.full((nq, n_ctu * (64 // w) ** 2), dist[w], np.uint32), np.full((nq, n_ctu * (64 // w) ** 2), rate[w], np.uint64), None)
            for w in WIDTHS}


def run(leaves, qps, lambdas=None, left=None, above=None):
    return ip.cu_tree({w: (d, r, np.zeros_like(r), m) for w, (d, r, m) in leaves.items()}, qps, lambdas, left, above)


@pytest.mark.parametrize("lambdas", [None, (0., 0.)])
def test_all_zero_leaves_give_one_cu_per_ctu(lambdas):
    """D = F = 0 everywhere: the unsplit alternative never costs more bits than the split one, and a tie stays unsplit"""
    zero = dict.fromkeys(WIDTHS, 0)
    got = run(constant_leaves(3, 2, zero, zero), (22, 37), lambdas)
    assert (got["cu_depths"] == 0).all() and (got["part_nxn"] == 0).all()
    assert np.array_equal(got["selected"], np.array([[0, 0, 0, 0, 3]] * 2, np.uint32))
    assert (got["ctu_dists"] == 0).all()


def test_only_the_4x4_leaves_cheap_gives_n_x_n_everywhere():
    dist = {4: 0, 8: 10 ** 6, 16: 10 ** 6, 32: 10 ** 6, 64: 10 ** 6}
    got = run(constant_leaves(3, 2, dist, dict.fromkeys(WIDTHS, 0)), (22, 37))
    assert (got["cu_depths"] == 3).all() and (got["part_nxn"] == 1).all()
    assert np.array_equal(got["selected"], np.array([[256 * 3, 0, 0, 0, 0]] * 2, np.uint32))


def test_lambda_zero_gives_the_partition_of_least_distortion():
    leaves, qps, _, left, above = cc.case_inputs(cc.CASES[3])
    got = ip.cu_tree(cc.as_rd_pass_tuples(leaves), qps, (0.,) * len(qps), left, above)
    for qi in range(len(qps)):
        for c in range(3):
            least = {}
            for w in WIDTHS:                              # bottom-up: the least distortion of every block, ties to the larger block
                count = (64 // w) ** 2
                own = leaves[w][0][qi, c * count:(c + 1) * count].astype(np.int64)
                if w == 4:
                    least[w] = own
                else:
                    below = least[w // 2].reshape(count, 4).sum(axis=1)
                    least[w] = np.where(below < own, below, own)
            assert int(got["ctu_dists"][qi, c]) == int(least[64][0])
            assert got["ctu_costs"][qi, c] == float(least[64][0])


def test_one_edge_cell_flips_the_root():
    """One CTU, lambda 1, D = 0 below the root: the root stays whole on a tie with no neighbour and splits once the first cell of its
    left edge holds a deeper CU, because the context moves from 0 to 1 and the unsplit bin becomes dearer, the split bin cheaper."""
    qp = 30
    bins = cc.fixture()["split_bits"][qp].astype(np.int64)

    def whole_bits(root_ctx, first_child_ctx):
        # every node below the root stays unsplit (no distortion, fewer bits); children 1 .. 3 of the root see no deeper neighbour
        children = int(bins[first_child_ctx][0]) + 3 * int(bins[0][0])
        return int(bins[root_ctx][0]) >> 15, (children + int(bins[root_ctx][1])) >> 15

    unsplit0, split0 = whole_bits(0, 0)
    unsplit1, split1 = whole_bits(1, 1)
    d = split0 - unsplit0                                 # a tie without the neighbour
    assert d > 0 and d + unsplit1 > split1, "the bins of QP %d do not allow the construction" % qp
    dist = {4: 0, 8: 0, 16: 0, 32: 0, 64: d}
    leaves = constant_leaves(1, 1, dist, dict.fromkeys(WIDTHS, 0))
    left = np.full((1, 1, 8), 255, np.uint8)
    alone = run(leaves, (qp,), (1.,), left, None)
    assert (alone["cu_depths"] == 0).all() and alone["node_costs"][0, 0, 0, 0] == alone["node_costs"][0, 0, 0, 1]
    left[0, 0, 0] = 3
    beside = run(leaves, (qp,), (1.,), left, None)
    assert (beside["cu_depths"] == 1).all()
    assert beside["node_costs"][0, 0, 0].tolist() == [float(d + unsplit1), float(split1)]


def test_the_childrens_fractions_carry():
    """Four 4 x 4 units of F = 0x6000 charge 3 whole bits together, not 0: the shift by 15 happens once per comparison"""
    qp = 30
    part = cc.fixture()["part_bits"][qp].astype(np.int64)
    leaves = constant_leaves(1, 1, dict.fromkeys(WIDTHS, 0), {4: 0x6000, 8: 0, 16: 0, 32: 0, 64: 0})
    got = run(leaves, (qp,), (1.,))
    want = float((4 * 0x6000 + int(part[0])) >> 15)
    assert want == 3.0 + float((int(part[0]) + 0) >> 15) and want >= 3.0
    assert (got["node_costs"][0, 0, 21:, 1] == want).all()
    assert (got["node_costs"][0, 0, 21:, 0] == float(int(part[1]) >> 15)).all()


def raw_host_call(nq=1, n_ctu=1, qps=(30,), lambdas=None, drop=None, modes=True, left=None, above=None, pnn_mode=35, outputs=range(8)):
    """pnn_cu_tree_host on zero leaves; `drop` = (which of dists / rates / modes, width index or None for the whole array)"""
    L = _lib.lib()
    pointers = ctypes.c_void_p * 5
    arrays = {"dists": [np.zeros((max(nq, 1), max(n_ctu, 1) * (64 // w) ** 2), np.uint32) for w in WIDTHS],
              "rates": [np.zeros((max(nq, 1), max(n_ctu, 1) * (64 // w) ** 2), np.uint64) for w in WIDTHS],
              "modes": [np.zeros((max(nq, 1), max(n_ctu, 1) * (64 // w) ** 2), np.uint8) for w in WIDTHS]}
    tables = {}
    for name, list_ in arrays.items():
        values = [a.ctypes.data for a in list_]
        if drop and drop[0] == name and drop[1] is not None:
            values[drop[1]] = None
        tables[name] = None if (drop and drop[0] == name and drop[1] is None) or (name == "modes" and not modes) else pointers(*values)
    shapes = ip.cu_tree_shapes(max(nq, 1), max(n_ctu, 1))
    outs = [np.full(shape, 7, dtype) for (_, dtype), shape in zip(ip.CU_TREE_OUTPUTS, shapes)]
    c_lambdas = None if lambdas is None else (ctypes.c_double * len(lambdas))(*lambdas)
    rc = L.pnn_cu_tree_host((ctypes.c_int * len(qps))(*qps), nq, c_lambdas, n_ctu, tables["dists"], tables["rates"], tables["modes"],
                            None if left is None else left.ctypes.data, None if above is None else above.ctypes.data, pnn_mode,
                            *[o.ctypes.data if i in outputs else None for i, o in enumerate(outs)])
    return rc, outs, arrays


REFUSALS = (dict(nq=0), dict(nq=9, qps=(30,) * 9), dict(qps=(52,)), dict(qps=(-1,)), dict(n_ctu=0), dict(n_ctu=-3),
            dict(drop=("dists", None)), dict(drop=("rates", None)), dict(drop=("dists", 0)), dict(drop=("dists", 4)), dict(drop=("rates", 2)),
            dict(drop=("modes", 3)), dict(lambdas=(float("nan"),)), dict(lambdas=(float("inf"),)), dict(lambdas=(-0.5,)),
            dict(left=np.array([0, 1, 2, 3, 4, 0, 0, 0], np.uint8)), dict(above=np.array([255, 254, 0, 0, 0, 0, 0, 0], np.uint8)),
            dict(modes=False, outputs=(7,)), dict(modes=False, outputs=range(8)), dict(outputs=()), dict(pnn_mode=256), dict(pnn_mode=-1))


@pytest.mark.parametrize("arguments", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals(arguments):
    rc, outs, _ = raw_host_call(**arguments)
    assert rc == -1
    assert all((o == 7).all() for o in outs), "a refused call wrote an output"


def test_good_raw_calls_and_each_output_alone():
    rc, all_outs, _ = raw_host_call(lambdas=(0.,), left=np.array([0, 1, 2, 3, 255, 0, 0, 0], np.uint8))
    assert rc == 0
    for i in range(8):
        rc, outs, _ = raw_host_call(lambdas=(0.,), left=np.array([0, 1, 2, 3, 255, 0, 0, 0], np.uint8), outputs=(i,))
        assert rc == 0 and outs[i].tobytes() == all_outs[i].tobytes()
        assert all((o == 7).all() for k, o in enumerate(outs) if k != i)
    assert raw_host_call(modes=False, outputs=range(7))[0] == 0


def test_python_layer_refuses_before_the_library():
    leaves, qps, lambdas, left, above = cc.case_inputs(cc.CASES[0])
    tuples = cc.as_rd_pass_tuples(leaves)
    with pytest.raises(ValueError):
        ip.cu_tree({w: tuples[w] for w in (4, 8, 16, 32)}, qps)
    with pytest.raises(ValueError):
        ip.cu_tree(tuples, (22, 37))                      # the leaves hold one QP
    with pytest.raises(ValueError):
        ip.cu_tree(tuples, qps, lambdas=(-1.,))
    with pytest.raises(ValueError):
        ip.cu_tree(tuples, qps, left_depths=np.full((1, 1, 8), 4))
    with pytest.raises(ValueError):
        ip.cu_tree(tuples, qps, above_depths=np.zeros((1, 2, 8), np.uint8))
    with pytest.raises(ValueError):
        ip.cu_tree(tuples, qps, pnn_mode=300)
    with pytest.raises(ValueError):
        ip.cu_tree({w: tuple(a[:, :-1] for a in t) if w == 8 else t for w, t in tuples.items()}, qps)
    with pytest.raises(ValueError):
        ip.cu_tree_bins(52)


@pytest.mark.parametrize("w", WIDTHS)
def test_ctu_block_positions_against_brute_force(w):
    ctu_rows, ctu_cols = np.array([64, 64, 192]), np.array([64, 128, 320])
    rows, cols = ip.ctu_block_positions(w, ctu_rows, ctu_cols)
    order = cc.z_order_brute_force(64 // w)
    want_rows = [r + y * w - w for r in ctu_rows for x, y in order]
    want_cols = [c + x * w - w for c in ctu_cols for x, y in order]
    assert rows.dtype == np.int64 and rows.tolist() == want_rows and cols.tolist() == want_cols
    # the blocks tile the CTUs exactly
    covered = np.zeros((3, 64, 64), np.int64)
    for i, (r, c) in enumerate(zip(rows + w, cols + w)):
        k = i // len(order)
        covered[k, r - ctu_rows[k]:r - ctu_rows[k] + w, c - ctu_cols[k]:c - ctu_cols[k] + w] += 1
    assert (covered == 1).all()
    with pytest.raises(ValueError):
        ip.ctu_block_positions(w, np.array([w - 1]), np.array([64]))
    with pytest.raises(ValueError):
        ip.ctu_block_positions(12, ctu_rows, ctu_cols)
