"""Shared by the coding-tree tests (tests/test_cu_tree.py on the CPU, tests/test_gpu_cu_tree.py on the GPU): a recursive restatement
of include/pnn_hip.h, "the coding tree", written from that text alone -- plain Python integers and floats, the bins read from the
fixture HM recorded (tests/golden/hm_cu_tree.npz), nothing shared with csrc/pnn_cu_tree.h -- and the seeded leaves.

The seeded leaves are drawn so that the restatement ALONE gives every alternative its share.  Measured with it over the cases of CASES
together (seed 4 of the seeds 0 .. 9 tried on the CPU; `shares` recomputes them and tests/test_cu_tree.py asserts every one >= 5 %):
    share of the selected area per width 4, 8, 16, 32, 64:   19.9 %, 18.3 %, 19.7 %, 30.4 %, 11.7 %
    N x N wins / loses among the 8 x 8 CUs:                     42.1 % / 57.9 %
    split_cu_flag context 0, 1, 2 among the 21 nodes that code one: 32.9 %, 44.2 %, 22.9 %
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (4, 8, 16, 32, 64)
NO_DEPTH = 255
SEED = 4


def fixture():
    return np.load(os.path.join(HERE, "golden", "hm_cu_tree.npz"))


def hm_lambda(qp):
    return 0.57 * 2.0 ** ((qp - 12) / 3.0)


def z_index(x, y):
    """HM's z-order index of cell (x, y): bit j of x at bit 2 j, bit j of y at bit 2 j + 1."""
    z = 0
    for j in range(8):
        z |= ((x >> j) & 1) << (2 * j) | ((y >> j) & 1) << (2 * j + 1)
    return z


def z_order_brute_force(side):
    """[(x, y)] of a side x side square in z-order, by the recursion itself: four quadrants, top-left, top-right, bottom-left, bottom-right."""
    if side == 1:
        return [(0, 0)]
    half = z_order_brute_force(side // 2)
    return [(x + dx * side // 2, y + dy * side // 2) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)) for x, y in half]


def restate(leaves, qps, lambdas=None, left=None, above=None, pnn_mode=35, bins=None):
    """leaves: {w: (dist [nq, n_ctu * c], rate [nq, n_ctu * c], modes or None)} with c = (64 / w)^2 -> the entry's outputs as a dictionary."""
    bins = bins or fixture()
    nq = len(qps)
    n_ctu = leaves[64][0].shape[1]
    with_modes = all(leaves[w][2] is not None for w in WIDTHS)
    out = {"cu_depths": np.zeros((nq, n_ctu, 64), np.uint8), "part_nxn": np.zeros((nq, n_ctu, 64), np.uint8),
           "node_costs": np.zeros((nq, n_ctu, 85, 2), np.float64), "ctu_costs": np.zeros((nq, n_ctu), np.float64),
           "ctu_dists": np.zeros((nq, n_ctu), np.uint64), "ctu_rates": np.zeros((nq, n_ctu), np.uint64),
           "selected": np.zeros((nq, 5), np.uint32)}
    if with_modes:
        out["selected_pnn"] = np.zeros((nq, 5), np.uint32)
    contexts = np.zeros(3, np.int64)                      # how often each split context was met (for `shares`)
    first = {0: 0, 1: 1, 2: 5, 3: 21}
    for qi, qp in enumerate(qps):
        lam = float(hm_lambda(qp) if lambdas is None else lambdas[qi])
        split_bits, part_bits = bins["split_bits"][qp], bins["part_bits"][qp]
        for c in range(n_ctu):
            def leaf(w, x, y):                            # the block of width w at (x, y) in units of w
                count = (64 // w) ** 2
                at = c * count + z_index(x, y)
                return int(leaves[w][0][qi, at]), int(leaves[w][1][qi, at]), at

            depth_map = np.full((8, 8), 255, np.int64)    # [y][x] over the 8 x 8 cells
            nxn_map = np.zeros((8, 8), np.int64)
            edge_left = [NO_DEPTH] * 8 if left is None else [int(v) for v in left[qi, c]]
            edge_above = [NO_DEPTH] * 8 if above is None else [int(v) for v in above[qi, c]]

            def cost(d, f):
                return float(d) + lam * float(f >> 15)

            def decide(depth, x, y):                      # node at (x, y) in units of its own size 64 >> depth -> its chosen (D, F)
                size, cells = 64 >> depth, 8 >> depth
                node = first[depth] + z_index(x, y)
                d0, f0, _ = leaf(size, x, y)
                if depth == 3:
                    f0 += int(part_bits[1])
                    d1, f1 = 0, int(part_bits[0])
                    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        d, f, _ = leaf(4, 2 * x + dx, 2 * y + dy)
                        d1, f1 = d1 + d, f1 + f
                    j0, j1 = cost(d0, f0), cost(d1, f1)
                    out["node_costs"][qi, c, node] = (j0, j1)
                    depth_map[y, x] = 3
                    nxn_map[y, x] = int(j1 < j0)
                    return (d1, f1) if j1 < j0 else (d0, f0)
                cx, cy = x * cells, y * cells             # the node's top-left cell
                l = depth_map[cy, cx - 1] if cx else edge_left[cy]
                a = depth_map[cy - 1, cx] if cy else edge_above[cx]
                ctx = int(l != NO_DEPTH and l > depth) + int(a != NO_DEPTH and a > depth)
                contexts[ctx] += 1
                f0 += int(split_bits[ctx][0])
                d1, f1 = 0, int(split_bits[ctx][1])
                for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    d, f = decide(depth + 1, 2 * x + dx, 2 * y + dy)
                    d1, f1 = d1 + d, f1 + f
                j0, j1 = cost(d0, f0), cost(d1, f1)
                out["node_costs"][qi, c, node] = (j0, j1)
                if j1 < j0:
                    return d1, f1
                depth_map[cy:cy + cells, cx:cx + cells] = depth
                nxn_map[cy:cy + cells, cx:cx + cells] = 0
                return d0, f0

            d, f = decide(0, 0, 0)
            out["ctu_dists"][qi, c], out["ctu_rates"][qi, c] = d, f
            out["ctu_costs"][qi, c] = out["node_costs"][qi, c, 0].min()
            for y in range(8):
                for x in range(8):
                    out["cu_depths"][qi, c, z_index(x, y)] = depth_map[y, x]
                    out["part_nxn"][qi, c, z_index(x, y)] = nxn_map[y, x]
                    depth = int(depth_map[y, x])
                    cells = 8 >> depth
                    if x % cells or y % cells:
                        continue
                    if depth == 3 and nxn_map[y, x]:
                        blocks = [leaf(4, 2 * x + dx, 2 * y + dy)[2] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
                        k = 0
                    else:
                        blocks = [leaf(64 >> depth, x // cells, y // cells)[2]]
                        k = 4 - depth
                    out["selected"][qi, k] += len(blocks)
                    if with_modes:
                        out["selected_pnn"][qi, k] += sum(int(leaves[WIDTHS[k]][2][qi, at]) == pnn_mode for at in blocks)
    out["split_contexts"] = contexts
    return out


def seeded_leaves(n_ctu, qps, lambdas=None, seed=SEED, modes=True):
    """{w: (dist uint32, rate uint64, modes uint8 or None)}, each [nb_qps, n_ctu * (64 / w)^2]: a positive field over the 4 x 4 cells of
    every CTU whose sums make a block and its four sub-blocks cost about the same, a per-block factor that decides between them, rates
    of a few to a few hundred bits with all 15 fractional bits in use; both scale with the QP's lambda so that neither term rules."""
    rng = np.random.default_rng(seed)
    nq = len(qps)
    leaves = {}
    field = rng.gamma(2.0, 1.0, (nq, n_ctu, 16, 16))      # [y][x] over the 4 x 4 cells
    busy = rng.random((nq, n_ctu, 2, 2)) < 0.5            # quadrants with detail: there small blocks pay off
    for w in WIDTHS:
        side, per = 64 // w, w // 4
        sums = field.reshape(nq, n_ctu, side, per, side, per).sum(axis=(3, 5))          # [y][x] in units of w
        detail = np.repeat(np.repeat(busy, max(side // 2, 1), axis=2), max(side // 2, 1), axis=3)[:, :, :side, :side] if side > 1 \
            else busy.any(axis=(2, 3))[:, :, None, None]
        penalty = np.where(detail, 1.0 + 0.14 * np.log2(w / 4.0), 1.0 - 0.09 * np.log2(w / 4.0))
        factor = penalty * np.exp(rng.normal(0.0, 0.25, sums.shape))
        lam = np.array([hm_lambda(q) if lambdas is None else lambdas[i] for i, q in enumerate(qps)])[:, None, None, None]
        dist = np.floor(sums * factor * (40.0 * lam + 25.0))
        rate = np.floor((6.0 + sums * rng.uniform(0.2, 1.2, sums.shape)) * 32768.0) + rng.integers(0, 32768, sums.shape)
        order = [z for z in range(side * side)]
        xy = z_order_brute_force(side)
        d = np.stack([dist[:, :, xy[z][1], xy[z][0]] for z in order], axis=2).reshape(nq, n_ctu * side * side)
        r = np.stack([rate[:, :, xy[z][1], xy[z][0]] for z in order], axis=2).reshape(nq, n_ctu * side * side)
        m = rng.choice(np.array([0, 1, 10, 18, 26, 35], np.uint8), size=d.shape) if modes else None
        leaves[w] = (np.ascontiguousarray(d.astype(np.uint32)), np.ascontiguousarray(r.astype(np.uint64)), m)
    return leaves


def seeded_edges(n_ctu, nq, seed=SEED):
    rng = np.random.default_rng(seed + 1000)
    values = np.array([0, 1, 2, 3, 3, NO_DEPTH], np.uint8)
    return rng.choice(values, size=(nq, n_ctu, 8)), rng.choice(values, size=(nq, n_ctu, 8))


EIGHT_QPS = (0, 12, 22, 27, 32, 37, 45, 51)
# (name, n_ctu, qps, the caller's lambdas or None for HM's, edges given)
CASES = (("one CTU, one QP", 1, (32,), None, False),
         ("one CTU, eight QPs, edges", 1, EIGHT_QPS, None, True),
         ("three CTUs, one QP, own lambda, edges", 3, (27,), (31.5,), True),
         ("three CTUs, eight QPs", 3, EIGHT_QPS, None, False),
         ("three CTUs, eight QPs, own lambdas, edges", 3, EIGHT_QPS, tuple(0.4 * 1.3 ** q for q in (0, 3, 7, 11, 14, 17, 20, 23)), True))


def case_inputs(case, modes=True):
    name, n_ctu, qps, lambdas, edges = case
    leaves = seeded_leaves(n_ctu, qps, lambdas, SEED + len(name), modes)
    left, above = seeded_edges(n_ctu, len(qps), SEED + len(name)) if edges else (None, None)
    return leaves, qps, lambdas, left, above


def shares(results):
    """The conditions' shares over the restatement's outputs of several cases: (area per width [5], N x N wins, N x N loses, contexts [3])."""
    area, nxn_wins, cus8, contexts = np.zeros(5), 0, 0, np.zeros(3)
    for r in results:
        area += r["selected"].sum(axis=0) * np.array([w * w for w in WIDTHS], np.float64)
        costs = r["node_costs"][:, :, 21:]
        nxn_wins += int((costs[..., 1] < costs[..., 0]).sum())
        cus8 += costs[..., 0].size
        contexts += r["split_contexts"]
    return area / area.sum(), nxn_wins / cus8, 1.0 - nxn_wins / cus8, contexts / contexts.sum()


def as_rd_pass_tuples(leaves):
    """The restatement's leaves as intraprediction.cu_tree takes them: (sses, rates, side_rates, modes), the rate split in two parts."""
    return {w: (d, r - r // np.uint64(3), r // np.uint64(3), m) for w, (d, r, m) in leaves.items()}
