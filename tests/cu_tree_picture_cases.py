"""Shared by the tests of the coding tree over whole pictures (tests/test_cu_tree_picture.py on the CPU, tests/test_gpu_cu_tree_picture.py
on the GPU): the independent yardstick, the seeded cases and the conditions that keep them from being vacuous.

The yardstick is the existing entry pnn_cu_tree_host, through intraprediction.cu_tree: it is called CTU BY CTU in raster order, one CTU
per call, and its left_depths / above_depths are cut here in numpy from the maps it returned for the CTU left of and the CTU above the
one it is asked about.  Nothing of the picture entries is used.

Conditions, computed from the yardstick alone over the cases of CASES together (`conditions`; tests/test_cu_tree_picture.py asserts
each).  Seeds 0 .. 9 were tried on the CPU; seed 3 is the only one of them that meets all four -- with each of the others at least
one multi-CTU case, mostly the 1x2 or the 2x1 one, kept every map of its unchained decision.  A "node"
is one of the 21 nodes of depths 0 .. 2 of a CTU that has a CTU left of it or above it in its image; its context is the one the
decision read when the node was decided, replayed here from the yardstick's node costs; it "reads a cross-CTU neighbour" when it
touches the CTU's left or top edge and a CTU lies beyond it:
    nodes whose context differs from the one absent edges give:                 18.0 %
    nodes that read a cross-CTU neighbour and get context 0, 1, 2:              15.8 %, 18.1 %, 6.7 %
    multi-CTU cases, (QP, CTU) maps that differ from the unchained decision:    1, 1, 5, 2, 14, 6 (in CASES' order)
    share of the selected area per width 4, 8, 16, 32, 64:                      15.7 %, 15.1 %, 15.0 %, 26.2 %, 28.0 %
EXTRA_CASES (longer diagonals, one row, one column, three images) stand apart from these figures; their own floor and the seeds tried
are written beside them.

The evaluator's cases (tests/test_gpu_cu_tree_picture_evaluator.py) follow below: the 2 x 2 picture of one image, then EVALUATOR_CASES
-- two images on a 1 x 2 and a 2 x 1 grid, and transform skip on the 2 x 2 grid -- with a yardstick built on the host image by image
(host_leaves, tree_leaves_of_host, case_yardstick) and its floors (evaluator_floors: the edges count 2 / 2 / 6 of 8 (QP, CTU) pairs
and 2.4 % / 3.6 % / 4.8 % of the nodes' contexts in A / B / the crossing; image 1 does not depend on image 0 and would if stacked; a
transposition moves 1 (QP, CTU) pair in A and in B; the images differ; transform skip moves 2356 and 2383 width-4 leaf values).
"""
import numpy as np

from context_adaptive_neural_network_based_prediction_amd import intraprediction as ip
from tests import cu_tree_cases as cc

WIDTHS = cc.WIDTHS
NO_DEPTH = cc.NO_DEPTH
SEED = 3
EIGHT_QPS = cc.EIGHT_QPS
OWN_LAMBDAS = tuple(0.4 * 1.3 ** q for q in (0, 3, 7, 11, 14, 17, 20, 23))
TREE_KEYS = ("cu_depths", "part_nxn", "node_costs", "ctu_costs", "ctu_dists", "ctu_rates", "selected", "selected_pnn")

# (name, n_images, ctu_rows, ctu_cols, qps, the caller's lambdas or None for HM's, modes given)
CASES = (("1x1, one image, one QP", 1, 1, 1, (32,), None, True),
         ("1x2, one image, eight QPs", 1, 1, 2, EIGHT_QPS, None, True),
         ("2x1, two images, one QP, own lambda", 2, 2, 1, (27,), (31.5,), True),
         ("2x3, one image, eight QPs, no modes", 1, 2, 3, EIGHT_QPS, None, False),
         ("3x2, two images, one QP", 2, 3, 2, (37,), None, True),
         ("2x3, two images, eight QPs, own lambdas", 2, 2, 3, EIGHT_QPS, OWN_LAMBDAS, True),
         ("3x2, one image, eight QPs", 1, 3, 2, EIGHT_QPS, None, True))


MU, SIGMA = 1.0, 3.0


def near_tie_leaves(n_ctu, qps, lambdas=None, seed=SEED, modes=True, mu=MU, sigma=SIGMA):
    """{w: (dist uint32, rate uint64, modes uint8 or None)}, each [nb_qps, n_ctu * (64 / w)^2] in (CTU, z-order) order.  The leaves of
    tests/cu_tree_cases.py put a block and its four sub-blocks tens of bits apart, so a neighbour's depth -- which moves a flag by a
    bit or two -- hardly ever moves a decision.  Here a block's distortion is the sum of its four sub-blocks' plus lambda times a
    normal draw of a few bits, and every rate is below one bit with all 15 fractional bits in use: the alternatives of a node lie a
    few bits apart, and the edge of the neighbouring CTU decides a fair share of them."""
    rng = np.random.default_rng(seed)
    nq = len(qps)
    lam = np.array([cc.hm_lambda(q) if lambdas is None else lambdas[i] for i, q in enumerate(qps)])[:, None]
    leaves, below = {}, None
    for w in WIDTHS:
        n = n_ctu * (64 // w) ** 2
        if below is None:
            dist = np.floor(rng.gamma(2.0, 1.0, (nq, n)) * (40.0 * lam + 25.0))
        else:                                             # block g of a width has the sub-blocks 4 g .. 4 g + 3 one width down
            dist = np.maximum(below.reshape(nq, n, 4).sum(axis=2) + np.rint(lam * rng.normal(mu, sigma, (nq, n))), 0.0)
        below = dist
        rate = rng.integers(0, 32768, (nq, n))
        m = rng.choice(np.array([0, 1, 10, 18, 26, 35], np.uint8), size=(nq, n)) if modes else None
        leaves[w] = (np.ascontiguousarray(dist.astype(np.uint32)), np.ascontiguousarray(rate.astype(np.uint64)), m)
    return leaves


# The direct entry's further grids (tests/test_cu_tree_picture.py, tests/test_gpu_cu_tree_picture.py), kept apart from CASES: `conditions`
# and the figures above are computed over CASES alone.  4x3: anti-diagonals of 1, 2, 3, 3, 2, 1 CTUs, three images; 1x5: every diagonal
# holds one CTU and only left edges exist; 5x1: only above edges exist.
EXTRA_CASES = (("4x3, three images, eight QPs, own lambdas", 3, 4, 3, EIGHT_QPS, OWN_LAMBDAS, True),
               ("1x5, one image, one QP", 1, 1, 5, (32,), None, True),
               ("5x1, two images, eight QPs, no modes", 2, 5, 1, EIGHT_QPS, None, False))
# Their seeds, chosen per case on the CPU as SEED was: the first of 0, 1, ... at which the yardstick alone shows at least one (QP, CTU)
# map that differs from the unchained decision (`moved_maps`; tests/test_cu_tree_picture.py asserts it).  Tried: seed 0 gives the 4x3 case 55 such maps of 288 and the 5x1 case 3 of 80; the 1x5 case, with one QP and four
# CTUs that have a neighbour, keeps every map at seeds 0 .. 5 and moves 1 of its 5 at seed 6.
EXTRA_SEEDS = {"4x3, three images, eight QPs, own lambdas": 0, "1x5, one image, one QP": 6, "5x1, two images, eight QPs, no modes": 0}


def case_leaves(case, seed=None):
    """{w: (dist, rate, modes or None)} of a case, in (image, CTU row, CTU column, z-order) order; the seed of an extra case is its own"""
    name, n_images, rows, cols, qps, lambdas, modes = case
    seed = EXTRA_SEEDS.get(name, SEED) if seed is None else seed
    return near_tie_leaves(n_images * rows * cols, qps, lambdas, seed + len(name), modes)


def one_ctu(leaves, ctu, n_ctu):
    """The leaves of CTU `ctu` alone, as intraprediction.cu_tree takes them (the rate in two parts)"""
    cut = {}
    for w, (d, r, m) in leaves.items():
        count = (64 // w) ** 2
        sl = slice(ctu * count, (ctu + 1) * count)
        cut[w] = (np.ascontiguousarray(d[:, sl]), np.ascontiguousarray(r[:, sl]), None if m is None else np.ascontiguousarray(m[:, sl]))
    return cc.as_rd_pass_tuples(cut)


def edges_of_maps(left_map, above_map, nq):
    """left_depths / above_depths [nq, 1, 8] cut from two maps [nq, 64] (z-order) or None: column x = 7 of the one, row y = 7 of the other"""
    left, above = np.full((nq, 1, 8), NO_DEPTH, np.uint8), np.full((nq, 1, 8), NO_DEPTH, np.uint8)
    for k in range(8):
        if left_map is not None:
            left[:, 0, k] = left_map[:, cc.z_index(7, k)]
        if above_map is not None:
            above[:, 0, k] = above_map[:, cc.z_index(k, 7)]
    return left, above


def yardstick(leaves, qps, n_images, rows, cols, lambdas=None, pnn_mode=35, chain=True):
    """The picture's tree from pnn_cu_tree_host called once per CTU in raster order (chain=False: every CTU with absent edges).
    Returns the eight outputs as the picture entries lay them out, 'image_dists' / 'image_rates' as numpy sums, and 'edges':
    (left, above) uint8 [nq, n_ctu, 8] as they were given."""
    nq, n_ctu = len(qps), n_images * rows * cols
    with_modes = all(leaves[w][2] is not None for w in WIDTHS)
    out = {"cu_depths": np.zeros((nq, n_ctu, 64), np.uint8), "part_nxn": np.zeros((nq, n_ctu, 64), np.uint8),
           "node_costs": np.zeros((nq, n_ctu, 85, 2), np.float64), "ctu_costs": np.zeros((nq, n_ctu), np.float64),
           "ctu_dists": np.zeros((nq, n_ctu), np.uint64), "ctu_rates": np.zeros((nq, n_ctu), np.uint64),
           "selected": np.zeros((nq, 5), np.uint32)}
    if with_modes:
        out["selected_pnn"] = np.zeros((nq, 5), np.uint32)
    lefts, aboves = np.zeros((nq, n_ctu, 8), np.uint8), np.zeros((nq, n_ctu, 8), np.uint8)
    for image in range(n_images):
        for r in range(rows):
            for c in range(cols):
                ctu = (image * rows + r) * cols + c
                left, above = edges_of_maps(out["cu_depths"][:, ctu - 1] if chain and c else None,
                                            out["cu_depths"][:, ctu - cols] if chain and r else None, nq)
                got = ip.cu_tree(one_ctu(leaves, ctu, n_ctu), qps, lambdas, left, above, pnn_mode)
                for key in ("cu_depths", "part_nxn", "node_costs", "ctu_costs", "ctu_dists", "ctu_rates"):
                    out[key][:, ctu] = got[key][:, 0]
                out["selected"] += got["selected"]
                if with_modes:
                    out["selected_pnn"] += got["selected_pnn"]
                lefts[:, ctu], aboves[:, ctu] = left[:, 0], above[:, 0]
    per_image = out["ctu_dists"].reshape(nq, n_images, rows * cols)
    out["image_dists"] = per_image.sum(axis=2, dtype=np.uint64)
    out["image_rates"] = out["ctu_rates"].reshape(nq, n_images, rows * cols).sum(axis=2, dtype=np.uint64)
    out["edges"] = (lefts, aboves)
    return out


def moved_maps(case, seed=None):
    """How many (QP, CTU) maps of a case differ between the chained yardstick and the unchained decision"""
    name, n_images, rows, cols, qps, lambdas, _ = case
    leaves = case_leaves(case, seed)
    chained = yardstick(leaves, qps, n_images, rows, cols, lambdas)
    alone = yardstick(leaves, qps, n_images, rows, cols, lambdas, chain=False)
    return int((chained["cu_depths"] != alone["cu_depths"]).any(axis=2).sum())


FIRST = {0: 0, 1: 1, 2: 5, 3: 21}


def replay_contexts(node_costs, left, above):
    """The context each of the 21 upper nodes of ONE CTU read when it was decided, replayed from its node costs [85, 2] and edges [8]:
    [(depth, context, context with absent edges, whether an available cross-CTU cell was read)] in decision order."""
    depth_map = np.full((8, 8), 3, np.int64)              # [y][x]; the depth-3 level is decided first
    records = []

    def visit(depth, x, y):                               # node at (x, y) in units of its own size
        if depth == 3:
            return
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            visit(depth + 1, 2 * x + dx, 2 * y + dy)
        cells = 8 >> depth
        cx, cy = x * cells, y * cells
        inside_left = int(cx > 0 and depth_map[cy, cx - 1] > depth)
        inside_above = int(cy > 0 and depth_map[cy - 1, cx] > depth)
        cross_left = int(cx == 0 and left[cy] != NO_DEPTH and left[cy] > depth)
        cross_above = int(cy == 0 and above[cx] != NO_DEPTH and above[cx] > depth)
        reads_cross = (cx == 0 and left[cy] != NO_DEPTH) or (cy == 0 and above[cx] != NO_DEPTH)
        records.append((depth, inside_left + inside_above + cross_left + cross_above, inside_left + inside_above, bool(reads_cross)))
        node = FIRST[depth] + cc.z_index(x, y)
        if not node_costs[node, 1] < node_costs[node, 0]:
            depth_map[cy:cy + cells, cx:cx + cells] = depth

    visit(0, 0, 0)
    return records


def conditions(seed=SEED):
    """(share of nodes whose context differs from absent edges, share of nodes reading a cross-CTU neighbour with context 0 / 1 / 2 [3],
    {multi-CTU case: CTUs whose final map differs from the unchained decision}, area share per width [5]) over CASES, yardstick only."""
    nodes, differing, by_context = 0, 0, np.zeros(3)
    moved, area = {}, np.zeros(5)
    for case in CASES:
        name, n_images, rows, cols, qps, lambdas, _ = case
        leaves = case_leaves(case, seed)
        chained = yardstick(leaves, qps, n_images, rows, cols, lambdas)
        area += chained["selected"].sum(axis=0) * np.array([w * w for w in WIDTHS], np.float64)
        if rows * cols == 1:
            continue
        alone = yardstick(leaves, qps, n_images, rows, cols, lambdas, chain=False)
        moved[name] = int((chained["cu_depths"] != alone["cu_depths"]).any(axis=2).sum())
        lefts, aboves = chained["edges"]
        for qi in range(len(qps)):
            for ctu in range(n_images * rows * cols):
                if ctu % (rows * cols) == 0:              # an image's first CTU: no CTU left of it or above it
                    continue
                for depth, ctx, ctx_absent, reads_cross in replay_contexts(chained["node_costs"][qi, ctu], lefts[qi, ctu], aboves[qi, ctu]):
                    nodes += 1
                    differing += ctx != ctx_absent
                    if reads_cross:
                        by_context[ctx] += 1
    return differing / nodes, by_context / nodes, moved, area / area.sum()


# ---- the evaluator's test picture (tests/test_gpu_cu_tree_picture_evaluator.py, tools/cu_tree_picture_rate.py) ----
# 2 x 2 CTUs with their 64-wide contexts: the grid starts at (64, 64), where the 64-wide block's context corner is (0, 0), and the
# widest context of the last CTU ends at 256 -- the smallest picture that holds them.
EVALUATOR_QPS = (22, 37)
ROW_1ST, COL_1ST, CTU_ROWS, CTU_COLS, SIDE = 64, 64, 2, 2, 256
POSITIONS = {w: ip.ctu_block_positions(w, *ip.ctu_grid(ROW_1ST, COL_1ST, CTU_ROWS, CTU_COLS)) for w in ip.WIDTHS}
OPTIONS = dict(reference_smoothing=2, transform_rate=True, transform_sign_hiding=True, transform_rdoq=True)
# The picture seeds.  With seeded predictors the leaves of a block and of its four sub-blocks lie far apart, and a neighbour's depth,
# worth a bit or two, seldom moves a map.  SEEDS holds, per codec, the first of 5200, 5201, ... for which the HOST path shows a
# differing map: 5227 for the switch codec from pictures (none of 5200 .. 5226 does), 5262 for the substitution codec from pairs (none
# of 5200 .. 5261 does); 1 of the 8 (QP, CTU) maps differs at each.  They depend on tests/util.py's `pictures` and `make_net`: after
# a change to either, find them again on a GPU with this loop, per codec, and write the first seed that gives a nonzero count here:
#     nets = {w: util.make_net(w, w <= 8, POSITIONS[w][0].size) for w in ip.WIDTHS}
#     for seed in range(5200, 5600):
#         scores = {w: score_masks_*(evaluator_channels(pairs, seed), w, *POSITIONS[w], nets[w], util.MEAN, ((0, 0),),
#                                    keep_predictions=False, first_pass=True, transform_qps=EVALUATOR_QPS, rd_pass=True,
#                                    rd_pass_signalling=True, rd_pass_codec=codec, **OPTIONS) for w in ip.WIDTHS}
#         leaves = leaves_of_scores(scores)
#         chained = ip.cu_tree_picture(leaves, EVALUATOR_QPS, 1, CTU_ROWS, CTU_COLS, pnn_mode=35 or 18)        # device=None
#         alone = ip.cu_tree(leaves, EVALUATOR_QPS, pnn_mode=35 or 18)                                         # device=None
#         count = (chained['cu_depths'] != alone['cu_depths']).any(axis=2).sum()
SEEDS = {'switch': 5227, 'substitution': 5262}


def leaves_of_scores(scores):
    """The leaves of the five per-width score dictionaries as evaluation.coding_tree_from_scores builds them"""
    out = {}
    for w, d in scores.items():
        d = d[(0, 0)] if (0, 0) in d else d
        out[w] = (d['rd_pass_sses'], (d['rd_pass_rate_bits'] * 32768.).astype(np.uint64), (d['rd_pass_side_rate_bits'] * 32768.).astype(np.uint64),
                  d['rd_pass_modes'])
    return out


def evaluator_channels(pairs, seed):
    """[1, 256, 256, 1] seeded picture, or [1, 256, 256, 2] with `pairs` (a second seeded picture as the decoded plane)"""
    from tests import util
    pictures = util.pictures(2 if pairs else 1, SIDE, SIDE, seed)
    return np.ascontiguousarray(np.stack([pictures[0], pictures[1]], axis=-1)[None] if pairs else pictures[..., None])


# ---- two images, grids that are not square, every codec / plane form (tests/test_gpu_cu_tree_picture_evaluator.py) ----
# A and B are the smallest pictures that hold a 1 x 2 and a 2 x 1 grid from (64, 64) with the 64-wide contexts; `crossing` puts transform
# skip on the 2 x 2 grid of the test above, which has both kinds of edge.  Width 4 has 1024 blocks per call in A and B, width 64 has 4.
#
# The floors (`evaluator_floors`, from the yardstick alone; the test asserts each) and the seeds.  For A and B the seeds 5300, 5301, ...
# were tried in turn on an MI355X, the first that meets every floor kept.  What is scarce is a map with a depth beyond 1: exchanging
# rows and columns shows only where a neighbour's last column and last row differ, and with seeded predictors most CTUs are one CU or
# four.  A: 5714 -- none of 5300 .. 5713 (414 seeds) held a cell of depth 2, so none showed a transposition; 266 of them also gave
# stacked images the node costs of separate ones (the last CTU of image 0 is one CU), 210 had no node cost that an edge moves, 123
# gave both images the same maps.  B: 5304 -- 5300 .. 5303 met every floor but the transposition.  The crossing keeps SEEDS['switch'].
# Measured at these seeds (floors, not figures to reproduce: a floor is "at least one", "differs" or "equal"):
#                                                                        A          B          crossing
#   (QP, CTU) pairs whose node costs the edges move                      2 of 8     2 of 8     6 of 8
#   upper nodes of CTUs with a neighbour whose context the edges move    2.4 %      3.6 %      4.8 %
#   (QP, CTU) pairs whose node costs differ with rows and columns
#   exchanged                                                            1          1          (square grid)
#   first CTU of image 1: node costs of absent edges / other ones
#   with the images stacked as one grid of 1 x 4 (A), 4 x 1 (B)          yes / yes  yes / yes
#   the two images' depth maps differ / their image_dists differ         yes / yes  yes / yes
#   cells of depth 0, 1, 2 over both QPs                                 256 240 16 128 352 32 0 512 0
#   width-4 leaf values (of 4 x 2 x blocks) that transform skip moves    2356       --         2383
EVALUATOR_CASES = {
    'A': dict(n_images=2, ctu_rows=1, ctu_cols=2, height=192, width=256, codec='switch', pairs=True, transform_skip=True, seed=5714),
    'B': dict(n_images=2, ctu_rows=2, ctu_cols=1, height=256, width=192, codec='substitution', pairs=False, transform_skip=False, seed=5304),
    'crossing': dict(n_images=1, ctu_rows=2, ctu_cols=2, height=SIDE, width=SIDE, codec='switch', pairs=False, transform_skip=True,
                     seed=SEEDS['switch'])}
LEAF_KEYS = {'rd_pass_sses': 'sses', 'rd_pass_rate_bits': 'rate_bits', 'rd_pass_side_rate_bits': 'side_rate_bits', 'rd_pass_modes': 'modes'}


def case_positions(case):
    """{w: (row_1sts, col_1sts)} of the case's grid from (ROW_1ST, COL_1ST), one image's blocks in (CTU, z-order) order"""
    return {w: ip.ctu_block_positions(w, *ip.ctu_grid(ROW_1ST, COL_1ST, case['ctu_rows'], case['ctu_cols'])) for w in ip.WIDTHS}


def case_channels(case, seed=None):
    """[images, H, W, 1] different seeded pictures, or [images, H, W, 2] with pairs: further seeded pictures as the decoded planes"""
    from tests import util
    n = case['n_images']
    pictures = util.pictures(2 * n if case['pairs'] else n, case['height'], case['width'], case['seed'] if seed is None else seed)
    return np.ascontiguousarray(np.stack([pictures[:n], pictures[n:]], axis=-1) if case['pairs'] else pictures[..., None])


def case_pnn_mode(case):
    return 35 if case['codec'] == 'switch' else 18


def case_score_options(case, w, keep_predictions):
    """The options of score_masks_* that make the calls coding_tree_from_pictures makes for width w"""
    return dict(OPTIONS, keep_predictions=keep_predictions, first_pass=True, transform_qps=EVALUATOR_QPS, rd_pass=True, rd_pass_signalling=True,
                rd_pass_codec=case['codec'], rd_pass_transform_skip=case['transform_skip'] and w == 4)


def host_leaves(case, channels, nets, transform_skip=None):
    """{w: {'sses', 'rate_bits', 'side_rate_bits', 'modes': [nb_qps, images * blocks]}} from the second pass's HOST twin, image by
    image: score_masks_* on each image ALONE gives the targets and the PNN's uint8 predictions, the patterns are cut on the host from
    that image's context plane, intraprediction.rd_pass(device=None) decides; the images are then joined along the block axis.
    Nothing here goes through a device call on more than one image, the second pass on the device or the picture entries of the tree."""
    from context_adaptive_neural_network_based_prediction_amd import evaluation
    from tests import util
    score = evaluation.score_masks_from_picture_pairs if case['pairs'] else evaluation.score_masks_from_pictures
    transform_skip = case['transform_skip'] if transform_skip is None else transform_skip
    positions, out = case_positions(case), {}
    for w in ip.WIDTHS:
        rows, cols = positions[w]
        per_image = []
        for i in range(case['n_images']):
            alone = channels[i:i + 1]
            kept = score(alone, w, rows, cols, nets[w], util.MEAN, ((0, 0),), **case_score_options(case, w, True))[(0, 0)]
            patterns = ip.extract_intra_patterns(alone[..., -1:], w, rows + w - 1, cols + w - 1, (0, 0))[..., 0]
            host = ip.rd_pass(patterns, kept['targets_uint8'][..., 0], kept['predictions_pnn_uint8'][..., 0], EVALUATOR_QPS,
                              reference_smoothing=OPTIONS['reference_smoothing'], sign_data_hiding=OPTIONS['transform_sign_hiding'],
                              rdoq=OPTIONS['transform_rdoq'], signalling=True, codec=case['codec'], transform_skip=transform_skip and w == 4)
            host['predictions_pnn_uint8'], host['targets_uint8'] = kept['predictions_pnn_uint8'], kept['targets_uint8']
            per_image.append(host)
        out[w] = {key: np.concatenate([h[key] for h in per_image], axis=1) for key in LEAF_KEYS.values()}
        for key in ('predictions_pnn_uint8', 'targets_uint8'):
            out[w][key] = np.concatenate([h[key] for h in per_image], axis=0)
    return out


def tree_leaves_of_host(host):
    """{w: (dist, rate + side rate, modes)} as `yardstick` takes them, formed as leaves_of_scores forms the two rates"""
    return {w: (h['sses'], (h['rate_bits'] * 32768.).astype(np.uint64) + (h['side_rate_bits'] * 32768.).astype(np.uint64), h['modes'])
            for w, h in host.items()}


def case_yardstick(case, leaves, **changes):
    """`yardstick` on the case's leaves; changes: n_images / rows / cols / chain other than the case's own"""
    arguments = dict(n_images=case['n_images'], rows=case['ctu_rows'], cols=case['ctu_cols'], pnn_mode=case_pnn_mode(case))
    arguments.update(changes)
    return yardstick(leaves, EVALUATOR_QPS, **arguments)


def evaluator_floors(case, leaves, chained):
    """What keeps an evaluator case from passing vacuously, from the yardstick alone.  Returns a dictionary:
    'edges' -- (QP, CTU) pairs whose node costs differ between the chained yardstick and absent edges; 'context_share' -- the share of
    the upper nodes of CTUs with a neighbour whose context differs from the one absent edges give (replay_contexts); and for two images
    'first_of_image_1_alone' -- the first CTU of image 1 has the node costs absent edges give; 'stacked' -- and other ones when the
    two images are stacked as ONE taller (one column) or wider (one row) grid; 'transposed' -- (QP, CTU) pairs whose node costs differ
    with rows and columns exchanged; 'depth_maps_differ', 'image_dists_differ' -- between the two images."""
    rows, cols, n_images = case['ctu_rows'], case['ctu_cols'], case['n_images']
    per_image = rows * cols

    def differing(other):
        return int((chained['node_costs'] != other['node_costs']).any(axis=(2, 3)).sum())

    alone = case_yardstick(case, leaves, chain=False)
    lefts, aboves = chained['edges']
    nodes = moved = 0
    for qi in range(len(EVALUATOR_QPS)):
        for ctu in range(n_images * per_image):
            if ctu % per_image:
                for _, ctx, ctx_absent, _ in replay_contexts(chained['node_costs'][qi, ctu], lefts[qi, ctu], aboves[qi, ctu]):
                    nodes += 1
                    moved += ctx != ctx_absent
    floors = {'edges': differing(alone), 'context_share': moved / nodes,
              'transposed': differing(case_yardstick(case, leaves, rows=cols, cols=rows))}
    if n_images == 2:
        first = per_image
        stacked = case_yardstick(case, leaves, n_images=1, rows=rows * (2 if cols == 1 else 1), cols=cols * (2 if cols != 1 else 1))
        floors['first_of_image_1_alone'] = bool(np.array_equal(chained['node_costs'][:, first], alone['node_costs'][:, first]))
        floors['stacked'] = bool((chained['node_costs'][:, first] != stacked['node_costs'][:, first]).any())
        floors['depth_maps_differ'] = bool((chained['cu_depths'][:, :per_image] != chained['cu_depths'][:, per_image:]).any())
        floors['image_dists_differ'] = bool((chained['image_dists'][:, 0] != chained['image_dists'][:, 1]).any())
    return floors


def floors_hold(floors):
    return all(bool(value) for value in floors.values())
