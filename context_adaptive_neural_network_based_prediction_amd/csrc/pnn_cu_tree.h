// The one home of the coding-tree pass (include/pnn_hip.h, "the coding tree"): the decision of
// TEncCu::xCompressCU between a coding unit and its four sub-units, and at 8 x 8 between SIZE_2Nx2N and SIZE_NxN, from the distortion
// and fractional rate the second pass left at every aligned block of the five widths inside a 64 x 64 CTU.  Luma only, I slice,
// minimum CU 8.  Shared by the host twin (pnn_cu_tree.cpp, plain C++) and the kernel (pnn_cu_tree.hip): both compile THESE lines, so
// there is no HIP in it beyond the function qualifiers, and no loop without a compile-time bound.
//
// Per CTU, everything in HM's z-order, depth by depth: 85 CU nodes (depth d = 0 .. 3, size 64 >> d, node i of depth d at kNodeFirst[d]
// + i, its children 4 i + k one depth down) and 256 4 x 4 units (the four of 8 x 8 node i at 4 i + k).  The 341 leaves of a CTU lie in
// that order: leaf n < 85 is node n's own block, leaf 85 + u unit u.
#pragma once

#include "pnn_cabac_tables.h"

#include <cmath>

namespace pnn {
namespace cutree {

constexpr int kWidths = 5;                         // 4, 8, 16, 32, 64: the order of every per-width argument
constexpr int kNodes = 85, kUnits = 256, kLeaves = kNodes + kUnits, kCells = 64, kMaxQps = 8;
constexpr int kNoDepth = 255;                      // an edge cell without an available neighbour
// I-slice rows of HM's ContextTables.h: INIT_SPLIT_FLAG (three contexts), INIT_PART_SIZE (context 0, the only one an intra CU reads)
constexpr int kInitSplit[3] = {139, 141, 157}, kInitPart = 184;

PNN_TQ_HD inline int node_first(int depth) { return depth == 0 ? 0 : depth == 1 ? 1 : depth == 2 ? 5 : 21; }
PNN_TQ_HD inline int leaves_of_width(int k) { return 256 >> (2 * k); }                  // per CTU: 256, 64, 16, 4, 1
PNN_TQ_HD inline int first_leaf_of_width(int k) { return k == 0 ? kNodes : node_first(4 - k); }

// z-order of the 8 x 8 minimum-CU cells: bit 2 j of the index is bit j of x, bit 2 j + 1 bit j of y
PNN_TQ_HD inline int cell_x(int z) { return (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4); }
PNN_TQ_HD inline int cell_y(int z) { return cell_x(z >> 1); }
PNN_TQ_HD inline int cell_of(int x, int y)
{
    return (x & 1) | ((y & 1) << 1) | ((x & 2) << 1) | ((y & 2) << 2) | ((x & 4) << 2) | ((y & 4) << 3);
}

// entropyBits[state ^ bin] of the four contexts from the state an I slice of the QP starts with, in 2^-15 bit (made on the host, for
// twin and kernel alike: it travels in the kernel's argument block).  part[1] is SIZE_2Nx2N's bin, part[0] SIZE_NxN's.
struct QpBits { uint32_t split[3][2], part[2]; };
inline QpBits qp_bits(int qp)
{
    const int* entropy_bits = cabac::entropy_bits_table();
    QpBits b;
    for (int v = 0; v < 2; v++) {
        for (int c = 0; c < 3; c++) b.split[c][v] = (uint32_t)entropy_bits[cabac::init_state(qp, kInitSplit[c]) ^ v];
        b.part[v] = (uint32_t)entropy_bits[cabac::init_state(qp, kInitPart) ^ v];
    }
    return b;
}

// TComRdCost::calcRdCost on whole bits: one IEEE multiply and one IEEE add, each rounded once
PNN_TQ_HD inline double rd_cost(uint64_t dist, uint64_t frac_bits, double lambda)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double bits = lambda * (double)(frac_bits >> 15);
    return (double)dist + bits;
}

// What one CTU's decision works on: the staged leaves, the chosen D and F of every node, both alternatives' J, the depth map of the
// minimum-CU cells (z-order), the part size of the 8 x 8 nodes and the depths along the CTU's two outer edges (kNoDepth: not available)
struct Work {
    const uint32_t* dist; const uint64_t* rate;    // [kLeaves]
    uint64_t* best_dist; uint64_t* best_rate;      // [kNodes]
    double* costs;                                 // [kNodes][2]
    uint8_t* depth; uint8_t* nxn;                  // [kCells]
    const uint8_t* left; const uint8_t* above;     // [8]
};

// Depth 3, 8 x 8 node i: SIZE_2Nx2N first, SIZE_NxN second, strict <.  No neighbour is read: 64 lanes decide the 64 nodes at once.
PNN_TQ_HD inline void decide_part_size(const Work& w, int i, const QpBits& b, double lambda)
{
    const int node = node_first(3) + i, unit = kNodes + 4 * i;
    const uint64_t d0 = w.dist[node], f0 = w.rate[node] + b.part[1];
    uint64_t d1 = 0, f1 = b.part[0];
#pragma unroll
    for (int k = 0; k < 4; k++) { d1 += w.dist[unit + k]; f1 += w.rate[unit + k]; }
    const double j0 = rd_cost(d0, f0, lambda), j1 = rd_cost(d1, f1, lambda);
    const bool nxn = j1 < j0;
    w.costs[2 * node] = j0; w.costs[2 * node + 1] = j1;
    w.best_dist[node] = nxn ? d1 : d0; w.best_rate[node] = nxn ? f1 : f0;
    w.nxn[i] = nxn; w.depth[i] = 3;
}

// TComDataCU::getCtxSplitFlag of node i of depth d: the depths of the CUs that cover the sample left of and the sample over the node's
// top-left sample, from the map inside the CTU (both precede the node in z-order: their subtrees are decided) and from the edges outside
PNN_TQ_HD inline int split_context(const Work& w, int d, int i)
{
    const int z = i << (2 * (3 - d)), x = cell_x(z), y = cell_y(z);
    const int left = x ? w.depth[cell_of(x - 1, y)] : w.left[y], above = y ? w.depth[cell_of(x, y - 1)] : w.above[x];
    return (left != kNoDepth && left > d ? 1 : 0) + (above != kNoDepth && above > d ? 1 : 0);
}

// Depths 2, 1, 0, node i of depth d once its four children are decided: unsplit first, split second, strict <; the winner's depth goes
// into the map (a split node's cells hold its children's already)
PNN_TQ_HD inline void decide_split(const Work& w, int d, int i, const QpBits& b, double lambda)
{
    const int node = node_first(d) + i, child = node_first(d + 1) + 4 * i, ctx = split_context(w, d, i);
    const uint64_t d0 = w.dist[node], f0 = w.rate[node] + b.split[ctx][0];
    uint64_t d1 = 0, f1 = b.split[ctx][1];
#pragma unroll
    for (int k = 0; k < 4; k++) { d1 += w.best_dist[child + k]; f1 += w.best_rate[child + k]; }
    const double j0 = rd_cost(d0, f0, lambda), j1 = rd_cost(d1, f1, lambda);
    const bool split = j1 < j0;
    w.costs[2 * node] = j0; w.costs[2 * node + 1] = j1;
    w.best_dist[node] = split ? d1 : d0; w.best_rate[node] = split ? f1 : f0;
    if (!split) {
        const int cells = 1 << (2 * (3 - d)), z = i * cells;
#pragma unroll 1
        for (int k = 0; k < kCells; k++)
            if (k < cells) { w.depth[z + k] = (uint8_t)d; w.nxn[z + k] = 0; }
    }
}

// The 21 upper nodes in z-order post-order: a serial walk, because a node's context reads what the subtrees before it wrote
PNN_TQ_HD inline void walk_upper(const Work& w, const QpBits& b, double lambda)
{
#pragma unroll 1
    for (int a = 0; a < 4; a++) {
#pragma unroll 1
        for (int c = 0; c < 4; c++) decide_split(w, 2, 4 * a + c, b, lambda);
        decide_split(w, 1, a, b, lambda);
    }
    decide_split(w, 0, 0, b, lambda);
}

// Cell z of the final map as a selected block: -1 unless z is the first cell of its CU; else the width index k (0 .. 4) of the CU's
// prediction blocks, *leaf the first of them among the width's leaves of the CTU, *count how many (4 for N x N, else 1)
PNN_TQ_HD inline int selected_block(const Work& w, int z, int* leaf, int* count)
{
    const int d = w.depth[z], shift = 2 * (3 - d);
    if (z & ((1 << shift) - 1)) return -1;
    const bool nxn = d == 3 && w.nxn[z];
    *leaf = nxn ? 4 * z : z >> shift;
    *count = nxn ? 4 : 1;
    return nxn ? 0 : 4 - d;
}

// The picture form (include/pnn_hip.h, "the coding tree over a picture"): edge cell e of a CTU -- e < 8 is left[y = e], else above[x =
// e - 8] -- from the FINAL maps of the CTU left of it and of the CTU above it (NULL: there is none in the image): cell (7, y) of the
// one, cell (x, 7) of the other.  The one place where a finished map becomes an edge, for twin and kernel alike.
PNN_TQ_HD inline uint8_t edge_from_maps(const uint8_t* left_map, const uint8_t* above_map, int e)
{
    const uint8_t* map = e < 8 ? left_map : above_map;
    return map ? map[e < 8 ? cell_of(7, e) : cell_of(e - 8, 7)] : (uint8_t)kNoDepth;
}

// The refusals every entry shares (pnn_cu_tree_host, pnn_cu_tree_device and the two picture entries): NULL, or the text of the first
// one that applies
inline const char* refusal(const int* qps, int nb_qps, const double* lambdas, int n_ctu, const uint32_t* const* dists, const uint64_t* const* rates,
                           const uint8_t* const* modes, int pnn_mode, bool any_output, bool wants_selected_pnn)
{
    if (nb_qps < 1 || nb_qps > kMaxQps || !qps) return "the QPs are not 1 to 8";
    for (int i = 0; i < nb_qps; i++)
        if (qps[i] < 0 || qps[i] > 51) return "a QP does not belong to [0, 51]";
    if (n_ctu < 1) return "fewer than one CTU";
    if (!dists || !rates) return "a leaf array is missing";
    for (int k = 0; k < kWidths; k++)
        if (!dists[k] || !rates[k] || (modes && !modes[k])) return "a leaf array is missing";
    for (int i = 0; lambdas && i < nb_qps; i++)
        if (!std::isfinite(lambdas[i]) || lambdas[i] < 0.) return "a lambda is not finite or below 0";
    if (pnn_mode < 0 || pnn_mode > 255) return "pnn_mode does not belong to [0, 255]";
    if (wants_selected_pnn && !modes) return "selected_pnn without the modes";
    if (!any_output) return "every output is NULL";
    return nullptr;
}
// The picture entries' grid, ahead of `refusal`: *n_ctu = n_images ctu_rows ctu_cols where that is an int
inline const char* grid_refusal(int n_images, int ctu_rows, int ctu_cols, int* n_ctu)
{
    if (n_images < 1 || ctu_rows < 1 || ctu_cols < 1) return "fewer than one image, CTU row or CTU column";
    const long long per_image = (long long)ctu_rows * ctu_cols;
    if (per_image > 0x7fffffffLL || per_image * n_images > 0x7fffffffLL) return "the CTUs of the pictures do not fit an int";
    *n_ctu = (int)(per_image * n_images);
    return nullptr;
}
inline const char* edge_refusal(const uint8_t* edge, size_t count)
{
    for (size_t i = 0; edge && i < count; i++)
        if (edge[i] > 3 && edge[i] != kNoDepth) return "an edge depth is not 0 .. 3 or 255";
    return nullptr;
}

}  // namespace cutree
}  // namespace pnn
