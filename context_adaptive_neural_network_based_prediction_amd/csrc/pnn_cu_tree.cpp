// Host twin of the coding-tree pass (no HIP in this file; include/pnn_hip.h, "the coding tree"; DESIGN.md sections 5q and 5r): per QP
// and CTU the partition TEncCu::xCompressCU's recursion chooses from the second pass's winners at every aligned block of the five
// widths.  Every line of the decision is pnn_cu_tree.h's; pnn_cu_tree.hip computes the same on the GPU.  tests/test_hm_cu_tree.py pins
// the six split_cu_flag bins and the two part_mode bins to HM's own counter, tests/test_cu_tree.py this file to a restatement.
// pnn_cu_tree_host takes every CTU's edges from the caller; pnn_cu_tree_picture_host takes them from the CTU left of it and the one
// above it in the same image (tests/test_cu_tree_picture.py holds it to the first, called CTU by CTU).  One CTU is decided in one place.
#include "../../include/pnn_hip.h"
#include "pnn_cu_tree.h"
#include "pnn_rdoq.h"

#include <cstdint>
#include <cstdio>
#include <vector>

// the costs are doubles rounded once per operation: nothing in this file may be contracted
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace ct = pnn::cutree;

extern "C" int pnn_cu_tree_bins_host(int qp, uint32_t* out)
{
    if (qp < 0 || qp > 51 || !out) { fprintf(stderr, "pnn_cu_tree_bins_host: a QP outside [0, 51] or a NULL output.\n"); return PNN_E_ARG; }
    const ct::QpBits b = ct::qp_bits(qp);
    for (int c = 0; c < 3; c++)
        for (int v = 0; v < 2; v++) out[2 * c + v] = b.split[c][v];
    out[6] = b.part[0];
    out[7] = b.part[1];
    return PNN_OK;
}

namespace {

struct Leaves { const uint32_t* const* dists; const uint64_t* const* rates; const uint8_t* const* modes; int pnn_mode; };
struct Outputs {
    uint8_t* cu_depths; uint8_t* part_nxn; double* node_costs; double* ctu_costs; uint64_t* ctu_dists; uint64_t* ctu_rates;
    uint32_t* selected; uint32_t* selected_pnn;
    bool any() const { return cu_depths || part_nxn || node_costs || ctu_costs || ctu_dists || ctu_rates || selected || selected_pnn; }
};

void zero_counts(const Outputs& o, int nb_qps)
{
    for (int i = 0; i < nb_qps * ct::kWidths; i++) {
        if (o.selected) o.selected[i] = 0;
        if (o.selected_pnn) o.selected_pnn[i] = 0;
    }
}

// CTU `at` = qi n_ctu + ctu of QP qi under the edges left / above [8]: every output that was asked for; the final map also to `map`
// [kCells] and the root's chosen D and F to *root_dist / *root_rate where those are given
void decide_ctu(const Leaves& in, int qi, size_t at, const ct::QpBits& bits, double lambda, const uint8_t* left, const uint8_t* above,
                const Outputs& o, uint8_t* map, uint64_t* root_dist, uint64_t* root_rate)
{
    uint32_t dist[ct::kLeaves];
    uint64_t rate[ct::kLeaves], best_dist[ct::kNodes], best_rate[ct::kNodes];
    double costs[ct::kNodes * 2];
    uint8_t depth[ct::kCells], nxn[ct::kCells];
    for (int k = 0; k < ct::kWidths; k++) {
        const int count = ct::leaves_of_width(k), first = ct::first_leaf_of_width(k);
        for (int i = 0; i < count; i++) {
            dist[first + i] = in.dists[k][at * count + i];
            rate[first + i] = in.rates[k][at * count + i];
        }
    }
    const ct::Work w{dist, rate, best_dist, best_rate, costs, depth, nxn, left, above};
    for (int i = 0; i < ct::kCells; i++) ct::decide_part_size(w, i, bits, lambda);
    ct::walk_upper(w, bits, lambda);
    for (int z = 0; z < ct::kCells; z++) {
        if (o.cu_depths) o.cu_depths[at * ct::kCells + z] = depth[z];
        if (o.part_nxn) o.part_nxn[at * ct::kCells + z] = nxn[z];
        if (map) map[z] = depth[z];
        int leaf, count;
        const int k = ct::selected_block(w, z, &leaf, &count);
        if (k < 0) continue;
        if (o.selected) o.selected[qi * ct::kWidths + k] += (uint32_t)count;
        for (int i = 0; o.selected_pnn && i < count; i++)
            o.selected_pnn[qi * ct::kWidths + k] += in.modes[k][at * ct::leaves_of_width(k) + leaf + i] == in.pnn_mode;
    }
    for (int i = 0; o.node_costs && i < ct::kNodes * 2; i++) o.node_costs[at * ct::kNodes * 2 + i] = costs[i];
    if (o.ctu_costs) o.ctu_costs[at] = costs[1] < costs[0] ? costs[1] : costs[0];
    if (o.ctu_dists) o.ctu_dists[at] = best_dist[0];
    if (o.ctu_rates) o.ctu_rates[at] = best_rate[0];
    if (root_dist) *root_dist = best_dist[0];
    if (root_rate) *root_rate = best_rate[0];
}

}  // namespace

extern "C" int pnn_cu_tree_host(const int* qps, int nb_qps, const double* lambdas, int n_ctu, const uint32_t* const* dists,
                                const uint64_t* const* rates, const uint8_t* const* modes, const uint8_t* left_depths, const uint8_t* above_depths,
                                int pnn_mode, uint8_t* cu_depths, uint8_t* part_nxn, double* node_costs, double* ctu_costs, uint64_t* ctu_dists,
                                uint64_t* ctu_rates, uint32_t* selected, uint32_t* selected_pnn)
{
    const Outputs o{cu_depths, part_nxn, node_costs, ctu_costs, ctu_dists, ctu_rates, selected, selected_pnn};
    const char* refusal = ct::refusal(qps, nb_qps, lambdas, n_ctu, dists, rates, modes, pnn_mode, o.any(), selected_pnn != nullptr);
    const size_t edge_cells = refusal ? 0 : (size_t)nb_qps * n_ctu * 8;
    if (!refusal) refusal = ct::edge_refusal(left_depths, edge_cells);
    if (!refusal) refusal = ct::edge_refusal(above_depths, edge_cells);
    if (refusal) { fprintf(stderr, "pnn_cu_tree_host: %s.\n", refusal); return PNN_E_ARG; }
    zero_counts(o, nb_qps);
    const Leaves in{dists, rates, modes, pnn_mode};
    uint8_t none[8];
    for (uint8_t& v : none) v = ct::kNoDepth;
    for (int qi = 0; qi < nb_qps; qi++) {
        const double lambda = lambdas ? lambdas[qi] : pnn::rdoq::hm_intra_lambda(qps[qi]);
        const ct::QpBits bits = ct::qp_bits(qps[qi]);
        for (int ctu = 0; ctu < n_ctu; ctu++) {
            const size_t at = (size_t)qi * n_ctu + ctu;
            decide_ctu(in, qi, at, bits, lambda, left_depths ? left_depths + at * 8 : none, above_depths ? above_depths + at * 8 : none, o,
                       nullptr, nullptr, nullptr);
        }
    }
    return PNN_OK;
}

// The picture form: per QP and image the CTUs in raster order, as HM decides them; the maps of one image's CTUs are kept for the edges
// of those right of and below them, whether or not cu_depths was asked for.
extern "C" int pnn_cu_tree_picture_host(const int* qps, int nb_qps, const double* lambdas, int n_images, int ctu_rows, int ctu_cols,
                                        const uint32_t* const* dists, const uint64_t* const* rates, const uint8_t* const* modes, int pnn_mode,
                                        uint8_t* cu_depths, uint8_t* part_nxn, double* node_costs, double* ctu_costs, uint64_t* ctu_dists,
                                        uint64_t* ctu_rates, uint32_t* selected, uint32_t* selected_pnn, uint64_t* image_dists,
                                        uint64_t* image_rates)
{
    const Outputs o{cu_depths, part_nxn, node_costs, ctu_costs, ctu_dists, ctu_rates, selected, selected_pnn};
    int n_ctu = 0;
    const char* refusal = ct::grid_refusal(n_images, ctu_rows, ctu_cols, &n_ctu);
    if (!refusal)
        refusal = ct::refusal(qps, nb_qps, lambdas, n_ctu, dists, rates, modes, pnn_mode, o.any() || image_dists || image_rates,
                              selected_pnn != nullptr);
    if (refusal) { fprintf(stderr, "pnn_cu_tree_picture_host: %s.\n", refusal); return PNN_E_ARG; }
    zero_counts(o, nb_qps);
    const Leaves in{dists, rates, modes, pnn_mode};
    std::vector<uint8_t> maps((size_t)ctu_rows * ctu_cols * ct::kCells);
    for (int qi = 0; qi < nb_qps; qi++) {
        const double lambda = lambdas ? lambdas[qi] : pnn::rdoq::hm_intra_lambda(qps[qi]);
        const ct::QpBits bits = ct::qp_bits(qps[qi]);
        for (int image = 0; image < n_images; image++) {
            uint64_t sum_dist = 0, sum_rate = 0;
            for (int r = 0; r < ctu_rows; r++)
                for (int c = 0; c < ctu_cols; c++) {
                    const size_t in_image = (size_t)r * ctu_cols + c;
                    const size_t at = (size_t)qi * n_ctu + (size_t)image * ctu_rows * ctu_cols + in_image;
                    uint8_t* map = maps.data() + in_image * ct::kCells;
                    uint8_t edge[16];
                    for (int e = 0; e < 16; e++) edge[e] = ct::edge_from_maps(c ? map - ct::kCells : nullptr, r ? map - (size_t)ctu_cols * ct::kCells : nullptr, e);
                    uint64_t root_dist, root_rate;
                    decide_ctu(in, qi, at, bits, lambda, edge, edge + 8, o, map, &root_dist, &root_rate);
                    sum_dist += root_dist;
                    sum_rate += root_rate;
                }
            if (image_dists) image_dists[(size_t)qi * n_images + image] = sum_dist;
            if (image_rates) image_rates[(size_t)qi * n_images + image] = sum_rate;
        }
    }
    return PNN_OK;
}
