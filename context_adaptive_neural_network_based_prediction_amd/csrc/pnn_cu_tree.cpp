// Host twin of the coding-tree pass (no HIP in this file; include/pnn_hip.h, "the coding tree"): per QP and CTU
// the partition TEncCu::xCompressCU's recursion chooses from the second pass's winners at every aligned block of the five widths.
// Every line of the decision is pnn_cu_tree.h's; pnn_cu_tree.hip computes the same on the GPU.  tests/test_hm_cu_tree.py pins the
// six split_cu_flag bins and the two part_mode bins to HM's own counter, tests/test_cu_tree.py this file to a restatement.
#include "../../include/pnn_hip.h"
#include "pnn_cu_tree.h"
#include "pnn_rdoq.h"

#include <cstdint>
#include <cstdio>

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

extern "C" int pnn_cu_tree_host(const int* qps, int nb_qps, const double* lambdas, int n_ctu, const uint32_t* const* dists,
                                const uint64_t* const* rates, const uint8_t* const* modes, const uint8_t* left_depths, const uint8_t* above_depths,
                                int pnn_mode, uint8_t* cu_depths, uint8_t* part_nxn, double* node_costs, double* ctu_costs, uint64_t* ctu_dists,
                                uint64_t* ctu_rates, uint32_t* selected, uint32_t* selected_pnn)
{
    const bool any = cu_depths || part_nxn || node_costs || ctu_costs || ctu_dists || ctu_rates || selected || selected_pnn;
    const char* refusal = ct::refusal(qps, nb_qps, lambdas, n_ctu, dists, rates, modes, pnn_mode, any, selected_pnn != nullptr);
    const size_t edge_cells = refusal ? 0 : (size_t)nb_qps * n_ctu * 8;
    if (!refusal) refusal = ct::edge_refusal(left_depths, edge_cells);
    if (!refusal) refusal = ct::edge_refusal(above_depths, edge_cells);
    if (refusal) { fprintf(stderr, "pnn_cu_tree_host: %s.\n", refusal); return PNN_E_ARG; }
    for (int i = 0; i < nb_qps * ct::kWidths; i++) {
        if (selected) selected[i] = 0;
        if (selected_pnn) selected_pnn[i] = 0;
    }
    uint8_t none[8];
    for (uint8_t& v : none) v = ct::kNoDepth;
    for (int qi = 0; qi < nb_qps; qi++) {
        const double lambda = lambdas ? lambdas[qi] : pnn::rdoq::hm_intra_lambda(qps[qi]);
        const ct::QpBits bits = ct::qp_bits(qps[qi]);
        for (int ctu = 0; ctu < n_ctu; ctu++) {
            const size_t at = (size_t)qi * n_ctu + ctu;
            uint32_t dist[ct::kLeaves];
            uint64_t rate[ct::kLeaves], best_dist[ct::kNodes], best_rate[ct::kNodes];
            double costs[ct::kNodes * 2];
            uint8_t depth[ct::kCells], nxn[ct::kCells];
            for (int k = 0; k < ct::kWidths; k++) {
                const int count = ct::leaves_of_width(k), first = ct::first_leaf_of_width(k);
                for (int i = 0; i < count; i++) {
                    dist[first + i] = dists[k][at * count + i];
                    rate[first + i] = rates[k][at * count + i];
                }
            }
            const ct::Work w{dist, rate, best_dist, best_rate, costs, depth, nxn, left_depths ? left_depths + at * 8 : none,
                             above_depths ? above_depths + at * 8 : none};
            for (int i = 0; i < ct::kCells; i++) ct::decide_part_size(w, i, bits, lambda);
            ct::walk_upper(w, bits, lambda);
            for (int z = 0; z < ct::kCells; z++) {
                if (cu_depths) cu_depths[at * ct::kCells + z] = depth[z];
                if (part_nxn) part_nxn[at * ct::kCells + z] = nxn[z];
                int leaf, count;
                const int k = ct::selected_block(w, z, &leaf, &count);
                if (k < 0) continue;
                if (selected) selected[qi * ct::kWidths + k] += (uint32_t)count;
                for (int i = 0; selected_pnn && i < count; i++)
                    selected_pnn[qi * ct::kWidths + k] += modes[k][at * ct::leaves_of_width(k) + leaf + i] == pnn_mode;
            }
            for (int i = 0; node_costs && i < ct::kNodes * 2; i++) node_costs[at * ct::kNodes * 2 + i] = costs[i];
            if (ctu_costs) ctu_costs[at] = costs[1] < costs[0] ? costs[1] : costs[0];
            if (ctu_dists) ctu_dists[at] = best_dist[0];
            if (ctu_rates) ctu_rates[at] = best_rate[0];
        }
    }
    return PNN_OK;
}
