// Host twin of HM's second intra pass as a column (no HIP in this file; include/pnn_hip.h, "the second intra pass"; DESIGN.md section
// 5l): per block the first-pass list (pnn_hevc_mode_hads_hm_host, the candidate competing as 35) plus 35 if the list lacks it, every
// candidate's prediction (pnn_hevc_intra_predict_hm, the candidate's own for 35) coded by pnn_trquant_sdh_host at every QP, J = D +
// lambda R per candidate, and the least J in list order under a strict <.  Nothing here but the composition and the decision: the
// entries it calls are the zero-tolerance yardsticks of their kernels, and this one is the yardstick of pnn_rd_pass_device.
// The cost is one IEEE multiply and one IEEE add in double; the pragmas below keep the compiler from contracting them into an FMA,
// as rd_cost does in rd_decide_kernel (pnn_hevc_intra.hip).
#include "../../include/pnn_hip.h"
#include "pnn_rdoq.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace {

constexpr int kCandidate = 35, kUnused = 255;
constexpr long kChunk = 1024;                                                  // blocks coded per call of the transform entry

int refuse(const char* why)
{
    fprintf(stderr, "pnn_rd_pass_host: %s\n", why);
    return PNN_E_ARG;
}

}  // namespace

extern "C" double pnn_hm_intra_lambda(int qp)
{
    // TEncSlice::calculateLambda, I slice, GOP size 1, 8-bit, no modifier: dQPFactor 0.57 * 2^((qp - 12) / 3)
    return pnn::rdoq::hm_intra_lambda(qp);
}

extern "C" int pnn_rd_pass_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                int sign_data_hiding, uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot,
                                double* best_cost, uint32_t* best_sse, uint64_t* best_rate)
{
    return pnn_rd_pass_rdoq_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, 0,
                                 cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate);
}

// rdoq nonzero: the candidates are coded with HM's RDOQ (pnn_trquant_rdoq_host) under the lambda that decides
extern "C" int pnn_rd_pass_rdoq_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                     const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                     int sign_data_hiding, int rdoq, uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode,
                                     uint8_t* best_slot, double* best_cost, uint32_t* best_sse, uint64_t* best_rate)
{
    const int k = pnn_first_pass_list_size(width);
    if (k < 0) return refuse("the width of the target patch is not 4, 8, 16, 32 or 64.");
    if (n < 0) return refuse("negative batch size.");
    if (n > 0 && !cand_pred) return refuse("the candidate's predictions are NULL.");
    if (!cand_modes && !cand_costs && !best_mode && !best_slot && !best_cost && !best_sse && !best_rate) return refuse("every output is NULL.");
    if (!qps || nb_qps < 1 || nb_qps > 8) return refuse("the QPs are not 1 to 8 integers in [0, 51].");
    for (int qi = 0; qi < nb_qps; qi++) {
        if (qps[qi] < 0 || qps[qi] > 51) return refuse("the QPs are not 1 to 8 integers in [0, 51].");
        if (lambdas && !(std::isfinite(lambdas[qi]) && lambdas[qi] >= 0.)) return refuse("a lambda is negative or not finite.");
        if (rdoq && lambdas && !(lambdas[qi] > 0.)) return refuse("RDOQ with a lambda that is not above 0.");
    }
    const int k1 = k + 1;
    const size_t w2 = (size_t)width * width, pattern = (size_t)pattern_h * pattern_w;
    // the list, which also checks the patterns' sides, the inputs and the smoothing
    std::vector<uint8_t> list((size_t)std::max(n, 1) * k);
    if (pnn_hevc_mode_hads_hm_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, nullptr, nullptr, list.data(),
                                   nullptr) != PNN_OK)
        return refuse("the first pass refused the arguments (pattern sides, NULL inputs or smoothing).");
    if (n == 0) return PNN_OK;
    double lambda[8];
    for (int qi = 0; qi < nb_qps; qi++) lambda[qi] = lambdas ? lambdas[qi] : pnn_hm_intra_lambda(qps[qi]);

    const long chunk = std::min<long>(n, kChunk);
    std::vector<uint8_t> slot_modes(chunk * k1), scan_modes(chunk * k1), pred(chunk * k1 * w2), tgt(chunk * k1 * w2);
    std::vector<uint32_t> sse((size_t)nb_qps * chunk * k1);
    std::vector<uint64_t> rate((size_t)nb_qps * chunk * k1);
    for (long b0 = 0; b0 < n; b0 += chunk) {
        const long nb = std::min<long>(chunk, n - b0), slots = nb * k1;
        for (long i = 0; i < nb; i++) {
            const long b = b0 + i;
            bool listed = false;
            for (int s = 0; s < k; s++) {
                slot_modes[i * k1 + s] = list[b * k + s];
                listed = listed || list[b * k + s] == kCandidate;
            }
            slot_modes[i * k1 + k] = listed ? kUnused : kCandidate;
            for (int s = 0; s < k1; s++) {
                const int m = slot_modes[i * k1 + s];
                uint8_t* out = pred.data() + (i * k1 + s) * w2;
                std::copy(targets + b * w2, targets + (b + 1) * w2, tgt.data() + (i * k1 + s) * w2);
                if (m == kCandidate) std::copy(cand_pred + b * w2, cand_pred + (b + 1) * w2, out);
                else if (m == kUnused) std::copy(targets + b * w2, targets + (b + 1) * w2, out);         // a zero residual; never wins
                else if (pnn_hevc_intra_predict_hm(patterns + b * pattern, pattern_h, pattern_w, width, m, smoothing, out) != 0)
                    return refuse("the predictor refused a listed mode.");
                scan_modes[i * k1 + s] = m > 34 ? 0 : (uint8_t)m;                                        // 35 scans diagonally, as planar does
            }
        }
        if (pnn_trquant_rdoq_host(pred.data(), tgt.data(), width, (int)slots, scan_modes.data(), qps, nb_qps, sse.data(), nullptr, nullptr, nullptr,
                                  rate.data(), sign_data_hiding, rdoq, rdoq ? lambda : nullptr) != PNN_OK)
            return refuse("the transform coding refused the arguments.");
        for (int qi = 0; qi < nb_qps; qi++)
            for (long i = 0; i < nb; i++) {
                const size_t at = (size_t)qi * n + b0 + i;
                double best = std::numeric_limits<double>::infinity();
                int slot = kUnused, mode = kUnused;
                uint32_t d_best = 0;
                uint64_t r_best = 0;
                for (int s = 0; s < k1; s++) {
                    const int m = slot_modes[i * k1 + s];
                    const uint32_t d = sse[(size_t)qi * slots + i * k1 + s];
                    const uint64_t r = rate[(size_t)qi * slots + i * k1 + s];
                    double j = std::numeric_limits<double>::infinity();
                    if (m != kUnused) {
                        const double bits = lambda[qi] * (double)(r >> 15);                               // HM's whole written bits
                        j = (double)d + bits;
                    }
                    if (cand_costs) cand_costs[at * k1 + s] = j;
                    if (j < best) { best = j; slot = s; mode = m; d_best = d; r_best = r; }
                }
                if (best_mode) best_mode[at] = (uint8_t)mode;
                if (best_slot) best_slot[at] = (uint8_t)slot;
                if (best_cost) best_cost[at] = best;
                if (best_sse) best_sse[at] = d_best;
                if (best_rate) best_rate[at] = r_best;
            }
        if (cand_modes) std::copy(slot_modes.begin(), slot_modes.begin() + slots, cand_modes + b0 * k1);
    }
    return PNN_OK;
}
