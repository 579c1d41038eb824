// Host twin of HM's second intra pass as a column (no HIP in this file; include/pnn_hip.h, "the second intra pass"; DESIGN.md section
// 5l): per block the first-pass list (pnn_hevc_mode_hads_hm_host, the candidate competing as 35) plus 35 if the list lacks it, every
// candidate's prediction (pnn_hevc_intra_predict_hm, the candidate's own for 35) coded by pnn_trquant_sdh_host at every QP, J = D +
// lambda R per candidate, and the least J in list order under a strict <.  Nothing here but the composition and the decision: the
// entries it calls are the zero-tolerance yardsticks of their kernels, and this one is the yardstick of pnn_rd_pass_device.
// The cost is one IEEE multiply and one IEEE add in double; the pragmas below keep the compiler from contracting them into an FMA,
// as rd_cost does in rd_decide_kernel (pnn_hevc_intra.hip).
#include "../../include/pnn_hip.h"
#include "pnn_rd_pass_host.h"
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

#include "pnn_mode_signal.h"                                                   // (behind the pragma: its first-pass cost is two operations too)

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

// ---- The second pass with the side information HM charges (include/pnn_hip.h, "mode signalling") ----
// Again nothing but compositions: the definition is pnn_mode_signal.h, whose lines the kernels compile too, the Hadamard costs are
// pnn_hevc_mode_hads_hm_host's, the predictions pnn_hevc_intra_predict_hm's, the coding pnn_trquant_rdoq_host's at ONE QP per call --
// the list, and with it the slots, now depend on the QP.
namespace {

using namespace pnn;

int refuse_signal(const char* entry, const char* why)
{
    fprintf(stderr, "%s: %s\n", entry, why);
    return PNN_E_ARG;
}

bool neighbours_ok(const uint8_t* modes, int n, int pnn_flag)
{
    for (int i = 0; modes && i < n; i++)
        if (!msig::neighbour_ok(modes[i], pnn_flag)) return false;
    return true;
}

msig::Mpm block_mpm(const uint8_t* left, const uint8_t* above, long b)
{
    return msig::derive_mpm(msig::neighbour_dir(left ? left[b] : msig::kNoNeighbour), msig::neighbour_dir(above ? above[b] : msig::kNoNeighbour));
}

// the first pass of n blocks at one QP from their 35 + 1 Hadamard costs: list [n][K], costs [n][K], slots [n][K + 3], each NULL or that
template <int K>
void first_pass_signal(const uint32_t* hads, const uint32_t* cand, int n, const uint8_t* left, const uint8_t* above, const msig::FlagBits& f,
                       double sqrt_lambda, uint8_t* list_modes, double* list_costs, uint8_t* slot_modes)
{
    constexpr int S = K + msig::kExtraSlots;
    for (long b = 0; b < n; b++) {
        int lm[K], extra[msig::kExtraSlots];
        double lc[K];
        msig::list_and_slots<K>([&](int i) { return i < 35 ? hads[b * 35 + i] : cand[b]; }, block_mpm(left, above, b), f, sqrt_lambda, lm, lc, extra);
        for (int j = 0; j < K; j++) {
            if (list_modes) list_modes[b * K + j] = (uint8_t)lm[j];
            if (list_costs) list_costs[b * K + j] = lc[j];
            if (slot_modes) slot_modes[b * S + j] = (uint8_t)lm[j];
        }
        for (int t = 0; slot_modes && t < msig::kExtraSlots; t++) slot_modes[b * S + K + t] = (uint8_t)extra[t];
    }
}

// ... and the substitution codec's: 35 modes, mode 18's cost the candidate's, slots [n][K + 2]
template <int K>
void first_pass_substitution(const uint32_t* hads, const uint32_t* cand, int n, const uint8_t* left, const uint8_t* above, const msig::FlagBits& f,
                             double sqrt_lambda, uint8_t* list_modes, double* list_costs, uint8_t* slot_modes)
{
    constexpr int S = K + msig::kExtraSlotsSubstitution;
    for (long b = 0; b < n; b++) {
        int lm[K], extra[msig::kExtraSlotsSubstitution];
        double lc[K];
        msig::list_and_slots_substitution<K>([&](int i) { return i == msig::kSubstitutedMode ? cand[b] : hads[b * 35 + i]; },
                                             block_mpm(left, above, b), f, sqrt_lambda, lm, lc, extra);
        for (int j = 0; j < K; j++) {
            if (list_modes) list_modes[b * K + j] = (uint8_t)lm[j];
            if (list_costs) list_costs[b * K + j] = lc[j];
            if (slot_modes) slot_modes[b * S + j] = (uint8_t)lm[j];
        }
        for (int t = 0; slot_modes && t < msig::kExtraSlotsSubstitution; t++) slot_modes[b * S + K + t] = (uint8_t)extra[t];
    }
}

int extra_slots(int codec) { return codec ? msig::kExtraSlotsSubstitution : msig::kExtraSlots; }

// the bodies of pnn_first_pass_signal_host / pnn_rd_pass_signal_host (codec 0, under their names) and of the substitution codec's
// forms of the two (codec 1, under the *_codec_* names)
int first_pass_body(const char* entry, int codec, const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                    const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, const uint8_t* left_modes,
                    const uint8_t* above_modes, uint8_t* list_modes, double* list_costs, uint8_t* slot_modes);
int rd_pass_body(const char* entry, int codec, const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                 const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding, int rdoq,
                 const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode,
                 uint8_t* best_slot, double* best_cost, uint32_t* best_sse, uint64_t* best_rate, double* first_pass_costs,
                 uint64_t* best_side_rate, pnn::RdSlotCoder coder = nullptr, uint8_t* best_ts_flag = nullptr);

}  // namespace

extern "C" int pnn_rd_pass_slot_count(int width, int signalling)
{
    const int k = pnn_first_pass_list_size(width);
    return k < 0 ? -1 : k + (signalling ? msig::kExtraSlots : 1);
}

extern "C" int pnn_intra_mode_signal_host(const uint8_t* left_modes, const uint8_t* above_modes, int n, int qp, int pnn_flag, uint8_t* mpm,
                                          uint8_t* num_append, uint32_t* mode_frac_bits, uint32_t* cbf_frac_bits)
{
    const char* entry = "pnn_intra_mode_signal_host";
    if (n < 0) return refuse_signal(entry, "negative batch size.");
    if (qp < 0 || qp > 51) return refuse_signal(entry, "the QP is not in [0, 51].");
    if (!mpm && !num_append && !mode_frac_bits && !cbf_frac_bits) return refuse_signal(entry, "every output is NULL.");
    if (!neighbours_ok(left_modes, n, pnn_flag) || !neighbours_ok(above_modes, n, pnn_flag))
        return refuse_signal(entry, "a neighbour mode is not 0 .. 34, 35 (with the PNN flag only) or 255.");
    const msig::FlagBits f = msig::flag_bits(qp);
    for (long b = 0; b < n; b++) {
        const msig::Mpm m = block_mpm(left_modes, above_modes, b);
        if (mpm) { mpm[b * 3] = (uint8_t)m.m0; mpm[b * 3 + 1] = (uint8_t)m.m1; mpm[b * 3 + 2] = (uint8_t)m.m2; }
        if (num_append) num_append[b] = (uint8_t)m.num_append;
        for (int i = 0; mode_frac_bits && i < 36; i++) mode_frac_bits[b * 36 + i] = msig::mode_frac_bits(i, m, f, pnn_flag != 0);
    }
    for (int i = 0; cbf_frac_bits && i < 4; i++) cbf_frac_bits[i] = f.cbf[i >> 1][i & 1];
    return PNN_OK;
}

extern "C" int pnn_first_pass_signal_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                          const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                          const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* list_modes, double* list_costs,
                                          uint8_t* slot_modes)
{
    return first_pass_body("pnn_first_pass_signal_host", 0, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps,
                           lambdas, left_modes, above_modes, list_modes, list_costs, slot_modes);
}

namespace {

int first_pass_body(const char* entry, int codec, const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                    const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, const uint8_t* left_modes,
                    const uint8_t* above_modes, uint8_t* list_modes, double* list_costs, uint8_t* slot_modes)
{
    const int k = pnn_first_pass_list_size(width);
    if (k < 0) return refuse_signal(entry, "the width of the target patch is not 4, 8, 16, 32 or 64.");
    if (n < 0) return refuse_signal(entry, "negative batch size.");
    if (n > 0 && !cand_pred) return refuse_signal(entry, "the candidate's predictions are NULL.");
    if (!list_modes && !list_costs && !slot_modes) return refuse_signal(entry, "every output is NULL.");
    if (!qps || nb_qps < 1 || nb_qps > 8) return refuse_signal(entry, "the QPs are not 1 to 8 integers in [0, 51].");
    for (int qi = 0; qi < nb_qps; qi++) {
        if (qps[qi] < 0 || qps[qi] > 51) return refuse_signal(entry, "the QPs are not 1 to 8 integers in [0, 51].");
        if (lambdas && !(std::isfinite(lambdas[qi]) && lambdas[qi] >= 0.)) return refuse_signal(entry, "a lambda is negative or not finite.");
    }
    if (!neighbours_ok(left_modes, n, !codec) || !neighbours_ok(above_modes, n, !codec))
        return refuse_signal(entry, codec ? "a neighbour mode is not 0 .. 34 or 255." : "a neighbour mode is not 0 .. 35 or 255.");
    std::vector<uint32_t> hads((size_t)std::max(n, 1) * 35), cand((size_t)std::max(n, 1));
    if (pnn_hevc_mode_hads_hm_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, hads.data(),
                                   cand_pred ? cand.data() : nullptr, nullptr, nullptr) != PNN_OK)                  // (no candidate: no block)
        return refuse_signal(entry, "the first pass refused the arguments (pattern sides, NULL inputs or smoothing).");
    const int s = k + extra_slots(codec);
    for (int qi = 0; qi < nb_qps; qi++) {
        const msig::FlagBits f = msig::flag_bits(qps[qi]);
        const double sqrt_lambda = std::sqrt(lambdas ? lambdas[qi] : pnn_hm_intra_lambda(qps[qi]));   // TComRdCost::setLambda
        uint8_t* lm = list_modes ? list_modes + (size_t)qi * n * k : nullptr;
        double* lc = list_costs ? list_costs + (size_t)qi * n * k : nullptr;
        uint8_t* sm = slot_modes ? slot_modes + (size_t)qi * n * s : nullptr;
        if (codec && k == 8) first_pass_substitution<8>(hads.data(), cand.data(), n, left_modes, above_modes, f, sqrt_lambda, lm, lc, sm);
        else if (codec) first_pass_substitution<3>(hads.data(), cand.data(), n, left_modes, above_modes, f, sqrt_lambda, lm, lc, sm);
        else if (k == 8) first_pass_signal<8>(hads.data(), cand.data(), n, left_modes, above_modes, f, sqrt_lambda, lm, lc, sm);
        else first_pass_signal<3>(hads.data(), cand.data(), n, left_modes, above_modes, f, sqrt_lambda, lm, lc, sm);
    }
    return PNN_OK;
}

}  // namespace

extern "C" int pnn_rd_pass_signal_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                       const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                       int sign_data_hiding, int rdoq, int signalling, const uint8_t* left_modes, const uint8_t* above_modes,
                                       uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost,
                                       uint32_t* best_sse, uint64_t* best_rate, double* first_pass_costs, uint64_t* best_side_rate)
{
    const char* entry = "pnn_rd_pass_signal_host";
    if (!signalling) {
        if (first_pass_costs || best_side_rate) return refuse_signal(entry, "first_pass_costs or best_side_rate without signalling.");
        return pnn_rd_pass_rdoq_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding,
                                     rdoq, cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate);
    }
    return rd_pass_body(entry, 0, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, rdoq,
                        left_modes, above_modes, cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate, first_pass_costs,
                        best_side_rate);
}

namespace {

int rd_pass_body(const char* entry, int codec, const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                 const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding, int rdoq,
                 const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode,
                 uint8_t* best_slot, double* best_cost, uint32_t* best_sse, uint64_t* best_rate, double* first_pass_costs,
                 uint64_t* best_side_rate, pnn::RdSlotCoder coder, uint8_t* best_ts_flag)
{
    const int candidate = codec ? msig::kSubstitutedMode : kCandidate;            // the mode the caller's prediction stands for
    const int k = pnn_first_pass_list_size(width);
    if (k < 0) return refuse_signal(entry, "the width of the target patch is not 4, 8, 16, 32 or 64.");
    if (!cand_modes && !cand_costs && !best_mode && !best_slot && !best_cost && !best_sse && !best_rate && !first_pass_costs && !best_side_rate &&
        !best_ts_flag)
        return refuse_signal(entry, "every output is NULL.");
    for (int qi = 0; rdoq && lambdas && qps && qi < nb_qps && qi < 8; qi++)
        if (!(lambdas[qi] > 0.)) return refuse_signal(entry, "RDOQ with a lambda that is not above 0.");
    // the lists and slots of every QP, which also checks everything else but the outputs
    const int s = k + extra_slots(codec);
    std::vector<uint8_t> slots_all((size_t)std::max(nb_qps, 1) * std::max(n, 1) * s);
    if (const int rc = first_pass_body(codec ? "pnn_first_pass_codec_host" : "pnn_first_pass_signal_host", codec, patterns, pattern_h, pattern_w, targets,
                                       width, n, cand_pred, smoothing, qps, nb_qps, lambdas, left_modes, above_modes, nullptr, first_pass_costs,
                                       slots_all.data()))
        return rc;
    if (n == 0) return PNN_OK;
    const size_t w2 = (size_t)width * width, pattern = (size_t)pattern_h * pattern_w;
    const int ctx = msig::cbf_context(width);
    const long chunk = std::min<long>(n, kChunk);
    std::vector<uint8_t> scan_modes(chunk * s), pred(chunk * s * w2), tgt(chunk * s * w2);
    std::vector<uint32_t> sse(chunk * s), nonzero(chunk * s);
    std::vector<uint64_t> rate(chunk * s);
    std::vector<uint32_t> mode_bits(coder ? chunk * s : 0);                // transform skip: what each slot's
    std::vector<uint8_t> ts_flag(coder ? chunk * s : 0);                   // decision charges, and which form it keeps
    std::vector<int32_t> levels(width == 64 ? w2 : 0);
    std::vector<uint8_t> quadrant_coded(width == 64 ? chunk * s * 4 : 0);
    for (int qi = 0; qi < nb_qps; qi++) {
        const double lambda = lambdas ? lambdas[qi] : pnn_hm_intra_lambda(qps[qi]);
        const msig::FlagBits f = msig::flag_bits(qps[qi]);
        const uint8_t* slot_modes = slots_all.data() + (size_t)qi * n * s;
        for (long b0 = 0; b0 < n; b0 += chunk) {
            const long nb = std::min<long>(chunk, n - b0);
            for (long i = 0; i < nb; i++) {
                const long b = b0 + i;
                for (int j = 0; j < s; j++) {
                    const int m = slot_modes[b * s + j];
                    uint8_t* out = pred.data() + (i * s + j) * w2;
                    std::copy(targets + b * w2, targets + (b + 1) * w2, tgt.data() + (i * s + j) * w2);
                    if (m == candidate) std::copy(cand_pred + b * w2, cand_pred + (b + 1) * w2, out);
                    else if (m == kUnused) std::copy(targets + b * w2, targets + (b + 1) * w2, out);
                    else if (pnn_hevc_intra_predict_hm(patterns + b * pattern, pattern_h, pattern_w, width, m, smoothing, out) != 0)
                        return refuse_signal(entry, "the predictor refused a listed mode.");
                    scan_modes[i * s + j] = m > 34 ? 0 : (uint8_t)m;
                }
            }
            if (coder) {
                // both forms of every slot, decided per slot inside the candidate's coding (pnn_tskip.cpp's coder, so that this file
                // links without it): sse, count and rate are the kept form's
                for (long i = 0; i < nb; i++) {
                    const msig::Mpm mpm = block_mpm(left_modes, above_modes, b0 + i);
                    for (int j = 0; j < s; j++) {
                        const int m = slot_modes[(b0 + i) * s + j];
                        mode_bits[i * s + j] = m == kUnused ? 0u : msig::mode_frac_bits(m, mpm, f, codec ? 0 : 1);
                    }
                }
                if (coder(pred.data(), tgt.data(), (int)(nb * s), scan_modes.data(), qps[qi], sse.data(), nonzero.data(), rate.data(), sign_data_hiding,
                          rdoq, lambda, mode_bits.data(), ts_flag.data()) != PNN_OK)
                    return refuse_signal(entry, "the transform coding with transform skip refused the arguments.");
            } else if (pnn_trquant_rdoq_host(pred.data(), tgt.data(), width, (int)(nb * s), scan_modes.data(), qps + qi, 1, sse.data(), nonzero.data(), nullptr,
                                      nullptr, rate.data(), sign_data_hiding, rdoq, rdoq ? &lambda : nullptr) != PNN_OK)
                return refuse_signal(entry, "the transform coding refused the arguments.");
            // width 64: one cbf bin per quadrant (transform depth 1, context 0), so the levels themselves are asked for -- the stages entry
            // on the same slot with that context -- and counted quadrant by quadrant
            if (width == 64)
                for (long u = 0; u < nb * s; u++) {
                    if (pnn_trquant_stages_rdoq_host(pred.data() + u * w2, tgt.data() + u * w2, width, qps[qi], 0, sign_data_hiding, rdoq, lambda, 0,
                                                     nullptr, nullptr, nullptr, levels.data(), nullptr, nullptr) != PNN_OK)
                        return refuse_signal(entry, "the transform stages refused the arguments.");
                    for (int q = 0; q < 4; q++) {
                        bool any = false;
                        for (int y = 0; y < 32; y++)
                            for (int x = 0; x < 32; x++) any = any || levels[(size_t)((q >> 1) * 32 + y) * 64 + (q & 1) * 32 + x] != 0;
                        quadrant_coded[u * 4 + q] = any;
                    }
                }
            for (long i = 0; i < nb; i++) {
                const long b = b0 + i;
                const size_t at = (size_t)qi * n + b;
                const msig::Mpm mpm = block_mpm(left_modes, above_modes, b);
                double best = std::numeric_limits<double>::infinity();
                int slot = kUnused, mode = kUnused;
                uint32_t d_best = 0;
                uint64_t r_best = 0, side_best = 0;
                for (int j = 0; j < s; j++) {
                    const int m = slot_modes[b * s + j];
                    const uint32_t d = sse[i * s + j];
                    const uint64_t r = rate[i * s + j];                                                  // (0 for a unit without a level)
                    uint64_t side = 0;
                    double cost = std::numeric_limits<double>::infinity();
                    if (m != kUnused) {
                        side = msig::mode_frac_bits(m, mpm, f, codec ? 0 : 1);
                        if (width == 64)
                            for (int q = 0; q < 4; q++) side += msig::side_frac_bits(0, f, ctx, quadrant_coded[(i * s + j) * 4 + q]);
                        else side += msig::side_frac_bits(0, f, ctx, nonzero[i * s + j]);
                        const double bits = lambda * (double)((side + r) >> 15);                         // one shift over the sum
                        cost = (double)d + bits;
                    }
                    if (cand_costs) cand_costs[at * s + j] = cost;
                    if (cost < best) { best = cost; slot = j; mode = m; d_best = d; r_best = r; side_best = side; }
                }
                if (best_mode) best_mode[at] = (uint8_t)mode;
                if (best_slot) best_slot[at] = (uint8_t)slot;
                if (best_cost) best_cost[at] = best;
                if (best_sse) best_sse[at] = d_best;
                if (best_rate) best_rate[at] = r_best;
                if (best_side_rate) best_side_rate[at] = side_best;
                if (best_ts_flag) best_ts_flag[at] = coder && slot != kUnused ? ts_flag[i * s + slot] : (uint8_t)0;
            }
        }
        if (cand_modes) std::copy(slot_modes, slot_modes + (size_t)n * s, cand_modes + (size_t)qi * n * s);
    }
    return PNN_OK;
}

}  // namespace

// ---- The codec as an argument (include/pnn_hip.h, "the substitution codec") ----
extern "C" int pnn_rd_pass_codec_slot_count(int width, int signalling, int codec)
{
    if (codec == 0) return pnn_rd_pass_slot_count(width, signalling);
    const int k = pnn_first_pass_list_size(width);
    return codec != 1 || !signalling || k < 0 ? -1 : k + msig::kExtraSlotsSubstitution;
}

extern "C" int pnn_first_pass_codec_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                         const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                         const uint8_t* left_modes, const uint8_t* above_modes, int codec, uint8_t* list_modes, double* list_costs,
                                         uint8_t* slot_modes)
{
    if (codec == 0)
        return pnn_first_pass_signal_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, left_modes,
                                          above_modes, list_modes, list_costs, slot_modes);
    if (codec != 1) return refuse_signal("pnn_first_pass_codec_host", "the codec is not 0 (switch) or 1 (substitution).");
    return first_pass_body("pnn_first_pass_codec_host", 1, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas,
                           left_modes, above_modes, list_modes, list_costs, slot_modes);
}

extern "C" int pnn_rd_pass_codec_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                      const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                      int sign_data_hiding, int rdoq, int signalling, const uint8_t* left_modes, const uint8_t* above_modes, int codec,
                                      uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost,
                                      uint32_t* best_sse, uint64_t* best_rate, double* first_pass_costs, uint64_t* best_side_rate)
{
    const char* entry = "pnn_rd_pass_codec_host";
    if (codec == 0)
        return pnn_rd_pass_signal_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding,
                                       rdoq, signalling, left_modes, above_modes, cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse,
                                       best_rate, first_pass_costs, best_side_rate);
    if (codec != 1) return refuse_signal(entry, "the codec is not 0 (switch) or 1 (substitution).");
    if (!signalling) return refuse_signal(entry, "the substitution codec without signalling: HM never searches without the mode bits.");
    return rd_pass_body(entry, 1, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, rdoq,
                        left_modes, above_modes, cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate, first_pass_costs,
                        best_side_rate);
}

// The body with signalling for pnn_tskip.cpp, which brings the coder of the slots' two forms: this file does not
// name that file's entries, so it links without it.
int pnn::rd_pass_host_with_coder(const char* entry, int codec, const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width,
                                 int n, const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                                 int rdoq, const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* cand_modes, double* cand_costs,
                                 uint8_t* best_mode, uint8_t* best_slot, double* best_cost, uint32_t* best_sse, uint64_t* best_rate,
                                 double* first_pass_costs, uint64_t* best_side_rate, pnn::RdSlotCoder coder, uint8_t* best_ts_flag)
{
    return rd_pass_body(entry, codec, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, rdoq,
                        left_modes, above_modes, cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate, first_pass_costs,
                        best_side_rate, coder, best_ts_flag);
}

// The mode statistics (include/pnn_hip.h, "mode statistics"): the yardstick of mode_stats_kernel, three plain counts.
extern "C" int pnn_rd_pass_mode_stats_host(const uint8_t* slot_modes, int per_qp, int slots, const uint8_t* best_mode, int n, int nb_qps,
                                           uint32_t* stats)
{
    const char* entry = "pnn_rd_pass_mode_stats_host";
    if (n < 0) return refuse_signal(entry, "negative batch size.");
    if (slots < 1 || slots > 16) return refuse_signal(entry, "the slots per block are not 1 to 16.");
    if (nb_qps < 1 || nb_qps > 8) return refuse_signal(entry, "the QPs are not 1 to 8.");
    if (!stats) return refuse_signal(entry, "the output is NULL.");
    if (n > 0 && (!slot_modes || !best_mode)) return refuse_signal(entry, "the slot modes or the best modes are NULL.");
    std::fill(stats, stats + (size_t)nb_qps * 3 * 36, 0u);
    for (int qi = 0; qi < nb_qps; qi++) {
        uint32_t* out = stats + (size_t)qi * 3 * 36;
        for (long b = 0; b < n; b++) {
            const uint8_t* row = slot_modes + ((per_qp ? (size_t)qi * n : 0) + b) * slots;
            for (int j = 0; j < slots; j++) {
                if (row[j] > 35) continue;
                out[row[j]]++;
                if (j == 0) out[36 + row[j]]++;
            }
            const int winner = best_mode[(size_t)qi * n + b];
            if (winner <= 35) out[72 + winner]++;
        }
    }
    return PNN_OK;
}
