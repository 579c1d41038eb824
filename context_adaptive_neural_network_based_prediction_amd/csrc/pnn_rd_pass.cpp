// Host twin of HM's second intra pass as a column (no HIP in this file; include/pnn_hip.h, "the second intra pass"; DESIGN.md sections
// 5l, 5n, 5o): per block the first-pass list plus the slots appended behind it, every slot's prediction (pnn_hevc_intra_predict_hm, the
// candidate's own for 35) coded by pnn_trquant_rdoq_host, J = D + lambda R per slot, and the least J in slot order under a strict <.
// Nothing here but the composition and the decision: the entries it calls are the zero-tolerance yardsticks of their kernels, and this
// one is the yardstick of the pnn_rd_pass_*_device entries.
// Every entry fills one RdPassHostCall (pnn_rd_pass_host.h), or forwards to the entry one rung up; the checks, the slots' predictions
// (build_slots) and the decision of one block (decide_block) are each written once, behind two drivers: without signalling one list
// and one call of the transform coding serve every QP, with it the list depends on the QP.
// The cost is one IEEE multiply and one IEEE add in double; the pragmas below keep the compiler from contracting them into an FMA,
// as rd_cost does in rd_decide_kernel (pnn_hevc_intra.hip).
#include "../../include/pnn_hip.h"
#include "pnn_rd_pass_host.h"
#include "pnn_rdoq.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pnn_mode_signal.h"                                                   // (behind the pragma: its first-pass cost is two operations too)

namespace {

using namespace pnn;

constexpr int kCandidate = 35, kUnused = 255;
constexpr long kChunk = 1024;                                                  // blocks coded per call of the transform entry
const char* const kBadWidth = "the width of the target patch is not 4, 8, 16, 32 or 64.";

int refuse(const RdPassHostCall& q, const char* why) { return rd_pass_refuse(q.entry, why); }

// what both passes check first: the width, the batch, the candidate
int check_blocks(const RdPassHostCall& q)
{
    if (pnn_first_pass_list_size(q.width) < 0) return refuse(q, kBadWidth);
    if (q.n < 0) return refuse(q, "negative batch size.");
    if (q.n > 0 && !q.cand_pred) return refuse(q, "the candidate's predictions are NULL.");
    return PNN_OK;
}

// the QPs and the lambdas given, index by index; rdoq: the lambdas must be above 0 too
int check_qps_and_lambdas(const RdPassHostCall& q, int rdoq)
{
    if (!q.qps || q.nb_qps < 1 || q.nb_qps > 8) return refuse(q, "the QPs are not 1 to 8 integers in [0, 51].");
    for (int qi = 0; qi < q.nb_qps; qi++) {
        if (q.qps[qi] < 0 || q.qps[qi] > 51) return refuse(q, "the QPs are not 1 to 8 integers in [0, 51].");
        if (q.lambdas && !(std::isfinite(q.lambdas[qi]) && q.lambdas[qi] >= 0.)) return refuse(q, "a lambda is negative or not finite.");
        if (rdoq && q.lambdas && !(q.lambdas[qi] > 0.)) return refuse(q, "RDOQ with a lambda that is not above 0.");
    }
    return PNN_OK;
}

// The predictions, targets [nb][s][w][w] and scan modes [nb][s] of the slots of blocks b0 .. b0 + nb from their modes [nb][s]: the
// caller's prediction for `candidate` (35, or 18 under the substitution codec), HM's predictor for every other mode, the target itself
// for an unused slot -- a zero residual; never wins.  35 scans diagonally, as planar does.
int build_slots(const RdPassHostCall& q, long b0, long nb, const uint8_t* slot_modes, int s, int candidate, uint8_t* pred, uint8_t* tgt,
                uint8_t* scan_modes)
{
    const size_t w2 = (size_t)q.width * q.width, pattern = (size_t)q.pattern_h * q.pattern_w;
    for (long i = 0; i < nb; i++) {
        const uint8_t* target = q.targets + (b0 + i) * w2;
        for (int j = 0; j < s; j++) {
            const int m = slot_modes[i * s + j];
            uint8_t* out = pred + (i * s + j) * w2;
            std::copy(target, target + w2, tgt + (i * s + j) * w2);
            if (m == candidate) std::copy(q.cand_pred + (b0 + i) * w2, q.cand_pred + (b0 + i + 1) * w2, out);
            else if (m == kUnused) std::copy(target, target + w2, out);
            else if (pnn_hevc_intra_predict_hm(q.patterns + (b0 + i) * pattern, q.pattern_h, q.pattern_w, q.width, m, q.smoothing, out) != 0)
                return refuse(q, "the predictor refused a listed mode.");
            scan_modes[i * s + j] = m > 34 ? 0 : (uint8_t)m;
        }
    }
    return PNN_OK;
}

// The decision of one block at one QP, into element `at` of the outputs: J = D + lambda ((side + R) >> 15) of each of its s slots -- d,
// r, modes [s]; side_bits(j) what slot j is charged beside its levels, 0 without signalling; inf for an unused slot --, HM's whole
// written bits from one shift over the sum, and the first least J.  ts_flag: NULL or the slots' kept forms.
template <typename SideBits>
void decide_block(const RdPassHostOutputs& out, size_t at, int s, const uint8_t* modes, const uint32_t* d, const uint64_t* r, double lambda,
                  SideBits side_bits, const uint8_t* ts_flag)
{
    double best = std::numeric_limits<double>::infinity();
    int slot = kUnused, mode = kUnused;
    uint32_t d_best = 0;
    uint64_t r_best = 0, side_best = 0;
    for (int j = 0; j < s; j++) {
        uint64_t side = 0;
        double cost = std::numeric_limits<double>::infinity();
        if (modes[j] != kUnused) {
            side = side_bits(j);
            const double bits = lambda * (double)((side + r[j]) >> 15);
            cost = (double)d[j] + bits;
        }
        if (out.cand_costs) out.cand_costs[at * s + j] = cost;
        if (cost < best) { best = cost; slot = j; mode = modes[j]; d_best = d[j]; r_best = r[j]; side_best = side; }
    }
    if (out.best_mode) out.best_mode[at] = (uint8_t)mode;
    if (out.best_slot) out.best_slot[at] = (uint8_t)slot;
    if (out.best_cost) out.best_cost[at] = best;
    if (out.best_sse) out.best_sse[at] = d_best;
    if (out.best_rate) out.best_rate[at] = r_best;
    if (out.best_side_rate) out.best_side_rate[at] = side_best;
    if (out.best_ts_flag) out.best_ts_flag[at] = ts_flag && slot != kUnused ? ts_flag[slot] : (uint8_t)0;
}

// Without signalling: the list (pnn_hevc_mode_hads_hm_host's, the candidate competing as 35) does not depend on the QP, so ONE list and
// ONE call of the transform coding per chunk serve every QP; the slots are the list plus 35 if the list lacks it.
int rd_pass_without_signalling(const RdPassHostCall& q)
{
    const int n = q.n, nb_qps = q.nb_qps;
    if (const int rc = check_blocks(q)) return rc;
    if (!q.out.any()) return refuse(q, "every output is NULL.");
    if (const int rc = check_qps_and_lambdas(q, q.rdoq)) return rc;
    const int k = pnn_first_pass_list_size(q.width), k1 = k + 1;
    const size_t w2 = (size_t)q.width * q.width;
    // the list, which also checks the patterns' sides, the inputs and the smoothing
    std::vector<uint8_t> list((size_t)std::max(n, 1) * k);
    if (pnn_hevc_mode_hads_hm_host(q.patterns, q.pattern_h, q.pattern_w, q.targets, q.width, n, q.cand_pred, q.smoothing, nullptr, nullptr, list.data(),
                                   nullptr) != PNN_OK)
        return refuse(q, "the first pass refused the arguments (pattern sides, NULL inputs or smoothing).");
    if (n == 0) return PNN_OK;
    double lambda[8];
    for (int qi = 0; qi < nb_qps; qi++) lambda[qi] = q.lambda(qi);

    const long chunk = std::min<long>(n, kChunk);
    std::vector<uint8_t> slot_modes(chunk * k1), scan_modes(chunk * k1), pred(chunk * k1 * w2), tgt(chunk * k1 * w2);
    std::vector<uint32_t> sse((size_t)nb_qps * chunk * k1);
    std::vector<uint64_t> rate((size_t)nb_qps * chunk * k1);
    for (long b0 = 0; b0 < n; b0 += chunk) {
        const long nb = std::min<long>(chunk, n - b0), slots = nb * k1;
        for (long i = 0; i < nb; i++) {
            const uint8_t* listed = list.data() + (b0 + i) * k;
            std::copy(listed, listed + k, slot_modes.data() + i * k1);
            slot_modes[i * k1 + k] = std::find(listed, listed + k, kCandidate) != listed + k ? kUnused : kCandidate;
        }
        if (const int rc = build_slots(q, b0, nb, slot_modes.data(), k1, kCandidate, pred.data(), tgt.data(), scan_modes.data())) return rc;
        if (pnn_trquant_rdoq_host(pred.data(), tgt.data(), q.width, (int)slots, scan_modes.data(), q.qps, nb_qps, sse.data(), nullptr, nullptr, nullptr,
                                  rate.data(), q.sign_data_hiding, q.rdoq, q.rdoq ? lambda : nullptr) != PNN_OK)
            return refuse(q, "the transform coding refused the arguments.");
        for (int qi = 0; qi < nb_qps; qi++)
            for (long i = 0; i < nb; i++)
                decide_block(q.out, (size_t)qi * n + b0 + i, k1, &slot_modes[i * k1], &sse[(size_t)qi * slots + i * k1], &rate[(size_t)qi * slots + i * k1],
                             lambda[qi], [](int) { return (uint64_t)0; }, nullptr);
        if (q.out.cand_modes) std::copy(slot_modes.begin(), slot_modes.begin() + slots, q.out.cand_modes + b0 * k1);
    }
    return PNN_OK;
}

// ---- The side information HM charges (include/pnn_hip.h, "mode signalling") and the codec as an argument ("the
// substitution codec"; section 5o) ----
// Again nothing but compositions: the definition is pnn_mode_signal.h, whose lines the kernels compile too, the Hadamard costs are
// pnn_hevc_mode_hads_hm_host's, the predictions pnn_hevc_intra_predict_hm's, the coding pnn_trquant_rdoq_host's at ONE QP per call --
// the list, and with it the slots, now depend on the QP.

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

int extra_slots(int codec) { return codec ? msig::kExtraSlotsSubstitution : msig::kExtraSlots; }

// The first pass of q's blocks at one QP from their 35 + 1 Hadamard costs: list [n][K], costs [n][K], slots [n][K + extra], each NULL
// or that.  Codec 0: 36 modes, the candidate the 36th, slots K + 3.  Codec 1 (the substitution codec): 35 modes,
// mode 18's cost the candidate's, slots K + 2.
template <int K, int Codec>
void first_pass_lists(const RdPassHostCall& q, const uint32_t* hads, const uint32_t* cand, const msig::FlagBits& f, double sqrt_lambda,
                      uint8_t* list_modes, double* list_costs, uint8_t* slot_modes)
{
    constexpr int E = Codec ? msig::kExtraSlotsSubstitution : msig::kExtraSlots, S = K + E;
    for (long b = 0; b < q.n; b++) {
        int lm[K], extra[E];
        double lc[K];
        const msig::Mpm mpm = block_mpm(q.left, q.above, b);
        if constexpr (Codec)
            msig::list_and_slots_substitution<K>([&](int i) { return i == msig::kSubstitutedMode ? cand[b] : hads[b * 35 + i]; }, mpm, f, sqrt_lambda,
                                                 lm, lc, extra);
        else msig::list_and_slots<K>([&](int i) { return i < 35 ? hads[b * 35 + i] : cand[b]; }, mpm, f, sqrt_lambda, lm, lc, extra);
        for (int j = 0; j < K; j++) {
            if (list_modes) list_modes[b * K + j] = (uint8_t)lm[j];
            if (list_costs) list_costs[b * K + j] = lc[j];
            if (slot_modes) slot_modes[b * S + j] = (uint8_t)lm[j];
        }
        for (int t = 0; slot_modes && t < E; t++) slot_modes[b * S + K + t] = (uint8_t)extra[t];
    }
}

// the first pass with signalling under q's codec, at every QP: everything of q is checked here but the second pass's outputs
int first_pass(const RdPassHostCall& q, uint8_t* list_modes, double* list_costs, uint8_t* slot_modes)
{
    const int n = q.n, codec = q.codec;
    if (const int rc = check_blocks(q)) return rc;
    if (!list_modes && !list_costs && !slot_modes) return refuse(q, "every output is NULL.");
    if (const int rc = check_qps_and_lambdas(q, 0)) return rc;
    if (!neighbours_ok(q.left, n, !codec) || !neighbours_ok(q.above, n, !codec))
        return refuse(q, codec ? "a neighbour mode is not 0 .. 34 or 255." : "a neighbour mode is not 0 .. 35 or 255.");
    std::vector<uint32_t> hads((size_t)std::max(n, 1) * 35), cand((size_t)std::max(n, 1));
    if (pnn_hevc_mode_hads_hm_host(q.patterns, q.pattern_h, q.pattern_w, q.targets, q.width, n, q.cand_pred, q.smoothing, hads.data(),
                                   q.cand_pred ? cand.data() : nullptr, nullptr, nullptr) != PNN_OK)                // (no candidate: no block)
        return refuse(q, "the first pass refused the arguments (pattern sides, NULL inputs or smoothing).");
    const int k = pnn_first_pass_list_size(q.width), s = k + extra_slots(codec);
    const auto lists = codec ? (k == 8 ? first_pass_lists<8, 1> : first_pass_lists<3, 1>) : (k == 8 ? first_pass_lists<8, 0> : first_pass_lists<3, 0>);
    for (int qi = 0; qi < q.nb_qps; qi++)
        lists(q, hads.data(), cand.data(), msig::flag_bits(q.qps[qi]), std::sqrt(q.lambda(qi)),                     // TComRdCost::setLambda
              list_modes ? list_modes + (size_t)qi * n * k : nullptr, list_costs ? list_costs + (size_t)qi * n * k : nullptr,
              slot_modes ? slot_modes + (size_t)qi * n * s : nullptr);
    return PNN_OK;
}

// With signalling: the first pass's slots of every QP, then per QP and chunk the slots' predictions, their coding -- by q.coder in both
// forms where there is one (transform skip; pnn_tskip.cpp's, so that this file links without it) --, the decision
// with the mode bits and the cbf bin(s) charged.
int rd_pass_with_signalling(const RdPassHostCall& q)
{
    const int n = q.n, width = q.width, codec = q.codec;
    const int candidate = codec ? msig::kSubstitutedMode : kCandidate;            // the mode the caller's prediction stands for
    const int k = pnn_first_pass_list_size(width);
    if (k < 0) return refuse(q, kBadWidth);
    if (!q.out.any()) return refuse(q, "every output is NULL.");
    if (q.rdoq && !q.given_lambdas_are([](double lambda) { return lambda > 0.; })) return refuse(q, "RDOQ with a lambda that is not above 0.");
    // the lists and slots of every QP, which also checks everything else but the outputs: under the first pass's own name
    const int s = k + extra_slots(codec);
    std::vector<uint8_t> slots_all((size_t)std::max(q.nb_qps, 1) * std::max(n, 1) * s);
    RdPassHostCall first = q;
    first.entry = codec ? "pnn_first_pass_codec_host" : "pnn_first_pass_signal_host";
    if (const int rc = first_pass(first, nullptr, q.out.first_pass_costs, slots_all.data())) return rc;
    if (n == 0) return PNN_OK;
    const size_t w2 = (size_t)width * width;
    const int ctx = msig::cbf_context(width);
    const long chunk = std::min<long>(n, kChunk);
    std::vector<uint8_t> scan_modes(chunk * s), pred(chunk * s * w2), tgt(chunk * s * w2);
    std::vector<uint32_t> sse(chunk * s), nonzero(chunk * s);
    std::vector<uint64_t> rate(chunk * s);
    std::vector<uint32_t> mode_bits(q.coder ? chunk * s : 0);              // transform skip: what each slot's decision charges,
    std::vector<uint8_t> ts_flag(q.coder ? chunk * s : 0);                 // and which form it keeps
    std::vector<int32_t> levels(width == 64 ? w2 : 0);
    std::vector<uint8_t> quadrant_coded(width == 64 ? chunk * s * 4 : 0);
    for (int qi = 0; qi < q.nb_qps; qi++) {
        const int qp = q.qps[qi];
        const double lambda = q.lambda(qi);
        const msig::FlagBits f = msig::flag_bits(qp);
        const uint8_t* slot_modes = slots_all.data() + (size_t)qi * n * s;
        for (long b0 = 0; b0 < n; b0 += chunk) {
            const long nb = std::min<long>(chunk, n - b0);
            if (const int rc = build_slots(q, b0, nb, slot_modes + b0 * s, s, candidate, pred.data(), tgt.data(), scan_modes.data())) return rc;
            if (q.coder) {
                // both forms of every slot, decided per slot inside the candidate's coding: sse, count and rate are the kept form's
                for (long i = 0; i < nb; i++) {
                    const msig::Mpm mpm = block_mpm(q.left, q.above, b0 + i);
                    for (int j = 0; j < s; j++) {
                        const int m = slot_modes[(b0 + i) * s + j];
                        mode_bits[i * s + j] = m == kUnused ? 0u : msig::mode_frac_bits(m, mpm, f, !codec);
                    }
                }
                if (q.coder(pred.data(), tgt.data(), (int)(nb * s), scan_modes.data(), qp, sse.data(), nonzero.data(), rate.data(), q.sign_data_hiding,
                            q.rdoq, lambda, mode_bits.data(), ts_flag.data()) != PNN_OK)
                    return refuse(q, "the transform coding with transform skip refused the arguments.");
            } else if (pnn_trquant_rdoq_host(pred.data(), tgt.data(), width, (int)(nb * s), scan_modes.data(), &qp, 1, sse.data(), nonzero.data(), nullptr,
                                             nullptr, rate.data(), q.sign_data_hiding, q.rdoq, q.rdoq ? &lambda : nullptr) != PNN_OK)
                return refuse(q, "the transform coding refused the arguments.");
            // width 64: one cbf bin per quadrant (transform depth 1, context 0), so the levels themselves are asked for -- the stages entry
            // on the same slot with that context -- and counted quadrant by quadrant
            if (width == 64)
                for (long u = 0; u < nb * s; u++) {
                    if (pnn_trquant_stages_rdoq_host(pred.data() + u * w2, tgt.data() + u * w2, width, qp, 0, q.sign_data_hiding, q.rdoq, lambda, 0,
                                                     nullptr, nullptr, nullptr, levels.data(), nullptr, nullptr) != PNN_OK)
                        return refuse(q, "the transform stages refused the arguments.");
                    for (int quadrant = 0; quadrant < 4; quadrant++) {
                        bool any = false;
                        for (int y = 0; y < 32; y++)
                            for (int x = 0; x < 32; x++) any = any || levels[(size_t)((quadrant >> 1) * 32 + y) * 64 + (quadrant & 1) * 32 + x] != 0;
                        quadrant_coded[u * 4 + quadrant] = any;
                    }
                }
            for (long i = 0; i < nb; i++) {
                const long b = b0 + i;
                const msig::Mpm mpm = block_mpm(q.left, q.above, b);
                const auto side_bits = [&](int j) {                                                      // the mode bits and the cbf bin(s)
                    uint64_t side = msig::mode_frac_bits(slot_modes[b * s + j], mpm, f, !codec);
                    if (width == 64)
                        for (int quadrant = 0; quadrant < 4; quadrant++) side += msig::side_frac_bits(0, f, ctx, quadrant_coded[(i * s + j) * 4 + quadrant]);
                    else side += msig::side_frac_bits(0, f, ctx, nonzero[i * s + j]);
                    return side;
                };
                decide_block(q.out, (size_t)qi * n + b, s, slot_modes + b * s, &sse[i * s], &rate[i * s], lambda, side_bits,
                             q.coder ? &ts_flag[i * s] : nullptr);
            }
        }
        if (q.out.cand_modes) std::copy(slot_modes, slot_modes + (size_t)n * s, q.out.cand_modes + (size_t)qi * n * s);
    }
    return PNN_OK;
}


// one call, every argument in the record
int rd_pass(const RdPassHostCall& q) { return q.signalling ? rd_pass_with_signalling(q) : rd_pass_without_signalling(q); }

}  // namespace

int pnn::rd_pass_host_with_coder(const RdPassHostCall& q) { return rd_pass(q); }

extern "C" double pnn_hm_intra_lambda(int qp)
{
    // TEncSlice::calculateLambda, I slice, GOP size 1, 8-bit, no modifier: dQPFactor 0.57 * 2^((qp - 12) / 3)
    return pnn::rdoq::hm_intra_lambda(qp);
}

// ---- The entries of the second pass.  _host forwards to _rdoq_host; _signal_host without signalling and _codec_host with codec 0
// forward one rung down, so such a call is refused under the lower rung's name; every other call fills its record here. ----
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
    RdPassHostCall q{"pnn_rd_pass_host", patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas};
    q.sign_data_hiding = sign_data_hiding; q.rdoq = rdoq;
    q.out = {cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate, nullptr, nullptr, nullptr};
    return rd_pass(q);
}

extern "C" int pnn_rd_pass_signal_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                       const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                       int sign_data_hiding, int rdoq, int signalling, const uint8_t* left_modes, const uint8_t* above_modes,
                                       uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost,
                                       uint32_t* best_sse, uint64_t* best_rate, double* first_pass_costs, uint64_t* best_side_rate)
{
    const char* entry = "pnn_rd_pass_signal_host";
    if (!signalling) {
        if (first_pass_costs || best_side_rate) return rd_pass_refuse(entry, "first_pass_costs or best_side_rate without signalling.");
        return pnn_rd_pass_rdoq_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding,
                                     rdoq, cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate);
    }
    RdPassHostCall q{entry, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas};
    q.sign_data_hiding = sign_data_hiding; q.rdoq = rdoq; q.signalling = 1; q.left = left_modes; q.above = above_modes;
    q.out = {cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate, first_pass_costs, best_side_rate, nullptr};
    return rd_pass(q);
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
    if (codec != 1) return rd_pass_refuse(entry, "the codec is not 0 (switch) or 1 (substitution).");
    if (!signalling) return rd_pass_refuse(entry, "the substitution codec without signalling: HM never searches without the mode bits.");
    RdPassHostCall q{entry, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas};
    q.sign_data_hiding = sign_data_hiding; q.rdoq = rdoq; q.signalling = 1; q.codec = 1; q.left = left_modes; q.above = above_modes;
    q.out = {cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate, first_pass_costs, best_side_rate, nullptr};
    return rd_pass(q);
}

// ---- The entries of the first pass with signalling, of the slot counts and of the side information alone ----
extern "C" int pnn_first_pass_signal_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                          const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                          const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* list_modes, double* list_costs,
                                          uint8_t* slot_modes)
{
    RdPassHostCall q{"pnn_first_pass_signal_host", patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas};
    q.left = left_modes; q.above = above_modes;
    return first_pass(q, list_modes, list_costs, slot_modes);
}

extern "C" int pnn_first_pass_codec_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                         const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                         const uint8_t* left_modes, const uint8_t* above_modes, int codec, uint8_t* list_modes, double* list_costs,
                                         uint8_t* slot_modes)
{
    const char* entry = "pnn_first_pass_codec_host";
    if (codec == 0)
        return pnn_first_pass_signal_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas, left_modes,
                                          above_modes, list_modes, list_costs, slot_modes);
    if (codec != 1) return rd_pass_refuse(entry, "the codec is not 0 (switch) or 1 (substitution).");
    RdPassHostCall q{entry, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas};
    q.codec = 1; q.left = left_modes; q.above = above_modes;
    return first_pass(q, list_modes, list_costs, slot_modes);
}

extern "C" int pnn_rd_pass_slot_count(int width, int signalling)
{
    const int k = pnn_first_pass_list_size(width);
    return k < 0 ? -1 : k + (signalling ? msig::kExtraSlots : 1);
}

extern "C" int pnn_rd_pass_codec_slot_count(int width, int signalling, int codec)
{
    if (codec == 0) return pnn_rd_pass_slot_count(width, signalling);
    const int k = pnn_first_pass_list_size(width);
    return codec != 1 || !signalling || k < 0 ? -1 : k + msig::kExtraSlotsSubstitution;
}

extern "C" int pnn_intra_mode_signal_host(const uint8_t* left_modes, const uint8_t* above_modes, int n, int qp, int pnn_flag, uint8_t* mpm,
                                          uint8_t* num_append, uint32_t* mode_frac_bits, uint32_t* cbf_frac_bits)
{
    const char* entry = "pnn_intra_mode_signal_host";
    if (n < 0) return rd_pass_refuse(entry, "negative batch size.");
    if (qp < 0 || qp > 51) return rd_pass_refuse(entry, "the QP is not in [0, 51].");
    if (!mpm && !num_append && !mode_frac_bits && !cbf_frac_bits) return rd_pass_refuse(entry, "every output is NULL.");
    if (!neighbours_ok(left_modes, n, pnn_flag) || !neighbours_ok(above_modes, n, pnn_flag))
        return rd_pass_refuse(entry, "a neighbour mode is not 0 .. 34, 35 (with the PNN flag only) or 255.");
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

// The mode statistics (include/pnn_hip.h, "mode statistics"): the yardstick of mode_stats_kernel, three plain counts.
extern "C" int pnn_rd_pass_mode_stats_host(const uint8_t* slot_modes, int per_qp, int slots, const uint8_t* best_mode, int n, int nb_qps,
                                           uint32_t* stats)
{
    const char* entry = "pnn_rd_pass_mode_stats_host";
    if (n < 0) return rd_pass_refuse(entry, "negative batch size.");
    if (slots < 1 || slots > 16) return rd_pass_refuse(entry, "the slots per block are not 1 to 16.");
    if (nb_qps < 1 || nb_qps > 8) return rd_pass_refuse(entry, "the QPs are not 1 to 8.");
    if (!stats) return rd_pass_refuse(entry, "the output is NULL.");
    if (n > 0 && (!slot_modes || !best_mode)) return rd_pass_refuse(entry, "the slot modes or the best modes are NULL.");
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
