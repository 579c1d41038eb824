// Host twin of HM's transform skip for 4 x 4 luma units (no HIP in this file): the skipped form of a unit --
// residual << 5, the quantiser of the transform coding as it stands (xQuant with signBitHidingHDQ, or xRateDistOptQuant: nothing in
// either reads the flag with the range-extension tools off), dequantisation, (coefficient + 16) >> 5, reconstruction --, the bits
// codeCoeffNxN counts with the PPS flag on, and the decision of TEncSearch::xRecurIntraCodingLumaQT between the two forms.  The shared
// lines are pnn_tskip.h's; quantiser, hiding, RDOQ and the rate of the levels are the existing unit entries of pnn_trquant.cpp, called as
// they stand; the transformed form is pnn_trquant_rdoq_host's.  pnn_tskip.hip computes the same on the GPU;
// tests/test_hm_transform_skip.py pins this file to recorded outputs of HM itself, tests/test_transform_skip.py to a restatement.
#include "../../include/pnn_hip.h"
#include "pnn_rd_pass_host.h"
#include "pnn_rdoq.h"
#include "pnn_tskip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

// the decision's costs are doubles rounded once per operation: nothing in this file may be contracted
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace {

using namespace pnn::trquant;
namespace ts = pnn::tskip;

using pnn::rdoq::lambda_ok;

// the skipped form of one unit at one QP: coefficients, levels (as dequantised), HM's uiAbsSum, the decoded residual
int skipped_unit(const int* residual, int scan, int qp, bool sdh, bool rdoq, double lambda, int32_t* coeffs, int32_t* levels, int32_t* abs_sum,
                 int32_t* back)
{
    const QpConsts q = qp_consts(2, qp);
    for (int i = 0; i < 16; i++) coeffs[i] = ts::forward(residual[i]);
    *abs_sum = 0;
    if (rdoq) {
        if (const int rc = pnn_rdoq_unit_host(coeffs, 4, scan, qp, lambda, pnn::msig::cbf_context(ts::kWidth), sdh, levels, abs_sum)) return rc;
    } else {
        int32_t delta_u[16];
        for (int i = 0; i < 16; i++) {
            int mag;
            levels[i] = quant_level(coeffs[i], q, &mag, &delta_u[i]);
            *abs_sum += mag;
        }
        if (sdh)
            if (const int rc = pnn_sign_hide_unit_host(levels, coeffs, delta_u, 4, scan)) return rc;
    }
    for (int i = 0; i < 16; i++) back[i] = ts::inverse(dequant_level(levels[i], q));
    return PNN_OK;
}

}  // namespace

extern "C" int pnn_tskip_unit_host(const int32_t* residual, int scan, int qp, int sign_data_hiding, int rdoq, double lambda, int transform_skip,
                                   int32_t* coeffs, int32_t* levels, int32_t* abs_sum, int32_t* residual_back, uint64_t* bits, uint64_t* flag_bins)
{
    if (!residual) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (scan < 0 || scan > 2) { fprintf(stderr, "The scan is not 0 (diagonal), 1 (horizontal) or 2 (vertical).\n"); return PNN_E_ARG; }
    if (!qps_ok(&qp, 1)) { fprintf(stderr, "The QP does not belong to [0, 51].\n"); return PNN_E_ARG; }
    if (transform_skip != 0 && transform_skip != 1) { fprintf(stderr, "transform_skip is not 0 or 1.\n"); return PNN_E_ARG; }
    if (rdoq && !lambda_ok(lambda)) { fprintf(stderr, "RDOQ with a lambda that is not finite or not above 0.\n"); return PNN_E_ARG; }
    for (int i = 0; i < 16; i++)
        if (residual[i] < -255 || residual[i] > 255) { fprintf(stderr, "A residual sample is outside [-255, 255].\n"); return PNN_E_ARG; }
    const bool sdh = sign_data_hiding != 0;
    int32_t c[16], l[16], back[16], sum = 0;
    if (transform_skip) {
        if (const int rc = skipped_unit(residual, scan, qp, sdh, rdoq != 0, lambda, c, l, &sum, back)) return rc;
    } else {
        // the transformed form of the same residual, through the stages of the transform coding: target - prediction = residual
        uint8_t prediction[16], target[16];
        for (int i = 0; i < 16; i++) {
            prediction[i] = (uint8_t)(residual[i] < 0 ? -residual[i] : 0);
            target[i] = (uint8_t)(residual[i] < 0 ? 0 : residual[i]);
        }
        int32_t before[16];
        if (const int rc = pnn_trquant_stages_rdoq_host(prediction, target, 4, qp, scan, sdh, rdoq, rdoq ? lambda : 0., pnn::msig::cbf_context(ts::kWidth),
                                                        c, before, nullptr, l, nullptr, back)) return rc;
        if (rdoq) {
            int32_t again[16];
            if (const int rc = pnn_rdoq_unit_host(c, 4, scan, qp, lambda, pnn::msig::cbf_context(ts::kWidth), sdh, again, &sum)) return rc;
        } else {
            const QpConsts q = qp_consts(2, qp);
            for (int i = 0; i < 16; i++) { int mag; quant_level(c[i], q, &mag); sum += mag; }
        }
    }
    uint32_t nonzero = 0;
    for (int i = 0; i < 16; i++) nonzero += l[i] != 0;
    const ts::QpBits b = ts::qp_bits(qp);
    if (bits) {
        uint64_t level_bits = 0;
        if (const int rc = pnn_cabac_rate_levels_sdh_host(l, 4, scan, qp, sdh, &level_bits)) return rc;
        *bits = ts::unit_frac_bits(b, transform_skip, nonzero, level_bits);
    }
    for (int i = 0; i < 16; i++) {
        if (coeffs) coeffs[i] = c[i];
        if (levels) levels[i] = l[i];
        if (residual_back) residual_back[i] = back[i];
    }
    if (abs_sum) *abs_sum = sum;
    if (flag_bins) { flag_bins[0] = b.flag[0]; flag_bins[1] = b.flag[1]; }
    return PNN_OK;
}

extern "C" int pnn_trquant_tskip_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                                      int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon,
                                      uint64_t* rate, int sign_data_hiding, int rdoq, const double* lambdas, int transform_skip,
                                      const uint32_t* mode_bits, int charge_cbf, uint8_t* ts_flag)
{
    if (transform_skip < 0 || transform_skip > 2) { fprintf(stderr, "transform_skip is not 0 (off), 1 (forced) or 2 (decide).\n"); return PNN_E_ARG; }
    if (transform_skip && width != ts::kWidth) { fprintf(stderr, "Transform skip at a width other than 4.\n"); return PNN_E_ARG; }
    if (charge_cbf != 0 && charge_cbf != 1) { fprintf(stderr, "charge_cbf is not 0 or 1.\n"); return PNN_E_ARG; }
    if (!transform_skip) {
        const int rc = pnn_trquant_rdoq_host(predictions, targets, width, n, modes, qps, nb_qps, sses_recon, nb_nonzero, sum_abs_levels, recon, rate,
                                             sign_data_hiding, rdoq, lambdas);
        if (rc == PNN_OK && ts_flag)
            for (size_t i = 0; i < (size_t)nb_qps * n; i++) ts_flag[i] = 0;
        return rc;
    }
    if (n < 0 || (n > 0 && (!predictions || !targets))) { fprintf(stderr, "Bad batch size or NULL inputs.\n"); return PNN_E_ARG; }
    if (!qps_ok(qps, nb_qps)) { fprintf(stderr, "The QPs are not 1 to 8 integers in [0, 51].\n"); return PNN_E_ARG; }
    if (!sses_recon && !nb_nonzero && !sum_abs_levels && !recon && !rate && !ts_flag) { fprintf(stderr, "Every output is NULL.\n"); return PNN_E_ARG; }
    for (long b = 0; modes && b < n; b++)
        if (modes[b] > 34) { fprintf(stderr, "An intra mode is above 34.\n"); return PNN_E_ARG; }
    for (int qi = 0; (rdoq || transform_skip == 2) && lambdas && qi < nb_qps; qi++)
        if (!lambda_ok(lambdas[qi])) { fprintf(stderr, "A lambda that is not finite or not above 0.\n"); return PNN_E_ARG; }
    if (n == 0) return PNN_OK;
    const bool sdh = sign_data_hiding != 0, decide = transform_skip == 2;
    const size_t qn = (size_t)nb_qps * n;
    // the transformed form of every unit, as the transform coding leaves it (with the modes it needs them for: always, here, for the rate)
    std::vector<uint32_t> t_sse(decide ? qn : 0), t_nonzero(decide ? qn : 0), t_sum(decide ? qn : 0);
    std::vector<uint64_t> t_rate(decide ? qn : 0);
    std::vector<uint8_t> t_recon(decide ? qn * 16 : 0);
    if (decide)
        if (const int rc = pnn_trquant_rdoq_host(predictions, targets, width, n, modes, qps, nb_qps, t_sse.data(), t_nonzero.data(), t_sum.data(),
                                                 t_recon.data(), t_rate.data(), sign_data_hiding, rdoq, lambdas)) return rc;
    for (int qi = 0; qi < nb_qps; qi++) {
        const double lambda = lambdas ? lambdas[qi] : pnn::rdoq::hm_intra_lambda(qps[qi]);
        const ts::QpBits bits = ts::qp_bits(qps[qi]);
        for (long b = 0; b < n; b++) {
            const size_t at = (size_t)qi * n + b;
            const uint8_t* prediction = predictions + (size_t)b * 16;
            const uint8_t* target = targets + (size_t)b * 16;
            const int scan = modes ? pnn::cabac::scan_of_mode(2, modes[b]) : pnn::cabac::kScanDiag;
            int32_t residual[16], coeffs[16], levels[16], back[16], sum = 0;
            for (int i = 0; i < 16; i++) residual[i] = (int)target[i] - (int)prediction[i];
            if (const int rc = skipped_unit(residual, scan, qps[qi], sdh, rdoq != 0, lambda, coeffs, levels, &sum, back)) return rc;
            ts::Form s{0, 0, 0};
            uint8_t rec[16];
            for (int i = 0; i < 16; i++) {
                const int v = (int)prediction[i] + back[i], r = v < 0 ? 0 : v > 255 ? 255 : v, d = r - (int)target[i];
                rec[i] = (uint8_t)r;
                s.sse += (uint32_t)(d * d);
                s.nb_nonzero += levels[i] != 0;
            }
            if (const int rc = pnn_cabac_rate_levels_sdh_host(levels, 4, scan, qps[qi], sdh, &s.level_bits)) return rc;
            const ts::Form t = decide ? ts::Form{t_sse[at], t_nonzero[at], t_rate[at]} : ts::Form{0, 0, 0};
            const bool skipped = !decide || ts::skipped_wins(bits, mode_bits ? mode_bits[at] : 0u, charge_cbf, lambda, t, s);
            const ts::Form& f = skipped ? s : t;
            if (sses_recon) sses_recon[at] = f.sse;
            if (nb_nonzero) nb_nonzero[at] = f.nb_nonzero;
            if (sum_abs_levels) sum_abs_levels[at] = skipped ? (uint32_t)sum : t_sum[at];
            if (rate) rate[at] = ts::unit_frac_bits(bits, skipped, f.nb_nonzero, f.level_bits);
            if (ts_flag) ts_flag[at] = skipped;
            if (recon)
                for (int i = 0; i < 16; i++) recon[at * 16 + i] = skipped ? rec[i] : t_recon[at * 16 + i];
        }
    }
    return PNN_OK;
}

// ---- The second pass with transform skip (include/pnn_hip.h, "transform skip"): pnn_rd_pass.cpp's pass with
// signalling, whose record carries the coder below -- both forms, decided per slot under the slot's mode bits and the cbf bin ----
namespace {
int code_slots_both_forms(const uint8_t* pred, const uint8_t* targets, int n, const uint8_t* modes, int qp, uint32_t* sse, uint32_t* nonzero,
                          uint64_t* rate, int sign_data_hiding, int rdoq, double lambda, const uint32_t* mode_bits, uint8_t* ts_flag)
{
    return pnn_trquant_tskip_host(pred, targets, ts::kWidth, n, modes, &qp, 1, sse, nonzero, nullptr, nullptr, rate, sign_data_hiding, rdoq, &lambda, 2,
                                  mode_bits, 1, ts_flag);
}
}  // namespace

extern "C" int pnn_rd_pass_tskip_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                      const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                      int sign_data_hiding, int rdoq, int signalling, const uint8_t* left_modes, const uint8_t* above_modes, int codec,
                                      int transform_skip, uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot,
                                      double* best_cost, uint32_t* best_sse, uint64_t* best_rate, double* first_pass_costs, uint64_t* best_side_rate,
                                      uint8_t* best_ts_flag)
{
    const char* entry = "pnn_rd_pass_tskip_host";
    pnn::RdPassHostCall q{entry, patterns, pattern_h, pattern_w, targets, width, n, cand_pred, smoothing, qps, nb_qps, lambdas};
    q.sign_data_hiding = sign_data_hiding; q.rdoq = rdoq; q.signalling = 1; q.codec = codec; q.left = left_modes; q.above = above_modes;
    q.out = {cand_modes, cand_costs, best_mode, best_slot, best_cost, best_sse, best_rate, first_pass_costs, best_side_rate, best_ts_flag};
    q.coder = transform_skip ? code_slots_both_forms : nullptr;
    if (transform_skip != 0 && transform_skip != 1) return pnn::rd_pass_refuse(entry, "transform_skip is not 0 or 1.");
    if (transform_skip && width != ts::kWidth) return pnn::rd_pass_refuse(entry, "transform skip at a width other than 4.");
    if (codec != 0 && codec != 1) return pnn::rd_pass_refuse(entry, "the codec is not 0 (switch) or 1 (substitution).");
    if (!signalling) return pnn::rd_pass_refuse(entry, "the second pass with transform skip without signalling.");
    if (transform_skip && !q.given_lambdas_are(lambda_ok)) return pnn::rd_pass_refuse(entry, "transform skip with a lambda that is not finite or not above 0.");
    return pnn::rd_pass_host_with_coder(q);
}
