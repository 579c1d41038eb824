// Host twin of the open-loop transform coding (no HIP in this file): HM's residual path with RDOQ 0 on a prediction somebody else made
// -- residual, forward core transform (xTrMxN), quantisation (the non-RDOQ branch of xQuant, I slice), dequantisation (xDeQuant without
// scaling lists), inverse transform (xITrMxN), reconstruction -- for 8-bit luma intra blocks, per transform unit: T = w up to 32, the
// four 32 x 32 quadrants of the one prediction at w = 64 (this project's definition; HM would predict each quadrant again).  The
// definition is restated at the declarations in include/pnn_hip.h; the constants live in pnn_trquant_tables.h.  HM's butterflies are
// exact integer factorisations of the matrix products written here, so the integers are the same.  RDOQ with its own sign hiding is an
// option (pnn_rdoq.h, DESIGN.md section 5m: bit estimates from the state a slice STARTS with); no transform skip.  Sign-data hiding as
// xQuant does it with RDOQ 0 (signBitHidingHDQ) reads coefficients, levels, remainders and the scan only: it is
// here, behind a flag.  The CABAC rate of the levels is counted from the state a slice STARTS with:
// pnn_cabac_tables.h, whose lines the kernel compiles too.
// pnn_trquant.hip computes the same on the GPU; tests/test_gpu_trquant.py checks one against the other, tests/test_trquant.py pins this
// file to a numpy restatement and to recorded outputs of HM's own transforms.
#include "../../include/pnn_hip.h"
#include "pnn_cabac_tables.h"
#include "pnn_rdoq.h"
#include "pnn_trquant_tables.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

// RDOQ's costs are doubles rounded once per operation (pnn_rdoq.h): nothing in this file may be contracted
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace {

using namespace pnn::trquant;

bool width_ok(int w) { return w == 4 || w == 8 || w == 16 || w == 32 || w == 64; }
bool unit_size_ok(int t) { return t == 4 || t == 8 || t == 16 || t == 32; }
// 0, 1 or 2, and diagonal where the unit is above 8 x 8
bool scan_ok(int scan, int t) { return scan >= 0 && scan <= 2 && (t <= 8 || scan == pnn::cabac::kScanDiag); }
const char* const kBadScan = "The scan is not 0 (diagonal), 1 (horizontal) or 2 (vertical), or not diagonal above 8 x 8.\n";

// log2_t (2 .. 5) as a compile-time L: f(std::integral_constant<int, L>()), the one dispatch to the templates over the unit size
template <typename F>
auto with_log2(int log2_t, F f)
{
    switch (log2_t) {
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 5>());
    }
}

// M[k][x] of one unit size, dense
struct Matrix {
    int t, log2_t, m[32 * 32];
    explicit Matrix(int log2_t_) : t(1 << log2_t_), log2_t(log2_t_)
    {
        for (int k = 0; k < t; k++)
            for (int x = 0; x < t; x++) m[k * t + x] = matrix_coeff(log2_t, k, x);
    }
    int at(int k, int x) const { return m[k * t + x]; }
};

// the per-TU routine, stage by stage; every array is dense [t][t]
void forward(const Matrix& M, const int* residual, int* coeffs)
{
    const int t = M.t, s1 = fwd_shift1(M.log2_t), s2 = fwd_shift2(M.log2_t);
    int y1[32 * 32];
    for (int y = 0; y < t; y++)
        for (int k = 0; k < t; k++) {
            int acc = 0;
            for (int x = 0; x < t; x++) acc += residual[y * t + x] * M.at(k, x);
            y1[y * t + k] = (acc + (1 << (s1 - 1))) >> s1;
        }
    for (int l = 0; l < t; l++)
        for (int k = 0; k < t; k++) {
            int acc = 0;
            for (int y = 0; y < t; y++) acc += y1[y * t + k] * M.at(l, y);
            coeffs[l * t + k] = (acc + (1 << (s2 - 1))) >> s2;
        }
}

void inverse(const Matrix& M, const int* dequant, int* residual)
{
    const int t = M.t;
    int z[32 * 32];
    for (int y = 0; y < t; y++)
        for (int k = 0; k < t; k++) {
            int acc = 0;
            for (int l = 0; l < t; l++) acc += M.at(l, y) * dequant[l * t + k];
            z[y * t + k] = clip16((acc + (1 << (kInvShift1 - 1))) >> kInvShift1);
        }
    for (int y = 0; y < t; y++)
        for (int x = 0; x < t; x++) {
            int acc = 0;
            for (int k = 0; k < t; k++) acc += M.at(k, x) * z[y * t + k];
            residual[y * t + x] = clip16((acc + (1 << (kInvShift2 - 1))) >> kInvShift2);
        }
}

// HM's signBitHidingHDQ over one unit (levels, coeffs, delta_u dense [t][t]), line for line: the groups from the highest scan index
// down; the first one met with a level is the "last group", whose candidates start at its last level.  (HM's minPos = -1 cannot
// occur and its uiAbsSum >= 2 guard never decides: include/pnn_hip.h.)
template <int L>
void sign_hide_unit(int* levels, const int* coeffs, const int* delta_u, int scan)
{
    constexpr int T = 1 << L, LG = L - 2, NG = 1 << LG;
    bool last_group = true;                                                // no group with a level has been met yet
    for (int c = NG * NG - 1; c >= 0; c--) {
        int cx, cy, pos[16];
        pnn::cabac::scan_position<LG>(scan, c, &cx, &cy);
        for (int n = 0; n < 16; n++) {
            int x, y;
            pnn::cabac::scan_position<2>(scan, n, &x, &y);
            pos[n] = (cy * 4 + y) * T + cx * 4 + x;
        }
        int first = 16, last = -1, abs_sum = 0;
        for (int n = 15; n >= 0; n--)
            if (levels[pos[n]]) { last = n; break; }
        for (int n = 0; n < 16; n++)
            if (levels[pos[n]]) { first = n; break; }
        for (int n = first; n <= last; n++) abs_sum += levels[pos[n]];
        if (last < 0) continue;
        if (last - first >= kSbhThreshold) {
            const int signbit = levels[pos[first]] > 0 ? 0 : 1;
            if (signbit != (abs_sum & 1)) {
                int min_cost = kSdhForbidden, min_n = -1, final_change = 0;
                for (int n = last_group ? last : 15; n >= 0; n--) {
                    int change;
                    const int cost = sdh_cost(levels[pos[n]], coeffs[pos[n]], delta_u[pos[n]], n, first, signbit, &change);
                    if (cost < min_cost) { min_cost = cost; final_change = change; min_n = n; }
                }
                levels[pos[min_n]] = sdh_changed_level(levels[pos[min_n]], coeffs[pos[min_n]], final_change);
            }
        }
        last_group = false;
    }
}
void sign_hide_unit(int log2_t, int* levels, const int* coeffs, const int* delta_u, int scan)
{
    with_log2(log2_t, [&](auto L) { sign_hide_unit<decltype(L)::value>(levels, coeffs, delta_u, scan); });
}

// RDOQ (pnn_rdoq.h): what one QP and lambda turn into at a unit size -- the constants and the bit estimates
struct Rdoq {
    pnn::rdoq::Consts k;
    pnn::rdoq::EstBits e;
    Rdoq(int log2_t, int qp, double lambda) : k(pnn::rdoq::consts(log2_t, qp, lambda))
    {
        using namespace pnn::cabac;
        uint8_t init[kNumCtx], cbf[2];
        for (int i = 0; i < kNumCtx; i++) init[i] = (uint8_t)init_state(qp, init_value(i));
        for (int i = 0; i < 2; i++) cbf[i] = (uint8_t)init_state(qp, pnn::rdoq::kCbfInit[i]);
        int* words = &e.ctx[0][0];
        with_log2(log2_t, [&](auto L) {
            for (int i = 0; i < pnn::rdoq::kEstBitsWords; i++) words[i] = pnn::rdoq::est_bits_word<decltype(L)::value>(i, init, cbf, entropy_bits_table());
        });
    }
};
// the cbf context of the unit(s) of a block of width w: one transform unit of a 2N x 2N coding unit at 8, 16, 32; what HM reaches as N x N
// at 4; the quadrants at 64 (this project's definition)
int cbf_ctx_of_width(int w) { return w == 8 || w == 16 || w == 32 ? 1 : 0; }
using pnn::rdoq::lambda_ok;

// xRateDistOptQuant of one unit: the levels (and those in front of RDOQ's own hiding), returns uiAbsSum
template <int L>
int rdoq_unit(const int* coeffs, int scan, const QpConsts& q, const Rdoq& r, int cbf_ctx, bool sdh, int* levels, int* before_hiding)
{
    constexpr int TT = 1 << (2 * L);
    double cost[TT], cost0[TT], cost_sig[TT], group_sig[TT / 16];
    int rate_up[TT], rate_down[TT], sig_delta[TT];
    short delta_u[TT];
    for (int i = 0; i < TT; i++)
        cost0[i] = pnn::rdoq::uncoded_cost(pnn::rdoq::level_double(coeffs[pnn::rdoq::block_position<L>(scan, i)], q.scale, q.qbits), r.k.err_scale);
    const pnn::rdoq::Work w{cost, cost0, cost_sig, group_sig, rate_up, rate_down, sig_delta, delta_u};
    return pnn::rdoq::unit<L>(coeffs, scan, q.scale, q.qbits, r.k, r.e, cbf_ctx, sdh, levels, w, before_hiding);
}
int rdoq_unit(int log2_t, const int* coeffs, int scan, const QpConsts& q, const Rdoq& r, int cbf_ctx, bool sdh, int* levels, int* before_hiding)
{
    return with_log2(log2_t, [&](auto L) { return rdoq_unit<decltype(L)::value>(coeffs, scan, q, r, cbf_ctx, sdh, levels, before_hiding); });
}

// quantise -> (hide signs) -> dequantise -> inverse of one unit's coefficients at one QP; the counts ADD into *nb_nonzero / *sum_abs.
// levels: as quantised; hidden: what is dequantised (the same array may serve for both; equal without sdh)
// rdoq NULL: HM with RDOQ 0.  Otherwise xRateDistOptQuant with its own hiding: levels = what it leaves in front of the hiding (the
// same array as hidden may serve), delta_u is not written
void code_unit(const Matrix& M, const int* coeffs, const QpConsts& q, int scan, bool sdh, int* levels, int* delta_u, int* hidden, int* dequant,
               int* residual, uint32_t* nb_nonzero, uint32_t* sum_abs, const Rdoq* rdoq = nullptr, int cbf_ctx = 0)
{
    const int tt = M.t * M.t;
    if (rdoq)
        *sum_abs += (uint32_t)rdoq_unit(M.log2_t, coeffs, scan, q, *rdoq, cbf_ctx, sdh, hidden, levels == hidden ? nullptr : levels);
    else {
        for (int i = 0; i < tt; i++) {
            int mag;
            hidden[i] = levels[i] = quant_level(coeffs[i], q, &mag, &delta_u[i]);
            *sum_abs += (uint32_t)mag;                                         // HM's uiAbsSum: before the clip, before the hiding
        }
        if (sdh) sign_hide_unit(M.log2_t, hidden, coeffs, delta_u, scan);
    }
    for (int i = 0; i < tt; i++) {
        dequant[i] = dequant_level(hidden[i], q);
        *nb_nonzero += hidden[i] != 0;
    }
    inverse(M, dequant, residual);
}

// the unit at (uy, ux) of a w x w block: target - prediction
void unit_residual(const uint8_t* prediction, const uint8_t* target, int w, int t, int uy, int ux, int* residual)
{
    for (int y = 0; y < t; y++)
        for (int x = 0; x < t; x++) {
            const int i = (uy * t + y) * w + ux * t + x;
            residual[y * t + x] = (int)target[i] - (int)prediction[i];
        }
}

// the CABAC rate of one unit's levels (dense [t][t]) from the initial states of a QP
struct InitStates {
    uint8_t s[pnn::cabac::kNumCtx];
    explicit InitStates(int qp)
    {
        for (int i = 0; i < pnn::cabac::kNumCtx; i++) s[i] = (uint8_t)pnn::cabac::init_state(qp, pnn::cabac::init_value(i));
    }
};
uint64_t unit_rate(int log2_t, const int* levels, int scan, const InitStates& init, bool sdh)
{
    using namespace pnn::cabac;
    uint8_t state[kNumCtx];
    return with_log2(log2_t, [&](auto L) {
        constexpr int kL = decltype(L)::value;
        return sdh ? pnn::cabac::unit_rate<kL, true>(levels, scan, init.s, state, rom_tables())
                   : pnn::cabac::unit_rate<kL>(levels, scan, init.s, state, rom_tables());
    });
}

}  // namespace

extern "C" int pnn_trquant_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const int* qps, int nb_qps,
                                uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon)
{
    return pnn_trquant_rate_host(predictions, targets, width, n, nullptr, qps, nb_qps, sses_recon, nb_nonzero, sum_abs_levels, recon, nullptr);
}

extern "C" int pnn_trquant_rate_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                                     int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon,
                                     uint64_t* rate)
{
    return pnn_trquant_sdh_host(predictions, targets, width, n, modes, qps, nb_qps, sses_recon, nb_nonzero, sum_abs_levels, recon, rate, 0);
}

extern "C" int pnn_trquant_sdh_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                                    int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon,
                                    uint64_t* rate, int sign_data_hiding)
{
    return pnn_trquant_rdoq_host(predictions, targets, width, n, modes, qps, nb_qps, sses_recon, nb_nonzero, sum_abs_levels, recon, rate,
                                 sign_data_hiding, 0, nullptr);
}

extern "C" int pnn_trquant_rdoq_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                                     int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon,
                                     uint64_t* rate, int sign_data_hiding, int rdoq, const double* lambdas)
{
    const bool sdh = sign_data_hiding != 0;
    if (!width_ok(width)) { fprintf(stderr, "The width of the target patch is not 4, 8, 16, 32 or 64.\n"); return PNN_E_ARG; }
    if (n < 0 || (n > 0 && (!predictions || !targets))) { fprintf(stderr, "Bad batch size or NULL inputs.\n"); return PNN_E_ARG; }
    if (!qps_ok(qps, nb_qps)) { fprintf(stderr, "The QPs are not 1 to 8 integers in [0, 51].\n"); return PNN_E_ARG; }
    if (!sses_recon && !nb_nonzero && !sum_abs_levels && !recon && !rate) { fprintf(stderr, "Every output is NULL.\n"); return PNN_E_ARG; }
    if (modes && !rate && !sdh && !rdoq) { fprintf(stderr, "Intra modes without a rate output, sign-data hiding or RDOQ.\n"); return PNN_E_ARG; }
    for (long b = 0; modes && b < n; b++)
        if (modes[b] > 34) { fprintf(stderr, "An intra mode is above 34.\n"); return PNN_E_ARG; }
    for (int qi = 0; rdoq && lambdas && qi < nb_qps; qi++)
        if (!lambda_ok(lambdas[qi])) { fprintf(stderr, "RDOQ with a lambda that is not finite or not above 0.\n"); return PNN_E_ARG; }
    const Matrix M(log2_tu(width));
    const int t = M.t, units = width / t;
    const size_t w2 = (size_t)width * width;
    std::vector<InitStates> init;
    for (int qi = 0; rate && qi < nb_qps; qi++) init.emplace_back(qps[qi]);
    std::vector<Rdoq> rd;
    for (int qi = 0; rdoq && qi < nb_qps; qi++) rd.emplace_back(M.log2_t, qps[qi], lambdas ? lambdas[qi] : pnn::rdoq::hm_intra_lambda(qps[qi]));
    const int cbf_ctx = cbf_ctx_of_width(width);
    int residual[32 * 32], coeffs[32 * 32], levels[32 * 32], delta_u[32 * 32], dequant[32 * 32], decoded[32 * 32];
    for (long b = 0; b < n; b++) {
        const uint8_t* prediction = predictions + b * w2;
        const uint8_t* target = targets + b * w2;
        uint32_t sse[kMaxQps] = {}, nonzero[kMaxQps] = {}, sum_abs[kMaxQps] = {};
        uint64_t bits[kMaxQps] = {};
        const int scan = modes ? pnn::cabac::scan_of_mode(M.log2_t, modes[b]) : pnn::cabac::kScanDiag;
        for (int uy = 0; uy < units; uy++)
            for (int ux = 0; ux < units; ux++) {
                unit_residual(prediction, target, width, t, uy, ux, residual);
                forward(M, residual, coeffs);                                  // once per unit, whatever the number of QPs
                for (int qi = 0; qi < nb_qps; qi++) {
                    code_unit(M, coeffs, qp_consts(M.log2_t, qps[qi]), scan, sdh, levels, delta_u, levels, dequant, decoded, &nonzero[qi],
                              &sum_abs[qi], rdoq ? &rd[qi] : nullptr, cbf_ctx);
                    if (rate) bits[qi] += unit_rate(M.log2_t, levels, scan, init[qi], sdh);
                    for (int y = 0; y < t; y++)
                        for (int x = 0; x < t; x++) {
                            const size_t i = (size_t)(uy * t + y) * width + ux * t + x;
                            const int v = (int)prediction[i] + decoded[y * t + x], rec = v < 0 ? 0 : v > 255 ? 255 : v;
                            const int d = rec - (int)target[i];
                            sse[qi] += (uint32_t)(d * d);
                            if (recon) recon[((size_t)qi * n + b) * w2 + i] = (uint8_t)rec;
                        }
                }
            }
        for (int qi = 0; qi < nb_qps; qi++) {
            if (sses_recon) sses_recon[(size_t)qi * n + b] = sse[qi];
            if (nb_nonzero) nb_nonzero[(size_t)qi * n + b] = nonzero[qi];
            if (sum_abs_levels) sum_abs_levels[(size_t)qi * n + b] = sum_abs[qi];
            if (rate) rate[(size_t)qi * n + b] = bits[qi];
        }
    }
    return PNN_OK;
}

extern "C" int pnn_cabac_rate_levels_host(const int32_t* levels, int t, int scan, int qp, uint64_t* rate)
{
    return pnn_cabac_rate_levels_sdh_host(levels, t, scan, qp, 0, rate);
}

extern "C" int pnn_cabac_rate_levels_sdh_host(const int32_t* levels, int t, int scan, int qp, int sign_data_hiding, uint64_t* rate)
{
    if (!unit_size_ok(t)) { fprintf(stderr, "The unit size is not 4, 8, 16 or 32.\n"); return PNN_E_ARG; }
    if (!levels || !rate) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (!scan_ok(scan, t)) { fprintf(stderr, kBadScan); return PNN_E_ARG; }
    if (!qps_ok(&qp, 1)) { fprintf(stderr, "The QP does not belong to [0, 51].\n"); return PNN_E_ARG; }
    for (int i = 0; i < t * t; i++)
        if (levels[i] < -32768 || levels[i] > 32767) { fprintf(stderr, "A level is outside [-32768, 32767].\n"); return PNN_E_ARG; }
    *rate = unit_rate(log2_tu(t), levels, scan, InitStates(qp), sign_data_hiding != 0);
    return PNN_OK;
}

extern "C" int pnn_sign_hide_unit_host(int32_t* levels, const int32_t* coeffs, const int32_t* delta_u, int t, int scan)
{
    if (!unit_size_ok(t)) { fprintf(stderr, "The unit size is not 4, 8, 16 or 32.\n"); return PNN_E_ARG; }
    if (!levels || !coeffs || !delta_u) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (!scan_ok(scan, t)) { fprintf(stderr, kBadScan); return PNN_E_ARG; }
    for (int i = 0; i < t * t; i++) {
        if (levels[i] < -32768 || levels[i] > 32767) { fprintf(stderr, "A level is outside [-32768, 32767].\n"); return PNN_E_ARG; }
        if (delta_u[i] == INT32_MIN) { fprintf(stderr, "A remainder cannot be negated.\n"); return PNN_E_ARG; }
    }
    sign_hide_unit(log2_tu(t), levels, coeffs, delta_u, scan);
    return PNN_OK;
}

extern "C" int pnn_trquant_stages_host(const uint8_t* prediction, const uint8_t* target, int width, int qp, int32_t* coeffs, int32_t* levels,
                                       int32_t* dequant, int32_t* residual)
{
    return pnn_trquant_stages_sdh_host(prediction, target, width, qp, 0, 0, coeffs, levels, nullptr, nullptr, dequant, residual);
}

extern "C" int pnn_trquant_stages_sdh_host(const uint8_t* prediction, const uint8_t* target, int width, int qp, int scan, int sign_data_hiding,
                                           int32_t* coeffs, int32_t* levels, int32_t* delta_u, int32_t* levels_hidden, int32_t* dequant,
                                           int32_t* residual)
{
    return pnn_trquant_stages_rdoq_host(prediction, target, width, qp, scan, sign_data_hiding, 0, 0., 0, coeffs, levels, delta_u, levels_hidden,
                                        dequant, residual);
}

extern "C" int pnn_trquant_stages_rdoq_host(const uint8_t* prediction, const uint8_t* target, int width, int qp, int scan, int sign_data_hiding,
                                            int rdoq, double lambda, int cbf_ctx, int32_t* coeffs, int32_t* levels, int32_t* delta_u,
                                            int32_t* levels_hidden, int32_t* dequant, int32_t* residual)
{
    if (!width_ok(width)) { fprintf(stderr, "The width of the target patch is not 4, 8, 16, 32 or 64.\n"); return PNN_E_ARG; }
    if (!prediction || !target) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (!qps_ok(&qp, 1)) { fprintf(stderr, "The QP does not belong to [0, 51].\n"); return PNN_E_ARG; }
    if (!scan_ok(scan, width)) { fprintf(stderr, kBadScan); return PNN_E_ARG; }
    if (!coeffs && !levels && !delta_u && !levels_hidden && !dequant && !residual) { fprintf(stderr, "Every output is NULL.\n"); return PNN_E_ARG; }
    if (rdoq && !lambda_ok(lambda)) { fprintf(stderr, "RDOQ with a lambda that is not finite or not above 0.\n"); return PNN_E_ARG; }
    if (rdoq && cbf_ctx != 0 && cbf_ctx != 1) { fprintf(stderr, "The cbf context is not 0 or 1.\n"); return PNN_E_ARG; }
    const Matrix M(log2_tu(width));
    const int t = M.t, units = width / t;
    const QpConsts q = qp_consts(M.log2_t, qp);
    const Rdoq rd(M.log2_t, qp, rdoq ? lambda : 1.);
    int in[32 * 32], stage[6][32 * 32] = {};                                   // (RDOQ leaves delta_u as it is: zero)
    int32_t* const outs[6] = {coeffs, levels, delta_u, levels_hidden, dequant, residual};
    for (int uy = 0; uy < units; uy++)
        for (int ux = 0; ux < units; ux++) {
            uint32_t nonzero = 0, sum_abs = 0;
            unit_residual(prediction, target, width, t, uy, ux, in);
            forward(M, in, stage[0]);
            code_unit(M, stage[0], q, scan, sign_data_hiding != 0, stage[1], stage[2], stage[3], stage[4], stage[5], &nonzero, &sum_abs,
                      rdoq ? &rd : nullptr, cbf_ctx);
            for (int s = 0; s < 6; s++)                                        // each unit's arrays where the unit lies in the block
                if (outs[s])
                    for (int y = 0; y < t; y++)
                        for (int x = 0; x < t; x++) outs[s][(size_t)(uy * t + y) * width + ux * t + x] = stage[s][y * t + x];
        }
    return PNN_OK;
}

extern "C" int pnn_rdoq_unit_host(const int32_t* coeffs, int t, int scan, int qp, double lambda, int cbf_ctx, int sign_data_hiding, int32_t* levels,
                                  int32_t* abs_sum)
{
    if (!unit_size_ok(t)) { fprintf(stderr, "The unit size is not 4, 8, 16 or 32.\n"); return PNN_E_ARG; }
    if (!coeffs || !levels) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (!scan_ok(scan, t)) { fprintf(stderr, kBadScan); return PNN_E_ARG; }
    if (!qps_ok(&qp, 1)) { fprintf(stderr, "The QP does not belong to [0, 51].\n"); return PNN_E_ARG; }
    if (!lambda_ok(lambda)) { fprintf(stderr, "RDOQ with a lambda that is not finite or not above 0.\n"); return PNN_E_ARG; }
    if (cbf_ctx != 0 && cbf_ctx != 1) { fprintf(stderr, "The cbf context is not 0 or 1.\n"); return PNN_E_ARG; }
    for (int i = 0; i < t * t; i++)
        if (coeffs[i] < -32768 || coeffs[i] > 32767) { fprintf(stderr, "A coefficient is outside [-32768, 32767].\n"); return PNN_E_ARG; }
    const int log2_t = log2_tu(t);
    const int sum = rdoq_unit(log2_t, coeffs, scan, qp_consts(log2_t, qp), Rdoq(log2_t, qp, lambda), cbf_ctx, sign_data_hiding != 0, levels, nullptr);
    if (abs_sum) *abs_sum = sum;
    return PNN_OK;
}

extern "C" int pnn_rdoq_est_bits_host(int t, int qp, int32_t* est_bits)
{
    if (!unit_size_ok(t)) { fprintf(stderr, "The unit size is not 4, 8, 16 or 32.\n"); return PNN_E_ARG; }
    if (!est_bits) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (!qps_ok(&qp, 1)) { fprintf(stderr, "The QP does not belong to [0, 51].\n"); return PNN_E_ARG; }
    const Rdoq rd(log2_tu(t), qp, 1.);
    const int* words = &rd.e.ctx[0][0];
    for (int i = 0; i < pnn::rdoq::kEstBitsWords; i++) est_bits[i] = words[i];
    return PNN_OK;
}
