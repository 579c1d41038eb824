// The one home of HM's rate-distortion optimised quantisation of one transform unit (include/pnn_hip.h, "rate-distortion optimised
// quantisation"): TComTrQuant::xRateDistOptQuant of HM-16.15 restricted to 8-bit luma intra units of an I slice,
// flat quantisation, no transform skip -- the bit estimates TEncSbac::estBit fills, taken from the context states a slice of the QP
// STARTS with (no state ever moves here), the decision walk over the reverse scan, the zeroing of coefficient groups, the search for the
// best last position against "nothing coded", and RDOQ's own sign-data hiding.  Shared by the host twin (pnn_trquant.cpp, plain C++)
// and the kernel (pnn_trquant.hip): both compile THESE lines.  Every cost is an IEEE double, each operation rounded once, in HM's order:
// nothing here may be contracted into a fused multiply-add, hence the pragma in every function that holds a double.  The constants that
// need a division or a power (Consts) are made on the host and handed over.
#pragma once

#include "pnn_cabac_tables.h"

#include <cmath>

#if defined(__clang__)
#define PNN_RDOQ_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PNN_RDOQ_NO_CONTRACT
#endif

namespace pnn {
namespace rdoq {

constexpr double kMaxDouble = 1.7e+308;        // HM's MAX_DOUBLE
constexpr int kCbfInit[2] = {111, 141};        // H.265 table 9-22 / HM's INIT_QT_CBF, I slice, luma: transform depth > 0, depth 0
constexpr long long kRdFactorMax = 1ll << 52;  // see consts()

// HM's lambda of an I slice (TEncSlice::calculateLambda, GOP size 1, 8-bit, no modifier), the one home of the formula: pnn_hm_intra_lambda
// returns it, and it is what RDOQ runs under when the caller hands no lambda
inline double hm_intra_lambda(int qp) { return 0.57 * std::pow(2.0, (qp - 12) / 3.0); }
// a lambda RDOQ, and the decision of transform skip, can run under: the one home of the check
inline bool lambda_ok(double lambda) { return std::isfinite(lambda) && lambda > 0.; }

// What a QP and a lambda turn into, computed in double on the host, in HM's operation order:
//   err_scale: getErrScaleCoeffNoScalingList as setErrScaleCoeff leaves it -- 2^15 * 2^(-2 transformShift) / scale / scale / 1;
//   rd_factor: (Int64)(inv * inv * (1 << 2 per) / lambda / 16 / 1 + 0.5) of RDOQ's sign hiding.  HM's conversion is undefined once the
//     value leaves 64 bits; here it saturates at 2^52 (lambda below about 5e-9), THIS PROJECT'S DEFINITION, so that rd_factor * deltaU
//     stays inside 64 bits.  Below that it is HM's number.
struct Consts { double lambda, err_scale; long long rd_factor; };
inline Consts consts(int log2_t, int qp, double lambda)
{
    PNN_RDOQ_NO_CONTRACT
    static constexpr int kQuantScale[6] = {26214, 23302, 20560, 18396, 16384, 14564};
    static constexpr int kInvQuantScale[6] = {40, 45, 51, 57, 64, 72};
    const int per = qp / 6, rem = qp % 6, transform_shift = 7 - log2_t;
    Consts c;
    c.lambda = lambda;
    double e = (double)(1 << 15);
    e = e * std::pow(2.0, -2.0 * transform_shift);
    c.err_scale = e / kQuantScale[rem] / kQuantScale[rem] / 1;
    const double inv = (double)kInvQuantScale[rem];
    const double f = inv * inv * (1 << (2 * per)) / lambda / 16 / 1 + 0.5;
    c.rd_factor = f >= (double)kRdFactorMax ? kRdFactorMax : (long long)f;
    return c;
}

// The tables estBit fills, luma: bits of bin b in context i of pnn_cabac_tables.h's numbering (significantBits = kCtxSig .., with HM's
// index the offset from kCtxSig; m_greaterOneBits = kCtxOne ..; m_levelAbsBits = kCtxAbs ..; significantCoeffGroupBits = kCtxGroup ..),
// lastXBits / lastYBits with their cumulative sums up to group 2 L - 1, and blockCbpBits of the two luma contexts.
struct EstBits {
    int ctx[cabac::kNumCtx][2];
    int last_x[10], last_y[10];
    int cbf[2][2];
};
constexpr int kEstBitsWords = sizeof(EstBits) / 4;

// word i of the tables of unit size 2^L at a QP (so that a workgroup can fill them one word per lane): init_states are the QP's kNumCtx
// initial states, cbf_states those of the two cbf contexts, bits the entropy-bits table
template <int L>
PNN_TQ_HD inline int est_bits_word(int i, const uint8_t* init_states, const uint8_t* cbf_states, const int* bits)
{
    constexpr int offset = 3 * (L - 2) + ((L - 1) >> 2), shift = (L + 1) >> 2, top = 2 * L - 1;
    if (i < 2 * cabac::kNumCtx) return bits[init_states[i >> 1] ^ (i & 1)];
    i -= 2 * cabac::kNumCtx;
    if (i < 20) {
        const int base = i < 10 ? cabac::kCtxLastX : cabac::kCtxLastY, g = i % 10;
        if (g > top) return 0;
        int sum = 0;
        for (int k = 0; k < top; k++)
            if (k < g) sum += bits[init_states[base + offset + (k >> shift)] ^ 1];
        return g < top ? sum + bits[init_states[base + offset + (g >> shift)]] : sum;
    }
    i -= 20;
    return bits[cbf_states[i >> 1] ^ (i & 1)];
}

// per-position quantities that do not depend on the walk
PNN_TQ_HD inline int level_double(int coeff, int scale, int qbits)
{
    const long long a = coeff < 0 ? -(long long)coeff : coeff, t = a * scale, cap = 2147483647ll - (1ll << (qbits - 1));
    return (int)(t < cap ? t : cap);
}
PNN_TQ_HD inline int max_abs_level(int level_dbl, int qbits)
{
    const int v = (level_dbl + (1 << (qbits - 1))) >> qbits;
    return v < 32767 ? v : 32767;
}
PNN_TQ_HD inline double uncoded_cost(int level_dbl, double err_scale)
{
    PNN_RDOQ_NO_CONTRACT
    const double err = (double)level_dbl;
    return err * err * err_scale;
}

// xGetICRate without extended precision
PNN_TQ_HD inline int ic_rate(int abs_level, int one_ctx, int abs_ctx, int rice, int c1_idx, int c2_idx, const EstBits& e)
{
    const int base = c1_idx < 8 ? 2 + (c2_idx < 1) : 1;
    int rate = cabac::kBypassBits;                                           // the sign
    if (abs_level >= base) {
        rate += cabac::remaining_bins(abs_level - base, rice) << 15;
        if (c1_idx < 8) {
            rate += e.ctx[cabac::kCtxOne + one_ctx][1];
            if (c2_idx < 1) rate += e.ctx[cabac::kCtxAbs + abs_ctx][1];
        }
    } else if (abs_level == 1) rate += e.ctx[cabac::kCtxOne + one_ctx][0];
    else if (abs_level == 2) rate += e.ctx[cabac::kCtxOne + one_ctx][1] + e.ctx[cabac::kCtxAbs + abs_ctx][0];
    else rate = 0;
    return rate;
}

// xGetRateLast, the caller has swapped x and y for the vertical scan
PNN_TQ_HD inline double rate_last(int x, int y, double lambda, const EstBits& e)
{
    PNN_RDOQ_NO_CONTRACT
    const int gx = cabac::last_group(x), gy = cabac::last_group(y);
    double cost = (double)(e.last_x[gx] + e.last_y[gy]);
    if (gx > 3) cost += 32768. * (double)((gx - 2) >> 1);
    if (gy > 3) cost += 32768. * (double)((gy - 2) >> 1);
    return lambda * cost;
}

// the working memory of one unit, T * T entries each, indexed by SCAN position (group_sig: one per coefficient group).  cost0 is an
// INPUT: uncoded_cost of every position, which the caller fills (the kernel with one lane per position).  deltaU of a unit whose
// coefficients lie in [-32768, 32767] lies in [-128, 640]: 16 bits hold it
struct Work {
    double* cost; double* cost0; double* cost_sig; double* group_sig;
    int* rate_up; int* rate_down; int* sig_delta; short* delta_u;     // read by the hiding only: not written without sdh (may be NULL)
};

// block position of scan position i
template <int L>
PNN_TQ_HD inline int block_position(int scan, int i)
{
    int cx, cy, x, y;
    cabac::scan_position<L - 2>(scan, i >> 4, &cx, &cy);
    cabac::scan_position<2>(scan, i & 15, &x, &y);
    return ((cy * 4 + y) << L) + cx * 4 + x;
}

// xRateDistOptQuant on one unit: coeffs dense [T][T] (T = 1 << L) -> levels dense [T][T]; returns HM's uiAbsSum (the sum of the
// magnitudes up to the best last position, before the hiding).  before_hiding NULL or [T][T]: the levels RDOQ leaves in front of its
// sign hiding (what `levels` holds without sdh).
template <int L>
PNN_TQ_HD inline int unit(const int* coeffs, int scan, int scale, int qbits, const Consts& k, const EstBits& e, int cbf_ctx, bool sdh, int* levels,
                          const Work& w, int* before_hiding)
{
    PNN_RDOQ_NO_CONTRACT
    using namespace cabac;
    constexpr int T = 1 << L, TT = T * T, LG = L - 2, NG = 1 << LG, NGG = NG * NG;
    constexpr int sig_first = L == 2 ? 0 : L == 3 ? 9 : 21;
    const int sig_base = kCtxSig + sig_first + (L == 3 && scan != kScanDiag ? 6 : 0);
    const double lambda = k.lambda;
    double block_uncoded = 0., base_cost = 0.;
    unsigned long long group_flags = 0;                                      // bit cy * NG + cx: uiSigCoeffGroupFlag
    int ctx_set = 0, c1 = 1, c2 = 0, c1_idx = 0, c2_idx = 0, rice = 0, last_pos = -1, last_group_pos = -1;
#pragma unroll 1
    for (int g = NGG - 1; g >= 0; g--) {
        int cx, cy;
        scan_position<LG>(scan, g, &cx, &cy);
        const int right = cx < NG - 1 ? (int)((group_flags >> (cy * NG + cx + 1)) & 1) : 0;
        const int below = cy < NG - 1 ? (int)((group_flags >> ((cy + 1) * NG + cx)) & 1) : 0;
        const int pattern = right + 2 * below;
        const unsigned long long own = 1ull << (cy * NG + cx);
        double sig_cost = 0., sig_cost_0 = 0., coded_level_and_dist = 0., uncoded_dist = 0.;   // coeffGroupRDStats
        int nnz_before_pos0 = 0;
        w.group_sig[g] = 0.;
#pragma unroll 1
        for (int n = 15; n >= 0; n--) {
            const int i = g * 16 + n;
            int x, y;
            scan_position<2>(scan, n, &x, &y);
            const int px = cx * 4 + x, py = cy * 4 + y, pos = (py << L) + px;
            const double cost0 = w.cost0[i];
            block_uncoded += cost0;
            const int coeff = coeffs[pos];
            if (last_pos < 0 && coeff == 0) {                                // in front of the first level: nothing but the uncoded cost
                levels[pos] = 0;
                base_cost += cost0;
                continue;
            }
            const int level_dbl = level_double(coeff, scale, qbits), max_level = max_abs_level(level_dbl, qbits);
            if (max_level > 0 && last_pos < 0) {
                last_pos = i;
                ctx_set = g > 0 ? 2 : 0;
                last_group_pos = g;
            }
            if (last_pos < 0) {
                levels[pos] = 0;
                base_cost += cost0;
                continue;
            }
            const int one_ctx = 4 * ctx_set + c1, abs_ctx = ctx_set + c2;
            const bool is_last = i == last_pos;
            // xGetCodedLevel
            int level = 0, sig_ctx = 0;
            double coded = kMaxDouble, coded_sig = 0., curr_sig = 0.;
            if (!is_last) {
                if (px + py == 0) sig_ctx = kCtxSig;
                else if (L == 2) sig_ctx = sig_base + sig_ctx_4x4(px, py);
                else {
                    const int s = pattern == 0 ? x + y : pattern == 1 ? y : pattern == 2 ? x : 0;
                    const int cnt = pattern == 0 ? (s >= 3 ? 0 : s >= 1 ? 1 : 2) : pattern == 3 ? 2 : (s >= 2 ? 0 : s >= 1 ? 1 : 2);
                    sig_ctx = sig_base + (cx + cy > 0 ? 3 : 0) + cnt;
                }
                if (max_level < 3) {
                    coded_sig = lambda * (double)e.ctx[sig_ctx][0];
                    coded = cost0 + coded_sig;
                }
                curr_sig = lambda * (double)e.ctx[sig_ctx][1];
            }
            if (max_level > 0) {
                const int min_level = max_level > 1 ? max_level - 1 : 1;
                for (int a = max_level; a >= min_level; a--) {
                    const double err = (double)(level_dbl - (a << qbits));
                    double curr = err * err * k.err_scale + lambda * (double)ic_rate(a, one_ctx, abs_ctx, rice, c1_idx, c2_idx, e);
                    curr += curr_sig;
                    if (curr < coded) { level = a; coded = curr; coded_sig = curr_sig; }
                }
            }
            w.cost[i] = coded;
            w.cost_sig[i] = coded_sig;
            if (sdh) {
                w.sig_delta[i] = is_last ? 0 : e.ctx[sig_ctx][1] - e.ctx[sig_ctx][0];
                w.delta_u[i] = (short)((level_dbl - (level << qbits)) >> (qbits - 8));
                if (level > 0) {
                    const int now = ic_rate(level, one_ctx, abs_ctx, rice, c1_idx, c2_idx, e);
                    w.rate_up[i] = ic_rate(level + 1, one_ctx, abs_ctx, rice, c1_idx, c2_idx, e) - now;
                    w.rate_down[i] = ic_rate(level - 1, one_ctx, abs_ctx, rice, c1_idx, c2_idx, e) - now;
                } else {
                    w.rate_up[i] = e.ctx[kCtxOne + one_ctx][0];
                    w.rate_down[i] = 0;
                }
            }
            levels[pos] = level;
            base_cost += coded;
            const int base_level = c1_idx < 8 ? 2 + (c2_idx < 1) : 1;
            if (level >= base_level && level > (3 << rice) && rice < 4) rice++;
            if (level >= 1) c1_idx++;
            if (level > 1) { c1 = 0; c2 += c2 < 2; c2_idx++; }
            else if (c1 < 3 && c1 > 0 && level) c1++;
            if (n == 0 && i > 0) {                                           // the context set of the next group
                ctx_set = (g - 1 > 0 ? 2 : 0) + (c1 == 0);
                c1 = 1; c2 = 0; c1_idx = 0; c2_idx = 0; rice = 0;
            }
            sig_cost += coded_sig;
            if (n == 0) sig_cost_0 = coded_sig;
            if (level) {
                group_flags |= own;
                coded_level_and_dist += coded - coded_sig;
                uncoded_dist += cost0;
                if (n != 0) nnz_before_pos0++;
            }
        }
        if (last_group_pos < 0) continue;
        if (g == 0) { group_flags |= own; continue; }
        const int group_ctx = kCtxGroup + (right | below);
        if (!(group_flags & own)) {
            base_cost += lambda * (double)e.ctx[group_ctx][0] - sig_cost;
            w.group_sig[g] = lambda * (double)e.ctx[group_ctx][0];
        } else if (g < last_group_pos) {
            if (nnz_before_pos0 == 0) {
                base_cost -= sig_cost_0;
                sig_cost -= sig_cost_0;
            }
            double zero_cost = base_cost;
            base_cost += lambda * (double)e.ctx[group_ctx][1];
            zero_cost += lambda * (double)e.ctx[group_ctx][0];
            w.group_sig[g] = lambda * (double)e.ctx[group_ctx][1];
            zero_cost += uncoded_dist;
            zero_cost -= coded_level_and_dist;
            zero_cost -= sig_cost;
            if (zero_cost < base_cost) {
                group_flags &= ~own;
                base_cost = zero_cost;
                w.group_sig[g] = lambda * (double)e.ctx[group_ctx][0];
#pragma unroll 1
                for (int n = 15; n >= 0; n--) {
                    const int i = g * 16 + n, pos = block_position<L>(scan, i);
                    if (levels[pos]) {
                        levels[pos] = 0;
                        w.cost[i] = w.cost0[i];
                        w.cost_sig[i] = 0.;
                    }
                }
            }
        }
    }
    if (before_hiding)
        for (int i = 0; i < TT; i++) before_hiding[i] = 0;
    if (last_pos < 0) return 0;

    // the best last position, against cbf = 0
    double best_cost = block_uncoded + lambda * (double)e.cbf[cbf_ctx][0];
    base_cost += lambda * (double)e.cbf[cbf_ctx][1];
    int best_last_p1 = 0;
    bool found_last = false;
#pragma unroll 1
    for (int g = last_group_pos; g >= 0 && !found_last; g--) {
        int cx, cy;
        scan_position<LG>(scan, g, &cx, &cy);
        base_cost -= w.group_sig[g];
        if (!((group_flags >> (cy * NG + cx)) & 1)) continue;
#pragma unroll 1
        for (int n = 15; n >= 0; n--) {
            const int i = g * 16 + n;
            if (i > last_pos) continue;
            int x, y;
            scan_position<2>(scan, n, &x, &y);
            const int px = cx * 4 + x, py = cy * 4 + y, level = levels[(py << L) + px];
            if (level) {
                const double cost_last = scan == kScanVer ? rate_last(py, px, lambda, e) : rate_last(px, py, lambda, e);
                const double total = base_cost + cost_last - w.cost_sig[i];
                if (total < best_cost) { best_last_p1 = i + 1; best_cost = total; }
                if (level > 1) { found_last = true; break; }
                base_cost -= w.cost[i];
                base_cost += w.cost0[i];
            } else
                base_cost -= w.cost_sig[i];
        }
    }
    int abs_sum = 0;
#pragma unroll 1
    for (int i = 0; i <= last_pos; i++) {
        const int pos = block_position<L>(scan, i);
        if (i < best_last_p1) {
            const int level = levels[pos];
            abs_sum += level;
            levels[pos] = coeffs[pos] < 0 ? -level : level;
        } else
            levels[pos] = 0;
    }
    if (before_hiding)
        for (int i = 0; i < TT; i++) before_hiding[i] = levels[i];
    if (!sdh || abs_sum < 2) return abs_sum;                                 // (a group that hides has two levels: the guard never decides)

    // RDOQ's sign-data hiding
    bool last_group = true;                                                  // HM's lastCG: -1 / 1 until the first group with a level is done
#pragma unroll 1
    for (int g = NGG - 1; g >= 0; g--) {
        int first = 16, last = -1, sum = 0;
#pragma unroll 1
        for (int n = 0; n < 16; n++)
            if (levels[block_position<L>(scan, g * 16 + n)]) { last = n; if (first == 16) first = n; }
        if (last < 0) continue;
#pragma unroll 1
        for (int n = first; n <= last; n++) sum += levels[block_position<L>(scan, g * 16 + n)];
        if (last - first >= trquant::kSbhThreshold) {
            const int signbit = levels[block_position<L>(scan, g * 16 + first)] > 0 ? 0 : 1;
            if (signbit != (sum & 1)) {
                long long min_cost = 0x7fffffffffffffffll;
                int min_n = -1, final_change = 0;
#pragma unroll 1
                for (int n = last_group ? last : 15; n >= 0; n--) {
                    const int i = g * 16 + n, at = block_position<L>(scan, i), level = levels[at], a = level < 0 ? -level : level;
                    long long cur;
                    int change;
                    if (level != 0) {
                        const long long up = k.rd_factor * (long long)(-w.delta_u[i]) + w.rate_up[i];
                        long long down = k.rd_factor * (long long)w.delta_u[i] + w.rate_down[i] - (a == 1 ? w.sig_delta[i] : 0);
                        if (last_group && last == n && a == 1) down -= 4 << 15;
                        if (up < down) { cur = up; change = 1; }
                        else {
                            change = -1;
                            cur = n == first && a == 1 ? 0x7fffffffffffffffll : down;
                        }
                    } else {
                        const int du = w.delta_u[i] < 0 ? -w.delta_u[i] : w.delta_u[i];
                        cur = k.rd_factor * (long long)(-du) + (1 << 15) + w.rate_up[i] + w.sig_delta[i];
                        change = 1;
                        if (n < first && (coeffs[at] >= 0 ? 0 : 1) != signbit) cur = 0x7fffffffffffffffll;
                    }
                    if (cur < min_cost) { min_cost = cur; final_change = change; min_n = n; }
                }
                if (min_n >= 0) {                                            // (always: the group's last level is never forbidden)
                    const int at = block_position<L>(scan, g * 16 + min_n);
                    if (levels[at] == 32767 || levels[at] == -32768) final_change = -1;
                    levels[at] += coeffs[at] >= 0 ? final_change : -final_change;
                }
            }
        }
        last_group = false;
    }
    return abs_sum;
}

}  // namespace rdoq
}  // namespace pnn
