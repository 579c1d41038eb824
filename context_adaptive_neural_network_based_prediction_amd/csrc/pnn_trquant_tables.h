// The one home of the constants of the open-loop transform coding (include/pnn_hip.h, "transform coding"): the HEVC
// core transform matrix, the 4 x 4 DST-VII, the quantisation tables and what a QP turns into.  Shared by the host twin
// (pnn_trquant.cpp, plain C++), the kernel (pnn_trquant.hip) and the device entry (pnn_eval.cpp), so there is no HIP in it beyond the
// function qualifiers.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PNN_TQ_HD __host__ __device__
#else
#define PNN_TQ_HD
#endif

namespace pnn {
namespace trquant {

constexpr int kMaxQps = 8;     // QPs per call
constexpr int kMaxQp = 51;

// log2 of the transform-unit size T of a block of width w: T = w up to 32; a 64 x 64 block is four 32 x 32 units (-1: no such width)
PNN_TQ_HD inline int log2_tu(int w) { return w == 4 ? 2 : w == 8 ? 3 : w == 16 ? 4 : w == 32 || w == 64 ? 5 : -1; }

// H.265 8.6.4.2: transMatrix is 32 x 32 with 31 distinct magnitudes, entry [k][x] = the rounded 64 sqrt(2) cos(pi a / 64) at the angle
// index a = k (2x + 1), 64 in row 0.  kCos[a], a = 0 .. 31, is the matrix's first column; cos folds every other a onto it (a = 32 mod
// 64 never occurs for k < 32).  The T-point matrix is rows 0, 32 / T, 2 * 32 / T, ... and the first T columns of it.
PNN_TQ_HD inline int dct_coeff(int log2_t, int k, int x)
{
    static constexpr int8_t kCos[32] = {64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67,
                                        64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4};
    int a = ((k << (5 - log2_t)) * (2 * x + 1)) & 127;
    if (a > 64) a = 128 - a;
    return a > 32 ? -kCos[64 - a] : kCos[a];
}

// H.265 8.6.4.2, the 4 x 4 DST-VII of intra luma: rows {29 55 74 84}, {74 74 0 -74}, {84 -29 -74 55}, {55 -84 74 -29}
PNN_TQ_HD inline int dst4_coeff(int k, int x)
{
    static constexpr int8_t kDst[16] = {29, 55, 74, 84, 74, 74, 0, -74, 84, -29, -74, 55, 55, -84, 74, -29};
    return kDst[k * 4 + x];
}

// M[k][x] of the transform this project applies to a T x T luma intra unit: the DST at T = 4, the core transform otherwise
PNN_TQ_HD inline int matrix_coeff(int log2_t, int k, int x) { return log2_t == 2 ? dst4_coeff(k, x) : dct_coeff(log2_t, k, x); }

// forward shifts (8-bit video, 15-bit coefficients): first stage log2 T - 1, second log2 T + 6; inverse: 7, then 12
PNN_TQ_HD inline int fwd_shift1(int log2_t) { return log2_t - 1; }
PNN_TQ_HD inline int fwd_shift2(int log2_t) { return log2_t + 6; }
constexpr int kInvShift1 = 7, kInvShift2 = 12;

// What a QP turns into at unit size 2^log2_t (HM's xQuant without RDOQ in an I slice, xDeQuant without scaling lists):
//   mag = (|C| scale + add) >> qbits (64 bits), level = clip16(sign(C) mag);
//   C' = clip16(rs > 0 ? (level inv + (1 << (rs - 1))) >> rs : (level inv) * (1 << -rs))
struct QpConsts { int scale, qbits, add, inv, rs; };
inline QpConsts qp_consts(int log2_t, int qp)
{
    static constexpr int kQuantScale[6] = {26214, 23302, 20560, 18396, 16384, 14564};
    static constexpr int kInvQuantScale[6] = {40, 45, 51, 57, 64, 72};
    const int per = qp / 6, rem = qp % 6, ts = 7 - log2_t;
    QpConsts c;
    c.scale = kQuantScale[rem];
    c.qbits = 14 + per + ts;
    c.add = 171 << (c.qbits - 9);        // the I-slice rounding offset, 171 / 512
    c.inv = kInvQuantScale[rem];
    c.rs = 6 - (ts + per);
    return c;
}

// 1 .. kMaxQps QPs, each in [0, kMaxQp]
inline bool qps_ok(const int* qps, int nb_qps)
{
    if (!qps || nb_qps < 1 || nb_qps > kMaxQps) return false;
    for (int i = 0; i < nb_qps; i++)
        if (qps[i] < 0 || qps[i] > kMaxQp) return false;
    return true;
}

PNN_TQ_HD inline int clip16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// one coefficient through quantisation: the magnitude (HM's addend of uiAbsSum, before the clip) and the level
PNN_TQ_HD inline int quant_level(int coeff, const QpConsts& q, int* mag)
{
    const int a = coeff < 0 ? -coeff : coeff;
    *mag = (int)(((long long)a * q.scale + q.add) >> q.qbits);
    return clip16(coeff < 0 ? -*mag : *mag);
}

// the same with xQuant's rounding remainder, which sign-data hiding costs its changes by:
//   deltaU = (|C| scale - (mag << qbits)) >> (qbits - 8), in 64 bits; qbits - 8 >= 8 for every unit size and QP.
// mag 2^qbits <= |C| scale + add < (mag + 1) 2^qbits and add = 171 * 2^(qbits - 9), so deltaU lies in [-86, 170]
constexpr int kDeltaUMin = -86, kDeltaUMax = 170;
PNN_TQ_HD inline int quant_level(int coeff, const QpConsts& q, int* mag, int* delta_u)
{
    const int a = coeff < 0 ? -coeff : coeff;
    const long long tmp = (long long)a * q.scale;
    *mag = (int)((tmp + q.add) >> q.qbits);
    *delta_u = (int)((tmp - ((long long)*mag << q.qbits)) >> (q.qbits - 8));
    return clip16(coeff < 0 ? -*mag : *mag);
}

// Sign-data hiding (TComTrQuant::signBitHidingHDQ): a 4 x 4 group whose first and last nonzero scan positions are at least
// kSbhThreshold apart hides the sign of the first one in the parity of its levels.  What changing position n of such a group costs and
// which way it goes (the table of include/pnn_hip.h): first = the group's lowest nonzero position, signbit = the sign to hide.
constexpr int kSbhThreshold = 4;
constexpr int kSdhForbidden = 0x7fffffff;
PNN_TQ_HD inline int sdh_cost(int level, int coeff, int delta_u, int n, int first, int signbit, int* change)
{
    *change = 1;
    if (level != 0) {
        if (delta_u > 0) return -delta_u;
        if (n == first && (level == 1 || level == -1)) return kSdhForbidden;
        *change = -1;
        return delta_u;
    }
    if (n < first && (coeff >= 0 ? 0 : 1) != signbit) return kSdhForbidden;
    return -delta_u;
}
// the winner's new level: +-32767 / -32768 can only come down
PNN_TQ_HD inline int sdh_changed_level(int level, int coeff, int change)
{
    if (level == 32767 || level == -32768) change = -1;
    return coeff >= 0 ? level + change : level - change;
}

PNN_TQ_HD inline int dequant_level(int level, const QpConsts& q)
{
    const int v = level * q.inv;          // |v| <= 32768 * 72
    return clip16(q.rs > 0 ? (v + (1 << (q.rs - 1))) >> q.rs : v * (1 << -q.rs));   // |v| << 7 stays below 2^31
}

}  // namespace trquant
}  // namespace pnn
