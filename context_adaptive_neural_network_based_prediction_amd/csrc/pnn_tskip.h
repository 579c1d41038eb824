// The one home of HM's transform skip for 4 x 4 luma units (include/pnn_hip.h, "transform skip"): the two shifts of
// xTransformSkip / xITransformSkip, the bits of transform_skip_flag from the state an I slice of the QP starts with, and the rule by
// which TEncSearch::xRecurIntraCodingLumaQT keeps the transformed or the skipped form of a unit.  Shared by the host twin
// (pnn_tskip.cpp, plain C++) and the kernels (pnn_tskip.hip): both compile THESE lines, so there is no HIP in it beyond the function
// qualifiers.  Quantisation, hiding, RDOQ, the rate of the levels and the cbf bin are the existing headers', as they stand.
#pragma once

#include "pnn_cabac_tables.h"
#include "pnn_mode_signal.h"

namespace pnn {
namespace tskip {

constexpr int kWidth = 4;                          // Log2MaxTransformSkipBlockSize 2: the only unit size with the flag
// getTransformShift: maxLog2TrDynamicRange 15 - bit depth 8 - log2 of the unit size 2
constexpr int kShift = 15 - 8 - 2;
// I-slice row of HM's INIT_TRANSFORMSKIP_FLAG, luma (m_cTransformSkipSCModel)
constexpr int kInitFlag = 139;

// xTransformSkip: residual << shift (a multiplication: the residual may be negative); |residual| <= 255 gives |coefficient| <= 8160
PNN_TQ_HD inline int forward(int residual) { return residual * (1 << kShift); }
// xITransformSkip: (coefficient + half) >> shift, arithmetic
PNN_TQ_HD inline int inverse(int coeff) { return (coeff + (1 << (kShift - 1))) >> kShift; }

// entropyBits[state ^ bin] of the flag's context from the state an I slice of the QP starts with, in 2^-15 bit (made on the host, for
// twin and kernels alike: it travels in the kernels' argument block), beside the cbf bin's of the unit's context
struct QpBits { uint32_t flag[2], cbf[2]; };
inline QpBits qp_bits(int qp)
{
    const int* entropy_bits = cabac::entropy_bits_table();
    const msig::FlagBits f = msig::flag_bits(qp);
    const int state = cabac::init_state(qp, kInitFlag), ctx = msig::cbf_context(kWidth);
    return QpBits{{(uint32_t)entropy_bits[state], (uint32_t)entropy_bits[state ^ 1]}, {f.cbf[ctx][0], f.cbf[ctx][1]}};
}

// What codeCoeffNxN adds for one 4 x 4 unit with the PPS flag on: the flag bin in front of the levels, nothing without a level
PNN_TQ_HD inline uint64_t unit_frac_bits(const QpBits& b, int skipped, uint32_t nb_nonzero, uint64_t level_bits)
{
    return nb_nonzero ? (uint64_t)b.flag[skipped ? 1 : 0] + level_bits : 0;
}

// One form's bits on HM's counter when the tree costs it: the mode's bits, the cbf_luma bin (charge_cbf) and what codeCoeffNxN adds
PNN_TQ_HD inline uint64_t form_frac_bits(const QpBits& b, uint32_t mode_bits, int charge_cbf, int skipped, uint32_t nb_nonzero, uint64_t level_bits)
{
    return (uint64_t)mode_bits + (charge_cbf ? b.cbf[nb_nonzero ? 1 : 0] : 0u) + unit_frac_bits(b, skipped, nb_nonzero, level_bits);
}

// TComRdCost::calcRdCost on the counter's whole bits: one IEEE multiply and one IEEE add, each rounded once
PNN_TQ_HD inline double rd_cost(uint32_t sse, uint64_t frac_bits, double lambda)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double bits = lambda * (double)(frac_bits >> 15);
    return (double)sse + bits;
}

// The checkTransformSkip loop: the transformed form first, the skipped one second and forbidden without a level; strict <
struct Form { uint32_t sse, nb_nonzero; uint64_t level_bits; };
PNN_TQ_HD inline bool skipped_wins(const QpBits& b, uint32_t mode_bits, int charge_cbf, double lambda, const Form& transformed, const Form& skipped)
{
    if (!skipped.nb_nonzero) return false;
    const double j0 = rd_cost(transformed.sse, form_frac_bits(b, mode_bits, charge_cbf, 0, transformed.nb_nonzero, transformed.level_bits), lambda);
    const double j1 = rd_cost(skipped.sse, form_frac_bits(b, mode_bits, charge_cbf, 1, skipped.nb_nonzero, skipped.level_bits), lambda);
    return j1 < j0;
}

}  // namespace tskip
}  // namespace pnn
