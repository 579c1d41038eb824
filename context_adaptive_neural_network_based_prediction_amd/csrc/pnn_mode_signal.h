// The one home of the side information HM's intra search charges a luma candidate with (include/pnn_hip.h, "mode signalling";
// DESIGN.md section 5n): the three most probable modes of TComDataCU::getIntraDirPredictor as the reference's hm_16_15_switch derives
// them (its branches for a neighbour coded with mode 35 included; without such a neighbour they are HM-16.15's own), the bits
// TEncSbac::codeIntraDirLumaAng adds to a TEncBinCABACCounter for one prediction unit, the cbf_luma bin of codeQtCbf, the first-pass
// cost SATD + modeBits * sqrtLambda with HM's sorted list over it, and the slots of the second pass: the list, the missing MPMs, 35.
// Shared by the host twin (pnn_rd_pass.cpp, plain C++) and the kernels (pnn_hevc_intra.hip): both compile THESE lines, so there is no
// HIP in it beyond the function qualifiers, no array indexed by a runtime value and no loop without a compile-time bound.
//
// Cold contexts, as the rate of the levels (section 5j): the PNN flag's context and prev_intra_luma_pred_flag's start every unit from
// the state an I slice of the QP begins with, and so do the two cbf contexts.  LEFT OUT: part size, split and subdivision flags (equal
// for all candidates of a block), the interleaving of the four units' flags in an N x N coding unit (the counter adds the same bins in
// any order), chroma, running contexts.
// The substitution codec (hm_16_15_substitution) keeps HM's 35 modes and signalling -- derive_mpm without a
// neighbour 35, mode_frac_bits with pnn_flag 0 -- and predicts mode 18 with the PNN: list_and_slots_substitution below.
#pragma once

#include "pnn_cabac_tables.h"

namespace pnn {
namespace msig {

constexpr int kPnnMode = 35, kNoNeighbour = 255, kUnusedSlot = 255;
constexpr int kExtraSlots = 3;                    // two most probable modes and 35 behind the K list entries
// I-slice rows of HM's ContextTables.h: INIT_INTRA_PNNS_MODE (the switch codec's flag), INIT_INTRA_PRED_MODE, INIT_QT_CBF for luma
// (transform depth > 0, depth 0: getCtxQtCbf gives context 1 at depth 0)
constexpr int kInitPnnFlag = 154, kInitPrevIntraPred = 184, kInitCbf[2] = {111, 141};

// a neighbour's mode as the caller gives it: 0 .. 34, 35 with the PNN flag, 255 = none or not intra
PNN_TQ_HD inline bool neighbour_ok(int mode, int pnn_flag) { return mode == kNoNeighbour || mode < kPnnMode || (pnn_flag && mode == kPnnMode); }
// ... and as getIntraDirPredictor sees it: a missing or non-intra neighbour counts as DC
PNN_TQ_HD inline int neighbour_dir(int mode) { return mode == kNoNeighbour ? 1 : mode; }
// the cbf context of a unit of a block of width w: 1 at transform depth 0 (w = 8, 16, 32), 0 at depth 1 (w = 4; each quadrant at w = 64)
PNN_TQ_HD inline int cbf_context(int w) { return w == 8 || w == 16 || w == 32 ? 1 : 0; }

// uiIntraDirPred[0 .. 2] and *piMode (1 when left and above are equal, else 2: how many of the three the search appends)
struct Mpm { int m0, m1, m2, num_append; };
PNN_TQ_HD inline Mpm derive_mpm(int left, int above)
{
    Mpm r;
    if (left == above) {
        r.num_append = 1;
        if (left > 1 && left < kPnnMode) {        // the same angular mode: it and its two neighbours, wrapping between 2 and 34
            r.m0 = left; r.m1 = ((left + 29) % 32) + 2; r.m2 = ((left - 1) % 32) + 2;
        } else {                                  // planar, DC -- or 35 twice: the PNN never enters the three
            r.m0 = 0; r.m1 = 1; r.m2 = 26;
        }
    } else {
        r.num_append = 2;
        if (left == kPnnMode || above == kPnnMode) {
            const int other = left == kPnnMode ? above : left;
            r.m0 = other;
            if (other > 1) { r.m1 = 0; r.m2 = 1; }
            else if (other == 1) { r.m1 = 0; r.m2 = 26; }
            else { r.m1 = 1; r.m2 = 26; }
        } else {
            r.m0 = left; r.m1 = above;
            r.m2 = left && above ? 0 : left + above < 2 ? 26 : 1;
        }
    }
    return r;
}

// entropyBits[state ^ bin] of the four contexts from the state an I slice of the QP starts with, in 2^-15 bit
// (made on the host, for twin and kernels alike: it travels in the kernels' argument block)
struct FlagBits { uint32_t pnn[2], prev[2], cbf[2][2]; };
inline FlagBits flag_bits(int qp)
{
    const int* entropy_bits = cabac::entropy_bits_table();
    FlagBits f;
    const int pnn = cabac::init_state(qp, kInitPnnFlag), prev = cabac::init_state(qp, kInitPrevIntraPred);
    for (int b = 0; b < 2; b++) {
        f.pnn[b] = (uint32_t)entropy_bits[pnn ^ b];
        f.prev[b] = (uint32_t)entropy_bits[prev ^ b];
        for (int c = 0; c < 2; c++) f.cbf[c][b] = (uint32_t)entropy_bits[cabac::init_state(qp, kInitCbf[c]) ^ b];
    }
    return f;
}

// codeIntraDirLumaAng for one unit of mode `mode` on a counter: the PNN flag (with pnn_flag), then for a regular mode
// prev_intra_luma_pred_flag and mpm_idx (1 bypass bin for index 0, 2 for 1 and 2) or the 5 bypass bins of the remainder.  HM sorts the
// three ascending before it takes the remainder; the remainder's VALUE costs nothing here, its 5 bins do.  Mode 35 without the flag: 0.
PNN_TQ_HD inline uint32_t mode_frac_bits(int mode, const Mpm& mpm, const FlagBits& f, int pnn_flag)
{
    if (mode == kPnnMode) return pnn_flag ? f.pnn[1] : 0u;
    const uint32_t flag = pnn_flag ? f.pnn[0] : 0u;
    if (mode == mpm.m0) return flag + f.prev[1] + (uint32_t)cabac::kBypassBits;
    if (mode == mpm.m1 || mode == mpm.m2) return flag + f.prev[1] + 2u * (uint32_t)cabac::kBypassBits;
    return flag + f.prev[0] + 5u * (uint32_t)cabac::kBypassBits;
}

// the first-pass cost (TEncSearch.cpp: (Double) uiSad + (Double) iModeBits * sqrtLambdaForFirstPass, iModeBits the counter's whole
// bits): one IEEE multiply and one IEEE add, each rounded once
PNN_TQ_HD inline double first_pass_cost(uint32_t satd, uint32_t frac_bits, double sqrt_lambda)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double bits = (double)(frac_bits >> 15) * sqrt_lambda;
    return (double)satd + bits;
}

// The first pass of one block at one QP.  satd(i): the Hadamard cost of mode i (35: the candidate).  xUpdateCandList over modes 0 ..
// 35 in that order on the doubles above (an entry goes in front of the first strictly larger cost; the earlier mode keeps its place
// on a tie), then the slots: the K list entries, mpm[0 .. num_append - 1] where the list lacks them, 35 if absent, 255 behind them.
template <int K, typename Satd>
PNN_TQ_HD inline void list_and_slots(Satd satd, const Mpm& mpm, const FlagBits& f, double sqrt_lambda, int (&list_mode)[K], double (&list_cost)[K],
                                     int (&extra)[kExtraSlots])
{
#pragma unroll
    for (int j = 0; j < K; j++) { list_cost[j] = __builtin_inf(); list_mode[j] = kUnusedSlot; }
#pragma unroll 1
    for (int i = 0; i <= kPnnMode; i++) {
        double ci = first_pass_cost(satd(i), mode_frac_bits(i, mpm, f, 1), sqrt_lambda);
        int mi = i;
        bool in = false;
#pragma unroll
        for (int j = 0; j < K; j++) {
            in = in || ci < list_cost[j];
            const double tc = list_cost[j];
            const int tm = list_mode[j];
            list_cost[j] = in ? ci : tc; list_mode[j] = in ? mi : tm;
            ci = in ? tc : ci; mi = in ? tm : mi;
        }
    }
    int count = 0;
#pragma unroll
    for (int t = 0; t < kExtraSlots; t++) extra[t] = kUnusedSlot;
#pragma unroll
    for (int a = 0; a < kExtraSlots; a++) {
        const int cand = a == 0 ? mpm.m0 : a == 1 ? mpm.m1 : kPnnMode;
        bool missing = a != 1 || mpm.num_append == 2;
#pragma unroll
        for (int j = 0; j < K; j++) missing = missing && list_mode[j] != cand;
        if (missing) {
#pragma unroll
            for (int t = 0; t < kExtraSlots; t++)
                if (count == t) extra[t] = cand;
            count++;
        }
    }
}

// The substitution codec's first pass of one block at one QP (hm_16_15_substitution, TEncSearch.cpp:2325-2430): HM's own loop.  satd(i):
// the Hadamard cost of mode i, 0 .. 34 (18: the candidate's, whose prediction stands in that mode's place).  xUpdateCandList over modes
// 0 .. 34 in that order on SATD + (bits without a flag bin >> 15) sqrt(lambda), then the slots: the K list entries, mpm[0 ..
// num_append - 1] where the list lacks them, 255 behind them.  Nothing is appended for the PNN: 18 is coded if listed or a missing MPM.
constexpr int kSubstitutedMode = 18, kNbRegularModes = 35;
constexpr int kExtraSlotsSubstitution = 2;        // two most probable modes behind the K list entries
template <int K, typename Satd>
PNN_TQ_HD inline void list_and_slots_substitution(Satd satd, const Mpm& mpm, const FlagBits& f, double sqrt_lambda, int (&list_mode)[K],
                                                  double (&list_cost)[K], int (&extra)[kExtraSlotsSubstitution])
{
#pragma unroll
    for (int j = 0; j < K; j++) { list_cost[j] = __builtin_inf(); list_mode[j] = kUnusedSlot; }
#pragma unroll 1
    for (int i = 0; i < kNbRegularModes; i++) {
        double ci = first_pass_cost(satd(i), mode_frac_bits(i, mpm, f, 0), sqrt_lambda);
        int mi = i;
        bool in = false;
#pragma unroll
        for (int j = 0; j < K; j++) {
            in = in || ci < list_cost[j];
            const double tc = list_cost[j];
            const int tm = list_mode[j];
            list_cost[j] = in ? ci : tc; list_mode[j] = in ? mi : tm;
            ci = in ? tc : ci; mi = in ? tm : mi;
        }
    }
    int count = 0;
#pragma unroll
    for (int t = 0; t < kExtraSlotsSubstitution; t++) extra[t] = kUnusedSlot;
#pragma unroll
    for (int a = 0; a < kExtraSlotsSubstitution; a++) {
        const int cand = a == 0 ? mpm.m0 : mpm.m1;
        bool missing = a == 0 || mpm.num_append == 2;
#pragma unroll
        for (int j = 0; j < K; j++) missing = missing && list_mode[j] != cand;
        if (missing) {
#pragma unroll
            for (int t = 0; t < kExtraSlotsSubstitution; t++)
                if (count == t) extra[t] = cand;
            count++;
        }
    }
}

// The bits of one coded candidate as HM's counter holds them for the second pass: the mode's bits, the cbf_luma bin and, with a level,
// the rate of the levels.  side = what this header adds to `rate`.
PNN_TQ_HD inline uint64_t side_frac_bits(uint32_t mode_bits, const FlagBits& f, int cbf_ctx, uint32_t nb_nonzero)
{
    return (uint64_t)mode_bits + f.cbf[cbf_ctx][nb_nonzero ? 1 : 0];
}

}  // namespace msig
}  // namespace pnn
