// HM's transform skip for 4 x 4 luma units on the GPU (include/pnn_hip.h, "transform skip"), beside the untouched
// trquant_kernel (pnn_trquant.hip), which codes the transformed form.  Bit-exact against the host twin (pnn_tskip.cpp), with which it
// shares pnn_tskip.h and, through it, every line of the quantiser, the hiding, RDOQ and the rate.
//
// tskip4_kernel: the skipped form of N units x up to 8 QPs in one launch, with trquant_kernel<4, ..>'s arguments, outputs and layouts.
// A workgroup of 4 waves owns 64 units = 1024 samples, sample e = 256 j + tid (j = 0 .. 3) on lane tid: unit e / 16, row (e / 4) % 4,
// column e % 4.  There is no matrix stage: the coefficient is the lane's own residual << 5 (kept in LDS for the lanes that read it by
// scan position), the decoded residual the lane's own dequantised level, (c + 16) >> 5.  Per QP the structure is trquant_kernel's at
// T = 4: quantise per sample; with SDH one lane per scan position, 16 consecutive lanes per unit, ballots cut to the unit's 16 bits (a
// 4 x 4 unit is its own last group); with RDOQ the bit estimates to LDS, one lane per scan position for the uncoded costs, ONE LANE PER
// UNIT for the walk of rdoq::unit; then, with a rate output, one lane per unit walks cabac::unit_rate while the others reconstruct.  The
// sums of a unit go by shuffles over its 16 lanes.  Units past N carry a zero residual and are never stored.
//
// tskip_decide_kernel: one lane per (QP, unit) reads both forms' SSE, counts and level bits, forms both J in doubles (contraction off,
// pnn_tskip.h) and writes the merged outputs -- the rate with the flag bin of the kept form, nothing for a unit without a level -- and
// ts_flag; forced (mode 1) it takes the skipped form of every unit.
#include "pnn_cabac_tables.h"
#include "pnn_kernels.h"
#include "pnn_tskip.h"

namespace pnn {
namespace {

constexpr int kTsThreads = 256;
constexpr int kTsElems = 1024;                    // residual samples a workgroup holds: 64 units
constexpr int kTsPerLane = kTsElems / kTsThreads;

template <bool SDH, bool RDOQ>
__global__ __launch_bounds__(kTsThreads) void tskip4_kernel(const TrQuantParams p)
{
    using namespace trquant;
    constexpr int L = 2, T = 4, TT = 16, G = kTsElems / TT;
    __shared__ int coef[kTsElems], lev[kTsElems];
    __shared__ unsigned sums[kMaxQps][3][G];      // [qp][sse, nonzero, sum of magnitudes][unit]
    __shared__ int ebits[128];
    __shared__ uint8_t lps[64], states[G * cabac::kNumCtx];
    __shared__ unsigned long long bits[kMaxQps * G];

    // the hiding's remainders exist in the SDH instantiations only, RDOQ's arrays in the RDOQ ones
    [[maybe_unused]] int* du = nullptr;
    if constexpr (SDH && !RDOQ) {
        __shared__ int du_s[kTsElems];
        du = du_s;
    }
    [[maybe_unused]] rdoq::Work rw{};
    [[maybe_unused]] rdoq::EstBits* est = nullptr;
    [[maybe_unused]] int* unit_abs = nullptr;
    if constexpr (RDOQ) {
        __shared__ double cost_s[kTsElems], cost0_s[kTsElems], cost_sig_s[kTsElems], group_sig_s[kTsElems / 16];
        __shared__ rdoq::EstBits est_s;
        __shared__ int unit_abs_s[G];
        rw.cost = cost_s; rw.cost0 = cost0_s; rw.cost_sig = cost_sig_s; rw.group_sig = group_sig_s; est = &est_s; unit_abs = unit_abs_s;
        if constexpr (SDH) {
            __shared__ int rate_up_s[kTsElems], rate_down_s[kTsElems], sig_delta_s[kTsElems];
            __shared__ short delta_u_s[kTsElems];
            rw.rate_up = rate_up_s; rw.rate_down = rate_down_s; rw.sig_delta = sig_delta_s; rw.delta_u = delta_u_s;
        }
    }

    const int tid = threadIdx.x;
    if (tid < 128) ebits[tid] = cabac::entropy_bits_table()[tid];
    if (tid < 64) lps[tid] = cabac::trans_idx_lps_table()[tid];
    for (int i = tid; i < kMaxQps * G; i += kTsThreads) bits[i] = 0;
    for (int i = tid; i < kMaxQps * 3 * G; i += kTsThreads) (&sums[0][0][0])[i] = 0;

    const int col = tid % T;                      // e % T of all four samples
    int row[kTsPerLane], pred[kTsPerLane], tgt[kTsPerLane];
    long blk[kTsPerLane];                         // the sample's unit; -1 past N
    const long blk0 = (long)blockIdx.x * G;
#pragma unroll
    for (int j = 0; j < kTsPerLane; j++) {
        const int e = j * kTsThreads + tid;
        row[j] = (e / T) % T;
        const long b = blk0 + e / TT;
        blk[j] = b < p.N ? b : -1;
        pred[j] = 0; tgt[j] = 0;
        if (blk[j] >= 0) {
            const size_t at = ((size_t)blk[j] * T + row[j]) * T + col;
            pred[j] = p.pred[at]; tgt[j] = p.targets[at];
        }
        coef[e] = tskip::forward(tgt[j] - pred[j]);
    }

    // lane tid of round j is scan position (256 j + tid) % 16 of unit (256 j + tid) / 16; where that lies in LDS
    [[maybe_unused]] int hide_at[kTsPerLane];
    if constexpr (SDH || RDOQ) {
#pragma unroll
        for (int j = 0; j < kTsPerLane; j++) {
            const int s = j * kTsThreads + tid, u = s / TT, i = s % TT;
            const long b = blk0 + u;
            const int scan = p.modes && b < p.N ? cabac::scan_of_mode(L, p.modes[b]) : cabac::kScanDiag;
            int x, y;
            cabac::scan_position<2>(scan, i, &x, &y);
            hide_at[j] = u * TT + y * T + x;
        }
    }
    __syncthreads();                              // coef, the tables and the zeroed sums are written

#pragma unroll 1
    for (int qi = 0; qi < p.nb_qps; qi++) {
        const QpConsts qc = p.qp[qi];
        unsigned nonzero[kTsPerLane], sum_abs[kTsPerLane], sse[kTsPerLane];
        int deq[kTsPerLane];
        if constexpr (RDOQ) {
            for (int i = tid; i < rdoq::kEstBitsWords; i += kTsThreads)
                (&est->ctx[0][0])[i] = rdoq::est_bits_word<L>(i, p.init_states[qi], p.cbf_states[qi], ebits);
#pragma unroll
            for (int j = 0; j < kTsPerLane; j++)
                rw.cost0[j * kTsThreads + tid] = rdoq::uncoded_cost(rdoq::level_double(coef[hide_at[j]], qc.scale, qc.qbits), p.rd[qi].err_scale);
            __syncthreads();
            if (tid < G) {                        // lane g quantises unit g (a unit past N has a zero residual: nothing to decide)
                const long b = blk0 + tid;
                const int scan = p.modes && b < p.N ? cabac::scan_of_mode(L, p.modes[b]) : cabac::kScanDiag;
                rdoq::Work w = rw;
                const int s0 = tid * TT;
                w.cost0 += s0; w.cost += s0; w.cost_sig += s0; w.group_sig += s0 / 16;
                if constexpr (SDH) { w.rate_up += s0; w.rate_down += s0; w.sig_delta += s0; w.delta_u += s0; }
                unit_abs[tid] = rdoq::unit<L>(coef + s0, scan, qc.scale, qc.qbits, p.rd[qi], *est, p.cbf_ctx, SDH, lev + s0, w, nullptr);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kTsPerLane; j++) {
                const int level = lev[j * kTsThreads + tid];
                nonzero[j] = level != 0;
                sum_abs[j] = 0;                                    // HM's uiAbsSum is the walk's: added per unit below
                deq[j] = dequant_level(level, qc);
            }
            if (tid < G) atomicAdd(&sums[qi][2][tid], (unsigned)unit_abs[tid]);
        } else if constexpr (SDH) {
#pragma unroll
            for (int j = 0; j < kTsPerLane; j++) {
                int mag, delta_u;
                lev[j * kTsThreads + tid] = quant_level(coef[j * kTsThreads + tid], qc, &mag, &delta_u);
                du[j * kTsThreads + tid] = delta_u;
                sum_abs[j] = (unsigned)mag;                        // HM's uiAbsSum: before the hiding
            }
            __syncthreads();
            // one lane per scan position: 16 consecutive lanes are one unit, n = tid % 16
            const int n = tid & 15, shift = tid & 48;
#pragma unroll
            for (int j = 0; j < kTsPerLane; j++) {
                const int lv = lev[hide_at[j]], cf = coef[hide_at[j]], dl = du[hide_at[j]];
                const unsigned nz = (unsigned)(__ballot(lv != 0) >> shift) & 0xffffu, neg = (unsigned)(__ballot(lv < 0) >> shift) & 0xffffu;
                const unsigned odd = (unsigned)(__ballot(lv & 1) >> shift) & 0xffffu;
                const int first = nz ? __builtin_ctz(nz) : 16, last = nz ? 31 - __builtin_clz(nz) : -1;
                const int signbit = (int)(neg >> (first & 15)) & 1;
                int key = kSdhForbidden, change = 0;
                if (last - first >= kSbhThreshold && signbit != (__builtin_popcount(odd) & 1) && n <= last) {
                    const int cost = sdh_cost(lv, cf, dl, n, first, signbit, &change);
                    if (cost != kSdhForbidden) key = ((cost + 256) << 4) | (15 - n);
                }
                int best = key;
#pragma unroll
                for (int d = 8; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d));
                if (key == best && key != kSdhForbidden) lev[hide_at[j]] = sdh_changed_level(lv, cf, change);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kTsPerLane; j++) {
                const int level = lev[j * kTsThreads + tid];
                nonzero[j] = level != 0;
                deq[j] = dequant_level(level, qc);
            }
        } else {
#pragma unroll
            for (int j = 0; j < kTsPerLane; j++) {
                int mag;
                const int level = quant_level(coef[j * kTsThreads + tid], qc, &mag);
                nonzero[j] = level != 0;
                sum_abs[j] = (unsigned)mag;
                deq[j] = dequant_level(level, qc);
                lev[j * kTsThreads + tid] = level;
            }
            __syncthreads();
        }
        if (p.rate && tid < G && blk0 + tid < p.N) {               // lane g codes unit g (units past N have no slot to add to)
            const int scan = p.modes ? cabac::scan_of_mode(L, p.modes[blk0 + tid]) : cabac::kScanDiag;
            bits[qi * G + tid] += cabac::unit_rate<L, SDH>(lev + tid * TT, scan, p.init_states[qi], states + tid * cabac::kNumCtx,
                                                           cabac::Tables{ebits, lps});
        }
#pragma unroll
        for (int j = 0; j < kTsPerLane; j++) {
            const int rec = min(max(pred[j] + tskip::inverse(deq[j]), 0), 255), d = rec - tgt[j];
            sse[j] = (unsigned)(d * d);
            if (p.recon && blk[j] >= 0) p.recon[(((size_t)qi * p.N + blk[j]) * T + row[j]) * T + col] = (uint8_t)rec;
#pragma unroll
            for (int k = TT / 2; k > 0; k >>= 1) {
                sse[j] += __shfl_xor(sse[j], k);
                nonzero[j] += __shfl_xor(nonzero[j], k);
                sum_abs[j] += __shfl_xor(sum_abs[j], k);
            }
            if (tid % TT == 0) {
                const int g = (j * kTsThreads + tid) / TT;
                atomicAdd(&sums[qi][0][g], sse[j]);
                atomicAdd(&sums[qi][1][g], nonzero[j]);
                atomicAdd(&sums[qi][2][g], sum_abs[j]);
            }
        }
        __syncthreads();                          // the walks have read this QP's levels (and estimates): the next QP may write them
    }
    for (int i = tid; i < p.nb_qps * G; i += kTsThreads) {
        const int qi = i / G, g = i % G;
        const long b = blk0 + g;
        if (b < p.N) {
            const size_t at = (size_t)qi * p.N + b;
            if (p.sse) p.sse[at] = sums[qi][0][g];
            if (p.nonzero) p.nonzero[at] = sums[qi][1][g];
            if (p.sum_abs) p.sum_abs[at] = sums[qi][2][g];
            if (p.rate) p.rate[at] = bits[qi * G + g];
        }
    }
}

__global__ __launch_bounds__(kTsThreads) void tskip_decide_kernel(const TskipDecideParams p)
{
    const long i = (long)blockIdx.x * kTsThreads + threadIdx.x;
    if (i >= (long)p.nb_qps * p.N) return;
    const int qi = (int)(i / p.N);
    const tskip::Form s{p.skipped.sse[i], p.skipped.nonzero[i], p.skipped.rate[i]};
    tskip::Form t{0, 0, 0};
    bool skipped = true;
    if (p.decide) {
        t = tskip::Form{p.transformed.sse[i], p.transformed.nonzero[i], p.transformed.rate[i]};
        skipped = tskip::skipped_wins(p.bits[qi], p.mode_bits ? p.mode_bits[i] : 0u, p.charge_cbf, p.lambda[qi], t, s);
    }
    const tskip::Form& f = skipped ? s : t;
    const TskipForm& from = skipped ? p.skipped : p.transformed;
    if (p.sse) p.sse[i] = f.sse;
    if (p.nonzero) p.nonzero[i] = f.nb_nonzero;
    if (p.sum_abs) p.sum_abs[i] = from.sum_abs[i];
    if (p.rate) p.rate[i] = tskip::unit_frac_bits(p.bits[qi], skipped, f.nb_nonzero, f.level_bits);
    if (p.ts_flag) p.ts_flag[i] = skipped;
    if (p.recon) {
        // the workspace's sections are 256-byte aligned, the caller's array need not be: words in, bytes out
        const uint4 v = reinterpret_cast<const uint4*>(from.recon)[i];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) p.recon[(size_t)i * 16 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

__global__ __launch_bounds__(kTsThreads) void tskip_slot_bits_kernel(const TskipSlotBitsParams p)
{
    const long i = (long)blockIdx.x * kTsThreads + threadIdx.x;
    if (i >= (long)p.N * p.S) return;
    const long b = i / p.S;
    const int m = p.slot_modes[i];
    const msig::Mpm mpm = msig::derive_mpm(msig::neighbour_dir(p.left ? p.left[b] : msig::kNoNeighbour),
                                           msig::neighbour_dir(p.above ? p.above[b] : msig::kNoNeighbour));
    p.mode_bits[i] = m == msig::kUnusedSlot ? 0u : msig::mode_frac_bits(m, mpm, p.bits, p.pnn_flag);
}

__global__ __launch_bounds__(kTsThreads) void tskip_best_flag_kernel(const TskipBestFlagParams p)
{
    const long b = (long)blockIdx.x * kTsThreads + threadIdx.x;
    if (b >= p.N) return;
    const int slot = p.best_slot[b];
    p.best_flag[b] = slot < p.S ? p.ts_flag[b * p.S + slot] : (uint8_t)0;
}

}  // namespace

hipError_t launch_tskip_slot_bits(const TskipSlotBitsParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.slot_modes || !p.mode_bits || p.S < 1) return hipErrorInvalidValue;
    const long lanes = (long)p.N * p.S;
    hipLaunchKernelGGL(tskip_slot_bits_kernel, dim3((unsigned)((lanes + kTsThreads - 1) / kTsThreads)), dim3(kTsThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tskip_best_flag(const TskipBestFlagParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.ts_flag || !p.best_slot || !p.best_flag || p.S < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tskip_best_flag_kernel, dim3((unsigned)((p.N + kTsThreads - 1) / kTsThreads)), dim3(kTsThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tskip4(const TrQuantParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.pred || !p.targets || p.w != tskip::kWidth || p.nb_qps < 1 || p.nb_qps > trquant::kMaxQps) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.N + kTsElems / 16 - 1) / (kTsElems / 16))), block(kTsThreads);
    if (p.rdoq) {
        if (p.sdh) hipLaunchKernelGGL((tskip4_kernel<true, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((tskip4_kernel<false, true>), grid, block, 0, s, p);
    } else if (p.sdh) hipLaunchKernelGGL((tskip4_kernel<true, false>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((tskip4_kernel<false, false>), grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tskip_decide(const TskipDecideParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    // a form's sum of magnitudes and reconstruction are read for the outputs that ask for them only; a lane reads both forms' element
    // before it writes its own, so an output may be the transformed form's array
    const auto complete = [&](const TskipForm& f) {
        return f.sse && f.nonzero && f.rate && (f.sum_abs || !p.sum_abs) && (f.recon || !p.recon);
    };
    if (p.nb_qps < 1 || p.nb_qps > trquant::kMaxQps || !complete(p.skipped) || (p.decide && !complete(p.transformed))) return hipErrorInvalidValue;
    const long lanes = (long)p.nb_qps * p.N;
    hipLaunchKernelGGL(tskip_decide_kernel, dim3((unsigned)((lanes + kTsThreads - 1) / kTsThreads)), dim3(kTsThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace pnn
