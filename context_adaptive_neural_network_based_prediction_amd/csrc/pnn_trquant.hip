// Open-loop HEVC transform coding of predicted blocks (include/pnn_hip.h, "transform coding"): for N predictions
// and targets [N][w][w] uint8 and up to 8 QPs, HM's residual path with RDOQ 0 -- forward core transform, quantisation, dequantisation,
// inverse transform, reconstruction -- and per (QP, block) the number of nonzero levels, the sum of their magnitudes and the SSE of the
// reconstruction.  Integer VALU arithmetic only, plain matrix products (HM's butterflies factorise the same integers); bit-exact against
// the host twin (pnn_trquant.cpp), with which it shares every constant (pnn_trquant_tables.h).
//
// Layout.  A workgroup of 4 waves owns kElems = 1024 residual samples at a time: G = 1024 / T^2 whole blocks (64, 16, 4, 1 for T = 4, 8,
// 16, 32) or, at w = 64, the four 32 x 32 quadrants of ONE block one after the other, whose counts add into that block's slot.  Sample e
// = 256 j + tid (j = 0 .. 3) belongs to lane tid: unit e / T^2, row (e / T) % T, column e % T -- the four samples of a lane share their
// column.  Every stage is "one output element per (lane, j), a T-long dot product of an LDS row or column with a matrix row or
// column", int32 in LDS:
//   forward 1   Y[y][k] = sum_x X[y][x] M[k][x]     X: one address per T lanes (broadcast); M: stride T + 1 across lanes
//   forward 2   C[l][k] = sum_y Y[y][k] M[l][y]     Y: consecutive lanes, consecutive words;  M: broadcast
//   inverse 1   Z[y][k] = sum_l M[l][y] C'[l][k]    M: broadcast; C': consecutive
//   inverse 2   R[y][x] = sum_k M[k][x] Z[y][k]     M: consecutive; Z: broadcast
// so the only strided access is M's in the first stage, and the matrix's LDS copy has the odd row stride T + 1 for it; the data arrays
// are dense (units of T^2 words side by side: lanes of one wave never meet in a bank on another word).  The forward transform of a unit
// is computed once and stays in LDS; the chain quantise -> dequantise -> inverse -> reconstruct -> reduce runs per QP, two barriers
// each.  The three sums go by wave shuffles over the lanes of one unit (64, or 16 at T = 4), then one LDS add per unit and wave.  The QP's
// constants come ready in the argument block (qp_consts on the host).  Blocks past N in the last workgroup carry a zero residual and are
// never stored.
//
// RATE: the instantiations with RATE also keep the levels of the current QP in LDS (dense per unit, as every
// other array) and, behind the QP's first barrier, ONE LANE PER UNIT -- lane g of the workgroup for unit g: 64 lanes at T = 4, one at
// T = 32 -- walks its unit's levels with cabac::unit_rate, the very lines the host twin compiles (pnn_cabac_tables.h), its 80 context
// states and the two tables in LDS.  The other lanes go on to the inverse transform and wait at its barrier, so the levels stay until
// the walk is over; the next QP overwrites them only behind that barrier.  The bits of a block's units add in a 64-bit LDS slot.  The
// instantiations without RATE are the kernel as it was: no statement of theirs mentions the rate's arrays.
//
// SDH: the instantiations with SDH put HM's sign-data hiding (signBitHidingHDQ) between quantisation and
// dequantisation.  The levels and the remainders deltaU of the current QP go to LDS, dense per unit; then ONE LANE PER SCAN POSITION,
// 16 consecutive lanes per 4 x 4 group (the workgroup's 1024 positions in four rounds of 256 lanes): a lane looks its block position
// up in its unit's scan once, at the kernel's start, and per QP reads its level, coefficient and remainder from there.  first, last,
// the parity and the sign bit of a group are ballots cut to the group's 16 bits; the unit's last group is the highest group with a
// level -- of the wave's ballot where a unit fits a wave (T <= 8), else one LDS max per unit and a barrier; the winner is a 16-lane min
// (__shfl_xor below 16) over the key (cost + 256) << 4 | (15 - n) -- the costs lie in [-170, 170], the tie goes to the highest n -- and
// the winning lane rewrites its one level in LDS.  Behind a barrier every lane reads back the levels of its own samples, counts the
// nonzero ones and dequantises; from there on the kernel is the one above (the rate walk with the SDH rule of unit_rate).  The
// instantiations without SDH are the kernels as they were: no statement of theirs mentions the hiding's arrays.
//
// RDOQ: the instantiations with RDOQ put HM's xRateDistOptQuant (pnn_rdoq.h, the lines the host twin compiles)
// in the quantiser's place, and with SDH its own sign hiding in signBitHidingHDQ's.  Per QP: the bit estimates of the QP go to LDS one
// word per lane, and ONE LANE PER SCAN POSITION (the mapping of the SDH path, hide_at) computes the uncoded cost of its position -- into
// buf_a / buf_b, which hold nothing between two QPs, read as 2 x 512 doubles (an array of its own at T = 32) --; behind a barrier ONE LANE PER UNIT walks its unit (the
// chain c1 / c2 / Rice / context set / coded groups / base cost is serial by construction) over LDS arrays: two doubles per position,
// with SDH three ints and a short, one double per group.  Behind the next barrier every lane reads back the levels of its samples and
// the kernel is the one above.  The other instantiations are the kernels as they were: no statement of theirs mentions these arrays.
#include "pnn_cabac_tables.h"
#include "pnn_kernels.h"
#include "pnn_trquant_tables.h"

namespace pnn {
namespace {

constexpr int kTqThreads = 256;
constexpr int kElems = 1024;                      // residual samples a workgroup holds: one 32 x 32 unit, or G smaller blocks
constexpr int kPerLane = kElems / kTqThreads;

template <int W, bool RATE, bool SDH, bool RDOQ = false>
__global__ __launch_bounds__(kTqThreads) void trquant_kernel(const TrQuantParams p)
{
    using namespace trquant;
    constexpr int T = W < 32 ? W : 32, L = W == 4 ? 2 : W == 8 ? 3 : W == 16 ? 4 : 5, TT = T * T;
    constexpr int U = W / T, NQ = U * U;          // units per block side; units a workgroup walks one after the other
    constexpr int G = kElems / TT;                // units side by side = blocks per workgroup (one at w = 64)
    constexpr int MS = T + 1;                     // the matrix's row stride in LDS
    constexpr int SEG = TT < 64 ? TT : 64;        // lanes of one wave that share a unit
    __shared__ int mat[T * MS];
    // (no alignas here: an explicit alignment, even the type's own, takes away the 16 bytes the compiler gives these arrays by itself --
    // the ds_read_b128 of the stages below -- and changes the code of every instantiation; the RDOQ path's doubles rely on those 16 bytes)
    __shared__ int buf_a[kElems], buf_b[kElems], coef[kElems];
    __shared__ unsigned sums[kMaxQps][3][G];      // [qp][sse, nonzero, sum of magnitudes][block]

    // the rate's arrays exist in the RATE instantiations only
    int* lev = nullptr; int* ebits = nullptr; uint8_t* lps = nullptr; uint8_t* states = nullptr; unsigned long long* bits = nullptr;
    if constexpr (RATE) {
        __shared__ int lev_s[kElems], ebits_s[128];
        __shared__ uint8_t lps_s[64], states_s[G * cabac::kNumCtx];
        __shared__ unsigned long long bits_s[kMaxQps * G];
        lev = lev_s; ebits = ebits_s; lps = lps_s; states = states_s; bits = bits_s;
    }

    // the hiding's arrays exist in the SDH instantiations only (the levels are the rate's array where there is one)
    int* du = nullptr; int* lastg = nullptr;
    if constexpr (SDH && !RDOQ) {
        __shared__ int du_s[kElems], lastg_s[G];
        du = du_s; lastg = lastg_s;
        if constexpr (!RATE) {
            __shared__ int lev_sdh[kElems];
            lev = lev_sdh;
        }
    }

    // RDOQ's arrays exist in the RDOQ instantiations only (levels and entropy bits are the rate's arrays where there are any)
    [[maybe_unused]] rdoq::Work rw{};
    [[maybe_unused]] rdoq::EstBits* est = nullptr;
    [[maybe_unused]] int* unit_abs = nullptr;
    if constexpr (RDOQ) {
        static_assert(2 * sizeof(int) == sizeof(double), "buf_a and buf_b hold the uncoded costs");
        __shared__ double cost_s[kElems], cost_sig_s[kElems], group_sig_s[kElems / 16];
        __shared__ rdoq::EstBits est_s;
        __shared__ int unit_abs_s[G];
        rw.cost = cost_s; rw.cost_sig = cost_sig_s; rw.group_sig = group_sig_s; est = &est_s; unit_abs = unit_abs_s;
        if constexpr (T == 32) {                  // one unit of 1024 positions: an array of its own (there is room at this size)
            __shared__ double cost0_s[kElems];
            rw.cost0 = cost0_s;
        }
        if constexpr (SDH) {
            __shared__ int rate_up_s[kElems], rate_down_s[kElems], sig_delta_s[kElems];
            __shared__ short delta_u_s[kElems];
            rw.rate_up = rate_up_s; rw.rate_down = rate_down_s; rw.sig_delta = sig_delta_s; rw.delta_u = delta_u_s;
        }
        if constexpr (!RATE) {
            __shared__ int lev_rdoq[kElems], ebits_rdoq[128];
            lev = lev_rdoq; ebits = ebits_rdoq;
        }
    }

    const int tid = threadIdx.x;
    if constexpr (RDOQ && !RATE) {
        if (tid < 128) ebits[tid] = cabac::entropy_bits_table()[tid];
    }
    if constexpr (RATE) {
        if (tid < 128) ebits[tid] = cabac::entropy_bits_table()[tid];
        if (tid < 64) lps[tid] = cabac::trans_idx_lps_table()[tid];
        for (int i = tid; i < kMaxQps * G; i += kTqThreads) bits[i] = 0;
    }
    for (int i = tid; i < TT; i += kTqThreads) mat[(i / T) * MS + i % T] = matrix_coeff(L, i / T, i % T);
    for (int i = tid; i < kMaxQps * 3 * G; i += kTqThreads) (&sums[0][0][0])[i] = 0;

    const int col = tid % T;                      // e % T of all four samples
    int row[kPerLane], base[kPerLane], pred[kPerLane], tgt[kPerLane];
    long blk[kPerLane];                           // the sample's block; -1 past N
    const long blk0 = (long)blockIdx.x * G;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const int e = j * kTqThreads + tid;
        row[j] = (e / T) % T;
        base[j] = e / TT * TT;
        const long b = blk0 + e / TT;
        blk[j] = b < p.N ? b : -1;
    }

    // SDH: lane tid of round j is scan position (256 j + tid) % TT of unit (256 j + tid) / TT; where that lies in LDS
    [[maybe_unused]] int hide_at[kPerLane];
    if constexpr (SDH || RDOQ) {
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const int s = j * kTqThreads + tid, u = s / TT, i = s % TT;
            const long b = blk0 + u;
            const int scan = p.modes && b < p.N ? cabac::scan_of_mode(L, p.modes[b]) : cabac::kScanDiag;
            int cx, cy, x, y;
            cabac::scan_position<L - 2>(scan, i >> 4, &cx, &cy);
            cabac::scan_position<2>(scan, i & 15, &x, &y);
            hide_at[j] = u * TT + (cy * 4 + y) * T + cx * 4 + x;
        }
    }

#pragma unroll 1
    for (int q = 0; q < NQ; q++) {
        const int uy = q / U, ux = q % U;
        // residual of the unit(s): target - prediction
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            pred[j] = 0; tgt[j] = 0;
            if (blk[j] >= 0) {
                const size_t at = ((size_t)blk[j] * W + uy * T + row[j]) * W + ux * T + col;
                pred[j] = p.pred[at]; tgt[j] = p.targets[at];
            }
            buf_a[j * kTqThreads + tid] = tgt[j] - pred[j];
        }
        __syncthreads();                          // (also: mat and sums are written)
        {   // forward, first stage: rows
            int acc[kPerLane] = {};
#pragma unroll 8
            for (int x = 0; x < T; x++) {
                const int m = mat[col * MS + x];
#pragma unroll
                for (int j = 0; j < kPerLane; j++) acc[j] += buf_a[base[j] + row[j] * T + x] * m;
            }
#pragma unroll
            for (int j = 0; j < kPerLane; j++) buf_b[j * kTqThreads + tid] = (acc[j] + (1 << (fwd_shift1(L) - 1))) >> fwd_shift1(L);
        }
        __syncthreads();
        {   // forward, second stage: columns
            int acc[kPerLane] = {};
#pragma unroll 8
            for (int y = 0; y < T; y++)
#pragma unroll
                for (int j = 0; j < kPerLane; j++) acc[j] += buf_b[base[j] + y * T + col] * mat[row[j] * MS + y];
#pragma unroll
            for (int j = 0; j < kPerLane; j++) coef[j * kTqThreads + tid] = (acc[j] + (1 << (fwd_shift2(L) - 1))) >> fwd_shift2(L);
        }
        // (each lane reads back only the coefficients it wrote: no barrier)
#pragma unroll 1
        for (int qi = 0; qi < p.nb_qps; qi++) {
            const QpConsts qc = p.qp[qi];
            unsigned nonzero[kPerLane], sum_abs[kPerLane], sse[kPerLane];
            if constexpr (RDOQ) {
                // below T = 32 the uncoded costs lie in buf_a (scan positions 0 .. 511) and buf_b (512 .. 1023), each read as 512
                // doubles: no unit straddles the two, and both hold nothing between two QPs
                // (nothing declares the 8 bytes -- see the arrays' declaration --: a layout that loses them stops here, loudly; two scalar
                // instructions per QP beside the walk)
                if (T < 32 && ((reinterpret_cast<uintptr_t>(buf_a) | reinterpret_cast<uintptr_t>(buf_b)) & 7)) __builtin_trap();
                double* const cost0_lo = T == 32 ? rw.cost0 : reinterpret_cast<double*>(buf_a);
                double* const cost0_hi = T == 32 ? rw.cost0 + kElems / 2 : reinterpret_cast<double*>(buf_b);
                __syncthreads();                  // the coefficients are written; buf_b and the last QP's tables and levels are read
                for (int i = tid; i < rdoq::kEstBitsWords; i += kTqThreads)
                    (&est->ctx[0][0])[i] = rdoq::est_bits_word<L>(i, p.init_states[qi], p.cbf_states[qi], ebits);
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    const double c0 = rdoq::uncoded_cost(rdoq::level_double(coef[hide_at[j]], qc.scale, qc.qbits), p.rd[qi].err_scale);
                    (j < kPerLane / 2 ? cost0_lo : cost0_hi)[(j % (kPerLane / 2)) * kTqThreads + tid] = c0;
                }
                __syncthreads();
                if (tid < G) {                    // lane g quantises unit g (a unit past N has a zero residual: nothing to decide)
                    const long b = blk0 + tid;
                    const int scan = p.modes && b < p.N ? cabac::scan_of_mode(L, p.modes[b]) : cabac::kScanDiag;
                    rdoq::Work w = rw;
                    const int s0 = tid * TT;      // the unit's first scan position: in the lower or the upper half of the costs
                    w.cost0 = (s0 < kElems / 2 ? cost0_lo + s0 : cost0_hi + (s0 - kElems / 2));
                    w.cost += s0; w.cost_sig += s0; w.group_sig += s0 / 16;
                    if constexpr (SDH) { w.rate_up += s0; w.rate_down += s0; w.sig_delta += s0; w.delta_u += s0; }
                    unit_abs[tid] = rdoq::unit<L>(coef + s0, scan, qc.scale, qc.qbits, p.rd[qi], *est, p.cbf_ctx, SDH, lev + s0, w, nullptr);
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    const int level = lev[j * kTqThreads + tid];
                    nonzero[j] = level != 0;
                    sum_abs[j] = 0;                                // HM's uiAbsSum is the walk's: added per unit below
                    buf_a[j * kTqThreads + tid] = dequant_level(level, qc);
                }
                if (tid < G) atomicAdd(&sums[qi][2][tid], (unsigned)unit_abs[tid]);
            } else if constexpr (SDH) {
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    int mag, delta_u;
                    lev[j * kTqThreads + tid] = quant_level(coef[j * kTqThreads + tid], qc, &mag, &delta_u);
                    du[j * kTqThreads + tid] = delta_u;
                    sum_abs[j] = (unsigned)mag;                    // HM's uiAbsSum: before the hiding
                }
                if (TT > 64 && tid < G) lastg[tid] = -1;
                __syncthreads();
                // one lane per scan position: 16 consecutive lanes are one group, n = tid % 16
                const int n = tid & 15, shift = tid & 48;
                int lv[kPerLane], cf[kPerLane], dl[kPerLane];
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    lv[j] = lev[hide_at[j]]; cf[j] = coef[hide_at[j]]; dl[j] = du[hide_at[j]];
                    if (TT > 64) {                                 // the unit's last group: the highest one with a level
                        const unsigned long long any = __ballot(lv[j] != 0);
                        if (any && (tid & 63) == 0)
                            atomicMax(&lastg[(j * kTqThreads + tid) / TT], ((j * kTqThreads + tid) % TT >> 4) + ((63 - __builtin_clzll(any)) >> 4));
                    }
                }
                if (TT > 64) __syncthreads();
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    const unsigned long long any = __ballot(lv[j] != 0);
                    const unsigned nz = (unsigned)(any >> shift) & 0xffffu, neg = (unsigned)(__ballot(lv[j] < 0) >> shift) & 0xffffu;
                    const unsigned odd = (unsigned)(__ballot(lv[j] & 1) >> shift) & 0xffffu;
                    const int first = nz ? __builtin_ctz(nz) : 16, last = nz ? 31 - __builtin_clz(nz) : -1;
                    const int signbit = (int)(neg >> (first & 15)) & 1;
                    const int c = (j * kTqThreads + tid) % TT >> 4;
                    const bool last_group = TT == 16 ? true : TT == 64 ? c == (63 - __builtin_clzll(any | 1)) >> 4
                                                                       : c == lastg[(j * kTqThreads + tid) / TT];
                    int key = kSdhForbidden, change = 0;
                    if (last - first >= kSbhThreshold && signbit != (__builtin_popcount(odd) & 1) && n <= (last_group ? last : 15)) {
                        const int cost = sdh_cost(lv[j], cf[j], dl[j], n, first, signbit, &change);
                        if (cost != kSdhForbidden) key = ((cost + 256) << 4) | (15 - n);
                    }
                    int best = key;
#pragma unroll
                    for (int d = 8; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d));
                    if (key == best && key != kSdhForbidden) lev[hide_at[j]] = sdh_changed_level(lv[j], cf[j], change);
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    const int level = lev[j * kTqThreads + tid];
                    nonzero[j] = level != 0;
                    buf_a[j * kTqThreads + tid] = dequant_level(level, qc);
                }
            } else {
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    int mag;
                    const int level = quant_level(coef[j * kTqThreads + tid], qc, &mag);
                    nonzero[j] = level != 0;
                    sum_abs[j] = (unsigned)mag;
                    buf_a[j * kTqThreads + tid] = dequant_level(level, qc);
                    if constexpr (RATE) lev[j * kTqThreads + tid] = level;
                }
            }
            __syncthreads();
            if constexpr (RATE) {
                if (tid < G && blk0 + tid < p.N) {    // lane g codes unit g (units past N have no slot to add to)
                    const int scan = p.modes ? cabac::scan_of_mode(L, p.modes[blk0 + tid]) : cabac::kScanDiag;
                    bits[qi * G + tid] += cabac::unit_rate<L, SDH>(lev + tid * TT, scan, p.init_states[qi], states + tid * cabac::kNumCtx,
                                                              cabac::Tables{ebits, lps});
                }
            }
            {   // inverse, first stage: columns
                int acc[kPerLane] = {};
#pragma unroll 8
                for (int l = 0; l < T; l++)
#pragma unroll
                    for (int j = 0; j < kPerLane; j++) acc[j] += mat[l * MS + row[j]] * buf_a[base[j] + l * T + col];
#pragma unroll
                for (int j = 0; j < kPerLane; j++) buf_b[j * kTqThreads + tid] = clip16((acc[j] + (1 << (kInvShift1 - 1))) >> kInvShift1);
            }
            __syncthreads();
            {   // inverse, second stage: rows; reconstruction
                int acc[kPerLane] = {};
#pragma unroll 8
                for (int k = 0; k < T; k++) {
                    const int m = mat[k * MS + col];
#pragma unroll
                    for (int j = 0; j < kPerLane; j++) acc[j] += m * buf_b[base[j] + row[j] * T + k];
                }
#pragma unroll
                for (int j = 0; j < kPerLane; j++) {
                    const int r = clip16((acc[j] + (1 << (kInvShift2 - 1))) >> kInvShift2);
                    const int rec = min(max(pred[j] + r, 0), 255), d = rec - tgt[j];
                    sse[j] = (unsigned)(d * d);
                    if (p.recon && blk[j] >= 0)
                        p.recon[(((size_t)qi * p.N + blk[j]) * W + uy * T + row[j]) * W + ux * T + col] = (uint8_t)rec;
                }
            }
            // the three sums of each unit: at T = 32 the lane's four samples are one unit's, otherwise one unit per j
            if (G == 1) {
#pragma unroll
                for (int j = 1; j < kPerLane; j++) { sse[0] += sse[j]; nonzero[0] += nonzero[j]; sum_abs[0] += sum_abs[j]; }
            }
#pragma unroll
            for (int j = 0; j < (G == 1 ? 1 : kPerLane); j++) {
#pragma unroll
                for (int d = SEG / 2; d > 0; d >>= 1) {
                    sse[j] += __shfl_xor(sse[j], d);
                    nonzero[j] += __shfl_xor(nonzero[j], d);
                    sum_abs[j] += __shfl_xor(sum_abs[j], d);
                }
                if (tid % SEG == 0) {
                    const int g = (j * kTqThreads + tid) / TT;
                    atomicAdd(&sums[qi][0][g], sse[j]);
                    atomicAdd(&sums[qi][1][g], nonzero[j]);
                    atomicAdd(&sums[qi][2][g], sum_abs[j]);
                }
            }
            // the next QP (or unit) writes buf_a, which no lane reads after the barrier above; its own first barrier orders buf_b
        }
    }
    __syncthreads();
    for (int i = tid; i < p.nb_qps * G; i += kTqThreads) {
        const int qi = i / G, g = i % G;
        const long b = blk0 + g;
        if (b < p.N) {
            const size_t at = (size_t)qi * p.N + b;
            if (p.sse) p.sse[at] = sums[qi][0][g];
            if (p.nonzero) p.nonzero[at] = sums[qi][1][g];
            if (p.sum_abs) p.sum_abs[at] = sums[qi][2][g];
            if constexpr (RATE) p.rate[at] = bits[qi * G + g];
        }
    }
}

template <bool RATE, bool SDH>
hipError_t launch_width(const TrQuantParams& p, dim3 grid, dim3 block, hipStream_t s)
{
    switch (p.w) {
    case 4: hipLaunchKernelGGL((trquant_kernel<4, RATE, SDH>), grid, block, 0, s, p); break;
    case 8: hipLaunchKernelGGL((trquant_kernel<8, RATE, SDH>), grid, block, 0, s, p); break;
    case 16: hipLaunchKernelGGL((trquant_kernel<16, RATE, SDH>), grid, block, 0, s, p); break;
    case 32: hipLaunchKernelGGL((trquant_kernel<32, RATE, SDH>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((trquant_kernel<64, RATE, SDH>), grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

template <bool RATE, bool SDH>
hipError_t launch_width_rdoq(const TrQuantParams& p, dim3 grid, dim3 block, hipStream_t s)
{
    switch (p.w) {
    case 4: hipLaunchKernelGGL((trquant_kernel<4, RATE, SDH, true>), grid, block, 0, s, p); break;
    case 8: hipLaunchKernelGGL((trquant_kernel<8, RATE, SDH, true>), grid, block, 0, s, p); break;
    case 16: hipLaunchKernelGGL((trquant_kernel<16, RATE, SDH, true>), grid, block, 0, s, p); break;
    case 32: hipLaunchKernelGGL((trquant_kernel<32, RATE, SDH, true>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((trquant_kernel<64, RATE, SDH, true>), grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

}  // namespace

int trquant_blocks_per_workgroup(int w) { return w >= 32 ? 1 : kElems / (w * w); }

hipError_t launch_trquant(const TrQuantParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.pred || !p.targets || p.nb_qps < 1 || p.nb_qps > trquant::kMaxQps) return hipErrorInvalidValue;
    if (trquant::log2_tu(p.w) < 0) return hipErrorInvalidValue;
    const int g = trquant_blocks_per_workgroup(p.w);
    const dim3 grid((unsigned)((p.N + g - 1) / g)), block(kTqThreads);
    if (p.rdoq) {
        if (p.rate) return p.sdh ? launch_width_rdoq<true, true>(p, grid, block, s) : launch_width_rdoq<true, false>(p, grid, block, s);
        return p.sdh ? launch_width_rdoq<false, true>(p, grid, block, s) : launch_width_rdoq<false, false>(p, grid, block, s);
    }
    if (p.rate) return p.sdh ? launch_width<true, true>(p, grid, block, s) : launch_width<true, false>(p, grid, block, s);
    return p.sdh ? launch_width<false, true>(p, grid, block, s) : launch_width<false, false>(p, grid, block, s);
}

}  // namespace pnn
