// HEVC best-intra-mode search for the evaluator's competitor (comparing_pnn_ipfcns_hevc_best_mode.py:162-322 via
// hevc/intraprediction/intraprediction.py:231-294): for each of N blocks, all 35 luma predictions of HM's xPredIntraPlanar /
// DC / xPredIntraAng from the block's intra pattern (no reference smoothing unless asked for, below: the reference did not extract it), the SSE of
// each against the target, and the mode of smallest SSE (lowest index among ties -- the reference keeps a mode only when its
// PSNR, strictly decreasing in the SSE, is strictly larger).  Integer VALU arithmetic only; bit-exact against the host twin
// (pnn_hevc_intra.cpp), which builds refMain the way HM does.
//
// Layout.  A workgroup of 7 waves takes G blocks and stages their 4w+1 reference samples (padded as the reference pads them)
// and targets in LDS.  Its 35 * 64 tasks are (mode, block, row group): each wave runs one mode at a time (5 rounds), so the
// mode -- planar, DC or one angle -- is wave-uniform and nothing diverges.  A lane covers R rows of one block in the mode's own
// orientation (v along the side reference, u along the main one); w <= 8: the whole block (R = w, no reduction), w >= 16: R = 4
// rows, partial SSEs added with LDS integer atomics (exact in any order).  The angular prediction is the closed form of
// refMain: index k >= 0 reads the main reference, k < 0 the side one at (128 - k * invAngle) >> 8, as HM's projection loop fills it.
// Then one lane per block picks the best mode and the workgroup recomputes that mode's prediction only if it is asked for.
// The staging loops have a second source: the evaluator's pictures themselves (PIC), 4w + 1 + w^2 bytes per block instead of a
// dense (2w + 1)^2 pattern and a target copy; everything after the staging is shared.  The pictures are a pair of planes (decoded
// for the reference samples, original for the targets); a single picture is the pair of one plane with itself.
//
// hevc_mode_hads_kernel is the SATD twin of the search, the metric of HM's first intra pass (TEncSearch.cpp:2376-2492): the same
// staging and the same per-pixel mode functions, but a lane owns one T x T sub-block (T = 8, 4 at w = 4) of one block and one mode at
// a time -- its T^2 residuals in registers, the Walsh-Hadamard butterflies of pnn_wht.h, the rounding of TComRdCost::xGetHADs -- and
// adds the sub-block's cost into cost[block][mode] in LDS.  A candidate prediction handed in (the PNN's) is costed as index 35 in a
// sixth round of one wave; then one lane per block builds HM's sorted candidate list (xUpdateCandList).  Reference smoothing as an option (as
// below) and no modeBits * sqrtLambda term: the costs are the distortions alone.
//
// HM's reference-sample smoothing (include/pnn_hip.h, "smoothing") is the compile-time axis SMOOTH of both kernels, instantiated for
// w = 8, 16, 32 only (no mode smooths at 4 and 64).  A second staging pass, stage_smoothed, filters the staged line LDS -> LDS into
// ref_s (same stride); at w = 32 one lane per block first takes the strong-filter decision into LDS, and whether the strong filter is
// allowed at all is the runtime field p.smoothing, one uniform branch.  In the mode rounds the mode is wave-uniform, so the wave picks
// ref or ref_s by mode_smooths(mode) with one scalar select and runs the same pixel functions; DC and the modes 10 / 26 are not in that
// table, so the DC value, the DC filter and the edge filter read ref by construction.  With SMOOTH = false the kernels are the code
// they were.
#include "pnn_kernels.h"
#include "pnn_wht.h"

namespace pnn {
namespace {

constexpr int kThreads = 448;                     // 7 waves: 35 modes in 5 rounds
constexpr int kRounds = 35 / (kThreads / 64);

__device__ inline int intra_angle(int mode)       // angTable with its sign, modes 2..34
{
    const int rel = mode >= 18 ? mode - 26 : 10 - mode, a = rel < 0 ? -rel : rel;
    const int t = a == 0 ? 0 : a == 1 ? 2 : a == 2 ? 5 : a == 3 ? 9 : a == 4 ? 13 : a == 5 ? 17 : a == 6 ? 21 : a == 7 ? 26 : 32;
    return rel < 0 ? -t : t;
}

__device__ inline int intra_inv_angle(int ang)     // invAngTable for a negative angle
{
    const int a = -ang;
    return a == 2 ? 4096 : a == 5 ? 1638 : a == 9 ? 910 : a == 13 ? 630 : a == 17 ? 482 : a == 21 ? 390 : a == 26 ? 315 : 256;
}

// refMain[k] in the orientation S (+1: vertical modes, main = above; -1: horizontal, main = left); rf[j], j in [-2w, 2w], holds
// left[-j - 1] for j < 0, the corner at 0 and above[j - 1] for j > 0.  k <= 2w + 1 (the +1 only where its weight is zero).
template <int W, int S>
__device__ inline int ref_main(const int* rf, int k, int inv)
{
    const int idx = k >= 0 ? min(k, 2 * W) : -((128 - k * inv) >> 8);
    return rf[S * idx];
}

template <int W, int S>
__device__ inline int angular_pixel(const int* rf, int ang, int inv, int v, int u)
{
    const int pos = (v + 1) * ang, f = pos & 31, k = u + (pos >> 5) + 1;
    const int a = ref_main<W, S>(rf, k, inv);
    int p = ((32 - f) * a + f * ref_main<W, S>(rf, k + 1, inv) + 16) >> 5;
    if (W <= 16 && ang == 0 && u == 0) p = min(max(a + ((rf[-S * (v + 1)] - rf[0]) >> 1), 0), 255);
    return p;
}

template <int W>
__device__ inline int planar_pixel(const int* rf, int y, int x)
{
    constexpr int shift = W == 4 ? 2 : W == 8 ? 3 : W == 16 ? 4 : W == 32 ? 5 : 6;
    return ((W - 1 - x) * rf[-1 - y] + (x + 1) * rf[1 + W] + (W - 1 - y) * rf[1 + x] + (y + 1) * rf[-1 - W] + W) >> (shift + 1);
}

template <int W>
__device__ inline int dc_pixel(const int* rf, int dc, int y, int x)
{
    if (W > 16 || (x > 0 && y > 0)) return dc;
    if (x == 0 && y == 0) return (rf[1] + rf[-1] + 2 * dc + 2) >> 2;
    return ((y == 0 ? rf[1 + x] : rf[-1 - y]) + 3 * dc + 2) >> 2;
}

template <int W>
__device__ inline int mode_pixel(const int* rf, int dc, int mode, int y, int x)
{
    if (mode == 0) return planar_pixel<W>(rf, y, x);
    if (mode == 1) return dc_pixel<W>(rf, dc, y, x);
    const int ang = intra_angle(mode), inv = ang < 0 ? intra_inv_angle(ang) : 0;
    return mode >= 18 ? angular_pixel<W, 1>(rf, ang, inv, y, x) : angular_pixel<W, -1>(rf, ang, inv, x, y);
}

// SSE of rows v = rg, rg + RG, ... (R of them) of an angular mode in its own orientation; target element (y, x) at tg[y * W + x]
template <int W, int R, int RG, int S>
__device__ inline unsigned angular_rows_sse(const int* rf, const uint8_t* tg, int ang, int inv, int rg)
{
    unsigned acc = 0;
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const int v = rg + RG * r;
        const int pos = (v + 1) * ang, f = pos & 31;
        int k = (pos >> 5) + 1;
        int a = ref_main<W, S>(rf, k, inv);
#pragma unroll 8
        for (int u = 0; u < W; u++, k++) {
            const int b = ref_main<W, S>(rf, k + 1, inv);
            int p = ((32 - f) * a + f * b + 16) >> 5;
            if (W <= 16 && u == 0 && ang == 0) p = min(max(a + ((rf[-S * (v + 1)] - rf[0]) >> 1), 0), 255);
            const int d = p - (int)tg[S > 0 ? v * W + u : u * W + v];
            acc += (unsigned)(d * d);
            a = b;
        }
    }
    return acc;
}

// offset of the top-left pixel of block b's context square from the first picture (b = image * positions + position)
__device__ inline size_t picture_corner(const PictureBlocks& pic, long b)
{
    const long img = b / pic.positions;
    const int pos = (int)(b - img * pic.positions);
    return ((size_t)img * pic.H + pic.rows[pos]) * pic.W + pic.cols[pos];
}

// Staging shared by the two kernels: the padded 4w + 1 reference samples (ref, stride RS ints) and the w^2 targets (tgt, stride TS
// bytes) of the workgroup's G blocks, zeros for blocks past p.N; `Params` is either kernel's.  PIC = false: reference samples from dense
// intra patterns, targets from their own array; true: both from pictures -- the reference samples from the context plane (p.pic.channels),
// the targets from the target plane (p.pic_targets), which have one geometry and so share each block's offset `corner`.  For single
// pictures the two pointers are equal.  NT: the threads of the calling workgroup (rd_candidates_kernel has 256).
// MASKS (picture form only; p.pic.mask_w / mask_h set): every block is clamped with its OWN pw = 2w + 1 - mask_w[pos] and ph in place of
// the call's p.pw / p.ph, kept per staged block in G ints of LDS beside the corners.  MASKS = false is the staging of the scalar
// entries, instruction for instruction what it was before masks per block existed.
template <int W, int G, bool PIC, bool MASKS, int NT = kThreads, typename Params>
__device__ __forceinline__ void stage_blocks(const Params& p, long blk0, int tid, int* ref, uint8_t* tgt, size_t* corner)
{
    static_assert(PIC || !MASKS, "masks per block exist in the picture form only");
    constexpr int RS = 4 * W + 1, TS = W * W + 4;                 // LDS strides (odd in dwords: lanes of different blocks spread over banks)
    __shared__ int last[MASKS ? G : 1];                           // MASKS: (pw - 1) | (ph - 1) << 16 of each staged block
    if (PIC) {
        if (tid < G && blk0 + tid < p.N) {
            corner[tid] = picture_corner(p.pic, blk0 + tid);
            if (MASKS) {
                const int pos = (int)((blk0 + tid) % p.pic.positions);
                last[tid] = (2 * W - p.pic.mask_w[pos]) | (2 * W - p.pic.mask_h[pos]) << 16;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < G * RS; i += NT) {
        const int g = i / RS, j = i % RS - 2 * W;
        int v = 0;
        if (blk0 + g < p.N) {
            if (PIC) {                                 // the dense form's padding rule in picture coordinates: inside the block's 3w x 3w context square
                const uint8_t* pat = p.pic.channels + corner[g] + (size_t)(W - 1) * p.pic.W + W - 1;
                const int pw1 = MASKS ? last[g] & 0xffff : p.pw - 1, ph1 = MASKS ? last[g] >> 16 : p.ph - 1;
                v = j >= 0 ? pat[min(j, pw1)] : pat[(size_t)min(-j, ph1) * p.pic.W];
            } else {
                const uint8_t* pat = p.patterns + (size_t)(blk0 + g) * p.ph * p.pw;
                v = j >= 0 ? pat[min(j, p.pw - 1)] : pat[min(-j, p.ph - 1) * p.pw];
            }
        }
        ref[i] = v;
    }
    for (int i = tid; i < G * W * W; i += NT) {
        const int g = i / (W * W), e = i % (W * W);
        int v = 0;
        if (blk0 + g < p.N) {
            if (PIC) v = p.pic_targets[corner[g] + (size_t)(W + e / W) * p.pic.W + W + e % W];   // the target plane, same offset
            else v = p.targets[(size_t)(blk0 + g) * W * W + e];
        }
        tgt[g * TS + e] = (uint8_t)v;
    }
}

// predIntraGetPredValDC of the G staged blocks, one lane each
template <int W, int G>
__device__ __forceinline__ void stage_dc(const int* ref, int* dcv, int tid)
{
    if (tid < G) {
        const int* rf = ref + tid * (4 * W + 1) + 2 * W;
        int sum = 0;
        for (int i = 1; i <= W; i++) sum += rf[i] + rf[-i];
        dcv[tid] = (sum + W) / (2 * W);
    }
}

// intraFilterThreshold (TComPrediction.cpp:39-55): does `mode` read the smoothed line at this width?  Never DC, never modes 10 / 26.
template <int W>
__device__ inline bool mode_smooths(int mode)
{
    constexpr int thr = W == 8 ? 7 : W == 16 ? 1 : W == 32 ? 0 : 10;
    return mode != 1 && min(abs(mode - 10), abs(mode - 26)) > thr;
}

// filteringIntraReferenceSamples on the G staged (hence padded) lines, LDS -> LDS: ref_s has ref's layout.  Both ends are copied.
// W = 32: one lane per block decides whether its line is strong (both halves flat at their anchors; only when `allow_strong`), then
// every thread writes bilinear samples (corner copied) or [1 2 1] ones as its block's flag says.  Called between two barriers: ref is
// complete on entry, the caller's next barrier publishes ref_s.
template <int W, int G, int NT = kThreads>
__device__ __forceinline__ void stage_smoothed(const int* ref, int* ref_s, int* strong, bool allow_strong, int tid)
{
    constexpr int RS = 4 * W + 1;
    if (W == 32) {
        const int g = tid - 64;                        // the second wave: the first one is in stage_dc
        if (g >= 0 && g < G) {
            const int* rf = ref + g * RS + 2 * W;
            int s = 0;
            if (allow_strong) s = abs(rf[-64] + rf[0] - 2 * rf[-32]) < 8 && abs(rf[0] + rf[64] - 2 * rf[32]) < 8;   // 1 << (bitDepth - 5)
            strong[g] = s;
        }
        __syncthreads();
    }
    for (int i = tid; i < G * RS; i += NT) {
        const int g = i / RS, j = i % RS - 2 * W;
        const int* rf = ref + g * RS + 2 * W;
        int v;
        if (j == -2 * W || j == 2 * W) v = rf[j];
        else if (W == 32 && strong[g]) v = j == 0 ? rf[0] : j < 0 ? (-j * rf[-64] + (64 + j) * rf[0] + 32) >> 6 : ((64 - j) * rf[0] + j * rf[64] + 32) >> 6;
        else v = (rf[j - 1] + 2 * rf[j] + rf[j + 1] + 2) >> 2;
        ref_s[i] = v;
    }
}

template <int W, bool PIC, bool SMOOTH, bool MASKS = false>
__global__ __launch_bounds__(kThreads) void hevc_best_mode_kernel(const HevcBestModeParams p)
{
    constexpr int R = W <= 8 ? W : 4, RG = W / R, G = 64 / RG;    // rows per lane, lanes per block, blocks per workgroup
    constexpr int RS = 4 * W + 1, TS = W * W + 4;                 // LDS strides, those of stage_blocks
    static_assert(!SMOOTH || W == 8 || W == 16 || W == 32, "no mode smooths at w = 4 and 64");
    __shared__ int ref[G * RS];
    __shared__ int ref_s[SMOOTH ? G * RS : 1];
    __shared__ int strong[SMOOTH && W == 32 ? G : 1];
    __shared__ uint8_t tgt[G * TS];
    __shared__ unsigned sse[G * 35];
    __shared__ int dcv[G], best[G];
    __shared__ size_t corner[PIC ? G : 1];
    const int tid = threadIdx.x;
    const long blk0 = (long)blockIdx.x * G;

    stage_blocks<W, G, PIC, MASKS>(p, blk0, tid, ref, tgt, corner);
    for (int i = tid; i < G * 35; i += kThreads) sse[i] = 0;
    __syncthreads();
    stage_dc<W, G>(ref, dcv, tid);
    if (SMOOTH) stage_smoothed<W, G>(ref, ref_s, strong, p.smoothing == 2, tid);
    __syncthreads();

    const int lane = tid & 63, g = lane / RG, rg = lane % RG;
    const uint8_t* tg = tgt + g * TS;
    for (int round = 0; round < kRounds; round++) {
        const int mode = __builtin_amdgcn_readfirstlane(round * (kThreads / 64) + tid / 64);
        const int* rf = (SMOOTH && mode_smooths<W>(mode) ? ref_s : ref) + g * RS + 2 * W;   // the line this mode reads: a scalar select
        unsigned acc = 0;
        if (mode <= 1) {
            const int dc = dcv[g];
#pragma unroll 1
            for (int r = 0; r < R; r++) {
                const int y = rg + RG * r;
#pragma unroll 8
                for (int x = 0; x < W; x++) {
                    const int d = (mode == 0 ? planar_pixel<W>(rf, y, x) : dc_pixel<W>(rf, dc, y, x)) - (int)tg[y * W + x];
                    acc += (unsigned)(d * d);
                }
            }
        } else {
            const int ang = intra_angle(mode), inv = ang < 0 ? intra_inv_angle(ang) : 0;
            acc = mode >= 18 ? angular_rows_sse<W, R, RG, 1>(rf, tg, ang, inv, rg) : angular_rows_sse<W, R, RG, -1>(rf, tg, ang, inv, rg);
        }
        if (RG == 1) sse[g * 35 + mode] = acc;
        else atomicAdd(&sse[g * 35 + mode], acc);
    }
    __syncthreads();

    if (tid < G && blk0 + tid < p.N) {
        const unsigned* s = sse + tid * 35;
        int m = 0;
        for (int i = 1; i < 35; i++) m = s[i] < s[m] ? i : m;
        if (p.best_mode) p.best_mode[blk0 + tid] = (uint8_t)m;
        if (p.best_sse) p.best_sse[blk0 + tid] = s[m];
        best[tid] = s[m] == 65025u * W * W ? -1 : m;   // no mode beats the reference's 0 dB start: index 0, all-zero prediction
    }
    if (p.mode_sse)
        for (int i = tid; i < G * 35; i += kThreads)
            if (blk0 + i / 35 < p.N) p.mode_sse[blk0 * 35 + i] = sse[i];
    if (!p.best_pred) return;
    __syncthreads();
    for (int i = tid; i < G * W * W; i += kThreads) {
        const int gg = i / (W * W), e = i % (W * W);
        if (blk0 + gg >= p.N) break;
        const int m = best[gg];
        const int* rf = (SMOOTH && mode_smooths<W>(m) ? ref_s : ref) + gg * RS + 2 * W;    // the winner's line
        const int v = m < 0 ? 0 : mode_pixel<W>(rf, dcv[gg], m, e / W, e % W);
        p.best_pred[blk0 * W * W + i] = (uint8_t)v;
    }
}

// Hadamard cost of the T x T sub-block at (by, bx) of one block: residual = target - pred(y, x) in registers, transform, sum of
// absolute coefficients, xGetHADs' rounding.  Target rows are read as 32-bit words (tg and every row start are 4-byte aligned).
template <int W, int T, typename Pred>
__device__ __forceinline__ unsigned sub_block_hads(const uint8_t* tg, int by, int bx, Pred pred)
{
    int d[T * T];
#pragma unroll
    for (int y = 0; y < T; y++) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(tg + (by + y) * W + bx);
#pragma unroll
        for (int x4 = 0; x4 < T; x4 += 4) {
            const uint32_t word = row[x4 / 4];
#pragma unroll
            for (int x = x4; x < x4 + 4; x++) d[y * T + x] = (int)((word >> (8 * (x - x4))) & 255u) - pred(by + y, bx + x);
        }
        __builtin_amdgcn_sched_barrier(0);             // a row at a time: hoisting all T^2 pixels' loads and addresses costs > 200 VGPRs
    }
    wht_rows_cols<T>(d);
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < T * T; k++) s += (unsigned)abs(d[k]);
    return hads_round<T>(s);
}

// The SATD twin of hevc_best_mode_kernel (same staging, same forms PIC).  Lane = (block g, sub-block sb) of the workgroup's G =
// 64 / (w / T)^2 blocks; wave = one mode per round, so the mode is wave-uniform.  cost[g][0 .. 34] the modes, [35] the candidate.
template <int W, bool PIC, bool SMOOTH, bool MASKS = false>
__global__ __launch_bounds__(kThreads) void hevc_mode_hads_kernel(const HevcModeHadsParams p)
{
    static_assert(!SMOOTH || W == 8 || W == 16 || W == 32, "no mode smooths at w = 4 and 64");
    constexpr int T = W == 4 ? 4 : 8, SB = W / T, NSB = SB * SB, G = 64 / NSB;   // sub-block side, sub-blocks per side / block, blocks per workgroup
    constexpr int K = W <= 8 ? 8 : 3, NC = 36;                                  // list entries, costs per block
    constexpr int RS = 4 * W + 1, TS = W * W + 4;                               // LDS strides, those of stage_blocks
    __shared__ int ref[G * RS];
    __shared__ int ref_s[SMOOTH ? G * RS : 1];
    __shared__ int strong[SMOOTH && W == 32 ? G : 1];
    __shared__ __attribute__((aligned(4))) uint8_t tgt[G * TS];
    __shared__ __attribute__((aligned(4))) uint8_t cnd[G * TS];
    __shared__ unsigned cost[G * NC];
    __shared__ int dcv[G];
    __shared__ size_t corner[PIC ? G : 1];
    const int tid = threadIdx.x;
    const long blk0 = (long)blockIdx.x * G;

    stage_blocks<W, G, PIC, MASKS>(p, blk0, tid, ref, tgt, corner);
    if (p.cand_pred)
        for (int i = tid; i < G * W * W; i += kThreads) {
            const int g = i / (W * W), e = i % (W * W);
            cnd[g * TS + e] = blk0 + g < p.N ? p.cand_pred[blk0 * W * W + i] : (uint8_t)0;
        }
    for (int i = tid; i < G * NC; i += kThreads) cost[i] = 0;
    __syncthreads();
    stage_dc<W, G>(ref, dcv, tid);
    if (SMOOTH) stage_smoothed<W, G>(ref, ref_s, strong, p.smoothing == 2, tid);
    __syncthreads();

    const int lane = tid & 63, g = lane / NSB, sb = lane % NSB;
    const int by = sb / SB * T, bx = sb % SB * T;
    const uint8_t* tg = tgt + g * TS;
    for (int round = 0; round < kRounds; round++) {
        const int mode = __builtin_amdgcn_readfirstlane(round * (kThreads / 64) + tid / 64);
        const int* rf = (SMOOTH && mode_smooths<W>(mode) ? ref_s : ref) + g * RS + 2 * W;   // the line this mode reads: a scalar select
        unsigned acc;
        if (mode == 0) {
            acc = sub_block_hads<W, T>(tg, by, bx, [&](int y, int x) { return planar_pixel<W>(rf, y, x); });
        } else if (mode == 1) {
            const int dc = dcv[g];
            acc = sub_block_hads<W, T>(tg, by, bx, [&](int y, int x) { return dc_pixel<W>(rf, dc, y, x); });
        } else {
            const int ang = intra_angle(mode), inv = ang < 0 ? intra_inv_angle(ang) : 0;
            if (mode >= 18) acc = sub_block_hads<W, T>(tg, by, bx, [&](int y, int x) { return angular_pixel<W, 1>(rf, ang, inv, y, x); });
            else acc = sub_block_hads<W, T>(tg, by, bx, [&](int y, int x) { return angular_pixel<W, -1>(rf, ang, inv, x, y); });
        }
        if (NSB == 1) cost[g * NC + mode] = acc;
        else atomicAdd(&cost[g * NC + mode], acc);
    }
    if (p.cand_pred && tid < 64) {                     // the sixth round: the candidate, one wave
        const uint8_t* cd = cnd + g * TS;
        const unsigned acc = sub_block_hads<W, T>(tg, by, bx, [&](int y, int x) { return (int)cd[y * W + x]; });
        if (NSB == 1) cost[g * NC + 35] = acc;
        else atomicAdd(&cost[g * NC + 35], acc);
    }
    __syncthreads();

    if (p.mode_hads)
        for (int i = tid; i < G * 35; i += kThreads)
            if (blk0 + i / 35 < p.N) p.mode_hads[blk0 * 35 + i] = cost[i / 35 * NC + i % 35];
    if (p.cand_hads && tid < G && blk0 + tid < p.N) p.cand_hads[blk0 + tid] = cost[tid * NC + 35];
    if ((p.list_modes || p.list_costs) && tid < G && blk0 + tid < p.N) {
        // xUpdateCandList for indices 0, 1, ... in turn: an entry goes in front of the first strictly larger cost, the rest moves down
        const unsigned* c = cost + tid * NC;
        const int nc = p.cand_pred ? 36 : 35;
        unsigned lc[K];
        int lm[K];
#pragma unroll
        for (int j = 0; j < K; j++) { lc[j] = 0xffffffffu; lm[j] = 255; }
#pragma unroll 1
        for (int i = 0; i < nc; i++) {
            unsigned ci = c[i];
            int mi = i;
            bool in = false;
#pragma unroll
            for (int j = 0; j < K; j++) {
                in = in || ci < lc[j];
                const unsigned tc = lc[j];
                const int tm = lm[j];
                lc[j] = in ? ci : tc; lm[j] = in ? mi : tm;
                ci = in ? tc : ci; mi = in ? tm : mi;
            }
        }
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (p.list_modes) p.list_modes[(blk0 + tid) * K + j] = (uint8_t)lm[j];
            if (p.list_costs) p.list_costs[(blk0 + tid) * K + j] = lc[j];
        }
    }
}

// Candidates of HM's second intra pass: the predictions the RD choice codes.  A workgroup of 4 waves takes G
// blocks -- as many as trquant_kernel, which codes what this kernel writes -- stages them as the kernels above do, and one lane per
// block turns the block's first-pass list (K modes a launch of hevc_mode_hads_kernel left on the device) into K + 1 slots: the list in
// order, then 35 if the list lacks it, else 255.  Then the G (K + 1) w^2 output pixels, one after the other over the workgroup: slot
// s of block g gets mode_pixel of its mode from the line that mode reads (modes 0 .. 34), the candidate's own pixel (35) or the target
// (255, and any value above 35: a zero residual), and the target beside it.  Outputs are dense per workgroup: consecutive lanes,
// consecutive bytes.
constexpr int kRdThreads = 256;

// SLOTS: list_modes holds the block's K + 3 slot modes as signal_list_kernel left them, [N][K + 3], and the
// kernel derives nothing: it predicts them (cand_modes is not written).  Everything else is as it stands.
// SUBST (with SLOTS): the substitution codec's K + 2 slots, in which mode 18 is the candidate's prediction and 35
// does not occur.  Without it the statements are the ones they were.
template <int W, bool PIC, bool SMOOTH, bool SLOTS = false, bool SUBST = false, bool MASKS = false>
__global__ __launch_bounds__(kRdThreads) void rd_candidates_kernel(const RdCandidatesParams p)
{
    static_assert(!SMOOTH || W == 8 || W == 16 || W == 32, "no mode smooths at w = 4 and 64");
    constexpr int G = W >= 32 ? 1 : 1024 / (W * W);                // blocks per workgroup: trquant_kernel's
    static_assert(!SUBST || SLOTS, "the substitution codec has the slots form only");
    constexpr int K = W <= 8 ? 8 : 3, K1 = SLOTS ? K + (SUBST ? msig::kExtraSlotsSubstitution : msig::kExtraSlots) : K + 1;   // list entries, slots
    constexpr int kCand = SUBST ? msig::kSubstitutedMode : 35;     // the mode whose prediction is the caller's candidate
    constexpr int RS = 4 * W + 1, TS = W * W + 4;                  // LDS strides, those of stage_blocks
    __shared__ int ref[G * RS];
    __shared__ int ref_s[SMOOTH ? G * RS : 1];
    __shared__ int strong[SMOOTH && W == 32 ? G : 1];
    __shared__ uint8_t tgt[G * TS];
    __shared__ int dcv[G], slot_mode[G * K1];
    __shared__ size_t corner[PIC ? G : 1];
    const int tid = threadIdx.x;
    const long blk0 = (long)blockIdx.x * G;

    stage_blocks<W, G, PIC, MASKS, kRdThreads>(p, blk0, tid, ref, tgt, corner);
    __syncthreads();
    stage_dc<W, G>(ref, dcv, tid);
    if (SMOOTH) stage_smoothed<W, G, kRdThreads>(ref, ref_s, strong, p.smoothing == 2, tid);
    if constexpr (SLOTS) {
        for (int i = tid; i < G * K1; i += kRdThreads)
            if (blk0 + i / K1 < p.N) {
                const int m = p.list_modes[blk0 * K1 + i];
                slot_mode[i] = m > (SUBST ? 34 : 35) ? kRdUnusedSlot : m;
            }
    } else if (tid < G && blk0 + tid < p.N) {
        bool listed = false;
#pragma unroll
        for (int j = 0; j < K; j++) {
            const int m = p.list_modes[(blk0 + tid) * K + j];
            listed = listed || m == 35;
            slot_mode[tid * K1 + j] = m > 35 ? kRdUnusedSlot : m;
        }
        slot_mode[tid * K1 + K] = listed ? kRdUnusedSlot : 35;
#pragma unroll
        for (int j = 0; j < K1; j++) p.cand_modes[(blk0 + tid) * K1 + j] = (uint8_t)slot_mode[tid * K1 + j];
    }
    __syncthreads();

    const size_t out0 = (size_t)blk0 * K1 * W * W;
    if constexpr (SLOTS && W == 64) {
        // quadrant-major: each slot leaves as four 32 x 32 blocks, which the w = 32 transform launch codes as units of their own
        // (a loop of its own, so that the one below stays the statements it was)
        for (int i = tid; i < G * K1 * W * W; i += kRdThreads) {
            const int g = i / (K1 * W * W), q = (i >> 10) & 3, r = i & 1023;
            const int e = ((q >> 1) * 32 + (r >> 5)) * 64 + (q & 1) * 32 + (r & 31);
            if (blk0 + g >= p.N) break;
            const int m = slot_mode[g * K1 + i / (W * W) % K1];
            const int t = tgt[g * TS + e];
            int v = t;
            if (m == kCand) {
                v = p.cand_pred[(size_t)(blk0 + g) * W * W + e];
            } else if (m < 35) {
                const int* rf = ref + g * RS + 2 * W;
                v = mode_pixel<W>(rf, dcv[g], m, e / W, e % W);
            }
            p.slot_pred[out0 + i] = (uint8_t)v;
            p.slot_targets[out0 + i] = (uint8_t)t;
        }
        return;
    }
    for (int i = tid; i < G * K1 * W * W; i += kRdThreads) {
        const int g = i / (K1 * W * W), e = i % (W * W);
        if (blk0 + g >= p.N) break;
        const int m = slot_mode[g * K1 + i / (W * W) % K1];
        const int t = tgt[g * TS + e];
        int v = t;
        if (m == kCand) {
            v = p.cand_pred[(size_t)(blk0 + g) * W * W + e];
        } else if (m < 35) {
            const int* rf = (SMOOTH && mode_smooths<W>(m) ? ref_s : ref) + g * RS + 2 * W;
            v = mode_pixel<W>(rf, dcv[g], m, e / W, e % W);
        }
        p.slot_pred[out0 + i] = (uint8_t)v;
        p.slot_targets[out0 + i] = (uint8_t)t;
    }
}

// J = D + lambda R: one IEEE multiply and one IEEE add, each rounded once -- the host twin's two operations.  HIP's __dmul_rn and
// __dadd_rn are a plain * and + whose results the compiler may still contract into one v_fma_f64 (it did); the pragma is what forbids
// that, so the two operations stand here as themselves.
__device__ inline double rd_cost(uint32_t d, uint64_t r, double lambda)
{
#pragma clang fp contract(off)
    const double bits = lambda * (double)(r >> 15);
    return (double)d + bits;
}

// The costs and the winner, one lane per (QP, block); the K + 1 slots in order.
template <int K1>
__global__ __launch_bounds__(kRdThreads) void rd_decide_kernel(const RdDecideParams p)
{
    const long i = (long)blockIdx.x * kRdThreads + threadIdx.x;
    if (i >= (long)p.nb_qps * p.N) return;
    const int qi = (int)(i / p.N);
    const long b = i - (long)qi * p.N;
    const double lambda = p.lambda[qi];
    const size_t slot0 = (size_t)b * K1, at0 = (size_t)qi * p.N * K1 + slot0;
    double best = __builtin_inf();
    int best_slot = kRdUnusedSlot, best_mode = kRdUnusedSlot;
    uint32_t best_sse = 0;
    uint64_t best_rate = 0;
#pragma unroll
    for (int s = 0; s < K1; s++) {
        const int m = p.cand_modes[slot0 + s];
        const uint32_t d = p.sse[at0 + s];
        const uint64_t r = p.rate[at0 + s];
        const double j = m == kRdUnusedSlot ? __builtin_inf() : rd_cost(d, r, lambda);
        if (p.cand_costs) p.cand_costs[at0 + s] = j;
        if (j < best) { best = j; best_slot = s; best_mode = m; best_sse = d; best_rate = r; }
    }
    if (p.best_mode) p.best_mode[i] = (uint8_t)best_mode;
    if (p.best_slot) p.best_slot[i] = (uint8_t)best_slot;
    if (p.best_cost) p.best_cost[i] = best;
    if (p.best_sse) p.best_sse[i] = best_sse;
    if (p.best_rate) p.best_rate[i] = best_rate;
}

// The first pass with HM's mode-bit term, behind a launch of hevc_mode_hads_kernel that left the 35 + 1
// Hadamard costs of every block on the device: one lane per (QP, block) derives the block's most probable modes, ranks the 36 costs
// SATD + modeBits sqrt(lambda) into HM's list and appends the missing MPMs and 35 -- msig::list_and_slots, the lines the host twin
// compiles.  The QPs' flag bits and sqrt(lambda) come ready in the argument block; a mode's bits are a few compares on the three MPMs,
// so there is no table, and the list lives in registers (every index into it is a compile-time one).
template <int K>
__global__ __launch_bounds__(kRdThreads) void signal_list_kernel(const SignalListParams p)
{
    constexpr int S = K + msig::kExtraSlots;
    const long i = (long)blockIdx.x * kRdThreads + threadIdx.x;
    if (i >= (long)p.nb_qps * p.N) return;
    const int qi = (int)(i / p.N);
    const long b = i - (long)qi * p.N;
    const msig::Mpm mpm = msig::derive_mpm(msig::neighbour_dir(p.left ? p.left[b] : msig::kNoNeighbour),
                                           msig::neighbour_dir(p.above ? p.above[b] : msig::kNoNeighbour));
    const uint32_t* hads = p.mode_hads + b * 35;
    const uint32_t cand = p.cand_hads[b];
    int lm[K], extra[msig::kExtraSlots];
    double lc[K];
    msig::list_and_slots<K>([&](int m) { return m < 35 ? hads[m] : cand; }, mpm, p.bits[qi], p.sqrt_lambda[qi], lm, lc, extra);
#pragma unroll
    for (int j = 0; j < K; j++) {
        if (p.list_costs) p.list_costs[(size_t)i * K + j] = lc[j];
        p.slot_modes[(size_t)i * S + j] = (uint8_t)lm[j];
    }
#pragma unroll
    for (int t = 0; t < msig::kExtraSlots; t++) p.slot_modes[(size_t)i * S + K + t] = (uint8_t)extra[t];
}

// The substitution codec's first pass: signal_list_kernel over HM's 35 modes, mode 18's Hadamard cost being the
// candidate's, without a flag bin and with K + 2 slots -- msig::list_and_slots_substitution, the lines the host twin compiles.
template <int K>
__global__ __launch_bounds__(kRdThreads) void substitution_list_kernel(const SignalListParams p)
{
    constexpr int S = K + msig::kExtraSlotsSubstitution;
    const long i = (long)blockIdx.x * kRdThreads + threadIdx.x;
    if (i >= (long)p.nb_qps * p.N) return;
    const int qi = (int)(i / p.N);
    const long b = i - (long)qi * p.N;
    const msig::Mpm mpm = msig::derive_mpm(msig::neighbour_dir(p.left ? p.left[b] : msig::kNoNeighbour),
                                           msig::neighbour_dir(p.above ? p.above[b] : msig::kNoNeighbour));
    const uint32_t* hads = p.mode_hads + b * 35;
    const uint32_t cand = p.cand_hads[b];
    int lm[K], extra[msig::kExtraSlotsSubstitution];
    double lc[K];
    msig::list_and_slots_substitution<K>([&](int m) { return m == msig::kSubstitutedMode ? cand : hads[m]; }, mpm, p.bits[qi], p.sqrt_lambda[qi],
                                         lm, lc, extra);
#pragma unroll
    for (int j = 0; j < K; j++) {
        if (p.list_costs) p.list_costs[(size_t)i * K + j] = lc[j];
        p.slot_modes[(size_t)i * S + j] = (uint8_t)lm[j];
    }
#pragma unroll
    for (int t = 0; t < msig::kExtraSlotsSubstitution; t++) p.slot_modes[(size_t)i * S + K + t] = (uint8_t)extra[t];
}

// rd_decide_kernel with the side bits, for the blocks of ONE QP (the slots are that QP's): J = D + lambda ((mode bits + cbf bin +
// rate) >> 15), one shift over the sum as HM's counter does over one candidate; the cbf bin follows the slot's count of nonzero levels.
__device__ inline double rd_cost_bits(uint32_t d, uint64_t whole_bits, double lambda)
{
#pragma clang fp contract(off)
    const double bits = lambda * (double)whole_bits;
    return (double)d + bits;
}

// Q: transform units per slot -- 1, or the 4 quadrants of a 64 x 64 block, each coded as a 32 x 32 block of its own: D and the rate
// add up, and every quadrant pays its own cbf bin.  FLAG: 1 with the switch codec's PNN flag in the mode bits, 0 without (the
// substitution codec, whose S is K + 2).
template <int S, int Q = 1, int FLAG = 1>
__global__ __launch_bounds__(kRdThreads) void rd_decide_signal_kernel(const RdDecideSignalParams p)
{
    const long b = (long)blockIdx.x * kRdThreads + threadIdx.x;
    if (b >= p.N) return;
    const msig::Mpm mpm = msig::derive_mpm(msig::neighbour_dir(p.left ? p.left[b] : msig::kNoNeighbour),
                                           msig::neighbour_dir(p.above ? p.above[b] : msig::kNoNeighbour));
    const size_t slot0 = (size_t)b * S;
    double best = __builtin_inf();
    int best_slot = kRdUnusedSlot, best_mode = kRdUnusedSlot;
    uint32_t best_sse = 0;
    uint64_t best_rate = 0, best_side = 0;
#pragma unroll
    for (int s = 0; s < S; s++) {
        const int m = p.slot_modes[slot0 + s];
        uint32_t d = 0;
        uint64_t r = 0, cbf = 0;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            d += p.sse[(slot0 + s) * Q + q];
            r += p.rate[(slot0 + s) * Q + q];
            cbf += msig::side_frac_bits(0, p.bits, p.cbf_ctx, p.nonzero[(slot0 + s) * Q + q]);
        }
        uint64_t side = 0;
        double j = __builtin_inf();
        if (m != kRdUnusedSlot) {
            side = msig::mode_frac_bits(m, mpm, p.bits, FLAG) + cbf;
            j = rd_cost_bits(d, (side + r) >> 15, p.lambda);
        }
        if (p.cand_costs) p.cand_costs[slot0 + s] = j;
        if (j < best) { best = j; best_slot = s; best_mode = m; best_sse = d; best_rate = r; best_side = side; }
    }
    if (p.best_mode) p.best_mode[b] = (uint8_t)best_mode;
    if (p.best_slot) p.best_slot[b] = (uint8_t)best_slot;
    if (p.best_cost) p.best_cost[b] = best;
    if (p.best_sse) p.best_sse[b] = best_sse;
    if (p.best_rate) p.best_rate[b] = best_rate;
    if (p.best_side_rate) p.best_side_rate[b] = best_side;
}

// The mode statistics of a second pass: per QP three histograms over the modes 0 .. 35 -- the mode occupies a used
// slot, the mode is in slot 0, the mode wins -- as stats [nb_qps][3][36].  One lane per (QP, block), the QP in blockIdx.y; the slot
// modes are [N][S] for all QPs or, per_qp, [nb_qps][N][S]; a value above 35 (255: unused slot, no winner) counts nowhere.  Every
// workgroup counts into LDS and adds its nonzero bins to the output, which the launcher's caller zeroed on the stream: integer sums,
// so the order of the atomics does not show.
constexpr int kStatsBins = 3 * 36;
__global__ __launch_bounds__(kRdThreads) void mode_stats_kernel(const ModeStatsParams p)
{
    __shared__ uint32_t hist[kStatsBins];
    const int tid = threadIdx.x, qi = blockIdx.y;
    for (int i = tid; i < kStatsBins; i += kRdThreads) hist[i] = 0;
    __syncthreads();
    const long b = (long)blockIdx.x * kRdThreads + tid;
    if (b < p.N) {
        const uint8_t* slots = p.slot_modes + ((p.per_qp ? (size_t)qi * p.N : 0) + b) * p.S;
        for (int s = 0; s < p.S; s++) {
            const int m = slots[s];
            if (m > 35) continue;
            atomicAdd(&hist[m], 1u);
            if (s == 0) atomicAdd(&hist[36 + m], 1u);
        }
        const int winner = p.best_mode[(size_t)qi * p.N + b];
        if (winner <= 35) atomicAdd(&hist[72 + winner], 1u);
    }
    __syncthreads();
    for (int i = tid; i < kStatsBins; i += kRdThreads)
        if (hist[i]) atomicAdd(&p.stats[(size_t)qi * kStatsBins + i], hist[i]);
}

}  // namespace

hipError_t launch_mode_stats(const ModeStatsParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.slot_modes || !p.best_mode || !p.stats || p.S < 1 || p.nb_qps < 1 || p.nb_qps > trquant::kMaxQps) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.N + kRdThreads - 1) / kRdThreads), (unsigned)p.nb_qps), block(kRdThreads);
    hipLaunchKernelGGL(mode_stats_kernel, grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_substitution_list(const SignalListParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.mode_hads || !p.cand_hads || !p.slot_modes || p.nb_qps < 1 || p.nb_qps > trquant::kMaxQps) return hipErrorInvalidValue;
    const long total = (long)p.nb_qps * p.N;
    const dim3 grid((unsigned)((total + kRdThreads - 1) / kRdThreads)), block(kRdThreads);
    if (p.w <= 8) hipLaunchKernelGGL((substitution_list_kernel<8>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((substitution_list_kernel<3>), grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_rd_candidates_substitution(const RdCandidatesParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    const int g = rd_candidates_blocks_per_workgroup(p.w);
    const dim3 grid((unsigned)((p.N + g - 1) / g)), block(kRdThreads);
    const bool pic = p.patterns == nullptr;
    if (pic && (!p.pic.channels || !p.pic_targets || !p.pic.mask_w != !p.pic.mask_h)) return hipErrorInvalidValue;
    const bool masks = pic && p.pic.mask_w;           // masks per position: the MASKS instantiation (the scalar entries keep theirs)
    if (!p.cand_pred || !p.list_modes || !p.slot_pred || !p.slot_targets) return hipErrorInvalidValue;
    if (p.smoothing < 0 || p.smoothing > 2) return hipErrorInvalidValue;
#define PNN_RD_LAUNCH(W_, SMOOTH_) \
    if (masks) hipLaunchKernelGGL((rd_candidates_kernel<W_, true, SMOOTH_, true, true, true>), grid, block, 0, s, p); \
    else if (pic) hipLaunchKernelGGL((rd_candidates_kernel<W_, true, SMOOTH_, true, true>), grid, block, 0, s, p); \
    else hipLaunchKernelGGL((rd_candidates_kernel<W_, false, SMOOTH_, true, true>), grid, block, 0, s, p);
#define PNN_RD_LAUNCH_SMOOTH(W_) if (p.smoothing) { PNN_RD_LAUNCH(W_, true) } else { PNN_RD_LAUNCH(W_, false) }
    switch (p.w) {                                     // (width 64 writes each slot as its four quadrants, 32 x 32 blocks)
    case 4: PNN_RD_LAUNCH(4, false) break;
    case 8: PNN_RD_LAUNCH_SMOOTH(8) break;
    case 16: PNN_RD_LAUNCH_SMOOTH(16) break;
    case 32: PNN_RD_LAUNCH_SMOOTH(32) break;
    case 64: PNN_RD_LAUNCH(64, false) break;
    default: return hipErrorInvalidValue;
    }
#undef PNN_RD_LAUNCH_SMOOTH
#undef PNN_RD_LAUNCH
    return hipGetLastError();
}

hipError_t launch_rd_decide_substitution(const RdDecideSignalParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.sse || !p.rate || !p.nonzero || !p.slot_modes || p.cbf_ctx < 0 || p.cbf_ctx > 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.N + kRdThreads - 1) / kRdThreads)), block(kRdThreads);
    if (p.w <= 8) hipLaunchKernelGGL((rd_decide_signal_kernel<8 + msig::kExtraSlotsSubstitution, 1, 0>), grid, block, 0, s, p);
    else if (p.w == 64) hipLaunchKernelGGL((rd_decide_signal_kernel<3 + msig::kExtraSlotsSubstitution, 4, 0>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((rd_decide_signal_kernel<3 + msig::kExtraSlotsSubstitution, 1, 0>), grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_signal_list(const SignalListParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.mode_hads || !p.cand_hads || !p.slot_modes || p.nb_qps < 1 || p.nb_qps > trquant::kMaxQps) return hipErrorInvalidValue;
    const long total = (long)p.nb_qps * p.N;
    const dim3 grid((unsigned)((total + kRdThreads - 1) / kRdThreads)), block(kRdThreads);
    if (p.w <= 8) hipLaunchKernelGGL((signal_list_kernel<8>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((signal_list_kernel<3>), grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_rd_candidates_slots(const RdCandidatesParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    const int g = rd_candidates_blocks_per_workgroup(p.w);
    const dim3 grid((unsigned)((p.N + g - 1) / g)), block(kRdThreads);
    const bool pic = p.patterns == nullptr;
    if (pic && (!p.pic.channels || !p.pic_targets || !p.pic.mask_w != !p.pic.mask_h)) return hipErrorInvalidValue;
    const bool masks = pic && p.pic.mask_w;           // masks per position: the MASKS instantiation (the scalar entries keep theirs)
    if (!p.cand_pred || !p.list_modes || !p.slot_pred || !p.slot_targets) return hipErrorInvalidValue;
    if (p.smoothing < 0 || p.smoothing > 2) return hipErrorInvalidValue;
#define PNN_RD_LAUNCH(W_, SMOOTH_) \
    if (masks) hipLaunchKernelGGL((rd_candidates_kernel<W_, true, SMOOTH_, true, false, true>), grid, block, 0, s, p); \
    else if (pic) hipLaunchKernelGGL((rd_candidates_kernel<W_, true, SMOOTH_, true>), grid, block, 0, s, p); \
    else hipLaunchKernelGGL((rd_candidates_kernel<W_, false, SMOOTH_, true>), grid, block, 0, s, p);
#define PNN_RD_LAUNCH_SMOOTH(W_) if (p.smoothing) { PNN_RD_LAUNCH(W_, true) } else { PNN_RD_LAUNCH(W_, false) }
    switch (p.w) {                                     // (width 64 writes each slot as its four quadrants, 32 x 32 blocks)
    case 4: PNN_RD_LAUNCH(4, false) break;
    case 8: PNN_RD_LAUNCH_SMOOTH(8) break;
    case 16: PNN_RD_LAUNCH_SMOOTH(16) break;
    case 32: PNN_RD_LAUNCH_SMOOTH(32) break;
    case 64: PNN_RD_LAUNCH(64, false) break;
    default: return hipErrorInvalidValue;
    }
#undef PNN_RD_LAUNCH_SMOOTH
#undef PNN_RD_LAUNCH
    return hipGetLastError();
}

hipError_t launch_rd_decide_signal(const RdDecideSignalParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.sse || !p.rate || !p.nonzero || !p.slot_modes || p.cbf_ctx < 0 || p.cbf_ctx > 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.N + kRdThreads - 1) / kRdThreads)), block(kRdThreads);
    if (p.w <= 8) hipLaunchKernelGGL((rd_decide_signal_kernel<8 + msig::kExtraSlots>), grid, block, 0, s, p);
    else if (p.w == 64) hipLaunchKernelGGL((rd_decide_signal_kernel<3 + msig::kExtraSlots, 4>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((rd_decide_signal_kernel<3 + msig::kExtraSlots>), grid, block, 0, s, p);
    return hipGetLastError();
}

int rd_candidates_blocks_per_workgroup(int w) { return w >= 32 ? 1 : 1024 / (w * w); }

hipError_t launch_rd_candidates(const RdCandidatesParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    const int g = rd_candidates_blocks_per_workgroup(p.w);
    const dim3 grid((unsigned)((p.N + g - 1) / g)), block(kRdThreads);
    const bool pic = p.patterns == nullptr;
    if (pic && (!p.pic.channels || !p.pic_targets || !p.pic.mask_w != !p.pic.mask_h)) return hipErrorInvalidValue;
    const bool masks = pic && p.pic.mask_w;           // masks per position: the MASKS instantiation (the scalar entries keep theirs)
    if (!p.cand_pred || !p.list_modes || !p.cand_modes || !p.slot_pred || !p.slot_targets) return hipErrorInvalidValue;
    if (p.smoothing < 0 || p.smoothing > 2) return hipErrorInvalidValue;
#define PNN_RD_LAUNCH(W_, SMOOTH_) \
    if (masks) hipLaunchKernelGGL((rd_candidates_kernel<W_, true, SMOOTH_, false, false, true>), grid, block, 0, s, p); \
    else if (pic) hipLaunchKernelGGL((rd_candidates_kernel<W_, true, SMOOTH_>), grid, block, 0, s, p); \
    else hipLaunchKernelGGL((rd_candidates_kernel<W_, false, SMOOTH_>), grid, block, 0, s, p);
#define PNN_RD_LAUNCH_SMOOTH(W_) if (p.smoothing) { PNN_RD_LAUNCH(W_, true) } else { PNN_RD_LAUNCH(W_, false) }
    switch (p.w) {                                     // at w = 4 and 64 no mode smooths: the one instantiation for every `smoothing`
    case 4: PNN_RD_LAUNCH(4, false) break;
    case 8: PNN_RD_LAUNCH_SMOOTH(8) break;
    case 16: PNN_RD_LAUNCH_SMOOTH(16) break;
    case 32: PNN_RD_LAUNCH_SMOOTH(32) break;
    case 64: PNN_RD_LAUNCH(64, false) break;
    default: return hipErrorInvalidValue;
    }
#undef PNN_RD_LAUNCH_SMOOTH
#undef PNN_RD_LAUNCH
    return hipGetLastError();
}

hipError_t launch_rd_decide(const RdDecideParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    if (!p.sse || !p.rate || !p.cand_modes || p.nb_qps < 1 || p.nb_qps > trquant::kMaxQps) return hipErrorInvalidValue;
    const long total = (long)p.nb_qps * p.N;
    const dim3 grid((unsigned)((total + kRdThreads - 1) / kRdThreads)), block(kRdThreads);
    if (p.w <= 8) hipLaunchKernelGGL((rd_decide_kernel<9>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((rd_decide_kernel<4>), grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_hevc_best_mode(const HevcBestModeParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    const int rows_per_lane = p.w <= 8 ? p.w : 4, blocks_per_wg = 64 / (p.w / rows_per_lane);
    const dim3 grid((unsigned)((p.N + blocks_per_wg - 1) / blocks_per_wg)), block(kThreads);
    const bool pic = p.patterns == nullptr;
    if (pic && (!p.pic.channels || !p.pic_targets || !p.pic.mask_w != !p.pic.mask_h)) return hipErrorInvalidValue;
    const bool masks = pic && p.pic.mask_w;           // masks per position: the MASKS instantiation (the scalar entries keep theirs)
    if (p.smoothing < 0 || p.smoothing > 2) return hipErrorInvalidValue;
#define PNN_HEVC_LAUNCH(W_, SMOOTH_) \
    if (masks) hipLaunchKernelGGL((hevc_best_mode_kernel<W_, true, SMOOTH_, true>), grid, block, 0, s, p); \
    else if (pic) hipLaunchKernelGGL((hevc_best_mode_kernel<W_, true, SMOOTH_>), grid, block, 0, s, p); \
    else hipLaunchKernelGGL((hevc_best_mode_kernel<W_, false, SMOOTH_>), grid, block, 0, s, p);
#define PNN_HEVC_LAUNCH_SMOOTH(W_) if (p.smoothing) { PNN_HEVC_LAUNCH(W_, true) } else { PNN_HEVC_LAUNCH(W_, false) }
    switch (p.w) {                                     // at w = 4 and 64 no mode smooths: the one instantiation for every `smoothing`
    case 4: PNN_HEVC_LAUNCH(4, false) break;
    case 8: PNN_HEVC_LAUNCH_SMOOTH(8) break;
    case 16: PNN_HEVC_LAUNCH_SMOOTH(16) break;
    case 32: PNN_HEVC_LAUNCH_SMOOTH(32) break;
    case 64: PNN_HEVC_LAUNCH(64, false) break;
    default: return hipErrorInvalidValue;
    }
#undef PNN_HEVC_LAUNCH_SMOOTH
#undef PNN_HEVC_LAUNCH
    return hipGetLastError();
}

hipError_t launch_hevc_mode_hads(const HevcModeHadsParams& p, hipStream_t s)
{
    if (p.N <= 0) return hipSuccess;
    const int t = p.w == 4 ? 4 : 8, blocks_per_wg = 64 / ((p.w / t) * (p.w / t));
    const dim3 grid((unsigned)((p.N + blocks_per_wg - 1) / blocks_per_wg)), block(kThreads);
    const bool pic = p.patterns == nullptr;
    if (pic && (!p.pic.channels || !p.pic_targets || !p.pic.mask_w != !p.pic.mask_h)) return hipErrorInvalidValue;
    const bool masks = pic && p.pic.mask_w;           // masks per position: the MASKS instantiation (the scalar entries keep theirs)
    if (p.smoothing < 0 || p.smoothing > 2) return hipErrorInvalidValue;
#define PNN_HADS_LAUNCH(W_, SMOOTH_) \
    if (masks) hipLaunchKernelGGL((hevc_mode_hads_kernel<W_, true, SMOOTH_, true>), grid, block, 0, s, p); \
    else if (pic) hipLaunchKernelGGL((hevc_mode_hads_kernel<W_, true, SMOOTH_>), grid, block, 0, s, p); \
    else hipLaunchKernelGGL((hevc_mode_hads_kernel<W_, false, SMOOTH_>), grid, block, 0, s, p);
#define PNN_HADS_LAUNCH_SMOOTH(W_) if (p.smoothing) { PNN_HADS_LAUNCH(W_, true) } else { PNN_HADS_LAUNCH(W_, false) }
    switch (p.w) {
    case 4: PNN_HADS_LAUNCH(4, false) break;
    case 8: PNN_HADS_LAUNCH_SMOOTH(8) break;
    case 16: PNN_HADS_LAUNCH_SMOOTH(16) break;
    case 32: PNN_HADS_LAUNCH_SMOOTH(32) break;
    case 64: PNN_HADS_LAUNCH(64, false) break;
    default: return hipErrorInvalidValue;
    }
#undef PNN_HADS_LAUNCH_SMOOTH
#undef PNN_HADS_LAUNCH
    return hipGetLastError();
}

}  // namespace pnn
