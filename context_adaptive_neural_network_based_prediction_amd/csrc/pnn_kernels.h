// Internal launch interface between the C-ABI layer (pnn_abi.cpp) and the gfx950 kernels
// (pnn_kernels.hip).  Not part of the public boundary -- see include/pnn_hip.h for that.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "pnn_cabac_tables.h"
#include "pnn_cu_tree.h"
#include "pnn_mode_signal.h"
#include "pnn_rdoq.h"
#include "pnn_trquant_tables.h"
#include "pnn_tskip.h"

namespace pnn {

// see signal_done, pnn_device_common.h.  per_wg = 1 (round 6, fc_out_f32_chain_kernel): workgroup g raises host_flag[g] by itself -- no
// counter, no second fence; the host waits for all of the launch's flags
struct DoneSignal { unsigned* counter; unsigned* host_flag; unsigned seq, per_wg; };

// Per-launch timing (pnn_abi.cpp, option time_launches): when set, the GEMM launchers attach these events to the kernel
// itself (hipExtLaunchKernelGGL), so that their elapsed time is the kernel's own begin -> end -- what rocprofv3
// reports -- instead of the record-to-record time of two hipEventRecord calls around the launch (~4 us more).
struct LaunchEvents { hipEvent_t start, stop; };
extern thread_local const LaunchEvents* g_launch_events;
template <typename K, typename... A>
inline void pnn_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args)
{
    if (g_launch_events) hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)lds, s, g_launch_events->start, g_launch_events->stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

// What the launch rules need to know about the CURRENT device (hipGetDevice), read once per device from hipDeviceProp: compute units
// and LDS bytes per CU (MI355X: 256 and 160 KiB; a partitioned GPU -- CPX / DPX -- or another SKU shows other numbers).
struct DeviceInfo { int cus = 256; size_t lds = (size_t)160 << 10; int dev = -1; };
const DeviceInfo& device_info();

hipError_t probe_queue_shared(hipStream_t a, hipStream_t b, bool* shared);   // pnn_small.hip: do two streams sit on one hardware queue?

constexpr int kMaxTaps = 32;
constexpr int kMaxClasses = 4;

// One "tap GEMM": Y[pix(m)][n] = act( sum_{t in class} sum_{ci} X[b, i*a+dy[t], j*a+dx[t], ci] * W[t][ci][n] + bias[n] )
// with m = (b, i, j) over a SH x SW sub-grid per image and the output pixel (i*os+py, j*os+px).
//   forward conv, stride s : one class, a = s, os = 1, dy = ky - pad_before        
//   transposed conv, s = 1 : one class, a = 1, os = 1, dy = pad_before - ky         (Appendix B.3)
//   transposed conv, s = 2 : four output-parity classes, a = 1, os = 2, dy = (py + 1 - ky) / 2
//   fully-connected layer  : one tap, 1x1 "image", Cin = K                            (components.py:169-176)
// Weights are pre-packed per 16-deep K chunk as [chunk][q = 4][Npad][4] floats (k = 16*chunk + 4*q + e),
// the order in which one 16x16x4 f32 MFMA lane group consumes them.
struct TbDev;
struct TapGemmParams {
    const float* X;    // f32 activations, or the hi f16 plane for the split-precision kernel
    const void* Xlo;   // lo f16 plane (split-precision kernel only)
    const void* zero;  // >= 256 bytes of zeros (ring kernel: source of padding / out-of-range pieces)
    // ring kernel, fused next fully-connected layer (<= 64 outputs): its split-packed weights, their Npad, the number of
    // packed 16-deep chunks, and the partial-product buffer [column tiles][M][64] (see pnn_gemm_ring.hip)
    // (the image kernel never reads these; when it applies a net's LAST layer to its output tile -- k1 != 0 below, see
    // pnn_convimg_sp.hip -- that layer's weights [k1][k1][Cout], and the net's outputs (float and / or HM epilogue) live in the same bytes)
    union {
        struct { const float* W2p; int Npad2; int K2chunks; float* part; };
        struct { const float* W1; float* Y1; int32_t* Yi1; };
        // tapgemm_f32_small_kernel, a K-segmented layer (nseg > 1) whose planes are added up INSIDE the launch (seg_cnt != NULL): the
        // workgroup that is the last of a tile's nseg to arrive (a counter per tile in seg_cnt, zero between launches) adds the planes in
        // order, + bias, activation, and stores the layer's real output seg_Y; `bias` and `act` are then the layer's own, Y the planes
        struct { unsigned* seg_cnt; float* seg_Y; };
    };
    // convimg kernel, fused FIRST convolution of a branch (Cin = 1 -> this layer's Cin channels, stride s0, kernel k0 x k0,
    // SAME padding with pad0 before, LeakyReLU): X0 != NULL makes the kernel compute its input maps from the raw f32
    // context X0 [images][IH * s0][IW * s0] instead of reading them from X (see pnn_convimg_sp.hip)
    // (The ring kernel never reads these fields; its position-major launches keep their position order in the same bytes --
    // pos_order below -- so that the argument block stays at 8 lines of 64 bytes: every line is a round trip at kernel entry,
    // and a ninth cost the FC 8x8 pass 0.7 %.)
    union {
        struct {
            const float* X0; const float* W0; const float* B0; int s0, k0, pad0;
            const float* W0sp; float scale0; int Npad0;   // the first convolution's taps x channels matrix in the split pack (FirstConv, pnn_device_common.h)
            // ... and, when plane0 != NULL, the context gather too (extraction_context.cpp:3-208): X0 is not read; image i's raw context
            // comes straight from the picture plane through TB descriptor tbs0[i] -- branch0 = 0: the above portion (rows y - w ..
            // y - 1, columns x - w .. x + 2w - 1, masked per unit0-pixel unit), 1: the left portion (rows y .. y + 2w - 1, columns
            // x - w .. x - 1, the first left_units units) --, Pel (pel0 bytes) -> float, minus `mean`
            const void* plane0; const void* tbs0; int pel0, branch0, unit0, w0;
        };
        // ring kernel, position-major tiles: the positions by decreasing number of in-image taps, one byte each (grids of <= 64
        // positions; larger grids: rank = position)
        unsigned pos_order[16];
    };
    const float* Wp;
    const float* bias;
    float* Y;          // float output (may be null when Yi is set)
    int32_t* Yi;       // optional fused HM epilogue: (int) round(clamp(v + mean, 0, 255))
    void* Yhi;         // optional split-f16 output planes (split-precision kernel only)
    void* Ylo;
    int* range_flag;   // raised (host-visible int) when a split-f16 output leaves the f16 range, see pnn_device_common.h
    float out_scale;   // split-precision kernel: exact power of two undoing the weight pre-scale
    unsigned x_bytes;  // size of X in bytes (< 2^31): bound of the activation buffer descriptor
    int M, SH, SW;
    int IH, IW, Cin, a;
    int OH, OW, Cout, os;
    int Npad;
    int act;
    float mean;
    int ncls;
    int tap_begin[kMaxClasses + 1];
    int chunk_begin[kMaxClasses + 1];   // first packed 16-deep chunk of each class (classes padded to kChunkPad)
    int py[kMaxClasses], px[kMaxClasses];
    int tap[kMaxTaps];   // (dy << 16) | (dx & 0xffff): one scalar load per tap
    // ring kernel, position-major tiles (set by launch_tapgemm_ring, see pnn_gemm_ring.hip): pm_groups > 0 = a workgroup's BM
    // rows are BM BLOCKS at ONE position of the SH x SW grid, so a tap that falls outside the image does so for the whole
    // tile and is skipped; pm_groups = number of block groups, nblk = number of blocks; the position order: pos_order above
    // (tapgemm_f32_small kernels, in nblk's bytes: chain_io bit 0 = the activations X are in CHAIN ORDER -- NHWC with every 16-channel
    // group permuted so that the four values a lane group of the 16x16x4 chain multiplies are contiguous, pnn_gemm_f32_small.hip --,
    // bit 1 = write the output that way; set by the pass for tensors whose producer AND consumer are those kernels)
    int pm_groups; union { int nblk; int chain_io; };
    // image kernel, fused last layer (Cout == 64 -> 1 transposed convolution, kernel k1, stride s1, pad1 before, bias1): k1 != 0
    float bias1; int k1, s1, pad1;
    // tapgemm_f32_kernel, K segments (nseg > 1, see GemmLayer::nseg): grid z = class * nseg + segment; a workgroup walks only its
    // segment's share of the class's taps and stores its sums at Y + segment * seg_stride (floats) -- the caller passes a zero
    // bias and act = 0 and finishes with launch_seg_reduce
    // ONE-TAP layers (FC, round 6; GemmLayer::fc_seg_chunks): segments of seg_chunks 16-deep chunks of the tap, always folded inside the
    // workgroup (seg_seq = 1 in tapgemm_f32_kernel; fcseg_f32_small_kernel runs them as parallel chains of one workgroup) -- seg_stride's bytes
    int nseg; union { unsigned seg_stride; unsigned seg_chunks; };
    // seg_seq = 1: the segments one after the other inside each workgroup instead (grid z = class), folded into a running total in
    // the same order -- same bits, no partial planes, no second launch; the caller passes the real Y, bias and act
    int seg_seq;
    // tapgemm_f32_kernel: the launch's tiles (set by launch_f32; the kernel's grid is 1-D over them, or smaller: persistent workgroups)
    int grid_x, grid_y, grid_z;
    // tapgemm_f32 launches: persist > 0 = persistent workgroups, that many per CU (see launch_f32); a PAIRED launch (launch_f32_pair,
    // never persistent) reads the same bytes as pair_occ: 0 = ask the runtime how many of its workgroups a CU holds, N > 0 = take N for the answer
    union { int persist; int pair_occ; };
};
static_assert(sizeof(TapGemmParams) <= 512, "the argument block of the tap-GEMM kernels: 8 lines of 64 bytes");
inline int pack_tap(int dy, int dx) { return (int)(((unsigned)dy << 16) | ((unsigned)dx & 0xffffu)); }

constexpr int kChunkPad = 4;   // packed weights: every class is zero-padded to a multiple of 4 chunks
constexpr int kSegDepth = 1600, kSegMinDepth = 2304;   // K segments of the exact-f32 summation order, see finish_gemm_layer (pnn_model.cpp)
constexpr int kFcSegChunks = 20;                       // ... of a one-tap (FC) layer deeper than this many 16-deep chunks: segments of 320 inputs
// a tile configuration of one of the tap-GEMM kernel families (mf: rows of the MFMA shape; pair: tapgemm_f32 only, see PairTile)
struct TileCfg { int rt, nt, kc, mf, wm = 4, d = 2, pair = 0; };
int tapgemm_sp_num_cfgs();
TileCfg tapgemm_sp_cfg(int idx);
hipError_t launch_tapgemm_sp(const TapGemmParams& p, int idx, hipStream_t s);   // 3 x f16 MFMA, f32-class accuracy
int tapgemm_ring_num_cfgs();
TileCfg tapgemm_ring_cfg(int idx);
size_t tapgemm_ring_lds_bytes(const TileCfg& t);
bool tapgemm_ring_can_fuse(int idx);
// Y[i] = act(bias[i % Cout] + ((part[0][i] + part[1][i]) + ... + part[nseg - 1][i])), i < n (n and Cout multiples of 4): the K segments of
// a tapgemm_f32 layer in their canonical order
hipError_t launch_seg_reduce(const float* part, int nseg, size_t n, int Cout, const float* bias, int act, float* Y, hipStream_t s);
hipError_t launch_fuse_reduce(const float* part, int ntiles, int M, int N2, const float* bias, float scale, float mean, float* Y, int32_t* Yi,
                              hipStream_t s, const DoneSignal& done = DoneSignal{nullptr, nullptr, 0, 0});
hipError_t launch_tapgemm_ring(const TapGemmParams& p, int idx, hipStream_t s);     // LDS-DMA ring pipeline (pnn_gemm_ring.hip)
// Position-major tiles (a workgroup's BM rows = BM blocks at ONE position of the SH x SW grid: the taps that only meet padding are
// skipped): whether a launch of tile BM x BN, KC chunks per stage, `lds` bytes per workgroup takes them, in how many block
// groups, and the position order (pnn_gemm_ring.hip; shared by the ring kernel and tapgemm_f32_kernel).  p.pm_groups on entry:
// -1 never, 1 whenever possible, 0 by the planner's list-scheduling model.
struct PmPlan { bool use = false; int groups = 0; unsigned order[16] = {}; double live_frac = 1.0; };   // live_frac: in-image taps / all taps, over the positions
// Fraction of a tap GEMM's algorithmic multiply-adds that the LAST launch of this thread issued: 1 for block-major tiles, the plan's
// live_frac for position-major ones (the skipped taps only meet SAME padding) -- bench.py's executed-MFMA fractions
extern thread_local double g_last_issued_frac;
const PmPlan& position_major_plan(const TapGemmParams& p, int BM, int BN, int KC, size_t lds, double l2_mb = 4.5);
int convimg_sp_num_cfgs();
TileCfg convimg_sp_cfg(int idx);
size_t convimg_sp_lds_bytes(const TapGemmParams& p, const TileCfg& t, int G);
bool convimg_sp_can_fuse_first(const TapGemmParams& p, const TileCfg& t, int G, int s0, int k0);   // the raw context tiles fit the weight staging area
struct TConv1Params;
bool convimg_sp_can_fuse_last(const TapGemmParams& p, const TileCfg& t, int G, const TConv1Params& last);   // the net's last layer on the output tile (k1 != 0)
hipError_t launch_convimg_sp(const TapGemmParams& p, int idx, int G, hipStream_t s);   // G images per workgroup, resident in LDS
hipError_t launch_split(const float* x, long n, void* hi, void* lo, int* range_flag, hipStream_t s);
// Small-M split-precision tap GEMM (pnn_gemm_small.hip): one wave per 32 x 32 output tile, same per-output summation
// order as the three big-tile kernels.  a_is_f32: p.X holds plain f32 rows (split in registers); seg_chunks > 0: K-segment
// mode of an FC output layer (<= 64 outputs), raw partials to p.part[segment][M][64] for launch_fuse_reduce.
long tapgemm_small_tiles(const TapGemmParams& p);
// host_input (optional, with a_is_f32): the same rows in HOST memory; when they fit they travel inside the argument block
hipError_t launch_tapgemm_small(const TapGemmParams& p, bool a_is_f32, int seg_chunks, hipStream_t s, const float* host_input = nullptr);
hipError_t launch_tapgemm_small_pair(const TapGemmParams& a, const TapGemmParams& b, hipStream_t s);   // two independent layers, one launch
// Exact-f32 tap GEMM on v_mfma_f32_32x32x2_f32, one wave per SIMD (pnn_gemm_f32.hip): the canonical f32 summation order.
// fuse: apply the output layer p.W2p (f32 pack, <= 64 outputs) to the activated tile, partial sums to p.part[column tile][M][64]
int tapgemm_f32_num_cfgs();
TileCfg tapgemm_f32_cfg(int idx);
size_t tapgemm_f32_lds_bytes(const TileCfg& t, bool fuse, bool row_out = false);   // row_out: an FC layer's f32 output leaves through an LDS tile
bool tapgemm_f32_can_fuse(int idx);
int tapgemm_f32_regs(int idx);   // registers per lane of tile idx (residency estimate of choose_cfg_f32)
// PAIRED tiles of tapgemm_f32_kernel (TileCfg::pair; one-tap layers without a fused output layer): the 128 x 160 share of a CU as TWO
// workgroups, a WIDE one of 128 x 96 (columns [160 g, 160 g + 96) of column group g) and a NARROW one of 128 x 64 (the 64 behind),
// resident together -- two waves per SIMD of unequal length, so that the narrow tile's epilogue falls under the wide tile's MFMAs.
// Workgroup w of the 1-D grid (kPairGridStep-aligned, see f32_pair_grid): the hardware deals workgroups to the 8 XCDs in turn, so
// slot k = w / 8 counts the workgroups of XCD w % 8 in dispatch order.  Slots 2 j and 2 j + 1 are the two tiles of ONE pair (they share
// the row tile: the second fetch of the activation panel hits the CU's cache), and which of them is the wide one alternates every
// 32 slots -- whether an XCD's dispatcher fills a CU before it goes to the next or deals its 32 CUs in turn, a CU gets one of each.
// group >= the launch's column groups: no tile (the grid's padding).
struct PairTile { int bx, group, narrow; };
constexpr int kPairGridStep = 16, kPairWide = 96, kPairNarrow = 64;
__host__ __device__ inline PairTile f32_pair_tile(int w, int gx)
{
    const int k = w >> 3, q = (k >> 1) * 8 + (w & 7);
    return PairTile{q % gx, q / gx, (k ^ (k >> 5)) & 1};
}
inline void f32_pair_grid(int M, int Cout, int* gx, int* groups, int* nwg)
{
    *gx = (M + 127) / 128;
    *groups = (Cout + kPairWide + kPairNarrow - 1) / (kPairWide + kPairNarrow);
    *nwg = (*gx * *groups + 7) / 8 * kPairGridStep;
}
// what the last launch_tapgemm_f32 of this thread did with a paired tile: 0 = not a paired tile, 1 = launched the pair, 2 = the pair does
// not fit a CU together and the one 128 x 160 tile ran instead
extern thread_local int g_last_pair_mode;
hipError_t launch_tapgemm_f32(const TapGemmParams& p, int idx, bool fuse, hipStream_t s);
// Small-M form of the same order on v_mfma_f32_16x16x4_f32 (pnn_gemm_f32_small.hip): one wave per 16 x 16 tile, K segments as grid z;
// host_input (optional, FC layers): the same rows in HOST memory; when they fit they travel inside the argument block
long tapgemm_f32_small_tiles(const TapGemmParams& p);
hipError_t launch_tapgemm_f32_small(const TapGemmParams& p, hipStream_t s, const float* host_input = nullptr, int deep_mode = 1);   // deep_mode: pnn_ctx::opt_f32_small_deep
hipError_t launch_tapgemm_f32_small_pair(const TapGemmParams& a, const TapGemmParams& b, hipStream_t s, int deep_mode = 1);   // two independent layers, one launch
// A K-segmented one-tap (FC) layer at small M: one workgroup per 16 x 16 output tile runs the layer's <= 4 segments as 4 chains side by
// side and adds them up in order (p.nseg, p.seg_chunks; the bits of tapgemm_f32_kernel's seg_seq form)
long fcseg_f32_small_tiles(const TapGemmParams& p);
bool fcseg_f32_small_fits(const TapGemmParams& p);
hipError_t launch_fcseg_f32_small(const TapGemmParams& p, hipStream_t s);
// the same output layer from stored activations p.X [M][Cin], in the fused kernel's order: p.part[segment of 160][M][64]
hipError_t launch_fc_out_f32(const TapGemmParams& p, hipStream_t s, int* segments);
// ... and, for small M, the same segments AND their reduction (+ bias, HM epilogue) in one launch: fuse_reduce_kernel's bits
bool fc_out_f32_small_fits(const TapGemmParams& p);
hipError_t launch_fc_out_f32_small(const TapGemmParams& p, hipStream_t s, const DoneSignal& done = DoneSignal{nullptr, nullptr, 0, 0});

// Cin == 1 forward convolution (first layer of each branch): direct VALU kernel.
struct Conv1Params {
    const float* X; const float* W; const float* bias; float* Y;
    int B, IH, IW, s, k, pad, OH, OW, Cout;
    int split;   // 1: write Y as split activations [pixel][Cout/16][hi 16 x f16 | lo 16 x f16] for the split-precision GEMM
    int band_rows;   // output rows per workgroup (set by the launcher)
    int* range_flag; // split output only: raised when a value leaves the f16 range
    const float* Wsp; float out_scale; int npad;   // split output: the taps x channels matrix in the split pack of the GEMM layers, its inverse pre-scale, its Npad
    // X == NULL: the context gather fused in (extraction_context.cpp:3-208) -- image b's raw context comes straight from the picture
    // plane through TB descriptor tbs[b] (branch 0: the above portion w x 3w, 1: the left portion 2w x w; unit-pixel availability
    // units), Pel (pel_bytes) -> float, minus mean: the values gather_f32x4_kernel would have written
    const void* plane; const TbDev* tbs; int pel_bytes, unit, w, branch; float mean;
    int chain;       // f32 output only: 1 = write it in chain order (its consumer is a small exact-f32 kernel, pnn_gemm_f32_small.hip)
    int mfma;        // f32 output only: 1 = the taps' chain on the f32 matrix instruction instead of the VALU (same bits; set by the launcher)
};
hipError_t launch_conv_cin1(const Conv1Params& p, hipStream_t s);
hipError_t launch_conv_cin1_pair(const Conv1Params& a, const Conv1Params& b, hipStream_t s);   // both branches in one launch (same batch, same kernel size)

// Cout == 1 transposed convolution (last merger layer), optional fused HM epilogue.
struct TConv1Params {
    const float* X; const float* W; /* [k][k][Cin] */ float bias; float* Y; int32_t* Yi;
    int B, IH, IW, Cin, s, k, pad; float mean;
    int ni;   // images per workgroup (set by the launcher)
    DoneSignal done;   // host_flag != NULL: this is the last kernel of a host call, see signal_done (pnn_device_common.h)
};
hipError_t launch_tconv_cout1(const TConv1Params& p, hipStream_t s);

// Channel-wise fully-connected merger + LeakyReLU (Appendix B.4). Wp is [p = 80][j = 16][C].
struct MergerParams {
    const float* A; const float* L; const float* Wp; const float* bias /* [j][C] */; float* Y;
    int B, C, na, nl, nout;
    int split;   // 1: write Y in the split f16 activation layout
    int* range_flag; // split output only: raised when a value leaves the f16 range
    int chain;       // f32 output only: 1 = write it in chain order (its consumer is a small exact-f32 kernel, pnn_gemm_f32_small.hip)
};
hipError_t launch_merger(const MergerParams& p, hipStream_t s);

// A small layer run as the TAIL of the small exact-f32 GEMM launch in front of it (pnn_gemm_f32_small.hip, round 6): kind 1 = the
// merger per (block, channel group) behind the pair launch of the branches' last layers, kind 2 = the last transposed convolution
// (with the HM epilogue and one completion flag per block, DoneSignal::per_wg) per block behind the last GEMM of the transposed
// stack.  cnt: one zeroed counter per instance (kind 1: blocks x C / 16, kind 2: blocks); the launch leaves them zero.
struct SmallTail { int kind; unsigned* cnt; MergerParams m; TConv1Params t; };
bool f32_small_cout1_tail_ok(const TapGemmParams& p, const TConv1Params& t);
bool f32_small_merger_tail_ok(const TapGemmParams& a, const TapGemmParams& b, const MergerParams& m);
hipError_t launch_tapgemm_f32_small_tail(const TapGemmParams& p, const SmallTail& t, hipStream_t s, int deep_mode = 1);
hipError_t launch_tapgemm_f32_small_pair_tail(const TapGemmParams& a, const TapGemmParams& b, const SmallTail& t, hipStream_t s, int deep_mode = 1);

// L-shaped context gather (extraction_context.cpp:3-208) over a descriptor array.
struct TbDev {           // mirrors pnn_tb_dev of include/pnn_hip.h
    int64_t origin;      // element index of the TB's top-left pixel from the plane base
    int32_t stride;      // row stride in elements
    uint32_t above_mask; // bit u = above/above-right unit u (left to right) available
    int32_t left_units;  // number of available left/below-left units, counted from the top
    int32_t reserved;
};
struct GatherParams {
    const void* plane; int pel_bytes; const TbDev* tbs; int N; int w; int unit; float mean;
    float* above; float* left; long pitch_above; long pitch_left;
    int split;   // 1 (FC layout only, one [5w^2] row per TB): write the split f16 activation layout instead of f32
};
hipError_t launch_gather(const GatherParams& p, hipStream_t s);

// (f4) HM distortion (HADs or SAD) of predicted blocks [N][w][w] against the original picture at the descriptors' positions.
struct BlockCostParams {
    const void* org_plane; int pel_bytes; const TbDev* tbs; int N; int w; const int32_t* pred; int hadamard; uint32_t* cost;
};
hipError_t launch_block_cost(const BlockCostParams& p, hipStream_t s);

// Blocks of the evaluator's pictures (pnn_score_pictures_device): uint8 pictures [images][H][W], context corners (rows[pos], cols[pos])
// of `positions` positions, block b = image * positions + pos.  The block's 3w x 3w context square starts at its corner, its w x w
// target at (row + w, col + w).  The caller has checked that every square lies inside the picture.
// mask_w / mask_h: NULL (every block under the call's scalar masks) or uint8 [positions], the masks of the blocks at each POSITION, in
// samples and checked by the caller; both or none.
struct PictureBlocks {
    const uint8_t* channels; int H, W; const int32_t* rows; const int32_t* cols; int positions;
    const uint8_t* mask_w; const uint8_t* mask_h;
};

// HEVC best intra mode (pnn_hevc_intra.hip): N intra patterns [N][ph][pw] (first row and column used) and targets [N][w][w], all uint8;
// any of the four outputs may be NULL.  With patterns == NULL the reference samples and the targets of block b come from `pic`
// instead: the pattern's first row and column start at (row + w - 1, col + w - 1), ph and pw say how much of them is not masked.
// The picture form has two planes of equal geometry: the reference samples are read from pic.channels (the context plane -- the
// decoded picture of a pair), the targets from pic_targets (the original; the same pointer for single pictures).
// smoothing: HM's reference-sample smoothing (include/pnn_hip.h), 0 none, 1 the [1 2 1] filter, 2 also the strong filter at w = 32; 1
// and 2 launch the SMOOTH instantiations at w = 8, 16, 32 (no mode smooths at 4 and 64), where "strong allowed" is a runtime branch.
struct HevcBestModeParams {
    const uint8_t* patterns; int ph; int pw; const uint8_t* targets; int N; int w;
    uint8_t* best_mode; uint32_t* best_sse; uint8_t* best_pred; uint32_t* mode_sse;
    PictureBlocks pic;
    const uint8_t* pic_targets;   // behind the dense form's arguments, which keep their offsets
    int smoothing;
};
hipError_t launch_hevc_best_mode(const HevcBestModeParams& p, hipStream_t s);

// First-pass ranking (pnn_hevc_intra.hip): the same inputs in the same two forms, plus an optional candidate prediction cand_pred
// [N][w][w] uint8.  Per block the Hadamard cost (TComRdCost::xGetHADs, 8-bit) of the 35 predictions and of the candidate (index 35)
// against the target, and HM's sorted candidate list of K = hevc_first_pass_list_size(w) entries (ascending cost, the lower index
// first among equal costs).  Outputs, each NULL or per block: mode_hads [N][35], cand_hads [N], list_modes [N][K], list_costs [N][K].
struct HevcModeHadsParams {
    const uint8_t* patterns; int ph; int pw; const uint8_t* targets; int N; int w;
    const uint8_t* cand_pred; uint32_t* mode_hads; uint32_t* cand_hads; uint8_t* list_modes; uint32_t* list_costs;
    PictureBlocks pic;
    const uint8_t* pic_targets;
    int smoothing;
};
inline int hevc_first_pass_list_size(int w) { return w <= 8 ? 8 : 3; }   // g_aucIntraModeNumFast_UseMPM for w = 4 .. 64
hipError_t launch_hevc_mode_hads(const HevcModeHadsParams& p, hipStream_t s);

// Candidates of HM's second intra pass (pnn_hevc_intra.hip): the same inputs in the same two forms, the
// candidate's predictions cand_pred [N][w][w] and the first-pass list list_modes [N][K] a launch_hevc_mode_hads call left on the
// device.  Per block K + 1 slots: the list's modes in order, then 35 if the list lacks it, else 255 (unused).  Outputs, all required:
// cand_modes [N][K + 1], slot_pred [N][K + 1][w][w] (a mode's prediction, cand_pred for 35, the target for 255: a zero residual) and
// slot_targets, the block's target once per slot -- what launch_trquant codes as N (K + 1) blocks with cand_modes as its mode array.
struct RdCandidatesParams {
    const uint8_t* patterns; int ph; int pw; const uint8_t* targets; int N; int w;
    const uint8_t* cand_pred; const uint8_t* list_modes; uint8_t* cand_modes; uint8_t* slot_pred; uint8_t* slot_targets;
    PictureBlocks pic;
    const uint8_t* pic_targets;
    int smoothing;
};
constexpr int kRdUnusedSlot = 255;                 // cand_modes of a slot that holds no candidate
int rd_candidates_blocks_per_workgroup(int w);
hipError_t launch_rd_candidates(const RdCandidatesParams& p, hipStream_t s);
// The decision: J = D + lambda R per (QP, block, slot) -- D = sse [nb_qps][N (K + 1)], R = rate >> 15 of rate [nb_qps][N (K + 1)], one
// IEEE multiply and one IEEE add in double, lambda[qi] as the host computed it -- +inf in an unused slot, and the least J over the
// slots in order under a strict <.  Outputs, each NULL or: cand_costs [nb_qps][N][K + 1]; best_* [nb_qps][N] (mode and slot 255, cost
// +inf, sse and rate 0 where no slot is below +inf).
struct RdDecideParams {
    const uint32_t* sse; const uint64_t* rate; const uint8_t* cand_modes; int N; int w; int nb_qps; double lambda[trquant::kMaxQps];
    double* cand_costs; uint8_t* best_mode; uint8_t* best_slot; double* best_cost; uint32_t* best_sse; uint64_t* best_rate;
};
hipError_t launch_rd_decide(const RdDecideParams& p, hipStream_t s);

// The second pass with mode signalling (pnn_hevc_intra.hip; the definition is pnn_mode_signal.h).
// The first pass with HM's mode-bit term: mode_hads [N][35] and cand_hads [N] as launch_hevc_mode_hads left them, left / above NULL
// (no neighbour) or uint8 [N] (0 .. 35, 255), per QP the four contexts' bits and sqrt(lambda), made on the host.  Outputs: slot_modes
// [nb_qps][N][K + 3] (the list, the missing MPMs, 35; 255 behind them), list_costs NULL or double [nb_qps][N][K].
struct SignalListParams {
    const uint32_t* mode_hads; const uint32_t* cand_hads; const uint8_t* left; const uint8_t* above; int N; int w; int nb_qps;
    msig::FlagBits bits[trquant::kMaxQps]; double sqrt_lambda[trquant::kMaxQps];
    double* list_costs; uint8_t* slot_modes;
};
hipError_t launch_signal_list(const SignalListParams& p, hipStream_t s);
// launch_rd_candidates with list_modes = the slot modes of one QP, [N][K + 3]: they are predicted as they stand; cand_modes is not
// written.  At width 64 slot_pred and slot_targets leave quadrant-major: [N][K + 3][4 quadrants][32][32].
hipError_t launch_rd_candidates_slots(const RdCandidatesParams& p, hipStream_t s);
// The decision of ONE QP over its N (K + 3) slots: sse, rate and nonzero [N (K + 3)] ([N (K + 3)][4] at width 64, per quadrant) of a
// launch_trquant call with that one QP,
// J = D + lambda ((mode bits + cbf bin + rate) >> 15).  Outputs, each NULL or: cand_costs [N][K + 3]; best_* and best_side_rate [N].
struct RdDecideSignalParams {
    const uint32_t* sse; const uint64_t* rate; const uint32_t* nonzero; const uint8_t* slot_modes; const uint8_t* left; const uint8_t* above;
    int N; int w; int cbf_ctx; double lambda; msig::FlagBits bits;
    double* cand_costs; uint8_t* best_mode; uint8_t* best_slot; double* best_cost; uint32_t* best_sse; uint64_t* best_rate;
    uint64_t* best_side_rate;
};
hipError_t launch_rd_decide_signal(const RdDecideSignalParams& p, hipStream_t s);
// The substitution codec's forms of the three (msig::list_and_slots_substitution): K + 2 slots wherever the ones
// above have K + 3, HM's 35 modes with mode 18's Hadamard cost and prediction the candidate's, no flag bin in the mode bits.
hipError_t launch_substitution_list(const SignalListParams& p, hipStream_t s);
hipError_t launch_rd_candidates_substitution(const RdCandidatesParams& p, hipStream_t s);
hipError_t launch_rd_decide_substitution(const RdDecideSignalParams& p, hipStream_t s);
// The mode statistics of a second pass: slot_modes [N][S] (per_qp 0: shared by the QPs) or [nb_qps][N][S], best_mode [nb_qps][N];
// stats uint32 [nb_qps][3][36] (used slot, slot 0, winner; a mode above 35 counts nowhere), ZEROED by the caller on the stream: the
// kernel adds to it.
struct ModeStatsParams { const uint8_t* slot_modes; const uint8_t* best_mode; int per_qp; int S; int N; int nb_qps; uint32_t* stats; };
hipError_t launch_mode_stats(const ModeStatsParams& p, hipStream_t s);

// Open-loop transform coding (pnn_trquant.hip): N predictions and targets [N][w][w] uint8, nb_qps <= 8 QPs whose constants the host has
// worked out (trquant::qp_consts at the unit size of w).  Outputs, each NULL or [nb_qps][N] uint32: the SSE of the reconstruction, the
// number of nonzero levels, the sum of the quantised magnitudes; recon NULL or uint8 [nb_qps][N][w][w].  rate NULL (the kernel without
// the rate) or uint64 [nb_qps][N], the CABAC rate of the levels in 2^-15 bit; with it modes NULL (diagonal scan) or uint8 [N], the intra
// mode that picks a block's scan (a value above 34 scans diagonally), and init_states, the context states each QP starts a unit with.
// sdh nonzero: the kernels with HM's sign-data hiding between quantisation and dequantisation; modes is then read
// with or without rate.
struct TrQuantParams {
    const uint8_t* pred; const uint8_t* targets; int N; int w; int nb_qps; trquant::QpConsts qp[trquant::kMaxQps];
    uint32_t* sse; uint32_t* nonzero; uint32_t* sum_abs; uint8_t* recon;
    uint64_t* rate; const uint8_t* modes; uint8_t init_states[trquant::kMaxQps][cabac::kNumCtx];
    int sdh;
    // rdoq nonzero: the kernels with HM's RDOQ in the quantiser's place (with sdh its own hiding): the host-made
    // constants of each QP, the initial states of the two cbf contexts and the unit's cbf context.  init_states is then read with or
    // without rate.  (At the end, so that the fields above stay where the kernels without RDOQ read them.)
    int rdoq; int cbf_ctx; rdoq::Consts rd[trquant::kMaxQps]; uint8_t cbf_states[trquant::kMaxQps][2];
};
int trquant_blocks_per_workgroup(int w);
hipError_t launch_trquant(const TrQuantParams& p, hipStream_t s);

// Transform skip of 4 x 4 units (pnn_tskip.hip).  launch_tskip4: the skipped form of the units of a TrQuantParams
// with w = 4 -- the same inputs, outputs and layouts as launch_trquant; the rate is walked where rate is given.  launch_tskip_decide:
// per (QP, unit) the merge of the two forms a launch_trquant and a launch_tskip4 call left in the caller's workspace (each array
// [nb_qps][N], recon [nb_qps][N][4][4] at a multiple of 16 bytes): decide 0 takes the skipped form of every unit (the transformed one
// is not read), decide 1 applies tskip::skipped_wins with mode_bits NULL (0) or uint32 [nb_qps][N].  Outputs, each NULL or as
// launch_trquant's, the rate with the flag bin of the kept form; ts_flag NULL or uint8 [nb_qps][N].
struct TskipForm { const uint32_t* sse; const uint32_t* nonzero; const uint32_t* sum_abs; const uint64_t* rate; const uint8_t* recon; };
struct TskipDecideParams {
    int N; int nb_qps; int decide; int charge_cbf; TskipForm transformed; TskipForm skipped; const uint32_t* mode_bits;
    double lambda[trquant::kMaxQps]; tskip::QpBits bits[trquant::kMaxQps];
    uint32_t* sse; uint32_t* nonzero; uint32_t* sum_abs; uint8_t* recon; uint64_t* rate; uint8_t* ts_flag;
};
hipError_t launch_tskip4(const TrQuantParams& p, hipStream_t s);
hipError_t launch_tskip_decide(const TskipDecideParams& p, hipStream_t s);
// The second pass with transform skip (width 4, the slots of ONE QP): launch_tskip_slot_bits writes the mode bits the tree charges
// each of the N S slots (msig::mode_frac_bits under the block's MPMs; 0 for an unused slot) for launch_tskip_decide's mode_bits;
// launch_tskip_best_flag gathers the winner's flag: best_flag[b] = ts_flag[b S + best_slot[b]], 0 for a block without a winner.
struct TskipSlotBitsParams {
    const uint8_t* slot_modes; const uint8_t* left; const uint8_t* above; int N; int S; int pnn_flag; msig::FlagBits bits; uint32_t* mode_bits;
};
hipError_t launch_tskip_slot_bits(const TskipSlotBitsParams& p, hipStream_t s);
struct TskipBestFlagParams { const uint8_t* ts_flag; const uint8_t* best_slot; int N; int S; uint8_t* best_flag; };
hipError_t launch_tskip_best_flag(const TskipBestFlagParams& p, hipStream_t s);

// The coding-tree pass (pnn_cu_tree.hip; the definition is pnn_cu_tree.h): per (QP, CTU) the partition of
// xCompressCU's recursion from the leaves dist / rate [5 widths: 4 .. 64] of [nb_qps][n_ctu][(64 / w)^2] (z-order), mode NULL or
// likewise, left / above NULL or uint8 [nb_qps][n_ctu][8], per QP lambda and the bins' bits, made on the host.  Outputs, each NULL or:
// cu_depths, part_nxn [nb_qps][n_ctu][64]; node_costs [nb_qps][n_ctu][85][2]; ctu_costs, ctu_dists, ctu_rates [nb_qps][n_ctu];
// selected, selected_pnn uint32 [nb_qps][5], ZEROED by the caller on the stream: the kernel adds to them.
struct CuTreeParams {
    const uint32_t* dist[cutree::kWidths]; const uint64_t* rate[cutree::kWidths]; const uint8_t* mode[cutree::kWidths];
    const uint8_t* left; const uint8_t* above; int n_ctu; int nb_qps; int pnn_mode;
    double lambda[cutree::kMaxQps]; cutree::QpBits bits[cutree::kMaxQps];
    uint8_t* cu_depths; uint8_t* part_nxn; double* node_costs; double* ctu_costs; uint64_t* ctu_dists; uint64_t* ctu_rates;
    uint32_t* selected; uint32_t* selected_pnn;
};
hipError_t launch_cu_tree(const CuTreeParams& p, hipStream_t s);
// The picture form: n_ctu = n_images ctu_rows ctu_cols CTUs in (image, CTU row, CTU column) order, left / above
// of p NOT read: a CTU's edges are gathered from the maps p.cu_depths holds of the CTU left of it and of the one above it in the same
// image (cutree::edge_from_maps), so p.cu_depths is REQUIRED (the entry points it into the caller's workspace where the caller asked
// for no map).  launch_cu_tree_picture makes ctu_rows + ctu_cols - 1 launches on s, one per anti-diagonal r + c, each of (CTUs of the
// diagonal x n_images, nb_qps) wavefronts: stream order makes the earlier diagonals' maps visible, and no workgroup waits on another.
// image_dists / image_rates NULL or uint64 [nb_qps][n_images], ZEROED by the caller on the stream: the roots' D and F are added.
struct CuTreePictureGrid { int n_images, ctu_rows, ctu_cols, diagonal; uint64_t* image_dists; uint64_t* image_rates; };
hipError_t launch_cu_tree_picture(const CuTreeParams& p, const CuTreePictureGrid& g, hipStream_t s);
// The leaves of one width from a second pass's outputs, each [total] = [nb_qps][n]: dist = sses, rate = rates + side_rates, mode =
// modes.  A copy, four elements per lane; vector loads and stores where every array is aligned to 16 bytes (modes to 4), else scalar.
struct CuTreeLeavesParams {
    const uint32_t* sses; const uint64_t* rates; const uint64_t* side_rates; const uint8_t* modes; long total;
    uint32_t* dist; uint64_t* rate; uint8_t* mode;
};
hipError_t launch_cu_tree_leaves(const CuTreeLeavesParams& p, hipStream_t s);

// IPFCN-S, the evaluator's second competitor (pnn_ipfcns.hip).  Blocks b0 .. b0 + nb - 1 of images x positions (image-major): the
// two groups of 8 reference lines at line origin (rows[pos], cols[pos]) of uint8 picture `img` [H][W] -- rows [r, r + 8) x columns
// [c, c + 2w + 8), then rows [r + 8, r + 2w + 8) x columns [c, c + 8), both row-major -- minus their mean fl32(S / K) (S the integer
// sum of the K = 64 + 32w samples): x [nb][K] and mean [nb].  The caller has checked that every origin lies inside the picture.
struct IpfcnsGatherParams {
    const uint8_t* channels; int H, W; const int32_t* rows; const int32_t* cols; int positions; long b0; int nb; int w;
    float* x; float* mean;
};
hipError_t launch_ipfcns_gather(const IpfcnsGatherParams& p, hipStream_t s);
// y[i] = y[i] > 0 ? y[i] : slope[i % H] * y[i] in place, i < total (total and H multiples of 4)
hipError_t launch_ipfcns_prelu(float* y, const float* slope, long total, int H, hipStream_t s);
// Output epilogue of nb blocks of w2 = w^2 values: pred = fl32(fc4 + mean[b]); f32 (optional) = pred; u8 (optional) =
// rint(clip(pred, 0, 255)) (half to even); sse (optional, with targets) = per-block uint32 sum of squared uint8 differences.
struct IpfcnsEpilogueParams {
    const float* fc4; const float* mean; int nb; int w2; uint8_t* u8; float* f32; const uint8_t* targets; uint32_t* sse;
};
hipError_t launch_ipfcns_epilogue(const IpfcnsEpilogueParams& p, hipStream_t s);

// Picture scoring (pnn_ipfcns.hip), blocks b0 .. b0 + nb - 1 of `pic`; every output pointer addresses block b0.  Of a pair of planes
// (pnn_score_picture_pairs_device) each kernel sees ONE: the descriptors address the context plane (they go to tbs_pass with it), the
// epilogue's pic.channels is the target plane.  Positions and geometry are those of both.
// Descriptors of the blocks' L-shaped contexts, as context.py builds them: origin = (image * H + row + w) * W + col + w (the target's
// top-left pixel), stride = W, above_mask = 2^(units - mask_w / 4) - 1 (units = 2w / 4; all 32 bits at w = 64 without a mask),
// left_units = units - mask_h / 4.  mask_w / mask_h: the call's; with pic.mask_w / pic.mask_h set, the block's own, by its position.
struct ScoreDescParams { PictureBlocks pic; long b0; int nb; int w; int mask_w, mask_h; TbDev* tbs; };
hipError_t launch_score_desc(const ScoreDescParams& p, hipStream_t s);
// Score epilogue: q = rint(clip(fl32(pred + mean), 0, 255)) (half to even) against the target read from the picture.  Each of u8
// [nb][w][w], targets [nb][w][w] (a copy of the picture's) and sse [nb] (uint32, exact) is optional; pred [nb][w][w] may be NULL
// when only the targets are wanted.
struct ScoreEpilogueParams {
    PictureBlocks pic; long b0; int nb; int w; const float* pred; float mean; uint8_t* u8; uint8_t* targets; uint32_t* sse;
};
hipError_t launch_score_epilogue(const ScoreEpilogueParams& p, hipStream_t s);

// Stand-alone HM epilogue for float predictions.
hipError_t launch_epilogue(const float* pred, long n, float mean, int32_t* dst, hipStream_t s);

}  // namespace pnn
