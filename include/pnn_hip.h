/*
 * pnn_hip.h -- C ABI of libpnn_hip.so: the MI355X (gfx950) replacement for the TensorFlow-1
 * frozen-graph inference that the reference's modified HM-16.15 calls per transform block.
 *
 * Boundary replaced (reference file:line):
 *   - tensor allocation      hevc/hm_common/c++/source_common/integration_prediction_neural_network.cpp:3-27
 *   - load_graph(s)          integration_prediction_neural_network.cpp:29-69,
 *                            selection logic hm_16_15_substitution/source/Lib/TLibCommon/TComPrediction.cpp:143-178
 *   - Session::Run + epilogue TComPrediction.cpp:554-635 (substitution), :550-661 (switch)
 *   - extract_context_portions hevc/hm_common/c++/source_common/extraction_context.cpp:3-208
 *   - model table parser      hevc/hm_common/c++/source_common/tools.cpp:52-111
 *   - Python batched driver   pnn/batching.py:7-88 (through the *_device entry points)
 *
 * Conventions: plain C types only; every function returns 0 on success and a negative PNN_E_* code on
 * error (pnn_last_error() gives the text); nothing throws across this boundary; the caller owns all
 * buffers; a context is thread-compatible (one context per thread), which is how the reference uses its
 * sessions (one TComPrediction object per encoder/decoder).
 *
 * Tensors keep the frozen graph's layout: float32, NHWC, mean-subtracted in AND out:
 *   FC   (w = 4, 8[, 16]) : node_flattened_context [N][5w^2] = [above w x 3w | left 2w x w]  -> [N][w][w]
 *   conv (w = 4 .. 64)    : node_portion_above [N][w][3w], node_portion_left [N][2w][w]       -> [N][w][w]
 */
#ifndef PNN_HIP_H
#define PNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNN_OK 0
#define PNN_E_ARG (-1)      /* bad argument (the reference's "return -1") */
#define PNN_E_IO (-2)       /* file missing / malformed */
#define PNN_E_MODEL (-3)    /* no model loaded for that width, or wrong kind */
#define PNN_E_HIP (-4)      /* HIP runtime error */
#define PNN_E_NOMEM (-5)
#define PNN_E_RANGE (-6)    /* an asynchronous split-precision pass left the f16 range: its results are invalid */

typedef struct pnn_ctx pnn_ctx;

/* ---- lifetime / models (replaces create_tensors_* + load_graphs + the mean pickle) ------------------ */

/* Creates a context on HIP device `device` with no model. `mean` is mean_training (117.8952234192841 for
 * luminance, sets/results/training_set/means/luminance/mean_training.pkl). */
int pnn_create_empty(pnn_ctx** out, float mean, int device);

/* As TComPrediction::initTempBuff (TComPrediction.cpp:108-178): parses the `width,is_pair,channel,path`
 * table (delimiters ',' and ';', blank lines ignored, tools.cpp:52-111), picks the `pair` models iff the
 * table lists them and use_pair != 0 (the caller passes qp >= 32), and loads the five luminance models
 * (widths 4, 8 fully-connected; 16, 32, 64 convolutional). Paths are `.pnnw` flat weight files (see
 * INTEGRATION.md); relative paths are resolved against the table's directory, then the working directory. */
int pnn_create(pnn_ctx** out, const char* model_table_path, int use_pair, float mean, int device);

/* Loads one model from a `.pnnw` file (width and kind come from its header). */
int pnn_load_model_file(pnn_ctx* ctx, const char* path);
/* Loads one model from host memory: `params` in the canonical flat order (weights.py:tensor_specs). */
int pnn_load_model_params(pnn_ctx* ctx, int width, int is_fc, const float* params, size_t n_params);

int pnn_model_info(const pnn_ctx* ctx, int width, int* is_fc, int* n_layers, long* n_params);
void pnn_destroy(pnn_ctx* ctx);
const char* pnn_last_error(const pnn_ctx* ctx);     /* ctx may be NULL: last error of a failed create */
float pnn_mean(const pnn_ctx* ctx);

/* Options (name, default, meaning).  None of them changes a result bit unless it says so; most exist for A/B measurements.
 *
 * ARITHMETIC -- the one option an encoder and its decoder must agree on:
 *   "precision"      0  the reference's arithmetic: IEEE float32 products and sums (Session::Run in float32, TComPrediction.cpp:572-579,
 *                       601-608; pnn/components.py:169-176) on the f32 matrix instructions.  Default since round 5.
 *                    1  every f32 product from three f16 MFMAs on hi/lo operand halves (22 significand bits per operand, lo x lo dropped:
 *                       f32-class accuracy, within the same +-1 LSB of the oracle) -- 2.3-2.7 x the blocks/s at batch, 5-25 % less per
 *                       single-block call.  Predictions of the two modes differ in the last float bits, i.e. by one LSB on .5 ties.
 *   Within a mode ONE per-output summation order holds at every batch size and on every kernel: a block's prediction is bit-identical
 *   whether it is predicted alone, in a handful or in any batch ("canonical_order" is kept as a name and accepts only 1).
 *
 * EXACT-F32 KERNELS ("precision" 0; also the range fallback of mode 1):
 *   "f32_small"            1   launches of at most "f32_small_max_tiles" (1024) output tiles of 16 x 16 -- single-block calls, the
 *                              batching service's handfuls -- run on tapgemm_f32_small_kernel (the canonical fmaf chain issued through
 *                              v_mfma_f32_16x16x4_f32, one wave per tile); 0: tapgemm_f32_kernel's 128-row tiles at every size
 *   "fc_out_f32"           1   nonzero: FC passes of <= 512 blocks run the output layer's K segments + their reduction as one launch;
 *                              0: two launches (the segments, then their reduction)
 *   "chain_io"             1   tensors between two launches of the small kernels travel with every 16-channel group in the order the 16x16x4
 *                              chain consumes it (one 16-byte LDS-DMA instruction per chunk of activations instead of four 4-byte ones); 0: never
 *   "tails"                1   small exact-f32 conv passes: the merger runs inside the branches' last pair launch (per block and channel group, by the
 *                              last of its five tiles to arrive) and the last transposed convolution inside the launch of the GEMM in front of it (per
 *                              block) -- two launches less per single-block call, the same bits; 0: every layer its own launch
 *   "f32_cfg"             -1   >= 0: force tile code [0, pnn_num_f32_configs()) of tapgemm_f32_kernel on every layer it is legal for
 *                              (the last two codes: PAIRED tiles for FC layers that keep their output -- a CU's 128 x 160 share as a 128 x 96
 *                              and a 128 x 64 workgroup resident together; off by rule, the tuner may take them)
 *   "f32_pair_occ"         0   paired tiles: 0 ask the runtime whether two such workgroups fit a CU (one: the launch runs the one 128 x 160 tile
 *                              instead, the same bits); N > 0: take N for its answer (tuning aid)
 *   "f32_seg_mode"         0   K segments of the deep convolution layers (> 2304 per output: summed in segments of <= 1600, whole taps,
 *                              added in order): 0 separate workgroups + a reduction launch, 1 in sequence inside the workgroups, -1 by model
 *   "f32_persist"         -1   convolution launches of 2-6 tiles per CU on two persistent workgroups per CU; 0 never; N > 0: N per CU
 *   "f32_overlap"          1   the two branches of a conv pass at batch on two streams
 *   "fuse_last"            1   FC passes of >= 1024 blocks run the <= 64-output layer inside the last hidden layer's kernel (both modes)
 * SPLIT-F16 KERNELS ("precision" 1):
 *   "sp_cfg"              -1   >= 0: force configuration code [0, pnn_num_split_configs()) of the three split-GEMM kernel families
 *   "ring" / "convimg"     1   the LDS-DMA ring kernel / the LDS-resident-image convolution kernel may be chosen
 *   "small"                1   GEMMs of at most "small_max_tiles" (512) tiles of 32 x 32 run on tapgemm_small_kernel (one wave per tile)
 *   "fuse_first"           1   the image kernel computes a branch's first (one-input-channel) convolution itself
 *   "fuse_tail"            1   the image kernel of the last 64-channel layer applies the net's last layer to its output tile
 *   "ring_pm"              1   position-major tiles (skip the taps that only meet SAME padding) where the launch model expects a gain;
 *                              2 wherever possible; 0 never.  Applies to tapgemm_f32_kernel's convolution launches too
 *   "autotune"             2   on first sight of a (layer, batch) pair time the legal configurations on the device and keep the fastest:
 *                              2 only launches >= 4 GFLOP, 1 always, 0 rule-based choice only.  Never while the stream is being captured
 * BOTH:
 *   "host_slice"           0   host-array calls (pnn_predict_fc / _conv / _pel) of at least two slices' worth of blocks run slice by slice on two
 *                              staging sets: slice i + 1 is copied in and slice i - 1 copied out while slice i computes.  0: slices of the bench
 *                              batch of the width (4096 / 4096 / 1024 / 256 / 64 blocks); N > 0: N blocks; -1: never (one copy in, passes, one copy out)
 *   "pair"                 1   small conv passes run layer i of BOTH branches as one launch
 *   "branch_streams"       1   small passes of the 32x32 / 64x64 nets, and passes at batch, run the two branches on two streams; 2: every
 *                              small conv pass too; 0: one stream
 *   "fuse_gather"          1   pnn_predict_tbs_device on a conv net: the first convolution reads the picture plane through the descriptors
 *   "cache_mb"             0   > 0: single-block host calls are answered from a direct-mapped cache of that many MiB when the same input
 *                              bytes were predicted before (HM's RD search repeats itself); dropped on any option / model change
 *   "flag_wait"            1   a small host call ends when its LAST kernel raises a sequence number in pinned host memory (3-7 us earlier
 *                              than the runtime's completion signal)
 *   "stream_priority"      0   < 0 / > 0: the context's own stream (host entry points) at the device's greatest / least priority
 *   "stream"               -   a hipStream_t (cast to long): the context's host entry points run on the caller's stream from now on
 *   "wait_sleep"           0   1: the thread of a small host call sleeps through the predictable part of its wait (running mean per batch
 *                              size, minus a margin) and spins only for the rest: the batching service's workers set it (two thirds of
 *                              their CPU time was that spin); a stand-alone codec keeps 0
 *   "seg_fold"             1   exact f32, small calls: the K segments of a deep layer (32x32 / 64x64 nets) are added up inside the
 *                              layer's launch by the last workgroup of each tile to arrive (planes written through, read back past
 *                              the caches, added in plane order) instead of by a reduction launch behind it: 17 -> 11 / 20 -> 11
 *                              launches per single-block call, the same bits
 *   "f32_small_deep"       1   exact f32, small calls: the weight ring of the small kernel 12 instead of 6 stages ahead of the MFMA chain
 *                              (84 instead of 48 KiB of LDS per workgroup) -- 0: never, 1: for the FC layers, 2: for every launch of at
 *                              most one workgroup per CU (the batching service sets 2: inside a campaign the weights come from the
 *                              MALL / HBM, a 4x4 call 55 -> 47 us; alone nothing changes for the FC nets, conv 16x16 82 -> 87 us)
 *   "graphs"               0   1: small host calls (<= 64 blocks): the launch chain of a shape (model, blocks, result kinds) is captured
 *                              on its second call and replayed with one hipGraphLaunch afterwards -- same kernels, same arguments,
 *                              same bits; a single-block call 1-4 us shorter for a thread that calls alone, nothing behind the
 *                              batching service.  Off by default: in this runtime a capture is invalidated when ANOTHER thread of the
 *                              process allocates / frees / copies synchronously meanwhile; the library's own such calls are
 *                              serialised against captures, a host application's own HIP calls are not
 *   "max_chunk" 0 (blocks per pass, 0 = by workspace), "ws_cap_mb" 8192, "time_launches" 0 (HIP events around every tap-GEMM launch)
 */
int pnn_set_option(pnn_ctx* ctx, const char* name, long value);
/* Environment variables read at pnn_create* (same meaning as the options; PNN_F32_SMALL_TILES is "f32_small_max_tiles"): PNN_PRECISION,
 * PNN_GRAPHS, PNN_AUTOTUNE, PNN_RING, PNN_CONVIMG, PNN_SMALL, PNN_F32_SMALL, PNN_F32_SMALL_TILES, PNN_F32_SMALL_DEEP, PNN_CHAIN_IO,
 * PNN_TAILS, PNN_CACHE_MB, PNN_FLAG_WAIT, PNN_WAIT_SLEEP, PNN_FUSE_FIRST, PNN_FUSE_GATHER, PNN_FUSE_TAIL, PNN_FUSE_LAST, PNN_RING_PM,
 * PNN_BRANCH_STREAMS, PNN_MAX_CHUNK, PNN_F32_CFG, PNN_F32_OVERLAP, PNN_F32_SEG_MODE, PNN_F32_PERSIST.
 * Diagnostics: PNN_DEBUG (kernel choice of every GEMM launch on stderr), PNN_DEBUG_TUNE, PNN_PROFILE (synchronous per-launch timing),
 * PNN_HOST_TRACE, PNN_LIB_PATH (Python loader: another build of the library); diagnostic library of `make diag` only: PNN_SP_DIAG,
 * PNN_F32_DIAG, PNN_F32S_DIAG. */
/* Input-range contract of "precision" 1: operands travel as pairs of f16 values, so every intermediate activation must satisfy
 * |v| < 65504.  8-bit contexts through trained models stay two orders of magnitude below that; arbitrary float inputs or
 * models may not.  The kernels detect a violation (never a silent NaN): host entry points then recompute, on the exact-f32 kernels,
 * exactly the blocks that overflow when predicted alone (batches of <= 256; the other blocks keep the bits they get in any batch) and
 * refuse non-finite inputs (PNN_E_ARG); models with a non-finite parameter are refused at load (PNN_E_MODEL).  Device entry points are
 * asynchronous: the NEXT call on the context fails with PNN_E_RANGE, and pnn_check_range -- which waits for `stream` -- tells right
 * away (*host_fallbacks, optional = how many host calls took the exact-f32 repeat so far).  "precision" 0 has no such bound. */
int pnn_check_range(pnn_ctx* ctx, void* stream, long* host_fallbacks);

/* A short string naming everything that decides the last float bits of this context's predictions -- the arithmetic ("precision"), its
 * per-output summation order and the K-segment layout of the deep exact-f32 layers, the library's order revision.  An encoder and its
 * decoder (or an encoder and the batching service it talks to) produce identical predictions iff their tags are equal: compare them
 * once at start-up. */
int pnn_arithmetic_tag(const pnn_ctx* ctx, char* out, size_t bytes);

/* Number of configuration codes "sp_cfg" accepts (tile shapes of tapgemm_sp_kernel, convimg_sp_kernel, tapgemm_ring_kernel). */
int pnn_num_split_configs(void);
/* Number of configuration codes "f32_cfg" accepts (tiles of tapgemm_f32_kernel; all of them give the same bits). */
int pnn_num_f32_configs(void);
/* Paired tiles of tapgemm_f32_kernel: launches of this context that ran as pairs / that fell back to the one 128 x 160 tile. */
int pnn_f32_pair_stats(const pnn_ctx* ctx, long* paired, long* fell_back);
/* ... and the grid arithmetic of such a launch of an M x cout layer (host only, no device needed): *num_wgs = workgroups of its 1-D
 * grid; workgroup wg < *num_wgs owns rows [*row0, *row0 + 128) and columns [*col0, *col0 + *cols), clipped to the layer; *cols = 0:
 * it has no tile. */
int pnn_f32_pair_tile(int M, int cout, int wg, int* num_wgs, int* row0, int* col0, int* cols);
/* Hits / misses of the "cache_mb" prediction cache since the option was last set. */
int pnn_cache_stats(pnn_ctx* ctx, long* hits, long* misses);

/* ---- host-buffer entry points (what the HM side binds; synchronous) ---------------------------------- */

/* == Session::Run({{"node_flattened_context", T}}, {"fully_connected/node_output"}) for N stacked inputs. */
int pnn_predict_fc(pnn_ctx* ctx, int width, const float* context, int n, float* out);
/* == Session::Run({{"node_portion_above", A}, {"node_portion_left", L}}, {".../node_output"}). */
int pnn_predict_conv(pnn_ctx* ctx, int width, const float* above, const float* left, int n, float* out);
/* Either of the above followed by the HM epilogue (TComPrediction.cpp:621-635), written with row stride
 * `dst_stride` into `dst` for n == 1, or densely [n][w][w] when dst_stride == width. For FC models
 * `left` is ignored when it equals above + 3w^2 or is NULL (one flattened buffer, TComPattern.cpp:352-353). */
int pnn_predict_pel(pnn_ctx* ctx, int width, const float* above, const float* left, int n, int32_t* dst,
                    int dst_stride);

/* Batched calls of these entry points (more than 64 KiB of input) copy in, compute, copy out.  From PINNED caller arrays the copies
 * run ~10 % of the call faster (no staging inside the runtime): hipHostMalloc / hipHostRegister, or these two (page-locked,
 * device-visible; any thread may free). */
int pnn_host_alloc(void** out, size_t bytes);
void pnn_host_free(void* p);

/* The runtime deals HIP streams onto a few hardware queues (4 by default); streams that share one run their kernels in submission order,
 * so two threads with a context each may find themselves waiting for each other's whole calls.  pnn_streams_on_distinct_queues creates
 * `want` (<= 8) streams that were MEASURED to sit on different hardware queues and returns how many it found; give one to a context with
 * pnn_set_option(ctx, "stream", (long) stream) -- its host entry points then run there -- and release them after the contexts.
 * (The batching service does this for its width workers: pnn_service_run_table.) */
int pnn_streams_on_distinct_queues(void** out_streams, int want);
void pnn_streams_release(void** streams, int n);

/* Both results of one pass: the float prediction (as pnn_predict_fc / pnn_predict_conv) into `out` [n][w][w] and the
 * HM-epilogue Pel values (as pnn_predict_pel, dense) into `dst` [n][w][w]; either may be NULL. */
int pnn_predict_f32_pel(pnn_ctx* ctx, int width, const float* above, const float* left, int n, float* out, int32_t* dst);

/* == extract_context_portions (extraction_context.cpp:3-208), same argument order and error behaviour
 * (returns -1 on NULL pointers, n_avail <= 0, unavailable corner unit). Pure host code. */
int pnn_extract_context(const int32_t* roi_origin, float* above, float* left, const uint8_t* neighbor_flags,
                        int n_avail, int unit_w, int unit_h, int above_units, int left_units, int tu_w,
                        int tu_h, int pic_stride, float mean);

/* Parses the model table; returns the number of entries written (<= max_entries) or a negative code.
 * paths[i] points into an internal buffer valid until the next call on the same thread. */
int pnn_parse_model_table(const char* path, int* widths, int* is_pair, int* channels, const char** paths,
                          int max_entries);

/* ---- device-resident entry points (batched path, asynchronous on `stream`) --------------------------- */

/* All pointers are device pointers on the context's device; `stream` is a hipStream_t (NULL = HIP's
 * default stream, as everywhere in HIP). Calls only enqueue work; the caller synchronises. */
int pnn_predict_fc_device(pnn_ctx* ctx, int width, const float* d_context, int n, float* d_out, void* stream);
int pnn_predict_conv_device(pnn_ctx* ctx, int width, const float* d_above, const float* d_left, int n,
                            float* d_out, void* stream);

/* One transform block of the batched gather. Build it with pnn_make_tb_desc from HM's neighbour flags. */
typedef struct {
    int64_t origin;       /* element index of the TB's top-left pixel from the plane base pointer */
    int32_t stride;       /* plane row stride in elements */
    uint32_t above_mask;  /* bit u: above / above-right unit u (left to right) is available */
    int32_t left_units;   /* number of available left / below-left units, counted from the top */
    int32_t reserved;
} pnn_tb_dev;

/* Translates HM's (bNeighborFlags, iNumIntraNeighbor) of TComPattern.cpp:260-280 into a descriptor with
 * exactly the semantics of extraction_context.cpp:49-205. Returns -1 where the reference returns -1. */
int pnn_make_tb_desc(pnn_tb_dev* out, int64_t origin, int32_t stride, const uint8_t* neighbor_flags,
                     int n_avail, int above_units, int left_units);

/* Batched gather only: Pel plane (pel_bytes 4 = HM `Pel`/int32, 1 = uint8 image) -> mean-subtracted,
 * masked float portions. For FC layouts pass d_left = d_above + 3w^2 and both pitches = 5w^2. */
int pnn_gather_device(pnn_ctx* ctx, int width, int unit, const void* d_plane, int pel_bytes,
                      const pnn_tb_dev* d_tbs, int n, float* d_above, long pitch_above, float* d_left,
                      long pitch_left, void* stream);

/* The whole hot path for n TBs of one width: gather -> net -> (+mean, clamp, round) -> int32 [n][w][w]
 * (and, when d_out_f32 != NULL, the raw float prediction as the frozen graph returns it). */
int pnn_predict_tbs_device(pnn_ctx* ctx, int width, const void* d_plane, int pel_bytes, const pnn_tb_dev* d_tbs,
                           int n, int32_t* d_dst, float* d_out_f32, void* stream);

/* Distortion of n predicted blocks d_pred [n][w][w] against the ORIGINAL picture d_org_plane (same geometry as the
 * reconstructed plane: the descriptors' origin / stride address both), as HM's first intra pass computes it for a
 * candidate mode (TEncSearch.cpp:2376-2389, distParam.DistFunc): hadamard != 0 -> TComRdCost::xGetHADs (8x8 / 4x4
 * Hadamard SATD, TComRdCost.cpp:1753-1824), 0 -> SAD; 8-bit video.  Integer arithmetic, bit-exact. */
int pnn_block_cost_device(pnn_ctx* ctx, int width, const void* d_org_plane, int pel_bytes, const pnn_tb_dev* d_tbs, int n,
                          const int32_t* d_pred, int hadamard, uint32_t* d_cost, void* stream);
/* pnn_predict_tbs_device followed by pnn_block_cost_device on the same stream: only the n cost scalars need to leave
 * the device for candidates that are not selected (d_dst may be NULL). */
int pnn_predict_tbs_cost_device(pnn_ctx* ctx, int width, const void* d_plane, const void* d_org_plane, int pel_bytes,
                                const pnn_tb_dev* d_tbs, int n, int hadamard, uint32_t* d_cost, int32_t* d_dst, void* stream);

/* ---- HEVC intra prediction: the evaluator's best-mode competitor ------------------------------------- */

/* == hevc_intraprediction (hevc/intraprediction/c++/source/extracted_hevc_intraprediction.cpp:3-134, called per mode by
 * interface.pyx:15-64): the prediction [width][width] of HEVC intra mode `mode` (0 planar, 1 DC, 2..34 angular; 8-bit luma)
 * from a dense uint8 intra pattern [pattern_h][pattern_w] of which only the first row (corner, above, above-right) and the
 * first column (corner, left, below-left) are read; a shorter row / column is padded with its last sample.  No reference
 * sample smoothing (the reference did not extract it; pnn_hevc_intra_predict_hm below has it as an option); DC filtering and the
 * mode 10 / 26 edge filter for width <= 16.
 * Returns -1 + a line on stderr where the reference throws: NULL pointers, mode > 34, a side of the pattern outside
 * [width + 1, 2 width + 1]; also for a width other than 4, 8, 16, 32, 64 and for mode < 0.  Pure host code. */
int pnn_hevc_intra_predict(const uint8_t* intra_pattern, int pattern_h, int pattern_w, int width, int mode, uint8_t* out);

/* HM's reference-sample smoothing (filteringIntraReferenceSamples, TComPattern.cpp:410-478 and :721-746; the decision table
 * TComPrediction.cpp:39-55; called at TEncSearch.cpp:2402-2422), the option `smoothing` of every *_hm entry of this header:
 *   0  none: the reference's extracted predictor.  Every entry without the suffix is its *_hm sibling called with 0, same bits.
 *   1  HM with StrongIntraSmoothing 0: the [1 2 1] filter alone.
 *   2  HM's default (StrongIntraSmoothing 1): the strong filter where it applies, the [1 2 1] filter elsewhere.
 * Which modes read smoothed samples: mode != 1 and min(|mode - 10|, |mode - 26|) > thr, thr = 10, 7, 1, 0, 10 for width 4 .. 64 --
 * none at width 4 and 64, {0, 2, 18, 34} at 8, all but {1, 9, 10, 11, 25, 26, 27} at 16, all but {1, 10, 26} at 32.  DC and the modes
 * 10 / 26 never do, so the DC filter and the edge filter always read unsmoothed samples.
 * The smoothed line: the 4 width + 1 samples AFTER the padding rule above (HM substitutes first and filters afterwards), rf[j] for j
 * in [-2 width, 2 width] with the corner at 0, the left column below it and the above row to the right.  rf[+-2 width] are copied;
 * every other sample becomes (rf[j - 1] + 2 rf[j] + rf[j + 1] + 2) >> 2.  Strong filter: only width 32, only smoothing 2, only when
 * |rf[-64] + rf[0] - 2 rf[-32]| < 8 and |rf[0] + rf[64] - 2 rf[32]| < 8 (8 = 1 << (bitDepth - 5)); then the corner and both ends are
 * copied, rf[-64 + i] = ((64 - i) rf[-64] + i rf[0] + 32) >> 6 and rf[i] = ((64 - i) rf[0] + i rf[64] + 32) >> 6 for i = 1 .. 63.
 * 8-bit luma, integers only.  PNN_E_ARG for a smoothing outside {0, 1, 2}.
 *
 * 1 if `mode` (0 .. 34) reads smoothed samples at `width`, else 0; PNN_E_ARG + a line on stderr for another width or mode. */
int pnn_hevc_mode_uses_smoothing(int width, int mode);
/* The line itself, so that it can be looked at: line[2 width + j] = rf[j] of `pattern` (as for pnn_hevc_intra_predict), padded and then
 * smoothed as `smoothing` says (0, or a width of 4 or 64: the padded line); *strong_used (may be NULL) = 1 if the strong filter was
 * applied.  PNN_E_ARG + a line on stderr for NULL pointers, a bad width, pattern side or smoothing.  Pure host code. */
int pnn_hevc_smoothed_reference_host(const uint8_t* pattern, int pattern_h, int pattern_w, int width, int smoothing, uint8_t* line,
                                     int* strong_used);
/* pnn_hevc_intra_predict with `mode` reading the smoothed line where the table says so.  Same refusals, and a bad smoothing. */
int pnn_hevc_intra_predict_hm(const uint8_t* intra_pattern, int pattern_h, int pattern_w, int width, int mode, int smoothing,
                              uint8_t* out);

/* == predict_via_hevc_best_mode (hevc/intraprediction/intraprediction.py:231-294) for n blocks at once, on the GPU.
 * Inputs: dense patterns [n][pattern_h][pattern_w] (as above) and targets [n][width][width], uint8.  For each block all 35
 * predictions and their SSE against the target; the best mode is the one of smallest SSE, the lowest index among ties (the
 * reference keeps a mode only when its PSNR 10 log10(255^2 / (SSE / width^2 + 1e-6)) is strictly larger than the best so far,
 * starting from 0 dB).  Outputs, each NULL or [n]: d_best_mode (uint8), d_best_sse (uint32), d_best_pred [n][width][width]
 * (uint8; all zeros when even the best SSE is 65025 width^2, as the reference keeps its zero start), d_mode_sse [n][35]
 * (uint32).  Not every output may be NULL; n == 0 does nothing.  A context without models (pnn_create_empty) suffices. */
int pnn_hevc_best_mode_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w,
                              const uint8_t* d_targets, int n, uint8_t* d_best_mode, uint32_t* d_best_sse,
                              uint8_t* d_best_pred, uint32_t* d_mode_sse, void* stream);
/* The same search over the predictions of pnn_hevc_intra_predict_hm(.., smoothing, ..); d_best_pred is that function's prediction of
 * d_best_mode.  PNN_E_ARG for a smoothing outside {0, 1, 2}, before any launch. */
int pnn_hevc_best_mode_hm_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w,
                                 const uint8_t* d_targets, int n, int smoothing, uint8_t* d_best_mode, uint32_t* d_best_sse,
                                 uint8_t* d_best_pred, uint32_t* d_mode_sse, void* stream);

/* ---- IPFCN-S: the evaluator's second competitor ------------------------------------------------------ */

/* IPFCN-S (Li et al.; the reference's ipfcns/ipfcns.py with IntraFCN205_deploy_Size{4,8,16,32}.prototxt): four InnerProduct
 * layers, input K = 64 + 32 width, hidden H = 512 (width 4), 1024 (8, 16), 2048 (32), output width^2, PReLU (one slope per
 * channel, v > 0 ? v : a v) behind fc1 .. fc3.  `params` in ONE flat canonical order, Caffe's own layouts:
 *   W1[H][K], b1[H], a1[H], W2[H][H], b2, a2, W3[H][H], b3, a3, W4[width^2][H], b4[width^2].
 * Arithmetic: exact-f32 order revision 6, items 4, 6 and 8 on every layer ("IPFCN-S").
 *
 * Host twin (pure host code, threads over blocks; the bits do not depend on their number): x [n][K] -> the activations after
 * layer `layers` (1 .. 3: [n][H] behind the PReLU; 4: fc4 [n][width^2], without the mean).  PNN_E_ARG for a bad width / layers. */
int pnn_ipfcns_forward_host(int width, const float* params, const float* x, int n, int layers, float* out);
/* Loads (or replaces) the IPFCN-S of `width` on the context; a model-less pnn_create_empty context suffices.  PNN_E_ARG for a
 * width outside {4, 8, 16, 32}, a count other than the architecture's, a non-finite parameter. */
int pnn_ipfcns_load(pnn_ctx* ctx, int width, const float* params, size_t n_floats);
/* The reference's flattened-input entry (predict_by_batch_via_ipfcns): d_x [n][K] (mean-subtracted rows) -> d_out_f32 [n][width^2]
 * = fc4, asynchronous on `stream`; bit-identical to pnn_ipfcns_forward_host(..., 4, ...).  n == 0 does nothing. */
int pnn_ipfcns_forward_device(pnn_ctx* ctx, int width, const float* d_x, int n, float* d_out_f32, void* stream);
/* The fused path from pictures: d_channels uint8 [images][height][width_ch]; line origins (d_rows[p], d_cols[p]), int32
 * [positions]; blocks image-major (b = image * positions + p).  Per block the two groups of 8 reference lines (rows [r, r + 8) x
 * columns [c, c + 2 width + 8), then rows [r + 8, r + 2 width + 8) x columns [c, c + 8), row-major), S their integer sum,
 * mean = fl32(S / K), x = fl32(sample - mean); fc1 .. fc4; pred = fl32(fc4 + mean).  Outputs, each NULL or per block:
 * d_pred_u8 [n][width][width] = rint(clip(pred, 0, 255)) (half to even, tools.cast_float_to_uint8), d_pred_f32 = pred,
 * d_means [n], d_sse [n] uint32 = sum of squared differences of d_pred_u8 against d_targets [n][width][width] (needs d_targets).
 * n == 0 does nothing.  PNN_E_ARG, before any launch, for an origin whose lines leave the picture, a width outside
 * {4, 8, 16, 32} or no net loaded for it.  Reads d_rows / d_cols back to the host (the call waits for `stream` once). */
int pnn_ipfcns_predict_device(pnn_ctx* ctx, int width, const uint8_t* d_channels, int images, int height, int width_ch,
                              const int32_t* d_rows, const int32_t* d_cols, int positions, const uint8_t* d_targets,
                              uint8_t* d_pred_u8, float* d_pred_f32, float* d_means, uint32_t* d_sse, void* stream);

/* ---- the evaluator's scores from pictures --------------------------------------------------------------- */

/* The columns of the reference's predict_mask (comparing_pnn_ipfcns_hevc_best_mode.py:162-322) for one mask, from uint8 pictures
 * that stay on the device: d_channels [images][height][width_ch]; (d_rows[p], d_cols[p]), int32 [positions], is the top-left
 * corner of a block's 3 width x 3 width context square (the evaluator's row_1sts / col_1sts), its target the width x width
 * square at (row + width, col + width); blocks image-major (b = image * positions + p), n = images * positions of them.
 * (mask_w, mask_h) in {0, 4, .., width}: the rightmost mask_w columns of the above portion and the lowest mask_h rows of the left
 * one are masked for the PNN (the descriptors of pnn_gather_device), and the intra pattern of the HEVC search ends there.
 * Outputs, each NULL or per block:
 *   d_targets   uint8 [n][width][width]  the targets, copied from the pictures
 *   d_pnn_f32   float [n][width][width]  the raw net output without the mean, as pnn_predict_tbs_device's d_out_f32 gives it
 *   d_pnn_u8    uint8 [n][width][width]  rint(clip(fl32(net + mean), 0, 255)), half to even (tools.cast_float_to_uint8)
 *   d_pnn_sse   uint32 [n]               sum of squared differences of d_pnn_u8 against the target
 *   d_hevc_mode / d_hevc_sse / d_hevc_pred   as d_best_mode / d_best_sse / d_best_pred of pnn_hevc_best_mode_device on the
 *               intra pattern at (row + width - 1, col + width - 1); the search reads the pictures, no dense pattern is built
 * The PNN half is descriptors -> the pass of pnn_predict_tbs_device (pel_bytes 1) -> epilogue, in slices that keep the workspace
 * bounded ("max_chunk"); a block's bits do not depend on the slice it travels in.  The three PNN outputs need a model of that
 * width on the context (PNN_E_ARG without one); for the targets and the HEVC outputs alone a pnn_create_empty context suffices.
 * n == 0 does nothing.  PNN_E_ARG, before any launch, for a width outside {4, 8, 16, 32, 64}, a mask outside {0, 4, .., width},
 * a negative position, row + 3 width > height or col + 3 width > width_ch, or every output NULL.  Reads d_rows / d_cols back to
 * the host to check them (the call waits for `stream` once); everything after that is asynchronous on `stream`. */
int pnn_score_pictures_device(pnn_ctx* ctx, int width, const uint8_t* d_channels, int images, int height, int width_ch,
                              const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w, int mask_h,
                              uint8_t* d_targets, uint8_t* d_pnn_u8, float* d_pnn_f32, uint32_t* d_pnn_sse,
                              uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred, void* stream);
/* pnn_score_pictures_device on PAIRS of pictures, as the reference carries the data of its "pair" models ([images, H, W, 2]: channel 0
 * the original, channel 1 the HEVC-decoded picture; sets/common.py gathers contexts from the last channel and targets from channel 0):
 * d_context_channels (the decoded pictures) and d_target_channels (the originals), both uint8 [images][height][width_ch], in place of
 * d_channels.  The caller de-interleaves; the planes have one geometry and share positions, masks and block order.
 *   read from the CONTEXT plane:  the PNN's contexts (descriptors and gather of the pass), and the intra pattern of the HEVC search at
 *                                 (row + width - 1, col + width - 1)
 *   read from the TARGET plane:   d_targets, and the targets of both SSEs (d_pnn_sse, d_hevc_sse; d_hevc_mode minimises the latter)
 * The reference's extract_intra_patterns takes single-channel pictures only and has no pair form, so which plane feeds the intra
 * pattern is THIS PROJECT'S DEFINITION: the decoded plane, because the reconstructed neighbourhood is what an encoder holds when it
 * predicts a block (the original's samples are not available to a decoder at all).
 * Outputs, slices, checks (all before any launch) and the read-back of d_rows / d_cols are those of pnn_score_pictures_device; in
 * addition PNN_E_ARG when exactly one of the two planes is NULL.  With d_context_channels == d_target_channels every output has the
 * bits of pnn_score_pictures_device, which is this entry called that way.
 * The two entries that take the targets apart from the pictures need no pair form.  A pair caller passes
 *   pnn_score_f32_device:       d_channels = the TARGET plane (the entry reads nothing but targets from it);
 *   pnn_ipfcns_predict_device:  d_channels = the CONTEXT plane (the reference lines, ipfcns.py:60-65 reads the last channel), d_targets =
 *                               target blocks taken from the target plane (the d_targets output of this entry). */
int pnn_score_picture_pairs_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                   int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                   int mask_w, int mask_h, uint8_t* d_targets, uint8_t* d_pnn_u8, float* d_pnn_f32, uint32_t* d_pnn_sse,
                                   uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred, void* stream);
/* The same with the HEVC search of pnn_hevc_best_mode_hm_device: `smoothing` as above, the smoothed line built from the padded samples
 * of the CONTEXT plane, as the unsmoothed one is.  The PNN outputs and d_targets do not depend on it. */
int pnn_score_picture_pairs_hm_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                      int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                      int mask_w, int mask_h, int smoothing, uint8_t* d_targets, uint8_t* d_pnn_u8, float* d_pnn_f32,
                                      uint32_t* d_pnn_sse, uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred, void* stream);
/* The epilogue alone, on any predictor's floats: d_pred_f32 [n][width][width] (mean-subtracted) -> d_pred_u8 = rint(clip(fl32(pred
 * + pnn_mean(ctx)), 0, 255)), half to even, and d_sse [n] against the targets in the pictures (either may be NULL, not both).
 * Same geometry, same checks and the same read-back of d_rows / d_cols as above.  The result for a non-finite prediction is
 * unspecified (none can come from a uint8 picture through a loaded model). */
int pnn_score_f32_device(pnn_ctx* ctx, int width, const float* d_pred_f32, const uint8_t* d_channels, int images, int height,
                         int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                         uint8_t* d_pred_u8, uint32_t* d_sse, void* stream);

/* ---- HM's first intra pass: the 35 modes and a candidate ranked by Hadamard cost ------------------------ */

/* The SATD twin of pnn_hevc_best_mode_device: where does a candidate prediction (the PNN's) rank among the 35 modes in the metric HM's
 * first intra pass selects by (TEncSearch.cpp:2376-2492)?
 *   Predictions.  The 35 predictions of pnn_hevc_intra_predict, from the same intra patterns.  HM also smooths the reference samples
 *     for some modes and sizes (filteringIntraReferenceSamples); the reference's extracted predictor does not.  SMOOTHING IS AN OPTION
 *     of the *_hm entries below (see pnn_hevc_mode_uses_smoothing): 0, and every entry without the suffix, reproduces the reference's
 *     extracted predictor, so its costs are those of the evaluator's competitor; 2 gives the costs of HM's own filtered predictor.
 *   Cost of one prediction.  TComRdCost::xGetHADs for 8-bit video (TComRdCost.cpp:1753-1824) against the width x width target: the
 *     Walsh-Hadamard transform of target - prediction per T x T sub-block, T = 8 (4 at width 4); per sub-block the sum s of the
 *     absolute coefficients, rounded (s + 2) >> 2 for T = 8 and (s + 1) >> 1 for T = 4; the (width / T)^2 sub-block sums added.
 *     All integers, exact in any order, uint32 (below 2^25 at width 64).
 *   The list.  xUpdateCandList applied to modes 0 .. 34 in index order, then to the candidate as index 35 if one was given, with the
 *     cost alone: K = pnn_first_pass_list_size(width) entries in ascending cost; among equal costs the lower index comes first (HM
 *     inserts on strict <, so the candidate loses every tie).  HM adds modeBits * sqrtLambda to each cost; that term depends on the
 *     neighbours' coded modes and on QP, does not exist open-loop and IS LEFT OUT.  (The switch encoder appends mode 35 to its list
 *     unconditionally, TEncSearch.cpp:2476-2491; this list says whether it would have entered on merit.)
 * K = 8, 8, 3, 3, 3 for width 4, 8, 16, 32, 64 (g_aucIntraModeNumFast_UseMPM); PNN_E_ARG for another width. */
int pnn_first_pass_list_size(int width);
/* Inputs: dense patterns [n][pattern_h][pattern_w] and targets [n][width][width] as for pnn_hevc_best_mode_device; cand_pred NULL or
 * [n][width][width] uint8, the candidate's predictions.  Outputs, each NULL or per block: mode_hads [n][35] (uint32), cand_hads [n]
 * (uint32; needs cand_pred), list_modes [n][K] (uint8; 35 = the candidate), list_costs [n][K] (uint32).  Without a candidate the list
 * ranges over the 35 modes.  n == 0 does nothing.  PNN_E_ARG for a width outside {4, 8, 16, 32, 64}, a pattern side outside
 * [width + 1, 2 width + 1], n < 0, NULL inputs with n > 0, every output NULL, cand_hads without cand_pred.
 * The host twin: pure host code, the zero-tolerance yardstick of the device entries and what a CPU-only user calls. */
int pnn_hevc_mode_hads_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                            const uint8_t* cand_pred, uint32_t* mode_hads, uint32_t* cand_hads, uint8_t* list_modes,
                            uint32_t* list_costs);
/* The same over the predictions of pnn_hevc_intra_predict_hm(.., smoothing, ..); in addition PNN_E_ARG (+ a line on stderr) for a
 * smoothing outside {0, 1, 2}. */
int pnn_hevc_mode_hads_hm_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                               const uint8_t* cand_pred, int smoothing, uint32_t* mode_hads, uint32_t* cand_hads, uint8_t* list_modes,
                               uint32_t* list_costs);
/* The same on the GPU, all 35 modes x cost, the candidate and the list of n blocks in one launch; device pointers, asynchronous on
 * `stream`, every argument error reported before the launch.  A context without models (pnn_create_empty) suffices. */
int pnn_hevc_mode_hads_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w,
                              const uint8_t* d_targets, int n, const uint8_t* d_cand_pred, uint32_t* d_mode_hads, uint32_t* d_cand_hads,
                              uint8_t* d_list_modes, uint32_t* d_list_costs, void* stream);
/* pnn_hevc_mode_hads_hm_host on the GPU: bit-identical to it.  PNN_E_ARG for a smoothing outside {0, 1, 2}, before any launch. */
int pnn_hevc_mode_hads_hm_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w,
                                 const uint8_t* d_targets, int n, const uint8_t* d_cand_pred, int smoothing, uint32_t* d_mode_hads,
                                 uint32_t* d_cand_hads, uint8_t* d_list_modes, uint32_t* d_list_costs, void* stream);
/* The same from the evaluator's pictures: geometry, block order (n = images * positions, image-major), masks and checks of
 * pnn_score_picture_pairs_device.  The reference samples (the intra pattern at (row + width - 1, col + width - 1), ending where the
 * mask says) come from the CONTEXT (decoded) plane, the targets from the TARGET (original) plane; d_cand_pred [n][width][width] is
 * what that entry's d_pnn_u8 holds.  With d_context_channels == d_target_channels it is the single-picture form.  PNN_E_ARG, before
 * any launch, for a width outside {4, 8, 16, 32, 64}, a mask outside {0, 4, .., width}, a negative position, row + 3 width > height
 * or col + 3 width > width_ch, exactly one NULL plane, every output NULL, d_cand_hads without d_cand_pred.  n == 0 does nothing.
 * Reads d_rows / d_cols back to the host to check them (the call waits for `stream` once); everything after is asynchronous. */
int pnn_first_pass_picture_pairs_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                        int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols,
                                        int positions, int mask_w, int mask_h, const uint8_t* d_cand_pred, uint32_t* d_mode_hads,
                                        uint32_t* d_cand_hads, uint8_t* d_list_modes, uint32_t* d_list_costs, void* stream);
/* The same with `smoothing`: the smoothed line from the padded samples of the CONTEXT plane. */
int pnn_first_pass_picture_pairs_hm_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols,
                                           int positions, int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing,
                                           uint32_t* d_mode_hads, uint32_t* d_cand_hads, uint8_t* d_list_modes, uint32_t* d_list_costs,
                                           void* stream);

/* ---- open-loop transform coding: what is left of a prediction after HM's residual path ------------------ */

/* Every column above judges a PREDICTION; HM keeps what the residual leaves after transform, quantisation, dequantisation and inverse
 * transform.  These entries code the residual target - prediction of n blocks at up to 8 QPs the way HM does with RDOQ 0 (xTrMxN, the
 * non-RDOQ branch of xQuant, the no-scaling-list branch of xDeQuant, xITrMxN of TComTrQuant.cpp; the decoder half is normative HEVC).
 * 8-bit luma, intra, I slice, coefficients of 15 bits + sign.  OPEN-LOOP: the prediction is given, nothing is predicted again from a
 * reconstruction.  LEFT OUT, because each needs bit estimates from the running entropy-coder state, which does not exist open-loop
 * (as modeBits * sqrtLambda above): RDOQ with its own sign hiding, transform skip.  (The CABAC rate of the levels, counted from the
 * state a slice STARTS with, is the next group of entries; the sign-data hiding xQuant does with RDOQ 0, which needs no such state,
 * the group after it.)
 *   Transform units.  T = width up to 32.  At width 64 the units are the four 32 x 32 quadrants of the ONE 64 x 64 prediction, in
 *     raster order (HEVC has no 64-point transform).  That the quadrants are not predicted again one by one, as HM would, is THIS
 *     PROJECT'S DEFINITION.  L = log2 T.
 *   Matrices.  M = the T-point HEVC core transform matrix of H.265 8.6.4.2; at T = 4 the 4 x 4 DST-VII {29 55 74 84; 74 74 0 -74;
 *     84 -29 -74 55; 55 -84 74 -29} (intra luma 4 x 4 always uses it).  HM's butterflies are exact integer factorisations: the plain
 *     products below give the same integers, every intermediate within int32 (at most 32 * 90 * 2^15).
 *   Forward.  X = target - prediction, rows y, columns x; >> is the arithmetic shift of a signed value.
 *     Y[y][k] = (sum_x X[y][x] M[k][x] + (1 << (s1 - 1))) >> s1, s1 = L - 1;  C[l][k] = (sum_y Y[y][k] M[l][y] + (1 << (s2 - 1))) >> s2, s2 = L + 6.
 *   Quantisation at QP q in [0, 51].  per = q / 6, rem = q % 6, scale = {26214, 23302, 20560, 18396, 16384, 14564}[rem], ts = 7 - L,
 *     qbits = 14 + per + ts, add = 171 << (qbits - 9) (171: the I-slice value);  mag = (|C| scale + add) >> qbits in 64 bits;
 *     level = clip(sign(C) mag, -32768, 32767).  sum_abs_levels = sum of mag (HM's uiAbsSum, before the clip), nb_nonzero = number of
 *     levels != 0, both over the block (over its four units at width 64).
 *   Dequantisation.  inv = {40, 45, 51, 57, 64, 72}[rem], rs = 6 - (ts + per);  C' = (level inv + (1 << (rs - 1))) >> rs if rs > 0, else
 *     (level inv) << -rs;  clipped to [-32768, 32767].
 *   Inverse.  Vertical first: Z[y][k] = clip16((sum_l M[l][y] C'[l][k] + 64) >> 7);  then R[y][x] = clip16((sum_k M[k][x] Z[y][k] + 2048) >> 12).
 *   Reconstruction.  rec = clip(prediction + R, 0, 255);  sse_recon = sum (rec - target)^2, uint32 (at most 2.7e8 at width 64).
 *
 * The host twin: pure host code, the zero-tolerance yardstick of the device entry and what a CPU-only user calls.  predictions and
 * targets dense uint8 [n][width][width]; qps: nb_qps (1 .. 8) host ints in [0, 51].  Outputs, each NULL or: sses_recon, nb_nonzero,
 * sum_abs_levels uint32 [nb_qps][n]; recon uint8 [nb_qps][n][width][width].  n == 0 does nothing.  PNN_E_ARG + a line on stderr for a
 * width outside {4, 8, 16, 32, 64}, n < 0, NULL inputs with n > 0, a bad QP list, every output NULL. */
int pnn_trquant_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const int* qps, int nb_qps,
                     uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon);
/* One block, every stage, so that each can be looked at: coeffs = C, levels, dequant = C', residual = R, each NULL (not all) or int32
 * [width][width]; at width 64 each unit's 32 x 32 array lies where the unit lies in the block.  Same refusals; pure host code. */
int pnn_trquant_stages_host(const uint8_t* prediction, const uint8_t* target, int width, int qp, int32_t* coeffs, int32_t* levels,
                            int32_t* dequant, int32_t* residual);
/* pnn_trquant_host on the GPU, all n blocks and all QPs in ONE launch (the forward transform of a unit once, the rest per QP);
 * bit-identical to it.  d_* are device pointers, qps is a HOST array; asynchronous on `stream`; every argument error (those of the host
 * twin) is reported before the launch.  A context without models (pnn_create_empty) suffices.
 * Pairs: hand in the predictions the score call made from the decoded plane and the targets it copied from the original plane
 * (pnn_score_picture_pairs_device's d_pnn_u8 / d_hevc_pred and d_targets): residual and SSE are then against the original, the table
 * of that entry. */
int pnn_trquant_device(pnn_ctx* ctx, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const int* qps, int nb_qps,
                       uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels, uint8_t* d_recon, void* stream);

/* ---- the CABAC rate of the coded levels, HM's bit counter ----------------------------------------------- */

/* The entries above report how many levels survive and how large they are; HM decides by bits.  These report, per (QP, block), THE
 * FRACTIONAL BITS THAT HM-16.15's TEncSbac::codeCoeffNxN ADDS TO A TEncBinCABACCounter (m_fracBits) FOR THE LEVELS OF THE TRANSFORM
 * UNIT, WERE THE UNIT THE FIRST RESIDUAL OF AN I SLICE OF THAT QP: every context model starts each unit at its initial state
 * (ContextModel::init, H.265 9.3.2.2, initType 0, SliceQpY = the QP).  That is well defined open-loop; the running state of a slice is
 * not.  Unit: 2^-15 bit, uint64.  Luma, intra, 8-bit video, maxLog2TrDynamicRange 15; sign-data hiding (OFF in these entries, a flag
 * of the next group's), transform skip, transquant bypass, extended precision, persistent Rice adaptation and CABAC bypass alignment
 * are all OFF.  NOT COUNTED: cbf_luma (its context
 * depends on a transform tree that does not exist here), mode bits; RDOQ is an option of its own group below.  No lambda here either: these entries report bits; the
 * lambda and the cost D + lambda R over them are the second intra pass's, the last group of evaluator entries below.
 *   Units.  The transform units of the entries above: T = width up to 32; at width 64 the four 32 x 32 quadrants, each coded as a unit
 *     of its own (all contexts at their initial states again), bits added.  A unit whose levels are all zero costs 0.
 *   Scan.  0 diagonal, 1 horizontal, 2 vertical, generated as HM's initROM does (4 x 4 groups in scan order, the scan again inside a
 *     group).  From the block's intra mode by TComTU::getCoefScanIdx with MDCS_ANGLE_LIMIT 4: at T = 4 and T = 8 modes 22 .. 30
 *     (vertical +- 4) scan horizontally, modes 6 .. 14 (horizontal +- 4) vertically, every other mode diagonally; at T = 16 and 32
 *     always diagonally.  Without a mode array: diagonally.  The PNN has no mode: that its blocks are coded under the diagonal scan is
 *     THIS PROJECT'S DEFINITION.
 *   Bins, in codeCoeffNxN's order.  (1) The last significant position (x and y swapped under the vertical scan): per coordinate,
 *     group g = {0,1,2,3,4,4,5,5,6,6,6,6,7,7,7,7,8 x 8,9 x 8}[pos]: g bins 1 and, if g < the group of T - 1, a bin 0, bin k on context
 *     offset + (k >> shift), offset = 3 (L - 2) + ((L - 1) >> 2), shift = (L + 1) >> 2, of the lastX / lastY set; then (g - 2) >> 1
 *     bypass bins per coordinate with g > 3.  (2) Per 4 x 4 group from the last one back to the first: coded_sub_block_flag when the
 *     group is neither the last nor the first, on context (right or lower group coded ? 1 : 0); in a coded group (the first always
 *     counts as coded) the sig_coeff_flags from the position before the last one (from 15 in other groups) down to 0, the flag at 0
 *     inferred when the group was flagged and nothing else in it is set; context 0 at DC, else at T = 4 ctxIdxMap {0 1 4 5; 2 3 4 5;
 *     6 6 8 8; 7 7 8 8}, else first + (group is not the first ? 3 : 0) + cnt, first = 9 at T = 8 diagonal, 15 at T = 8 otherwise, 21
 *     above, cnt from the pattern right + 2 lower of the coded neighbour groups and the position (x, y) inside the group: pattern 0:
 *     x + y >= 3 ? 0 : x + y >= 1 ? 1 : 2; 1: y >= 2 ? 0 : y >= 1 ? 1 : 2; 2: the same of x; 3: 2.  Then for the first 8 levels of the
 *     group in coding order a greater-than-1 flag on context 4 set + c1, set = (group is not the first ? 2 : 0) + (the previous group
 *     with levels ended with c1 == 0), c1 = 1 at the group's start, 0 after a flag 1, else + 1 up to 3; one greater-than-2 flag, for
 *     the first level above 1, on context `set`; one bypass bin per sign; coeff_abs_level_remaining for every level >= its base (3
 *     until a level >= 2 has passed, then 2; 1 from the ninth level on) by xWriteCoefRemainExGolomb: value v = |level| - base at Rice
 *     parameter r: v < 3 << r: (v >> r) + 1 + r bypass bins, else 4 + 2 l - r with l = floor(log2(v - (3 << r) + (1 << r))); r starts
 *     each group at 0 and goes up by one, to 4 at most, after a level > 3 << r.
 *   Cost.  A context-coded bin costs entropyBits[state ^ bin] (HM's ContextModel::m_entropyBits, the FAST_BIT_EST table) and moves its
 *     context by H.265 table 9-41, as TEncBinCABACCounter::encodeBin does; a bypass bin costs 32768.
 * The numbers live in csrc/pnn_cabac_tables.h, whose lines host and device both compile.
 * Pinned to HM: the tables and context-selection functions piece by piece (tests/golden/hm_cabac_rate.npz); the whole of the above --
 * levels, scan of the mode, order of the bins, bits -- to HM's own transformNxN / getCoefScanIdx / codeCoeffNxN / invTransformNxN on
 * whole units (tests/golden/hm_unit_coding.npz), which host twin and kernel are each compared with.  Not pinned: cbf_luma, mode bits,
 * the running contexts of a slice.  (RDOQ: its own group below, tests/golden/hm_rdoq.npz.)
 *
 * pnn_trquant_host with the rate: modes NULL or uint8 [n], each in [0, 34] (0 planar, 1 DC, 2 .. 34 angular); rate NULL or uint64
 * [nb_qps][n].  Every other argument and refusal as there; also PNN_E_ARG for a mode above 34, for modes without rate, and `every
 * output NULL` now counts rate.  Pure host code, the zero-tolerance yardstick of the device entry. */
int pnn_trquant_rate_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                          int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon, uint64_t* rate);
/* The rate of ONE unit given its levels: int32 [t][t], t in {4, 8, 16, 32}, each level in [-32768, 32767]; scan 0, 1 or 2 (0 only at
 * t = 16 and 32); qp in [0, 51].  *rate in 2^-15 bit.  PNN_E_ARG + a line on stderr otherwise.  Pure host code. */
int pnn_cabac_rate_levels_host(const int32_t* levels, int t, int scan, int qp, uint64_t* rate);
/* pnn_trquant_rate_host on the GPU, in the ONE launch of pnn_trquant_device (which is this call with d_modes and d_rate NULL and
 * launches the kernel without the rate, bit-identical to what it was); bit-identical to the host twin.  d_modes NULL or a device uint8
 * [n] -- pnn_score_pictures_device's d_hevc_mode as it lies; the array is NOT read back, a value above 34 scans diagonally.  d_rate NULL
 * or device uint64 [nb_qps][n].  PNN_E_ARG before the launch for everything the host twin refuses but the mode values. */
int pnn_trquant_rate_device(pnn_ctx* ctx, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                            const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                            uint8_t* d_recon, uint64_t* d_rate, void* stream);

/* ---- sign-data hiding, as HM's quantiser does it with RDOQ 0 -------------------------------------------- */

/* With SignHideFlag 1 (HM's default) and RDOQ 0, xQuant hands every unit to TComTrQuant::signBitHidingHDQ, which reads the unit's
 * coefficients, its levels, the rounding remainders deltaU and the scan -- no context model, no lambda, no bit estimate (only the
 * variant inside xRateDistOptQuant needs those: it comes with RDOQ, in its own group below).  The entries below are the ones above with a flag
 * sign_data_hiding; with the flag 0 they ARE the ones above.  Everything of the two groups above holds unless changed here.
 *   Terms.  A group is a 4 x 4 coefficient group; `scan` is the unit's grouped scan as above (from the block's intra mode; diagonal
 *     without a mode array, hence for the PNN: this project's definition); position n = 0 .. 15 of group c is block position
 *     scan[16 c + n].
 *   Remainder.  tmp = |C| scale (64 bits), mag = (tmp + add) >> qbits, deltaU = (int32)((tmp - ((int64)mag << qbits)) >> (qbits - 8)):
 *     xQuant's line; qbits - 8 >= 8 for every T and QP.  (mag 2^qbits <= tmp + add < (mag + 1) 2^qbits and add = 171 2^(qbits - 9), so
 *     deltaU lies in [-86, 170].)
 *   Hiding, signBitHidingHDQ line for line.  Groups are visited from the highest scan index down.  In a group, last / first = the
 *     highest / lowest n with a nonzero level (last = -1: none), absSum = the signed sum of the levels from first to last (only its low
 *     bit is used).  The LAST GROUP is the first group met, going down, that has a nonzero level.  A group takes part when last - first
 *     >= 4 (SBH_THRESHOLD).  signbit = (level at first > 0 ? 0 : 1).  If signbit == (absSum & 1) nothing changes.  Otherwise every
 *     candidate n -- from last down to 0 in the last group, from 15 down to 0 in every other -- gets a cost and a change:
 *       nonzero level, deltaU > 0:                                    cost -deltaU, change +1
 *       nonzero level, deltaU <= 0, n == first and |level| == 1:      not allowed (cost INT32_MAX)
 *       nonzero level, deltaU <= 0, otherwise:                        cost deltaU, change -1
 *       zero level, n < first, (C >= 0 ? 0 : 1) != signbit:           not allowed
 *       zero level, any other case:                                   cost -deltaU, change +1
 *     The winner is the smallest cost under a strict < while n descends: of equal costs the HIGHEST n wins.  A level of 32767 or
 *     -32768 at the winner forces the change to -1.  The winner's level becomes level + change when C >= 0, level - change otherwise.
 *     (1) A participating group always has an allowed candidate: its position `last` holds a nonzero level and is not `first`, so
 *     neither forbidden row applies to it; HM's minPos = -1 cannot occur.  (2) HM's guard uiAbsSum >= 2 never changes a result: a
 *     group needs two nonzero levels to take part, and then uiAbsSum >= 2; the guard is not computed.
 *   What follows the levels.  nb_nonzero, the dequantisation, the reconstruction, sse_recon and the rate use the levels AFTER hiding.
 *     sum_abs_levels stays HM's uiAbsSum, the sum of mag BEFORE hiding and before the clip: HM does not update it either.
 *   Rate (codeCoeffNxN with beValid; transform skip, transquant bypass and RDPCM are off, so beValid is the flag): in every group
 *     whose FINAL levels have last - first >= 4 the sign of the level at `first`, the last one in coding order, is not coded: one bypass
 *     bin (32768) fewer.  Nothing else changes.
 *   Width 64: each 32 x 32 quadrant is hidden and rated as a unit of its own.
 *   Pinned to HM's own signBitHidingHDQ by recorded calls (tests/golden/hm_sign_hiding.npz), and -- the deltaU line, the hand-over
 *   from xQuant and the sign rule of the rate included -- to HM's own transformNxN and codeCoeffNxN on whole units with
 *   SignDataHidingEnabledFlag 1 (tests/golden/hm_unit_coding.npz).
 *
 * signBitHidingHDQ on ONE unit: levels int32 [t][t] in and out (each in [-32768, 32767]), coeffs and delta_u int32 [t][t] (delta_u from
 * the caller, any value but INT32_MIN), t in {4, 8, 16, 32}, scan 0, 1 or 2 (0 only at t = 16 and 32).  PNN_E_ARG + a line on stderr
 * otherwise and for a NULL pointer.  Pure host code. */
int pnn_sign_hide_unit_host(int32_t* levels, const int32_t* coeffs, const int32_t* delta_u, int t, int scan);
/* pnn_trquant_rate_host with the flag.  sign_data_hiding 0: that entry.  Nonzero: as defined above; modes are then allowed without
 * rate (the scan shapes the levels).  Every other refusal as there.  Pure host code, the zero-tolerance yardstick of the device entry. */
int pnn_trquant_sdh_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                         int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon, uint64_t* rate,
                         int sign_data_hiding);
/* pnn_trquant_stages_host under scan `scan` (0, 1, 2; 0 only at width >= 16) with the flag: also delta_u and levels_hidden, the levels
 * after hiding (equal to levels with the flag 0); dequant and residual come from levels_hidden.  Each output NULL (not all) or int32
 * [width][width].  Same refusals, and PNN_E_ARG for a bad scan. */
int pnn_trquant_stages_sdh_host(const uint8_t* prediction, const uint8_t* target, int width, int qp, int scan, int sign_data_hiding,
                                int32_t* coeffs, int32_t* levels, int32_t* delta_u, int32_t* levels_hidden, int32_t* dequant,
                                int32_t* residual);
/* pnn_cabac_rate_levels_host with the flag: the rate of the given levels when the hidden signs are not coded. */
int pnn_cabac_rate_levels_sdh_host(const int32_t* levels, int t, int scan, int qp, int sign_data_hiding, uint64_t* rate);
/* pnn_trquant_sdh_host on the GPU, in ONE launch; bit-identical to the host twin.  pnn_trquant_rate_device is this call with the flag 0
 * and launches the kernels it launched before, unchanged.  With the flag, the hiding runs one lane per scan position, 16 lanes per
 * group, between quantisation and dequantisation of each QP.  d_modes is then read with or without d_rate (a value above 34 scans
 * diagonally).  PNN_E_ARG before the launch for everything the host twin refuses but the mode values. */
int pnn_trquant_sdh_device(pnn_ctx* ctx, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                           const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                           uint8_t* d_recon, uint64_t* d_rate, int sign_data_hiding, void* stream);

/* ---- HM's second intra pass: the RD choice among the first-pass candidates and the PNN ------------------- */

/* The groups above each answer one of HM's questions about a prediction.  This one puts them together the way the encoder does: the
 * reference's hm_16_15_switch takes the first-pass list, appends the PNN as mode 35 if it is absent (TEncSearch.cpp:2476-2491),
 * transform-codes EVERY candidate and keeps the one of least distortion + lambda bits under a strict < in list order
 * (TEncSearch.cpp:2546-2605).  Per block and per QP:
 *   Candidates.  The list of pnn_hevc_mode_hads_hm_* called WITH the candidate prediction (35 competes on Hadamard cost): K =
 *     pnn_first_pass_list_size(width) entries in list order, slots 0 .. K - 1.  If 35 is not among them it is appended as slot K.
 *     K or K + 1 candidates in K + 1 slots; an unused slot K carries mode 255, cost +inf, and never wins.  HM also appends the most
 *     probable modes that are missing; they depend on the neighbours' coded modes, do not exist open-loop and ARE LEFT OUT, as
 *     modeBits * sqrtLambda is in the first pass.
 *   Prediction.  Modes 0 .. 34: pnn_hevc_intra_predict_hm(.., mode, smoothing, ..).  Mode 35: the given candidate prediction.
 *   Coding.  pnn_trquant_sdh_* exactly as it stands, that prediction against the target at every QP of the list, sign_data_hiding as
 *     given; the scan follows the candidate's mode, mode 35 scans diagonally.  D = sse_recon, R = rate >> 15: HM's whole written bits.
 *   Lambda.  lambda(QP) = 0.57 * 2^((QP - 12) / 3): TEncSlice::calculateLambda for an I slice, GOP size 1, 8-bit, no modifier -- what
 *     an all-intra configuration gives.  pnn_hm_intra_lambda computes it on the HOST in double; it travels in the kernel's argument
 *     block, so host twin and kernel use the same 64 bits.  lambdas: NULL (HM's) or the caller's own [nb_qps], each finite and >= 0.
 *   Cost.  J = (double) D + lambda * (double) R, TComRdCost::calcRdCost with DF_DEFAULT: one IEEE multiply and one IEEE add, each
 *     rounded once, never contracted into an FMA (contraction is switched off around the two operations in the kernel -- HIP's
 *     __dmul_rn / __dadd_rn alone do not prevent it -- and for the host twin's translation unit).  Pinned to calcRdCost's own bit
 *     patterns, triples that differ under an FMA included (tests/golden/hm_unit_coding.npz); lambda itself stays restated:
 *     calculateLambda cannot be called alone.
 *   Winner.  Slots 0 .. K in order under a strict <, starting from +inf: of equal costs the earlier slot wins, so an appended 35 loses
 *     every tie.  Where no cost is below +inf (a caller's lambda so large that every lambda R overflows) there is no winner: mode and
 *     slot 255, cost +inf, sse and rate 0.
 * STILL LEFT OUT: split flags (mode bits, cbf_luma and the appended MPMs are the option of the mode-signalling group below); transform skip (RDOQ, which campaigns run, is the option of the next group);
 * the transform quadtree (one unit per block, four quadrants at width 64, as in the transform-coding group); chroma; and the contexts
 * start cold for every candidate, as in the rate group.
 *
 * The lambda above; any int is accepted (the formula has no bound of its own). */
double pnn_hm_intra_lambda(int qp);
/* The host twin: pure host code composed of the host twins above plus the decision; the zero-tolerance yardstick of the device
 * entries.  patterns [n][pattern_h][pattern_w], targets and cand_pred [n][width][width], uint8; qps: nb_qps (1 .. 8) ints in [0, 51].
 * Outputs, each NULL (not all) or:
 *   cand_modes  uint8  [n][K + 1]             the slots' modes
 *   cand_costs  double [nb_qps][n][K + 1]     J per slot, +inf in an unused slot
 *   best_mode, best_slot  uint8 [nb_qps][n];  best_cost  double [nb_qps][n]
 *   best_sse    uint32 [nb_qps][n]            D of the winner
 *   best_rate   uint64 [nb_qps][n]            the winner's rate in 2^-15 bit, as pnn_trquant_sdh_host reports it (not shifted)
 * n == 0 does nothing.  PNN_E_ARG + a line on stderr for what the entries it is made of refuse (width, pattern sides, n < 0, NULL inputs
 * with n > 0, smoothing, QP list), for cand_pred NULL, every output NULL, a lambdas entry that is negative or not finite. */
int pnn_rd_pass_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                     const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                     uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost, uint32_t* best_sse,
                     uint64_t* best_rate);
/* The scratch of the device entries comes from the caller: the candidates' predictions, the replicated targets, the slots' modes, the
 * first-pass list and the per-slot SSE and rate.  Its size in bytes for n blocks (0 for a bad width, n < 0 or nb_qps outside 1 .. 8);
 * the pointer must be a multiple of 8.  The entries neither allocate nor keep anything. */
size_t pnn_rd_pass_workspace_bytes(int width, int n, int nb_qps);
/* pnn_rd_pass_host on the GPU, bit-identical to it; d_* are device pointers, qps and lambdas HOST arrays; asynchronous on `stream`;
 * every argument error (the host twin's; also d_workspace NULL, misaligned or workspace_bytes below pnn_rd_pass_workspace_bytes)
 * is reported before any launch.  Four launches: the first-pass kernel of pnn_hevc_mode_hads_hm_device (its list into the scratch),
 * rd_candidates_kernel (reads that list, writes the K + 1 predictions per block, the target once per slot and the slots' modes; an
 * unused slot gets the target as its prediction: a zero residual), the UNCHANGED launch of pnn_trquant_sdh_device on the n (K + 1) slots
 * with the slots' modes as its mode array, rd_decide_kernel.  A context without models (pnn_create_empty) suffices. */
int pnn_rd_pass_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                       const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                       uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost,
                       uint32_t* d_best_sse, uint64_t* d_best_rate, void* d_workspace, size_t workspace_bytes, void* stream);
/* The same from the evaluator's pictures: geometry, block order, masks, planes, checks and the read-back of d_rows / d_cols of
 * pnn_first_pass_picture_pairs_hm_device (reference samples from the CONTEXT plane, targets from the TARGET plane); d_cand_pred
 * [n][width][width] is what pnn_score_picture_pairs_device's d_pnn_u8 holds.  Equal to pnn_rd_pass_host on the dense patterns and
 * targets of the same blocks. */
int pnn_rd_pass_picture_pairs_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                     int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                     int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                     const double* lambdas, int sign_data_hiding, uint8_t* d_cand_modes, double* d_cand_costs,
                                     uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                                     uint64_t* d_best_rate, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- rate-distortion optimised quantisation: HM's quantiser with RDOQ 1 -------------------------------- */

/* Every group above is HM with RDOQ 0; the reference's configurations and campaigns run RDOQ 1, where TComTrQuant::xRateDistOptQuant
 * (TComTrQuant.cpp 2119-2661 of HM-16.15) picks every level by distortion + lambda bits.  The entries below are the transform-coding
 * and second-pass entries with an option rdoq; with rdoq 0 they ARE those entries.  Settings as above: luma, intra, I slice, 8 bit,
 * maxLog2TrDynamicRange 15, flat quantisation, no transform skip, extended precision, persistent Rice adaptation or adaptive QP
 * selection, 32-bit Intermediate_Int.  The definition lives in csrc/pnn_rdoq.h, whose lines host and device both compile.
 *   Bit estimates.  TEncSbac::estBit's tables for luma from the state a slice of the QP STARTS with -- the state the rate group codes
 *     every unit from; no state moves during RDOQ.  bits(i, b) = entropyBits[initial state of context i ^ b]:
 *       significantBits[k][b] = bits(sig context k, b), k as in the rate group (0 DC, 1 .. 8 at T = 4, 9 .. / 15 .. at T = 8, 21 .. above);
 *       m_greaterOneBits[k][b], k = 4 set + c1;  m_levelAbsBits[k][b], k = set;  significantCoeffGroupBits[k][b], k = 0, 1;
 *       lastXBits[g] = sum_{k < g} bits(lastX context offset + (k >> shift), 1) + (g < top ? bits(.. (g >> shift), 0) : 0), g = 0 .. top
 *         = 2 L - 1, the group of position T - 1; lastYBits alike; xGetRateLast adds 32768 ((g - 2) >> 1) per coordinate with g > 3;
 *       blockCbpBits[c][b] = bits(cbf context c, b), initial values 111 (c = 0) and 141 (c = 1).
 *   cbf context.  getCtxQtCbf: 1 at transform depth 0, else 0.  Width 8, 16, 32 (one unit of a 2N x 2N coding unit): 1.  Width 4 (HM
 *     reaches 4 x 4 only as N x N): 0.  The four quadrants at width 64: 0, THIS PROJECT'S DEFINITION, as the quadrants themselves are.
 *     The cbf bits enter RDOQ's decision only; the reported rate stays codeCoeffNxN's on the final levels, without cbf.
 *   Lambda.  The second pass's: pnn_hm_intra_lambda(QP) or the caller's lambdas [nb_qps]; with rdoq each must be finite and > 0.
 *   Per-QP constants, made on the HOST in double and handed to the kernel as they are: lambda; errScale = 2^15 * 2^(-2 ts) / scale /
 *     scale / 1 (setErrScaleCoeff's order; ts = 7 - L); rdFactor = (int64)(inv * inv * (1 << 2 per) / lambda / 16 / 1 + 0.5),
 *     saturated at 2^52 (lambda below about 5e-9; HM's conversion is undefined once the value leaves 64 bits: this project's definition).
 *   Arithmetic.  Every cost is an IEEE double, each operation rounded once, in HM's order, never contracted into a fused multiply-add.
 *   Per position (reverse scan; i = scan position, n = i % 16, group g = i / 16).  lLevelDouble = min(|C| scale, INT32_MAX - (1 <<
 *     (qbits - 1))); maxAbs = min(32767, (lLevelDouble + (1 << (qbits - 1))) >> qbits); cost0[i] = (double) lLevelDouble squared times
 *     errScale, added to blockUncoded.  In front of the first position with maxAbs > 0 (the LAST position, whose group is the last
 *     group) a position adds cost0 to base and its level is 0.  From there on xGetCodedLevel: at the last position the candidates are
 *     maxAbs and, if maxAbs > 1, maxAbs - 1, without a significance cost; elsewhere, with the sig context of the rate group (pattern from
 *     the groups RDOQ has left coded), level 0 at cost0 + lambda sig[0] competes when maxAbs < 3, and a level a costs err^2 errScale +
 *     lambda ICRate(a) + lambda sig[1], err = lLevelDouble - (a << qbits); the least cost under a strict <, maxAbs tried first.
 *     ICRate is xGetICRate: 32768 for the sign, plus, with base = (c1Idx < 8 ? 2 + (c2Idx < 1) : 1): for a >= base the bypass bins of
 *     a - base at the Rice parameter (the rate group's formula) and, while c1Idx < 8, greaterOne[ctx][1] and, while c2Idx < 1,
 *     levelAbs[set][1]; a == 1: greaterOne[ctx][0]; a == 2: greaterOne[ctx][1] + levelAbs[set][0].  Recorded per position: cost, the
 *     significance part costSig, deltaU = (lLevelDouble - (level << qbits)) >> (qbits - 8), rateIncUp / rateIncDown = ICRate(level +- 1)
 *     - ICRate(level) (level 0: rateIncUp = greaterOne[ctx][0]), sigRateDelta = sig[1] - sig[0] (0 at the last position).  Then the
 *     chain: Rice + 1 up to 4 after a level >= base above 3 << Rice; c1Idx + 1 per level; a level > 1 sets c1 = 0, c2Idx + 1; a level 1
 *     takes c1 up to 3; at n = 0 of a group other than the first, set = (g - 1 > 0 ? 2 : 0) + (c1 == 0) and c1, c1Idx, c2Idx, Rice start
 *     again.
 *   Per group, once the last position is passed (group 0 always counts as coded).  Without a level: base += lambda group[ctx][0] - the
 *     group's costSig sum.  With levels, below the last group: if no level lies above n = 0, costSig of n = 0 leaves base and the sum
 *     (the flag would be inferred); zero = base + lambda group[ctx][0] + sum cost0 - sum (cost - costSig) - sum costSig over the
 *     positions with a level (costSig over all), base += lambda group[ctx][1]; if zero < base the group is zeroed: base = zero, its
 *     levels 0, their cost = cost0, costSig = 0.  ctx = right or lower group coded.
 *   Best last position.  best = blockUncoded + lambda cbf[c][0]; base += lambda cbf[c][1].  From the last group down: base -= the
 *     group's flag cost; in a coded group, from n = 15 (from the last position) down: a zero level takes its costSig from base; a level
 *     gives total = base + lambda RateLast(x, y) - costSig (x and y swapped under the vertical scan), the new best under a strict <;
 *     a level > 1 ends the search; a level 1 leaves: base = base - cost + cost0.  Levels from the best last position on become 0 (all
 *     of them when nothing beat "nothing coded"); the others get the coefficient's sign.  sum_abs_levels = HM's uiAbsSum = the sum of
 *     the magnitudes kept here, BEFORE the hiding.
 *   Sign-data hiding with rdoq is RDOQ's own (lines 2530-2660), not signBitHidingHDQ.  Groups, first / last, the last group, the
 *     parity test and the candidates' range as in the hiding group above; costs are int64:
 *       nonzero level:  up = rdFactor (-deltaU) + rateIncUp;  down = rdFactor deltaU + rateIncDown - (|level| == 1 ? sigRateDelta : 0),
 *                       less 4 << 15 in the last group at n == last with |level| == 1;  up < down: cost up, change +1;  else change
 *                       -1 at cost down, not allowed when n == first and |level| == 1
 *       zero level:     cost rdFactor (-|deltaU|) + (1 << 15) + rateIncUp + sigRateDelta, change +1; not allowed when n < first and
 *                       the coefficient's sign differs from signbit
 *     deltaU and the rate increments are those of the level the WALK chose (a zeroed group keeps them).  Strict < while n descends:
 *     the highest n wins a tie.  HM's guard uiAbsSum >= 2 never decides here either: a group that hides holds two levels.
 *   Downstream nothing changes: nb_nonzero, dequantisation, inverse transform, reconstruction, sse_recon and the rate use the final
 *     levels.  Width 64 runs each quadrant as a unit of its own.
 *   Pinned to HM's own transformNxN with RDOQ on, est-bits tables included (tests/golden/hm_rdoq.npz).
 *
 * pnn_trquant_sdh_host with the option: rdoq 0 is that entry (lambdas is not read).  Nonzero: as above; modes are then allowed
 * without rate or hiding.  PNN_E_ARG also for a lambdas entry that is not finite or not > 0. */
int pnn_trquant_rdoq_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                          int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon, uint64_t* rate,
                          int sign_data_hiding, int rdoq, const double* lambdas);
/* pnn_trquant_stages_sdh_host with the option, under lambda and cbf context cbf_ctx (0 or 1, whatever the width): levels = what RDOQ
 * leaves in front of its hiding, levels_hidden = after it, delta_u stays 0.  With rdoq 0 lambda and cbf_ctx are not read. */
int pnn_trquant_stages_rdoq_host(const uint8_t* prediction, const uint8_t* target, int width, int qp, int scan, int sign_data_hiding,
                                 int rdoq, double lambda, int cbf_ctx, int32_t* coeffs, int32_t* levels, int32_t* delta_u,
                                 int32_t* levels_hidden, int32_t* dequant, int32_t* residual);
/* xRateDistOptQuant on ONE unit: coeffs int32 [t][t], each in [-32768, 32767], t in {4, 8, 16, 32}, scan 0, 1 or 2 (0 only at t = 16
 * and 32), qp in [0, 51], lambda finite and > 0, cbf_ctx 0 or 1 -> levels int32 [t][t] and *abs_sum (NULL or HM's uiAbsSum).
 * PNN_E_ARG + a line on stderr otherwise.  Pure host code. */
int pnn_rdoq_unit_host(const int32_t* coeffs, int t, int scan, int qp, double lambda, int cbf_ctx, int sign_data_hiding, int32_t* levels,
                       int32_t* abs_sum);
/* The bit estimates of unit size t at QP qp, 184 int32: [80][2] per context of the rate group's numbering (last-position contexts:
 * the single bins), lastXBits [10], lastYBits [10] (entries above 2 log2 t - 1 are 0), blockCbpBits [2][2]. */
int pnn_rdoq_est_bits_host(int t, int qp, int32_t* est_bits);
/* pnn_trquant_rdoq_host on the GPU, in ONE launch; bit-identical to the host twin.  With rdoq 0 it launches the kernels
 * pnn_trquant_sdh_device launched before, unchanged.  lambdas is a HOST array.  PNN_E_ARG before the launch for everything the host twin
 * refuses but the mode values. */
int pnn_trquant_rdoq_device(pnn_ctx* ctx, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                            const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                            uint8_t* d_recon, uint64_t* d_rate, int sign_data_hiding, int rdoq, const double* lambdas, void* stream);
/* The second intra pass with the option: the lambda that decides also quantises, the coding of the K + 1 slots is the RDOQ form.  rdoq
 * 0: the entries above.  Nonzero: PNN_E_ARG also for a lambdas entry that is not > 0.  The workspace is that of
 * pnn_rd_pass_workspace_bytes. */
int pnn_rd_pass_rdoq_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                          const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                          int rdoq, uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost,
                          uint32_t* best_sse, uint64_t* best_rate);
int pnn_rd_pass_rdoq_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                            const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                            int rdoq, uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot,
                            double* d_best_cost, uint32_t* d_best_sse, uint64_t* d_best_rate, void* d_workspace, size_t workspace_bytes,
                            void* stream);
int pnn_rd_pass_rdoq_picture_pairs_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                          int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                          int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                          const double* lambdas, int sign_data_hiding, int rdoq, uint8_t* d_cand_modes, double* d_cand_costs,
                                          uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                                          uint64_t* d_best_rate, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- mode signalling: the side information HM's intra search charges, and the candidates it adds ---------- */

/* The second pass above compares candidates on D + lambda R(coefficients) alone.  hm_16_15_switch also charges each candidate its
 * mode bits and cbf_luma, ranks the first pass on SATD + modeBits sqrt(lambda), and appends the most probable modes the list lacks
 * before it appends 35 (TEncSearch.cpp:2427-2492 of the switch tree).  The entries below are the second-pass entries with an option
 * `signalling`; with 0 they ARE those entries.  The definition lives in csrc/pnn_mode_signal.h, whose lines host and device compile.
 *   Neighbours.  left_modes / above_modes: NULL (every block: none) or uint8 [n], a neighbour's coded mode 0 .. 35 or 255 = no
 *     neighbour or not intra, which HM treats as DC.  HM also treats an above neighbour outside the CTU as DC: a caller who wants that
 *     rule passes 255 there.  Any other value is PNN_E_ARG; so is 35 with pnn_flag 0.
 *   MPMs.  TComDataCU::getIntraDirPredictor of the switch tree: left == above: an angular mode a < 35 gives {a, 2 + (a + 29) % 32,
 *     2 + (a - 1) % 32}, anything else (planar, DC, 35 twice) {0, 1, 26}; num_append 1.  left != above, num_append 2: one of them 35 and
 *     the other o: {o, 0, 1} for o > 1, {1, 0, 26} for o = 1, {0, 1, 26} for o = 0; else {left, above, t}, t = 0 if neither is planar,
 *     else 26 if left + above < 2, else 1.  Without a neighbour 35 this is hm_16_15_regular's.
 *   Mode bits, in 2^-15 bit as a TEncBinCABACCounter adds them for one unit (TEncSbac::codeIntraDirLumaAng): with pnn_flag the flag on
 *     its own context (initial value 154): mode 35 costs that bin alone; a regular mode the bin for 0, then prev_intra_luma_pred_flag on
 *     its context (184) and mpm_idx, 1 bypass bin for mpm[0], 2 for mpm[1] and mpm[2], or the 5 bypass bins of the remainder (HM sorts
 *     the three ascending to form its value; the value costs nothing).  Bypass bins cost 32768.  Both contexts start from the state an
 *     I slice of the QP begins with (cold contexts, as the rate group).  pnn_flag 0 leaves the first flag out: regular HM.
 *   cbf_luma.  One bin on context getCtxQtCbf selects: 1 at transform depth 0 (width 8, 16, 32), 0 at depth 1 (width 4), initial
 *     values 141 and 111, cold.  A unit without a level pays the bin for 0 and no coefficient bits, one with levels the bin for 1
 *     plus the rate.  Width 64: each of the four 32 x 32 quadrants is a unit at depth 1 and pays its own bin on context 0, four bins
 *     per candidate (the quadrants are this project's definition, as in the transform-coding group).
 *   First pass.  cost = (double) SATD + (double) (mode bits >> 15) * sqrt(lambda), sqrt taken once on the host in double
 *     (TComRdCost::setLambda); one IEEE multiply and one IEEE add, never fused.  The list is xUpdateCandList over modes 0 .. 35 in that
 *     order under a strict <, K entries.  So the list depends on the QP and on the neighbours.
 *   Slots.  S = K + 3 = pnn_rd_pass_slot_count(width, 1): the list, then mpm[0 .. num_append - 1] where the list lacks them, in that
 *     order, then 35 if absent; unused slots carry mode 255 and cost +inf.
 *   Second pass.  R = (mode bits + cbf bin + rate of the levels) >> 15, ONE shift over the sum; J = D + lambda R and the winner rule
 *     as above.  A slot is coded at its own QP only.
 * LEFT OUT: part size, split and subdivision flags (equal for all candidates of a block); the interleaving of the four units' flags in
 * an N x N coding unit; chroma; running contexts; transform skip; the transform quadtree.  (The substitution codec: the next group.) */
int pnn_rd_pass_slot_count(int width, int signalling);      /* K + 1 or K + 3; -1 for a bad width */
/* The unit entry.  Outputs, each NULL (not all) or: mpm uint8 [n][3]; num_append uint8 [n]; mode_frac_bits uint32 [n][36] (entry 35
 * is 0 with pnn_flag 0); cbf_frac_bits uint32 [2 contexts][2 values] of the QP.  PNN_E_ARG + a line on stderr for n < 0, a QP outside
 * [0, 51], a bad neighbour mode.  Pure host code. */
int pnn_intra_mode_signal_host(const uint8_t* left_modes, const uint8_t* above_modes, int n, int qp, int pnn_flag, uint8_t* mpm,
                               uint8_t* num_append, uint32_t* mode_frac_bits, uint32_t* cbf_frac_bits);
/* The first pass with the mode-bit term, the candidate competing as 35 (cand_pred is required).  Outputs, each NULL (not all) or:
 * list_modes uint8 [nb_qps][n][K]; list_costs double [nb_qps][n][K]; slot_modes uint8 [nb_qps][n][K + 3].  Pure host code. */
int pnn_first_pass_signal_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                               const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                               const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* list_modes, double* list_costs,
                               uint8_t* slot_modes);
/* pnn_rd_pass_rdoq_host with the option.  signalling 0: that entry (the neighbours are not read; first_pass_costs and best_side_rate
 * must be NULL).  Nonzero: as above; cand_modes is then uint8 [nb_qps][n][K + 3] and cand_costs double [nb_qps][n][K + 3]; the added
 * outputs are first_pass_costs double [nb_qps][n][K] (the list's costs) and best_side_rate uint64 [nb_qps][n], the winner's mode bits
 * plus cbf bin in 2^-15 bit (best_rate stays the rate of its levels).  The twin is a composition of the host twins above. */
int pnn_rd_pass_signal_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                            const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                            int rdoq, int signalling, const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* cand_modes,
                            double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost, uint32_t* best_sse,
                            uint64_t* best_rate, double* first_pass_costs, uint64_t* best_side_rate);
/* The device entries' scratch (signalling 0: pnn_rd_pass_workspace_bytes; 0 for what the entries refuse). */
size_t pnn_rd_pass_signal_workspace_bytes(int width, int n, int nb_qps, int signalling);
/* pnn_rd_pass_signal_host on the GPU, bit-identical to it.  signalling 0 forwards to pnn_rd_pass_rdoq_device.  Nonzero: 2 + 3 nb_qps
 * launches on `stream`: the unchanged first-pass kernel (asked for the Hadamard costs, no list), signal_list_kernel (all QPs), then per
 * QP the slots form of rd_candidates_kernel, the unchanged launch of pnn_trquant_rdoq_device with that one QP, and
 * rd_decide_signal_kernel, all on the same scratch.  At width 64 the slots form writes every slot as its four quadrants and the
 * transform launch is the width-32 one on 4 n (K + 3) blocks under cbf context 0 -- the same units, now with a count of levels each.
 * d_left_modes / d_above_modes are DEVICE arrays or NULL; when one is given both are read back and checked behind ONE wait for the
 * stream (as the picture forms wait for their positions), so that every refusal comes before any launch; with both NULL the dense
 * entry stays asynchronous. */
int pnn_rd_pass_signal_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                              const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                              int rdoq, int signalling, const uint8_t* d_left_modes, const uint8_t* d_above_modes, uint8_t* d_cand_modes,
                              double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                              uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace,
                              size_t workspace_bytes, void* stream);
int pnn_rd_pass_signal_picture_pairs_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                            int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                            int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                            const double* lambdas, int sign_data_hiding, int rdoq, int signalling, const uint8_t* d_left_modes,
                                            const uint8_t* d_above_modes, uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode,
                                            uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse, uint64_t* d_best_rate,
                                            double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace, size_t workspace_bytes,
                                            void* stream);

/* ---- the substitution codec: HM's own intra search with the PNN in the place of mode 18; mode statistics ---------- */

/* hm_16_15_substitution keeps HM's 35 luma modes and lets the PNN's block stand for mode 18 (predIntraAng, TComPrediction.cpp:506-556
 * of that tree); its search loop (TEncSearch.cpp:2325-2584) is otherwise HM's.  The entries below are the second-pass entries of the
 * group above with one more argument, `codec`: 0 is the switch codec -- they then ARE those entries, byte for byte -- and 1 the
 * substitution codec, defined by csrc/pnn_mode_signal.h (list_and_slots_substitution) as follows.  Any other codec is PNN_E_ARG.
 *   Modes.  0 .. 34 only.  Mode 18's prediction is the caller's candidate (cand_pred, required), every other mode's is
 *     pnn_hevc_intra_predict_hm's with the given `smoothing`.  Mode 35 does not exist and appears in no output.
 *   Neighbours.  0 .. 34 or 255; 35 is PNN_E_ARG.  A neighbour 18 is an ordinary angular mode (equal neighbours 18: MPMs 18, 17, 19).
 *   MPMs and bits.  getIntraDirPredictor and codeIntraDirLumaAng of that tree are hm_16_15_regular's: the MPMs above without a
 *     neighbour 35, the mode bits above with pnn_flag 0 (prev_intra_luma_pred_flag, mpm_idx or the remainder's 5 bypass bins, no flag
 *     bin) -- what pnn_intra_mode_signal_host returns with pnn_flag 0.  cbf_luma as above.  Cold contexts.
 *   First pass.  cost = (double) SATD + (double) (mode bits >> 15) * sqrt(lambda) over modes 0 .. 34 in that order, mode 18's SATD being
 *     the candidate's Hadamard cost; xUpdateCandList's rule and the unfused arithmetic as above.
 *   Slots.  S = K + 2: the K list entries, then mpm[0 .. num_append - 1] where the list lacks them, then 255.  Nothing is appended for
 *     the PNN: if 18 is neither listed nor an appended MPM it is not coded.
 *   Coding.  The transform coding above with the slot's mode as its scan mode (18 scans diagonally, HM's getCoefScanIdx); sign-data
 *     hiding and RDOQ as given.
 *   Second pass.  R = (mode bits + cbf bin + rate) >> 15, J = D + lambda R, strict < in slot order; width 64 by quadrants as above.
 *   Signalling.  codec 1 requires signalling nonzero (HM never searches without the mode bits); otherwise PNN_E_ARG.
 *   No context.  Where the codec finds no usable context (contextFlag false) its PNN predicts zeros.  That stays the caller's business:
 *     a caller models it by passing a zero candidate for such a block.
 * Argument order: the *_signal_* signatures with `codec` behind above_modes, in front of the outputs. */
int pnn_rd_pass_codec_slot_count(int width, int signalling, int codec);   /* K + 1, K + 3; codec 1: K + 2; -1 for what is refused */
size_t pnn_rd_pass_codec_workspace_bytes(int width, int n, int nb_qps, int signalling, int codec);   /* 0 for what the entries refuse */
/* The first pass.  codec 0: pnn_first_pass_signal_host.  codec 1: slot_modes is uint8 [nb_qps][n][K + 2].  Pure host code. */
int pnn_first_pass_codec_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                              const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                              const uint8_t* left_modes, const uint8_t* above_modes, int codec, uint8_t* list_modes, double* list_costs,
                              uint8_t* slot_modes);
/* The second pass.  codec 1: cand_modes uint8 and cand_costs double [nb_qps][n][K + 2]; every other output as with signalling.  The
 * host twin composes the host twins above and the header, never fusing the cost's multiply and add. */
int pnn_rd_pass_codec_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                           const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                           int rdoq, int signalling, const uint8_t* left_modes, const uint8_t* above_modes, int codec, uint8_t* cand_modes,
                           double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost, uint32_t* best_sse,
                           uint64_t* best_rate, double* first_pass_costs, uint64_t* best_side_rate);
/* pnn_rd_pass_codec_host on the GPU, bit-identical to it.  codec 1: the 2 + 3 nb_qps launches of pnn_rd_pass_signal_device with
 * substitution_list_kernel, the K + 2 slots form of rd_candidates_kernel (mode 18 reads d_cand_pred) and the decision without the flag
 * bin; the first-pass and transform launches are the unchanged ones.  Every refusal -- a bad codec, a neighbour 35, signalling 0, a
 * NULL candidate, a workspace below pnn_rd_pass_codec_workspace_bytes and those of the group above -- comes before any launch. */
int pnn_rd_pass_codec_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                             const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                             int rdoq, int signalling, const uint8_t* d_left_modes, const uint8_t* d_above_modes, int codec, uint8_t* d_cand_modes,
                             double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                             uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace,
                             size_t workspace_bytes, void* stream);
int pnn_rd_pass_codec_picture_pairs_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                           int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                           const double* lambdas, int sign_data_hiding, int rdoq, int signalling, const uint8_t* d_left_modes,
                                           const uint8_t* d_above_modes, int codec, uint8_t* d_cand_modes, double* d_cand_costs,
                                           uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                                           uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace,
                                           size_t workspace_bytes, void* stream);
/* Mode statistics of a second pass, either codec: the tables the reference's codecs accumulate per mode (m_nbFastSelections,
 * m_nbFastWins, m_nbRDWins) for the blocks of ONE width.  slot_modes: the cand_modes of a second-pass entry, uint8 [n][slots] shared
 * by the QPs (per_qp 0: the entries without signalling) or [nb_qps][n][slots] (per_qp nonzero); best_mode uint8 [nb_qps][n]; slots 1
 * to 16.  stats uint32 [nb_qps][3][36]: [0] fast selections, the mode occupies a used slot (appended MPMs and 35 included: HM counts
 * after the appends); [1] fast wins, the mode is in slot 0; [2] RD wins, the mode is best_mode.  A value above 35 (255: an unused
 * slot, a block without a winner) counts nowhere.  m_cumNbModesForRD is the sum of [0] and m_nbFastRDRuns is n: no entry computes them.
 * The device entry zeroes d_stats on `stream`, then one launch (mode_stats_kernel) adds each workgroup's counts: integer sums, the same
 * whatever the order.  PNN_E_ARG for n < 0, slots outside [1, 16], nb_qps outside [1, 8], a NULL output or (n > 0) NULL inputs. */
int pnn_rd_pass_mode_stats_host(const uint8_t* slot_modes, int per_qp, int slots, const uint8_t* best_mode, int n, int nb_qps, uint32_t* stats);
int pnn_rd_pass_mode_stats_device(pnn_ctx* ctx, const uint8_t* d_slot_modes, int per_qp, int slots, const uint8_t* d_best_mode, int n,
                                  int nb_qps, uint32_t* d_stats, void* stream);

/* ---- transform skip: HM-16.15's second form of a 4 x 4 luma unit, as intra_main_rext.cfg switches it on
 * (TransformSkip 1, TransformSkipFast 1, RDOQTS 1), for the transform coding above.  Width 4 only: Log2MaxTransformSkipBlockSize is 2.
 * 8-bit luma, maxLog2TrDynamicRange 15; rotation, RDPCM, extended precision, transform_skip_context, scaling lists and transquant
 * bypass off.
 *   Forward (xTransformSkip): coefficient = residual << 5.  Quantisation, hiding, RDOQ (RDOQTS = RDOQ) and dequantisation: the
 *     transform coding's, on those coefficients, under the unit's scan; nothing in them reads the flag.
 *   Inverse (xITransformSkip): residual' = (coefficient' + 16) >> 5; reconstruction and SSE as in the transform coding.
 *   Rate: codeCoeffNxN with the PPS flag on codes transform_skip_flag in front of the levels of every 4 x 4 unit WITH a level -- one
 *     bin of a context of its own (I-slice initial value 139) from the state the QP starts with, value 0 for the transformed form --;
 *     a unit without a level codes neither.
 *   Decision (xRecurIntraCodingLumaQT, checkTransformSkip), per unit and QP: J = D + lambda (R >> 15), one multiply and one add,
 *     R = mode_bits + (charge_cbf: the cbf_luma bin of the form's cbf, context 0) + (cbf 1: flag bin + level bits); the transformed
 *     form first, the skipped one second, forbidden when its cbf is 0; strict <, so a tie stays transformed.  cbf = a nonzero level.
 *   Pinned to HM's own transformNxN / invTransformNxN / codeCoeffNxN / codeTransformSkipFlags (tests/golden/hm_transform_skip.npz).
 *
 * pnn_tskip_unit_host, ONE unit: residual int32 [4][4] in [-255, 255], scan 0 .. 2, qp in [0, 51], transform_skip 0 (the transformed
 * form: the transform coding's stages) or 1 -> each NULL or: coeffs, levels (the final ones), residual_back int32 [4][4], *abs_sum HM's
 * uiAbsSum, *bits what codeCoeffNxN adds with the PPS flag on (0 without a level), flag_bins [2] the flag's bin alone for 0 and 1.
 * lambda is read with rdoq only (finite, > 0).  Pure host code. */
int pnn_tskip_unit_host(const int32_t* residual, int scan, int qp, int sign_data_hiding, int rdoq, double lambda, int transform_skip,
                        int32_t* coeffs, int32_t* levels, int32_t* abs_sum, int32_t* residual_back, uint64_t* bits, uint64_t* flag_bins);
/* pnn_trquant_rdoq_host with the option.  transform_skip 0: that entry, byte for byte (ts_flag, where given, is zeroed).  1, forced:
 * every unit in its skipped form.  2, decide: both forms, the rule above per unit and QP under lambdas (NULL: pnn_hm_intra_lambda of
 * each QP; the same lambda quantises with rdoq), mode_bits NULL (0) or uint32 [nb_qps][n] in 2^-15 bit, charge_cbf 0 or 1.  Outputs as
 * pnn_trquant_rdoq_host's, of the kept form: rate = the levels' bits + the flag bin, 0 without a level; ts_flag NULL or uint8
 * [nb_qps][n] (forced: 1 everywhere; with option 0 one of the other five outputs is needed, as that entry asks).  Modes are allowed
 * whatever the outputs.  PNN_E_ARG also for: a nonzero option at a width other
 * than 4, an option outside 0 .. 2, charge_cbf outside 0 .. 1, with decide or rdoq a lambdas entry that is not finite or not > 0. */
int pnn_trquant_tskip_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                           int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon, uint64_t* rate,
                           int sign_data_hiding, int rdoq, const double* lambdas, int transform_skip, const uint32_t* mode_bits, int charge_cbf,
                           uint8_t* ts_flag);
/* The same on the GPU, bit-identical to the host twin.  transform_skip 0: pnn_trquant_rdoq_device's launch, unchanged; the workspace is
 * not read and ts_flag, where given, is zeroed on the stream.  1: tskip4_kernel into the workspace, tskip_decide_kernel out of it (2
 * launches); 2: the unchanged transform-coding launch and tskip4_kernel into the workspace, then tskip_decide_kernel (3 launches).
 * d_workspace: at least pnn_trquant_tskip_workspace_bytes(width, n, nb_qps) bytes of device memory at a multiple of 16 (0 for a width
 * other than 4 or bad sizes), needed with a nonzero option only.  d_mode_bits is a DEVICE array, qps and lambdas are HOST arrays.  Every
 * refusal (the host twin's but the mode values, a NULL, misaligned or short workspace) comes before any launch. */
size_t pnn_trquant_tskip_workspace_bytes(int width, int n, int nb_qps);
int pnn_trquant_tskip_device(pnn_ctx* ctx, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                             const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                             uint8_t* d_recon, uint64_t* d_rate, int sign_data_hiding, int rdoq, const double* lambdas, int transform_skip,
                             const uint32_t* d_mode_bits, int charge_cbf, uint8_t* d_ts_flag, void* d_workspace, size_t workspace_bytes,
                             void* stream);

/* The second intra pass with the option, for both codecs: pnn_rd_pass_codec_*'s arguments with transform_skip (0 or 1) behind `codec`
 * and the output best_ts_flag (NULL or uint8 [nb_qps][n]) behind best_side_rate.  signalling is required (PNN_E_ARG without), whatever
 * the option.  transform_skip 0: the pass of pnn_rd_pass_codec_* with signalling; best_ts_flag, where given, is zeroed.  1, width 4
 * only: per QP every slot is coded in both forms and decided per slot by the rule above (mode_bits = the slot's mode bits under the
 * block's MPMs, charge_cbf 1, the QP's lambda, which must be finite and > 0); the slots' merged D, count and R (with the flag bin)
 * then go to the unchanged decision.  cand_costs, best_* are those of the merged slots; best_ts_flag is the winning slot's flag (0
 * for a block without a winner).  Device: per QP 4 more launches (tskip4_kernel, the slots' mode bits, tskip_decide_kernel in place,
 * the winners' flags); the workspace is pnn_rd_pass_tskip_workspace_bytes (pnn_rd_pass_codec_workspace_bytes with the option 0; 0
 * for what the entries refuse).  Every refusal comes before any launch. */
int pnn_rd_pass_tskip_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                           const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                           int rdoq, int signalling, const uint8_t* left_modes, const uint8_t* above_modes, int codec, int transform_skip,
                           uint8_t* cand_modes, double* cand_costs, uint8_t* best_mode, uint8_t* best_slot, double* best_cost,
                           uint32_t* best_sse, uint64_t* best_rate, double* first_pass_costs, uint64_t* best_side_rate, uint8_t* best_ts_flag);
size_t pnn_rd_pass_tskip_workspace_bytes(int width, int n, int nb_qps, int signalling, int codec, int transform_skip);
int pnn_rd_pass_tskip_device(pnn_ctx* ctx, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                             const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                             int rdoq, int signalling, const uint8_t* d_left_modes, const uint8_t* d_above_modes, int codec, int transform_skip,
                             uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost,
                             uint32_t* d_best_sse, uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate,
                             uint8_t* d_best_ts_flag, void* d_workspace, size_t workspace_bytes, void* stream);
int pnn_rd_pass_tskip_picture_pairs_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                           int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                           const double* lambdas, int sign_data_hiding, int rdoq, int signalling, const uint8_t* d_left_modes,
                                           const uint8_t* d_above_modes, int codec, int transform_skip, uint8_t* d_cand_modes,
                                           double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost,
                                           uint32_t* d_best_sse, uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate,
                                           uint8_t* d_best_ts_flag, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- the coding tree: the decision of TEncCu::xCompressCU between a coding unit and its four sub-units, and at
 * 8 x 8 between SIZE_2Nx2N and SIZE_NxN, from the winners the second pass left at every aligned block of the five widths.  HM-16.15
 * regular tree, I slice, luma only (the reference codes its luminance sets as 4:0:0); CTU 64, minimum CU 8 (MaxPartitionDepth 4); PCM,
 * transquant bypass, cu_qp_delta and AMP off; whole CTUs only.  The quadtree of TRANSFORM units is not part of it.
 *   Nodes.  85 CU nodes per CTU, depth d = 0 .. 3 of size 64 >> d; below each depth-3 node four 4 x 4 prediction units.  Every per-CTU
 *     array is in HM's z-order, depth by depth: 1 + 4 + 16 + 64 nodes (node i of depth d has the children 4 i .. 4 i + 3 one depth
 *     down); 256 units, the four of a CU adjacent.  Cell z of a 64-entry map is the 8 x 8 cell whose x has bit j at bit 2 j of z and
 *     whose y has bit j at bit 2 j + 1.
 *   Leaves.  Per width w = 4, 8, 16, 32, 64 (the order of every per-width argument), each [nb_qps][n_ctu][(64 / w)^2]: dist uint32, the
 *     winner's SSE; rate uint64 in 2^-15 bit, the winner's rate + side rate (mode bits and cbf inside); optionally mode uint8.
 *   Depth 3, no neighbour involved.  2N x 2N: D = dist_8, F = rate_8 + the part_mode bin of value 1.  N x N: D = the four dist_4, F =
 *     the four rate_4 + the bin of value 0.  The bin is one bin of the part-size model, context 0, from the state an I slice of the QP
 *     starts with.  J = (double) D + lambda * (double) (F >> 15): one IEEE multiply and one IEEE add, never fused.  2N x 2N first,
 *     N x N second, strict <: a tie stays 2N x 2N.
 *   Depths 2, 1, 0, in z-order post-order.  Unsplit: D and F of the node's own leaf + the split_cu_flag bin of value 0.  Split: the
 *     four children's chosen D and F (at depth 3 the winner above, which codes no split flag) + the bin of value 1.  Unsplit first,
 *     strict <: a tie stays unsplit.  The children's F are summed exactly; the shift by 15 happens once per comparison.
 *   Context of split_cu_flag (TComDataCU::getCtxSplitFlag): [left available and its CU depth > d] + [above available and its CU depth
 *     > d], "left" the CU that covers the sample left of the node's top-left sample, "above" the one over it.  Inside the CTU the depth
 *     comes from an 8 x 8 map of minimum-CU cells into which a subtree writes its final depth when its root is decided; outside from
 *     left_depths / above_depths, uint8 [nb_qps][n_ctu][8], one cell per 8 samples along the edge (top to bottom, left to right),
 *     0 .. 3 or 255 = not available; NULL: nothing available.  No CTU's result is chained into the next CTU's edge here: that is
 *     "the coding tree over a picture" below.
 *   The three contexts start from the state an I slice of the QP begins with (initial values 139, 141, 157; part size 184).
 *   Where this differs from the tree (whole bits per CU, the counter's carried fraction, running contexts): DESIGN.md section 5q.
 * Outputs, each NULL or: cu_depths uint8 [nb_qps][n_ctu][64], the final map; part_nxn uint8 [nb_qps][n_ctu][64], 1 where the cell is
 * an 8 x 8 CU coded N x N; node_costs double [nb_qps][n_ctu][85][2], [0] unsplit (depth 3: 2N x 2N) and [1] split (depth 3: N x N) --
 * both alternatives exist at every node of this setting, +inf is reserved for one that does not; ctu_costs double, ctu_dists and
 * ctu_rates uint64 [nb_qps][n_ctu], the root's chosen J, D and F; selected uint32 [nb_qps][5], the blocks of each width in the chosen
 * partitions (an N x N CU counts four of width 4); selected_pnn uint32 [nb_qps][5], those of them whose mode equals pnn_mode (35 for
 * the switch codec, 18 for substitution; 0 .. 255).  lambdas NULL: pnn_hm_intra_lambda of each QP.
 * PNN_E_ARG, before any launch: nb_qps outside 1 .. 8 or a QP outside [0, 51]; n_ctu < 1; a missing leaf array (dists, rates or one of
 * their five entries NULL; modes given with a NULL entry); a lambda not finite or < 0; an edge depth outside 0 .. 3 / 255; selected_pnn
 * without modes; no output; pnn_mode outside [0, 255].
 * pnn_cu_tree_device: the same on leaves in device memory, bit-identical; dists, rates and modes are HOST arrays of five device
 * pointers, qps and lambdas HOST arrays.  Asynchronous on `stream` and without allocation on the device (with edges it first reads
 * them back and waits, to check them): the two count outputs are zeroed on the stream, then ONE launch.  Also PNN_E_ARG for an array
 * that is not aligned to its element.
 * pnn_cu_tree_bins_host: the bins' bits at one QP in 2^-15 bit, out [8]: split_cu_flag [2 ctx + value] for contexts 0 .. 2, then
 * part_mode of value 0 (N x N) and 1 (2N x 2N).  Pinned to HM's own counter (tests/golden/hm_cu_tree.npz). */
int pnn_cu_tree_host(const int* qps, int nb_qps, const double* lambdas, int n_ctu, const uint32_t* const* dists, const uint64_t* const* rates,
                     const uint8_t* const* modes, const uint8_t* left_depths, const uint8_t* above_depths, int pnn_mode, uint8_t* cu_depths,
                     uint8_t* part_nxn, double* node_costs, double* ctu_costs, uint64_t* ctu_dists, uint64_t* ctu_rates, uint32_t* selected,
                     uint32_t* selected_pnn);
int pnn_cu_tree_device(pnn_ctx* ctx, const int* qps, int nb_qps, const double* lambdas, int n_ctu, const uint32_t* const* d_dists,
                       const uint64_t* const* d_rates, const uint8_t* const* d_modes, const uint8_t* d_left_depths,
                       const uint8_t* d_above_depths, int pnn_mode, uint8_t* d_cu_depths, uint8_t* d_part_nxn, double* d_node_costs,
                       double* d_ctu_costs, uint64_t* d_ctu_dists, uint64_t* d_ctu_rates, uint32_t* d_selected, uint32_t* d_selected_pnn,
                       void* stream);
int pnn_cu_tree_bins_host(int qp, uint32_t* out);

/* ---- the coding tree over a picture: the pass above with every CTU's edges taken from its neighbours' results.
 *   Grid.  Per image the CTUs form a grid of ctu_rows x ctu_cols; every per-CTU array is in (image, CTU row, CTU column) order, so
 *     n_ctu = n_images ctu_rows ctu_cols.  Leaves, bins, costs, tie rules, z-order and outputs are those of the coding tree above.
 *   Edges, the only new rule.  left[y] of the CTU at (r, c) is the FINAL depth of cell (x = 7, y) of the CTU at (r, c - 1) of the same
 *     image and QP, 255 (not available) at c = 0; above[x] is the final depth of cell (x, y = 7) of the CTU at (r - 1, c), 255 at
 *     r = 0.  This is what TComDataCU::getPULeft / getPUAbove with their default arguments answer inside one slice and tile, which is
 *     what the reference's configurations code.  Nothing crosses an image or a QP.
 *   Order.  HM decides CTUs in raster order; only the CTU left of and the CTU above a CTU are read, so the CTUs of one anti-diagonal
 *     r + c do not depend on each other.
 *   The coding tree's other departures from HM stay: every bin starts from the state an I slice of the QP begins with (no running
 *     contexts), fractions are summed exactly and shifted once per comparison (not HM's whole bits per CU with the counter's carried
 *     fraction).  Whole CTUs only: no partial CTU at a picture's border.
 * Outputs: the eight of pnn_cu_tree_host, and image_dists, image_rates, each NULL or uint64 [nb_qps][n_images]: the sums of the roots'
 * chosen D and F (ctu_dists, ctu_rates) over the image's CTUs.
 * PNN_E_ARG, before anything is written: those of pnn_cu_tree_host without the edges; n_images, ctu_rows or ctu_cols < 1; n_ctu not
 * fitting an int.
 * pnn_cu_tree_picture_device: the same on leaves in device memory, bit-identical; dists, rates and modes are HOST arrays of five device
 * pointers.  The depth maps exist for the chaining whether or not cu_depths is given: without it they live in d_workspace, of
 * pnn_cu_tree_picture_workspace_bytes bytes (nb_qps n_ctu 64; 0 for a grid the entry refuses) and aligned to 16 bytes, which is
 * required either way.  Asynchronous on `stream`, no allocation on the device, nothing read back: the two count outputs and the two
 * sums are zeroed on the stream, then ctu_rows + ctu_cols - 1 launches, one per anti-diagonal, each of (CTUs of the diagonal x
 * n_images, nb_qps) wavefronts; stream order makes the earlier maps visible and no workgroup waits on another.  Also PNN_E_ARG,
 * before any launch and with outputs and workspace untouched: an array not aligned to its element, a workspace that is NULL,
 * misaligned or too small.
 * pnn_cu_tree_leaves_device: the leaves of ONE width from the device outputs of a second pass over that width's n blocks (n a positive
 * multiple of (64 / width)^2), each [nb_qps][n]: dist = sses, rate = rates + side_rates, mode = modes.  One launch, a copy.  PNN_E_ARG
 * before it: a width not of the five, such an n, nb_qps outside 1 .. 8, a NULL array, one not aligned to its element. */
int pnn_cu_tree_picture_host(const int* qps, int nb_qps, const double* lambdas, int n_images, int ctu_rows, int ctu_cols,
                             const uint32_t* const* dists, const uint64_t* const* rates, const uint8_t* const* modes, int pnn_mode,
                             uint8_t* cu_depths, uint8_t* part_nxn, double* node_costs, double* ctu_costs, uint64_t* ctu_dists,
                             uint64_t* ctu_rates, uint32_t* selected, uint32_t* selected_pnn, uint64_t* image_dists, uint64_t* image_rates);
size_t pnn_cu_tree_picture_workspace_bytes(int nb_qps, int n_images, int ctu_rows, int ctu_cols);
int pnn_cu_tree_picture_device(pnn_ctx* ctx, const int* qps, int nb_qps, const double* lambdas, int n_images, int ctu_rows, int ctu_cols,
                               const uint32_t* const* d_dists, const uint64_t* const* d_rates, const uint8_t* const* d_modes, int pnn_mode,
                               uint8_t* d_cu_depths, uint8_t* d_part_nxn, double* d_node_costs, double* d_ctu_costs, uint64_t* d_ctu_dists,
                               uint64_t* d_ctu_rates, uint32_t* d_selected, uint32_t* d_selected_pnn, uint64_t* d_image_dists,
                               uint64_t* d_image_rates, void* d_workspace, size_t workspace_bytes, void* stream);
int pnn_cu_tree_leaves_device(pnn_ctx* ctx, int width, int n, int nb_qps, const uint32_t* d_sses, const uint64_t* d_rates,
                              const uint64_t* d_side_rates, const uint8_t* d_modes, uint32_t* d_dist, uint64_t* d_rate, uint8_t* d_mode,
                              void* stream);

/* ---- context availability: which of a block's above-right and below-left neighbours an encoder holds when it
 * predicts the block, as HM-16.15 answers it (isAboveRightAvailable / isBelowLeftAvailable of TComPattern.cpp through getPUAboveRight /
 * getPUBelowLeft of TComDataCU.cpp; one slice, one tile, constrained intra prediction off), written as the masks of the picture entries.
 *   World.  The picture is the grid of R = ctu_rows x C = ctu_cols whole CTUs of 64, as for the tree's edges: nothing exists beyond the
 *     grid's right and bottom edges.  A CTU is 16 x 16 units of 4 x 4 samples; z(x, y) is the z-order index of unit (x, y) of a CTU (bit
 *     2 j of z is bit j of x, bit 2 j + 1 is bit j of y): the order in which the units of a CTU are coded.  CTUs are coded in raster order.
 *   A block of width w, n = w / 4 units, at unit (x, y) of the CTU at (r, c); x and y are multiples of n.
 *   Above-right, units (x + n .. x + 2 n - 1, y - 1):
 *     x + n < 16, y > 0:  available iff z(x + n, y - 1) < z(x + n - 1, y)   (inside the CTU: coded before the block's top-right unit)
 *     x + n < 16, y = 0:  available iff r > 0                               (the CTU above)
 *     x + n = 16, y > 0:  not available                                     (the CTU to the right is coded later)
 *     x + n = 16, y = 0:  available iff r > 0 and c + 1 < C                 (the above-right CTU; beyond the picture's right edge at c + 1 = C)
 *   Below-left, units (x - 1, y + n .. y + 2 n - 1):
 *     y + n = 16:         not available                                     (the CTU below or below-left is coded later, or the picture ends)
 *     x > 0:              available iff z(x - 1, y + n) < z(x, y + n - 1)   (coded before the block's bottom-left unit)
 *     x = 0:              available iff c > 0                               (the CTU to the left)
 *   For an aligned block every unit of a portion has the portion's answer (all or nothing), and the answer does not depend on the
 *     partition.  mask_w = 0 where the above-right portion is available, else w; mask_h likewise for the below-left portion: the masks
 *     (in samples) of pnn_score_picture_pairs_device and its kin.
 *   The one departure from HM: at the grid's first CTU row and column the above, corner and left portions are NOT masked -- the picture
 *     entries read them from the plane, whose margin the caller provides; HM would substitute them, and the PNN has no form without
 *     them.  The above-right of the first CTU row and the below-left of the first CTU column follow HM: absent.
 * pnn_hm_context_masks_host: mask_w, mask_h uint8 [ctu_rows ctu_cols (64 / width)^2], CTUs in raster order, a CTU's blocks in z-order
 * (the order of the coding tree's leaves).  PNN_E_ARG, nothing written: a width not of the five, ctu_rows or ctu_cols < 1, a number of
 * blocks that does not fit an int, a NULL output.  tests/test_hm_context_masks.py pins it to HM's own answers. */
int pnn_hm_context_masks_host(int width, int ctu_rows, int ctu_cols, uint8_t* mask_w, uint8_t* mask_h);

/* ---- masks per block: the picture entries with the masks of every POSITION in place of the call's two scalars.
 * Each entry is the widest existing entry of its operation -- pnn_score_picture_pairs_hm_device, pnn_first_pass_picture_pairs_hm_device,
 * pnn_rd_pass_tskip_picture_pairs_device (transform_skip 0: the codec entry's launches) -- with `int mask_w, int mask_h` replaced by
 * d_mask_w, d_mask_h: uint8 [positions] in device memory, in samples, the same for every image (block b = image positions + pos reads
 * element pos).  Both NULL: nothing is masked.
 * Contract: every output of block b has the bytes the existing entry gives that block when called with the scalar masks
 * (d_mask_w[pos], d_mask_h[pos]); a block's bits do not depend on the other blocks of the call.  Same launches, same workspace
 * functions, same order of checks as the entry each extends.
 * PNN_E_ARG, before any launch and with the outputs untouched: exactly one of the two arrays NULL (checked with the planes); a mask
 * outside {0, 4, .., width} -- the masks are read back with the positions, in the same single wait for the stream, and checked behind
 * them.  The geometry check is the existing one: the whole 3 width square of every position lies inside the picture, masked or not. */
int pnn_score_picture_pairs_masks_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                         int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                         const uint8_t* d_mask_w, const uint8_t* d_mask_h, int smoothing, uint8_t* d_targets, uint8_t* d_pnn_u8,
                                         float* d_pnn_f32, uint32_t* d_pnn_sse, uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred,
                                         void* stream);
int pnn_first_pass_picture_pairs_masks_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                              int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                              const uint8_t* d_mask_w, const uint8_t* d_mask_h, const uint8_t* d_cand_pred, int smoothing,
                                              uint32_t* d_mode_hads, uint32_t* d_cand_hads, uint8_t* d_list_modes, uint32_t* d_list_costs,
                                              void* stream);
int pnn_rd_pass_picture_pairs_masks_device(pnn_ctx* ctx, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                           const uint8_t* d_mask_w, const uint8_t* d_mask_h, const uint8_t* d_cand_pred, int smoothing,
                                           const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding, int rdoq, int signalling,
                                           const uint8_t* d_left_modes, const uint8_t* d_above_modes, int codec, int transform_skip,
                                           uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot,
                                           double* d_best_cost, uint32_t* d_best_sse, uint64_t* d_best_rate, double* d_first_pass_costs,
                                           uint64_t* d_best_side_rate, uint8_t* d_best_ts_flag, void* d_workspace, size_t workspace_bytes,
                                           void* stream);

/* Per-launch accounting of the last *_device call (for bench.py's roofline object): number of tap-GEMM
 * launches and their algorithmic FLOPs (2 * M * K * N summed, padding excluded). */
int pnn_last_call_stats(const pnn_ctx* ctx, int* n_gemm_launches, double* gemm_flops, int* n_launches);

/* The same FLOPs without the multiply-adds of the taps that position-major tiles skipped (they only meet SAME padding: exact zeros) --
 * what the matrix cores were actually asked to do, for bench.py's executed-MFMA fractions of the convolutional nets. */
int pnn_last_call_issued_flops(const pnn_ctx* ctx, double* flops);

/* With pnn_set_option(ctx, "time_launches", 1) every tap-GEMM launch is bracketed by HIP events on its launch
 * stream. This call waits for them and returns, for kernel family `kind` (0 = tapgemm_f32_kernel, 2 = tapgemm_sp_kernel,
 * 3 = convimg_sp_kernel, 4 = tapgemm_ring_kernel, 5 = tapgemm_small_kernel, 6 = tapgemm_f32_small_kernel), the number of
 * launches since the last call, their summed duration and their summed algorithmic FLOPs. */
int pnn_launch_times(pnn_ctx* ctx, int kind, int* n_launches, double* total_us, double* total_flops);

#ifdef __cplusplus
}
#endif
#endif /* PNN_HIP_H */
