// The C-ABI entries of the Python evaluator (include/pnn_hip.h; HM calls none of them): the best HEVC intra mode and the first-pass
// Hadamard ranking on dense patterns (each with its *_hm sibling: HM's reference-sample smoothing as an option; the entry without the
// suffix is the sibling called with 0), IPFCN-S, the scores from pictures and pairs of pictures, the open-loop transform
// coding of predictions, HM's second intra pass over the first-pass candidates.  Contexts, models, staging and the
// predictor's entries: pnn_abi.cpp.  Each argument check is written once and composed per entry; an entry's ORDER of checks is part of
// its behaviour (which of two bad arguments pnn_last_error names), so it is spelled out in the entry -- for the ten entries of the
// second pass in rd_pass, the one body behind them: the narrower entries forward upwards with the option they lack at 0, the _codec_
// and _tskip_ entries fill an RdPassCall, and rd_pass branches, with a comment, wherever rungs or forms of blocks differ in their order.
// tests/test_gpu_eval_errors.py pins every refusal and these orders.
#include "pnn_ctx.h"

#include <algorithm>
#include <cmath>

using namespace pnn;

namespace {

// ---- every check once: PNN_OK, or the refusal with its text left for pnn_last_error ----
int check_width(pnn_ctx* c, int w) { return width_index(w) >= 0 ? PNN_OK : fail(c, PNN_E_ARG, "width %d is not 4, 8, 16, 32 or 64", w); }
int check_ipfcns_width(pnn_ctx* c, int w) { return ipfcns_index(w) >= 0 ? PNN_OK : fail(c, PNN_E_ARG, "no IPFCN-S for width %d (4, 8, 16 or 32)", w); }
int check_some_output(pnn_ctx* c, bool any) { return any ? PNN_OK : fail(c, PNN_E_ARG, "every output is NULL"); }
int check_sizes(pnn_ctx* c, int images, int positions, int height, int width_ch)
{
    return images < 0 || positions < 0 || height < 0 || width_ch < 0 ? fail(c, PNN_E_ARG, "negative sizes") : PNN_OK;
}
int check_masks(pnn_ctx* c, int width, int mask_w, int mask_h)
{
    if (mask_w < 0 || mask_w > width || mask_w % 4 || mask_h < 0 || mask_h > width || mask_h % 4)
        return fail(c, PNN_E_ARG, "masks (%d, %d): both must belong to {0, 4, ..., %d}", mask_w, mask_h, width);
    return PNN_OK;
}
int count_blocks(pnn_ctx* c, int images, int positions, long* n)
{
    *n = (long)images * positions;
    return *n > 0x7fffffffL ? fail(c, PNN_E_ARG, "more than 2^31 - 1 blocks") : PNN_OK;
}
// the option of every *_hm entry (include/pnn_hip.h): HM's reference-sample smoothing
int check_smoothing(pnn_ctx* c, int smoothing)
{
    return smoothing < 0 || smoothing > 2 ? fail(c, PNN_E_ARG, "smoothing %d is not 0 (none), 1 ([1 2 1]) or 2 (HM: strong allowed)", smoothing) : PNN_OK;
}
// the outputs of the first-pass ranking, dense or from pictures
int check_hads_outputs(pnn_ctx* c, const void* d_cand_pred, const void* d_mode_hads, const void* d_cand_hads, const void* d_list_modes,
                       const void* d_list_costs)
{
    if (const int rc = check_some_output(c, d_mode_hads || d_cand_hads || d_list_modes || d_list_costs)) return rc;
    return d_cand_hads && !d_cand_pred ? fail(c, PNN_E_ARG, "d_cand_hads needs d_cand_pred") : PNN_OK;
}
// dense form of the 35-mode kernels, everything in front of the outputs
int check_dense_blocks(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n)
{
    if (const int rc = check_width(c, width)) return rc;
    if (pattern_h < width + 1 || pattern_h > 2 * width + 1 || pattern_w < width + 1 || pattern_w > 2 * width + 1)
        return fail(c, PNN_E_ARG, "intra pattern %dx%d: both sides must lie in [%d, %d]", pattern_h, pattern_w, width + 1, 2 * width + 1);
    return n < 0 || (n > 0 && (!d_patterns || !d_targets)) ? fail(c, PNN_E_ARG, "bad batch size or input buffers") : PNN_OK;
}

// d_mask_w / d_mask_h: the masks per position of the *_masks_ entries (include/pnn_hip.h, "masks per block"), NULL for the call's scalars
PictureBlocks picture_blocks(const uint8_t* d_channels, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                             const uint8_t* d_mask_w = nullptr, const uint8_t* d_mask_h = nullptr)
{
    PictureBlocks b;
    b.channels = d_channels; b.H = height; b.W = width_ch; b.rows = d_rows; b.cols = d_cols; b.positions = positions;
    b.mask_w = d_mask_w; b.mask_h = d_mask_h;
    return b;
}

// Where a 35-mode kernel reads its n blocks.  Dense form: patterns [n][ph][pw] and targets [n][w][w].  Picture form (`pictures`):
// contexts and intra patterns from the plane and the positions of `pic`, targets from the plane target_channels, the masks (what they
// leave of a pattern's first column and row: 2w + 1 - mask_h / mask_w); n = images * positions, set by count_blocks.
struct BlockSource {
    bool pictures = false;
    const uint8_t* patterns = nullptr; int ph = 0, pw = 0; const uint8_t* targets = nullptr;
    PictureBlocks pic{}; const uint8_t* target_channels = nullptr; int images = 0, mask_w = 0, mask_h = 0;
    long n = 0;
};
BlockSource dense_blocks(const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n)
{
    BlockSource b;
    b.patterns = d_patterns; b.ph = pattern_h; b.pw = pattern_w; b.targets = d_targets; b.n = n;
    return b;
}
BlockSource picture_pair_blocks(const PictureBlocks& context, const uint8_t* d_target_channels, int images, int mask_w, int mask_h)
{
    BlockSource b;
    b.pictures = true; b.pic = context; b.target_channels = d_target_channels; b.images = images; b.mask_w = mask_w; b.mask_h = mask_h;
    return b;
}

// picture-pair form, everything in front of the outputs: both planes or none, width, masks, sizes
int check_pair_geometry(pnn_ctx* c, int width, const BlockSource& b)
{
    int rc;
    if (!b.pic.channels != !b.target_channels)
        return fail(c, PNN_E_ARG, "one plane of the pair is NULL (%s)", b.pic.channels ? "d_target_channels" : "d_context_channels");
    if (!b.pic.mask_w != !b.pic.mask_h) return fail(c, PNN_E_ARG, "one mask array is NULL (%s)", b.pic.mask_w ? "d_mask_h" : "d_mask_w");
    if ((rc = check_width(c, width)) || (rc = check_masks(c, width, b.mask_w, b.mask_h))) return rc;
    return check_sizes(c, b.images, b.pic.positions, b.pic.H, b.pic.W);
}
// either form, everything in front of the smoothing
int check_blocks(pnn_ctx* c, int width, const BlockSource& b)
{
    return b.pictures ? check_pair_geometry(c, width, b) : check_dense_blocks(c, width, b.patterns, b.ph, b.pw, b.targets, (int)b.n);
}

// The positions are read back once (the call waits for the stream) and checked before any launch: the span x span pixels at each of
// them lie inside the picture.  `what` and `leaves` word the refusal: "position" / "context leaves" for the 3w contexts, "line origin" /
// "lines leave" for the 2w + 8 reference lines of IPFCN-S.  Masks per position (mask_width > 0 and pic.mask_w set) come back in the same
// wait and are checked behind the positions: each belongs to {0, 4, ..., mask_width}.
int check_positions(pnn_ctx* c, const PictureBlocks& pic, int span, const char* what, const char* leaves, hipStream_t s, int mask_width = 0)
{
    const bool masks = mask_width > 0 && pic.mask_w && pic.mask_h;
    std::vector<int32_t> rows(pic.positions), cols(pic.positions);
    std::vector<uint8_t> mask_w(masks ? pic.positions : 0), mask_h(masks ? pic.positions : 0);
    {
        PNN_UNSAFE_CALLS_GUARD;
        HIPCHK(c, hipMemcpyAsync(rows.data(), pic.rows, (size_t)pic.positions * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(cols.data(), pic.cols, (size_t)pic.positions * 4, hipMemcpyDeviceToHost, s));
        if (masks) {
            HIPCHK(c, hipMemcpyAsync(mask_w.data(), pic.mask_w, (size_t)pic.positions, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(mask_h.data(), pic.mask_h, (size_t)pic.positions, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(c, hipStreamSynchronize(s));
    }
    for (int i = 0; i < pic.positions; i++)
        if (rows[i] < 0 || cols[i] < 0 || (long)rows[i] + span > pic.H || (long)cols[i] + span > pic.W)
            return fail(c, PNN_E_ARG, "%s %d (%d, %d): the %dx%d %s the %dx%d picture", what, i, rows[i], cols[i], span, span, leaves, pic.H, pic.W);
    for (int i = 0; masks && i < pic.positions; i++)
        if (mask_w[i] > mask_width || mask_w[i] % 4 || mask_h[i] > mask_width || mask_h[i] % 4)
            return fail(c, PNN_E_ARG, "masks (%d, %d) of position %d: both must belong to {0, 4, ..., %d}", mask_w[i], mask_h[i], i, mask_width);
    return PNN_OK;
}

// inputs common to the scoring entries: the buffers, then every 3w x 3w context inside the picture
int check_picture_blocks(pnn_ctx* c, int width, const PictureBlocks& pic, hipStream_t s)
{
    if (!pic.channels || !pic.rows || !pic.cols) return fail(c, PNN_E_ARG, "NULL input buffers");
    return check_positions(c, pic, 3 * width, "position", "context leaves", s, width);
}

// The blocks of a 35-mode kernel, the fields its parameter structs share (pnn_kernels.h): the dense form has no picture, the picture
// form patterns == NULL.  smoothing: the checked option.  The outputs of the two structs made below are the caller's to set.
template <typename P>
void set_blocks(P& p, const BlockSource& b, int width, int smoothing)
{
    p.patterns = b.patterns; p.targets = b.targets; p.N = (int)b.n; p.w = width; p.pic = b.pic; p.pic_targets = b.target_channels;
    p.ph = b.pictures ? 2 * width + 1 - b.mask_h : b.ph; p.pw = b.pictures ? 2 * width + 1 - b.mask_w : b.pw; p.smoothing = smoothing;
}
HevcBestModeParams best_mode_params(const BlockSource& b, int width, int smoothing)
{
    HevcBestModeParams p;
    set_blocks(p, b, width, smoothing);
    p.best_mode = nullptr; p.best_sse = nullptr; p.best_pred = nullptr; p.mode_sse = nullptr;
    return p;
}
HevcModeHadsParams mode_hads_params(const BlockSource& b, int width, int smoothing, const uint8_t* cand_pred)
{
    HevcModeHadsParams p;
    set_blocks(p, b, width, smoothing);
    p.cand_pred = cand_pred; p.mode_hads = nullptr; p.cand_hads = nullptr; p.list_modes = nullptr; p.list_costs = nullptr;
    return p;
}

// transform coding, everything in front of the launch: width, batch, QPs, outputs
int check_trquant(pnn_ctx* c, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const int* qps, int nb_qps, bool any_output)
{
    if (const int rc = check_width(c, width)) return rc;
    if (n < 0 || (n > 0 && (!d_predictions || !d_targets))) return fail(c, PNN_E_ARG, "bad batch size or input buffers");
    if (!trquant::qps_ok(qps, nb_qps)) return fail(c, PNN_E_ARG, "the QPs are not 1 to %d integers in [0, %d]", trquant::kMaxQps, trquant::kMaxQp);
    return check_some_output(c, any_output);
}

// the launch's inputs: the QPs' constants and initial context states, worked out here; the outputs are the caller's to set
struct TrQuantOptions { int sign_data_hiding; int rdoq; const double* lambdas; };
TrQuantParams trquant_params(int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes, const int* qps,
                             int nb_qps, const TrQuantOptions& o)
{
    const int sign_data_hiding = o.sign_data_hiding, rdoq = o.rdoq;
    const double* lambdas = o.lambdas;
    TrQuantParams p;
    p.pred = d_predictions; p.targets = d_targets; p.N = n; p.w = width; p.nb_qps = nb_qps;
    for (int i = 0; i < trquant::kMaxQps; i++) {
        const int qp = qps[i < nb_qps ? i : 0];
        p.qp[i] = trquant::qp_consts(trquant::log2_tu(width), qp);
        for (int k = 0; k < cabac::kNumCtx; k++) p.init_states[i][k] = (uint8_t)cabac::init_state(qp, cabac::init_value(k));
    }
    p.sse = nullptr; p.nonzero = nullptr; p.sum_abs = nullptr; p.recon = nullptr; p.rate = nullptr;
    p.modes = d_modes; p.sdh = sign_data_hiding != 0;
    // RDOQ: lambda, error scale and rdFactor of each QP in double, here, so that twin and kernel use the same bits
    p.rdoq = rdoq != 0; p.cbf_ctx = width == 8 || width == 16 || width == 32 ? 1 : 0;
    for (int i = 0; i < trquant::kMaxQps; i++) {          // (zero without the option and behind the last QP: never read)
        p.rd[i] = rdoq::Consts{0., 0., 0};
        p.cbf_states[i][0] = p.cbf_states[i][1] = 0;
        if (!rdoq || i >= nb_qps) continue;
        p.rd[i] = rdoq::consts(trquant::log2_tu(width), qps[i], lambdas ? lambdas[i] : pnn_hm_intra_lambda(qps[i]));
        for (int k = 0; k < 2; k++) p.cbf_states[i][k] = (uint8_t)cabac::init_state(qps[i], rdoq::kCbfInit[k]);
    }
    return p;
}

// the codec of the second pass: 0 the switch codec, 1 the substitution codec, which HM never searches without the mode bits
int check_codec(pnn_ctx* c, int codec, int signalling)
{
    if (codec != 0 && codec != 1) return fail(c, PNN_E_ARG, "codec %d is not 0 (switch) or 1 (substitution)", codec);
    return codec && !signalling ? fail(c, PNN_E_ARG, "the substitution codec without signalling") : PNN_OK;
}

// the option rdoq of the transform coding and of the second pass: with it a caller's lambda is finite and above 0 (rdFactor divides by it)
int check_rdoq_lambdas(pnn_ctx* c, int rdoq, const double* lambdas, int nb_qps)
{
    for (int i = 0; rdoq && lambdas && i < nb_qps; i++)
        if (!(lambdas[i] > 0. && lambdas[i] <= 1.7976931348623157e308)) return fail(c, PNN_E_ARG, "RDOQ with lambda %d not finite or not above 0", i);
    return PNN_OK;
}

// the option transform_skip: 0 .. top, and nonzero at width 4 only
int check_tskip_option(pnn_ctx* c, int width, int transform_skip, int top)
{
    if (transform_skip < 0 || transform_skip > top) return fail(c, PNN_E_ARG, "transform_skip %d is not in 0 .. %d", transform_skip, top);
    return transform_skip && width != tskip::kWidth ? fail(c, PNN_E_ARG, "transform skip at width %d (4 only)", width) : PNN_OK;
}

// Carves a caller's scratch into sections, each at a multiple of 256 bytes.  With base NULL only `at`, the bytes taken, is of use.
struct Carver {
    void* base; size_t at = 0;
    template <typename T>
    T* take(size_t count)
    {
        T* p = (T*)((uintptr_t)base + at);
        at += (count * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};

// The caller's scratch of the transform coding with transform skip: both forms' outputs, [0] transformed and [1] skipped, each
// [nb_qps][n] (recon [nb_qps][n][4][4]).
struct TskipOut { uint32_t* sse; uint32_t* nonzero; uint32_t* sum_abs; uint64_t* rate; uint8_t* recon; };
struct TskipWorkspace { TskipOut form[2]; size_t bytes; };
TskipWorkspace tskip_workspace(void* base, long n, int nb_qps)
{
    const size_t qn = (size_t)n * nb_qps;
    Carver cv{base};
    TskipWorkspace ws;
    for (TskipOut& o : ws.form) {
        o.rate = cv.take<uint64_t>(qn);
        o.sse = cv.take<uint32_t>(qn);
        o.nonzero = cv.take<uint32_t>(qn);
        o.sum_abs = cv.take<uint32_t>(qn);
        o.recon = cv.take<uint8_t>(qn * 16);
    }
    ws.bytes = cv.at;
    return ws;
}

// The caller's scratch of the second intra pass, n (K + 1) slots: per-slot rate and SSE [nb_qps][slots], the slots' predictions and
// replicated targets [slots][w][w], their modes [slots], the first-pass list [n][K].
struct RdWorkspace { uint64_t* rate; uint32_t* sse; uint8_t* pred; uint8_t* targets; uint8_t* modes; uint8_t* list; size_t bytes; };
RdWorkspace rd_workspace(void* base, int width, long n, int nb_qps)
{
    const int k = hevc_first_pass_list_size(width);
    const size_t slots = (size_t)n * (k + 1), w2 = (size_t)width * width;
    Carver cv{base};
    RdWorkspace ws;
    ws.rate = cv.take<uint64_t>(slots * nb_qps);
    ws.sse = cv.take<uint32_t>(slots * nb_qps);
    ws.pred = cv.take<uint8_t>(slots * w2);
    ws.targets = cv.take<uint8_t>(slots * w2);
    ws.modes = cv.take<uint8_t>(slots);
    ws.list = cv.take<uint8_t>((size_t)n * k);
    ws.bytes = cv.at;
    return ws;
}

// The caller's scratch of the second pass with mode signalling, n (K + 3) slots of ONE QP at a time: per-slot rate, SSE and count of
// nonzero levels, the slots' predictions and replicated targets, every QP's slot modes [nb_qps][n][K + 3], the Hadamard costs of the
// 35 modes and of the candidate.
struct RdSignalWorkspace {
    uint64_t* rate; uint32_t* sse; uint32_t* nonzero; uint8_t* pred; uint8_t* targets; uint8_t* slot_modes; uint32_t* mode_hads; uint32_t* cand_hads;
    size_t bytes;
};
// (codec 1, the substitution codec of DESIGN.md section 5o: K + 2 slots wherever the switch codec has K + 3)
int signal_slots(int width, int codec) { return hevc_first_pass_list_size(width) + (codec ? msig::kExtraSlotsSubstitution : msig::kExtraSlots); }
RdSignalWorkspace rd_signal_workspace(void* base, int width, long n, int nb_qps, int codec)
{
    const size_t slots = (size_t)n * signal_slots(width, codec), w2 = (size_t)width * width;
    const size_t units = slots * (width == 64 ? 4 : 1);       // at width 64 every slot is coded as its four quadrants
    Carver cv{base};
    RdSignalWorkspace ws;
    ws.rate = cv.take<uint64_t>(units);
    ws.sse = cv.take<uint32_t>(units);
    ws.nonzero = cv.take<uint32_t>(units);
    ws.pred = cv.take<uint8_t>(slots * w2);
    ws.targets = cv.take<uint8_t>(slots * w2);
    ws.slot_modes = cv.take<uint8_t>(slots * nb_qps);
    ws.mode_hads = cv.take<uint32_t>((size_t)n * 35);
    ws.cand_hads = cv.take<uint32_t>((size_t)n);
    ws.bytes = cv.at;
    return ws;
}

// The scratch the second pass with transform skip adds behind rd_signal_workspace's: the skipped form's rate, SSE and count of the
// slots of ONE QP, the slots' mode bits and flags, the winners' slots.
struct RdTskipWorkspace { uint64_t* rate; uint32_t* sse; uint32_t* nonzero; uint32_t* mode_bits; uint8_t* ts_flag; uint8_t* best_slot; size_t bytes; };
RdTskipWorkspace rd_tskip_workspace(void* base, size_t slots, long n)
{
    Carver cv{base};
    RdTskipWorkspace ws;
    ws.rate = cv.take<uint64_t>(slots);
    ws.sse = cv.take<uint32_t>(slots);
    ws.nonzero = cv.take<uint32_t>(slots);
    ws.mode_bits = cv.take<uint32_t>(slots);
    ws.ts_flag = cv.take<uint8_t>(slots);
    ws.best_slot = cv.take<uint8_t>((size_t)n);
    ws.bytes = cv.at;
    return ws;
}

// One call of the second intra pass, whichever of the ten entries it came through (the narrower ones forward up to the _codec_
// entries with the options they lack at 0; the _tskip_ entries have checks of their own): the blocks, the candidate, the coding's
// arguments, the options, the outputs (NULL where the entry has none), the scratch.
struct RdPassOutputs {
    uint8_t* cand_modes; double* cand_costs; uint8_t* best_mode; uint8_t* best_slot; double* best_cost; uint32_t* best_sse; uint64_t* best_rate;
    double* first_pass_costs; uint64_t* best_side_rate; uint8_t* best_ts_flag;
    bool any() const
    {
        return cand_modes || cand_costs || best_mode || best_slot || best_cost || best_sse || best_rate || first_pass_costs || best_side_rate ||
               best_ts_flag;
    }
};
struct RdPassCall {
    int width; BlockSource blocks; const uint8_t* cand_pred; int smoothing;
    const int* qps; int nb_qps; const double* lambdas; int sign_data_hiding;
    int rdoq = 0, signalling = 0, codec = 0, transform_skip = 0;
    bool tskip_entry = false;                                 // came through a _tskip_ entry, whose checks no other rung has
    const uint8_t* left = nullptr; const uint8_t* above = nullptr;
    RdPassOutputs out{};
    void* workspace = nullptr; size_t workspace_bytes = 0; hipStream_t stream = nullptr;
    double lambda(int i) const { return lambdas ? lambdas[i] : pnn_hm_intra_lambda(qps[i]); }
};
RdPassCall rd_pass_call(int width, const BlockSource& blocks, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                        const double* lambdas, int sign_data_hiding)
{
    RdPassCall q;
    q.width = width; q.blocks = blocks; q.cand_pred = d_cand_pred; q.smoothing = smoothing; q.qps = qps; q.nb_qps = nb_qps; q.lambdas = lambdas;
    q.sign_data_hiding = sign_data_hiding;
    return q;
}

// what the _tskip_ entries check behind the option and the codec: signalling, a lambda the decision can use, the whole scratch
int check_rd_pass_tskip(pnn_ctx* c, const RdPassCall& q)
{
    const long n = q.blocks.n;
    if (!q.signalling) return fail(c, PNN_E_ARG, "the second pass with transform skip without signalling");
    if (!q.transform_skip) return PNN_OK;
    if (const int rc = check_rdoq_lambdas(c, 1, q.lambdas, trquant::qps_ok(q.qps, q.nb_qps) ? q.nb_qps : 0)) return rc;
    if (n <= 0 || !trquant::qps_ok(q.qps, q.nb_qps)) return PNN_OK;         // (refused or empty further down)
    const size_t need = rd_signal_workspace(nullptr, q.width, n, q.nb_qps, q.codec).bytes +
                        rd_tskip_workspace(nullptr, (size_t)n * signal_slots(q.width, q.codec), n).bytes;
    if (q.workspace && q.workspace_bytes < need)                            // (a NULL or misaligned scratch: check_rd_pass_arguments names it)
        return fail(c, PNN_E_ARG, "the workspace has %zu bytes, pnn_rd_pass_tskip_workspace_bytes asks for %zu", q.workspace_bytes, need);
    return PNN_OK;
}

// what every rung checks behind its blocks (the width is checked), up to the scratch: candidate, slot count, QPs, lambdas, outputs
int check_rd_pass_arguments(pnn_ctx* c, const RdPassCall& q)
{
    const long n = q.blocks.n;
    const long slots = q.signalling ? n * signal_slots(q.width, q.codec) * (q.width == 64 ? 4 : 1) : n * (hevc_first_pass_list_size(q.width) + 1);
    if (n > 0 && !q.cand_pred) return fail(c, PNN_E_ARG, "d_cand_pred is NULL");
    if (slots > 0x7fffffffL) return fail(c, PNN_E_ARG, "more than 2^31 - 1 candidate slots");
    if (!trquant::qps_ok(q.qps, q.nb_qps)) return fail(c, PNN_E_ARG, "the QPs are not 1 to %d integers in [0, %d]", trquant::kMaxQps, trquant::kMaxQp);
    for (int i = 0; q.lambdas && i < q.nb_qps; i++)
        if (!(q.lambdas[i] >= 0. && q.lambdas[i] <= 1.7976931348623157e308)) return fail(c, PNN_E_ARG, "lambda %d is negative or not finite", i);
    // with signalling RDOQ's lambda is checked here, in front of the outputs; without it behind the scratch (rd_pass)
    if (q.signalling)
        if (const int rc = check_rdoq_lambdas(c, q.rdoq, q.lambdas, q.nb_qps)) return rc;
    if (const int rc = check_some_output(c, q.out.any())) return rc;
    if (n == 0) return PNN_OK;
    const size_t need = q.signalling ? rd_signal_workspace(nullptr, q.width, n, q.nb_qps, q.codec).bytes : rd_workspace(nullptr, q.width, n, q.nb_qps).bytes;
    if (!q.workspace || (uintptr_t)q.workspace % 8) return fail(c, PNN_E_ARG, "d_workspace is NULL or not aligned to 8 bytes");
    if (q.workspace_bytes < need)                             // (the text names the rung's size function, not the entry's)
        return fail(c, PNN_E_ARG, "the workspace has %zu bytes, %s asks for %zu", q.workspace_bytes,
                    !q.signalling ? "pnn_rd_pass_workspace_bytes" : q.codec ? "pnn_rd_pass_codec_workspace_bytes" : "pnn_rd_pass_signal_workspace_bytes",
                    need);
    return PNN_OK;
}

// the neighbours' modes of a call with signalling, read back once: the call waits for the stream
int check_neighbours(pnn_ctx* c, const RdPassCall& q)
{
    const long n = q.blocks.n;
    if (!q.left && !q.above) return PNN_OK;
    std::vector<uint8_t> modes((size_t)n * 2, (uint8_t)msig::kNoNeighbour);
    {
        PNN_UNSAFE_CALLS_GUARD;                               // both arrays, then ONE wait
        if (q.left) HIPCHK(c, hipMemcpyAsync(modes.data(), q.left, (size_t)n, hipMemcpyDeviceToHost, q.stream));
        if (q.above) HIPCHK(c, hipMemcpyAsync(modes.data() + n, q.above, (size_t)n, hipMemcpyDeviceToHost, q.stream));
        HIPCHK(c, hipStreamSynchronize(q.stream));
    }
    for (long i = 0; i < 2L * n; i++)
        if (!msig::neighbour_ok(modes[i], !q.codec))
            return fail(c, PNN_E_ARG, "%s neighbour mode %d of block %ld is not 0 .. %d or 255", i < n ? "left" : "above", modes[i], i % n,
                        q.codec ? 34 : 35);
    return PNN_OK;
}

// The four launches of the second intra pass without signalling, everything checked: the first-pass list into the scratch, the
// candidates' predictions, the transform coding of the n (K + 1) slots -- the launch of pnn_trquant_rdoq_device with the slots' modes
// as its mode array and every QP at once --, the decision.
int rd_pass_launches(pnn_ctx* c, const RdPassCall& q)
{
    const long n = q.blocks.n;
    hipStream_t s = q.stream;
    const RdWorkspace ws = rd_workspace(q.workspace, q.width, n, q.nb_qps);
    const int k1 = hevc_first_pass_list_size(q.width) + 1;
    HevcModeHadsParams h = mode_hads_params(q.blocks, q.width, q.smoothing, q.cand_pred);
    h.list_modes = ws.list;
    HIPCHK(c, launch_hevc_mode_hads(h, s));
    RdCandidatesParams r;
    set_blocks(r, q.blocks, q.width, q.smoothing);
    r.cand_pred = q.cand_pred; r.list_modes = ws.list; r.cand_modes = q.out.cand_modes ? q.out.cand_modes : ws.modes;
    r.slot_pred = ws.pred; r.slot_targets = ws.targets;
    HIPCHK(c, launch_rd_candidates(r, s));
    TrQuantParams t = trquant_params(q.width, ws.pred, ws.targets, (int)(n * k1), r.cand_modes, q.qps, q.nb_qps,
                                     {q.sign_data_hiding, q.rdoq, q.lambdas});
    t.sse = ws.sse; t.rate = ws.rate;
    HIPCHK(c, launch_trquant(t, s));
    RdDecideParams d;
    d.sse = ws.sse; d.rate = ws.rate; d.cand_modes = r.cand_modes; d.N = (int)n; d.w = q.width; d.nb_qps = q.nb_qps;
    for (int i = 0; i < trquant::kMaxQps; i++) d.lambda[i] = i >= q.nb_qps ? 0. : q.lambda(i);
    d.cand_costs = q.out.cand_costs; d.best_mode = q.out.best_mode; d.best_slot = q.out.best_slot; d.best_cost = q.out.best_cost;
    d.best_sse = q.out.best_sse; d.best_rate = q.out.best_rate;
    HIPCHK(c, launch_rd_decide(d, s));
    c->stat_launches += 4;
    return PNN_OK;
}

// The launches of the second pass with signalling, everything checked: the Hadamard costs (the unchanged first-pass kernel, asked for
// no list), the lists and slots of every QP, then per QP the slots' predictions, their coding -- the launch of pnn_trquant_rdoq_device
// with that one QP -- and the decision, all on the same scratch in stream order: 2 + 3 nb_qps launches; with transform skip four
// more per QP, the last of them only for the flag output.
int rd_pass_signal_launches(pnn_ctx* c, const RdPassCall& q)
{
    const long n = q.blocks.n;
    const int width = q.width, nb_qps = q.nb_qps, codec = q.codec;
    const RdPassOutputs& out = q.out;
    hipStream_t s = q.stream;
    const RdSignalWorkspace ws = rd_signal_workspace(q.workspace, width, n, nb_qps, codec);
    const int slots = signal_slots(width, codec);
    // transform skip (width 4): the skipped form's arrays lie behind the pass's own scratch
    const RdTskipWorkspace ts = rd_tskip_workspace((uint8_t*)q.workspace + ws.bytes, n * slots, n);
    HevcModeHadsParams h = mode_hads_params(q.blocks, width, q.smoothing, q.cand_pred);
    h.mode_hads = ws.mode_hads; h.cand_hads = ws.cand_hads;
    HIPCHK(c, launch_hevc_mode_hads(h, s));
    SignalListParams l;
    l.mode_hads = ws.mode_hads; l.cand_hads = ws.cand_hads; l.left = q.left; l.above = q.above; l.N = (int)n; l.w = width; l.nb_qps = nb_qps;
    double lambda[trquant::kMaxQps];
    for (int i = 0; i < trquant::kMaxQps; i++) {
        lambda[i] = i >= nb_qps ? 0. : q.lambda(i);
        l.bits[i] = msig::flag_bits(q.qps[i < nb_qps ? i : 0]);
        l.sqrt_lambda[i] = std::sqrt(lambda[i]);                                  // TComRdCost::setLambda
    }
    l.list_costs = out.first_pass_costs; l.slot_modes = out.cand_modes ? out.cand_modes : ws.slot_modes;
    HIPCHK(c, codec ? launch_substitution_list(l, s) : launch_signal_list(l, s));
    for (int qi = 0; qi < nb_qps; qi++) {
        const size_t at = (size_t)qi * n;
        const uint8_t* slot_modes = l.slot_modes + at * slots;
        RdCandidatesParams r;
        set_blocks(r, q.blocks, width, q.smoothing);
        r.cand_pred = q.cand_pred; r.list_modes = slot_modes; r.cand_modes = nullptr; r.slot_pred = ws.pred; r.slot_targets = ws.targets;
        HIPCHK(c, codec ? launch_rd_candidates_substitution(r, s) : launch_rd_candidates_slots(r, s));
        // width 64: the slots lie there quadrant by quadrant, 4 n (K + 3) blocks of 32 x 32 under the diagonal scan, each a unit at
        // transform depth 1 (cbf context 0) -- what the w = 64 instantiation codes, with a count of levels per quadrant
        const bool quadrants = width == 64;
        TrQuantParams t = trquant_params(quadrants ? 32 : width, ws.pred, ws.targets, (int)(n * slots * (quadrants ? 4 : 1)),
                                         quadrants ? nullptr : slot_modes, q.qps + qi, 1,
                                         {q.sign_data_hiding, q.rdoq, q.rdoq ? lambda + qi : nullptr});
        if (quadrants) t.cbf_ctx = 0;
        t.sse = ws.sse; t.nonzero = ws.nonzero; t.rate = ws.rate;
        HIPCHK(c, launch_trquant(t, s));
        if (q.transform_skip) {
            // both forms of every slot, decided per slot as the tree does inside each candidate's coding: the skipped form beside the
            // transformed one, the mode bits the decision charges, the merge IN PLACE (sse, count and rate become the kept form's, the
            // rate with the flag bin); the unchanged decision below then compares the slots' merged D and R
            TrQuantParams k = t;
            k.sse = ts.sse; k.nonzero = ts.nonzero; k.rate = ts.rate;
            HIPCHK(c, launch_tskip4(k, s));
            TskipSlotBitsParams sb;
            sb.slot_modes = slot_modes; sb.left = q.left; sb.above = q.above; sb.N = (int)n; sb.S = slots; sb.pnn_flag = codec ? 0 : 1;
            sb.bits = l.bits[qi]; sb.mode_bits = ts.mode_bits;
            HIPCHK(c, launch_tskip_slot_bits(sb, s));
            TskipDecideParams m;
            m.N = (int)(n * slots); m.nb_qps = 1; m.decide = 1; m.charge_cbf = 1; m.mode_bits = ts.mode_bits;
            m.transformed = TskipForm{ws.sse, ws.nonzero, nullptr, ws.rate, nullptr};
            m.skipped = TskipForm{ts.sse, ts.nonzero, nullptr, ts.rate, nullptr};
            for (int i = 0; i < trquant::kMaxQps; i++) { m.lambda[i] = lambda[qi]; m.bits[i] = tskip::qp_bits(q.qps[qi]); }
            m.sse = ws.sse; m.nonzero = ws.nonzero; m.sum_abs = nullptr; m.recon = nullptr; m.rate = ws.rate; m.ts_flag = ts.ts_flag;
            HIPCHK(c, launch_tskip_decide(m, s));
            c->stat_launches += 3;
        }
        RdDecideSignalParams d;
        d.sse = ws.sse; d.rate = ws.rate; d.nonzero = ws.nonzero; d.slot_modes = slot_modes; d.left = q.left; d.above = q.above;
        d.N = (int)n; d.w = width; d.cbf_ctx = msig::cbf_context(width); d.lambda = lambda[qi]; d.bits = l.bits[qi];
        d.cand_costs = out.cand_costs ? out.cand_costs + at * slots : nullptr;
        d.best_mode = out.best_mode ? out.best_mode + at : nullptr; d.best_slot = out.best_slot ? out.best_slot + at : nullptr;
        d.best_cost = out.best_cost ? out.best_cost + at : nullptr; d.best_sse = out.best_sse ? out.best_sse + at : nullptr;
        d.best_rate = out.best_rate ? out.best_rate + at : nullptr; d.best_side_rate = out.best_side_rate ? out.best_side_rate + at : nullptr;
        if (q.transform_skip && !d.best_slot) d.best_slot = ts.best_slot;
        HIPCHK(c, codec ? launch_rd_decide_substitution(d, s) : launch_rd_decide_signal(d, s));
        if (q.transform_skip && out.best_ts_flag) {
            const TskipBestFlagParams g{ts.ts_flag, d.best_slot, (int)n, slots, out.best_ts_flag + at};
            HIPCHK(c, launch_tskip_best_flag(g, s));
            c->stat_launches++;
        }
    }
    c->stat_launches += 2 + 3 * nb_qps;
    return PNN_OK;
}

// One call of the second intra pass from its checks to its launches.  The ORDER below is the entries' behaviour: where the rungs or
// the two forms of blocks differ, the branch says so.
int rd_pass(pnn_ctx* c, RdPassCall& q)
{
    int rc;
    BlockSource& b = q.blocks;
    // the options of the wider rungs, in front of everything (codec 0 and signalling 0 pass check_codec)
    if (q.tskip_entry && (rc = check_tskip_option(c, q.width, q.transform_skip, 1))) return rc;
    if ((rc = check_codec(c, q.codec, q.signalling))) return rc;
    if (!q.tskip_entry && !q.signalling && (q.out.first_pass_costs || q.out.best_side_rate))
        return fail(c, PNN_E_ARG, "d_first_pass_costs or d_best_side_rate without signalling");
    // a _tskip_ entry checks signalling, lambda and scratch size on dense blocks BEFORE the blocks ...
    if (q.tskip_entry && !b.pictures && (rc = check_rd_pass_tskip(c, q))) return rc;
    if ((rc = check_blocks(c, q.width, b)) || (rc = check_smoothing(c, q.smoothing))) return rc;
    if (b.pictures && (rc = count_blocks(c, b.images, b.pic.positions, &b.n))) return rc;
    // ... and on picture pairs BEHIND geometry, smoothing and block count
    if (q.tskip_entry && b.pictures && (rc = check_rd_pass_tskip(c, q))) return rc;
    // with signalling the device is set in front of the checks that end in the neighbours' read-back, without it behind every check
    if (q.signalling && b.n > 0) HIPCHK(c, hipSetDevice(c->device));
    if ((rc = check_rd_pass_arguments(c, q))) return rc;
    // without signalling RDOQ's lambda is checked behind the scratch, also of a call without blocks
    if (!q.signalling && (rc = check_rdoq_lambdas(c, q.rdoq, q.lambdas, q.nb_qps))) return rc;
    if (b.n == 0) return PNN_OK;
    if (!q.signalling) HIPCHK(c, hipSetDevice(c->device));
    if (q.signalling && (rc = check_neighbours(c, q))) return rc;
    if (b.pictures && (rc = check_picture_blocks(c, q.width, b.pic, q.stream))) return rc;
    reset_stats(c);
    if (!q.signalling) return rd_pass_launches(c, q);
    if (!q.transform_skip && q.out.best_ts_flag) HIPCHK(c, hipMemsetAsync(q.out.best_ts_flag, 0, (size_t)q.nb_qps * b.n, q.stream));
    return rd_pass_signal_launches(c, q);
}

Model* ipfcns_for(pnn_ctx* c, int width, int* rc)
{
    if ((*rc = check_ipfcns_width(c, width))) return nullptr;
    Model* m = c->ipfcns[ipfcns_index(width)];
    if (!m) *rc = fail(c, PNN_E_ARG, "no IPFCN-S loaded for width %d", width);
    return m;
}

}  // namespace

extern "C" {

int pnn_hevc_best_mode_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w,
                              const uint8_t* d_targets, int n, uint8_t* d_best_mode, uint32_t* d_best_sse, uint8_t* d_best_pred,
                              uint32_t* d_mode_sse, void* stream)
{
    // the reference's extracted predictor is HM's without the smoothing
    return pnn_hevc_best_mode_hm_device(c, width, d_patterns, pattern_h, pattern_w, d_targets, n, 0, d_best_mode, d_best_sse, d_best_pred,
                                        d_mode_sse, stream);
}

int pnn_hevc_best_mode_hm_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w,
                                 const uint8_t* d_targets, int n, int smoothing, uint8_t* d_best_mode, uint32_t* d_best_sse,
                                 uint8_t* d_best_pred, uint32_t* d_mode_sse, void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    if ((rc = check_dense_blocks(c, width, d_patterns, pattern_h, pattern_w, d_targets, n)) || (rc = check_smoothing(c, smoothing)) ||
        (rc = check_some_output(c, d_best_mode || d_best_sse || d_best_pred || d_mode_sse))) return rc;
    if (n == 0) return PNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HevcBestModeParams p = best_mode_params(dense_blocks(d_patterns, pattern_h, pattern_w, d_targets, n), width, smoothing);
    p.best_mode = d_best_mode; p.best_sse = d_best_sse; p.best_pred = d_best_pred; p.mode_sse = d_mode_sse;
    HIPCHK(c, launch_hevc_best_mode(p, (hipStream_t)stream));
    return PNN_OK;
}

int pnn_hevc_mode_hads_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets,
                              int n, const uint8_t* d_cand_pred, uint32_t* d_mode_hads, uint32_t* d_cand_hads, uint8_t* d_list_modes,
                              uint32_t* d_list_costs, void* stream)
{
    return pnn_hevc_mode_hads_hm_device(c, width, d_patterns, pattern_h, pattern_w, d_targets, n, d_cand_pred, 0, d_mode_hads, d_cand_hads,
                                        d_list_modes, d_list_costs, stream);
}

int pnn_hevc_mode_hads_hm_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets,
                                 int n, const uint8_t* d_cand_pred, int smoothing, uint32_t* d_mode_hads, uint32_t* d_cand_hads,
                                 uint8_t* d_list_modes, uint32_t* d_list_costs, void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    if ((rc = check_dense_blocks(c, width, d_patterns, pattern_h, pattern_w, d_targets, n)) || (rc = check_smoothing(c, smoothing)) ||
        (rc = check_hads_outputs(c, d_cand_pred, d_mode_hads, d_cand_hads, d_list_modes, d_list_costs))) return rc;
    if (n == 0) return PNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HevcModeHadsParams p = mode_hads_params(dense_blocks(d_patterns, pattern_h, pattern_w, d_targets, n), width, smoothing, d_cand_pred);
    p.mode_hads = d_mode_hads; p.cand_hads = d_cand_hads; p.list_modes = d_list_modes; p.list_costs = d_list_costs;
    HIPCHK(c, launch_hevc_mode_hads(p, (hipStream_t)stream));
    return PNN_OK;
}

int pnn_ipfcns_load(pnn_ctx* c, int width, const float* params, size_t n_floats)
{
    if (!c) return PNN_E_ARG;
    if (const int rc = check_ipfcns_width(c, width)) return rc;
    if (!params) return fail(c, PNN_E_ARG, "NULL parameters");
    HIPCHK(c, hipSetDevice(c->device));
    Model* m = nullptr;
    const int rc = build_ipfcns_model(c, width, params, n_floats, &m);
    if (rc) return rc;
    const int idx = ipfcns_index(width);
    PNN_UNSAFE_CALLS_GUARD;
    if (c->ipfcns[idx]) HIPCHK(c, hipStreamSynchronize(c->stream));
    free_model(c->ipfcns[idx]);
    c->ipfcns[idx] = m;
    c->tuned.clear(); c->tune_gen++;                                 // keys point into the replaced net
    return PNN_OK;
}

int pnn_ipfcns_forward_device(pnn_ctx* c, int width, const float* d_x, int n, float* d_out_f32, void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    const Model* m = ipfcns_for(c, width, &rc);
    if (!m) return rc;
    if (n < 0 || (n > 0 && (!d_x || !d_out_f32))) return fail(c, PNN_E_ARG, "bad batch size or buffers");
    if (n == 0) return PNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    reset_stats(c);
    return ipfcns_pass(c, m, d_x, n, d_out_f32, (hipStream_t)stream);
}

int pnn_ipfcns_predict_device(pnn_ctx* c, int width, const uint8_t* d_channels, int images, int height, int width_ch,
                              const int32_t* d_rows, const int32_t* d_cols, int positions, const uint8_t* d_targets,
                              uint8_t* d_pred_u8, float* d_pred_f32, float* d_means, uint32_t* d_sse, void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    const Model* m = ipfcns_for(c, width, &rc);
    if (!m) return rc;
    if ((rc = check_sizes(c, images, positions, height, width_ch))) return rc;
    if (d_sse && !d_targets) return fail(c, PNN_E_ARG, "d_sse needs d_targets");
    long n;
    if ((rc = count_blocks(c, images, positions, &n))) return rc;
    if (n == 0) return PNN_OK;
    if (!d_channels || !d_rows || !d_cols) return fail(c, PNN_E_ARG, "NULL input buffers");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const PictureBlocks lines = picture_blocks(d_channels, height, width_ch, d_rows, d_cols, positions);
    if ((rc = check_positions(c, lines, 2 * width + 8, "line origin", "lines leave", s))) return rc;
    reset_stats(c);
    int K, H;
    ipfcns_dims(width, &K, &H);
    const long w2 = (long)width * width, chunk = std::min(n, ipfcns_chunk(c, m));
    if ((rc = dev_reserve(c, c->ipfcns_ws[0], (size_t)chunk * K * 4))) return rc;
    if ((rc = dev_reserve(c, c->ipfcns_ws[3], (size_t)chunk * (w2 + 1) * 4))) return rc;
    float* rows_f = (float*)c->ipfcns_ws[0].p;
    float* fc4 = (float*)c->ipfcns_ws[3].p;
    float* means_ws = fc4 + chunk * w2;
    for (long b0 = 0; b0 < n; b0 += chunk) {
        const int nb = (int)std::min(chunk, n - b0);
        float* means = d_means ? d_means + b0 : means_ws;
        IpfcnsGatherParams g;
        g.channels = d_channels; g.H = height; g.W = width_ch; g.rows = d_rows; g.cols = d_cols; g.positions = positions;
        g.b0 = b0; g.nb = nb; g.w = width; g.x = rows_f; g.mean = means;
        HIPCHK(c, launch_ipfcns_gather(g, s));
        if ((rc = ipfcns_pass(c, m, rows_f, nb, fc4, s))) return rc;
        IpfcnsEpilogueParams e;
        e.fc4 = fc4; e.mean = means; e.nb = nb; e.w2 = (int)w2;
        e.u8 = d_pred_u8 ? d_pred_u8 + b0 * w2 : nullptr; e.f32 = d_pred_f32 ? d_pred_f32 + b0 * w2 : nullptr;
        e.targets = d_targets ? d_targets + b0 * w2 : nullptr; e.sse = d_sse ? d_sse + b0 : nullptr;
        HIPCHK(c, launch_ipfcns_epilogue(e, s));
        c->stat_launches += 2;
    }
    return PNN_OK;
}

int pnn_score_pictures_device(pnn_ctx* c, int width, const uint8_t* d_channels, int images, int height, int width_ch,
                              const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w, int mask_h,
                              uint8_t* d_targets, uint8_t* d_pnn_u8, float* d_pnn_f32, uint32_t* d_pnn_sse,
                              uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred, void* stream)
{
    // a single picture is the pair of one plane with itself
    return pnn_score_picture_pairs_device(c, width, d_channels, d_channels, images, height, width_ch, d_rows, d_cols, positions, mask_w,
                                          mask_h, d_targets, d_pnn_u8, d_pnn_f32, d_pnn_sse, d_hevc_mode, d_hevc_sse, d_hevc_pred, stream);
}

int pnn_score_picture_pairs_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                   int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w,
                                   int mask_h, uint8_t* d_targets, uint8_t* d_pnn_u8, float* d_pnn_f32, uint32_t* d_pnn_sse,
                                   uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred, void* stream)
{
    return pnn_score_picture_pairs_hm_device(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols, positions,
                                             mask_w, mask_h, 0, d_targets, d_pnn_u8, d_pnn_f32, d_pnn_sse, d_hevc_mode, d_hevc_sse, d_hevc_pred,
                                             stream);
}

// The one body of the score entries: the call's scalar masks (the *_masks_ entry passes 0, 0), or masks per position where the two
// arrays are given.
static int score_picture_pairs(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                               int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w, int mask_h,
                               const uint8_t* d_mask_w, const uint8_t* d_mask_h, int smoothing, uint8_t* d_targets, uint8_t* d_pnn_u8,
                               float* d_pnn_f32, uint32_t* d_pnn_sse, uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred, void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    const bool want_pnn = d_pnn_u8 || d_pnn_f32 || d_pnn_sse, want_hevc = d_hevc_mode || d_hevc_sse || d_hevc_pred;
    // contexts and intra patterns from the context plane, targets (hence both SSEs) from the target plane
    const PictureBlocks pic = picture_blocks(d_context_channels, height, width_ch, d_rows, d_cols, positions, d_mask_w, d_mask_h);
    const PictureBlocks pic_tg = picture_blocks(d_target_channels, height, width_ch, d_rows, d_cols, positions);
    BlockSource blocks = picture_pair_blocks(pic, d_target_channels, images, mask_w, mask_h);
    if ((rc = check_pair_geometry(c, width, blocks)) ||
        (rc = check_smoothing(c, smoothing)) ||
        (rc = check_some_output(c, d_targets || want_pnn || want_hevc))) return rc;
    Model* m = want_pnn ? c->models[width_index(width)] : nullptr;
    if (want_pnn && !m) return fail(c, PNN_E_ARG, "a PNN output is asked for, but no model is loaded for width %d", width);
    if ((rc = count_blocks(c, images, positions, &blocks.n))) return rc;
    const long n = blocks.n;
    if (n == 0) return PNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if ((rc = check_picture_blocks(c, width, pic, s))) return rc;
    if (want_pnn && (rc = pending_range_error(c))) return rc;
    reset_stats(c);
    const long w2 = (long)width * width;
    // the PNN half in slices (descriptors -> gather -> net -> epilogue); the bits of a block do not depend on its slice
    const long chunk = want_pnn ? std::min(n, chunk_blocks(c, m)) : n;
    float* ws_f32 = nullptr;
    if (want_pnn) {
        if ((rc = dev_reserve(c, c->score_ws[0], (size_t)chunk * sizeof(TbDev)))) return rc;
        if (!d_pnn_f32) {
            if ((rc = dev_reserve(c, c->score_ws[1], (size_t)chunk * w2 * 4))) return rc;
            ws_f32 = (float*)c->score_ws[1].p;
        }
    }
    for (long b0 = 0; b0 < n && (want_pnn || d_targets); b0 += chunk) {
        const int nb = (int)std::min(chunk, n - b0);
        float* pred = nullptr;
        if (want_pnn) {
            ScoreDescParams d;
            d.pic = pic; d.b0 = b0; d.nb = nb; d.w = width; d.mask_w = mask_w; d.mask_h = mask_h; d.tbs = (TbDev*)c->score_ws[0].p;
            HIPCHK(c, launch_score_desc(d, s));
            pred = d_pnn_f32 ? d_pnn_f32 + b0 * w2 : ws_f32;
            if ((rc = tbs_pass(c, m, d_context_channels, 1, (const pnn_tb_dev*)c->score_ws[0].p, nb, nullptr, pred, s))) return rc;
            c->stat_launches++;
        }
        if (d_targets || d_pnn_u8 || d_pnn_sse) {
            ScoreEpilogueParams e;
            e.pic = pic_tg; e.b0 = b0; e.nb = nb; e.w = width; e.pred = pred; e.mean = c->mean;
            e.u8 = d_pnn_u8 ? d_pnn_u8 + b0 * w2 : nullptr; e.targets = d_targets ? d_targets + b0 * w2 : nullptr;
            e.sse = d_pnn_sse ? d_pnn_sse + b0 : nullptr;
            HIPCHK(c, launch_score_epilogue(e, s));
            c->stat_launches++;
        }
    }
    if (want_hevc) {
        HevcBestModeParams p = best_mode_params(blocks, width, smoothing);
        p.best_mode = d_hevc_mode; p.best_sse = d_hevc_sse; p.best_pred = d_hevc_pred;
        HIPCHK(c, launch_hevc_best_mode(p, s));
        c->stat_launches++;
    }
    return PNN_OK;
}

int pnn_score_picture_pairs_hm_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                      int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w,
                                      int mask_h, int smoothing, uint8_t* d_targets, uint8_t* d_pnn_u8, float* d_pnn_f32, uint32_t* d_pnn_sse,
                                      uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred, void* stream)
{
    return score_picture_pairs(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols, positions, mask_w, mask_h,
                               nullptr, nullptr, smoothing, d_targets, d_pnn_u8, d_pnn_f32, d_pnn_sse, d_hevc_mode, d_hevc_sse, d_hevc_pred, stream);
}

// ---- masks per block (include/pnn_hip.h, "masks per block") ----
int pnn_score_picture_pairs_masks_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                         int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                         const uint8_t* d_mask_w, const uint8_t* d_mask_h, int smoothing, uint8_t* d_targets, uint8_t* d_pnn_u8,
                                         float* d_pnn_f32, uint32_t* d_pnn_sse, uint8_t* d_hevc_mode, uint32_t* d_hevc_sse, uint8_t* d_hevc_pred,
                                         void* stream)
{
    return score_picture_pairs(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols, positions, 0, 0, d_mask_w,
                               d_mask_h, smoothing, d_targets, d_pnn_u8, d_pnn_f32, d_pnn_sse, d_hevc_mode, d_hevc_sse, d_hevc_pred, stream);
}

int pnn_first_pass_picture_pairs_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                        int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w,
                                        int mask_h, const uint8_t* d_cand_pred, uint32_t* d_mode_hads, uint32_t* d_cand_hads,
                                        uint8_t* d_list_modes, uint32_t* d_list_costs, void* stream)
{
    return pnn_first_pass_picture_pairs_hm_device(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols,
                                                  positions, mask_w, mask_h, d_cand_pred, 0, d_mode_hads, d_cand_hads, d_list_modes, d_list_costs,
                                                  stream);
}

// the one body of the first-pass entries from pictures: scalar masks or masks per position, as score_picture_pairs
static int first_pass_picture_pairs(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                    int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w, int mask_h,
                                    const uint8_t* d_mask_w, const uint8_t* d_mask_h, const uint8_t* d_cand_pred, int smoothing,
                                    uint32_t* d_mode_hads, uint32_t* d_cand_hads, uint8_t* d_list_modes, uint32_t* d_list_costs, void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    BlockSource blocks = picture_pair_blocks(picture_blocks(d_context_channels, height, width_ch, d_rows, d_cols, positions, d_mask_w, d_mask_h),
                                             d_target_channels, images, mask_w, mask_h);
    if ((rc = check_pair_geometry(c, width, blocks)) || (rc = check_smoothing(c, smoothing)) ||
        (rc = check_hads_outputs(c, d_cand_pred, d_mode_hads, d_cand_hads, d_list_modes, d_list_costs)) ||
        (rc = count_blocks(c, images, positions, &blocks.n))) return rc;
    if (blocks.n == 0) return PNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if ((rc = check_picture_blocks(c, width, blocks.pic, s))) return rc;
    reset_stats(c);
    HevcModeHadsParams p = mode_hads_params(blocks, width, smoothing, d_cand_pred);
    p.mode_hads = d_mode_hads; p.cand_hads = d_cand_hads; p.list_modes = d_list_modes; p.list_costs = d_list_costs;
    HIPCHK(c, launch_hevc_mode_hads(p, s));
    c->stat_launches++;
    return PNN_OK;
}

int pnn_first_pass_picture_pairs_hm_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                           int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, uint32_t* d_mode_hads,
                                           uint32_t* d_cand_hads, uint8_t* d_list_modes, uint32_t* d_list_costs, void* stream)
{
    return first_pass_picture_pairs(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols, positions, mask_w,
                                    mask_h, nullptr, nullptr, d_cand_pred, smoothing, d_mode_hads, d_cand_hads, d_list_modes, d_list_costs, stream);
}

int pnn_first_pass_picture_pairs_masks_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                              int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                              const uint8_t* d_mask_w, const uint8_t* d_mask_h, const uint8_t* d_cand_pred, int smoothing,
                                              uint32_t* d_mode_hads, uint32_t* d_cand_hads, uint8_t* d_list_modes, uint32_t* d_list_costs,
                                              void* stream)
{
    return first_pass_picture_pairs(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols, positions, 0, 0,
                                    d_mask_w, d_mask_h, d_cand_pred, smoothing, d_mode_hads, d_cand_hads, d_list_modes, d_list_costs, stream);
}

int pnn_trquant_device(pnn_ctx* c, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const int* qps, int nb_qps,
                       uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels, uint8_t* d_recon, void* stream)
{
    return pnn_trquant_rate_device(c, width, d_predictions, d_targets, n, nullptr, qps, nb_qps, d_sses_recon, d_nb_nonzero, d_sum_abs_levels,
                                   d_recon, nullptr, stream);
}

int pnn_trquant_rate_device(pnn_ctx* c, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                            const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                            uint8_t* d_recon, uint64_t* d_rate, void* stream)
{
    return pnn_trquant_sdh_device(c, width, d_predictions, d_targets, n, d_modes, qps, nb_qps, d_sses_recon, d_nb_nonzero, d_sum_abs_levels,
                                  d_recon, d_rate, 0, stream);
}

int pnn_trquant_sdh_device(pnn_ctx* c, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                           const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                           uint8_t* d_recon, uint64_t* d_rate, int sign_data_hiding, void* stream)
{
    return pnn_trquant_rdoq_device(c, width, d_predictions, d_targets, n, d_modes, qps, nb_qps, d_sses_recon, d_nb_nonzero, d_sum_abs_levels,
                                   d_recon, d_rate, sign_data_hiding, 0, nullptr, stream);
}

int pnn_trquant_rdoq_device(pnn_ctx* c, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                            const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                            uint8_t* d_recon, uint64_t* d_rate, int sign_data_hiding, int rdoq, const double* lambdas, void* stream)
{
    if (!c) return PNN_E_ARG;
    if (const int rc = check_trquant(c, width, d_predictions, d_targets, n, qps, nb_qps,
                                     d_sses_recon || d_nb_nonzero || d_sum_abs_levels || d_recon || d_rate)) return rc;
    if (d_modes && !d_rate && !sign_data_hiding && !rdoq) return fail(c, PNN_E_ARG, "intra modes without a rate output, sign-data hiding or RDOQ");
    if (const int rc = check_rdoq_lambdas(c, rdoq, lambdas, nb_qps)) return rc;
    if (n == 0) return PNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    TrQuantParams p = trquant_params(width, d_predictions, d_targets, n, d_modes, qps, nb_qps, {sign_data_hiding, rdoq, lambdas});
    p.sse = d_sses_recon; p.nonzero = d_nb_nonzero; p.sum_abs = d_sum_abs_levels; p.recon = d_recon; p.rate = d_rate;
    reset_stats(c);
    HIPCHK(c, launch_trquant(p, (hipStream_t)stream));
    c->stat_launches++;
    return PNN_OK;
}

size_t pnn_trquant_tskip_workspace_bytes(int width, int n, int nb_qps)
{
    if (width != tskip::kWidth || n < 0 || nb_qps < 1 || nb_qps > trquant::kMaxQps) return 0;
    return tskip_workspace(nullptr, n, nb_qps).bytes;
}

int pnn_trquant_tskip_device(pnn_ctx* c, int width, const uint8_t* d_predictions, const uint8_t* d_targets, int n, const uint8_t* d_modes,
                             const int* qps, int nb_qps, uint32_t* d_sses_recon, uint32_t* d_nb_nonzero, uint32_t* d_sum_abs_levels,
                             uint8_t* d_recon, uint64_t* d_rate, int sign_data_hiding, int rdoq, const double* lambdas, int transform_skip,
                             const uint32_t* d_mode_bits, int charge_cbf, uint8_t* d_ts_flag, void* d_workspace, size_t workspace_bytes,
                             void* stream)
{
    if (!c) return PNN_E_ARG;
    if (const int rc = check_tskip_option(c, width, transform_skip, 2)) return rc;
    if (charge_cbf != 0 && charge_cbf != 1) return fail(c, PNN_E_ARG, "charge_cbf %d is not 0 or 1", charge_cbf);
    if (!transform_skip) {                                // (needs one of the five outputs of the entry it forwards to)
        const int rc = pnn_trquant_rdoq_device(c, width, d_predictions, d_targets, n, d_modes, qps, nb_qps, d_sses_recon, d_nb_nonzero,
                                               d_sum_abs_levels, d_recon, d_rate, sign_data_hiding, rdoq, lambdas, stream);
        if (rc == PNN_OK && d_ts_flag && n > 0) HIPCHK(c, hipMemsetAsync(d_ts_flag, 0, (size_t)nb_qps * n, (hipStream_t)stream));
        return rc;
    }
    if (const int rc = check_trquant(c, width, d_predictions, d_targets, n, qps, nb_qps,
                                     d_sses_recon || d_nb_nonzero || d_sum_abs_levels || d_recon || d_rate || d_ts_flag)) return rc;
    const bool decide = transform_skip == 2;
    if (const int rc = check_rdoq_lambdas(c, rdoq || decide, lambdas, nb_qps)) return rc;
    if (n == 0) return PNN_OK;
    const TskipWorkspace ws = tskip_workspace(d_workspace, n, nb_qps);
    if (!d_workspace || (uintptr_t)d_workspace % 16) return fail(c, PNN_E_ARG, "d_workspace is NULL or not aligned to 16 bytes");
    if (workspace_bytes < ws.bytes)
        return fail(c, PNN_E_ARG, "the workspace has %zu bytes, pnn_trquant_tskip_workspace_bytes asks for %zu", workspace_bytes, ws.bytes);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    TrQuantParams p = trquant_params(width, d_predictions, d_targets, n, d_modes, qps, nb_qps, {sign_data_hiding, rdoq, lambdas});
    reset_stats(c);
    for (int form = decide ? 0 : 1; form < 2; form++) {   // the transformed form first (decide only), then the skipped one
        const TskipOut& o = ws.form[form];
        p.sse = o.sse; p.nonzero = o.nonzero; p.sum_abs = o.sum_abs; p.recon = o.recon; p.rate = o.rate;
        HIPCHK(c, form ? launch_tskip4(p, s) : launch_trquant(p, s));
        c->stat_launches++;
    }
    TskipDecideParams d;
    d.N = n; d.nb_qps = nb_qps; d.decide = decide; d.charge_cbf = charge_cbf; d.mode_bits = d_mode_bits;
    d.transformed = TskipForm{ws.form[0].sse, ws.form[0].nonzero, ws.form[0].sum_abs, ws.form[0].rate, ws.form[0].recon};
    d.skipped = TskipForm{ws.form[1].sse, ws.form[1].nonzero, ws.form[1].sum_abs, ws.form[1].rate, ws.form[1].recon};
    for (int i = 0; i < trquant::kMaxQps; i++) {
        const int qp = qps[i < nb_qps ? i : 0];
        d.lambda[i] = lambdas ? lambdas[i < nb_qps ? i : 0] : pnn_hm_intra_lambda(qp);
        d.bits[i] = tskip::qp_bits(qp);
    }
    d.sse = d_sses_recon; d.nonzero = d_nb_nonzero; d.sum_abs = d_sum_abs_levels; d.recon = d_recon; d.rate = d_rate; d.ts_flag = d_ts_flag;
    HIPCHK(c, launch_tskip_decide(d, s));
    c->stat_launches++;
    return PNN_OK;
}

size_t pnn_rd_pass_workspace_bytes(int width, int n, int nb_qps)
{
    if (width_index(width) < 0 || n < 0 || nb_qps < 1 || nb_qps > trquant::kMaxQps) return 0;
    return rd_workspace(nullptr, width, n, nb_qps).bytes;
}

int pnn_rd_pass_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                       const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                       uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost,
                       uint32_t* d_best_sse, uint64_t* d_best_rate, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return pnn_rd_pass_rdoq_device(c, width, d_patterns, pattern_h, pattern_w, d_targets, n, d_cand_pred, smoothing, qps, nb_qps, lambdas,
                                   sign_data_hiding, 0, d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse, d_best_rate,
                                   d_workspace, workspace_bytes, stream);
}

int pnn_rd_pass_rdoq_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                            const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                            int rdoq, uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot,
                            double* d_best_cost, uint32_t* d_best_sse, uint64_t* d_best_rate, void* d_workspace, size_t workspace_bytes,
                            void* stream)
{
    return pnn_rd_pass_signal_device(c, width, d_patterns, pattern_h, pattern_w, d_targets, n, d_cand_pred, smoothing, qps, nb_qps, lambdas,
                                     sign_data_hiding, rdoq, 0, nullptr, nullptr, d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost,
                                     d_best_sse, d_best_rate, nullptr, nullptr, d_workspace, workspace_bytes, stream);
}

int pnn_rd_pass_picture_pairs_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                     int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w,
                                     int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas,
                                     int sign_data_hiding, uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode,
                                     uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse, uint64_t* d_best_rate, void* d_workspace,
                                     size_t workspace_bytes, void* stream)
{
    return pnn_rd_pass_rdoq_picture_pairs_device(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols,
                                                 positions, mask_w, mask_h, d_cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, 0,
                                                 d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse, d_best_rate,
                                                 d_workspace, workspace_bytes, stream);
}

int pnn_rd_pass_rdoq_picture_pairs_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                          int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                          int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                          const double* lambdas, int sign_data_hiding, int rdoq, uint8_t* d_cand_modes, double* d_cand_costs,
                                          uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                                          uint64_t* d_best_rate, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return pnn_rd_pass_signal_picture_pairs_device(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols,
                                                   positions, mask_w, mask_h, d_cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, rdoq, 0,
                                                   nullptr, nullptr, d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse,
                                                   d_best_rate, nullptr, nullptr, d_workspace, workspace_bytes, stream);
}

size_t pnn_rd_pass_signal_workspace_bytes(int width, int n, int nb_qps, int signalling)
{
    if (!signalling) return pnn_rd_pass_workspace_bytes(width, n, nb_qps);
    if (width_index(width) < 0 || n < 0 || nb_qps < 1 || nb_qps > trquant::kMaxQps) return 0;
    return rd_signal_workspace(nullptr, width, n, nb_qps, 0).bytes;
}

int pnn_rd_pass_signal_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                              const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                              int rdoq, int signalling, const uint8_t* d_left_modes, const uint8_t* d_above_modes, uint8_t* d_cand_modes,
                              double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                              uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace,
                              size_t workspace_bytes, void* stream)
{
    return pnn_rd_pass_codec_device(c, width, d_patterns, pattern_h, pattern_w, d_targets, n, d_cand_pred, smoothing, qps, nb_qps, lambdas,
                                    sign_data_hiding, rdoq, signalling, d_left_modes, d_above_modes, 0, d_cand_modes, d_cand_costs, d_best_mode,
                                    d_best_slot, d_best_cost, d_best_sse, d_best_rate, d_first_pass_costs, d_best_side_rate, d_workspace,
                                    workspace_bytes, stream);
}

int pnn_rd_pass_signal_picture_pairs_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                            int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                            int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                            const double* lambdas, int sign_data_hiding, int rdoq, int signalling, const uint8_t* d_left_modes,
                                            const uint8_t* d_above_modes, uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode,
                                            uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse, uint64_t* d_best_rate,
                                            double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace, size_t workspace_bytes,
                                            void* stream)
{
    return pnn_rd_pass_codec_picture_pairs_device(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols,
                                                  positions, mask_w, mask_h, d_cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, rdoq,
                                                  signalling, d_left_modes, d_above_modes, 0, d_cand_modes, d_cand_costs, d_best_mode, d_best_slot,
                                                  d_best_cost, d_best_sse, d_best_rate, d_first_pass_costs, d_best_side_rate, d_workspace,
                                                  workspace_bytes, stream);
}

// ---- the codec as an argument (include/pnn_hip.h, "the substitution codec") ----
size_t pnn_rd_pass_codec_workspace_bytes(int width, int n, int nb_qps, int signalling, int codec)
{
    if (codec == 0) return pnn_rd_pass_signal_workspace_bytes(width, n, nb_qps, signalling);
    if (codec != 1 || !signalling || width_index(width) < 0 || n < 0 || nb_qps < 1 || nb_qps > trquant::kMaxQps) return 0;
    return rd_signal_workspace(nullptr, width, n, nb_qps, 1).bytes;
}

int pnn_rd_pass_codec_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                             const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                             int rdoq, int signalling, const uint8_t* d_left_modes, const uint8_t* d_above_modes, int codec, uint8_t* d_cand_modes,
                             double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                             uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace,
                             size_t workspace_bytes, void* stream)
{
    if (!c) return PNN_E_ARG;
    RdPassCall q = rd_pass_call(width, dense_blocks(d_patterns, pattern_h, pattern_w, d_targets, n), d_cand_pred, smoothing, qps, nb_qps, lambdas,
                                sign_data_hiding);
    q.rdoq = rdoq; q.signalling = signalling; q.left = d_left_modes; q.above = d_above_modes; q.codec = codec;
    q.out = {d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse, d_best_rate, d_first_pass_costs, d_best_side_rate,
             nullptr};
    q.workspace = d_workspace; q.workspace_bytes = workspace_bytes; q.stream = (hipStream_t)stream;
    return rd_pass(c, q);
}

int pnn_rd_pass_codec_picture_pairs_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                           int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                           const double* lambdas, int sign_data_hiding, int rdoq, int signalling, const uint8_t* d_left_modes,
                                           const uint8_t* d_above_modes, int codec, uint8_t* d_cand_modes, double* d_cand_costs,
                                           uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                                           uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate, void* d_workspace,
                                           size_t workspace_bytes, void* stream)
{
    if (!c) return PNN_E_ARG;
    const BlockSource blocks = picture_pair_blocks(picture_blocks(d_context_channels, height, width_ch, d_rows, d_cols, positions),
                                                   d_target_channels, images, mask_w, mask_h);
    RdPassCall q = rd_pass_call(width, blocks, d_cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding);
    q.rdoq = rdoq; q.signalling = signalling; q.left = d_left_modes; q.above = d_above_modes; q.codec = codec;
    q.out = {d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse, d_best_rate, d_first_pass_costs, d_best_side_rate,
             nullptr};
    q.workspace = d_workspace; q.workspace_bytes = workspace_bytes; q.stream = (hipStream_t)stream;
    return rd_pass(c, q);
}

// ---- the second pass with transform skip (include/pnn_hip.h, "transform skip") ----
size_t pnn_rd_pass_tskip_workspace_bytes(int width, int n, int nb_qps, int signalling, int codec, int transform_skip)
{
    const size_t base = pnn_rd_pass_codec_workspace_bytes(width, n, nb_qps, signalling, codec);
    if (!transform_skip || !base) return base;
    if (transform_skip != 1 || width != tskip::kWidth) return 0;
    return base + rd_tskip_workspace(nullptr, (size_t)n * signal_slots(width, codec), n).bytes;
}

int pnn_rd_pass_tskip_device(pnn_ctx* c, int width, const uint8_t* d_patterns, int pattern_h, int pattern_w, const uint8_t* d_targets, int n,
                             const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                             int rdoq, int signalling, const uint8_t* d_left_modes, const uint8_t* d_above_modes, int codec, int transform_skip,
                             uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost,
                             uint32_t* d_best_sse, uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate,
                             uint8_t* d_best_ts_flag, void* d_workspace, size_t workspace_bytes, void* stream)
{
    if (!c) return PNN_E_ARG;
    RdPassCall q = rd_pass_call(width, dense_blocks(d_patterns, pattern_h, pattern_w, d_targets, n), d_cand_pred, smoothing, qps, nb_qps, lambdas,
                                sign_data_hiding);
    q.rdoq = rdoq; q.signalling = signalling; q.left = d_left_modes; q.above = d_above_modes; q.codec = codec;
    q.transform_skip = transform_skip; q.tskip_entry = true;
    q.out = {d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse, d_best_rate, d_first_pass_costs, d_best_side_rate,
             d_best_ts_flag};
    q.workspace = d_workspace; q.workspace_bytes = workspace_bytes; q.stream = (hipStream_t)stream;
    return rd_pass(c, q);
}

// the one body of the _tskip_ entries from picture pairs: scalar masks or masks per position, as score_picture_pairs
static int rd_pass_tskip_picture_pairs(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels, int images,
                                       int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, int mask_w, int mask_h,
                                       const uint8_t* d_mask_w, const uint8_t* d_mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps,
                                       int nb_qps, const double* lambdas, int sign_data_hiding, int rdoq, int signalling, const uint8_t* d_left_modes,
                                       const uint8_t* d_above_modes, int codec, int transform_skip, const RdPassOutputs& out, void* d_workspace,
                                       size_t workspace_bytes, void* stream)
{
    if (!c) return PNN_E_ARG;
    const BlockSource blocks = picture_pair_blocks(picture_blocks(d_context_channels, height, width_ch, d_rows, d_cols, positions, d_mask_w, d_mask_h),
                                                   d_target_channels, images, mask_w, mask_h);
    RdPassCall q = rd_pass_call(width, blocks, d_cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding);
    q.rdoq = rdoq; q.signalling = signalling; q.left = d_left_modes; q.above = d_above_modes; q.codec = codec;
    q.transform_skip = transform_skip; q.tskip_entry = true;
    q.out = out;
    q.workspace = d_workspace; q.workspace_bytes = workspace_bytes; q.stream = (hipStream_t)stream;
    return rd_pass(c, q);
}

int pnn_rd_pass_tskip_picture_pairs_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                           int mask_w, int mask_h, const uint8_t* d_cand_pred, int smoothing, const int* qps, int nb_qps,
                                           const double* lambdas, int sign_data_hiding, int rdoq, int signalling, const uint8_t* d_left_modes,
                                           const uint8_t* d_above_modes, int codec, int transform_skip, uint8_t* d_cand_modes, double* d_cand_costs,
                                           uint8_t* d_best_mode, uint8_t* d_best_slot, double* d_best_cost, uint32_t* d_best_sse,
                                           uint64_t* d_best_rate, double* d_first_pass_costs, uint64_t* d_best_side_rate, uint8_t* d_best_ts_flag,
                                           void* d_workspace, size_t workspace_bytes, void* stream)
{
    return rd_pass_tskip_picture_pairs(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols, positions, mask_w,
                                       mask_h, nullptr, nullptr, d_cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, rdoq, signalling,
                                       d_left_modes, d_above_modes, codec, transform_skip,
                                       {d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse, d_best_rate, d_first_pass_costs,
                                        d_best_side_rate, d_best_ts_flag},
                                       d_workspace, workspace_bytes, stream);
}

// The _tskip_ entry from picture pairs with masks per position in place of the call's two scalars.
int pnn_rd_pass_picture_pairs_masks_device(pnn_ctx* c, int width, const uint8_t* d_context_channels, const uint8_t* d_target_channels,
                                           int images, int height, int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions,
                                           const uint8_t* d_mask_w, const uint8_t* d_mask_h, const uint8_t* d_cand_pred, int smoothing,
                                           const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding, int rdoq, int signalling,
                                           const uint8_t* d_left_modes, const uint8_t* d_above_modes, int codec, int transform_skip,
                                           uint8_t* d_cand_modes, double* d_cand_costs, uint8_t* d_best_mode, uint8_t* d_best_slot,
                                           double* d_best_cost, uint32_t* d_best_sse, uint64_t* d_best_rate, double* d_first_pass_costs,
                                           uint64_t* d_best_side_rate, uint8_t* d_best_ts_flag, void* d_workspace, size_t workspace_bytes,
                                           void* stream)
{
    return rd_pass_tskip_picture_pairs(c, width, d_context_channels, d_target_channels, images, height, width_ch, d_rows, d_cols, positions, 0, 0,
                                       d_mask_w, d_mask_h, d_cand_pred, smoothing, qps, nb_qps, lambdas, sign_data_hiding, rdoq, signalling,
                                       d_left_modes, d_above_modes, codec, transform_skip,
                                       {d_cand_modes, d_cand_costs, d_best_mode, d_best_slot, d_best_cost, d_best_sse, d_best_rate, d_first_pass_costs,
                                        d_best_side_rate, d_best_ts_flag},
                                       d_workspace, workspace_bytes, stream);
}

// The mode statistics of a second pass whose slot modes and winners are on the device: the output is zeroed on the stream, then one
// launch adds every workgroup's counts to it.
int pnn_rd_pass_mode_stats_device(pnn_ctx* c, const uint8_t* d_slot_modes, int per_qp, int slots, const uint8_t* d_best_mode, int n, int nb_qps,
                                  uint32_t* d_stats, void* stream)
{
    if (!c) return PNN_E_ARG;
    if (n < 0) return fail(c, PNN_E_ARG, "negative batch size");
    if (slots < 1 || slots > 16) return fail(c, PNN_E_ARG, "%d slots per block: not 1 to 16", slots);
    if (nb_qps < 1 || nb_qps > trquant::kMaxQps) return fail(c, PNN_E_ARG, "the QPs are not 1 to %d", trquant::kMaxQps);
    if (!d_stats) return fail(c, PNN_E_ARG, "the output is NULL");
    if ((uintptr_t)d_stats % 4) return fail(c, PNN_E_ARG, "the output is not aligned to 4 bytes");
    if (n > 0 && (!d_slot_modes || !d_best_mode)) return fail(c, PNN_E_ARG, "the slot modes or the best modes are NULL");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    reset_stats(c);
    HIPCHK(c, hipMemsetAsync(d_stats, 0, (size_t)nb_qps * 3 * 36 * 4, s));
    if (n == 0) return PNN_OK;
    ModeStatsParams p;
    p.slot_modes = d_slot_modes; p.best_mode = d_best_mode; p.per_qp = per_qp != 0; p.S = slots; p.N = n; p.nb_qps = nb_qps; p.stats = d_stats;
    HIPCHK(c, launch_mode_stats(p, s));
    c->stat_launches++;
    return PNN_OK;
}

// The coding-tree pass on leaves that lie on the device: the refusals are cutree::refusal's, the host twin's own;
// the edge depths are read back once (the call waits for the stream) and checked before the launch, as the positions of a picture are.
// selected / selected_pnn are zeroed on the stream, then ONE launch (cu_tree_kernel) does everything.
int pnn_cu_tree_device(pnn_ctx* c, const int* qps, int nb_qps, const double* lambdas, int n_ctu, const uint32_t* const* d_dists,
                       const uint64_t* const* d_rates, const uint8_t* const* d_modes, const uint8_t* d_left_depths, const uint8_t* d_above_depths,
                       int pnn_mode, uint8_t* d_cu_depths, uint8_t* d_part_nxn, double* d_node_costs, double* d_ctu_costs, uint64_t* d_ctu_dists,
                       uint64_t* d_ctu_rates, uint32_t* d_selected, uint32_t* d_selected_pnn, void* stream)
{
    if (!c) return PNN_E_ARG;
    const bool any = d_cu_depths || d_part_nxn || d_node_costs || d_ctu_costs || d_ctu_dists || d_ctu_rates || d_selected || d_selected_pnn;
    if (const char* refusal = cutree::refusal(qps, nb_qps, lambdas, n_ctu, d_dists, d_rates, d_modes, pnn_mode, any, d_selected_pnn != nullptr))
        return fail(c, PNN_E_ARG, "%s", refusal);
    for (int k = 0; k < cutree::kWidths; k++)
        if ((uintptr_t)d_dists[k] % 4 || (uintptr_t)d_rates[k] % 8) return fail(c, PNN_E_ARG, "a leaf array is not aligned to its element");
    if ((uintptr_t)d_node_costs % 8 || (uintptr_t)d_ctu_costs % 8 || (uintptr_t)d_ctu_dists % 8 || (uintptr_t)d_ctu_rates % 8 ||
        (uintptr_t)d_selected % 4 || (uintptr_t)d_selected_pnn % 4) return fail(c, PNN_E_ARG, "an output is not aligned to its element");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (d_left_depths || d_above_depths) {
        const size_t cells = (size_t)nb_qps * n_ctu * 8;
        std::vector<uint8_t> left(d_left_depths ? cells : 0), above(d_above_depths ? cells : 0);
        {
            PNN_UNSAFE_CALLS_GUARD;
            if (d_left_depths) HIPCHK(c, hipMemcpyAsync(left.data(), d_left_depths, cells, hipMemcpyDeviceToHost, s));
            if (d_above_depths) HIPCHK(c, hipMemcpyAsync(above.data(), d_above_depths, cells, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        const char* refusal = cutree::edge_refusal(left.data(), left.size());
        if (!refusal) refusal = cutree::edge_refusal(above.data(), above.size());
        if (refusal) return fail(c, PNN_E_ARG, "%s", refusal);
    }
    reset_stats(c);
    CuTreeParams p;
    for (int k = 0; k < cutree::kWidths; k++) { p.dist[k] = d_dists[k]; p.rate[k] = d_rates[k]; p.mode[k] = d_modes ? d_modes[k] : nullptr; }
    p.left = d_left_depths; p.above = d_above_depths; p.n_ctu = n_ctu; p.nb_qps = nb_qps; p.pnn_mode = pnn_mode;
    for (int i = 0; i < cutree::kMaxQps; i++) {
        const int qp = qps[i < nb_qps ? i : 0];
        p.lambda[i] = lambdas ? lambdas[i < nb_qps ? i : 0] : pnn_hm_intra_lambda(qp);
        p.bits[i] = cutree::qp_bits(qp);
    }
    p.cu_depths = d_cu_depths; p.part_nxn = d_part_nxn; p.node_costs = d_node_costs; p.ctu_costs = d_ctu_costs; p.ctu_dists = d_ctu_dists;
    p.ctu_rates = d_ctu_rates; p.selected = d_selected; p.selected_pnn = d_selected_pnn;
    if (d_selected) HIPCHK(c, hipMemsetAsync(d_selected, 0, (size_t)nb_qps * cutree::kWidths * 4, s));
    if (d_selected_pnn) HIPCHK(c, hipMemsetAsync(d_selected_pnn, 0, (size_t)nb_qps * cutree::kWidths * 4, s));
    HIPCHK(c, launch_cu_tree(p, s));
    c->stat_launches++;
    return PNN_OK;
}

// The coding tree over whole pictures: the depth maps every CTU's edges are gathered from, [nb_qps][n_ctu][64]
// bytes -- the caller's cu_depths where given, else the caller's workspace; 0 for a grid the entry refuses.
size_t pnn_cu_tree_picture_workspace_bytes(int nb_qps, int n_images, int ctu_rows, int ctu_cols)
{
    int n_ctu = 0;
    if (nb_qps < 1 || nb_qps > cutree::kMaxQps || cutree::grid_refusal(n_images, ctu_rows, ctu_cols, &n_ctu)) return 0;
    return (size_t)nb_qps * n_ctu * cutree::kCells;
}

// No caller edges, so nothing is read back: the four sum and count outputs are zeroed on the stream, then ctu_rows + ctu_cols - 1
// launches of cu_tree_picture_kernel, one per anti-diagonal.
int pnn_cu_tree_picture_device(pnn_ctx* c, const int* qps, int nb_qps, const double* lambdas, int n_images, int ctu_rows, int ctu_cols,
                               const uint32_t* const* d_dists, const uint64_t* const* d_rates, const uint8_t* const* d_modes, int pnn_mode,
                               uint8_t* d_cu_depths, uint8_t* d_part_nxn, double* d_node_costs, double* d_ctu_costs, uint64_t* d_ctu_dists,
                               uint64_t* d_ctu_rates, uint32_t* d_selected, uint32_t* d_selected_pnn, uint64_t* d_image_dists,
                               uint64_t* d_image_rates, void* d_workspace, size_t workspace_bytes, void* stream)
{
    if (!c) return PNN_E_ARG;
    const bool any = d_cu_depths || d_part_nxn || d_node_costs || d_ctu_costs || d_ctu_dists || d_ctu_rates || d_selected || d_selected_pnn ||
                     d_image_dists || d_image_rates;
    int n_ctu = 0;
    const char* refusal = cutree::grid_refusal(n_images, ctu_rows, ctu_cols, &n_ctu);
    if (!refusal) refusal = cutree::refusal(qps, nb_qps, lambdas, n_ctu, d_dists, d_rates, d_modes, pnn_mode, any, d_selected_pnn != nullptr);
    if (refusal) return fail(c, PNN_E_ARG, "%s", refusal);
    for (int k = 0; k < cutree::kWidths; k++)
        if ((uintptr_t)d_dists[k] % 4 || (uintptr_t)d_rates[k] % 8) return fail(c, PNN_E_ARG, "a leaf array is not aligned to its element");
    if ((uintptr_t)d_node_costs % 8 || (uintptr_t)d_ctu_costs % 8 || (uintptr_t)d_ctu_dists % 8 || (uintptr_t)d_ctu_rates % 8 ||
        (uintptr_t)d_selected % 4 || (uintptr_t)d_selected_pnn % 4 || (uintptr_t)d_image_dists % 8 || (uintptr_t)d_image_rates % 8)
        return fail(c, PNN_E_ARG, "an output is not aligned to its element");
    const size_t need = pnn_cu_tree_picture_workspace_bytes(nb_qps, n_images, ctu_rows, ctu_cols);
    if (!d_workspace || (uintptr_t)d_workspace % 16) return fail(c, PNN_E_ARG, "d_workspace is NULL or not aligned to 16 bytes");
    if (workspace_bytes < need)
        return fail(c, PNN_E_ARG, "the workspace has %zu bytes, pnn_cu_tree_picture_workspace_bytes asks for %zu", workspace_bytes, need);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    reset_stats(c);
    CuTreeParams p;
    for (int k = 0; k < cutree::kWidths; k++) { p.dist[k] = d_dists[k]; p.rate[k] = d_rates[k]; p.mode[k] = d_modes ? d_modes[k] : nullptr; }
    p.left = nullptr; p.above = nullptr; p.n_ctu = n_ctu; p.nb_qps = nb_qps; p.pnn_mode = pnn_mode;
    for (int i = 0; i < cutree::kMaxQps; i++) {
        const int qp = qps[i < nb_qps ? i : 0];
        p.lambda[i] = lambdas ? lambdas[i < nb_qps ? i : 0] : pnn_hm_intra_lambda(qp);
        p.bits[i] = cutree::qp_bits(qp);
    }
    p.cu_depths = d_cu_depths ? d_cu_depths : (uint8_t*)d_workspace;          // the maps exist for the chaining either way
    p.part_nxn = d_part_nxn; p.node_costs = d_node_costs; p.ctu_costs = d_ctu_costs; p.ctu_dists = d_ctu_dists;
    p.ctu_rates = d_ctu_rates; p.selected = d_selected; p.selected_pnn = d_selected_pnn;
    const CuTreePictureGrid g{n_images, ctu_rows, ctu_cols, 0, d_image_dists, d_image_rates};
    if (d_selected) HIPCHK(c, hipMemsetAsync(d_selected, 0, (size_t)nb_qps * cutree::kWidths * 4, s));
    if (d_selected_pnn) HIPCHK(c, hipMemsetAsync(d_selected_pnn, 0, (size_t)nb_qps * cutree::kWidths * 4, s));
    if (d_image_dists) HIPCHK(c, hipMemsetAsync(d_image_dists, 0, (size_t)nb_qps * n_images * 8, s));
    if (d_image_rates) HIPCHK(c, hipMemsetAsync(d_image_rates, 0, (size_t)nb_qps * n_images * 8, s));
    HIPCHK(c, launch_cu_tree_picture(p, g, s));
    c->stat_launches += ctu_rows + ctu_cols - 1;
    return PNN_OK;
}

// One width's leaves of the coding tree from the device outputs of a second pass over the width's blocks: one launch, a copy (the tree
// reads rate + side rate as one array, and leaf buffers of the caller's own outlive the score call's output buffer).
int pnn_cu_tree_leaves_device(pnn_ctx* c, int width, int n, int nb_qps, const uint32_t* d_sses, const uint64_t* d_rates,
                              const uint64_t* d_side_rates, const uint8_t* d_modes, uint32_t* d_dist, uint64_t* d_rate, uint8_t* d_mode,
                              void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    if ((rc = check_width(c, width))) return rc;
    const int per_ctu = (64 / width) * (64 / width);
    if (n < 1 || n % per_ctu) return fail(c, PNN_E_ARG, "%d blocks of width %d: not whole CTUs of %d", n, width, per_ctu);
    if (nb_qps < 1 || nb_qps > cutree::kMaxQps) return fail(c, PNN_E_ARG, "the QPs are not 1 to %d", cutree::kMaxQps);
    if (!d_sses || !d_rates || !d_side_rates || !d_modes || !d_dist || !d_rate || !d_mode) return fail(c, PNN_E_ARG, "an array is NULL");
    if ((uintptr_t)d_sses % 4 || (uintptr_t)d_dist % 4 || (uintptr_t)d_rates % 8 || (uintptr_t)d_side_rates % 8 || (uintptr_t)d_rate % 8)
        return fail(c, PNN_E_ARG, "an array is not aligned to its element");
    HIPCHK(c, hipSetDevice(c->device));
    reset_stats(c);
    CuTreeLeavesParams p;
    p.sses = d_sses; p.rates = d_rates; p.side_rates = d_side_rates; p.modes = d_modes; p.total = (long)nb_qps * n;
    p.dist = d_dist; p.rate = d_rate; p.mode = d_mode;
    HIPCHK(c, launch_cu_tree_leaves(p, (hipStream_t)stream));
    c->stat_launches++;
    return PNN_OK;
}

int pnn_score_f32_device(pnn_ctx* c, int width, const float* d_pred_f32, const uint8_t* d_channels, int images, int height,
                         int width_ch, const int32_t* d_rows, const int32_t* d_cols, int positions, uint8_t* d_pred_u8,
                         uint32_t* d_sse, void* stream)
{
    if (!c) return PNN_E_ARG;
    int rc;
    long n;
    if ((rc = check_width(c, width)) || (rc = check_sizes(c, images, positions, height, width_ch)) ||
        (rc = check_some_output(c, d_pred_u8 || d_sse)) || (rc = count_blocks(c, images, positions, &n))) return rc;
    if (n == 0) return PNN_OK;
    if (!d_pred_f32) return fail(c, PNN_E_ARG, "NULL input buffers");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    ScoreEpilogueParams e;
    e.pic = picture_blocks(d_channels, height, width_ch, d_rows, d_cols, positions);
    if ((rc = check_picture_blocks(c, width, e.pic, s))) return rc;
    reset_stats(c);
    e.b0 = 0; e.nb = (int)n; e.w = width; e.pred = d_pred_f32; e.mean = c->mean; e.u8 = d_pred_u8; e.targets = nullptr; e.sse = d_sse;
    HIPCHK(c, launch_score_epilogue(e, s));
    c->stat_launches++;
    return PNN_OK;
}

}  // extern "C"
