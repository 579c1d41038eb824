// Host twin of the HEVC intra predictor (no HIP in this file): one intra pattern, one mode, written the way HM writes it --
// pad the pattern into a full (2w+1)^2 one, build refMain / refSide per mode (negative angles project the side reference
// through invAngTable), predict the vertical orientation and transpose for the horizontal modes.  Same contract as the
// reference's hevc_intraprediction (hevc/intraprediction/c++/source/extracted_hevc_intraprediction.cpp:3-134): no reference
// sample smoothing (smoothing = 0), 8-bit luma, DC filtering and the mode 10 / 26 edge filter for w <= 16; -1 where the reference throws.
// pnn_hevc_intra.hip computes the same predictions in closed form; tests/test_gpu_hevc_intra.py checks one against the other.
// pnn_hevc_mode_hads_host is the host twin of the first-pass ranking (hevc_mode_hads_kernel): the 35 predictions above, HM's
// xGetHADs written from its rule, and xUpdateCandList; tests/test_gpu_mode_hads.py checks the kernel against it.
// HM's reference-sample smoothing (TComPattern.cpp:410-478, :721-746; TComPrediction.cpp:39-55) is an option of the *_hm entries:
// `smoothing` 0 = none (the reference's extracted predictor, what the older entries compute: they are the 0 case of the same bodies),
// 1 = the [1 2 1] filter for the modes and sizes HM filters, 2 = HM's default, which also allows the strong (bilinear) filter on flat
// 32 x 32 neighbourhoods.  tests/test_hevc_smoothing.py pins it to a numpy restatement, tests/test_gpu_hevc_smoothing.py the kernels to it.
#include "../../include/pnn_hip.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {

constexpr int kAng[9] = {0, 2, 5, 9, 13, 17, 21, 26, 32};                    // angTable
constexpr int kInvAng[9] = {0, 4096, 1638, 910, 630, 482, 390, 315, 256};    // invAngTable

int log2_width(int w)
{
    switch (w) { case 4: return 2; case 8: return 3; case 16: return 4; case 32: return 5; case 64: return 6; default: return -1; }
}

// top[0..2w] = corner, above, above-right; left[0..2w] = corner, left, below-left (both padded as the reference pads)
void predict(const int* top, const int* left, int w, int mode, int* pred)
{
    const int shift = log2_width(w);
    if (mode == 0) {                                                          // xPredIntraPlanar
        for (int y = 0; y < w; y++)
            for (int x = 0; x < w; x++)
                pred[y * w + x] = ((w - 1 - x) * left[1 + y] + (x + 1) * top[1 + w] + (w - 1 - y) * top[1 + x] +
                                   (y + 1) * left[1 + w] + w) >> (shift + 1);
        return;
    }
    if (mode == 1) {                                                          // predIntraGetPredValDC + xDCPredFiltering
        int sum = 0;
        for (int i = 0; i < w; i++) sum += top[1 + i] + left[1 + i];
        const int dc = (sum + w) / (2 * w);
        for (int i = 0; i < w * w; i++) pred[i] = dc;
        if (w <= 16) {
            pred[0] = (top[1] + left[1] + 2 * dc + 2) >> 2;
            for (int i = 1; i < w; i++) {
                pred[i] = (top[1 + i] + 3 * dc + 2) >> 2;
                pred[i * w] = (left[1 + i] + 3 * dc + 2) >> 2;
            }
        }
        return;
    }
    const bool vertical = mode >= 18;                                         // xPredIntraAng
    const int rel = vertical ? mode - 26 : 10 - mode, abs_rel = rel < 0 ? -rel : rel;
    const int ang = rel < 0 ? -kAng[abs_rel] : kAng[abs_rel];
    const int* main_src = vertical ? top : left;
    const int* side_src = vertical ? left : top;
    int buf[3 * 64 + 1];
    int* ref_main = buf + w;                                                  // indices -w .. 2w
    for (int k = 0; k <= 2 * w; k++) ref_main[k] = main_src[k];
    if (ang < 0) {
        const int inv = kInvAng[abs_rel];
        for (int k = -1, acc = 128; k > (w * ang) >> 5; k--) {
            acc += inv;
            ref_main[k] = side_src[acc >> 8];
        }
    }
    // p[v][u]: v along the side reference, u along the main one (p = pred for vertical modes, its transpose otherwise)
    for (int v = 0; v < w; v++) {
        const int pos = (v + 1) * ang, di = pos >> 5, f = pos & 31;
        for (int u = 0; u < w; u++) {
            int p = ref_main[u + di + 1];
            if (f) p = ((32 - f) * p + f * ref_main[u + di + 2] + 16) >> 5;
            if (ang == 0 && u == 0 && w <= 16) {
                p += (side_src[v + 1] - side_src[0]) >> 1;
                p = p < 0 ? 0 : p > 255 ? 255 : p;
            }
            pred[vertical ? v * w + u : u * w + v] = p;
        }
    }
}

// TComRdCost::xGetHADs for 8-bit video (TComRdCost.cpp:1753-1824): per t x t sub-block (t = 8, 4 for 4-wide blocks) the Walsh-Hadamard
// transform of org - pred, the sum of the absolute coefficients rounded (s + 2) >> 2 (t = 8) or (s + 1) >> 1 (t = 4); summed over the block.
uint32_t hads(const uint8_t* org, const int* pred, int w)
{
    const int t = w == 4 ? 4 : 8;
    uint32_t total = 0;
    for (int by = 0; by < w; by += t)
        for (int bx = 0; bx < w; bx += t) {
            int d[64];
            for (int y = 0; y < t; y++)
                for (int x = 0; x < t; x++) d[y * t + x] = (int)org[(by + y) * w + bx + x] - pred[(by + y) * w + bx + x];
            for (int pass = 0; pass < 2; pass++) {                            // rows, then columns
                const int es = pass == 0 ? 1 : t, vs = pass == 0 ? t : 1;
                for (int v = 0; v < t; v++)
                    for (int len = 1; len < t; len <<= 1)
                        for (int i = 0; i < t; i += len << 1)
                            for (int j = i; j < i + len; j++) {
                                const int a = d[v * vs + j * es], b = d[v * vs + (j + len) * es];
                                d[v * vs + j * es] = a + b;
                                d[v * vs + (j + len) * es] = a - b;
                            }
            }
            uint32_t sum = 0;
            for (int k = 0; k < t * t; k++) sum += (uint32_t)(d[k] < 0 ? -d[k] : d[k]);
            total += t == 8 ? (sum + 2) >> 2 : (sum + 1) >> 1;
        }
    return total;
}

// TEncSearch::xUpdateCandList with the cost alone: the entry goes in front of the first strictly larger cost, the last one drops out
void update_cand_list(int mode, uint32_t cost, int k, int* list_modes, uint64_t* list_costs)
{
    int shift = 0;
    while (shift < k && cost < list_costs[k - 1 - shift]) shift++;
    if (!shift) return;
    for (int i = 1; i < shift; i++) {
        list_modes[k - i] = list_modes[k - 1 - i];
        list_costs[k - i] = list_costs[k - 1 - i];
    }
    list_modes[k - shift] = mode;
    list_costs[k - shift] = cost;
}

// intraFilterThreshold: a mode reads smoothed samples iff it is not DC and lies further than thr[w] from both pure directions
bool mode_smooths(int w, int mode)
{
    const int thr = w == 8 ? 7 : w == 16 ? 1 : w == 32 ? 0 : 10;
    const int dh = mode > 10 ? mode - 10 : 10 - mode, dv = mode > 26 ? mode - 26 : 26 - mode;
    return mode != 1 && (dh < dv ? dh : dv) > thr;
}

bool smoothing_ok(int smoothing)
{
    if (smoothing >= 0 && smoothing <= 2) return true;
    fprintf(stderr, "The reference-sample smoothing %d is not 0 (none), 1 (HM without StrongIntraSmoothing) or 2 (HM).\n", smoothing);
    return false;
}

// The padding rule, its one home: line[2w + j], j in [-2w, 2w], = the corner at j = 0, left / below-left below it (first column), above /
// above-right to the right (first row); a short row or column is extended with its last sample.
void padded_line(const uint8_t* pat, int ph, int pw, int w, int* line)
{
    for (int i = 0; i <= 2 * w; i++) {
        line[2 * w + i] = pat[i < pw ? i : pw - 1];
        line[2 * w - i] = pat[(i < ph ? i : ph - 1) * pw];
    }
}

// filteringIntraReferenceSamples on the padded line (HM substitutes first, filters afterwards): both ends copied; strong (w = 32,
// `allow_strong`, both halves flat at their three anchors): the corner copied, each side bilinear between its anchors; else [1 2 1].
bool smooth_line(const int* line, int w, bool allow_strong, int* out)
{
    const int* rf = line + 2 * w;
    int* o = out + 2 * w;
    o[-2 * w] = rf[-2 * w];
    o[2 * w] = rf[2 * w];
    bool strong = false;
    if (w == 32 && allow_strong) {
        const int bl = rf[-64], tl = rf[0], tr = rf[64], thr = 1 << (8 - 5);
        const int dl = bl + tl - 2 * rf[-32], da = tl + tr - 2 * rf[32];
        strong = (dl < 0 ? -dl : dl) < thr && (da < 0 ? -da : da) < thr;
        if (strong) {
            o[0] = tl;
            for (int i = 1; i < 64; i++) {
                o[-64 + i] = ((64 - i) * bl + i * tl + 32) >> 6;
                o[i] = ((64 - i) * tl + i * tr + 32) >> 6;
            }
        }
    }
    if (!strong)
        for (int j = -2 * w + 1; j < 2 * w; j++) o[j] = (rf[j - 1] + 2 * rf[j] + rf[j + 1] + 2) >> 2;
    return strong;
}

// The reference samples of one pattern as predict() takes them: [0] the plain ones, [1] the ones the smoothed modes read (the same
// when `smoothing` is 0 or no mode of this width smooths).
struct RefSamples {
    int top[2][2 * 64 + 1], left[2][2 * 64 + 1];
    bool strong;
    RefSamples(const uint8_t* pat, int ph, int pw, int w, int smoothing) : strong(false)
    {
        int line[2][4 * 64 + 1];
        padded_line(pat, ph, pw, w, line[0]);
        const bool any = smoothing != 0 && (w == 8 || w == 16 || w == 32);
        if (any) strong = smooth_line(line[0], w, smoothing == 2, line[1]);
        for (int s = 0; s < 2; s++)
            for (int i = 0; i <= 2 * w; i++) {
                top[s][i] = line[any ? s : 0][2 * w + i];
                left[s][i] = line[any ? s : 0][2 * w - i];
            }
    }
    void predict_mode(int w, int mode, int* pred) const
    {
        const int s = mode_smooths(w, mode) ? 1 : 0;
        predict(top[s], left[s], w, mode, pred);
    }
};

bool pattern_sides_ok(int pattern_h, int pattern_w, int width)
{
    return pattern_h >= width + 1 && pattern_h <= 2 * width + 1 && pattern_w >= width + 1 && pattern_w <= 2 * width + 1;
}

}  // namespace

extern "C" int pnn_first_pass_list_size(int width)
{
    if (log2_width(width) < 0) return PNN_E_ARG;
    return width <= 8 ? 8 : 3;                                                // g_aucIntraModeNumFast_UseMPM
}

extern "C" int pnn_hevc_mode_uses_smoothing(int width, int mode)
{
    if (log2_width(width) < 0) { fprintf(stderr, "The width of the target patch is not 4, 8, 16, 32 or 64.\n"); return PNN_E_ARG; }
    if (mode < 0 || mode > 34) { fprintf(stderr, "The direction is not smaller than 34.\n"); return PNN_E_ARG; }
    return mode_smooths(width, mode) ? 1 : 0;
}

extern "C" int pnn_hevc_smoothed_reference_host(const uint8_t* pattern, int pattern_h, int pattern_w, int width, int smoothing, uint8_t* line,
                                                int* strong_used)
{
    if (!pattern || !line) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (log2_width(width) < 0) { fprintf(stderr, "The width of the target patch is not 4, 8, 16, 32 or 64.\n"); return PNN_E_ARG; }
    if (!pattern_sides_ok(pattern_h, pattern_w, width)) {
        fprintf(stderr, "A side of the intra pattern does not belong to [%d, %d].\n", width + 1, 2 * width + 1);
        return PNN_E_ARG;
    }
    if (!smoothing_ok(smoothing)) return PNN_E_ARG;
    const RefSamples r(pattern, pattern_h, pattern_w, width, smoothing);
    for (int i = 0; i <= 2 * width; i++) {
        line[2 * width + i] = (uint8_t)r.top[1][i];
        line[2 * width - i] = (uint8_t)r.left[1][i];
    }
    if (strong_used) *strong_used = r.strong ? 1 : 0;
    return PNN_OK;
}

extern "C" int pnn_hevc_mode_hads_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                       const uint8_t* cand_pred, uint32_t* mode_hads, uint32_t* cand_hads, uint8_t* list_modes,
                                       uint32_t* list_costs)
{
    return pnn_hevc_mode_hads_hm_host(patterns, pattern_h, pattern_w, targets, width, n, cand_pred, 0, mode_hads, cand_hads, list_modes, list_costs);
}

extern "C" int pnn_hevc_mode_hads_hm_host(const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width, int n,
                                          const uint8_t* cand_pred, int smoothing, uint32_t* mode_hads, uint32_t* cand_hads, uint8_t* list_modes,
                                          uint32_t* list_costs)
{
    if (log2_width(width) < 0) return PNN_E_ARG;
    if (!pattern_sides_ok(pattern_h, pattern_w, width)) return PNN_E_ARG;
    if (n < 0 || (n > 0 && (!patterns || !targets))) return PNN_E_ARG;
    if (!smoothing_ok(smoothing)) return PNN_E_ARG;
    if (!mode_hads && !cand_hads && !list_modes && !list_costs) return PNN_E_ARG;
    if (cand_hads && !cand_pred) return PNN_E_ARG;
    const int w2 = width * width, k = width <= 8 ? 8 : 3;
    std::vector<int> pred(w2);
    for (long b = 0; b < n; b++) {
        const uint8_t* org = targets + (size_t)b * w2;
        const RefSamples refs(patterns + (size_t)b * pattern_h * pattern_w, pattern_h, pattern_w, width, smoothing);
        int modes[8];
        uint64_t costs[8];
        for (int i = 0; i < k; i++) { modes[i] = 255; costs[i] = UINT64_MAX; }  // HM starts the list at MAX_DOUBLE
        for (int mode = 0; mode < 35; mode++) {
            refs.predict_mode(width, mode, pred.data());
            const uint32_t c = hads(org, pred.data(), width);
            if (mode_hads) mode_hads[b * 35 + mode] = c;
            update_cand_list(mode, c, k, modes, costs);
        }
        if (cand_pred) {
            for (int i = 0; i < w2; i++) pred[i] = cand_pred[(size_t)b * w2 + i];
            const uint32_t c = hads(org, pred.data(), width);
            if (cand_hads) cand_hads[b] = c;
            update_cand_list(35, c, k, modes, costs);
        }
        for (int i = 0; i < k; i++) {
            if (list_modes) list_modes[b * k + i] = (uint8_t)modes[i];
            if (list_costs) list_costs[b * k + i] = (uint32_t)costs[i];
        }
    }
    return PNN_OK;
}

extern "C" int pnn_hevc_intra_predict(const uint8_t* intra_pattern, int pattern_h, int pattern_w, int width, int mode,
                                      uint8_t* out)
{
    return pnn_hevc_intra_predict_hm(intra_pattern, pattern_h, pattern_w, width, mode, 0, out);
}

extern "C" int pnn_hevc_intra_predict_hm(const uint8_t* intra_pattern, int pattern_h, int pattern_w, int width, int mode, int smoothing,
                                         uint8_t* out)
{
    if (!intra_pattern || !out) { fprintf(stderr, "NULL pointer.\n"); return -1; }
    if (mode < 0 || mode > 34) { fprintf(stderr, "The direction is not smaller than 34.\n"); return -1; }
    if (log2_width(width) < 0) { fprintf(stderr, "The width of the target patch is not 4, 8, 16, 32 or 64.\n"); return -1; }
    if (pattern_h < width + 1 || pattern_h > 2 * width + 1) {
        fprintf(stderr, "The height of the intra pattern does not belong to [%d, %d].\n", width + 1, 2 * width + 1);
        return -1;
    }
    if (pattern_w < width + 1 || pattern_w > 2 * width + 1) {
        fprintf(stderr, "The width of the intra pattern does not belong to [%d, %d].\n", width + 1, 2 * width + 1);
        return -1;
    }
    if (!smoothing_ok(smoothing)) return PNN_E_ARG;
    int pred[64 * 64];
    RefSamples(intra_pattern, pattern_h, pattern_w, width, smoothing).predict_mode(width, mode, pred);
    for (int i = 0; i < width * width; i++) out[i] = (uint8_t)pred[i];
    return 0;
}
