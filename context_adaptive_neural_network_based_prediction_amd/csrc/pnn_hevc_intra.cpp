// Host twin of the HEVC intra predictor (no HIP in this file): one intra pattern, one mode, written the way HM writes it --
// pad the pattern into a full (2w+1)^2 one, build refMain / refSide per mode (negative angles project the side reference
// through invAngTable), predict the vertical orientation and transpose for the horizontal modes.  Same contract as the
// reference's hevc_intraprediction (hevc/intraprediction/c++/source/extracted_hevc_intraprediction.cpp:3-134): no reference
// sample smoothing, 8-bit luma, DC filtering and the mode 10 / 26 edge filter for w <= 16; -1 where the reference throws.
// pnn_hevc_intra.hip computes the same predictions in closed form; tests/test_gpu_hevc_intra.py checks one against the other.
#include "../../include/pnn_hip.h"

#include <cstdio>

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

}  // namespace

extern "C" int pnn_hevc_intra_predict(const uint8_t* intra_pattern, int pattern_h, int pattern_w, int width, int mode,
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
    int top[2 * 64 + 1], left[2 * 64 + 1], pred[64 * 64];
    for (int i = 0; i <= 2 * width; i++) {
        top[i] = intra_pattern[i < pattern_w ? i : pattern_w - 1];
        left[i] = intra_pattern[(i < pattern_h ? i : pattern_h - 1) * pattern_w];
    }
    predict(top, left, width, mode, pred);
    for (int i = 0; i < width * width; i++) out[i] = (uint8_t)pred[i];
    return 0;
}
