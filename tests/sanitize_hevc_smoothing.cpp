// Stand-alone driver for the AddressSanitizer + UBSan build of the host twin's reference-sample smoothing (tests/test_hevc_smoothing.py
// compiles it together with csrc/pnn_hevc_intra.cpp): pnn_hevc_mode_uses_smoothing, pnn_hevc_smoothed_reference_host,
// pnn_hevc_intra_predict_hm and pnn_hevc_mode_hads_hm_host on crafted w = 32 lines (strong, half-flat, at the threshold, masked) and on
// the smallest and largest pattern sides of every width, in buffers of exactly the documented sizes.  Any report aborts; a few known
// answers are checked on the way.
#include "pnn_hip.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_hevc_smoothing: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

namespace {

// a dense pattern [h][wd] whose first column / row hold line[2w - i] / line[2w + i]; the inside is never read
std::vector<uint8_t> pattern_of_line(const std::vector<int>& line, int w, int h, int wd)
{
    std::vector<uint8_t> pat((size_t)h * wd, 255);
    for (int i = 0; i < h; i++) pat[(size_t)i * wd] = (uint8_t)line[2 * w - i];
    for (int i = 0; i < wd; i++) pat[i] = (uint8_t)line[2 * w + i];
    return pat;
}

// the w = 32 line through five anchors, linear in between, +-3 zigzag off the anchors
std::vector<int> crafted_line(int bl, int ml, int tl, int ma, int tr)
{
    const int a[5] = {bl, ml, tl, ma, tr};
    std::vector<int> line(129);
    for (int i = 0; i < 129; i++) {
        const int s = i == 128 ? 3 : i / 32, f = i - 32 * s;
        line[i] = (a[s] * (32 - f) + a[s + 1] * f + 16) / 32 + (i % 32 == 0 ? 0 : i % 2 ? 3 : -3);
        if (line[i] < 0) line[i] = 0;
    }
    return line;
}

void run_block(const std::vector<uint8_t>& pat, int h, int wd, int w, int expect_strong)
{
    const int w2 = w * w, k = pnn_first_pass_list_size(w);
    std::vector<uint8_t> target(w2), cand(w2), line(4 * w + 1), pred(w2), modes(k);
    std::vector<uint32_t> hads(35), costs(k);
    uint32_t cand_hads = 0;
    for (int i = 0; i < w2; i++) { target[i] = (uint8_t)(i * 37 + 11); cand[i] = (uint8_t)(i * 37 + 14); }
    for (int smoothing = 0; smoothing <= 2; smoothing++) {
        int strong = -1;
        CHECK(pnn_hevc_smoothed_reference_host(pat.data(), h, wd, w, smoothing, line.data(), &strong) == PNN_OK);
        CHECK(strong == (smoothing == 2 && expect_strong > 0 ? 1 : 0) || expect_strong < 0);
        CHECK(pnn_hevc_smoothed_reference_host(pat.data(), h, wd, w, smoothing, line.data(), nullptr) == PNN_OK);
        CHECK(line[0] == pat[(size_t)(h - 1) * wd] && line[4 * w] == pat[wd - 1]);          // the ends: copies of the padded line's
        for (int mode = 0; mode < 35; mode++) CHECK(pnn_hevc_intra_predict_hm(pat.data(), h, wd, w, mode, smoothing, pred.data()) == 0);
        CHECK(pnn_hevc_mode_hads_hm_host(pat.data(), h, wd, target.data(), w, 1, cand.data(), smoothing, hads.data(), &cand_hads, modes.data(),
                                         costs.data()) == PNN_OK);
        CHECK(pnn_hevc_mode_hads_hm_host(pat.data(), h, wd, target.data(), w, 1, nullptr, smoothing, nullptr, nullptr, modes.data(), nullptr) == PNN_OK);
        for (int j = 1; j < k; j++) CHECK(costs[j - 1] <= costs[j]);
    }
}

}  // namespace

int main()
{
    const int widths[5] = {4, 8, 16, 32, 64};
    for (int w : widths) {
        int smoothed = 0;
        for (int mode = 0; mode < 35; mode++) smoothed += pnn_hevc_mode_uses_smoothing(w, mode);
        CHECK(smoothed == (w == 8 ? 4 : w == 16 ? 28 : w == 32 ? 32 : 0));
        // the smallest and the largest pattern sides, and both mixed ones: random-looking samples
        const int sides[2] = {w + 1, 2 * w + 1};
        for (int h : sides)
            for (int wd : sides) {
                std::vector<int> line(4 * w + 1);
                for (int i = 0; i <= 4 * w; i++) line[i] = (i * 73 + 5 * w) & 255;
                run_block(pattern_of_line(line, w, h, wd), h, wd, w, -1);
                // a constant line stays constant under every filter
                std::vector<uint8_t> flat((size_t)h * wd, 255), out(4 * w + 1);
                for (int i = 0; i < h; i++) flat[(size_t)i * wd] = 97;
                for (int i = 0; i < wd; i++) flat[i] = 97;
                for (int smoothing = 0; smoothing <= 2; smoothing++) {
                    CHECK(pnn_hevc_smoothed_reference_host(flat.data(), h, wd, w, smoothing, out.data(), nullptr) == PNN_OK);
                    for (int i = 0; i <= 4 * w; i++) CHECK(out[i] == 97);
                }
            }
    }
    // the crafted w = 32 lines: both sides flat, one side, none, anchor differences of exactly 7 and 8, a masked block
    run_block(pattern_of_line(crafted_line(100, 108, 116, 124, 132), 32, 65, 65), 65, 65, 32, 1);
    run_block(pattern_of_line(crafted_line(100, 118, 116, 124, 132), 32, 65, 65), 65, 65, 32, 0);
    run_block(pattern_of_line(crafted_line(100, 108, 116, 134, 132), 32, 65, 65), 65, 65, 32, 0);
    run_block(pattern_of_line(crafted_line(100, 118, 116, 134, 132), 32, 65, 65), 65, 65, 32, 0);
    run_block(pattern_of_line(crafted_line(100, 105, 117, 125, 133), 32, 65, 65), 65, 65, 32, 1);
    run_block(pattern_of_line(crafted_line(100, 104, 116, 124, 132), 32, 65, 65), 65, 65, 32, 0);
    run_block(pattern_of_line(crafted_line(0, 119, 116, 114, 0), 32, 33, 33), 33, 33, 32, 1);
    // refusals write nothing and read nothing
    uint8_t byte = 0;
    CHECK(pnn_hevc_mode_uses_smoothing(12, 0) == PNN_E_ARG && pnn_hevc_mode_uses_smoothing(8, 35) == PNN_E_ARG);
    CHECK(pnn_hevc_smoothed_reference_host(&byte, 9, 9, 8, 3, &byte, nullptr) == PNN_E_ARG);
    CHECK(pnn_hevc_intra_predict_hm(&byte, 9, 9, 8, 0, -1, &byte) == PNN_E_ARG);
    CHECK(pnn_hevc_mode_hads_hm_host(&byte, 9, 9, &byte, 8, 1, nullptr, 3, reinterpret_cast<uint32_t*>(&byte), nullptr, nullptr, nullptr) == PNN_E_ARG);
    printf("sanitize_hevc_smoothing: ok\n");
    return 0;
}
