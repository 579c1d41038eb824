// Stand-alone driver for the AddressSanitizer + UBSan build of the host entries of the substitution codec and of the mode statistics
// (tests/test_substitution.py compiles it together with csrc/pnn_rd_pass.cpp, pnn_hevc_intra.cpp and pnn_trquant.cpp):
// pnn_first_pass_codec_host, pnn_rd_pass_codec_host and pnn_rd_pass_mode_stats_host on the smallest case at each width, with buffers of
// exactly the documented sizes, every output together and a few alone, given neighbours and NULL, RDOQ off and on, both codecs.  Any
// report aborts; a few known answers are checked on the way.
#include "pnn_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_substitution: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

int main()
{
    const int widths[5] = {4, 8, 16, 32, 64}, qps[2] = {22, 51}, nq = 2, n = 3;
    const double own[2] = {0.5, 200.};
    for (int w : widths) {
        const int k = pnn_first_pass_list_size(w), s = pnn_rd_pass_codec_slot_count(w, 1, 1);
        CHECK(s == k + 2 && pnn_rd_pass_codec_slot_count(w, 1, 0) == k + 3 && pnn_rd_pass_codec_slot_count(w, 0, 0) == k + 1);
        CHECK(pnn_rd_pass_codec_slot_count(w, 0, 1) == -1 && pnn_rd_pass_codec_slot_count(w, 1, 2) == -1);
        const size_t w2 = (size_t)w * w;
        for (int side : {w + 1, 2 * w + 1}) {
            const size_t pat = (size_t)side * side;
            std::vector<uint8_t> patterns(n * pat), targets(n * w2), cand(n * w2), left(n), above(n);
            for (size_t i = 0; i < patterns.size(); i++) patterns[i] = (uint8_t)(i * 37 + 11 * w + (i / pat) * 50);
            for (size_t i = 0; i < targets.size(); i++) {
                targets[i] = (uint8_t)(i * 29 + 3 + (i % w) * 5);
                cand[i] = i / w2 == 1 ? targets[i] : i / w2 == 2 ? (uint8_t)(255 - targets[i]) : (uint8_t)(targets[i] ^ (i % 7));
            }
            for (int b = 0; b < n; b++) { left[b] = (uint8_t)(b == 0 ? 255 : 18); above[b] = (uint8_t)(b == 2 ? 18 : 17); }
            std::vector<uint8_t> list((size_t)nq * n * k), slots((size_t)nq * n * s);
            std::vector<double> list_costs((size_t)nq * n * k);
            CHECK(pnn_first_pass_codec_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, nullptr, left.data(), above.data(), 1,
                                            list.data(), list_costs.data(), slots.data()) == PNN_OK);
            for (size_t i = 0; i < (size_t)nq * n; i++) {
                CHECK(!memcmp(list.data() + i * k, slots.data() + i * s, k));
                for (int j = 1; j < k; j++) CHECK(list_costs[i * k + j - 1] <= list_costs[i * k + j]);
                for (int j = 0; j < s; j++) CHECK(slots[i * s + j] < 35 || slots[i * s + j] == 255);
                bool has18 = false;                                       // blocks 1 and 2 have 18 as their first MPM: listed or appended
                for (int j = 0; j < s; j++) has18 = has18 || slots[i * s + j] == 18;
                CHECK(i % n == 0 || has18);
            }
            for (int rdoq = 0; rdoq <= (w <= 8 || (w == 64 && side == w + 1) ? 1 : 0); rdoq++) {   // (64: the quadrants' own path)
                std::vector<uint8_t> modes((size_t)nq * n * s), bm(nq * n), bs(nq * n), alone8(nq * n);
                std::vector<double> costs((size_t)nq * n * s), bc(nq * n), fp((size_t)nq * n * k);
                std::vector<uint32_t> sse(nq * n);
                std::vector<uint64_t> rate(nq * n), side_rate(nq * n), alone64(nq * n);
                CHECK(pnn_rd_pass_codec_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, left.data(),
                                             above.data(), 1, modes.data(), costs.data(), bm.data(), bs.data(), bc.data(), sse.data(), rate.data(),
                                             fp.data(), side_rate.data()) == PNN_OK);
                for (size_t at = 0; at < (size_t)nq * n; at++) {
                    CHECK(bs[at] < s && bm[at] == modes[at * s + bs[at]] && bm[at] < 35 && bc[at] == costs[at * s + bs[at]]);
                    for (int j = 0; j < s; j++) CHECK(bc[at] <= costs[at * s + j] && (std::isinf(costs[at * s + j]) == (modes[at * s + j] == 255)));
                    CHECK(side_rate[at] > 0);
                }
                CHECK(pnn_rd_pass_codec_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, left.data(),
                                             above.data(), 1, nullptr, nullptr, alone8.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK &&
                      alone8 == bm);
                CHECK(pnn_rd_pass_codec_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, left.data(),
                                             above.data(), 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, alone64.data()) == PNN_OK &&
                      alone64 == side_rate);
                CHECK(pnn_rd_pass_codec_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, nullptr, nullptr,
                                             1, nullptr, nullptr, alone8.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
                // the statistics of this run, [nb_qps][n][s], and of the same slots read as one QP's for both
                std::vector<uint32_t> stats((size_t)nq * 3 * 36);
                CHECK(pnn_rd_pass_mode_stats_host(modes.data(), 1, s, bm.data(), n, nq, stats.data()) == PNN_OK);
                for (int qi = 0; qi < nq; qi++) {
                    uint32_t wins = 0, first = 0;
                    for (int m = 0; m < 36; m++) { wins += stats[(qi * 3 + 2) * 36 + m]; first += stats[(qi * 3 + 1) * 36 + m]; }
                    CHECK(wins == (uint32_t)n && first == (uint32_t)n && stats[(qi * 3) * 36 + 35] == 0);
                }
                CHECK(pnn_rd_pass_mode_stats_host(modes.data(), 0, s, bm.data(), n, nq, stats.data()) == PNN_OK);
            }
            // codec 0 with the same buffers' sizes for K + 3 slots
            const int s0 = k + 3;
            std::vector<uint8_t> modes0((size_t)nq * n * s0), bm0(nq * n);
            CHECK(pnn_rd_pass_codec_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 0, qps, nq, nullptr, 0, 0, 1, nullptr, nullptr, 0,
                                         modes0.data(), nullptr, bm0.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
            std::vector<uint32_t> stats0((size_t)nq * 3 * 36);
            CHECK(pnn_rd_pass_mode_stats_host(modes0.data(), 1, s0, bm0.data(), n, nq, stats0.data()) == PNN_OK);
            CHECK(stats0[35] == (uint32_t)n);                              // 35 occupies a slot of every block
        }
    }
    // refusals read nothing and write nothing
    uint8_t byte = 0, out = 7, bad = 35;
    const int good_qp = 22;
    uint32_t stat = 9;
    CHECK(pnn_rd_pass_codec_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, 0, 1, &bad, nullptr, 1, &out, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_codec_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, 0, 0, nullptr, nullptr, 1, &out, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_codec_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, 0, 1, nullptr, nullptr, 2, &out, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_codec_host(&byte, 9, 9, &byte, 4, 1, nullptr, 0, &good_qp, 1, nullptr, 0, 0, 1, nullptr, nullptr, 1, &out, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_codec_host(nullptr, 9, 9, nullptr, 4, 0, nullptr, 0, &good_qp, 1, nullptr, 0, 0, 1, nullptr, nullptr, 1, &out, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
    CHECK(pnn_rd_pass_mode_stats_host(&byte, 0, 0, &byte, 1, 1, &stat) == PNN_E_ARG && pnn_rd_pass_mode_stats_host(&byte, 0, 1, &byte, 1, 9, &stat) == PNN_E_ARG);
    CHECK(pnn_rd_pass_mode_stats_host(nullptr, 0, 1, &byte, 1, 1, &stat) == PNN_E_ARG && pnn_rd_pass_mode_stats_host(&byte, 0, 1, &byte, 1, 1, nullptr) == PNN_E_ARG);
    CHECK(out == 7 && stat == 9);
    printf("sanitize_substitution: ok\n");
    return 0;
}
