// Stand-alone driver for the AddressSanitizer + UBSan build of the host entries of the mode signalling (tests/test_mode_signal.py
// compiles it together with csrc/pnn_rd_pass.cpp, pnn_hevc_intra.cpp and pnn_trquant.cpp): pnn_intra_mode_signal_host over every pair
// of neighbours, pnn_first_pass_signal_host and pnn_rd_pass_signal_host at every width they take with buffers of exactly the
// documented sizes, every output alone, NULL neighbours and given ones, RDOQ off and on.  Any report aborts; a few known answers are
// checked on the way.
#include "pnn_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_mode_signal: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

int main()
{
    // the unit entry: 37 x 37 pairs
    {
        std::vector<uint8_t> left, above;
        for (int l = 0; l <= 36; l++)
            for (int a = 0; a <= 36; a++) { left.push_back(l == 36 ? 255 : (uint8_t)l); above.push_back(a == 36 ? 255 : (uint8_t)a); }
        const int n = (int)left.size();
        std::vector<uint8_t> mpm((size_t)n * 3), num(n);
        std::vector<uint32_t> bits((size_t)n * 36), cbf(4);
        for (int qp : {0, 22, 37, 51}) {
            CHECK(pnn_intra_mode_signal_host(left.data(), above.data(), n, qp, 1, mpm.data(), num.data(), bits.data(), cbf.data()) == PNN_OK);
            for (int b = 0; b < n; b++) {
                CHECK(num[b] == (left[b] == above[b] || (left[b] == 255 && above[b] == 1) || (left[b] == 1 && above[b] == 255) ? 1 : 2));
                CHECK(mpm[b * 3] < 35 && mpm[b * 3 + 1] < 35 && mpm[b * 3 + 2] < 35);
                CHECK(mpm[b * 3] != mpm[b * 3 + 1] && mpm[b * 3] != mpm[b * 3 + 2] && mpm[b * 3 + 1] != mpm[b * 3 + 2]);
                CHECK(bits[b * 36 + mpm[b * 3]] + 32768 == bits[b * 36 + mpm[b * 3 + 1]] && bits[b * 36 + mpm[b * 3 + 1]] == bits[b * 36 + mpm[b * 3 + 2]]);
            }
            std::vector<uint8_t> alone((size_t)n * 3);
            CHECK(pnn_intra_mode_signal_host(left.data(), above.data(), n, qp, 1, alone.data(), nullptr, nullptr, nullptr) == PNN_OK && alone == mpm);
            std::vector<uint32_t> bits_alone(bits.size());
            CHECK(pnn_intra_mode_signal_host(left.data(), above.data(), n, qp, 1, nullptr, nullptr, bits_alone.data(), nullptr) == PNN_OK && bits_alone == bits);
        }
        uint8_t none_mpm[3];
        CHECK(pnn_intra_mode_signal_host(nullptr, nullptr, 1, 30, 0, none_mpm, nullptr, nullptr, nullptr) == PNN_OK);
        CHECK(none_mpm[0] == 0 && none_mpm[1] == 1 && none_mpm[2] == 26);
        const uint8_t bad = 35, worse = 36;
        CHECK(pnn_intra_mode_signal_host(&bad, nullptr, 1, 30, 0, none_mpm, nullptr, nullptr, nullptr) == PNN_E_ARG);
        CHECK(pnn_intra_mode_signal_host(nullptr, &worse, 1, 30, 1, none_mpm, nullptr, nullptr, nullptr) == PNN_E_ARG);
        CHECK(pnn_intra_mode_signal_host(nullptr, nullptr, 1, 52, 1, none_mpm, nullptr, nullptr, nullptr) == PNN_E_ARG);
        CHECK(pnn_intra_mode_signal_host(nullptr, nullptr, 1, 30, 1, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    }
    const int widths[5] = {4, 8, 16, 32, 64}, qps[2] = {22, 51}, nq = 2, n = 5;
    const double own[2] = {0.5, 200.};
    for (int w : widths) {
        const int k = pnn_first_pass_list_size(w), s = pnn_rd_pass_slot_count(w, 1);
        CHECK(s == k + 3 && pnn_rd_pass_slot_count(w, 0) == k + 1);
        const size_t w2 = (size_t)w * w;
        for (int side : {w + 1, 2 * w + 1}) {
            const size_t pat = (size_t)side * side;
            std::vector<uint8_t> patterns(n * pat), targets(n * w2), cand(n * w2), left(n), above(n);
            for (size_t i = 0; i < patterns.size(); i++) patterns[i] = (uint8_t)(i * 37 + 11 * w + (i / pat) * 50);
            for (size_t i = 0; i < targets.size(); i++) {
                targets[i] = (uint8_t)(i * 29 + 3 + (i % w) * 5);
                cand[i] = i / w2 == 1 ? targets[i] : i / w2 == 2 ? (uint8_t)(255 - targets[i]) : (uint8_t)(targets[i] ^ (i % 7));
            }
            for (int b = 0; b < n; b++) { left[b] = (uint8_t)(b == 0 ? 255 : b == 1 ? 35 : 7 * b); above[b] = (uint8_t)(b == 2 ? 35 : b == 3 ? 21 : 2); }
            std::vector<uint8_t> list((size_t)nq * n * k), slots((size_t)nq * n * s);
            std::vector<double> list_costs((size_t)nq * n * k);
            CHECK(pnn_first_pass_signal_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, nullptr, left.data(), above.data(),
                                             list.data(), list_costs.data(), slots.data()) == PNN_OK);
            for (size_t i = 0; i < (size_t)nq * n; i++) {
                CHECK(!memcmp(list.data() + i * k, slots.data() + i * s, k));
                for (int j = 1; j < k; j++) CHECK(list_costs[i * k + j - 1] <= list_costs[i * k + j]);
            }
            for (int rdoq = 0; rdoq <= (w <= 8 || (w == 64 && side == w + 1) ? 1 : 0); rdoq++) {   // (64: the quadrants' own path)
                std::vector<uint8_t> modes((size_t)nq * n * s), bm(nq * n), bs(nq * n), alone8(nq * n);
                std::vector<double> costs((size_t)nq * n * s), bc(nq * n), fp((size_t)nq * n * k);
                std::vector<uint32_t> sse(nq * n);
                std::vector<uint64_t> rate(nq * n), side_rate(nq * n), alone64(nq * n);
                CHECK(pnn_rd_pass_signal_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, left.data(),
                                              above.data(), modes.data(), costs.data(), bm.data(), bs.data(), bc.data(), sse.data(), rate.data(), fp.data(),
                                              side_rate.data()) == PNN_OK);
                for (size_t at = 0; at < (size_t)nq * n; at++) {
                    CHECK(bs[at] < s && bm[at] == modes[at * s + bs[at]] && bm[at] <= 35 && bc[at] == costs[at * s + bs[at]]);
                    for (int j = 0; j < s; j++) CHECK(bc[at] <= costs[at * s + j] && (std::isinf(costs[at * s + j]) == (modes[at * s + j] == 255)));
                    CHECK(side_rate[at] > 0);
                }
                CHECK(pnn_rd_pass_signal_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, left.data(),
                                              above.data(), nullptr, nullptr, alone8.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK &&
                      alone8 == bm);
                CHECK(pnn_rd_pass_signal_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, left.data(),
                                              above.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, alone64.data()) == PNN_OK &&
                      alone64 == side_rate);
                CHECK(pnn_rd_pass_signal_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), 2, qps, nq, own, rdoq, rdoq, 1, nullptr, nullptr,
                                              nullptr, nullptr, alone8.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
            }
        }
    }
    // refusals read nothing and write nothing
    uint8_t byte = 0, out = 7, bad = 36;
    const int good_qp = 22;
    const double zero = 0.;
    CHECK(pnn_rd_pass_signal_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, 0, 1, &bad, nullptr, &out, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_signal_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, &zero, 0, 1, 1, nullptr, nullptr, &out, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_signal_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_signal_host(nullptr, 9, 9, nullptr, 4, 0, nullptr, 0, &good_qp, 1, nullptr, 0, 0, 1, nullptr, nullptr, &out, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
    CHECK(pnn_rd_pass_slot_count(12, 1) == -1);
    CHECK(out == 7);
    printf("sanitize_mode_signal: ok\n");
    return 0;
}
