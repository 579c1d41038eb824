// Stand-alone driver for the AddressSanitizer + UBSan build of the host entries of the second intra pass (tests/test_rd_pass.py compiles
// it together with csrc/pnn_rd_pass.cpp, pnn_hevc_intra.cpp and pnn_trquant.cpp): pnn_rd_pass_host at every width with every pattern
// size the masks leave at both ends, without smoothing and hiding under HM's lambdas and with both under the caller's, 1 and 8 QPs,
// buffers of exactly the documented sizes, every output alone; pnn_hm_intra_lambda.  Any report aborts; a few known answers are checked on the way.
#include "pnn_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_rd_pass: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

int main()
{
    CHECK(pnn_hm_intra_lambda(12) == 0.57 && pnn_hm_intra_lambda(15) == 1.14 && pnn_hm_intra_lambda(0) == 0.57 / 16);
    const int widths[5] = {4, 8, 16, 32, 64}, all_qps[8] = {0, 5, 17, 22, 27, 37, 46, 51}, n = 5;
    const double own[8] = {0., 0.5, 1., 2., 4., 1e3, 1e30, 1e300};
    for (int w : widths) {
        const int k1 = pnn_first_pass_list_size(w) + 1;
        const size_t w2 = (size_t)w * w;
        for (int side : {w + 1, 2 * w + 1})
            for (int smoothing : {0, 2})
                for (int sdh = smoothing / 2; sdh <= smoothing / 2; sdh++)        // plain with HM's lambdas, smoothed + hidden with the caller's
                    for (int nq : {1, 8}) {
                        const size_t pat = (size_t)side * side;
                        std::vector<uint8_t> patterns(n * pat), targets(n * w2), cand(n * w2), modes(n * k1), alone8(nq * n), bm(nq * n), bs(nq * n);
                        std::vector<double> costs((size_t)nq * n * k1), bc(nq * n), aloned(nq * n);
                        std::vector<uint32_t> sse(nq * n), alone32(nq * n);
                        std::vector<uint64_t> rate(nq * n), alone64(nq * n);
                        for (size_t i = 0; i < patterns.size(); i++) patterns[i] = (uint8_t)(i * 37 + 11 * w + (i / pat) * 50);
                        for (size_t i = 0; i < targets.size(); i++) {
                            targets[i] = (uint8_t)(i * 29 + 3 + (i % w) * 5);
                            cand[i] = i / w2 == 1 ? targets[i] : i / w2 == 2 ? (uint8_t)(255 - targets[i]) : (uint8_t)(targets[i] ^ (i % 7));
                        }
                        const double* lambdas = sdh ? own : nullptr;
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               modes.data(), costs.data(), bm.data(), bs.data(), bc.data(), sse.data(), rate.data()) == PNN_OK);
                        for (int q = 0; q < nq; q++)
                            for (int b = 0; b < n; b++) {
                                const size_t at = (size_t)q * n + b;
                                CHECK(bs[at] <= k1 - 1 && bm[at] == modes[b * k1 + bs[at]] && bm[at] <= 35);
                                CHECK(bc[at] == costs[at * k1 + bs[at]]);
                                for (int s = 0; s < k1; s++) CHECK(bc[at] <= costs[at * k1 + s] && (s >= bs[at] || bc[at] < costs[at * k1 + s]));
                                CHECK((modes[b * k1 + k1 - 1] == 255) == std::isinf(costs[at * k1 + k1 - 1]));
                                if (b == 1) CHECK(bc[at] == 0. && sse[at] == 0);                                 // the candidate is the target
                            }
                        if (nq > 1) continue;                                                     // every output alone: at one QP
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               nullptr, nullptr, alone8.data(), nullptr, nullptr, nullptr, nullptr) == PNN_OK && alone8 == bm);
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               nullptr, nullptr, nullptr, alone8.data(), nullptr, nullptr, nullptr) == PNN_OK && alone8 == bs);
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               nullptr, nullptr, nullptr, nullptr, aloned.data(), nullptr, nullptr) == PNN_OK &&
                              !memcmp(aloned.data(), bc.data(), aloned.size() * 8));
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, alone32.data(), nullptr) == PNN_OK && alone32 == sse);
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, alone64.data()) == PNN_OK && alone64 == rate);
                        std::vector<uint8_t> modes_alone(n * k1);
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               modes_alone.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK && modes_alone == modes);
                        std::vector<double> costs_alone(costs.size());
                        CHECK(pnn_rd_pass_host(patterns.data(), side, side, targets.data(), w, n, cand.data(), smoothing, all_qps, nq, lambdas, sdh,
                                               nullptr, costs_alone.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK &&
                              !memcmp(costs_alone.data(), costs.data(), costs.size() * 8));
                    }
    }
    // more blocks than the twin codes per call of the transform entry
    {
        const int w = 4, big = 1030, k1 = 9, qp = 30;
        std::vector<uint8_t> patterns((size_t)big * 81), targets((size_t)big * 16), cand((size_t)big * 16), modes((size_t)big * k1), first(k1);
        for (size_t i = 0; i < patterns.size(); i++) patterns[i] = (uint8_t)(i * 13 + (i / 81) * 7);
        for (size_t i = 0; i < targets.size(); i++) { targets[i] = (uint8_t)(i * 31 + 9); cand[i] = (uint8_t)(targets[i] + (i % 5)); }
        CHECK(pnn_rd_pass_host(patterns.data(), 9, 9, targets.data(), w, big, cand.data(), 0, &qp, 1, nullptr, 1, modes.data(), nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr) == PNN_OK);
        CHECK(pnn_rd_pass_host(patterns.data() + 1029 * 81, 9, 9, targets.data() + 1029 * 16, w, 1, cand.data() + 1029 * 16, 0, &qp, 1, nullptr, 1,
                               first.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
        CHECK(!memcmp(first.data(), modes.data() + 1029 * k1, k1));
    }
    // refusals read nothing and write nothing
    uint8_t byte = 0, out = 7;
    const int good_qp = 22, bad_qp = 52;
    const double minus = -1., nan = std::nan(""), inf = HUGE_VAL;
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 12, 1, &byte, 0, &good_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 4, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, nullptr, 0, &good_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(nullptr, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, &byte, 3, &good_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &bad_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 9, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, &minus, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, &nan, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, &inf, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, 1, &byte, 0, &good_qp, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(&byte, 9, 9, &byte, 4, -1, &byte, 0, &good_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_rd_pass_host(nullptr, 9, 9, nullptr, 4, 0, nullptr, 0, &good_qp, 1, nullptr, 0, &out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
    CHECK(out == 7);
    printf("sanitize_rd_pass: ok\n");
    return 0;
}
