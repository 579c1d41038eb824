// Stand-alone driver for the AddressSanitizer + UBSan build of the host twin of the open-loop transform coding (tests/test_trquant.py
// compiles it together with csrc/pnn_trquant.cpp): pnn_trquant_host and pnn_trquant_stages_host at every width and at the QPs whose
// shifts are the extreme ones, on the residuals of largest magnitude (+-255 flat, the checkerboard), on a zero residual and on
// pseudo-random blocks, in buffers of exactly the documented sizes, with every output alone and all together.  Any report aborts; a few
// known answers are checked on the way.
#include "pnn_hip.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_trquant: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

int main()
{
    const int widths[5] = {4, 8, 16, 32, 64}, qps[8] = {0, 5, 17, 22, 27, 37, 46, 51}, n = 5;
    for (int w : widths) {
        const size_t w2 = (size_t)w * w;
        std::vector<uint8_t> pred(n * w2), tgt(n * w2), recon(8 * n * w2);
        std::vector<uint32_t> sse(8 * n), nonzero(8 * n), sum_abs(8 * n);
        for (size_t i = 0; i < w2; i++) {
            const int y = (int)(i / w), x = (int)(i % w);
            pred[i] = 0; tgt[i] = 255;                                                        // + 255 everywhere
            pred[w2 + i] = 255; tgt[w2 + i] = 0;                                              // - 255 everywhere
            pred[2 * w2 + i] = (x + y) % 2 ? 0 : 255; tgt[2 * w2 + i] = (uint8_t)(255 - pred[2 * w2 + i]);   // the checkerboard
            pred[3 * w2 + i] = tgt[3 * w2 + i] = (uint8_t)(i * 29 + 3);                       // zero residual
            pred[4 * w2 + i] = (uint8_t)(i * 73 + 5 * w); tgt[4 * w2 + i] = (uint8_t)(i * i * 31 + 7);
        }
        CHECK(pnn_trquant_host(pred.data(), tgt.data(), w, n, qps, 8, sse.data(), nonzero.data(), sum_abs.data(), recon.data()) == PNN_OK);
        for (int q = 0; q < 8; q++) {
            CHECK(sse[q * n + 3] == 0 && nonzero[q * n + 3] == 0 && sum_abs[q * n + 3] == 0);
            for (size_t i = 0; i < w2; i++) CHECK(recon[(q * n + 3) * w2 + i] == pred[3 * w2 + i]);
        }
        // each output alone gives the same numbers; a single QP, a single block
        std::vector<uint32_t> alone(8 * n);
        CHECK(pnn_trquant_host(pred.data(), tgt.data(), w, n, qps, 8, alone.data(), nullptr, nullptr, nullptr) == PNN_OK && alone == sse);
        CHECK(pnn_trquant_host(pred.data(), tgt.data(), w, n, qps, 8, nullptr, alone.data(), nullptr, nullptr) == PNN_OK && alone == nonzero);
        CHECK(pnn_trquant_host(pred.data(), tgt.data(), w, n, qps, 8, nullptr, nullptr, alone.data(), nullptr) == PNN_OK && alone == sum_abs);
        std::vector<uint8_t> one(w2);
        CHECK(pnn_trquant_host(pred.data() + 4 * w2, tgt.data() + 4 * w2, w, 1, qps + 3, 1, nullptr, nullptr, nullptr, one.data()) == PNN_OK);
        for (size_t i = 0; i < w2; i++) CHECK(one[i] == recon[(3 * n + 4) * w2 + i]);
        CHECK(pnn_trquant_host(nullptr, nullptr, w, 0, qps, 8, sse.data(), nullptr, nullptr, nullptr) == PNN_OK);
        // the stages of every block at every QP: the sums of the levels are the counts above
        std::vector<int32_t> coeffs(w2), levels(w2), dequant(w2), residual(w2);
        for (int b = 0; b < n; b++)
            for (int q = 0; q < 8; q++) {
                CHECK(pnn_trquant_stages_host(pred.data() + b * w2, tgt.data() + b * w2, w, qps[q], coeffs.data(), levels.data(), dequant.data(),
                                              residual.data()) == PNN_OK);
                uint32_t count = 0, total = 0;
                for (size_t i = 0; i < w2; i++) {
                    count += levels[i] != 0; total += (uint32_t)abs(levels[i]);
                    const int v = pred[b * w2 + i] + residual[i];
                    CHECK(recon[(q * n + b) * w2 + i] == (v < 0 ? 0 : v > 255 ? 255 : v));
                }
                CHECK(count == nonzero[q * n + b] && total == sum_abs[q * n + b]);          // (no level reaches the clip here)
                CHECK(pnn_trquant_stages_host(pred.data() + b * w2, tgt.data() + b * w2, w, qps[q], nullptr, nullptr, nullptr, residual.data()) == PNN_OK);
            }
    }
    // refusals read nothing and write nothing
    uint8_t byte = 0;
    uint32_t word = 0;
    int32_t stage = 0;
    const int bad_qp = 52, good_qp = 22;
    CHECK(pnn_trquant_host(&byte, &byte, 12, 1, &good_qp, 1, &word, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_host(&byte, &byte, 8, 1, &bad_qp, 1, &word, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_host(&byte, &byte, 8, 1, &good_qp, 0, &word, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_host(&byte, &byte, 8, 1, &good_qp, 9, &word, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_host(&byte, &byte, 8, 1, nullptr, 1, &word, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_host(&byte, &byte, 8, -1, &good_qp, 1, &word, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_host(nullptr, &byte, 8, 1, &good_qp, 1, &word, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_host(&byte, &byte, 8, 1, &good_qp, 1, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_stages_host(&byte, &byte, 8, -1, &stage, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_stages_host(&byte, nullptr, 8, 22, &stage, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_stages_host(&byte, &byte, 8, 22, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(word == 0 && stage == 0);
    printf("sanitize_trquant: ok\n");
    return 0;
}
