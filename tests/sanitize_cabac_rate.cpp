// Stand-alone driver for the AddressSanitizer + UBSan build of the host entries of the CABAC rate (tests/test_cabac_rate.py compiles it
// together with csrc/pnn_trquant.cpp): pnn_cabac_rate_levels_host at every unit size, scan and extreme QP on empty, lone, dense and
// extreme levels (-32768: the longest escape code, whose negation must not overflow) in buffers of exactly the documented sizes, and
// pnn_trquant_rate_host at every width with and without modes, the rate alone and with every other output.  Any report aborts; a few
// known answers are checked on the way.
#include "pnn_hip.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_cabac_rate: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

int main()
{
    const int sizes[4] = {4, 8, 16, 32}, qps[4] = {0, 22, 37, 51};
    for (int t : sizes)
        for (int scan = 0; scan < (t <= 8 ? 3 : 1); scan++)
            for (int qp : qps) {
                std::vector<int32_t> levels((size_t)t * t, 0);
                uint64_t zero = 1, lone = 0, corner = 0, dense = 0, extreme = 0;
                CHECK(pnn_cabac_rate_levels_host(levels.data(), t, scan, qp, &zero) == PNN_OK && zero == 0);
                levels[0] = -1;
                CHECK(pnn_cabac_rate_levels_host(levels.data(), t, scan, qp, &lone) == PNN_OK && lone > 32768);
                levels[0] = 0; levels[(size_t)t * t - 1] = 1;
                CHECK(pnn_cabac_rate_levels_host(levels.data(), t, scan, qp, &corner) == PNN_OK && corner > lone);
                for (size_t i = 0; i < levels.size(); i++) levels[i] = (int32_t)((i * 37 + 11) % 9) - 4;
                CHECK(pnn_cabac_rate_levels_host(levels.data(), t, scan, qp, &dense) == PNN_OK && dense > corner);
                for (size_t i = 0; i < levels.size(); i++) levels[i] = i % 3 == 0 ? -32768 : i % 3 == 1 ? 32767 : 0;
                CHECK(pnn_cabac_rate_levels_host(levels.data(), t, scan, qp, &extreme) == PNN_OK && extreme > dense);
                CHECK(extreme < ((uint64_t)1 << 32));
            }
    const int widths[5] = {4, 8, 16, 32, 64}, all_qps[8] = {0, 5, 17, 22, 27, 37, 46, 51}, n = 5;
    const uint8_t modes[5] = {0, 26, 10, 34, 6};
    for (int w : widths) {
        const size_t w2 = (size_t)w * w;
        std::vector<uint8_t> pred(n * w2), tgt(n * w2), recon(8 * n * w2);
        std::vector<uint32_t> sse(8 * n), nonzero(8 * n), sum_abs(8 * n), plain(8 * n);
        std::vector<uint64_t> rate(8 * n), alone(8 * n), diagonal(8 * n);
        for (size_t i = 0; i < w2; i++) {
            const int y = (int)(i / w), x = (int)(i % w);
            pred[i] = 0; tgt[i] = 255;
            pred[w2 + i] = 255; tgt[w2 + i] = 0;
            pred[2 * w2 + i] = (x + y) % 2 ? 0 : 255; tgt[2 * w2 + i] = (uint8_t)(255 - pred[2 * w2 + i]);
            pred[3 * w2 + i] = tgt[3 * w2 + i] = (uint8_t)(i * 29 + 3);                       // zero residual
            pred[4 * w2 + i] = (uint8_t)(i * 73 + 5 * w); tgt[4 * w2 + i] = (uint8_t)(i * i * 31 + 7);
        }
        CHECK(pnn_trquant_rate_host(pred.data(), tgt.data(), w, n, modes, all_qps, 8, sse.data(), nonzero.data(), sum_abs.data(), recon.data(),
                                    rate.data()) == PNN_OK);
        CHECK(pnn_trquant_rate_host(pred.data(), tgt.data(), w, n, modes, all_qps, 8, nullptr, nullptr, nullptr, nullptr, alone.data()) == PNN_OK);
        CHECK(alone == rate);
        CHECK(pnn_trquant_rate_host(pred.data(), tgt.data(), w, n, nullptr, all_qps, 8, nullptr, nullptr, nullptr, nullptr, diagonal.data()) == PNN_OK);
        CHECK(pnn_trquant_host(pred.data(), tgt.data(), w, n, all_qps, 8, plain.data(), nullptr, nullptr, nullptr) == PNN_OK && plain == sse);
        for (int q = 0; q < 8; q++) {
            CHECK(rate[q * n + 3] == 0 && diagonal[q * n + 3] == 0);                          // nothing to code
            CHECK(rate[q * n] == diagonal[q * n]);                                            // mode 0 scans diagonally
            CHECK((rate[q * n + 4] != 0) == (nonzero[q * n + 4] != 0));
            if (w > 8) CHECK(rate[q * n + 1] == diagonal[q * n + 1] && rate[q * n + 2] == diagonal[q * n + 2]);
        }
        CHECK(pnn_trquant_rate_host(nullptr, nullptr, w, 0, nullptr, all_qps, 8, nullptr, nullptr, nullptr, nullptr, rate.data()) == PNN_OK);
    }
    // refusals read nothing and write nothing
    uint8_t byte = 0, bad_mode = 35;
    uint32_t word = 0;
    uint64_t bits = 0;
    int32_t level = 1, big = 32768;
    const int good_qp = 22, bad_qp = 52;
    CHECK(pnn_trquant_rate_host(&byte, &byte, 8, 1, &bad_mode, &good_qp, 1, nullptr, nullptr, nullptr, nullptr, &bits) == PNN_E_ARG);
    CHECK(pnn_trquant_rate_host(&byte, &byte, 8, 1, &byte, &good_qp, 1, &word, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_rate_host(&byte, &byte, 8, 1, nullptr, &good_qp, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_rate_host(&byte, &byte, 8, 1, nullptr, &bad_qp, 1, nullptr, nullptr, nullptr, nullptr, &bits) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_host(&level, 12, 0, 22, &bits) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_host(&level, 16, 1, 22, &bits) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_host(&level, 4, 3, 22, &bits) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_host(&level, 4, 0, 52, &bits) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_host(nullptr, 4, 0, 22, &bits) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_host(&level, 4, 0, 22, nullptr) == PNN_E_ARG);
    CHECK(word == 0 && bits == 0);
    (void)big;
    printf("sanitize_cabac_rate: ok\n");
    return 0;
}
