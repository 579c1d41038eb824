// Stand-alone driver for the AddressSanitizer + UBSan build of the host entries of the sign-data hiding (tests/test_sign_hiding.py
// compiles it together with csrc/pnn_trquant.cpp): pnn_sign_hide_unit_host at every unit size and scan on empty, dense, extreme
// (32767 / -32768, remainders at both ends of int32) and all-forbidden units in buffers of exactly the documented sizes;
// pnn_trquant_stages_sdh_host, pnn_cabac_rate_levels_sdh_host and pnn_trquant_sdh_host at every width with and without modes and rate,
// every output alone.  Any report aborts; a few known answers are checked on the way.
#include "pnn_hip.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sanitize_sign_hiding: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

int main()
{
    const int sizes[4] = {4, 8, 16, 32};
    for (int t : sizes)
        for (int scan = 0; scan < (t <= 8 ? 3 : 1); scan++) {
            const size_t tt = (size_t)t * t;
            std::vector<int32_t> levels(tt, 0), coeffs(tt, 0), delta_u(tt, 0), before;
            CHECK(pnn_sign_hide_unit_host(levels.data(), coeffs.data(), delta_u.data(), t, scan) == PNN_OK);
            for (int32_t v : levels) CHECK(v == 0);
            for (size_t i = 0; i < tt; i++) {
                levels[i] = (int32_t)((i * 37 + 11) % 9) - 4;
                coeffs[i] = levels[i] * 50 + (levels[i] ? 0 : (i % 2 ? 7 : -7));
                delta_u[i] = (int32_t)((i * 53) % 257) - 86;
            }
            before = levels;
            CHECK(pnn_sign_hide_unit_host(levels.data(), coeffs.data(), delta_u.data(), t, scan) == PNN_OK);
            size_t changed = 0;
            for (size_t i = 0; i < tt; i++) {
                CHECK(abs(levels[i] - before[i]) <= 1);
                changed += levels[i] != before[i];
            }
            CHECK(changed <= tt / 16);                                                        // one per group at the most
            for (size_t i = 0; i < tt; i++) {
                levels[i] = i % 3 == 0 ? -32768 : i % 3 == 1 ? 32767 : 0;
                coeffs[i] = i % 3 == 0 ? INT32_MIN : i % 3 == 1 ? INT32_MAX : (i % 2 ? 1 : -1);
                delta_u[i] = i % 5 == 0 ? INT32_MAX : i % 5 == 1 ? -INT32_MAX : (int32_t)(i % 7) - 3;
            }
            CHECK(pnn_sign_hide_unit_host(levels.data(), coeffs.data(), delta_u.data(), t, scan) == PNN_OK);
            for (int32_t v : levels) CHECK(v >= -32768 && v <= 32767);
            for (size_t i = 0; i < tt; i++) { levels[i] = i % 2 ? 1 : -1; coeffs[i] = levels[i]; delta_u[i] = 0; }    // every first level forbidden
            CHECK(pnn_sign_hide_unit_host(levels.data(), coeffs.data(), delta_u.data(), t, scan) == PNN_OK);
            uint64_t plain = 0, hidden = 0;
            CHECK(pnn_cabac_rate_levels_sdh_host(before.data(), t, scan, 22, 0, &plain) == PNN_OK);
            CHECK(pnn_cabac_rate_levels_sdh_host(before.data(), t, scan, 22, 1, &hidden) == PNN_OK);
            CHECK(plain - hidden == 32768 * (uint64_t)(tt / 16));                             // the dense unit: every group hides a sign
        }
    const int widths[5] = {4, 8, 16, 32, 64}, all_qps[8] = {0, 5, 17, 22, 27, 37, 46, 51}, n = 5;
    const uint8_t modes[5] = {0, 26, 10, 34, 6};
    for (int w : widths) {
        const size_t w2 = (size_t)w * w;
        std::vector<uint8_t> pred(n * w2), tgt(n * w2), recon(8 * n * w2), recon_alone(8 * n * w2);
        std::vector<uint32_t> sse(8 * n), nonzero(8 * n), sum_abs(8 * n), alone32(8 * n), off(8 * n), plain(8 * n);
        std::vector<uint64_t> rate(8 * n), alone(8 * n);
        for (size_t i = 0; i < w2; i++) {
            const int y = (int)(i / w), x = (int)(i % w);
            pred[i] = 0; tgt[i] = 255;
            pred[w2 + i] = 255; tgt[w2 + i] = 0;
            pred[2 * w2 + i] = (x + y) % 2 ? 0 : 255; tgt[2 * w2 + i] = (uint8_t)(255 - pred[2 * w2 + i]);
            pred[3 * w2 + i] = tgt[3 * w2 + i] = (uint8_t)(i * 29 + 3);                       // zero residual
            pred[4 * w2 + i] = (uint8_t)(i * 73 + 5 * w); tgt[4 * w2 + i] = (uint8_t)(i * i * 31 + 7);
        }
        for (const uint8_t* m : {(const uint8_t*)nullptr, modes}) {
            CHECK(pnn_trquant_sdh_host(pred.data(), tgt.data(), w, n, m, all_qps, 8, sse.data(), nonzero.data(), sum_abs.data(), recon.data(),
                                       rate.data(), 1) == PNN_OK);
            CHECK(pnn_trquant_sdh_host(pred.data(), tgt.data(), w, n, m, all_qps, 8, nullptr, nullptr, nullptr, nullptr, alone.data(), 1) == PNN_OK);
            CHECK(alone == rate);
            CHECK(pnn_trquant_sdh_host(pred.data(), tgt.data(), w, n, m, all_qps, 8, alone32.data(), nullptr, nullptr, nullptr, nullptr, 1) == PNN_OK);
            CHECK(alone32 == sse);
            CHECK(pnn_trquant_sdh_host(pred.data(), tgt.data(), w, n, m, all_qps, 8, nullptr, alone32.data(), nullptr, nullptr, nullptr, 1) == PNN_OK);
            CHECK(alone32 == nonzero);
            CHECK(pnn_trquant_sdh_host(pred.data(), tgt.data(), w, n, m, all_qps, 8, nullptr, nullptr, alone32.data(), nullptr, nullptr, 1) == PNN_OK);
            CHECK(alone32 == sum_abs);
            CHECK(pnn_trquant_sdh_host(pred.data(), tgt.data(), w, n, m, all_qps, 8, nullptr, nullptr, nullptr, recon_alone.data(), nullptr, 1) == PNN_OK);
            CHECK(recon_alone == recon);
            for (int q = 0; q < 8; q++) CHECK(rate[q * n + 3] == 0 && sse[q * n + 3] == 0);
        }
        // the flag 0 is the entry without it; sum_abs_levels is the same under either flag
        CHECK(pnn_trquant_sdh_host(pred.data(), tgt.data(), w, n, nullptr, all_qps, 8, off.data(), nullptr, alone32.data(), nullptr, nullptr, 0) == PNN_OK);
        CHECK(pnn_trquant_host(pred.data(), tgt.data(), w, n, all_qps, 8, plain.data(), nullptr, nullptr, nullptr) == PNN_OK && plain == off);
        CHECK(alone32 == sum_abs);
        CHECK(pnn_trquant_sdh_host(nullptr, nullptr, w, 0, nullptr, all_qps, 8, nullptr, nullptr, nullptr, nullptr, rate.data(), 1) == PNN_OK);
        std::vector<int32_t> stage[6];
        for (auto& s : stage) s.assign(w2, 0);
        for (int scan = 0; scan < (w <= 8 ? 3 : 1); scan++) {
            CHECK(pnn_trquant_stages_sdh_host(pred.data() + 4 * w2, tgt.data() + 4 * w2, w, 5, scan, 1, stage[0].data(), stage[1].data(),
                                              stage[2].data(), stage[3].data(), stage[4].data(), stage[5].data()) == PNN_OK);
            for (size_t i = 0; i < w2; i++) CHECK(abs(stage[1][i] - stage[3][i]) <= 1 && stage[2][i] >= -86 && stage[2][i] <= 170);
            CHECK(pnn_trquant_stages_sdh_host(pred.data(), tgt.data(), w, 5, scan, 1, nullptr, nullptr, stage[2].data(), nullptr, nullptr, nullptr) == PNN_OK);
        }
    }
    // refusals read nothing and write nothing
    uint8_t byte = 0, bad_mode = 35;
    uint32_t word = 0;
    uint64_t bits = 0;
    int32_t level = 1, big = 32768, worst = INT32_MIN;
    const int good_qp = 22, bad_qp = 52;
    CHECK(pnn_trquant_sdh_host(&byte, &byte, 8, 1, &bad_mode, &good_qp, 1, &word, nullptr, nullptr, nullptr, nullptr, 1) == PNN_E_ARG);
    CHECK(pnn_trquant_sdh_host(&byte, &byte, 8, 1, &byte, &good_qp, 1, &word, nullptr, nullptr, nullptr, nullptr, 0) == PNN_E_ARG);
    CHECK(pnn_trquant_sdh_host(&byte, &byte, 8, 1, nullptr, &good_qp, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == PNN_E_ARG);
    CHECK(pnn_trquant_sdh_host(&byte, &byte, 8, 1, nullptr, &bad_qp, 1, &word, nullptr, nullptr, nullptr, nullptr, 1) == PNN_E_ARG);
    CHECK(pnn_trquant_sdh_host(&byte, &byte, 12, 1, nullptr, &good_qp, 1, &word, nullptr, nullptr, nullptr, nullptr, 1) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(&level, &level, &level, 12, 0) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(&level, &level, &level, 64, 0) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(&level, &level, &level, 16, 1) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(&level, &level, &level, 4, 3) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(nullptr, &level, &level, 4, 0) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(&level, nullptr, &level, 4, 0) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(&level, &level, nullptr, 4, 0) == PNN_E_ARG);
    CHECK(pnn_sign_hide_unit_host(&big, &level, &level, 4, 0) == PNN_E_ARG);                  // (the first element decides: nothing else is read)
    CHECK(pnn_sign_hide_unit_host(&level, &level, &worst, 4, 0) == PNN_E_ARG);
    CHECK(pnn_trquant_stages_sdh_host(&byte, &byte, 8, 22, 3, 1, &level, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_stages_sdh_host(&byte, &byte, 16, 22, 1, 1, &level, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_stages_sdh_host(&byte, &byte, 8, 22, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_sdh_host(&level, 16, 1, 22, 1, &bits) == PNN_E_ARG);
    CHECK(pnn_cabac_rate_levels_sdh_host(&level, 4, 0, 22, 1, nullptr) == PNN_E_ARG);
    CHECK(word == 0 && bits == 0 && level == 1);
    printf("sanitize_sign_hiding: ok\n");
    return 0;
}
