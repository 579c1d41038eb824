// AddressSanitizer + UBSan driver of the RDOQ host entries (no GPU, no Python: build it with -fsanitize=address,undefined together with
// csrc/pnn_trquant.cpp, pnn_rd_pass.cpp and pnn_hevc_intra.cpp): pnn_rdoq_unit_host, pnn_rdoq_est_bits_host, pnn_trquant_rdoq_host,
// pnn_trquant_stages_rdoq_host and pnn_rd_pass_rdoq_host at every width, all scans, QPs 0 and 51 among others, tiny and huge lambdas,
// sign hiding off and on, buffers of exactly the documented sizes.  Any report aborts; a few known answers are checked on the way.
#include "../include/pnn_hip.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "sanitize_rdoq: %s failed at line %d\n", #x, __LINE__); abort(); } } while (0)

int main()
{
    std::mt19937 rng(5);
    const int qps[4] = {0, 22, 37, 51};
    const double factors[4] = {1e-12, 0.25, 1., 1e12};
    for (int t : {4, 8, 16, 32}) {
        std::vector<int32_t> coeffs(t * t), levels(t * t), est(184);
        for (int qp : qps) {
            CHECK(pnn_rdoq_est_bits_host(t, qp, est.data()) == PNN_OK);
            for (int scan = 0; scan < (t <= 8 ? 3 : 1); scan++)
                for (double f : factors)
                    for (int sdh = 0; sdh < 2; sdh++)
                        for (int extreme = 0; extreme < 2; extreme++) {
                            for (auto& c : coeffs) c = extreme ? (rng() & 1 ? 32767 : -32768) : (int)(rng() % 4001) - 2000;
                            int32_t sum = -1;
                            CHECK(pnn_rdoq_unit_host(coeffs.data(), t, scan, qp, pnn_hm_intra_lambda(qp) * f, (int)(rng() & 1), sdh, levels.data(),
                                                     &sum) == PNN_OK);
                            CHECK(sum >= 0);
                            if (f == 1e12) CHECK(sum == 0);                     // a huge lambda codes nothing
                        }
        }
    }
    for (int w : {4, 8, 16, 32, 64}) {
        const int n = 5, w2 = w * w, side = 2 * w + 1;
        std::vector<uint8_t> pred(n * w2), tgt(n * w2), modes(n), patterns(n * side * side), recon(4 * n * w2);
        for (auto& v : pred) v = (uint8_t)rng();
        for (auto& v : tgt) v = (uint8_t)rng();
        for (auto& v : patterns) v = (uint8_t)rng();
        for (int b = 0; b < n; b++) modes[b] = (uint8_t)(b * 8 % 35);
        std::vector<uint32_t> sse(4 * n), nonzero(4 * n), sum_abs(4 * n);
        std::vector<uint64_t> rate(4 * n);
        const double lambdas[4] = {1e-9, 3., 40., 1e9};
        for (int sdh = 0; sdh < 2; sdh++)
            for (const double* lam : {(const double*)nullptr, lambdas}) {
                CHECK(pnn_trquant_rdoq_host(pred.data(), tgt.data(), w, n, modes.data(), qps, 4, sse.data(), nonzero.data(), sum_abs.data(),
                                            recon.data(), rate.data(), sdh, 1, lam) == PNN_OK);
                CHECK(pnn_trquant_rdoq_host(pred.data(), tgt.data(), w, n, nullptr, qps, 4, nullptr, nullptr, sum_abs.data(), nullptr, nullptr, sdh, 1,
                                            lam) == PNN_OK);
            }
        std::vector<int32_t> stage(6 * w2);
        for (int ctx = 0; ctx < 2; ctx++)
            CHECK(pnn_trquant_stages_rdoq_host(pred.data(), tgt.data(), w, 30, 0, 1, 1, 2.5, ctx, stage.data(), stage.data() + w2, stage.data() + 2 * w2,
                                               stage.data() + 3 * w2, stage.data() + 4 * w2, stage.data() + 5 * w2) == PNN_OK);
        const int k1 = pnn_first_pass_list_size(w) + 1;
        std::vector<uint8_t> cand_modes(n * k1), best(4 * n);
        std::vector<double> costs(4 * n * k1);
        CHECK(pnn_rd_pass_rdoq_host(patterns.data(), side, side, tgt.data(), w, n, pred.data(), 2, qps, 4, nullptr, 1, 1, cand_modes.data(), costs.data(),
                                    best.data(), nullptr, nullptr, nullptr, nullptr) == PNN_OK);
        const double zero = 0.;
        CHECK(pnn_rd_pass_rdoq_host(patterns.data(), side, side, tgt.data(), w, n, pred.data(), 2, qps, 1, &zero, 1, 1, cand_modes.data(), nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
        CHECK(pnn_trquant_rdoq_host(pred.data(), tgt.data(), w, n, nullptr, qps, 1, sse.data(), nullptr, nullptr, nullptr, nullptr, 0, 1, &zero) ==
              PNN_E_ARG);
    }
    printf("sanitize_rdoq: ok\n");
    return 0;
}
