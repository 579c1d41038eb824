// Stand-alone AddressSanitizer + UBSan program over the host twin of transform skip (tests/test_transform_skip_sanitizer.py compiles it
// together with csrc/pnn_tskip.cpp and csrc/pnn_trquant.cpp): pnn_tskip_unit_host on zero, extreme and seeded residuals at every scan, the
// ends of the QP range, both forms, RDOQ and the hiding off and on, every output alone; pnn_trquant_tskip_host at n = 0, 1 and 67 in
// buffers of exactly the documented sizes, the three option values, every output alone; the refusals.  Any report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pnn_hip.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "sanitize_transform_skip: %s failed at line %d\n", #x, __LINE__); abort(); } } while (0)

int main()
{
    std::mt19937 rng(4405);
    const int qps[4] = {0, 22, 37, 51};
    for (int kind = 0; kind < 5; kind++)
        for (int scan = 0; scan < 3; scan++)
            for (int qp : qps)
                for (int options = 0; options < 8; options++) {
                    std::vector<int32_t> residual(16), coeffs(16), levels(16), back(16);
                    for (int i = 0; i < 16; i++)
                        residual[i] = kind == 0 ? 0 : kind == 1 ? 255 : kind == 2 ? -255 : kind == 3 ? ((i & 1) ? 255 : -255) : (int)(rng() % 511) - 255;
                    const int sdh = options & 1, rdoq = (options >> 1) & 1, form = options >> 2;
                    int32_t abs_sum = -1;
                    uint64_t bits = 0, bins[2] = {0, 0};
                    CHECK(pnn_tskip_unit_host(residual.data(), scan, qp, sdh, rdoq, pnn_hm_intra_lambda(qp), form, coeffs.data(), levels.data(), &abs_sum,
                                              back.data(), &bits, bins) == PNN_OK);
                    CHECK(abs_sum >= 0 && bins[0] > 0 && bins[1] > 0);
                    if (form)
                        for (int i = 0; i < 16; i++) CHECK(coeffs[i] == residual[i] * 32);
                    if (kind == 0) CHECK(bits == 0 && abs_sum == 0);
                    CHECK(pnn_tskip_unit_host(residual.data(), scan, qp, sdh, rdoq, 1., form, nullptr, nullptr, nullptr, nullptr, &bits, nullptr) == PNN_OK);
                    CHECK(pnn_tskip_unit_host(residual.data(), scan, qp, sdh, rdoq, 1., form, nullptr, levels.data(), nullptr, nullptr, nullptr, nullptr) == PNN_OK);
                }
    for (int n : {0, 1, 67}) {
        std::vector<uint8_t> pred((size_t)n * 16), tgt((size_t)n * 16), modes(n);
        for (auto& v : pred) v = (uint8_t)rng();
        for (auto& v : tgt) v = (uint8_t)rng();
        for (auto& v : modes) v = (uint8_t)(rng() % 35);
        const size_t qn = (size_t)4 * n;
        std::vector<uint32_t> mode_bits(qn);
        for (auto& v : mode_bits) v = (uint32_t)(rng() % (8u << 15));
        for (int option = 0; option < 3; option++)
            for (int options = 0; options < 4; options++) {
                const int sdh = options & 1, rdoq = options >> 1;
                const size_t one = qn ? 0 : 1;                              // (an empty vector's data() is NULL: "every output is NULL")
                std::vector<uint32_t> sse(qn + one), nonzero(qn + one), sum_abs(qn + one);
                std::vector<uint64_t> rate(qn + one);
                std::vector<uint8_t> recon(qn * 16 + one), flags(qn + one);
                CHECK(pnn_trquant_tskip_host(pred.data(), tgt.data(), 4, n, modes.data(), qps, 4, sse.data(), nonzero.data(), sum_abs.data(), recon.data(),
                                             rate.data(), sdh, rdoq, nullptr, option, option == 2 ? mode_bits.data() : nullptr, options & 1, flags.data()) == PNN_OK);
                for (size_t i = 0; i < qn; i++) CHECK(flags[i] <= 1 && (option != 0 || flags[i] == 0) && (option != 1 || flags[i] == 1));
                CHECK(pnn_trquant_tskip_host(pred.data(), tgt.data(), 4, n, nullptr, qps, 4, nullptr, nullptr, nullptr, nullptr, rate.data(), sdh, rdoq,
                                             nullptr, option, nullptr, 1, nullptr) == PNN_OK);
                if (option)
                    CHECK(pnn_trquant_tskip_host(pred.data(), tgt.data(), 4, n, nullptr, qps, 4, nullptr, nullptr, nullptr, nullptr, nullptr, sdh, rdoq,
                                                 nullptr, option, nullptr, 0, flags.data()) == PNN_OK);
                CHECK(pnn_trquant_tskip_host(pred.data(), tgt.data(), 4, n, modes.data(), qps, 4, nullptr, nullptr, nullptr, recon.data(), nullptr, sdh,
                                             1, nullptr, option, nullptr, 1, nullptr) == PNN_OK);
            }
    }
    // the refusals: nothing is written
    int32_t r[16] = {};
    uint8_t block[64] = {};
    uint32_t out[4] = {};
    const int qp = 22, bad_qp = 52;
    const double zero = 0.;
    CHECK(pnn_tskip_unit_host(nullptr, 0, 22, 0, 0, 1., 1, r, r, nullptr, r, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_tskip_unit_host(r, 3, 22, 0, 0, 1., 1, r, r, nullptr, r, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_tskip_unit_host(r, 0, 52, 0, 0, 1., 1, r, r, nullptr, r, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_tskip_unit_host(r, 0, 22, 0, 1, 0., 1, r, r, nullptr, r, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_tskip_unit_host(r, 0, 22, 0, 0, 1., 2, r, r, nullptr, r, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_tskip_host(block, block, 8, 1, nullptr, &qp, 1, out, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 1, nullptr, 1, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_tskip_host(block, block, 4, 1, nullptr, &qp, 1, out, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 3, nullptr, 1, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_tskip_host(block, block, 4, 1, nullptr, &qp, 1, out, nullptr, nullptr, nullptr, nullptr, 0, 0, &zero, 2, nullptr, 1, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_tskip_host(block, block, 4, 1, nullptr, &bad_qp, 1, out, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 2, nullptr, 1, nullptr) == PNN_E_ARG);
    CHECK(pnn_trquant_tskip_host(block, block, 4, 1, nullptr, &qp, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 2, nullptr, 1, nullptr) == PNN_E_ARG);
    CHECK(out[0] == 0);
    printf("sanitize_transform_skip: ok\n");
    return 0;
}
