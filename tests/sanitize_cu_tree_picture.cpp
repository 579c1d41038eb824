// Stand-alone AddressSanitizer + UBSan program over the host twin of the coding tree over whole pictures
// (tests/test_cu_tree_picture_sanitizer.py compiles it together with csrc/pnn_cu_tree.cpp): pnn_cu_tree_picture_host on seeded, zero
// and extreme leaves over the grids 1x1, 1x2, 2x1, 2x3 and 3x2, 1 and 2 images, 1 and 8 QPs, in buffers of exactly the documented
// sizes, modes NULL and given, every output alone and all together; the per-image sums against the per-CTU outputs; the refusals.
// Any report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pnn_hip.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "sanitize_cu_tree_picture: %s failed at line %d\n", #x, __LINE__); abort(); } } while (0)

int main()
{
    std::mt19937_64 rng(7331);
    const int all_qps[8] = {0, 12, 22, 27, 32, 37, 45, 51};
    const double own[8] = {0., 0.5, 3., 17., 90., 400., 2000., 1e6};
    const int grids[5][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 3}, {3, 2}};
    for (int kind = 0; kind < 3; kind++)                  // 0 seeded, 1 zero, 2 the largest values
        for (const auto& grid : grids)
            for (int n_images : {1, 2})
                for (int nq : {1, 8})
                    for (int options = 0; options < 4; options++) {
                        const bool with_modes = options & 1, lambdas = options & 2;
                        const int rows = grid[0], cols = grid[1], n_ctu = n_images * rows * cols;
                        std::vector<std::vector<uint32_t>> dist(5);
                        std::vector<std::vector<uint64_t>> rate(5);
                        std::vector<std::vector<uint8_t>> mode(5);
                        const uint32_t* d[5];
                        const uint64_t* r[5];
                        const uint8_t* m[5];
                        for (int k = 0; k < 5; k++) {
                            const size_t count = (size_t)nq * n_ctu * (256 >> (2 * k));
                            dist[k].resize(count); rate[k].resize(count); mode[k].resize(count);
                            for (size_t i = 0; i < count; i++) {
                                dist[k][i] = kind == 0 ? (uint32_t)(rng() % (4000u << (2 * k))) : kind == 1 ? 0u : 0xffffffffu;
                                rate[k][i] = kind == 0 ? rng() % (1u << 22) : kind == 1 ? 0u : (uint64_t)1 << 52;
                                mode[k][i] = (uint8_t)(rng() % 36);
                            }
                            d[k] = dist[k].data(); r[k] = rate[k].data(); m[k] = mode[k].data();
                        }
                        const size_t qc = (size_t)nq * n_ctu, qi_images = (size_t)nq * n_images;
                        for (int only = -1; only < 10; only++) {
                            if (only == 7 && !with_modes) continue;
                            const auto want = [&](int i) { return (only < 0 && (i != 7 || with_modes)) || only == i; };
                            std::vector<uint8_t> depths(qc * 64), nxn(qc * 64);
                            std::vector<double> node_costs(qc * 85 * 2), ctu_costs(qc);
                            std::vector<uint64_t> ctu_dists(qc), ctu_rates(qc), image_dists(qi_images), image_rates(qi_images);
                            std::vector<uint32_t> selected((size_t)nq * 5), selected_pnn((size_t)nq * 5);
                            CHECK(pnn_cu_tree_picture_host(all_qps, nq, lambdas ? own : nullptr, n_images, rows, cols, d, r, with_modes ? m : nullptr,
                                                           options & 1 ? 35 : 18, want(0) ? depths.data() : nullptr, want(1) ? nxn.data() : nullptr,
                                                           want(2) ? node_costs.data() : nullptr, want(3) ? ctu_costs.data() : nullptr,
                                                           want(4) ? ctu_dists.data() : nullptr, want(5) ? ctu_rates.data() : nullptr,
                                                           want(6) ? selected.data() : nullptr, want(7) ? selected_pnn.data() : nullptr,
                                                           want(8) ? image_dists.data() : nullptr, want(9) ? image_rates.data() : nullptr) == PNN_OK);
                            if (only >= 0) continue;
                            for (int qi = 0; qi < nq; qi++) {
                                uint64_t area = 0;
                                for (int k = 0; k < 5; k++) area += (uint64_t)selected[qi * 5 + k] << (4 + 2 * k);
                                CHECK(area == (uint64_t)n_ctu * 4096);
                                for (int image = 0; image < n_images; image++) {
                                    uint64_t sum_dist = 0, sum_rate = 0;
                                    for (int c = 0; c < rows * cols; c++) {
                                        sum_dist += ctu_dists[(size_t)qi * n_ctu + image * rows * cols + c];
                                        sum_rate += ctu_rates[(size_t)qi * n_ctu + image * rows * cols + c];
                                    }
                                    CHECK(image_dists[(size_t)qi * n_images + image] == sum_dist && image_rates[(size_t)qi * n_images + image] == sum_rate);
                                }
                            }
                        }
                    }
    // the refusals: nothing is read or written
    std::vector<uint32_t> dist(256);
    std::vector<uint64_t> rate(256);
    const uint32_t* d[5] = {dist.data(), dist.data(), dist.data(), dist.data(), dist.data()};
    const uint64_t* r[5] = {rate.data(), rate.data(), rate.data(), rate.data(), rate.data()};
    const uint32_t* d_hole[5] = {dist.data(), dist.data(), nullptr, dist.data(), dist.data()};
    const int qp = 30, bad_qp = 52;
    const double negative = -1.;
    uint64_t sum = 0;
    uint32_t counts[5];
    const auto call = [&](const int* qps, int nq, const double* lambdas, int n_images, int rows, int cols, const uint32_t* const* dists,
                          uint64_t* image_dists, uint32_t* selected_pnn) {
        return pnn_cu_tree_picture_host(qps, nq, lambdas, n_images, rows, cols, dists, r, nullptr, 35, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, selected_pnn, image_dists, nullptr);
    };
    CHECK(call(&qp, 1, nullptr, 1, 1, 1, d, &sum, nullptr) == PNN_OK);
    CHECK(call(&qp, 0, nullptr, 1, 1, 1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 9, nullptr, 1, 1, 1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&bad_qp, 1, nullptr, 1, 1, 1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 0, 1, 1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 1, 0, 1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 1, 1, -1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 65536, 65536, 1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 1, 65536, 65536, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 2, 32768, 32768, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 1, 1, 1, d_hole, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 1, 1, 1, nullptr, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, &negative, 1, 1, 1, d, &sum, nullptr) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 1, 1, 1, d, nullptr, counts) == PNN_E_ARG);
    CHECK(call(&qp, 1, nullptr, 1, 1, 1, d, nullptr, nullptr) == PNN_E_ARG);
    printf("sanitize_cu_tree_picture: ok\n");
    return 0;
}
