// Stand-alone AddressSanitizer + UBSan program over the host twin of the coding-tree pass (tests/test_cu_tree_sanitizer.py compiles it
// together with csrc/pnn_cu_tree.cpp): pnn_cu_tree_host on seeded, zero and extreme leaves at n_ctu = 1 and 3 and 1 and 8 QPs, in
// buffers of exactly the documented sizes, edges NULL and given, modes NULL and given, every output alone and all together;
// pnn_cu_tree_bins_host at every QP; the refusals.  Any report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pnn_hip.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "sanitize_cu_tree: %s failed at line %d\n", #x, __LINE__); abort(); } } while (0)

int main()
{
    std::mt19937_64 rng(5117);
    const int all_qps[8] = {0, 12, 22, 27, 32, 37, 45, 51};
    const double own[8] = {0., 0.5, 3., 17., 90., 400., 2000., 1e6};
    for (int kind = 0; kind < 3; kind++)                  // 0 seeded, 1 zero, 2 the largest values
        for (int n_ctu : {1, 3})
            for (int nq : {1, 8})
                for (int options = 0; options < 8; options++) {
                    const bool edges = options & 1, with_modes = options & 2, lambdas = options & 4;
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
                    std::vector<uint8_t> left((size_t)nq * n_ctu * 8), above(left.size());
                    for (size_t i = 0; i < left.size(); i++) {
                        left[i] = rng() % 5 == 4 ? 255 : (uint8_t)(rng() % 4);
                        above[i] = rng() % 5 == 4 ? 255 : (uint8_t)(rng() % 4);
                    }
                    const size_t qc = (size_t)nq * n_ctu;
                    for (int only = -1; only < 8; only++) {
                        if (only == 7 && !with_modes) continue;
                        const auto want = [&](int i) { return (only < 0 && (i != 7 || with_modes)) || only == i; };
                        std::vector<uint8_t> depths(qc * 64), nxn(qc * 64);
                        std::vector<double> node_costs(qc * 85 * 2), ctu_costs(qc);
                        std::vector<uint64_t> ctu_dists(qc), ctu_rates(qc);
                        std::vector<uint32_t> selected((size_t)nq * 5), selected_pnn((size_t)nq * 5);
                        CHECK(pnn_cu_tree_host(all_qps, nq, lambdas ? own : nullptr, n_ctu, d, r, with_modes ? m : nullptr, edges ? left.data() : nullptr,
                                               edges ? above.data() : nullptr, options & 2 ? 35 : 18, want(0) ? depths.data() : nullptr,
                                               want(1) ? nxn.data() : nullptr, want(2) ? node_costs.data() : nullptr, want(3) ? ctu_costs.data() : nullptr,
                                               want(4) ? ctu_dists.data() : nullptr, want(5) ? ctu_rates.data() : nullptr,
                                               want(6) ? selected.data() : nullptr, want(7) ? selected_pnn.data() : nullptr) == PNN_OK);
                        if (want(6)) {
                            for (int qi = 0; qi < nq; qi++) {
                                uint64_t area = 0;
                                for (int k = 0; k < 5; k++) area += (uint64_t)selected[qi * 5 + k] << (4 + 2 * k);
                                CHECK(area == (uint64_t)n_ctu * 4096);
                            }
                        }
                    }
                }
    for (int qp = 0; qp <= 51; qp++) {
        std::vector<uint32_t> bins(8);
        CHECK(pnn_cu_tree_bins_host(qp, bins.data()) == PNN_OK);
        for (uint32_t b : bins) CHECK(b > 0);
    }
    // the refusals: nothing is read or written
    std::vector<uint32_t> bins(8);
    CHECK(pnn_cu_tree_bins_host(52, bins.data()) == PNN_E_ARG && pnn_cu_tree_bins_host(-1, bins.data()) == PNN_E_ARG);
    CHECK(pnn_cu_tree_bins_host(30, nullptr) == PNN_E_ARG);
    std::vector<uint32_t> dist(256);
    std::vector<uint64_t> rate(256);
    const uint32_t* d[5] = {dist.data(), dist.data(), dist.data(), dist.data(), dist.data()};
    const uint64_t* r[5] = {rate.data(), rate.data(), rate.data(), rate.data(), rate.data()};
    const uint32_t* d_hole[5] = {dist.data(), dist.data(), nullptr, dist.data(), dist.data()};
    const int qp = 30, bad_qp = 52;
    const double negative = -1.;
    uint8_t edge[8] = {0, 1, 2, 3, 255, 4, 0, 0};
    double cost = 0.;
    uint32_t counts[5];
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 1, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_OK);
    CHECK(pnn_cu_tree_host(&qp, 0, nullptr, 1, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 9, nullptr, 1, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&bad_qp, 1, nullptr, 1, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 0, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 1, d_hole, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 1, nullptr, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, &negative, 1, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 1, d, r, nullptr, edge, nullptr, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 1, d, r, nullptr, nullptr, edge, 35, nullptr, nullptr, nullptr, &cost, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 1, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, counts) == PNN_E_ARG);
    CHECK(pnn_cu_tree_host(&qp, 1, nullptr, 1, d, r, nullptr, nullptr, nullptr, 35, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNN_E_ARG);
    printf("sanitize_cu_tree: ok\n");
    return 0;
}
