// Host-twin rate of the HEVC best-mode search (tools/hevc_best_mode_rate.py builds and runs it): per block the 35 calls of
// pnn_hevc_intra_predict, the SSE of each against the target and the smallest (lowest index among ties), blocks split over
// OpenMP threads.  Prints "w threads blocks seconds blocks_per_s checksum".
#include "../include/pnn_hip.h"

#include <omp.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s width blocks threads\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), n = atoi(argv[2]), threads = atoi(argv[3]), side = 2 * w + 1;
    std::vector<uint8_t> pats((size_t)n * side * side), tgts((size_t)n * w * w);
    unsigned s = 12345;
    for (auto& v : pats) v = (uint8_t)((s = s * 1103515245u + 12345u) >> 24);
    for (auto& v : tgts) v = (uint8_t)((s = s * 1103515245u + 12345u) >> 24);
    std::vector<int> best(n);
    omp_set_num_threads(threads);
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel
    {
        std::vector<uint8_t> pred((size_t)w * w);
#pragma omp for schedule(static)
        for (int b = 0; b < n; b++) {
            unsigned best_sse = ~0u;
            for (int m = 0; m < 35; m++) {
                if (pnn_hevc_intra_predict(&pats[(size_t)b * side * side], side, side, w, m, pred.data())) abort();
                unsigned sse = 0;
                for (int i = 0; i < w * w; i++) {
                    const int d = (int)pred[i] - tgts[(size_t)b * w * w + i];
                    sse += (unsigned)(d * d);
                }
                if (sse < best_sse) { best_sse = sse; best[b] = m; }
            }
        }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    long sum = 0;
    for (int v : best) sum += v;
    printf("%d %d %d %.6f %.1f %ld\n", w, threads, n, sec, n / sec, sum);
    return 0;
}
