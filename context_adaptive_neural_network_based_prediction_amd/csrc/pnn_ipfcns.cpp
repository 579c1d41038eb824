// IPFCN-S host twin (pure host code): the four InnerProduct layers of IntraFCN205_deploy_Size{w}.prototxt with PReLU between
// them, written from the exact-f32 order of INTEGRATION.md section 4 (revision 6, items 4, 6 and 8) -- what the device pass
// (ipfcns_pass, pnn_passes.cpp) computes on the tap-GEMM kernels.  Per output: K walked in 16-deep chunks, k = 0, 8, 1, 9, ..,
// 7, 15 inside a chunk; more than 20 chunks are summed in segments of 20 (the last one shorter), each a chain of fmaf from +0;
// the segment sums added in order; + bias; then PReLU v > 0 ? v : a * v behind fc1 .. fc3.  Every multiply-add is an explicit
// fmaf and nothing else may fuse (the pragma below).  Blocks are spread over threads; a block's arithmetic never depends on
// which thread or which group of blocks it travels in, so the bits do not depend on the thread count.
#include "pnn_ctx.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 8;                               // blocks per pass over a layer's weights
constexpr int kStrip = 256;                            // outputs per pass over a segment

// acc[j][co] = fma(x[j][k], Wt[k][co], acc[j][co]) for the nb blocks of a tile: one chain per output, outputs side by side
#define PNN_IPFCNS_AXPY(NAME, ATTR)                                                                        \
    ATTR static void NAME(float* acc, const float* xk, int nb, const float* row, int ns, int N)           \
    {                                                                                                      \
        for (int j = 0; j < nb; j++) {                                                                     \
            const float xv = xk[j];                                                                        \
            float* a = acc + (size_t)j * N;                                                                \
            for (int co = 0; co < ns; co++) a[co] = std::fma(xv, row[co], a[co]);                          \
        }                                                                                                  \
    }
#if defined(__x86_64__)
PNN_IPFCNS_AXPY(axpy_fma, __attribute__((target("avx2,fma"))))
#endif
PNN_IPFCNS_AXPY(axpy_plain, )

using AxpyFn = void (*)(float*, const float*, int, const float*, int, int);

AxpyFn pick_axpy()
{
#if defined(__x86_64__)
    if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) return axpy_fma;
#endif
    return axpy_plain;
}

// One layer for a tile of nb blocks: X [nb][K] -> Y [nb][N] (Wt: strips of kStrip outputs, each [K][strip]; slope == NULL: no activation)
void layer_tile(AxpyFn axpy, const float* Wt, const float* b, const float* slope, int K, int N, const float* X, int nb, float* Y,
                std::vector<float>& acc, std::vector<float>& tot, std::vector<float>& xk)
{
    const int nch = K / 16, segc = nch > 20 ? 20 : nch, nseg = (nch + segc - 1) / segc;
    acc.assign((size_t)nb * N, 0.f);
    tot.assign((size_t)nb * N, 0.f);
    xk.resize(nb);
    for (int sg = 0; sg < nseg; sg++) {
        std::fill(acc.begin(), acc.end(), 0.f);
        const int c1 = std::min(nch, (sg + 1) * segc);
        for (int o0 = 0; o0 < N; o0 += kStrip)       // strips of outputs: the tile's accumulators stay in L1
            for (int ch = sg * segc; ch < c1; ch++)
                for (int i = 0; i < 16; i++) {
                    const int k = 16 * ch + (i >> 1) + 8 * (i & 1);
                    for (int j = 0; j < nb; j++) xk[j] = X[(size_t)j * K + k];
                    axpy(acc.data() + o0, xk.data(), nb, Wt + (size_t)o0 * K + (size_t)k * std::min(kStrip, N - o0), std::min(kStrip, N - o0), N);
                }
        if (sg == 0) tot = acc;
        else for (size_t q = 0; q < tot.size(); q++) tot[q] = tot[q] + acc[q];
    }
    for (int j = 0; j < nb; j++)
        for (int co = 0; co < N; co++) {
            float v = tot[(size_t)j * N + co] + b[co];
            if (slope) v = v > 0.f ? v : slope[co] * v;
            Y[(size_t)j * N + co] = v;
        }
}

}  // namespace

extern "C" int pnn_ipfcns_forward_host(int width, const float* params, const float* x, int n, int layers, float* out)
{
    int K, H;
    if (!pnn::ipfcns_dims(width, &K, &H) || layers < 1 || layers > 4 || n < 0 || (n > 0 && (!params || !x || !out))) return PNN_E_ARG;
    if (n == 0) return PNN_OK;
    const int dims[5] = {K, H, H, H, width * width};
    std::vector<float> Wt[4];
    const float *bias[4], *slope[4] = {nullptr, nullptr, nullptr, nullptr};
    const float* p = params;
    for (int l = 0; l < 4; l++) {                       // Caffe's [out][in] -> strips of kStrip outputs, each [in][strip]
        const int ki = dims[l], ni = dims[l + 1];
        Wt[l].resize((size_t)ki * ni);
        for (int o = 0; o < ni; o++) {
            const int o0 = o / kStrip * kStrip, ns = std::min(kStrip, ni - o0);
            for (int k = 0; k < ki; k++) Wt[l][(size_t)o0 * ki + (size_t)k * ns + (o - o0)] = p[(size_t)o * ki + k];
        }
        p += (size_t)ki * ni;
        bias[l] = p; p += ni;
        if (l < 3) { slope[l] = p; p += ni; }
    }
    const AxpyFn axpy = pick_axpy();
    const int nout = dims[layers];
    const long ntiles = ((long)n + kTile - 1) / kTile;
    std::atomic<long> next{0};
    auto work = [&] {
        std::vector<float> acc, tot, xk, a((size_t)kTile * H), b((size_t)kTile * H);
        for (long t; (t = next.fetch_add(1)) < ntiles;) {
            const long j0 = t * kTile;
            const int nb = (int)std::min<long>(kTile, n - j0);
            const float* in = x + (size_t)j0 * K;
            for (int l = 0; l < layers; l++) {
                float* dst = l == layers - 1 ? out + (size_t)j0 * nout : (l % 2 ? b.data() : a.data());
                layer_tile(axpy, Wt[l].data(), bias[l], slope[l], dims[l], dims[l + 1], in, nb, dst, acc, tot, xk);
                in = dst;
            }
        }
    };
    const int nt = (int)std::max<long>(1, std::min<long>({16L, (long)std::max(1u, std::thread::hardware_concurrency()), ntiles}));
    std::vector<std::thread> th;
    for (int i = 1; i < nt; i++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return PNN_OK;
}
