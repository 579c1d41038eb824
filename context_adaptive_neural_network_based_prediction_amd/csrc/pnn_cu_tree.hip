// The coding-tree pass on the GPU (include/pnn_hip.h, "the coding tree").  Bit-exact against the host twin
// (pnn_cu_tree.cpp), with which it shares every line of the decision (pnn_cu_tree.h).
//
// cu_tree_kernel: one wavefront per (QP, CTU), the CTU in blockIdx.x and the QP in blockIdx.y.  The lanes stage the CTU's 341 leaves
// -- D as uint32, F as uint64, width by width, consecutive lanes reading consecutive elements -- and the 16 edge cells into LDS.  The
// depth-3 level then runs in one step, lane i deciding 8 x 8 node i between SIZE_2Nx2N and SIZE_NxN; lane 0 walks the 21 upper nodes
// in z-order post-order with the depth map in LDS (a node's split context reads what the subtrees before it wrote: the walk is serial
// and latency-bound by design, 63 lanes idle through it); then all lanes write the outputs that were asked for.  The tail counts the
// selected blocks per width: lane z speaks for minimum-CU cell z where that is the first cell of its CU, into a ten-bin LDS histogram
// whose nonzero bins go to the output with integer atomics -- the caller zeroed it on the stream, and integer sums do not show the
// order.  6.9 KiB of LDS per workgroup, no scratch, every loop with a compile-time bound.
#include "pnn_kernels.h"

namespace pnn {
namespace {

constexpr int kCtLanes = 64;

template <int K>
__device__ inline void stage_width(const CuTreeParams& p, size_t at, int lane, uint32_t* dist, uint64_t* rate)
{
    constexpr int count = 256 >> (2 * K), first = K == 0 ? cutree::kNodes : K == 1 ? 21 : K == 2 ? 5 : K == 3 ? 1 : 0;
    const uint32_t* d = p.dist[K] + at * count;
    const uint64_t* f = p.rate[K] + at * count;
#pragma unroll
    for (int i = 0; i < (count + kCtLanes - 1) / kCtLanes; i++) {
        const int e = i * kCtLanes + lane;
        if (e < count) { dist[first + e] = d[e]; rate[first + e] = f[e]; }
    }
}

__global__ __launch_bounds__(kCtLanes) void cu_tree_kernel(const CuTreeParams p)
{
    using namespace cutree;
    __shared__ uint64_t rate[kLeaves], best_dist[kNodes], best_rate[kNodes];
    __shared__ double costs[kNodes * 2];
    __shared__ uint32_t dist[kLeaves], hist[2 * kWidths];
    __shared__ uint8_t depth[kCells], nxn[kCells], edge[16];
    __shared__ QpBits bits;

    const int lane = threadIdx.x, qi = blockIdx.y;
    const size_t at = (size_t)qi * p.n_ctu + blockIdx.x;
    stage_width<0>(p, at, lane, dist, rate);
    stage_width<1>(p, at, lane, dist, rate);
    stage_width<2>(p, at, lane, dist, rate);
    stage_width<3>(p, at, lane, dist, rate);
    stage_width<4>(p, at, lane, dist, rate);
    if (lane < 16) {
        const uint8_t* e = lane < 8 ? p.left : p.above;
        edge[lane] = e ? e[at * 8 + (lane & 7)] : (uint8_t)kNoDepth;
    }
    if (lane < 2 * kWidths) hist[lane] = 0;
    // the QP's bins in LDS: the decision indexes them by context, and an argument indexed by a runtime value would go through scratch
    if (lane < (int)(sizeof(QpBits) / 4)) {
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < kMaxQps; i++)
            if (i == qi) word = reinterpret_cast<const uint32_t*>(&p.bits[i])[lane];
        reinterpret_cast<uint32_t*>(&bits)[lane] = word;
    }
    double lambda = 0.;
#pragma unroll
    for (int i = 0; i < kMaxQps; i++)
        if (i == qi) lambda = p.lambda[i];
    __syncthreads();

    const Work w{dist, rate, best_dist, best_rate, costs, depth, nxn, edge, edge + 8};
    decide_part_size(w, lane, bits, lambda);
    __syncthreads();
    if (lane == 0) walk_upper(w, bits, lambda);
    __syncthreads();

    if (p.cu_depths) p.cu_depths[at * kCells + lane] = depth[lane];
    if (p.part_nxn) p.part_nxn[at * kCells + lane] = nxn[lane];
    if (p.node_costs) {
#pragma unroll
        for (int i = 0; i < (kNodes * 2 + kCtLanes - 1) / kCtLanes; i++) {
            const int e = i * kCtLanes + lane;
            if (e < kNodes * 2) p.node_costs[at * kNodes * 2 + e] = costs[e];
        }
    }
    if (lane == 0) {
        if (p.ctu_costs) p.ctu_costs[at] = costs[1] < costs[0] ? costs[1] : costs[0];
        if (p.ctu_dists) p.ctu_dists[at] = best_dist[0];
        if (p.ctu_rates) p.ctu_rates[at] = best_rate[0];
    }
    if (!p.selected && !p.selected_pnn) return;

    int leaf = 0, count = 0;
    const int k = selected_block(w, lane, &leaf, &count);
    if (k >= 0) {
        atomicAdd(&hist[k], (uint32_t)count);
        if (p.selected_pnn) {
            // the width's mode array: chosen by comparisons, so that no pointer array is indexed by a runtime value
            const uint8_t* modes = k == 0 ? p.mode[0] : k == 1 ? p.mode[1] : k == 2 ? p.mode[2] : k == 3 ? p.mode[3] : p.mode[4];
            modes += at * (size_t)(256 >> (2 * k)) + leaf;
            uint32_t hits = 0;
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < count) hits += modes[i] == p.pnn_mode;
            if (hits) atomicAdd(&hist[kWidths + k], hits);
        }
    }
    __syncthreads();
    if (lane < kWidths) {
        if (p.selected && hist[lane]) atomicAdd(&p.selected[qi * kWidths + lane], hist[lane]);
    } else if (lane < 2 * kWidths) {
        if (p.selected_pnn && hist[lane]) atomicAdd(&p.selected_pnn[qi * kWidths + lane - kWidths], hist[lane]);
    }
}

}  // namespace

hipError_t launch_cu_tree(const CuTreeParams& p, hipStream_t s)
{
    if (p.n_ctu < 1 || p.nb_qps < 1 || p.nb_qps > cutree::kMaxQps) return hipErrorInvalidValue;
    for (int k = 0; k < cutree::kWidths; k++)
        if (!p.dist[k] || !p.rate[k] || (p.selected_pnn && !p.mode[k])) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cu_tree_kernel, dim3((unsigned)p.n_ctu, (unsigned)p.nb_qps), dim3(kCtLanes), 0, s, p);
    return hipGetLastError();
}

}  // namespace pnn
