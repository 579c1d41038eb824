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
//
// cu_tree_picture_kernel: the same body -- cu_tree_body<PICTURE>, written once -- for the CTUs of one
// anti-diagonal r + c of every image's CTU grid.  It differs in which CTU a workgroup decides, in where the 16 edge cells come from
// (the maps the launches of earlier diagonals left in cu_depths: cutree::edge_from_maps) and in lane 0 adding the root's D and F to
// the image's sums.  launch_cu_tree_picture makes one launch per diagonal on one stream; no workgroup ever waits on another.
// cu_tree_leaves_kernel: one width's leaves from a second pass's device outputs, four elements per lane, no LDS.
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

// Which CTU a workgroup of the picture kernel decides: blockIdx.x counts (image, CTU of the anti-diagonal g.diagonal, from the top)
struct PictureCtu { int image, row, col, ctu; };
__device__ inline PictureCtu picture_ctu(const CuTreePictureGrid& g, int block)
{
    const int first_row = g.diagonal < g.ctu_cols ? 0 : g.diagonal - (g.ctu_cols - 1);
    const int last_row = g.diagonal < g.ctu_rows ? g.diagonal : g.ctu_rows - 1, count = last_row - first_row + 1;
    PictureCtu c;
    c.image = block / count;
    c.row = first_row + block % count;
    c.col = g.diagonal - c.row;
    c.ctu = (c.image * g.ctu_rows + c.row) * g.ctu_cols + c.col;
    return c;
}

// The one body of both kernels.  PICTURE false: cu_tree_kernel, CTU blockIdx.x under the caller's edges (g is not read).  PICTURE
// true: cu_tree_picture_kernel, the CTU picture_ctu names under the edges of its neighbours' maps, its root added to the image's sums.
template <bool PICTURE>
__device__ __forceinline__ void cu_tree_body(const CuTreeParams& p, const CuTreePictureGrid& g)
{
    using namespace cutree;
    __shared__ uint64_t rate[kLeaves], best_dist[kNodes], best_rate[kNodes];
    __shared__ double costs[kNodes * 2];
    __shared__ uint32_t dist[kLeaves], hist[2 * kWidths];
    __shared__ uint8_t depth[kCells], nxn[kCells], edge[16];
    __shared__ QpBits bits;

    const int lane = threadIdx.x, qi = blockIdx.y;
    PictureCtu where = {0, 0, 0, (int)blockIdx.x};
    if (PICTURE) where = picture_ctu(g, (int)blockIdx.x);
    const size_t at = (size_t)qi * p.n_ctu + where.ctu;
    stage_width<0>(p, at, lane, dist, rate);
    stage_width<1>(p, at, lane, dist, rate);
    stage_width<2>(p, at, lane, dist, rate);
    stage_width<3>(p, at, lane, dist, rate);
    stage_width<4>(p, at, lane, dist, rate);
    if (lane < 16) {
        if (PICTURE) {
            // the neighbours' maps were written by launches of earlier diagonals on this stream; they lie one CTU and one CTU row back
            const uint8_t* own = p.cu_depths + at * kCells;
            edge[lane] = edge_from_maps(where.col ? own - kCells : nullptr, where.row ? own - (size_t)g.ctu_cols * kCells : nullptr, lane);
        } else {
            const uint8_t* e = lane < 8 ? p.left : p.above;
            edge[lane] = e ? e[at * 8 + (lane & 7)] : (uint8_t)kNoDepth;
        }
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
        if (PICTURE) {
            const size_t image = (size_t)qi * g.n_images + where.image;
            if (g.image_dists) atomicAdd(reinterpret_cast<unsigned long long*>(g.image_dists + image), (unsigned long long)best_dist[0]);
            if (g.image_rates) atomicAdd(reinterpret_cast<unsigned long long*>(g.image_rates + image), (unsigned long long)best_rate[0]);
        }
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

__global__ __launch_bounds__(kCtLanes) void cu_tree_kernel(const CuTreeParams p) { cu_tree_body<false>(p, CuTreePictureGrid{}); }

__global__ __launch_bounds__(kCtLanes) void cu_tree_picture_kernel(const CuTreeParams p, const CuTreePictureGrid g) { cu_tree_body<true>(p, g); }

// Four consecutive elements per lane: whole groups as one uint4, two pairs of uint64 and one uchar4 where the host found every array
// aligned for that (vec), else -- and in the last, partial group -- element by element.  No LDS.
constexpr int kLeafLanes = 256;

__global__ __launch_bounds__(kLeafLanes) void cu_tree_leaves_kernel(const CuTreeLeavesParams p, const int vec)
{
    const long first = 4 * ((long)blockIdx.x * kLeafLanes + threadIdx.x);
    if (first >= p.total) return;
    if (vec && first + 4 <= p.total) {
        *reinterpret_cast<uint4*>(p.dist + first) = *reinterpret_cast<const uint4*>(p.sses + first);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const ulonglong2 r = *reinterpret_cast<const ulonglong2*>(p.rates + first + 2 * h);
            const ulonglong2 side = *reinterpret_cast<const ulonglong2*>(p.side_rates + first + 2 * h);
            *reinterpret_cast<ulonglong2*>(p.rate + first + 2 * h) = make_ulonglong2(r.x + side.x, r.y + side.y);
        }
        *reinterpret_cast<uchar4*>(p.mode + first) = *reinterpret_cast<const uchar4*>(p.modes + first);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const long e = first + i;
        if (e < p.total) { p.dist[e] = p.sses[e]; p.rate[e] = p.rates[e] + p.side_rates[e]; p.mode[e] = p.modes[e]; }
    }
}

}  // namespace

static bool cu_tree_launchable(const CuTreeParams& p)
{
    if (p.n_ctu < 1 || p.nb_qps < 1 || p.nb_qps > cutree::kMaxQps) return false;
    for (int k = 0; k < cutree::kWidths; k++)
        if (!p.dist[k] || !p.rate[k] || (p.selected_pnn && !p.mode[k])) return false;
    return true;
}

hipError_t launch_cu_tree(const CuTreeParams& p, hipStream_t s)
{
    if (!cu_tree_launchable(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cu_tree_kernel, dim3((unsigned)p.n_ctu, (unsigned)p.nb_qps), dim3(kCtLanes), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_cu_tree_picture(const CuTreeParams& p, const CuTreePictureGrid& grid, hipStream_t s)
{
    if (!cu_tree_launchable(p) || !p.cu_depths || grid.n_images < 1 || grid.ctu_rows < 1 || grid.ctu_cols < 1 ||
        (long long)grid.n_images * grid.ctu_rows * grid.ctu_cols != p.n_ctu) return hipErrorInvalidValue;
    CuTreePictureGrid g = grid;
    for (g.diagonal = 0; g.diagonal < g.ctu_rows + g.ctu_cols - 1; g.diagonal++) {
        const int first_row = g.diagonal < g.ctu_cols ? 0 : g.diagonal - (g.ctu_cols - 1);
        const int last_row = g.diagonal < g.ctu_rows ? g.diagonal : g.ctu_rows - 1;
        // (the same two lines as picture_ctu: a workgroup beyond the diagonal's CTUs would write another CTU's outputs)
        const long long blocks = (long long)(last_row - first_row + 1) * g.n_images;
        hipLaunchKernelGGL(cu_tree_picture_kernel, dim3((unsigned)blocks, (unsigned)p.nb_qps), dim3(kCtLanes), 0, s, p, g);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_cu_tree_leaves(const CuTreeLeavesParams& p, hipStream_t s)
{
    if (p.total < 1 || !p.sses || !p.rates || !p.side_rates || !p.modes || !p.dist || !p.rate || !p.mode) return hipErrorInvalidValue;
    const long groups = (p.total + 3) / 4, blocks = (groups + kLeafLanes - 1) / kLeafLanes;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const int vec = ((uintptr_t)p.sses | (uintptr_t)p.rates | (uintptr_t)p.side_rates | (uintptr_t)p.dist | (uintptr_t)p.rate) % 16 == 0 &&
                    ((uintptr_t)p.modes | (uintptr_t)p.mode) % 4 == 0;
    hipLaunchKernelGGL(cu_tree_leaves_kernel, dim3((unsigned)blocks), dim3(kLeafLanes), 0, s, p, vec);
    return hipGetLastError();
}

}  // namespace pnn
