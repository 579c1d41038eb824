// IPFCN-S (Li et al., the fully-connected intra predictor of the reference's ipfcns/ipfcns.py) around the exact-f32 GEMM: the
// three element-wise kernels of its pass (pnn_passes.cpp, ipfcns_pass).  The four InnerProduct layers themselves run on the
// existing tap-GEMM family (build_fc_layer with act = 0, run_gemm): order revision 6, items 4, 6 and 8 of INTEGRATION.md section 4.
//   ipfcns_gather_kernel    uint8 picture -> the two groups of reference lines minus their mean (ipfcns.py:97-494)
//   ipfcns_prelu_kernel     Caffe PReLU, one slope per channel, in place
//   ipfcns_epilogue_kernel  + mean, clip, rint (half to even, tools.cast_float_to_uint8), optional f32 copy and per-block SSE
// ... and the two element-wise kernels of the evaluator's scoring path from pictures (pnn_score_pictures_device):
//   score_desc_kernel       (picture, position, masks) -> the gather's descriptor of every block
//   score_epilogue_kernel   the same uint8 rule on any predictor's floats, with the target read from the picture
// Of a pair of planes (decoded, original) score_desc_kernel's descriptors address the decoded one, the epilogue's picture is the original.
// One wave per block in the gather and the epilogues (K <= 1088, w^2 <= 4096 values), four waves per workgroup.  All plain f32
// operations: nothing here can contract (a subtraction, an addition, one multiply, a division by __fdiv_rn).
#include "pnn_kernels.h"

namespace pnn {
namespace {

constexpr int kWaves = 4;

__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sample k of the flattened pair of groups (row-major above group 8 x (2w + 8), then row-major left group 2w x 8)
__device__ inline int line_offset(int k, int w, int W)
{
    const int wa = 2 * w + 8, na = 8 * wa;
    if (k < na) return (k / wa) * W + k % wa;
    const int k2 = k - na;
    return (8 + (k2 >> 3)) * W + (k2 & 7);
}

__global__ __launch_bounds__(64 * kWaves) void ipfcns_gather_kernel(const IpfcnsGatherParams p)
{
    const int lane = threadIdx.x & 63;
    const long bb = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (bb >= p.nb) return;
    const long gb = p.b0 + bb;
    const long img = gb / p.positions;
    const int pos = (int)(gb - img * p.positions);
    const uint8_t* src = p.channels + (size_t)img * p.H * p.W + (size_t)p.rows[pos] * p.W + p.cols[pos];
    const int K = 64 + 32 * p.w;
    int s = 0;
    for (int k = lane; k < K; k += 64) s += src[line_offset(k, p.w, p.W)];
    s = wave_sum(s);                                   // exact: at most 255 * 1088 < 2^24
    const float mean = __fdiv_rn((float)s, (float)K);  // fl32(S / K), correctly rounded
    float* x = p.x + bb * K;
    for (int k = lane; k < K; k += 64) x[k] = (float)src[line_offset(k, p.w, p.W)] - mean;
    if (lane == 0) p.mean[bb] = mean;
}

__global__ __launch_bounds__(256) void ipfcns_prelu_kernel(float4* y, const float* slope, long total4, int H)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
        float4 v = y[i];
        const int c = (int)((i * 4) % H);
        v.x = v.x > 0.f ? v.x : slope[c] * v.x;
        v.y = v.y > 0.f ? v.y : slope[c + 1] * v.y;
        v.z = v.z > 0.f ? v.z : slope[c + 2] * v.z;
        v.w = v.w > 0.f ? v.w : slope[c + 3] * v.w;
        y[i] = v;
    }
}

__global__ __launch_bounds__(64 * kWaves) void ipfcns_epilogue_kernel(const IpfcnsEpilogueParams p)
{
    const int lane = threadIdx.x & 63;
    const long bb = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (bb >= p.nb) return;
    const float mean = p.mean[bb];
    const size_t o = (size_t)bb * p.w2;
    int acc = 0;
    for (int e = lane; e < p.w2; e += 64) {
        const float v = p.fc4[o + e] + mean;
        if (p.f32) p.f32[o + e] = v;
        const int q = (int)rintf(fminf(fmaxf(v, 0.f), 255.f));
        if (p.u8) p.u8[o + e] = (uint8_t)q;
        if (p.sse) { const int d = q - (int)p.targets[o + e]; acc += d * d; }
    }
    if (p.sse) {
        acc = wave_sum(acc);                           // <= 65025 * 1024 < 2^31
        if (lane == 0) p.sse[bb] = (uint32_t)acc;
    }
}

__global__ __launch_bounds__(256) void score_desc_kernel(const ScoreDescParams p)
{
    const long bb = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (bb >= p.nb) return;
    const long gb = p.b0 + bb;
    const long img = gb / p.pic.positions;
    const int pos = (int)(gb - img * p.pic.positions);
    const int units = 2 * p.w / 4;
    TbDev d;
    d.origin = (img * p.pic.H + p.pic.rows[pos] + p.w) * p.pic.W + p.pic.cols[pos] + p.w;
    d.stride = p.pic.W;
    const int mask_w = p.pic.mask_w ? p.pic.mask_w[pos] : p.mask_w, mask_h = p.pic.mask_h ? p.pic.mask_h[pos] : p.mask_h;   // per position, or the call's
    d.above_mask = (uint32_t)((1ull << (units - mask_w / 4)) - 1ull);      // 64 bits: the count is 32 at w = 64 without a mask
    d.left_units = units - mask_h / 4;
    d.reserved = 0;
    p.tbs[bb] = d;
}

__global__ __launch_bounds__(64 * kWaves) void score_epilogue_kernel(const ScoreEpilogueParams p)
{
    const int lane = threadIdx.x & 63;
    const long bb = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (bb >= p.nb) return;
    const long gb = p.b0 + bb;
    const long img = gb / p.pic.positions;
    const int pos = (int)(gb - img * p.pic.positions);
    const uint8_t* tg = p.pic.channels + ((size_t)img * p.pic.H + p.pic.rows[pos] + p.w) * p.pic.W + p.pic.cols[pos] + p.w;
    const int w2 = p.w * p.w;
    const size_t o = (size_t)bb * w2;
    int acc = 0;
    for (int e = lane; e < w2; e += 64) {
        const int t = tg[(size_t)(e / p.w) * p.pic.W + e % p.w];
        if (p.targets) p.targets[o + e] = (uint8_t)t;
        if (!p.pred) continue;
        const float v = __fadd_rn(p.pred[o + e], p.mean);
        const int q = (int)rintf(fminf(fmaxf(v, 0.f), 255.f));
        if (p.u8) p.u8[o + e] = (uint8_t)q;
        const int d = q - t;
        acc += d * d;
    }
    if (p.sse) {
        acc = wave_sum(acc);                           // <= 65025 * 4096 < 2^31
        if (lane == 0) p.sse[bb] = (uint32_t)acc;
    }
}

}  // namespace

hipError_t launch_ipfcns_gather(const IpfcnsGatherParams& p, hipStream_t s)
{
    if (p.nb <= 0) return hipSuccess;
    hipLaunchKernelGGL(ipfcns_gather_kernel, dim3((unsigned)((p.nb + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ipfcns_prelu(float* y, const float* slope, long total, int H, hipStream_t s)
{
    if (total <= 0) return hipSuccess;
    if (total % 4 || H % 4) return hipErrorInvalidValue;
    const long total4 = total / 4;
    const long blocks = std::min<long>((total4 + 255) / 256, 8L * device_info().cus);
    hipLaunchKernelGGL(ipfcns_prelu_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<float4*>(y), slope, total4, H);
    return hipGetLastError();
}

hipError_t launch_ipfcns_epilogue(const IpfcnsEpilogueParams& p, hipStream_t s)
{
    if (p.nb <= 0) return hipSuccess;
    if (p.sse && !p.targets) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ipfcns_epilogue_kernel, dim3((unsigned)((p.nb + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_score_desc(const ScoreDescParams& p, hipStream_t s)
{
    if (p.nb <= 0) return hipSuccess;
    hipLaunchKernelGGL(score_desc_kernel, dim3((unsigned)((p.nb + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_score_epilogue(const ScoreEpilogueParams& p, hipStream_t s)
{
    if (p.nb <= 0) return hipSuccess;
    if ((p.u8 || p.sse) && !p.pred) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_epilogue_kernel, dim3((unsigned)((p.nb + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s, p);
    return hipGetLastError();
}

}  // namespace pnn
