// Walsh-Hadamard transform of a T x T block held in registers, rows then columns: the butterflies of HM's xCalcHADs4x4 / xCalcHADs8x8
// (TComRdCost.cpp) up to the order of the coefficients, which a sum of absolute values does not see.  Integer adds only.  Shared by
// block_cost_kernel (pnn_small.hip) and hevc_mode_hads_kernel (pnn_hevc_intra.hip).
#pragma once

namespace pnn {

template <int T>
__device__ __forceinline__ void wht_rows_cols(int (&d)[T * T])
{
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {            // rows, then columns
        const int es = pass == 0 ? 1 : T, vs = pass == 0 ? T : 1;
#pragma unroll
        for (int v = 0; v < T; v++)
#pragma unroll
            for (int len = 1; len < T; len <<= 1)
#pragma unroll
                for (int i = 0; i < T; i += len << 1)
#pragma unroll
                    for (int j = i; j < i + len; j++) {
                        const int a = d[v * vs + j * es], b = d[v * vs + (j + len) * es];
                        d[v * vs + j * es] = a + b;
                        d[v * vs + (j + len) * es] = a - b;
                    }
    }
}

// the rounding of one sub-block's sum of absolute coefficients in TComRdCost::xGetHADs (TComRdCost.cpp:1753-1824), 8-bit video
template <int T>
__device__ __forceinline__ unsigned hads_round(unsigned s)
{
    return T == 8 ? (s + 2) >> 2 : (s + 1) >> 1;
}

}  // namespace pnn
