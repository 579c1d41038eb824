// Shim of tests/golden/make_hm_transforms.py: HM's own free functions xTrMxN and xITrMxN (TComTrQuant.cpp of an HM-16.15 tree, compiled
// by path next to this file) on blocks read from stdin, results to stdout.  A record is int32 {direction (0 forward, 1 inverse), T} and
// T * T int32 inputs; the answer is T * T int32 outputs.  8-bit video, maxLog2TrDynamicRange 15, the DST at 4 x 4.  Built and run by
// the generator only; nothing of it is shipped.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "TLibCommon/CommonDef.h"   // the tree's: TCoeff is what its build options make it

Void initROM();
Void destroyROM();
Void xTrMxN(Int bitDepth, TCoeff* block, TCoeff* coeff, Int iWidth, Int iHeight, Bool useDST, const Int maxLog2TrDynamicRange);
Void xITrMxN(Int bitDepth, TCoeff* coeff, TCoeff* block, Int iWidth, Int iHeight, Bool useDST, const Int maxLog2TrDynamicRange);

int main()
{
    initROM();
    int32_t head[2];
    while (fread(head, sizeof(int32_t), 2, stdin) == 2) {
        const int t = head[1];
        if (t != 4 && t != 8 && t != 16 && t != 32) return 2;
        std::vector<int32_t> io((size_t)t * t);
        std::vector<TCoeff> in(io.size()), out(io.size());
        if (fread(io.data(), sizeof(int32_t), io.size(), stdin) != io.size()) return 3;
        for (size_t i = 0; i < io.size(); i++) in[i] = io[i];
        if (head[0] == 0) xTrMxN(8, in.data(), out.data(), t, t, t == 4, 15);
        else xITrMxN(8, in.data(), out.data(), t, t, t == 4, 15);
        for (size_t i = 0; i < io.size(); i++) io[i] = (int32_t)out[i];
        if (fwrite(io.data(), sizeof(int32_t), io.size(), stdout) != io.size()) return 4;
    }
    destroyROM();
    return 0;
}
