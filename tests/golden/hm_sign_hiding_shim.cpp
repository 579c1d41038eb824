// Shim of tests/golden/make_hm_sign_hiding.py: HM-16.15's own TComTrQuant::signBitHidingHDQ, the sign-data hiding xQuant applies with
// RDOQ 0, asked of the tree's own code (TComTrQuant.cpp, TComRom.cpp and the tree's headers, compiled by path next to this file) on a
// default-constructed TComTrQuant.  The function is private: the class is opened for this one translation unit.  Reads cases from the
// file named on the command line -- per case a line `T scan` and three lines of T * T integers: pCoef, pQCoef, deltaU -- fills a
// TUEntropyCodingParameters from g_scanOrder after initROM as getTUEntropyCodingParameters does, and prints pQCoef after the call, one
// line per case.  Numbers only; built and run by the generator, nothing of it is shipped.
#include <cstdio>
#include <vector>

// every header the class's header pulls in, with its own access specifiers, before the one class is opened
#include "TLibCommon/CommonDef.h"
#include "TLibCommon/ContextTables.h"
#include "TLibCommon/TComChromaFormat.h"
#include "TLibCommon/TComDataCU.h"
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComYuv.h"
#include "TLibCommon/TComTU.h"
#include "TLibCommon/Debug.h"
#define private public
#include "TLibCommon/TComTrQuant.h"
#undef private

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    initROM();
    {
        TComTrQuant quantiser;
        int t, scan;
        while (fscanf(in, "%d %d", &t, &scan) == 2) {
            const int log2 = t == 4 ? 2 : t == 8 ? 3 : t == 16 ? 4 : 5, tt = t * t;
            std::vector<TCoeff> arrays[3];
            for (auto& a : arrays) {
                a.resize(tt);
                for (int i = 0; i < tt; i++) {
                    int v;
                    if (fscanf(in, "%d", &v) != 1) return 3;
                    a[i] = v;
                }
            }
            TUEntropyCodingParameters cp;
            cp.scanType = COEFF_SCAN_TYPE(scan);
            cp.widthInGroups = cp.heightInGroups = t >> MLS_CG_LOG2_WIDTH;
            cp.scan = g_scanOrder[SCAN_GROUPED_4x4][scan][log2][log2];
            cp.scanCG = g_scanOrder[SCAN_UNGROUPED][scan][log2 - 2][log2 - 2];
            cp.firstSignificanceMapContext = 0;
            quantiser.signBitHidingHDQ(arrays[1].data(), arrays[0].data(), arrays[2].data(), cp, 15);
            for (int i = 0; i < tt; i++) printf(i ? " %d" : "%d", (int)arrays[1][i]);
            printf("\n");
        }
    }
    destroyROM();
    fclose(in);
    return 0;
}
