// Shim of tests/golden/make_hm_context_masks.py: which above-right and below-left neighbours HM-16.15 itself says a block has, asked of
// the tree's own isAboveRightAvailable / isBelowLeftAvailable (TComPattern.cpp) compiled by path next to this file, the way
// tests/golden/hm_cu_tree_picture_shim.cpp asks the tree about CTU boundaries.  The world is that shim's: a 128 x 128 picture of 2 x 2
// CTUs of 64 in one slice and one tile, 4:0:0, I slice, constrained intra prediction off (the PPS's default).  For every CTU, every one
// of the five widths and every aligned block of that width the two functions are called with the block's LT / RT / LB partitions as
// TComPrediction::initIntraPatternChType forms them, and one line of integers is printed, numbers only; nothing of the tree is shipped:
//   blk ctu width z x y  above_right_count below_left_count  n above-right flags (left to right)  n below-left flags (top to bottom)
// z: the block's z-order index among the CTU's blocks of its width; (x, y): its first 4 x 4 unit in the CTU; n = width / 4; the counts
// are the functions' return values, the flags what they wrote.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "TLibCommon/CommonDef.h"
#include "TLibCommon/TComDataCU.h"
#include "TLibCommon/TComPic.h"
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComSlice.h"

// defined in TComPattern.cpp, which declares them for itself alone
Int isAboveRightAvailable(const TComDataCU* pcCU, UInt uiPartIdxLT, UInt uiPartIdxRT, Bool* bValidFlags);
Int isBelowLeftAvailable(const TComDataCU* pcCU, UInt uiPartIdxLT, UInt uiPartIdxLB, Bool* bValidFlags);

static const int CTU = 64, SIDE = 128, TOTAL_DEPTH = 4, PARTS = 1 << (2 * TOTAL_DEPTH), CTUS = 4, UNITS = 16;

int main()
{
    initROM();
    {
        // the partition address tables the neighbour functions read: filled by TEncCu::create in the encoder
        UInt* cursor = &g_auiZscanToRaster[0];
        initZscanToRaster(TOTAL_DEPTH + 1, 1, 0, cursor);
        initRasterToZscan(CTU, CTU, TOTAL_DEPTH + 1);
        initRasterToPelXY(CTU, CTU, TOTAL_DEPTH + 1);
    }
    {
        TComSPS sps;
        TComPPS pps;
        TComPic pic;
        sps.setChromaFormatIdc(CHROMA_400);
        sps.setPicWidthInLumaSamples(SIDE);
        sps.setPicHeightInLumaSamples(SIDE);
        sps.setMaxCUWidth(CTU);
        sps.setMaxCUHeight(CTU);
        sps.setMaxTotalCUDepth(TOTAL_DEPTH);
        sps.setLog2MinCodingBlockSize(3);
        sps.setLog2DiffMaxMinCodingBlockSize(3);
        sps.setQuadtreeTULog2MaxSize(5);
        sps.setQuadtreeTULog2MinSize(2);
        sps.setMaxTrSize(32);
        for (int ch = 0; ch < MAX_NUM_CHANNEL_TYPE; ch++) {
            sps.setBitDepth(ChannelType(ch), 8);
            sps.setQpBDOffset(ChannelType(ch), 0);
        }
        pps.setTransquantBypassEnabledFlag(false);
        if (pps.getConstrainedIntraPred()) return 6;
        pic.create(sps, pps, false, true);
        if ((int)pic.getNumberOfCtusInFrame() != CTUS || (int)pic.getFrameWidthInCtus() != 2 || (int)pic.getNumPartInCtuWidth() != UNITS) return 5;
        TComSlice* slice = pic.getSlice(0);
        slice->setSPS(&pic.getPicSym()->getSPS());
        slice->setPPS(&pic.getPicSym()->getPPS());
        slice->setPic(&pic);
        slice->setSliceType(I_SLICE);
        slice->setSliceQp(32);
        for (int c = 0; c < CTUS; c++) {
            TComDataCU* cu = pic.getCtu(c);
            cu->initCtu(&pic, c);
            memset(cu->getPredictionMode(), MODE_INTRA, PARTS);
            memset(cu->getPartitionSize(), SIZE_2Nx2N, PARTS);
        }
        for (int c = 0; c < CTUS; c++) {
            const TComDataCU* cu = pic.getCtu(c);
            for (int width = 4; width <= CTU; width *= 2) {
                const int n = width / 4, side = CTU / width;
                for (int z = 0; z < side * side; z++) {
                    const UInt lt = (UInt)z * (UInt)(n * n);                     // the block's first partition in z-order
                    const UInt raster = g_auiZscanToRaster[lt];
                    const UInt rt = g_auiRasterToZscan[raster + n - 1];
                    const UInt lb = g_auiRasterToZscan[raster + (n - 1) * UNITS];
                    Bool above_right[UNITS], below_left[UNITS];
                    memset(above_right, 0, sizeof above_right);
                    memset(below_left, 0, sizeof below_left);
                    const Int count_ar = isAboveRightAvailable(cu, lt, rt, above_right);
                    const Int count_bl = isBelowLeftAvailable(cu, lt, lb, below_left + n - 1);   // written downwards from the given flag
                    printf("blk %d %d %d %u %u  %d %d ", c, width, z, raster % UNITS, raster / UNITS, count_ar, count_bl);
                    for (int i = 0; i < n; i++) printf(" %d", above_right[i] ? 1 : 0);
                    printf(" ");
                    for (int i = 0; i < n; i++) printf(" %d", below_left[n - 1 - i] ? 1 : 0);
                    printf("\n");
                }
            }
        }
    }
    destroyROM();
    return 0;
}
