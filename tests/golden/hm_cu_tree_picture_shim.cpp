// Shim of tests/golden/make_hm_cu_tree_picture.py: what HM-16.15's own TComDataCU::getCtxSplitFlag answers ACROSS the boundaries of
// CTUs, asked of the tree's own code compiled by path next to this file, the way tests/golden/hm_cu_tree_shim.cpp asks it inside one
// CTU.  The world is a 128 x 128 picture of 2 x 2 CTUs of 64 in one slice and one tile, 4:0:0, I slice, minimum CU 8; every CTU is
// given the depth map the generator wrote into the file named by argv[1]: 4 x 64 integers 0 .. 3, CTU by CTU in raster order, each
// CTU's 8 x 8 minimum-CU cells in z-order (a valid quadtree: the generator made it).  Then, for every CTU and every node of depth
// 0 .. 2 that touches the CTU's left or top edge, one line of integers, numbers only; nothing of the tree is shipped:
//   ctx ctu depth node value  left_state left_other  above_state above_other
// node: the node's z-order index among the nodes of its depth; value = getCtxSplitFlag(the node's first partition, depth);
// *_state: what getPULeft / getPUAbove with their default arguments answered for that partition -- 0 nothing (NULL), else the
// depth of the partition they named against the node's: 1 shallower, 2 equal, 3 deeper; *_other: 1 where the CU they returned is
// another CTU than the node's own.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "TLibCommon/CommonDef.h"
#include "TLibCommon/TComDataCU.h"
#include "TLibCommon/TComPic.h"
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComSlice.h"

static const int CTU = 64, SIDE = 128, TOTAL_DEPTH = 4, PARTS = 1 << (2 * TOTAL_DEPTH), CTUS = 4, CELLS = 64;

static int state_of(const TComDataCU* cu, UInt part, int depth)
{
    if (!cu) return 0;
    const int d = cu->getDepth(part);
    return d < depth ? 1 : d == depth ? 2 : 3;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    int maps[CTUS][CELLS];
    FILE* f = fopen(argv[1], "r");
    if (!f) return 3;
    for (int c = 0; c < CTUS; c++)
        for (int z = 0; z < CELLS; z++)
            if (fscanf(f, "%d", &maps[c][z]) != 1 || maps[c][z] < 0 || maps[c][z] > 3) return 4;
    fclose(f);

    initROM();
    {
        // the partition address tables getPULeft / getPUAbove read: filled by TEncCu::create in the encoder
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
        pic.create(sps, pps, false, true);
        if ((int)pic.getNumberOfCtusInFrame() != CTUS || (int)pic.getFrameWidthInCtus() != 2) return 5;
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
            for (int z = 0; z < CELLS; z++) {             // a minimum-CU cell is four 4 x 4 partitions, adjacent in z-order
                memset(cu->getDepth() + 4 * z, maps[c][z], 4);
                memset(cu->getWidth() + 4 * z, CTU >> maps[c][z], 4);
                memset(cu->getHeight() + 4 * z, CTU >> maps[c][z], 4);
            }
        }
        for (int c = 0; c < CTUS; c++) {
            TComDataCU* cu = pic.getCtu(c);
            for (int depth = 0; depth < 3; depth++)
                for (int node = 0; node < (1 << (2 * depth)); node++) {
                    const UInt part = (UInt)node * (PARTS >> (2 * depth));
                    const UInt raster = g_auiZscanToRaster[part];
                    if (raster % 16 != 0 && raster / 16 != 0) continue;       // neither on the left column nor on the top row
                    UInt left_part = 0, above_part = 0;
                    const TComDataCU* left = cu->getPULeft(left_part, part);
                    const TComDataCU* above = cu->getPUAbove(above_part, part);
                    printf("ctx %d %d %d %u  %d %d  %d %d\n", c, depth, node, cu->getCtxSplitFlag(part, depth), state_of(left, left_part, depth),
                           left && left->getCtuRsAddr() != (UInt)c ? 1 : 0, state_of(above, above_part, depth),
                           above && above->getCtuRsAddr() != (UInt)c ? 1 : 0);
                }
        }
    }
    destroyROM();
    return 0;
}
