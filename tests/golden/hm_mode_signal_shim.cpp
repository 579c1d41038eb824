// Shim of tests/golden/make_hm_mode_signal.py: the side information of an intra luma prediction unit asked of an HM-16.15 tree's own
// code (TLibCommon, TEncSbac.cpp, TEncBinCoderCABAC*.cpp, TEncEntropy.cpp and the tree's headers, compiled by path next to this file).
// The one-CTU picture of hm_unit_coding_shim.cpp: one TComSPS / TComPPS, a TComPic of one 64 x 64 CTU, its slice and TComDataCU, 4:0:0,
// 8 bit, I slice, SliceQp = the case's QP.  The CTU is cut into 8 x 8 coding units (depth 3, 2N x 2N, intra); the unit asked about lies
// at (8, 8), (0, 8), (8, 0) or (0, 0), so that its left and / or above neighbour is inside the CTU or does not exist; a neighbour inside
// is intra with the given mode or, on request, not intra.
// Reads records from the file named on the command line and prints one line of integers per record:
//   mpm left above           ->  uiIntraDirPred[0 .. 2] and *piMode of TComDataCU::getIntraDirPredictor
//   bits left above qp modes ->  per mode 0 .. modes - 1 the increase of TEncBinCABACCounter's m_fracBits over ONE
//                                TEncEntropy::encodeIntraDirModeLuma right after resetEntropy
//   cbf qp                   ->  the increase over one TEncSbac::codeQtCbf for luma: transform depth 0 value 0, 1; depth 1 value 0, 1
// left / above: 0 .. 35 the neighbour's coded mode, 254 a neighbour that is not intra, 255 no neighbour.
// Numbers only; built and run by the generator, nothing of it is shipped.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "TLibCommon/CommonDef.h"
#include "TLibCommon/TComBitCounter.h"
#include "TLibCommon/TComChromaFormat.h"
#include "TLibCommon/TComDataCU.h"
#include "TLibCommon/TComPic.h"
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComSlice.h"
#include "TLibCommon/TComTU.h"
#include "TLibEncoder/TEncBinCoderCABACCounter.h"
#include "TLibEncoder/TEncEntropy.h"
#include "TLibEncoder/TEncSbac.h"

struct Counter : public TEncBinCABACCounter {            // m_fracBits is protected
    UInt64 fracBits() const { return m_fracBits; }
};

static const int CTU = 64, TOTAL_DEPTH = 4, PARTS = 1 << (2 * TOTAL_DEPTH), NONE = 255, NOT_INTRA = 254;

struct World {
    TComSPS sps;
    TComPPS pps;
    TComPic pic;
    TEncSbac sbac;
    TEncEntropy entropy;
    Counter counter;
    TComBitCounter bitCounter;

    World()
    {
        sps.setChromaFormatIdc(CHROMA_400);
        sps.setPicWidthInLumaSamples(CTU);
        sps.setPicHeightInLumaSamples(CTU);
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
        pps.setUseTransformSkip(false);
        pps.setTransquantBypassEnabledFlag(false);
        pic.create(sps, pps, false, true);
        sbac.init(&counter);
        sbac.setBitstream(&bitCounter);
        entropy.setEntropyCoder(&sbac);
    }

    // the CTU as 8 x 8 (or `size`) intra coding units of mode DC; returns it
    TComDataCU* ctu(int qp, int size = 8)
    {
        TComSlice* slice = pic.getSlice(0);
        slice->setSPS(&pic.getPicSym()->getSPS());
        slice->setPPS(&pic.getPicSym()->getPPS());
        slice->setPic(&pic);
        slice->setSliceType(I_SLICE);
        slice->setSliceQp(qp);
        TComDataCU* cu = pic.getCtu(0);
        cu->initCtu(&pic, 0);
        int depth = 0;
        while ((CTU >> depth) > size) depth++;
        memset(cu->getDepth(), depth, PARTS);
        memset(cu->getWidth(), size, PARTS);
        memset(cu->getHeight(), size, PARTS);
        memset(cu->getPredictionMode(), MODE_INTRA, PARTS);
        memset(cu->getPartitionSize(), SIZE_2Nx2N, PARTS);
        memset(cu->getTransformIdx(), 0, PARTS);
        memset(cu->getIntraDir(CHANNEL_TYPE_LUMA), DC_IDX, PARTS);
        memset(cu->getTransformSkip(COMPONENT_Y), 0, PARTS);
        memset(cu->getQP(), qp, PARTS);
        for (int i = 0; i < PARTS; i++) cu->getCUTransquantBypass()[i] = false;
        return cu;
    }

    // the partition index of the unit whose neighbours are as asked; the neighbours' arrays set
    UInt place(TComDataCU* cu, int left, int above)
    {
        const int x = left == NONE ? 0 : 2, y = above == NONE ? 0 : 2;          // in 4 x 4 partitions
        const UInt at = g_auiRasterToZscan[y * 16 + x];
        if (left != NONE) neighbour(cu, g_auiRasterToZscan[y * 16 + x - 1], left);
        if (above != NONE) neighbour(cu, g_auiRasterToZscan[(y - 1) * 16 + x], above);
        return at;
    }
    void neighbour(TComDataCU* cu, UInt at, int mode)
    {
        if (mode == NOT_INTRA) cu->getPredictionMode()[at] = MODE_INTER;
        else cu->getIntraDir(CHANNEL_TYPE_LUMA)[at] = (UChar)mode;
    }
};

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    initROM();
    ContextModel::buildNextStateTable();
    {
        UInt* order = &g_auiZscanToRaster[0];              // the partition orders, as TEncCu::create sets them up
        initZscanToRaster(TOTAL_DEPTH + 1, 1, 0, order);
        initRasterToZscan(CTU, CTU, TOTAL_DEPTH + 1);
        initRasterToPelXY(CTU, CTU, TOTAL_DEPTH + 1);
    }
    {
        World world;
        char word[16];
        while (fscanf(in, "%15s", word) == 1) {
            if (!strcmp(word, "mpm")) {
                int left, above;
                if (fscanf(in, "%d %d", &left, &above) != 2) return 3;
                TComDataCU* cu = world.ctu(30);
                const UInt at = world.place(cu, left, above);
                Int preds[NUM_MOST_PROBABLE_MODES] = {-1, -1, -1}, mode = -1;
                cu->getIntraDirPredictor(at, preds, COMPONENT_Y, &mode);
                printf("%d %d %d %d\n", preds[0], preds[1], preds[2], mode);
            } else if (!strcmp(word, "bits")) {
                int left, above, qp, modes;
                if (fscanf(in, "%d %d %d %d", &left, &above, &qp, &modes) != 4) return 3;
                for (int m = 0; m < modes; m++) {
                    TComDataCU* cu = world.ctu(qp);
                    const UInt at = world.place(cu, left, above);
                    cu->getIntraDir(CHANNEL_TYPE_LUMA)[at] = (UChar)m;
                    world.sbac.resetEntropy(cu->getSlice());
                    const UInt64 before = world.counter.fracBits();
                    world.entropy.encodeIntraDirModeLuma(cu, at);
                    printf(m ? " %lld" : "%lld", (long long)(world.counter.fracBits() - before));
                }
                printf("\n");
            } else if (!strcmp(word, "cbf")) {
                int qp;
                if (fscanf(in, "%d", &qp) != 1) return 3;
                for (int depth = 0; depth < 2; depth++)
                    for (int value = 0; value < 2; value++) {
                        TComDataCU* cu = world.ctu(qp, 16);
                        memset(cu->getCbf(COMPONENT_Y), value ? 0xff : 0, PARTS);
                        TComTURecurse root(cu, 0);
                        TComTURecurse child(root, false);
                        TComTU& tu = depth ? (TComTU&)child : (TComTU&)root;
                        if ((int)tu.GetTransformDepthRel() != depth) return 4;
                        world.sbac.resetEntropy(cu->getSlice());
                        const UInt64 before = world.counter.fracBits();
                        world.sbac.codeQtCbf(tu, COMPONENT_Y, true);
                        printf(depth + value ? " %lld" : "%lld", (long long)(world.counter.fracBits() - before));
                    }
                printf("\n");
            } else
                return 3;
        }
    }
    destroyROM();
    fclose(in);
    return 0;
}
