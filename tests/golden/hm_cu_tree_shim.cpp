// Shim of tests/golden/make_hm_cu_tree.py: what HM-16.15's own TEncSbac::codeSplitFlag and codePartSize add to a TEncBinCABACCounter, and
// what TComDataCU::getCtxSplitFlag answers, asked of the tree's own code compiled by path next to this file, the way
// tests/golden/hm_transform_skip_shim.cpp asks it for transform skip.  The world is one 64 x 64 CTU of a 4:0:0 I slice, minimum CU 8.
// A CU WITH neighbours can be constructed here: inside the CTU getPULeft / getPUAbove answer from the CTU's own depth array, so the four
// 32 x 32 nodes of depth 1 give every combination of an absent (outside the one-CTU picture), shallower, equal and deeper neighbour.
// Prints lines of integers, numbers only; built and run by the generator, nothing of it is shipped:
//   ctx   left above value          left / above: 0 absent, 1 shallower, 2 equal, 3 deeper; value = getCtxSplitFlag
//   split qp context flag bits      bits = the increase of m_fracBits over codeSplitFlag from the slice's initial states
//   part  qp flag bits              flag 1 = SIZE_2Nx2N, 0 = SIZE_NxN, an intra CU of the minimum size; likewise over codePartSize
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "TLibCommon/CommonDef.h"
#include "TLibCommon/TComBitCounter.h"
#include "TLibCommon/TComDataCU.h"
#include "TLibCommon/TComPic.h"
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComSlice.h"
#include "TLibEncoder/TEncBinCoderCABACCounter.h"
#include "TLibEncoder/TEncSbac.h"

struct Counter : public TEncBinCABACCounter {            // m_fracBits is protected
    UInt64 fracBits() const { return m_fracBits; }
};

static const int CTU = 64, TOTAL_DEPTH = 4, PARTS = 1 << (2 * TOTAL_DEPTH), QUARTER = PARTS / 4;

struct World {
    TComSPS sps;
    TComPPS pps;
    TComPic pic;
    TEncSbac sbac;
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
        pps.setTransquantBypassEnabledFlag(false);
        pic.create(sps, pps, false, true);
        sbac.init(&counter);
        sbac.setBitstream(&bitCounter);
    }

    TComDataCU* ctu(int qp)
    {
        TComSlice* slice = pic.getSlice(0);
        slice->setSPS(&pic.getPicSym()->getSPS());
        slice->setPPS(&pic.getPicSym()->getPPS());
        slice->setPic(&pic);
        slice->setSliceType(I_SLICE);
        slice->setSliceQp(qp);
        TComDataCU* cu = pic.getCtu(0);
        cu->initCtu(&pic, 0);
        memset(cu->getPredictionMode(), MODE_INTRA, PARTS);
        memset(cu->getPartitionSize(), SIZE_2Nx2N, PARTS);
        memset(cu->getQP(), qp, PARTS);
        return cu;
    }

    // the four 32 x 32 quarters of the CTU at the given depths (z-order: 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right)
    static void quarters(TComDataCU* cu, const int depth[4])
    {
        for (int k = 0; k < 4; k++) {
            memset(cu->getDepth() + k * QUARTER, depth[k], QUARTER);
            memset(cu->getWidth() + k * QUARTER, CTU >> depth[k], QUARTER);
            memset(cu->getHeight() + k * QUARTER, CTU >> depth[k], QUARTER);
        }
    }
};

// state of a neighbour of a depth-1 node -> its depth: 1 shallower, 2 equal, 3 deeper
static int depth_of(int state) { return state - 1; }

// The depth-1 node whose left / above neighbours are absent or present as asked, with the quarters set accordingly; `own` is the node's
// own depth (1: split_cu_flag 0 at depth 1, 2: flag 1)
static int place(TComDataCU* cu, int left, int above, int own)
{
    const int node = (left ? 1 : 0) + (above ? 2 : 0);
    int depth[4] = {1, 1, 1, 1};
    if (left) depth[node - 1] = depth_of(left);
    if (above) depth[node - 2] = depth_of(above);
    depth[node] = own;
    World::quarters(cu, depth);
    return node * QUARTER;
}

int main()
{
    initROM();
    ContextModel::buildNextStateTable();
    {
        // the partition address tables getPULeft / getPUAbove read: filled by TEncCu::create in the encoder
        UInt* cursor = &g_auiZscanToRaster[0];
        initZscanToRaster(TOTAL_DEPTH + 1, 1, 0, cursor);
        initRasterToZscan(CTU, CTU, TOTAL_DEPTH + 1);
        initRasterToPelXY(CTU, CTU, TOTAL_DEPTH + 1);
    }
    {
        World world;
        for (int left = 0; left < 4; left++)
            for (int above = 0; above < 4; above++) {
                TComDataCU* cu = world.ctu(32);
                const int part = place(cu, left, above, 1);
                printf("ctx %d %d %u\n", left, above, cu->getCtxSplitFlag(part, 1));
            }
        for (int qp = 0; qp <= 51; qp++) {
            // context 0: no neighbour; 1: a deeper left neighbour, none above; 2: both deeper
            const int lefts[3] = {0, 3, 3}, aboves[3] = {0, 0, 3};
            for (int ctx = 0; ctx < 3; ctx++)
                for (int flag = 0; flag < 2; flag++) {
                    TComDataCU* cu = world.ctu(qp);
                    const int part = place(cu, lefts[ctx], aboves[ctx], 1 + flag);
                    if ((int)cu->getCtxSplitFlag(part, 1) != ctx) return 4;
                    world.sbac.resetEntropy(cu->getSlice());
                    const UInt64 before = world.counter.fracBits();
                    world.sbac.codeSplitFlag(cu, part, 1);
                    printf("split %d %d %d %lld\n", qp, ctx, flag, (long long)(world.counter.fracBits() - before));
                }
            for (int flag = 0; flag < 2; flag++) {
                TComDataCU* cu = world.ctu(qp);
                memset(cu->getDepth(), 3, PARTS);
                memset(cu->getWidth(), 8, PARTS);
                memset(cu->getHeight(), 8, PARTS);
                memset(cu->getPartitionSize(), flag ? SIZE_2Nx2N : SIZE_NxN, PARTS);
                world.sbac.resetEntropy(cu->getSlice());
                const UInt64 before = world.counter.fracBits();
                world.sbac.codePartSize(cu, 0, 3);
                printf("part %d %d %lld\n", qp, flag, (long long)(world.counter.fracBits() - before));
            }
            // at the minimum CU size codeSplitFlag codes nothing
            TComDataCU* cu = world.ctu(qp);
            memset(cu->getDepth(), 3, PARTS);
            world.sbac.resetEntropy(cu->getSlice());
            const UInt64 before = world.counter.fracBits();
            world.sbac.codeSplitFlag(cu, 0, 3);
            if (world.counter.fracBits() != before) return 5;
        }
    }
    destroyROM();
    return 0;
}
