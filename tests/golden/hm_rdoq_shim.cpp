// Shim of tests/golden/make_hm_rdoq.py: HM-16.15's own quantiser with RDOQ ON (TComTrQuant::xRateDistOptQuant behind transformNxN), asked
// of the tree's own code compiled by path next to this file, the way tests/golden/hm_unit_coding_shim.cpp asks it with RDOQ 0.  The
// world differs from that shim's in four ways: quantiser.init(32, true, ...); quantiser.setLambdas / selectLambda(luma) per case; before every
// transformNxN, resetEntropy of the slice and TEncSbac::estBit into the quantiser's m_pcEstBitsSbac (what TEncSearch does through
// TEncEntropy::estimateBit); and, beside the unit at transform depth 0, a unit at transform depth 1 -- a coding unit of 2T with
// transform index 1, the first child of its TComTURecurse -- for which getCtxQtCbf returns 0.
// Reads records from the file named on the command line and prints one line of integers per record:
//   unit T mode qp sdh depth lambda + T * T residual samples (lambda as the 64-bit pattern of a double)
//        -> scan uiAbsSum bits cbf_ctx, T * T levels, T * T reconstructed residual samples
//   est T qp scan -> 184 integers: the tables estBit filled, in the layout of pnn_rdoq_est_bits_host, -1 where HM fills nothing
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
#include "TLibCommon/TComRdCost.h"
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComSlice.h"
#include "TLibCommon/TComTU.h"
#include "TLibCommon/TComTrQuant.h"
#include "TLibEncoder/TEncBinCoderCABACCounter.h"
#include "TLibEncoder/TEncSbac.h"

struct Counter : public TEncBinCABACCounter {            // m_fracBits is protected
    UInt64 fracBits() const { return m_fracBits; }
};

static const int CTU = 64, TOTAL_DEPTH = 4, PARTS = 1 << (2 * TOTAL_DEPTH);

struct World {
    TComSPS sps;
    TComPPS pps;
    TComPic pic;
    TComTrQuant quantiser;
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
        pps.setUseTransformSkip(false);
        pps.setTransquantBypassEnabledFlag(false);
        quantiser.init(32, true, false, false, true, false, false);     // RDOQ on; RDOQ-TS, selective RDOQ off; encoder; no adaptive QP selection
        const Int range[MAX_NUM_CHANNEL_TYPE] = {15, 15};
        quantiser.setFlatScalingList(range, sps.getBitDepths());
        quantiser.setUseScalingList(false);
        sbac.init(&counter);
        sbac.setBitstream(&bitCounter);
    }

    // the picture copies its parameter sets when it is created: made again whenever the sign-hiding flag changes
    // depth 0: a coding unit of t with one transform unit; depth 1: a coding unit of 2 t split once
    TComDataCU* unit(int t, int mode, int qp, int sdh, int tr_depth = 0)
    {
        if (!created || sdh != flag) {
            pps.setSignDataHidingEnabledFlag(sdh != 0);
            pic.create(sps, pps, false, true);
            created = true;
            flag = sdh;
        }
        TComSlice* slice = pic.getSlice(0);
        slice->setSPS(&pic.getPicSym()->getSPS());
        slice->setPPS(&pic.getPicSym()->getPPS());
        slice->setPic(&pic);
        slice->setSliceType(I_SLICE);
        slice->setSliceQp(qp);
        TComDataCU* cu = pic.getCtu(0);
        cu->initCtu(&pic, 0);
        int depth = 0;
        while ((CTU >> depth) > (t << tr_depth)) depth++;
        memset(cu->getDepth(), depth, PARTS);
        memset(cu->getWidth(), t << tr_depth, PARTS);
        memset(cu->getHeight(), t << tr_depth, PARTS);
        memset(cu->getPredictionMode(), MODE_INTRA, PARTS);
        memset(cu->getPartitionSize(), SIZE_2Nx2N, PARTS);
        memset(cu->getTransformIdx(), tr_depth, PARTS);
        memset(cu->getIntraDir(CHANNEL_TYPE_LUMA), mode, PARTS);
        memset(cu->getTransformSkip(COMPONENT_Y), 0, PARTS);
        memset(cu->getQP(), qp, PARTS);
        for (int i = 0; i < PARTS; i++) cu->getCUTransquantBypass()[i] = false;
        return cu;
    }

    void estimate(TComTU& tu, int t, int scan)
    {
        sbac.resetEntropy(tu.getCU()->getSlice());
        memset(quantiser.m_pcEstBitsSbac, 0xff, sizeof(estBitsSbacStruct));
        sbac.estBit(quantiser.m_pcEstBitsSbac, t, t, CHANNEL_TYPE_LUMA, COEFF_SCAN_TYPE(scan));
    }

    long long bits(TComTU& tu, TCoeff* levels)
    {
        sbac.resetEntropy(tu.getCU()->getSlice());
        const UInt64 before = counter.fracBits();
        sbac.codeCoeffNxN(tu, levels, COMPONENT_Y);
        return (long long)(counter.fracBits() - before);
    }

    bool created = false;
    int flag = -1;
};

static bool read_ints(FILE* in, std::vector<int>& v)
{
    for (int& x : v)
        if (fscanf(in, "%d", &x) != 1) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    initROM();
    ContextModel::buildNextStateTable();
    {
        World world;
        char word[16];
        while (fscanf(in, "%15s", word) == 1) {
            if (!strcmp(word, "unit")) {
                int t, mode, qp, sdh, depth;
                unsigned long long pattern;
                if (fscanf(in, "%d %d %d %d %d %llu", &t, &mode, &qp, &sdh, &depth, &pattern) != 6) return 3;
                if ((t != 4 && t != 8 && t != 16 && t != 32) || depth < 0 || depth > 1) return 3;
                std::vector<int> given(t * t);
                if (!read_ints(in, given)) return 3;
                double lambda;
                memcpy(&lambda, &pattern, 8);
                TComDataCU* cu = world.unit(t, mode, qp, sdh, depth);
                TComTURecurse root(cu, 0);
                TComTURecurse child(root, false);
                TComTU& tu = depth ? (TComTU&)child : (TComTU&)root;
                if ((int)tu.getRect(COMPONENT_Y).width != t || (int)tu.getRect(COMPONENT_Y).height != t) return 4;
                if ((int)tu.GetTransformDepthRel() != depth) return 4;
                TUEntropyCodingParameters cp;
                getTUEntropyCodingParameters(cp, tu, COMPONENT_Y);
                std::vector<TCoeff> levels(t * t), arl(t * t);
                std::vector<Pel> residual(t * t), back(t * t);
                for (int i = 0; i < t * t; i++) residual[i] = (Pel)given[i];
                const QpParam qpParam(*cu, COMPONENT_Y);
                if (qpParam.Qp != qp) return 4;
                const Double lambdas[MAX_NUM_COMPONENT] = {lambda, lambda, lambda};      // (RDOQ_CHROMA_LAMBDA: one per component, luma selected)
                world.quantiser.setLambdas(lambdas);
                world.quantiser.selectLambda(COMPONENT_Y);
                world.estimate(tu, t, (int)cp.scanType);
                TCoeff absSum = 0;
                world.quantiser.transformNxN(tu, COMPONENT_Y, residual.data(), t, levels.data(), arl.data(), absSum, qpParam);
                bool any = false;
                for (TCoeff v : levels) any = any || v != 0;
                printf("%d %d %lld %d", (int)cp.scanType, (int)absSum, any ? world.bits(tu, levels.data()) : 0LL,
                       (int)cu->getCtxQtCbf(tu, CHANNEL_TYPE_LUMA));
                for (TCoeff v : levels) printf(" %d", (int)v);
                world.quantiser.invTransformNxN(tu, COMPONENT_Y, back.data(), t, levels.data(), qpParam);
                for (Pel v : back) printf(" %d", (int)v);
                printf("\n");
            } else if (!strcmp(word, "est")) {
                int t, qp, scan;
                if (fscanf(in, "%d %d %d", &t, &qp, &scan) != 3) return 3;
                TComDataCU* cu = world.unit(t, 0, qp, 0);
                TComTURecurse tu(cu, 0);
                world.estimate(tu, t, scan);
                const estBitsSbacStruct& e = *world.quantiser.m_pcEstBitsSbac;
                for (int i = 0; i < 30; i++) printf("-1 -1 ");
                for (int i = 0; i < 2; i++) printf("%d %d ", e.significantCoeffGroupBits[i][0], e.significantCoeffGroupBits[i][1]);
                for (int i = 0; i < 28; i++) printf("%d %d ", e.significantBits[i][0], e.significantBits[i][1]);
                for (int i = 0; i < 16; i++) printf("%d %d ", e.m_greaterOneBits[i][0], e.m_greaterOneBits[i][1]);
                for (int i = 0; i < 4; i++) printf("%d %d ", e.m_levelAbsBits[i][0], e.m_levelAbsBits[i][1]);
                for (int i = 0; i < 10; i++) printf("%d ", e.lastXBits[CHANNEL_TYPE_LUMA][i]);
                for (int i = 0; i < 10; i++) printf("%d ", e.lastYBits[CHANNEL_TYPE_LUMA][i]);
                printf("%d %d %d %d\n", e.blockCbpBits[0][0], e.blockCbpBits[0][1], e.blockCbpBits[1][0], e.blockCbpBits[1][1]);
            } else
                return 3;
        }
    }
    destroyROM();
    fclose(in);
    return 0;
}
