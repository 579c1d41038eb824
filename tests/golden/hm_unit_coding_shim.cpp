// Shim of tests/golden/make_hm_unit_coding.py: HM-16.15's own coding of WHOLE transform units, asked of the tree's own code (TLibCommon,
// TEncSbac.cpp, TEncBinCoderCABAC*.cpp, TEncEntropy.cpp and the tree's headers, compiled by path next to this file).  What the earlier
// shims declined to stand up is stood up here: one TComSPS / TComPPS, a TComPic of one 64 x 64 CTU (TComPic::create, so that the
// picture symbol, its slice and its TComDataCU exist) and, per case, TComDataCU::initCtu and the per-partition arrays of ONE intra luma
// coding unit at depth log2(64 / T) with ONE transform unit of T x T (TComTURecurse).  At T = 4 that unit is what HM reaches as the
// first quarter of an 8 x 8 NxN coding unit; the functions asked read the unit's width, depth, prediction mode, intra direction and
// transform-skip / bypass arrays, all of which are set for every partition.
// Settings: 4:0:0, 8 bit, I slice, SliceQp = the case's QP, maxLog2TrDynamicRange 15, RDOQ 0, flat quantisation (no scaling list), no
// transform skip, transquant bypass, range extension tool or CABAC bypass alignment; SignDataHidingEnabledFlag per case.
// Reads records from the file named on the command line and prints one line of integers per record:
//   unit T mode qp sdh + T * T residual samples   ->  scan uiAbsSum bits, T * T levels, T * T reconstructed residual samples
//        TComTrQuant::transformNxN, getTUEntropyCodingParameters' scanType, the increase of TEncBinCABACCounter's m_fracBits over one
//        TEncSbac::codeCoeffNxN right after resetEntropy (0 without a call when every level is zero), TComTrQuant::invTransformNxN
//   code T mode qp sdh + T * T levels             ->  scan bits      (codeCoeffNxN on the given levels)
//   scans                                         ->  4 * 35 scan types: TComDataCU::getCoefScanIdx per T in {4, 8, 16, 32} and mode 0 .. 34
//   cost lambda D R (lambda as the 64-bit pattern of a double)  ->  the pattern of TComRdCost::calcRdCost(R, D, DF_DEFAULT) after setLambda
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
        quantiser.init(32, false, false, false, true, false, false);    // RDOQ, RDOQ-TS, selective RDOQ off; encoder; no adaptive QP selection
        const Int range[MAX_NUM_CHANNEL_TYPE] = {15, 15};
        quantiser.setFlatScalingList(range, sps.getBitDepths());
        quantiser.setUseScalingList(false);
        sbac.init(&counter);
        sbac.setBitstream(&bitCounter);
    }

    // the picture copies its parameter sets when it is created: made again whenever the sign-hiding flag changes
    TComDataCU* unit(int t, int mode, int qp, int sdh)
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
        while ((CTU >> depth) > t) depth++;
        memset(cu->getDepth(), depth, PARTS);
        memset(cu->getWidth(), t, PARTS);
        memset(cu->getHeight(), t, PARTS);
        memset(cu->getPredictionMode(), MODE_INTRA, PARTS);
        memset(cu->getPartitionSize(), SIZE_2Nx2N, PARTS);
        memset(cu->getTransformIdx(), 0, PARTS);
        memset(cu->getIntraDir(CHANNEL_TYPE_LUMA), mode, PARTS);
        memset(cu->getTransformSkip(COMPONENT_Y), 0, PARTS);
        memset(cu->getQP(), qp, PARTS);
        for (int i = 0; i < PARTS; i++) cu->getCUTransquantBypass()[i] = false;
        return cu;
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
            if (!strcmp(word, "unit") || !strcmp(word, "code")) {
                int t, mode, qp, sdh;
                if (fscanf(in, "%d %d %d %d", &t, &mode, &qp, &sdh) != 4) return 3;
                if (t != 4 && t != 8 && t != 16 && t != 32) return 3;
                std::vector<int> given(t * t);
                if (!read_ints(in, given)) return 3;
                TComDataCU* cu = world.unit(t, mode, qp, sdh);
                TComTURecurse tu(cu, 0);
                if ((int)tu.getRect(COMPONENT_Y).width != t || (int)tu.getRect(COMPONENT_Y).height != t) return 4;
                TUEntropyCodingParameters cp;
                getTUEntropyCodingParameters(cp, tu, COMPONENT_Y);
                std::vector<TCoeff> levels(t * t), arl(t * t);
                if (word[0] == 'c') {
                    for (int i = 0; i < t * t; i++) levels[i] = given[i];
                    printf("%d %lld\n", (int)cp.scanType, world.bits(tu, levels.data()));
                    continue;
                }
                std::vector<Pel> residual(t * t), back(t * t);
                for (int i = 0; i < t * t; i++) residual[i] = (Pel)given[i];
                const QpParam qpParam(*cu, COMPONENT_Y);
                if (qpParam.Qp != qp) return 4;
                TCoeff absSum = 0;
                world.quantiser.transformNxN(tu, COMPONENT_Y, residual.data(), t, levels.data(), arl.data(), absSum, qpParam);
                bool any = false;
                for (TCoeff v : levels) any = any || v != 0;
                printf("%d %d %lld", (int)cp.scanType, (int)absSum, any ? world.bits(tu, levels.data()) : 0LL);
                for (TCoeff v : levels) printf(" %d", (int)v);
                world.quantiser.invTransformNxN(tu, COMPONENT_Y, back.data(), t, levels.data(), qpParam);
                for (Pel v : back) printf(" %d", (int)v);
                printf("\n");
            } else if (!strcmp(word, "scans")) {
                for (int t = 4; t <= 32; t *= 2)
                    for (int mode = 0; mode < 35; mode++) {
                        TComDataCU* cu = world.unit(t, mode, 22, 0);
                        printf(t == 4 && mode == 0 ? "%d" : " %d", (int)cu->getCoefScanIdx(0, t, t, COMPONENT_Y));
                    }
                printf("\n");
            } else if (!strcmp(word, "cost")) {
                unsigned long long pattern, d, r;
                if (fscanf(in, "%llu %llu %llu", &pattern, &d, &r) != 3) return 3;
                double lambda, cost;
                memcpy(&lambda, &pattern, 8);
                TComRdCost rd;
                rd.setCostMode(COST_STANDARD_LOSSY);
                rd.setLambda(lambda, world.sps.getBitDepths());
                cost = rd.calcRdCost((Double)r, (Double)d, DF_DEFAULT);
                memcpy(&pattern, &cost, 8);
                printf("%llu\n", pattern);
            } else
                return 3;
        }
    }
    destroyROM();
    fclose(in);
    return 0;
}
