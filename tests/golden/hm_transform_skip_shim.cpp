// Shim of tests/golden/make_hm_transform_skip.py: HM-16.15's own coding of a 4 x 4 luma unit with transform_skip_flag 0 and 1, asked of
// the tree's own code compiled by path next to this file, the way tests/golden/hm_rdoq_shim.cpp asks it for RDOQ.  The world is that
// shim's with three differences: the PPS has transform skip on (so codeCoeffNxN codes the flag first); the quantiser is initialised per
// record with RDOQ and RDOQTS both off or both on; the unit is always the first 4 x 4 child of an 8 x 8 coding unit (transform depth 1,
// cbf context 0), and the coding unit's transform-skip flag is set per form.  A class derived from the quantiser reads the coefficients
// it keeps between xTransformSkip and xQuant.
// Reads records from the file named on the command line and prints one line of integers per record:
//   unit mode qp sdh rdoq lambda + 16 residual samples (lambda as the 64-bit pattern of a double)
//        -> scan, uiAbsSum and bits of the transformed form, uiAbsSum and bits of the skipped form (bits: the increase of m_fracBits over
//           codeCoeffNxN, 0 for a unit without a level, which HM never hands to it), 16 levels of the transformed form, 16 coefficients
//           of xTransformSkip, 16 levels of the skipped form, 16 samples of invTransformNxN of the skipped form
//   flag qp -> the increase of m_fracBits over codeTransformSkipFlags alone, for flag 0 and for flag 1
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
struct Quantiser : public TComTrQuant {                  // m_plTempCoeff is protected
    const TCoeff* kept() const { return m_plTempCoeff; }
};

static const int CTU = 64, TOTAL_DEPTH = 4, PARTS = 1 << (2 * TOTAL_DEPTH), T = 4;

struct World {
    TComSPS sps;
    TComPPS pps;
    TComPic pic;
    Quantiser quantiser;
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
        pps.setUseTransformSkip(true);
        pps.setTransquantBypassEnabledFlag(false);
        const Int range[MAX_NUM_CHANNEL_TYPE] = {15, 15};
        quantiser.init(32, false, false, false, true, true, false);
        quantiser.setFlatScalingList(range, sps.getBitDepths());
        quantiser.setUseScalingList(false);
        sbac.init(&counter);
        sbac.setBitstream(&bitCounter);
    }

    // the picture copies its parameter sets when it is created: made again whenever the sign-hiding flag changes
    TComDataCU* unit(int mode, int qp, int sdh)
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
        while ((CTU >> depth) > 2 * T) depth++;
        memset(cu->getDepth(), depth, PARTS);
        memset(cu->getWidth(), 2 * T, PARTS);
        memset(cu->getHeight(), 2 * T, PARTS);
        memset(cu->getPredictionMode(), MODE_INTRA, PARTS);
        memset(cu->getPartitionSize(), SIZE_NxN, PARTS);
        memset(cu->getTransformIdx(), 1, PARTS);
        memset(cu->getIntraDir(CHANNEL_TYPE_LUMA), mode, PARTS);
        memset(cu->getTransformSkip(COMPONENT_Y), 0, PARTS);
        memset(cu->getQP(), qp, PARTS);
        for (int i = 0; i < PARTS; i++) cu->getCUTransquantBypass()[i] = false;
        return cu;
    }

    void estimate(TComTU& tu, int scan)
    {
        sbac.resetEntropy(tu.getCU()->getSlice());
        memset(quantiser.m_pcEstBitsSbac, 0xff, sizeof(estBitsSbacStruct));
        sbac.estBit(quantiser.m_pcEstBitsSbac, T, T, CHANNEL_TYPE_LUMA, COEFF_SCAN_TYPE(scan));
    }

    long long bits(TComTU& tu, TCoeff* levels)
    {
        sbac.resetEntropy(tu.getCU()->getSlice());
        const UInt64 before = counter.fracBits();
        sbac.codeCoeffNxN(tu, levels, COMPONENT_Y);
        return (long long)(counter.fracBits() - before);
    }

    long long flag_bits(TComTU& tu)
    {
        sbac.resetEntropy(tu.getCU()->getSlice());
        const UInt64 before = counter.fracBits();
        sbac.codeTransformSkipFlags(tu, COMPONENT_Y);
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
                int mode, qp, sdh, rdoq;
                unsigned long long pattern;
                if (fscanf(in, "%d %d %d %d %llu", &mode, &qp, &sdh, &rdoq, &pattern) != 5) return 3;
                std::vector<int> given(T * T);
                if (!read_ints(in, given)) return 3;
                double lambda;
                memcpy(&lambda, &pattern, 8);
                TComDataCU* cu = world.unit(mode, qp, sdh);
                if (!cu->getSlice()->getPPS()->getUseTransformSkip()) return 4;
                if (cu->getSlice()->getPPS()->getPpsRangeExtension().getLog2MaxTransformSkipBlockSize() != 2) return 4;
                TComTURecurse root(cu, 0);
                TComTURecurse tu(root, false);
                if ((int)tu.getRect(COMPONENT_Y).width != T || (int)tu.getRect(COMPONENT_Y).height != T) return 4;
                if ((int)tu.GetTransformDepthRel() != 1 || cu->getCtxQtCbf(tu, CHANNEL_TYPE_LUMA) != 0) return 4;
                TUEntropyCodingParameters cp;
                getTUEntropyCodingParameters(cp, tu, COMPONENT_Y);
                const QpParam qpParam(*cu, COMPONENT_Y);
                if (qpParam.Qp != qp) return 4;
                world.quantiser.init(32, rdoq != 0, rdoq != 0, false, true, true, false);     // RDOQTS equals RDOQ
                const Double lambdas[MAX_NUM_COMPONENT] = {lambda, lambda, lambda};
                world.quantiser.setLambdas(lambdas);
                world.quantiser.selectLambda(COMPONENT_Y);
                std::vector<TCoeff> levels[2], arl(T * T), kept(T * T);
                std::vector<Pel> residual(T * T), back(T * T);
                TCoeff absSum[2] = {0, 0};
                long long bits[2] = {0, 0};
                for (int form = 0; form < 2; form++) {
                    levels[form].assign(T * T, 0);
                    for (int i = 0; i < T * T; i++) residual[i] = (Pel)given[i];       // (transformNxN may write its input)
                    memset(cu->getTransformSkip(COMPONENT_Y), form, PARTS);
                    world.estimate(tu, (int)cp.scanType);
                    world.quantiser.transformNxN(tu, COMPONENT_Y, residual.data(), T, levels[form].data(), arl.data(), absSum[form], qpParam);
                    if (form)
                        for (int i = 0; i < T * T; i++) kept[i] = world.quantiser.kept()[i];
                    bool any = false;
                    for (TCoeff v : levels[form]) any = any || v != 0;
                    bits[form] = any ? world.bits(tu, levels[form].data()) : 0LL;
                }
                world.quantiser.invTransformNxN(tu, COMPONENT_Y, back.data(), T, levels[1].data(), qpParam);
                printf("%d %d %lld %d %lld", (int)cp.scanType, (int)absSum[0], bits[0], (int)absSum[1], bits[1]);
                for (TCoeff v : levels[0]) printf(" %d", (int)v);
                for (TCoeff v : kept) printf(" %d", (int)v);
                for (TCoeff v : levels[1]) printf(" %d", (int)v);
                for (Pel v : back) printf(" %d", (int)v);
                printf("\n");
            } else if (!strcmp(word, "flag")) {
                int qp;
                if (fscanf(in, "%d", &qp) != 1) return 3;
                TComDataCU* cu = world.unit(0, qp, 0);
                TComTURecurse root(cu, 0);
                TComTURecurse tu(root, false);
                long long bits[2];
                for (int form = 0; form < 2; form++) {
                    memset(cu->getTransformSkip(COMPONENT_Y), form, PARTS);
                    bits[form] = world.flag_bits(tu);
                }
                printf("%lld %lld\n", bits[0], bits[1]);
            } else
                return 3;
        }
    }
    destroyROM();
    fclose(in);
    return 0;
}
