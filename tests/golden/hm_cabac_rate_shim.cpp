// Shim of tests/golden/make_hm_cabac_rate.py: the pieces of HM-16.15's residual entropy coding that stand without a coding unit, asked
// of the tree's own code (ContextModel.cpp, TComTrQuant.cpp, TComRom.cpp and the tree's headers, compiled by path next to this file)
// and printed as lines `name count values...`:
//   init_values                      the I-slice rows of INIT_LAST (luma, for x and again for y), INIT_SIG_CG_FLAG, INIT_SIG_FLAG,
//                                    INIT_ONE_FLAG, INIT_ABS_FLAG (luma parts), 80 values in this project's context order
//   model_bins [80][K]               a bin sequence per context, made here (runs of 100 of either value, clean or noisy, so that every state is reached)
//   model_bits / model_states [qp][80][K]   ContextModel::init(qp, value), then per bin getEntropyBits(bin) and, after update(bin), the state
//   scan_T_s, group_scan_T_s         g_scanOrder, grouped 4 x 4 at T x T and ungrouped at T / 4 x T / 4, after initROM
//   sig_ctx_T_s [4][T * T]           TComTrQuant::getSigCtxInc per pattern and scan position
//   group_maps / group_ctx / group_pattern   4 x 4 maps of coded groups, getSigCoeffGroupCtxInc and calcPatternSigCtx at each group
//   last_group, last_params          g_uiGroupIdx; getLastSignificantContextParameters (offset, shift) per T
// Built and run by the generator only; nothing of it is shipped.
#include <cstdio>
#include <vector>

#include "TLibCommon/CommonDef.h"
#include "TLibCommon/ContextModel.h"
#include "TLibCommon/ContextTables.h"
#include "TLibCommon/TComChromaFormat.h"
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComTrQuant.h"

static void put(const char* name, const std::vector<long>& v)
{
    printf("%s %zu", name, v.size());
    for (long x : v) printf(" %ld", x);
    printf("\n");
}

int main()
{
    initROM();
    ContextModel::buildNextStateTable();
    const int I = 2;   // I_SLICE's row of the INIT_ tables
    std::vector<long> init;
    for (int rep = 0; rep < 2; rep++)
        for (int i = 0; i < NUM_CTX_LAST_FLAG_XY; i++) init.push_back(INIT_LAST[I][i]);
    for (int i = 0; i < NUM_SIG_CG_FLAG_CTX; i++) init.push_back(INIT_SIG_CG_FLAG[I][i]);
    for (int i = 0; i < NUM_SIG_FLAG_CTX_LUMA; i++) init.push_back(INIT_SIG_FLAG[I][i]);
    for (int i = 0; i < NUM_ONE_FLAG_CTX_LUMA; i++) init.push_back(INIT_ONE_FLAG[I][i]);
    for (int i = 0; i < NUM_ABS_FLAG_CTX_LUMA; i++) init.push_back(INIT_ABS_FLAG[I][i]);
    put("init_values", init);

    const int K = 200, qps[4] = {0, 22, 37, 51};
    std::vector<long> bins, bits, states;
    unsigned lcg = 12345u;
    for (size_t c = 0; c < init.size(); c++)
        for (int k = 0; k < K; k++) {
            lcg = lcg * 1664525u + 1013904223u;
            const unsigned r = (lcg >> 16) % 100;
            const int favoured = (k / 100 + (int)c) % 2;    // 100 bins towards one value, then 100 towards the other: long enough to fall
            const unsigned noise = c % 4 < 2 ? 0 : c % 4 == 2 ? 4 : 30;   // from any state to 0 and climb to 62; clean, 4 % and 30 % of misses
            bins.push_back(r < noise ? 1 - favoured : favoured);
        }
    put("model_bins", bins);
    for (int qp : qps)
        for (size_t c = 0; c < init.size(); c++) {
            ContextModel m;
            m.init(qp, (Int)init[c]);
            for (int k = 0; k < K; k++) {
                const int b = (int)bins[c * K + k];
                bits.push_back(m.getEntropyBits((Short)b));
                m.update(b);
                states.push_back((m.getState() << 1) + m.getMps());
            }
        }
    put("model_bits", bits);
    put("model_states", states);

    for (int log2 = 2; log2 <= 5; log2++) {
        const int t = 1 << log2, g = t >> 2;
        for (int s = 0; s < SCAN_NUMBER_OF_TYPES; s++) {
            char name[64];
            std::vector<long> scan, group_scan;
            const UInt* grouped = g_scanOrder[SCAN_GROUPED_4x4][s][log2][log2];
            const UInt* plain = g_scanOrder[SCAN_UNGROUPED][s][log2 - 2][log2 - 2];
            for (int i = 0; i < t * t; i++) scan.push_back(grouped[i]);
            for (int i = 0; i < g * g; i++) group_scan.push_back(plain[i]);
            snprintf(name, sizeof name, "scan_%d_%d", t, s); put(name, scan);
            snprintf(name, sizeof name, "group_scan_%d_%d", t, s); put(name, group_scan);
            if (t > MDCS_MAXIMUM_WIDTH && s != SCAN_DIAG) continue;
            TUEntropyCodingParameters cp;
            cp.scan = grouped; cp.scanCG = plain; cp.scanType = COEFF_SCAN_TYPE(s); cp.widthInGroups = cp.heightInGroups = g;
            cp.firstSignificanceMapContext = significanceMapContextSetStart[CHANNEL_TYPE_LUMA][t == 4 ? CONTEXT_TYPE_4x4 : t == 8 ? CONTEXT_TYPE_8x8 : CONTEXT_TYPE_NxN];
            if (t == 8 && s != SCAN_DIAG) cp.firstSignificanceMapContext += nonDiagonalScan8x8ContextOffset[CHANNEL_TYPE_LUMA];
            std::vector<long> sig;
            for (int pattern = 0; pattern < 4; pattern++)
                for (int i = 0; i < t * t; i++) sig.push_back(TComTrQuant::getSigCtxInc(pattern, cp, i, log2, log2, CHANNEL_TYPE_LUMA));
            snprintf(name, sizeof name, "sig_ctx_%d_%d", t, s); put(name, sig);
        }
    }

    std::vector<long> maps, ctx, pattern;
    for (int k = 0; k < 48; k++) {
        UInt flags[16];
        for (int i = 0; i < 16; i++) { lcg = lcg * 1664525u + 1013904223u; flags[i] = k == 0 ? 0 : k == 1 ? 1 : ((lcg >> 16) % 100 < (unsigned)(10 + 2 * k)); }
        for (int i = 0; i < 16; i++) maps.push_back(flags[i]);
        for (int gy = 0; gy < 4; gy++)
            for (int gx = 0; gx < 4; gx++) {
                ctx.push_back(TComTrQuant::getSigCoeffGroupCtxInc(flags, gx, gy, 4, 4));
                pattern.push_back(TComTrQuant::calcPatternSigCtx(flags, gx, gy, 4, 4));
            }
    }
    put("group_maps", maps); put("group_ctx", ctx); put("group_pattern", pattern);

    std::vector<long> groups, params;
    for (int i = 0; i < 32; i++) groups.push_back(g_uiGroupIdx[i]);
    for (int t = 4; t <= 32; t *= 2) {
        Int ox, oy, sx, sy;
        getLastSignificantContextParameters(COMPONENT_Y, t, t, ox, oy, sx, sy);
        params.push_back(ox); params.push_back(sx);
        if (ox != oy || sx != sy) return 2;
    }
    put("last_group", groups); put("last_params", params);
    destroyROM();
    return 0;
}
