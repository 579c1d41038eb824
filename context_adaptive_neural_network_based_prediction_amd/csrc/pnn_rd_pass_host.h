// What the host twin of the second intra pass (pnn_rd_pass.cpp) and the host twin of transform skip (pnn_tskip.cpp; DESIGN.md section
// 5p) share: one call of the pass as a record -- laid out after RdPassCall and RdPassOutputs of pnn_eval.cpp, the device side --, the
// one refusal, the coder of n slots of ONE QP in both forms -- sse, nonzero, rate and ts_flag [n] of the kept form under mode_bits [n]
// -- and the pass with signalling that takes a record with one.  pnn_rd_pass.cpp names none of pnn_tskip.cpp's entries, so it links
// without that file.
#pragma once

#include "../../include/pnn_hip.h"

#include <cstdint>
#include <cstdio>

namespace pnn {
typedef int (*RdSlotCoder)(const uint8_t* pred, const uint8_t* targets, int n, const uint8_t* modes, int qp, uint32_t* sse, uint32_t* nonzero,
                           uint64_t* rate, int sign_data_hiding, int rdoq, double lambda, const uint32_t* mode_bits, uint8_t* ts_flag);

struct RdPassHostOutputs {
    uint8_t* cand_modes; double* cand_costs; uint8_t* best_mode; uint8_t* best_slot; double* best_cost; uint32_t* best_sse; uint64_t* best_rate;
    double* first_pass_costs; uint64_t* best_side_rate; uint8_t* best_ts_flag;
    bool any() const
    {
        return cand_modes || cand_costs || best_mode || best_slot || best_cost || best_sse || best_rate || first_pass_costs || best_side_rate ||
               best_ts_flag;
    }
};
// One call of the second intra pass or of its first pass, whichever entry it came through: the name a refusal is reported under, the
// blocks, the candidate, the coding's arguments -- what every entry's argument list starts with, in its order --, then the options, the
// neighbours, the outputs (NULL where the entry has none) and the coder of the slots' two forms (NULL: the transformed form alone).
struct RdPassHostCall {
    const char* entry;
    const uint8_t* patterns; int pattern_h, pattern_w; const uint8_t* targets; int width, n;
    const uint8_t* cand_pred; int smoothing;
    const int* qps; int nb_qps; const double* lambdas;
    int sign_data_hiding = 0, rdoq = 0, signalling = 0, codec = 0;
    const uint8_t* left = nullptr; const uint8_t* above = nullptr;
    RdPassHostOutputs out{};
    RdSlotCoder coder = nullptr;
    double lambda(int i) const { return lambdas ? lambdas[i] : pnn_hm_intra_lambda(qps[i]); }
    // a check of the lambdas given that runs in front of the QPs' own check: over the indices that exist whatever nb_qps holds
    template <typename Ok>
    bool given_lambdas_are(Ok ok) const
    {
        for (int i = 0; lambdas && qps && i < nb_qps && i < 8; i++)
            if (!ok(lambdas[i])) return false;
        return true;
    }
};
inline int rd_pass_refuse(const char* entry, const char* why)
{
    fprintf(stderr, "%s: %s\n", entry, why);
    return PNN_E_ARG;
}

// the second pass of one record, every slot coded by q.coder where there is one
int rd_pass_host_with_coder(const RdPassHostCall& q);
}  // namespace pnn
