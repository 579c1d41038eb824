// What the host twin of the second intra pass (pnn_rd_pass.cpp) and the host twin of transform skip (pnn_tskip.cpp; DESIGN.md section
// 5p) share: the coder of n slots of ONE QP in both forms -- sse, nonzero, rate and ts_flag [n] of the kept form under mode_bits [n] --
// and the body with signalling that takes it.  pnn_rd_pass.cpp names none of pnn_tskip.cpp's entries, so it links without that file.
#pragma once

#include <cstdint>

namespace pnn {
typedef int (*RdSlotCoder)(const uint8_t* pred, const uint8_t* targets, int n, const uint8_t* modes, int qp, uint32_t* sse, uint32_t* nonzero,
                           uint64_t* rate, int sign_data_hiding, int rdoq, double lambda, const uint32_t* mode_bits, uint8_t* ts_flag);
int rd_pass_host_with_coder(const char* entry, int codec, const uint8_t* patterns, int pattern_h, int pattern_w, const uint8_t* targets, int width,
                            int n, const uint8_t* cand_pred, int smoothing, const int* qps, int nb_qps, const double* lambdas, int sign_data_hiding,
                            int rdoq, const uint8_t* left_modes, const uint8_t* above_modes, uint8_t* cand_modes, double* cand_costs,
                            uint8_t* best_mode, uint8_t* best_slot, double* best_cost, uint32_t* best_sse, uint64_t* best_rate,
                            double* first_pass_costs, uint64_t* best_side_rate, RdSlotCoder coder, uint8_t* best_ts_flag);
}  // namespace pnn
