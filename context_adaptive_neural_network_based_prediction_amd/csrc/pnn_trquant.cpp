// Host twin of the open-loop transform coding (no HIP in this file): HM's residual path with RDOQ 0 on a prediction somebody else made
// -- residual, forward core transform (xTrMxN), quantisation (the non-RDOQ branch of xQuant, I slice), dequantisation (xDeQuant without
// scaling lists), inverse transform (xITrMxN), reconstruction -- for 8-bit luma intra blocks, per transform unit: T = w up to 32, the
// four 32 x 32 quadrants of the one prediction at w = 64 (this project's definition; HM would predict each quadrant again).  The
// definition is restated at the declarations in include/pnn_hip.h; the constants live in pnn_trquant_tables.h.  HM's butterflies are
// exact integer factorisations of the matrix products written here, so the integers are the same.  No RDOQ, sign-data hiding, transform
// skip: all need the running entropy-coder state, which does not exist open-loop.  The CABAC rate of the levels
// is counted from the state a slice STARTS with: pnn_cabac_tables.h, whose lines the kernel compiles too.
// pnn_trquant.hip computes the same on the GPU; tests/test_gpu_trquant.py checks one against the other, tests/test_trquant.py pins this
// file to a numpy restatement and to recorded outputs of HM's own transforms.
#include "../../include/pnn_hip.h"
#include "pnn_cabac_tables.h"
#include "pnn_trquant_tables.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {

using namespace pnn::trquant;

bool width_ok(int w) { return w == 4 || w == 8 || w == 16 || w == 32 || w == 64; }

// M[k][x] of one unit size, dense
struct Matrix {
    int t, log2_t, m[32 * 32];
    explicit Matrix(int log2_t_) : t(1 << log2_t_), log2_t(log2_t_)
    {
        for (int k = 0; k < t; k++)
            for (int x = 0; x < t; x++) m[k * t + x] = matrix_coeff(log2_t, k, x);
    }
    int at(int k, int x) const { return m[k * t + x]; }
};

// the per-TU routine, stage by stage; every array is dense [t][t]
void forward(const Matrix& M, const int* residual, int* coeffs)
{
    const int t = M.t, s1 = fwd_shift1(M.log2_t), s2 = fwd_shift2(M.log2_t);
    int y1[32 * 32];
    for (int y = 0; y < t; y++)
        for (int k = 0; k < t; k++) {
            int acc = 0;
            for (int x = 0; x < t; x++) acc += residual[y * t + x] * M.at(k, x);
            y1[y * t + k] = (acc + (1 << (s1 - 1))) >> s1;
        }
    for (int l = 0; l < t; l++)
        for (int k = 0; k < t; k++) {
            int acc = 0;
            for (int y = 0; y < t; y++) acc += y1[y * t + k] * M.at(l, y);
            coeffs[l * t + k] = (acc + (1 << (s2 - 1))) >> s2;
        }
}

void inverse(const Matrix& M, const int* dequant, int* residual)
{
    const int t = M.t;
    int z[32 * 32];
    for (int y = 0; y < t; y++)
        for (int k = 0; k < t; k++) {
            int acc = 0;
            for (int l = 0; l < t; l++) acc += M.at(l, y) * dequant[l * t + k];
            z[y * t + k] = clip16((acc + (1 << (kInvShift1 - 1))) >> kInvShift1);
        }
    for (int y = 0; y < t; y++)
        for (int x = 0; x < t; x++) {
            int acc = 0;
            for (int k = 0; k < t; k++) acc += M.at(k, x) * z[y * t + k];
            residual[y * t + x] = clip16((acc + (1 << (kInvShift2 - 1))) >> kInvShift2);
        }
}

// quantise -> dequantise -> inverse of one unit's coefficients at one QP; the counts ADD into *nb_nonzero / *sum_abs
void code_unit(const Matrix& M, const int* coeffs, const QpConsts& q, int* levels, int* dequant, int* residual, uint32_t* nb_nonzero,
               uint32_t* sum_abs)
{
    for (int i = 0; i < M.t * M.t; i++) {
        int mag;
        levels[i] = quant_level(coeffs[i], q, &mag);
        dequant[i] = dequant_level(levels[i], q);
        *nb_nonzero += levels[i] != 0;
        *sum_abs += (uint32_t)mag;
    }
    inverse(M, dequant, residual);
}

// the unit at (uy, ux) of a w x w block: target - prediction
void unit_residual(const uint8_t* prediction, const uint8_t* target, int w, int t, int uy, int ux, int* residual)
{
    for (int y = 0; y < t; y++)
        for (int x = 0; x < t; x++) {
            const int i = (uy * t + y) * w + ux * t + x;
            residual[y * t + x] = (int)target[i] - (int)prediction[i];
        }
}

// the CABAC rate of one unit's levels (dense [t][t]) from the initial states of a QP
struct InitStates {
    uint8_t s[pnn::cabac::kNumCtx];
    explicit InitStates(int qp)
    {
        for (int i = 0; i < pnn::cabac::kNumCtx; i++) s[i] = (uint8_t)pnn::cabac::init_state(qp, pnn::cabac::init_value(i));
    }
};
uint64_t unit_rate(int log2_t, const int* levels, int scan, const InitStates& init)
{
    using namespace pnn::cabac;
    uint8_t state[kNumCtx];
    switch (log2_t) {
    case 2: return pnn::cabac::unit_rate<2>(levels, scan, init.s, state, rom_tables());
    case 3: return pnn::cabac::unit_rate<3>(levels, scan, init.s, state, rom_tables());
    case 4: return pnn::cabac::unit_rate<4>(levels, scan, init.s, state, rom_tables());
    default: return pnn::cabac::unit_rate<5>(levels, scan, init.s, state, rom_tables());
    }
}

}  // namespace

extern "C" int pnn_trquant_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const int* qps, int nb_qps,
                                uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon)
{
    return pnn_trquant_rate_host(predictions, targets, width, n, nullptr, qps, nb_qps, sses_recon, nb_nonzero, sum_abs_levels, recon, nullptr);
}

extern "C" int pnn_trquant_rate_host(const uint8_t* predictions, const uint8_t* targets, int width, int n, const uint8_t* modes, const int* qps,
                                     int nb_qps, uint32_t* sses_recon, uint32_t* nb_nonzero, uint32_t* sum_abs_levels, uint8_t* recon,
                                     uint64_t* rate)
{
    if (!width_ok(width)) { fprintf(stderr, "The width of the target patch is not 4, 8, 16, 32 or 64.\n"); return PNN_E_ARG; }
    if (n < 0 || (n > 0 && (!predictions || !targets))) { fprintf(stderr, "Bad batch size or NULL inputs.\n"); return PNN_E_ARG; }
    if (!qps_ok(qps, nb_qps)) { fprintf(stderr, "The QPs are not 1 to 8 integers in [0, 51].\n"); return PNN_E_ARG; }
    if (!sses_recon && !nb_nonzero && !sum_abs_levels && !recon && !rate) { fprintf(stderr, "Every output is NULL.\n"); return PNN_E_ARG; }
    if (modes && !rate) { fprintf(stderr, "Intra modes without a rate output.\n"); return PNN_E_ARG; }
    for (long b = 0; modes && b < n; b++)
        if (modes[b] > 34) { fprintf(stderr, "An intra mode is above 34.\n"); return PNN_E_ARG; }
    const Matrix M(log2_tu(width));
    const int t = M.t, units = width / t;
    const size_t w2 = (size_t)width * width;
    std::vector<InitStates> init;
    for (int qi = 0; rate && qi < nb_qps; qi++) init.emplace_back(qps[qi]);
    int residual[32 * 32], coeffs[32 * 32], levels[32 * 32], dequant[32 * 32], decoded[32 * 32];
    for (long b = 0; b < n; b++) {
        const uint8_t* prediction = predictions + b * w2;
        const uint8_t* target = targets + b * w2;
        uint32_t sse[kMaxQps] = {}, nonzero[kMaxQps] = {}, sum_abs[kMaxQps] = {};
        uint64_t bits[kMaxQps] = {};
        const int scan = modes ? pnn::cabac::scan_of_mode(M.log2_t, modes[b]) : pnn::cabac::kScanDiag;
        for (int uy = 0; uy < units; uy++)
            for (int ux = 0; ux < units; ux++) {
                unit_residual(prediction, target, width, t, uy, ux, residual);
                forward(M, residual, coeffs);                                  // once per unit, whatever the number of QPs
                for (int qi = 0; qi < nb_qps; qi++) {
                    code_unit(M, coeffs, qp_consts(M.log2_t, qps[qi]), levels, dequant, decoded, &nonzero[qi], &sum_abs[qi]);
                    if (rate) bits[qi] += unit_rate(M.log2_t, levels, scan, init[qi]);
                    for (int y = 0; y < t; y++)
                        for (int x = 0; x < t; x++) {
                            const size_t i = (size_t)(uy * t + y) * width + ux * t + x;
                            const int v = (int)prediction[i] + decoded[y * t + x], rec = v < 0 ? 0 : v > 255 ? 255 : v;
                            const int d = rec - (int)target[i];
                            sse[qi] += (uint32_t)(d * d);
                            if (recon) recon[((size_t)qi * n + b) * w2 + i] = (uint8_t)rec;
                        }
                }
            }
        for (int qi = 0; qi < nb_qps; qi++) {
            if (sses_recon) sses_recon[(size_t)qi * n + b] = sse[qi];
            if (nb_nonzero) nb_nonzero[(size_t)qi * n + b] = nonzero[qi];
            if (sum_abs_levels) sum_abs_levels[(size_t)qi * n + b] = sum_abs[qi];
            if (rate) rate[(size_t)qi * n + b] = bits[qi];
        }
    }
    return PNN_OK;
}

extern "C" int pnn_cabac_rate_levels_host(const int32_t* levels, int t, int scan, int qp, uint64_t* rate)
{
    if (t != 4 && t != 8 && t != 16 && t != 32) { fprintf(stderr, "The unit size is not 4, 8, 16 or 32.\n"); return PNN_E_ARG; }
    if (!levels || !rate) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (scan < 0 || scan > 2 || (t > 8 && scan != pnn::cabac::kScanDiag)) {
        fprintf(stderr, "The scan is not 0 (diagonal), 1 (horizontal) or 2 (vertical), or not diagonal above 8 x 8.\n");
        return PNN_E_ARG;
    }
    if (!qps_ok(&qp, 1)) { fprintf(stderr, "The QP does not belong to [0, 51].\n"); return PNN_E_ARG; }
    for (int i = 0; i < t * t; i++)
        if (levels[i] < -32768 || levels[i] > 32767) { fprintf(stderr, "A level is outside [-32768, 32767].\n"); return PNN_E_ARG; }
    *rate = unit_rate(log2_tu(t), levels, scan, InitStates(qp));
    return PNN_OK;
}

extern "C" int pnn_trquant_stages_host(const uint8_t* prediction, const uint8_t* target, int width, int qp, int32_t* coeffs, int32_t* levels,
                                       int32_t* dequant, int32_t* residual)
{
    if (!width_ok(width)) { fprintf(stderr, "The width of the target patch is not 4, 8, 16, 32 or 64.\n"); return PNN_E_ARG; }
    if (!prediction || !target) { fprintf(stderr, "NULL pointer.\n"); return PNN_E_ARG; }
    if (!qps_ok(&qp, 1)) { fprintf(stderr, "The QP does not belong to [0, 51].\n"); return PNN_E_ARG; }
    if (!coeffs && !levels && !dequant && !residual) { fprintf(stderr, "Every output is NULL.\n"); return PNN_E_ARG; }
    const Matrix M(log2_tu(width));
    const int t = M.t, units = width / t;
    const QpConsts q = qp_consts(M.log2_t, qp);
    int in[32 * 32], stage[4][32 * 32];
    int32_t* const outs[4] = {coeffs, levels, dequant, residual};
    for (int uy = 0; uy < units; uy++)
        for (int ux = 0; ux < units; ux++) {
            uint32_t nonzero = 0, sum_abs = 0;
            unit_residual(prediction, target, width, t, uy, ux, in);
            forward(M, in, stage[0]);
            code_unit(M, stage[0], q, stage[1], stage[2], stage[3], &nonzero, &sum_abs);
            for (int s = 0; s < 4; s++)                                        // each unit's arrays where the unit lies in the block
                if (outs[s])
                    for (int y = 0; y < t; y++)
                        for (int x = 0; x < t; x++) outs[s][(size_t)(uy * t + y) * width + ux * t + x] = stage[s][y * t + x];
        }
    return PNN_OK;
}
