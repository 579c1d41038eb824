// Diagnostics of the pass layer (pnn_passes.cpp), out of its way: the environment switches, each read once, and the read-back-and-print
// blocks of the diagnostic library (make diag).  tools/profile_round.sh and tools/conv_layers.py parse the lines printed here.
#include "pnn_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace pnn {

bool env_debug() { static const bool on = getenv("PNN_DEBUG") != nullptr; return on; }
bool env_profile() { static const bool on = getenv("PNN_PROFILE") != nullptr; return on; }       // tuning aid: per-launch timing, synchronous
bool env_f32s_diag() { static const bool on = getenv("PNN_F32S_DIAG") != nullptr; return on; }   // the small exact-f32 kernel's MFMA loop
bool env_f32_diag() { static const bool on = getenv("PNN_F32_DIAG") != nullptr; return on; }     // per-workgroup cycle stamps of tapgemm_f32_kernel
bool env_sp_diag() { static const bool on = getenv("PNN_SP_DIAG") != nullptr; return on; }       // phase stamps of every split-precision workgroup

// Under PNN_B1_STAMPS: the next kernel's slot of per-workgroup 100 MHz stamps (host_predict prints them), or null.  64 bytes per
// workgroup: [3] loop start, [4] entry, [5] exit (behind the acknowledged stores), [1] loop ticks.
void* diag_stamp_slot(pnn_ctx* c, const char* name, long wgs, double k)
{
    if (!c->diag_stamps || c->diag_launch >= pnn_ctx::kDiagLaunches || wgs > pnn_ctx::kDiagWgs) return nullptr;
    c->diag_names.push_back(name);
    c->diag_wgs.push_back((int)wgs);
    c->diag_k.push_back(k);
    return (char*)c->diag_stamps + (size_t)c->diag_launch++ * pnn_ctx::kDiagWgs * 64;
}

// PNN_F32S_DIAG: the launch `ps` of tapgemm_f32_small_kernel once more with stamps: the MFMA wave's loop, cycles per chunk and clock
int diag_f32_small(pnn_ctx* c, const GemmLayer& L, const TapGemmParams& ps, int nseg, const float* host_rows, hipStream_t s)
{
    HIPCHK(c, hipStreamSynchronize(s));
    if (dev_reserve(c, c->stage_tbs, (size_t)4 << 20)) return PNN_E_NOMEM;
    HIPCHK(c, hipMemset(c->stage_tbs.p, 0, (size_t)4 << 20));
    TapGemmParams q = ps;
    q.Xlo = c->stage_tbs.p;
    HIPCHK(c, launch_tapgemm_f32_small(q, s, host_rows, (int)c->opt_f32_small_deep));
    HIPCHK(c, hipStreamSynchronize(s));
    const size_t nwg = std::min<size_t>((size_t)tapgemm_f32_small_tiles(ps), ((size_t)4 << 20) / 64);
    std::vector<unsigned long long> hbuf(8 * nwg);
    HIPCHK(c, hipMemcpy(hbuf.data(), c->stage_tbs.p, hbuf.size() * 8, hipMemcpyDeviceToHost));
    double cyc = 0, ticks = 0, chunks = 0;
    unsigned long long r0 = ~0ull, r1 = 0;
    for (size_t i = 0; i < nwg; i++) { cyc += (double)hbuf[8 * i]; ticks += (double)hbuf[8 * i + 1]; chunks += (double)hbuf[8 * i + 2]; r0 = std::min(r0, hbuf[8 * i + 3]); r1 = std::max(r1, hbuf[8 * i + 3] + hbuf[8 * i + 1]); }
    fprintf(stderr, "[pnn-f32s-diag] M=%ld K=%.0f N=%d ncls=%d nseg=%d: %zu WGs, loop %.0f cycles for %.0f chunks = %.0f cycles per chunk (160 = the chain), %.2f us, clock %.0f MHz; first loop start -> last loop end %.1f us\n",
            (long)ps.M, L.k_total, ps.Cout, ps.ncls, nseg, nwg, cyc / nwg, chunks / nwg, cyc / std::max(1.0, chunks), ticks / nwg / 100.0, cyc / std::max(1.0, ticks) * 100.0, (double)(r1 - r0) / 100.0);
    return PNN_OK;
}

// PNN_F32_DIAG: the launch `p` of tapgemm_f32_kernel (tile `tile`, `fused` = with the output layer, par_segs = K segments in the
// grid) 400 times with per-workgroup cycle stamps
int diag_f32_tiles(pnn_ctx* c, const GemmLayer& L, const TapGemmParams& p, int tile, bool fused, int par_segs, hipStream_t s)
{
    const TileCfg t = tapgemm_f32_cfg(tile);
    const long M = p.M;
    HIPCHK(c, hipStreamSynchronize(s));
    if (dev_reserve(c, c->stage_tbs, (size_t)16 << 20)) return PNN_E_NOMEM;
    TapGemmParams q = p;
    q.Xlo = c->stage_tbs.p;
    HIPCHK(c, hipMemset(c->stage_tbs.p, 0, (size_t)16 << 20));
    for (int rep = 0; rep < 400; rep++) HIPCHK(c, launch_tapgemm_f32(q, tile, fused, s));   // back to back: the stamps that
                                                                                       // stay are the last launch's, at the steady-state clock
    HIPCHK(c, hipStreamSynchronize(s));
    size_t nwg = (size_t)((M + 128L * t.rt - 1) / (128L * t.rt)) * ((p.Cout + 32L * t.nt - 1) / (32L * t.nt)) * p.ncls * par_segs;
    if (t.pair && g_last_pair_mode == 1) { int gx, groups, n; f32_pair_grid(p.M, p.Cout, &gx, &groups, &n); nwg = (size_t)n; }
    std::vector<unsigned long long> hbuf(8 * nwg);
    HIPCHK(c, hipMemcpy(hbuf.data(), c->stage_tbs.p, hbuf.size() * 8, hipMemcpyDeviceToHost));
    if (t.pair && g_last_pair_mode == 1) {
        // A paired launch: the wide and the narrow tiles apart (slot = workgroup; a slot without stamps had no tile), and where they ran --
        // per CU (XCC, SE, SH, CU of the hardware id) how many wide and narrow workgroups, and whether a pair's two met on one
        const int gx = (int)((M + 127) / 128);
        double sum[2][4] = {}; size_t cnt[2] = {0, 0};
        unsigned long long r0 = ~0ull, r1 = 0, end[2] = {0, 0};
        std::map<unsigned long long, std::pair<int, int>> per_cu;
        std::map<int, unsigned long long> cu_of[2];
        for (size_t i = 0; i < nwg; i++) {
            const unsigned long long* d = &hbuf[8 * i];
            if (!d[3]) continue;
            const PairTile pt = f32_pair_tile((int)i, gx);
            const int k = pt.narrow;
            for (int j = 0; j < 4; j++) sum[k][j] += (double)d[j];
            cnt[k]++;
            r0 = std::min(r0, d[4]); r1 = std::max(r1, d[4] + d[3]); end[k] = std::max(end[k], d[4] + d[3]);
            const unsigned long long cu = ((d[5] >> 32) & 0xf) << 16 | (d[5] & 0xff00);
            (k ? per_cu[cu].second : per_cu[cu].first)++;
            cu_of[k][pt.group * gx + pt.bx] = cu;
        }
        size_t one_each = 0, together = 0;
        for (const auto& kv : per_cu) one_each += kv.second.first == 1 && kv.second.second == 1;
        for (const auto& kv : cu_of[1]) { const auto w = cu_of[0].find(kv.first); together += w != cu_of[0].end() && w->second == kv.second; }
        for (int k = 0; k < 2; k++)
            fprintf(stderr, "[pnn-f32diag] M=%ld K=%.0f N=%d pair kc %d %s: %zu WGs; wave 0 mean cycles: prologue %.0f  loop %.0f  epilogue %.0f; lifetime %.1f us; last end %.1f us after the first start\n",
                    M, L.k_total, p.Cout, t.kc, k ? "narrow 128x64" : "wide 128x96", cnt[k], sum[k][0] / std::max<size_t>(cnt[k], 1), sum[k][1] / std::max<size_t>(cnt[k], 1),
                    sum[k][2] / std::max<size_t>(cnt[k], 1), sum[k][3] / std::max<size_t>(cnt[k], 1) / 100.0, (double)(end[k] - r0) / 100.0);
        fprintf(stderr, "[pnn-f32diag]   first start -> last end %.1f us; %zu CUs in use, %zu of them with one wide and one narrow workgroup; %zu of %zu pairs with both tiles on one CU\n",
                (double)(r1 - r0) / 100.0, per_cu.size(), one_each, together, cu_of[1].size());
        return PNN_OK;
    }
    double sum[4] = {0, 0, 0, 0};
    unsigned long long r0 = ~0ull, r1 = 0;
    for (size_t i = 0; i < nwg; i++) {
        for (int k = 0; k < 4; k++) sum[k] += (double)hbuf[8 * i + k];
        r0 = std::min(r0, hbuf[8 * i + 4]); r1 = std::max(r1, hbuf[8 * i + 4] + hbuf[8 * i + 3]);
    }
    size_t late = 0; unsigned long long life_max = 0;     // workgroups that start > 5 us behind the first; the longest lifetime
    for (size_t i = 0; i < nwg; i++) { late += hbuf[8 * i + 4] > r0 + 500; life_max = std::max(life_max, hbuf[8 * i + 3]); }
    const double chunks = std::ceil(L.k_total / 16.0 / p.ncls / par_segs / t.kc) * t.kc;
    const double cyc = (sum[0] + sum[1] + sum[2]) / nwg, rt_ticks = sum[3] / nwg;
    fprintf(stderr, "[pnn-f32diag] M=%ld K=%.0f N=%d {%d,%d,%d}%s: %zu WGs; wave 0 mean cycles: prologue %.0f  loop %.0f (MFMA work %.0f = %.3f)  epilogue %.0f;"
            " lifetime %.1f us (max %.1f), in-kernel clock %.0f MHz; first start -> last end %.1f us, %zu workgroups start > 5 us late\n", M, L.k_total, p.Cout, t.rt, t.nt, t.kc, fused ? "+out" : "", nwg,
            sum[0] / nwg, sum[1] / nwg, chunks * 8 * t.rt * t.nt * 64, chunks * 8 * t.rt * t.nt * 64 / (sum[1] / nwg), sum[2] / nwg, rt_ticks / 100.0, (double)life_max / 100.0,
            cyc / (rt_ticks / 100.0), (double)(r1 - r0) / 100.0, late);
    return PNN_OK;
}

// PNN_SP_DIAG: the phase stamps that tapgemm_sp_kernel, launched as `p` with tile `cfg`, left in stage_tbs (diag runs take no other kernel)
int diag_sp(pnn_ctx* c, const GemmLayer& L, const TapGemmParams& p, int cfg, hipStream_t s)
{
    HIPCHK(c, hipStreamSynchronize(s));
    const TileCfg tt = tapgemm_sp_cfg(cfg);
    const long M = p.M, bm = 32L * tt.rt * tt.wm, bn = 32L * tt.nt * (4 / tt.wm);
    const size_t nwg = (size_t)((M + bm - 1) / bm) * ((p.Cout + bn - 1) / bn) * p.ncls;
    std::vector<unsigned long long> h(4 * nwg);
    HIPCHK(c, hipMemcpy(h.data(), c->stage_tbs.p, h.size() * 8, hipMemcpyDeviceToHost));
    double sum[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < nwg; i++) for (int k = 0; k < 4; k++) sum[k] += (double)h[4 * i + k];
    const double stages = std::ceil(L.k_total / 16.0 / p.ncls / tt.kc);
    fprintf(stderr, "[pnn-diag] M=%ld K=%.0f N=%d cfg {%d,%d,%d,wm%d}: per stage (cycles, wave 0 mean over %zu WGs): issue %.0f  mfma %.0f  store %.0f  barrier %.0f\n",
            M, L.k_total, p.Cout, tt.rt, tt.nt, tt.kc, tt.wm, nwg, sum[0] / nwg / stages, sum[1] / nwg / stages, sum[2] / nwg / stages, sum[3] / nwg / stages);
    return PNN_OK;
}

}  // namespace pnn
