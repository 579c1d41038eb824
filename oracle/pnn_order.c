/* CPU model of the library's exact-f32 summation order, revision 6 ("precision" 0).
 *
 * TEST INFRASTRUCTURE beside the oracle (pnn_oracle.c): it reads the same flat canonical parameters (weights.tensor_specs order)
 * and computes, per output, the additions the GPU kernels perform in the order INTEGRATION.md section 4 "Exact-f32 summation
 * order, revision 6" specifies -- written from that text, not from the library's packing code.  Items of the specification are
 * cited as [O6.n].  Every multiply-add is an explicit fmaf() or _mm256_fmadd_ps() across independent output channels (one rounding
 * per multiply-add either way); the file is built with -ffp-contract=off and without fast-math, so nothing else fuses or reorders.
 * Blocks are spread over OpenMP threads, each output computed by one thread in one fixed order: the bits do not depend on the
 * thread count or on how a batch is cut.
 *
 * `variant` is a mask of deliberate departures from the order (ORDER_V_*): the sensitivity test uses them to show that the
 * bit-exact GPU comparison would see a kernel that drifts in that part of the order.  0 = the order itself.
 */
#include <immintrin.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define ORDER_V_CHUNK_PLAIN      0x001u   /* k = 0, 1, .., 15 inside a chunk instead of 0, 8, 1, 9, .. [O6.4] */
#define ORDER_V_NO_CONV_KSEG     0x002u   /* deep convolution layers as one chain [O6.5] */
#define ORDER_V_NO_FC_KSEG       0x004u   /* deep FC layers as one chain [O6.6] */
#define ORDER_V_FC_OUT_ONESEG    0x008u   /* FC output layer as one chain of 1200 [O6.7] */
#define ORDER_V_SEG_REVERSE      0x010u   /* segment sums added last to first [O6.8] */
#define ORDER_V_BIAS_FIRST       0x020u   /* tap GEMMs: the chain starts from the bias [O6.8] */
#define ORDER_V_CONV1_BIAS_LAST  0x040u   /* first convolution: chain from 0, bias added after it [O6.9] */
#define ORDER_V_MERGER_PLAIN     0x080u   /* merger: one chain over positions 0 .. 79 [O6.10] */
#define ORDER_V_LAST_PLAIN       0x100u   /* last layer: channels in plain order [O6.11] */
#define ORDER_V_FC_OUT_K16       0x200u   /* FC output layer in the hidden layers' in-chunk order [O6.7] */

static const char kTag[] = "pnn-order-6:f32:fmaf-chain k=0,8,1,9..7,15 per 16:kseg 1600/2304:fc-kseg 320:fc-out-seg 160";
enum { kSegDepth = 1600, kSegMinDepth = 2304, kFcSegChunks = 20, kFcOutSeg = 160, kHidden = 1200 };

const char *order_tag(void) { return kTag; }

void order_set_threads(int n)
{
#ifdef _OPENMP
    omp_set_num_threads(n > 0 ? n : 1);
#else
    (void)n;
#endif
}

static float leaky(float v)                          /* [O6.8]: max(0.1f * v, v) */
{
    const float t = 0.1f * v;
    return t > v ? t : v;
}

/* acc[co] = fma(x[k], W[k * ldw + co], acc[co]) for k = ks[0], ks[1], .. ks[nk - 1] in that order, co = 0 .. N - 1: one chain per
 * output; eight outputs per vector instruction, four vectors side by side (independent chains, same rounding as fmaf). */
static void chain(float *acc, const float *x, const float *W, long ldw, const int *ks, int nk, int N)
{
    int co = 0;
    for (; co + 32 <= N; co += 32) {
        __m256 a0 = _mm256_loadu_ps(acc + co), a1 = _mm256_loadu_ps(acc + co + 8);
        __m256 a2 = _mm256_loadu_ps(acc + co + 16), a3 = _mm256_loadu_ps(acc + co + 24);
        for (int j = 0; j < nk; j++) {
            const long k = ks[j];
            const __m256 xb = _mm256_set1_ps(x[k]);
            const float *w = W + k * ldw + co;
            a0 = _mm256_fmadd_ps(xb, _mm256_loadu_ps(w), a0);
            a1 = _mm256_fmadd_ps(xb, _mm256_loadu_ps(w + 8), a1);
            a2 = _mm256_fmadd_ps(xb, _mm256_loadu_ps(w + 16), a2);
            a3 = _mm256_fmadd_ps(xb, _mm256_loadu_ps(w + 24), a3);
        }
        _mm256_storeu_ps(acc + co, a0); _mm256_storeu_ps(acc + co + 8, a1);
        _mm256_storeu_ps(acc + co + 16, a2); _mm256_storeu_ps(acc + co + 24, a3);
    }
    for (; co + 8 <= N; co += 8) {
        __m256 a0 = _mm256_loadu_ps(acc + co);
        for (int j = 0; j < nk; j++) {
            const long k = ks[j];
            a0 = _mm256_fmadd_ps(_mm256_set1_ps(x[k]), _mm256_loadu_ps(W + k * ldw + co), a0);
        }
        _mm256_storeu_ps(acc + co, a0);
    }
    for (; co < N; co++) {
        float a = acc[co];
        for (int j = 0; j < nk; j++) a = fmaf(x[ks[j]], W[(long)ks[j] * ldw + co], a);
        acc[co] = a;
    }
}

/* ------------------------------------------------------------------------------------------------------------------------
 * Tap GEMM layers [O6.1-O6.8]: FC layers, convolutions (Cin >= 16) and transposed convolutions (Cout >= 4).
 * ------------------------------------------------------------------------------------------------------------------------ */
enum { kMaxTaps = 25, kMaxCls = 4, kMaxSeg = 8 };

typedef struct {
    int ncls, s_out;                 /* classes; output stride (tconv: s, the class is the output parity) */
    int ntap[kMaxCls];
    int dy[kMaxCls][kMaxTaps], dx[kMaxCls][kMaxTaps];   /* input offset of each tap of each class, in K order [O6.1] */
    int a;                           /* input step per output position of the class grid (conv: s; tconv: 1) */
    int IH, IW, Cin, SH, SW, Cout;   /* input map; class grid (outputs of one class); output channels */
    int act;
    float *w[kMaxCls];               /* [K_cls][Cout], row k = tap * Cin + ci */
    const float *bias;
    int nseg[kMaxCls];
    int *seq[kMaxCls][kMaxSeg];      /* k order of each segment */
    int seqn[kMaxCls][kMaxSeg];
} TapLayer;

/* [O6.4]: the visit order of the 16 k of a chunk */
static void chunk_order(int *dst, int k0, unsigned variant)
{
    for (int i = 0; i < 16; i++) dst[i] = k0 + ((variant & ORDER_V_CHUNK_PLAIN) ? i : (i >> 1) + 8 * (i & 1));
}

/* Segments of one class [O6.5, O6.6] and the k sequence of each. */
static void tap_layer_plan(TapLayer *L, unsigned variant, int fc_out)
{
    int tmax = 0, tmin = 1 << 30;
    for (int c = 0; c < L->ncls; c++) {
        tmax = L->ntap[c] > tmax ? L->ntap[c] : tmax;
        tmin = L->ntap[c] < tmin ? L->ntap[c] : tmin;
    }
    const int cpt = L->Cin / 16;
    for (int c = 0; c < L->ncls; c++) {
        const int t = L->ntap[c];
        const long K = (long)t * L->Cin;
        int nseg = 1;
        if (fc_out) {                                  /* [O6.7]: segments of 160 inputs, in-chunk order 0,4,1,5,2,6,3,7 per 8 */
            nseg = (variant & ORDER_V_FC_OUT_ONESEG) ? 1 : (int)((K + kFcOutSeg - 1) / kFcOutSeg);
            const long per = (variant & ORDER_V_FC_OUT_ONESEG) ? K : kFcOutSeg;
            L->nseg[c] = nseg;
            for (int s = 0; s < nseg; s++) {
                const long k0 = s * per, k1 = k0 + per < K ? k0 + per : K;
                L->seq[c][s] = malloc(sizeof(int) * (size_t)(k1 - k0));
                L->seqn[c][s] = (int)(k1 - k0);
                for (long k = k0; k < k1; k++) {
                    const long r = k - k0, g = r & ~7L, i = r & 7;
                    L->seq[c][s][r] = (variant & ORDER_V_FC_OUT_K16)
                                          ? (int)(k0 + (r & ~15L) + (((r & 15) >> 1) + 8 * (r & 1)))
                                          : (int)(k0 + g + (i >> 1) + 4 * (i & 1));
                }
            }
            continue;
        }
        int seg_taps[kMaxSeg + 1] = {0};               /* conv: first tap of each segment */
        long seg_chunks = 0;                           /* FC: chunks per segment */
        if (tmax > 1 && (long)tmax * L->Cin >= kSegMinDepth && !(variant & ORDER_V_NO_CONV_KSEG)) {
            long n = ((long)tmax * L->Cin + kSegDepth - 1) / kSegDepth;
            if (n > 8) n = 8;
            if (n > tmin) n = tmin;
            nseg = (int)n;
        } else if (tmax == 1 && L->ncls == 1 && cpt > kFcSegChunks && !(variant & ORDER_V_NO_FC_KSEG)) {
            seg_chunks = kFcSegChunks;
            nseg = (cpt + kFcSegChunks - 1) / kFcSegChunks;
        }
        L->nseg[c] = nseg;
        if (!seg_chunks) {                             /* whole taps dealt in order, the first (t % nseg) segments one more */
            const int base = t / nseg, rem = t % nseg;
            for (int s = 0; s < nseg; s++) seg_taps[s + 1] = seg_taps[s] + base + (s < rem);
        }
        for (int s = 0; s < nseg; s++) {
            long c0, c1;                               /* chunk range of the segment */
            if (seg_chunks) { c0 = s * seg_chunks; c1 = c0 + seg_chunks < cpt ? c0 + seg_chunks : cpt; }
            else { c0 = (long)seg_taps[s] * cpt; c1 = (long)seg_taps[s + 1] * cpt; }
            L->seq[c][s] = malloc(sizeof(int) * (size_t)(16 * (c1 - c0)));
            L->seqn[c][s] = (int)(16 * (c1 - c0));
            for (long ch = c0; ch < c1; ch++) chunk_order(L->seq[c][s] + 16 * (ch - c0), (int)(16 * ch), variant);
        }
    }
}

static void tap_layer_free(TapLayer *L)
{
    for (int c = 0; c < L->ncls; c++) {
        free(L->w[c]);
        for (int s = 0; s < L->nseg[c]; s++) free(L->seq[c][s]);
    }
}

/* One block: X [IH][IW][Cin] -> Y [SH * s_out][SW * s_out][Cout]. */
static void tap_layer_block(const TapLayer *L, const float *X, float *Y, unsigned variant, float *xk, float *acc, float *tot)
{
    const int OW = L->SW * L->s_out, Cout = L->Cout;
    for (int c = 0; c < L->ncls; c++) {
        const int py = c / L->s_out, px = c % L->s_out;
        for (int i = 0; i < L->SH; i++)
            for (int j = 0; j < L->SW; j++) {
                for (int t = 0; t < L->ntap[c]; t++) {     /* the K vector: (tap, ci), zeros outside the input [O6.1] */
                    const int iy = i * L->a + L->dy[c][t], ix = j * L->a + L->dx[c][t];
                    float *d = xk + (long)t * L->Cin;
                    if (iy >= 0 && iy < L->IH && ix >= 0 && ix < L->IW) memcpy(d, X + ((long)iy * L->IW + ix) * L->Cin, sizeof(float) * L->Cin);
                    else memset(d, 0, sizeof(float) * L->Cin);
                }
                const int ns = L->nseg[c];
                for (int q = 0; q < ns; q++) {           /* [O6.8]: each segment a chain from 0, the sums added in segment order */
                    const int s = (variant & ORDER_V_SEG_REVERSE) ? ns - 1 - q : q;
                    for (int co = 0; co < Cout; co++) acc[co] = (q == 0 && (variant & ORDER_V_BIAS_FIRST)) ? L->bias[co] : 0.f;
                    chain(acc, xk, L->w[c], Cout, L->seq[c][s], L->seqn[c][s], Cout);
                    if (q == 0) memcpy(tot, acc, sizeof(float) * Cout);
                    else for (int co = 0; co < Cout; co++) tot[co] = tot[co] + acc[co];
                }
                float *y = Y + ((long)(i * L->s_out + py) * OW + (j * L->s_out + px)) * Cout;
                for (int co = 0; co < Cout; co++) {
                    float v = (variant & ORDER_V_BIAS_FIRST) ? tot[co] : tot[co] + L->bias[co];
                    y[co] = L->act ? leaky(v) : v;
                }
            }
    }
}

/* Forward convolution, SAME padding (top / left pad = max((O - 1) s + k - I, 0) / 2), W [k][k][Cin][Cout] [O6.2]. */
static void conv_layer_init(TapLayer *L, const float *W, const float *b, int IH, int IW, int Cin, int Cout, int s, unsigned variant)
{
    memset(L, 0, sizeof(*L));
    const int k = 2 * s + 1, OH = (IH + s - 1) / s, OW = (IW + s - 1) / s;
    const int pad = ((OH - 1) * s + k - IH) > 0 ? ((OH - 1) * s + k - IH) / 2 : 0;
    L->ncls = 1; L->s_out = 1; L->a = s; L->IH = IH; L->IW = IW; L->Cin = Cin; L->SH = OH; L->SW = OW; L->Cout = Cout;
    L->act = 1; L->bias = b; L->ntap[0] = k * k;
    for (int ky = 0; ky < k; ky++)
        for (int kx = 0; kx < k; kx++) { L->dy[0][ky * k + kx] = ky - pad; L->dx[0][ky * k + kx] = kx - pad; }
    L->w[0] = malloc(sizeof(float) * (size_t)k * k * Cin * Cout);
    memcpy(L->w[0], W, sizeof(float) * (size_t)k * k * Cin * Cout);
    tap_layer_plan(L, variant, 0);
}

/* Transposed convolution, W [k][k][Cout][Cin], output (i s + py, j s + px) = class py * s + px [O6.3]. */
static void tconv_layer_init(TapLayer *L, const float *W, const float *b, int IH, int Cin, int Cout, int s, unsigned variant)
{
    memset(L, 0, sizeof(*L));
    const int k = 2 * s + 1, OH = IH * s;
    const int pad = ((IH - 1) * s + k - OH) > 0 ? ((IH - 1) * s + k - OH) / 2 : 0;
    L->ncls = s * s; L->s_out = s; L->a = 1; L->IH = IH; L->IW = IH; L->Cin = Cin; L->SH = IH; L->SW = IH; L->Cout = Cout;
    L->act = 1; L->bias = b;
    for (int py = 0; py < s; py++)
        for (int px = 0; px < s; px++) {
            const int c = py * s + px;
            int n = 0;
            for (int ky = 0; ky < k; ky++) {
                if ((py + pad - ky) % s) continue;
                for (int kx = 0; kx < k; kx++) {
                    if ((px + pad - kx) % s) continue;
                    L->dy[c][n] = (py + pad - ky) / s; L->dx[c][n] = (px + pad - kx) / s;
                    n++;
                }
            }
            L->ntap[c] = n;
            L->w[c] = malloc(sizeof(float) * (size_t)n * Cin * Cout);
            n = 0;
            for (int ky = 0; ky < k; ky++) {
                if ((py + pad - ky) % s) continue;
                for (int kx = 0; kx < k; kx++) {
                    if ((px + pad - kx) % s) continue;
                    const float *wt = W + (size_t)(ky * k + kx) * Cout * Cin;
                    for (int ci = 0; ci < Cin; ci++)
                        for (int co = 0; co < Cout; co++) L->w[c][((size_t)n * Cin + ci) * Cout + co] = wt[(size_t)co * Cin + ci];
                    n++;
                }
            }
        }
    tap_layer_plan(L, variant, 0);
}

static void fc_layer_init(TapLayer *L, const float *W, const float *b, int K, int N, int act, int out, unsigned variant)
{
    memset(L, 0, sizeof(*L));
    L->ncls = 1; L->s_out = 1; L->a = 1; L->IH = L->IW = 1; L->Cin = K; L->SH = L->SW = 1; L->Cout = N; L->act = act; L->bias = b;
    L->ntap[0] = 1;
    L->w[0] = malloc(sizeof(float) * (size_t)K * N);
    memcpy(L->w[0], W, sizeof(float) * (size_t)K * N);
    tap_layer_plan(L, variant, out);
}

/* ------------------------------------------------------------------------------------------------------------------------ */

/* [O6.9] First convolution (Cin = 1), W [k][k][1][Cout]: acc = bias, then fmaf over the taps in (ky, kx) order, LeakyReLU. */
static void conv1_block(const float *X, int IH, int IW, const float *W, const float *b, int Cout, int s, float *Y, unsigned variant)
{
    const int k = 2 * s + 1, OH = (IH + s - 1) / s, OW = (IW + s - 1) / s;
    const int pad = ((OH - 1) * s + k - IH) > 0 ? ((OH - 1) * s + k - IH) / 2 : 0;
    for (int oy = 0; oy < OH; oy++)
        for (int ox = 0; ox < OW; ox++)
            for (int co = 0; co < Cout; co++) {
                float acc = (variant & ORDER_V_CONV1_BIAS_LAST) ? 0.f : b[co];
                for (int ky = 0; ky < k; ky++)
                    for (int kx = 0; kx < k; kx++) {
                        const int iy = oy * s + ky - pad, ix = ox * s + kx - pad;
                        const float x = (iy >= 0 && iy < IH && ix >= 0 && ix < IW) ? X[iy * IW + ix] : 0.f;
                        acc = fmaf(x, W[(ky * k + kx) * Cout + co], acc);
                    }
                if (variant & ORDER_V_CONV1_BIAS_LAST) acc = acc + b[co];
                Y[((long)oy * OW + ox) * Cout + co] = leaky(acc);
            }
}

/* [O6.10] Merger: v = [above 4x12 row-major | left 8x4 row-major] per channel; four chains over the positions
 * p = 4 (w + 4 t) + e (t = 0..4, e = 0..3) for w = 0..3, then (S0 + S1) + (S2 + S3), + bias, LeakyReLU.  Y [16][C]. */
static void merger_block(const float *A, const float *Lf, int C, const float *Wm, const float *bm, float *Y, unsigned variant)
{
    for (int c = 0; c < C; c++)
        for (int j = 0; j < 16; j++) {
            float v;
            if (variant & ORDER_V_MERGER_PLAIN) {
                v = 0.f;
                for (int p = 0; p < 80; p++) v = fmaf(p < 48 ? A[p * C + c] : Lf[(p - 48) * C + c], Wm[((size_t)c * 80 + p) * 16 + j], v);
            } else {
                float S[4];
                for (int w = 0; w < 4; w++) {
                    float a = 0.f;
                    for (int t = 0; t < 5; t++)
                        for (int e = 0; e < 4; e++) {
                            const int p = 4 * (w + 4 * t) + e;
                            a = fmaf(p < 48 ? A[p * C + c] : Lf[(p - 48) * C + c], Wm[((size_t)c * 80 + p) * 16 + j], a);
                        }
                    S[w] = a;
                }
                v = (S[0] + S[1]) + (S[2] + S[3]);
            }
            Y[j * C + c] = leaky(v + bm[c * 16 + j]);
        }
}

/* [O6.11] Last transposed convolution (Cout = 1), W [k][k][1][Cin], input [IH][IH][Cin] -> Y [IH s][IH s]. */
static void last_block(const float *X, int IH, int Cin, const float *W, float bias, int s, float *Y, unsigned variant)
{
    const int k = 2 * s + 1, OH = IH * s;
    const int pad = ((IH - 1) * s + k - OH) > 0 ? ((IH - 1) * s + k - OH) / 2 : 0;
    for (int oy = 0; oy < OH; oy++)
        for (int ox = 0; ox < OH; ox++) {
            float v = 0.f;
            for (int ky = 0; ky < k; ky++) {
                if ((oy + pad - ky) % s) continue;
                const int iy = (oy + pad - ky) / s;
                if (iy < 0 || iy >= IH) continue;
                for (int kx = 0; kx < k; kx++) {
                    if ((ox + pad - kx) % s) continue;
                    const int ix = (ox + pad - kx) / s;
                    if (ix < 0 || ix >= IH) continue;
                    const float *x = X + ((long)iy * IH + ix) * Cin, *w = W + (ky * k + kx) * Cin;
                    if (Cin == 64 || (variant & ORDER_V_LAST_PLAIN)) {    /* the tap's product: one chain from 0, then v += it */
                        float t = 0.f;
                        for (int ci = 0; ci < Cin; ci++) {
                            const int cc = (variant & ORDER_V_LAST_PLAIN) ? ci : (ci & ~7) + ((ci & 7) >> 1) + 4 * (ci & 1);
                            t = fmaf(x[cc], w[cc], t);
                        }
                        v = v + t;
                    } else {                     /* other Cin: per channel quad x1 w1, then fma of x0, x2, x3; v += each quad */
                        for (int c4 = 0; c4 < Cin; c4 += 4) {
                            float q = x[c4 + 1] * w[c4 + 1];
                            q = fmaf(x[c4], w[c4], q);
                            q = fmaf(x[c4 + 2], w[c4 + 2], q);
                            q = fmaf(x[c4 + 3], w[c4 + 3], q);
                            v = v + q;
                        }
                    }
                }
            }
            Y[oy * OH + ox] = v + bias;
        }
}

/* ------------------------------------------------------------------------------------------------------------------------ */

static int strides_for(int w, int *st)
{
    static const int s4[] = {1, 1}, s8[] = {2, 1}, s16[] = {2, 1, 2, 1}, s32[] = {2, 2, 1, 2, 1}, s64[] = {2, 2, 2, 2, 1};
    const int *s; int n;
    switch (w) {
    case 4: s = s4; n = 2; break;
    case 8: s = s8; n = 2; break;
    case 16: s = s16; n = 4; break;
    case 32: s = s32; n = 5; break;
    case 64: s = s64; n = 5; break;
    default: return -1;
    }
    memcpy(st, s, sizeof(int) * n);
    return n;
}

static size_t tap_scratch(const TapLayer *L)
{
    int t = 0;
    for (int c = 0; c < L->ncls; c++) t = L->ntap[c] > t ? L->ntap[c] : t;
    return (size_t)t * L->Cin;
}

int order_fc_forward(const float *params, int w, const float *ctx, int B, float *out, unsigned variant)
{
    if (w != 4 && w != 8 && w != 16) return -1;
    const int dims[5] = {5 * w * w, kHidden, kHidden, kHidden, w * w};
    TapLayer L[4];
    const float *p = params;
    for (int i = 0; i < 4; i++) {
        /* [O6.7]: an output layer of <= 64 outputs (FC 4x4, 8x8) has its own order; the 16x16 net's 256 outputs are a tap GEMM layer */
        fc_layer_init(&L[i], p, p + (size_t)dims[i] * dims[i + 1], dims[i], dims[i + 1], i < 3, i == 3 && dims[4] <= 64, variant);
        p += (size_t)dims[i] * dims[i + 1] + dims[i + 1];
    }
#pragma omp parallel
    {
        float *x0 = malloc(sizeof(float) * kHidden), *x1 = malloc(sizeof(float) * kHidden);
        float *xk = malloc(sizeof(float) * 5 * 16 * 16), *acc = malloc(sizeof(float) * kHidden), *tot = malloc(sizeof(float) * kHidden);
#pragma omp for schedule(dynamic, 1)
        for (int b = 0; b < B; b++) {
            tap_layer_block(&L[0], ctx + (size_t)b * dims[0], x0, variant, xk, acc, tot);
            tap_layer_block(&L[1], x0, x1, variant, xk, acc, tot);
            tap_layer_block(&L[2], x1, x0, variant, xk, acc, tot);
            tap_layer_block(&L[3], x0, out + (size_t)b * dims[4], variant, xk, acc, tot);
        }
        free(x0); free(x1); free(xk); free(acc); free(tot);
    }
    for (int i = 0; i < 4; i++) tap_layer_free(&L[i]);
    return 0;
}

int order_conv_forward(const float *params, int w, const float *above, const float *left, int B, float *out, unsigned variant)
{
    int st[8];
    const int nl = strides_for(w, st);
    if (nl < 0) return -1;
    /* layer table, canonical order */
    const float *c1w[2], *c1b[2];
    int c1s[2], c1c[2];
    TapLayer br[2][8], tc[8];
    int hw[2][9][2];                                  /* map size in front of each branch layer */
    const float *p = params;
    int C = 32;
    for (int r = 0; r < 2; r++) {
        int H = r == 0 ? w : 2 * w, Wd = r == 0 ? 3 * w : w, cin = 1, ch = 32;
        for (int i = 0; i < nl; i++) {
            const int s = st[i], k = 2 * s + 1;
            ch *= s;
            const size_t nw = (size_t)k * k * cin * ch;
            hw[r][i][0] = H; hw[r][i][1] = Wd;
            if (i == 0) { c1w[r] = p; c1b[r] = p + nw; c1s[r] = s; c1c[r] = ch; }
            else conv_layer_init(&br[r][i], p, p + nw, H, Wd, cin, ch, s, variant);
            p += nw + ch;
            H = (H + s - 1) / s; Wd = (Wd + s - 1) / s; cin = ch;
        }
        hw[r][nl][0] = H; hw[r][nl][1] = Wd;
        C = ch;
    }
    const float *Wm = p, *bm = p + (size_t)C * 80 * 16;
    p = bm + (size_t)C * 16;
    int ci = C, H = 4;
    const float *lw = NULL;
    float lb = 0.f;
    int ls = 1, lcin = 0, lih = 0;
    for (int i = 0; i < nl; i++) {
        const int s = st[nl - 1 - i], k = 2 * s + 1;
        const int last = i == nl - 1, co = last ? 1 : ci / s;
        const size_t nw = (size_t)k * k * co * ci;
        if (last) { lw = p; lb = p[nw]; ls = s; lcin = ci; lih = H; }
        else tconv_layer_init(&tc[i], p, p + nw, H, ci, co, s, variant);
        p += nw + co;
        H *= s; ci = co;
    }
    /* scratch: the largest map of any layer */
    size_t maxmap = 0, maxk = 0;
    for (int r = 0; r < 2; r++)
        for (int i = 0; i < nl; i++) {
            const int s = st[i];
            const size_t o = (size_t)((hw[r][i][0] + s - 1) / s) * ((hw[r][i][1] + s - 1) / s) * (32 << 4);
            maxmap = o > maxmap ? o : maxmap;
            if (i) maxk = tap_scratch(&br[r][i]) > maxk ? tap_scratch(&br[r][i]) : maxk;
        }
    for (int i = 0; i + 1 < nl; i++) {
        const size_t o = (size_t)tc[i].SH * tc[i].s_out * tc[i].SW * tc[i].s_out * tc[i].Cout;
        maxmap = o > maxmap ? o : maxmap;
        maxk = tap_scratch(&tc[i]) > maxk ? tap_scratch(&tc[i]) : maxk;
    }
    const size_t cmax = 1024;
#pragma omp parallel
    {
        float *m0 = malloc(sizeof(float) * maxmap), *m1 = malloc(sizeof(float) * maxmap);
        float *fa = malloc(sizeof(float) * 48 * C), *fl = malloc(sizeof(float) * 32 * C);
        float *xk = malloc(sizeof(float) * maxk), *acc = malloc(sizeof(float) * cmax), *tot = malloc(sizeof(float) * cmax);
#pragma omp for schedule(dynamic, 1)
        for (int b = 0; b < B; b++) {
            for (int r = 0; r < 2; r++) {
                const float *in = r == 0 ? above + (size_t)b * 3 * w * w : left + (size_t)b * 2 * w * w;
                conv1_block(in, hw[r][0][0], hw[r][0][1], c1w[r], c1b[r], c1c[r], c1s[r], m0, variant);
                float *cur = m0, *nxt = m1;
                for (int i = 1; i < nl; i++) {
                    tap_layer_block(&br[r][i], cur, nxt, variant, xk, acc, tot);
                    float *t = cur; cur = nxt; nxt = t;
                }
                memcpy(r == 0 ? fa : fl, cur, sizeof(float) * (r == 0 ? 48 : 32) * C);
            }
            merger_block(fa, fl, C, Wm, bm, m0, variant);
            float *cur = m0, *nxt = m1;
            for (int i = 0; i + 1 < nl; i++) {
                tap_layer_block(&tc[i], cur, nxt, variant, xk, acc, tot);
                float *t = cur; cur = nxt; nxt = t;
            }
            last_block(cur, lih, lcin, lw, lb, ls, out + (size_t)b * w * w, variant);
        }
        free(m0); free(m1); free(fa); free(fl); free(xk); free(acc); free(tot);
    }
    for (int r = 0; r < 2; r++)
        for (int i = 1; i < nl; i++) tap_layer_free(&br[r][i]);
    for (int i = 0; i + 1 < nl; i++) tap_layer_free(&tc[i]);
    return 0;
}
