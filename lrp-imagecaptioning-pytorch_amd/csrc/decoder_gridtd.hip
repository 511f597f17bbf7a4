// The gridTD adaptive-attention decoder (models/gridTDmodel.py): forward trace, LRP relevance, guided-backprop gradient, host loops.
// What no model owns (the skinny linear, arg-max, re-weighting, pixel spread, ...) is in decoder_blocks.hip, reached through its C entry
// points; what the decoders share on the device is decoder_shared.h.
//
// Everything here is small next to the VGG16 relevance pass (<1 % of the FLOPs), HBM / latency bound,
// and written as fused per-time-step kernels batched over all (image, word) rows so that the
// reference's ~50 k tiny `lrp_linear_eps` calls per image (models/gridTDmodel.py:1060-1128) become
// ~5 launches per lock-step.  Row r = b*T + t is the explanation of word t of image b; at lock-step s
// every row with t >= s works on time index i = t - s (models/gridTDmodel.py:1060 `for i in range(t+1)[::-1]`).
//
// Trace tensors are [B][T(+1)][...] fp32; token ids int64 (torch.long).
#include <math.h>

#include "common.h"
#include "conv_mfma.h"
#include "conv_launch.h"
#include "decoder_shared.h"

namespace lrpx {

// ------------------------------------------------------------------------------------------------
// gridTD forward (trace) — models/gridTDmodel.py:933-1012
// ------------------------------------------------------------------------------------------------
struct GridFwd {
    int B, T, H, E, P;
    // trace ([B][T..] tensors)
    float *xh1, *xh2;                     // [B][T][2E+2H], [B][T][3H]
    float *h1, *c1, *h2, *c2;             // [B][T+1][H]
    float *g1, *i1, *f1, *g2, *i2, *f2;   // [B][T][H]
    float *s, *ctx, *ctx_hat, *hc;        // [B][T][H]
    float *alpha, *beta;                  // [B][T][P], [B][T]
    float *o1, *o2, *sgate;               // [B][T][H] output gates / sentinel gate (gradient explainers only; may be null)
};

// xh1[b,t] = [h2[b,t] | glob[b] | emb[tok[b,t]] | h1[b,t]]
__global__ void gridtd_fwd_pre_kernel(GridFwd g, int t, const float* __restrict__ glob, const float* __restrict__ emb,
                                      const long long* __restrict__ tok, int tok_ld) {
    const int b = blockIdx.x;
    const int W = 2 * g.E + 2 * g.H;
    float* dst = g.xh1 + ((long)b * g.T + t) * W;
    const long st = ((long)b * (g.T + 1) + t) * g.H;
    const long long k = tok[(long)b * tok_ld + t];
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        float v;
        if (c < g.H) v = g.h2[st + c];
        else if (c < g.H + g.E) v = glob[(long)b * g.E + (c - g.H)];
        else if (c < g.H + 2 * g.E) v = emb[k * g.E + (c - g.H - g.E)];
        else v = g.h1[st + (c - g.H - 2 * g.E)];
        dst[c] = v;
    }
}

// LSTM point-wise part (models/gridTDmodel.py:777-784) + sentinel s = sigmoid(gate) * tanh(c) (:982-983)
// zz: [B][4H (+H gate)] pre-activations incl. bias
__global__ void gridtd_fwd_lstm_kernel(GridFwd g, int t, const float* __restrict__ zz, int ldz, int which) {
    const int b = blockIdx.x;
    const int H = g.H;
    const long st0 = ((long)b * (g.T + 1) + t) * H, st1 = st0 + H, tr = ((long)b * g.T + t) * H;
    float *hh = which == 1 ? g.h1 : g.h2, *cc = which == 1 ? g.c1 : g.c2;
    float *gg = which == 1 ? g.g1 : g.g2, *ii = which == 1 ? g.i1 : g.i2, *ff = which == 1 ? g.f1 : g.f2;
    const float* z = zz + (long)b * ldz;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float zg = z[2 * H + c];
        const LstmCell l = lstm_cell(z[c], z[H + c], zg, z[3 * H + c], cc[st0 + c]);
        const float cn = l.cn, hn = l.o * tanhf(cn);
        cc[st1 + c] = cn; hh[st1 + c] = hn;
        gg[tr + c] = zg; ii[tr + c] = l.i; ff[tr + c] = l.f;
        float* oo = which == 1 ? g.o1 : g.o2;
        if (oo) oo[tr + c] = l.o;
        if (which == 1) {
            const float sg = sigmoidf_(z[4 * H + c]);
            g.s[tr + c] = sg * tanhf(cn);
            if (g.sgate) g.sgate[tr + c] = sg;
        } else {
            g.hc[tr + c] = hn + g.ctx_hat[tr + c];           // fc input (:990)
        }
    }
}

// AdaptiveAttention.forward (models/gridTDmodel.py:71-103), two kernels so that B images fill the chip; their bodies are
// att_scores_block / att_context_block of decoder_shared.h, which the single-LSTM model's kernels (lrpx_adaatt.hip) call too.  Here:
//  (1) scores, grid (B, pixel blocks), on h1[t + 1] and the sentinel;
//  (2) context, grid (B, channel blocks): c_hat and xh2[b,t] = [ctx_hat | h1_new | h2_old].
__global__ __launch_bounds__(256) void gridtd_fwd_att_scores_kernel(
    GridFwd g, int t, const float* __restrict__ att_img, const float* __restrict__ Wg, const float* __restrict__ Ws,
    const float* __restrict__ bs, const float* __restrict__ wh, float* __restrict__ scr, const float* __restrict__ sg_in) {
    extern __shared__ float sm[];
    const int b = blockIdx.x, H = g.H, P = g.P, tid = threadIdx.x;
    float* h1n = sm;          // H
    float* sv = h1n + H;      // H
    const long st1 = ((long)b * (g.T + 1) + t + 1) * H, tr = ((long)b * g.T + t) * H;
    if (sg_in) {
        // fused step (gridtd_linear_lstm_kernel): the sentinel s = sigmoid(gate) * tanh(c1) (:982-983) is formed here from the gate the
        // gate linear left in sg_in [B][H] and the cell state it wrote - the expression of gridtd_fwd_lstm_kernel on the same values;
        // the first pixel block keeps it for the trace
        for (int c = tid; c < H; c += 256) {
            const float sgv = sg_in[(long)b * H + c];
            const float s = sgv * tanhf(g.c1[st1 + c]);
            h1n[c] = g.h1[st1 + c]; sv[c] = s;
            if (blockIdx.y == 0) { g.s[tr + c] = s; if (g.sgate) g.sgate[tr + c] = sgv; }
        }
    } else {
        for (int c = tid; c < H; c += 256) { h1n[c] = g.h1[st1 + c]; sv[c] = g.s[tr + c]; }
    }
    __syncthreads();
    att_scores_block(h1n, sv, H, P, b, blockIdx.y, att_img, Wg, Ws, bs, wh, scr + (long)b * 3 * P);       // [z | h_proj | s_proj]
}

__global__ __launch_bounds__(256) void gridtd_fwd_att_context_kernel(GridFwd g, int t, const float* __restrict__ Vp,
                                                                     const float* __restrict__ wh,
                                                                     const float* __restrict__ scr) {
    extern __shared__ float sm[];
    const int b = blockIdx.x, H = g.H, P = g.P, tid = threadIdx.x;
    float a;
    const float beta = att_context_block(scr + (long)b * 3 * P, sm, H, P, b, blockIdx.y, blockIdx.y == 0, Vp, wh,
                                         g.alpha + ((long)b * g.T + t) * P, g.beta + (long)b * g.T + t, a);
    const int c = blockIdx.y * ATT_CB + (tid & 31), part = tid >> 5;
    if (c < H && part == 0) {
        const long tr = ((long)b * g.T + t) * H, st0 = ((long)b * (g.T + 1) + t) * H;
        const float sv = g.s[tr + c], h1n = g.h1[st0 + H + c];
        const float ch = beta * sv + (1.f - beta) * a;
        float* x2 = g.xh2 + ((long)b * g.T + t) * 3 * H;
        g.ctx[tr + c] = a; g.ctx_hat[tr + c] = ch;
        x2[c] = ch; x2[H + c] = h1n; x2[2 * H + c] = g.h2[st0 + c];
    }
}

// xg[b] = [h2_old | glob | emb | h1_NEW]: the sentinel gate of sample_lrp sees the new h1 (:672), not h_{t-1}
__global__ void gridtd_gate_input_kernel(GridFwd g, int t, float* __restrict__ xg) {
    const int b = blockIdx.x;
    const int W = 2 * g.E + 2 * g.H;
    const float* src = g.xh1 + ((long)b * g.T + t) * W;
    const float* h1n = g.h1 + ((long)b * (g.T + 1) + t + 1) * g.H;
    for (int c = threadIdx.x; c < W; c += blockDim.x) xg[(long)b * W + c] = c < W - g.H ? src[c] : h1n[c - (W - g.H)];
}

// s = sigmoid(gate) * tanh(c1_new)   (:672-673)
__global__ void gridtd_sentinel_kernel(GridFwd g, int t, const float* __restrict__ zg, int ldz) {
    const int b = blockIdx.x;
    const long st1 = ((long)b * (g.T + 1) + t + 1) * g.H, tr = ((long)b * g.T + t) * g.H;
    for (int c = threadIdx.x; c < g.H; c += blockDim.x) {
        const float sg = sigmoidf_(zg[(long)b * ldz + c]);
        g.s[tr + c] = sg * tanhf(g.c1[st1 + c]);
        if (g.sgate) g.sgate[tr + c] = sg;
    }
}

// ------------------------------------------------------------------------------------------------
// gridTD relevance — models/gridTDmodel.py:1014-1135.  One block (256 threads) per row, H = 512.
// ------------------------------------------------------------------------------------------------
struct GridRel {
    int B, T, H, E, P;
    const int* lens;                      // [B] caption length per image (null: T)
    // trace (const)
    const float *xh1, *xh2, *h2, *c1, *c2, *g1, *i1, *f1, *g2, *i2, *f2, *s, *ctx, *ctx_hat, *hc, *beta;
    // state per row
    float *r_h2n, *r_c2, *r_c1, *r_ch0, *r_h2p, *r_glob;   // [rows][H]   (r_glob: [rows][E])
    float *A, *rx;                                          // GEMM in [rows][H], GEMM out [rows][<=2E+2H]
    float *wacc;                                            // [rows][T][H]  r_ctx / z~(ctx)
    float *r_words;                                         // [rows][T]
};

__device__ __forceinline__ bool row_active(const GridRel& g, int b, int t, int s) {
    const int len = g.lens ? g.lens[b] : g.T;
    return t < len && t >= s;
}

// :1033-1059 — one-hot relevance at the target logit through fc, split between h2 and ctx_hat
__global__ void gridtd_rel_init_kernel(GridRel g, const float* __restrict__ fcw, const float* __restrict__ logit,
                                       const long long* __restrict__ tok, int tok_ld) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long long k = tok[(long)b * tok_ld + t + 1];
    const float lg = logit[row];
    const float zt = stab_eps(lg);
    const long tr = (long)row * H, st1 = ((long)b * (g.T + 1) + t + 1) * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float hc = g.hc[tr + c];
        const float r_hc = (fcw[k * H + c] * hc / zt) * lg;
        g.r_h2n[tr + c] = eps_id(r_hc, g.h2[st1 + c], hc);
        g.r_ch0[tr + c] = eps_id(r_hc, g.ctx_hat[tr + c], hc);
        g.r_c2[tr + c] = 0.f; g.r_c1[tr + c] = 0.f;
    }
    for (int c = threadIdx.x; c < g.E; c += blockDim.x) g.r_glob[(long)row * g.E + c] = 0.f;
    for (int c = threadIdx.x; c < g.T; c += blockDim.x) g.r_words[(long)row * g.T + c] = 0.f;
}

// :1061-1069 LanguageLSTM cell: r_c2 += r_h2; split into the g-gate path and the c-path; A = r_g2 / z~(g2)
__global__ void gridtd_rel_a_kernel(GridRel g, int s) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long tr = (long)row * H;
    if (!row_active(g, b, t, s)) {
        for (int c = threadIdx.x; c < H; c += blockDim.x) g.A[tr + c] = 0.f;
        return;
    }
    const int i = t - s;
    const long ti = ((long)b * g.T + i) * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H, sc0 = sc1 - H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float rc = g.r_c2[tr + c] + g.r_h2n[tr + c];
        const float cn = g.c2[sc1 + c];
        const float rg = eps_id(rc, g.i2[ti + c] * tanhf(g.g2[ti + c]), cn);
        g.r_c2[tr + c] = eps_id(rc, g.f2[ti + c] * g.c2[sc0 + c], cn);
        g.A[tr + c] = rg / stab_eps(g.g2[ti + c]);
    }
}

// :1074-1105 after the LanguageLSTM dense rule: split r_xh2, sentinel/context split, AdaLSTM cell
__global__ void gridtd_rel_b_kernel(GridRel g, int s) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long tr = (long)row * H;
    if (!row_active(g, b, t, s)) {
        for (int c = threadIdx.x; c < H; c += blockDim.x) g.A[tr + c] = 0.f;
        return;
    }
    const int i = t - s;
    const long ti = ((long)b * g.T + i) * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H, sc0 = sc1 - H;
    const float* rx = g.rx + (long)row * (3 * H);                 // r_xh2 = [ctx_hat | h1 | h2], row stride 3H
    const float beta = g.beta[(long)b * g.T + i];
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        g.r_h2p[tr + c] = rx[2 * H + c];                           // :1074
        const float r_h1 = rx[H + c];                              // :1075
        const float r_ch = (s == 0 ? g.r_ch0[tr + c] : 0.f) + rx[c];   // :1076
        const float ch = g.ctx_hat[ti + c], cx = g.ctx[ti + c];
        const float r_s = eps_id(r_ch, beta * g.s[ti + c], ch);    // :1077-1080
        const float r_cx = eps_id(r_ch, cx * (1.f - beta), ch);    // :1081-1084
        g.wacc[((long)row * g.T + i) * H + c] = r_cx / stab_eps(cx);   // pixel spread (:1091-1095) is finished in rel_pix
        float rc = g.r_c1[tr + c] + r_s;                           // :1096
        rc = rc + r_h1;                                            // :1097
        const float cn = g.c1[sc1 + c];
        const float rg = eps_id(rc, g.i1[ti + c] * tanhf(g.g1[ti + c]), cn);
        g.r_c1[tr + c] = eps_id(rc, g.f1[ti + c] * g.c1[sc0 + c], cn);
        g.A[tr + c] = rg / stab_eps(g.g1[ti + c]);
    }
}

// :1110-1115 after the AdaLSTM dense rule: r_xh1 = [h2 | glob | emb | h1]
__global__ __launch_bounds__(256) void gridtd_rel_c_kernel(GridRel g, int s) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, E = g.E;
    if (!row_active(g, b, t, s)) return;
    const int i = t - s;
    const long tr = (long)row * H;
    const float* rx = g.rx + (long)row * (2 * E + 2 * H);
    for (int c = threadIdx.x; c < H; c += 256) g.r_h2n[tr + c] = g.r_h2p[tr + c] + rx[c];           // :1111
    float acc = 0.f;
    for (int c = threadIdx.x; c < E; c += 256) {
        g.r_glob[(long)row * E + c] += rx[H + c];                                                    // :1114
        acc += rx[H + E + c];                                                                        // :1115, :1129
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) g.r_words[(long)row * g.T + i] = acc;
}

// gridtd_rel_c_kernel of lock-step s and gridtd_rel_a_kernel of lock-step s + 1 in one launch (same expressions, same order: a thread owns
// the same channels c in both; the r_h2n it writes is the one it reads).  One launch less per lock-step: they are ~5 us dependent launches.
__global__ __launch_bounds__(256) void gridtd_rel_ca_kernel(GridRel g, int s) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, E = g.E;
    const long tr = (long)row * H;
    if (!row_active(g, b, t, s)) {                 // (then not active at s + 1 either)
        for (int c = threadIdx.x; c < H; c += 256) g.A[tr + c] = 0.f;
        return;
    }
    const int i = t - s;
    const float* rx = g.rx + (long)row * (2 * E + 2 * H);
    const bool nxt = row_active(g, b, t, s + 1);
    const int i1 = i - 1;                          // time step of lock-step s + 1
    const long ti = ((long)b * g.T + i1) * H, sc1 = ((long)b * (g.T + 1) + i1 + 1) * H, sc0 = sc1 - H;
    for (int c = threadIdx.x; c < H; c += 256) {
        const float r_h2n = g.r_h2p[tr + c] + rx[c];                                                  // :1111
        g.r_h2n[tr + c] = r_h2n;
        if (nxt) {                                                                                    // :1061-1069 at s + 1
            const float rc = g.r_c2[tr + c] + r_h2n;
            const float cn = g.c2[sc1 + c];
            const float rg = eps_id(rc, g.i2[ti + c] * tanhf(g.g2[ti + c]), cn);
            g.r_c2[tr + c] = eps_id(rc, g.f2[ti + c] * g.c2[sc0 + c], cn);
            g.A[tr + c] = rg / stab_eps(g.g2[ti + c]);
        } else {
            g.A[tr + c] = 0.f;
        }
    }
    float acc = 0.f;
    for (int c = threadIdx.x; c < E; c += 256) {
        g.r_glob[(long)row * E + c] += rx[H + c];                                                    // :1114
        acc += rx[H + E + c];                                                                        // :1115, :1129
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) g.r_words[(long)row * g.T + i] = acc;
}

// :1116-1119 prologue: A = r_glob / z~(glob_pre)
__global__ void gridtd_rel_glob_kernel(GridRel g, const float* __restrict__ glob_pre, float* __restrict__ Aglob) {
    const int row = blockIdx.x, b = row / g.T;
    for (int c = threadIdx.x; c < g.E; c += blockDim.x)
        Aglob[(long)row * g.E + c] = g.r_glob[(long)row * g.E + c] / stab_eps(glob_pre[(long)b * g.E + c]);
}

// pixel spread :1091-1095 summed over i, and the prologue of the projector rule (:1125-1128):
// Aproj[row][k][c] = Vp[b][k][c] * sum_{i<=t} alpha[b][i][k] * wacc[row][i][c] / z~(proj_pre[b][k][c])
// AVG (the bottom-up model, models/gridTDmodel.py:1912-1915: the global feature is taken from the mean of the PROJECTED regions, so
// its relevance r_avg [B*T][H] comes back under the projector rule): the eye rule of the mean, r_avg / (P z~(avg)), joins the
// bracket - one value per (row, c), formed once outside the pixel loop:
// Aproj[row][k][c] = Vp[b][k][c] * (sum_i ... + r_avg[row][c] / (P * z~(avg[b][c]))) / z~(proj_pre[b][k][c])
template <bool AVG>
__global__ __launch_bounds__(256) void gridtd_rel_pix_kernel(GridRel g, const float* __restrict__ Vp,
                                                             const float* __restrict__ proj_pre,
                                                             const float* __restrict__ alpha,
                                                             float* __restrict__ Aproj, int kchunk,
                                                             const int* __restrict__ rowlist,
                                                             const float* __restrict__ r_avg,
                                                             const float* __restrict__ avg) {
    // rowlist (variable caption lengths): workgroup x computes row rowlist[x] and writes it as row x of a COMPACT Aproj
    const int row = rowlist ? rowlist[blockIdx.x] : blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, P = g.P;
    const long orow = blockIdx.x;
    const int len = g.lens ? g.lens[b] : g.T;
    const int k0 = blockIdx.y * kchunk, k1 = min(k0 + kchunk, P);
    extern __shared__ float al[];    // [t+1][kchunk]
    const bool act = t < len;
    const int n = act ? t + 1 : 0;
    for (int j = threadIdx.x; j < n * kchunk; j += 256) {
        const int i = j / kchunk, kk = j - i * kchunk;
        al[j] = (k0 + kk < P) ? alpha[((long)b * g.T + i) * P + k0 + kk] : 0.f;
    }
    __syncthreads();
    constexpr int TREG = 24;         // captions up to 24 words: the row's accumulated weights stay in registers
    for (int c = threadIdx.x; c < H; c += 256) {
        float wr[TREG];
        if (n <= TREG) {
#pragma unroll
            for (int i = 0; i < TREG; ++i) wr[i] = i < n ? g.wacc[((long)row * g.T + i) * H + c] : 0.f;
        }
        float ua = 0.f;              // AVG: the mean's share of the bracket (inactive rows read nothing)
        if constexpr (AVG) {
            if (act) ua = r_avg[(long)row * H + c] / ((float)P * stab_eps(avg[(long)b * H + c]));
        }
        for (int k = k0; k < k1; ++k) {
            float a = 0.f;
            if (n <= TREG) {         // (same summation order as the loop below: i = n-1 .. 0; the tail adds exact zeros)
#pragma unroll
                for (int i = TREG - 1; i >= 0; --i) a += (i < n ? al[i * kchunk + (k - k0)] : 0.f) * wr[i];
            } else {
                for (int i = n - 1; i >= 0; --i) a += al[i * kchunk + (k - k0)] * g.wacc[((long)row * g.T + i) * H + c];
            }
            if constexpr (AVG) a += ua;
            const long pi = ((long)b * P + k) * H + c;
            Aproj[(orow * P + k) * H + c] = act ? Vp[pi] * a / stab_eps(proj_pre[pi]) : 0.f;
        }
    }
}

// ================================================================================================
// gridTD guided-backprop decoder: hand-written BPTT with alpha/beta constant (models/gridTDmodel.py:1588-1675)
// ================================================================================================
struct GridGrad {
    int B, T, H, E, P;
    const int* lens;
    const float *c1, *c2, *g1, *i1, *f1, *o1, *g2, *i2, *f2, *o2, *sgate, *beta;   // g* are pre-activations
    float *d_h2n, *d_c2, *d_c1, *d_ch0, *d_h2p, *d_glob;    // [rows][H] (d_glob: [rows][E])
    float *gates, *dx;                                       // GEMM in [rows][4H], out [rows][3H]
    float *wacc, *r_words;                                   // [rows][T][H], [rows][T]
};

__device__ __forceinline__ bool grad_row_active(const GridGrad& g, int b, int t, int s) {
    const int len = g.lens ? g.lens[b] : g.T;
    return t < len && t >= s;
}

// :1592-1625  d_word_pred one-hot = 1  ->  d(h2+ctx_hat) = fc.weight[k]
__global__ void gridtd_grad_init_kernel(GridGrad g, const float* __restrict__ fcw, const long long* __restrict__ tok,
                                        int tok_ld) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long long k = tok[(long)b * tok_ld + t + 1];
    const long tr = (long)row * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float d = fcw[k * H + c];
        g.d_h2n[tr + c] = d; g.d_ch0[tr + c] = d; g.d_c2[tr + c] = 0.f; g.d_c1[tr + c] = 0.f;
    }
    for (int c = threadIdx.x; c < g.E; c += blockDim.x) g.d_glob[(long)row * g.E + c] = 0.f;
    for (int c = threadIdx.x; c < g.T; c += blockDim.x) g.r_words[(long)row * g.T + c] = 0.f;
}

// LSTM cell backward (:1627-1637 / :1647-1657): dh, running dc -> gate pre-activation gradients [i|f|g|o]
__device__ __forceinline__ void lstm_cell_bwd(float dh, float& dc, float c_new, float c_old, float i, float f, float gpre,
                                              float o, float* gates, int H, int c) {
    const float tc = tanhf(c_new), ga = tanhf(gpre);
    const float d_oa = dh * tc;
    dc = dc + dh * o * (1.f - tc * tc);
    const float d_fa = dc * c_old, d_ia = dc * ga, d_ga = dc * i;
    gates[c] = d_ia * i * (1.f - i);
    gates[H + c] = d_fa * f * (1.f - f);
    gates[2 * H + c] = d_ga * (1.f - ga * ga);
    gates[3 * H + c] = d_oa * o * (1.f - o);
    dc = dc * f;      // d_c[i] = d_c[i+1] * f   (:1630 / :1650)
}

__global__ void gridtd_grad_a_kernel(GridGrad g, int s) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    float* gates = g.gates + (long)row * 4 * H;
    if (!grad_row_active(g, b, t, s)) {
        for (int c = threadIdx.x; c < 4 * H; c += blockDim.x) gates[c] = 0.f;
        return;
    }
    const int i = t - s;
    const long tr = (long)row * H, ti = ((long)b * g.T + i) * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H, sc0 = sc1 - H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        float dc = g.d_c2[tr + c];
        lstm_cell_bwd(g.d_h2n[tr + c], dc, g.c2[sc1 + c], g.c2[sc0 + c], g.i2[ti + c], g.f2[ti + c], g.g2[ti + c],
                      g.o2[ti + c], gates, H, c);
        g.d_c2[tr + c] = dc;
    }
}

// dx = gates2 @ [W_ih | W_hh] = [d_ctx_hat | d_h1 | d_h2]   (:1638-1646), then the AdaLSTM cell backward
__global__ void gridtd_grad_b_kernel(GridGrad g, int s) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    float* gates = g.gates + (long)row * 4 * H;
    if (!grad_row_active(g, b, t, s)) {
        for (int c = threadIdx.x; c < 4 * H; c += blockDim.x) gates[c] = 0.f;
        return;
    }
    const int i = t - s;
    const long tr = (long)row * H, ti = ((long)b * g.T + i) * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H, sc0 = sc1 - H;
    const float* dx = g.dx + (long)row * 3 * H;
    const float beta = g.beta[(long)b * g.T + i];
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        g.d_h2p[tr + c] = dx[2 * H + c];                                    // :1638
        const float d_ch = (s == 0 ? g.d_ch0[tr + c] : 0.f) + dx[c];        // :1640
        g.wacc[((long)row * g.T + i) * H + c] = d_ch * (1.f - beta);        // d_context (:1641), spread in rel_pix
        const float d_s = d_ch * beta;                                      // :1644
        const float tc1 = tanhf(g.c1[sc1 + c]);
        float dc = g.d_c1[tr + c] + d_s * g.sgate[ti + c] * (1.f - tc1 * tc1);   // :1645
        lstm_cell_bwd(dx[H + c], dc, g.c1[sc1 + c], g.c1[sc0 + c], g.i1[ti + c], g.f1[ti + c], g.g1[ti + c],
                      g.o1[ti + c], gates, H, c);                           // :1646-1657
        g.d_c1[tr + c] = dc;
    }
}

// dx = gates1 @ W_ih = [d_h2 | d_glob | d_emb]  (:1659-1662)
__global__ __launch_bounds__(256) void gridtd_grad_c_kernel(GridGrad g, int s) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, E = g.E;
    if (!grad_row_active(g, b, t, s)) return;
    const int i = t - s;
    const long tr = (long)row * H;
    const float* dx = g.dx + (long)row * 3 * H;      // row stride of the GEMM output buffer (H + 2E == 3H)
    for (int c = threadIdx.x; c < H; c += 256) g.d_h2n[tr + c] = g.d_h2p[tr + c] + dx[c];
    float acc = 0.f;
    for (int c = threadIdx.x; c < E; c += 256) {
        g.d_glob[(long)row * E + c] += dx[H + c];
        acc += dx[H + E + c];
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) g.r_words[(long)row * g.T + i] = acc;
}

// ---- gridTD: the two gate linears of a decoder step with their LSTM cells (gridtd_fwd_lstm_kernel) in the epilogue, and the next step's
// input row (gridtd_fwd_pre_kernel) behind the second: 7 launches per time step -> 4.  Weight rows interleaved as in decoder_aoa.hip (w_il / b_il:
// row 16 j + 4 gate + u = row gate * H + 4 j + u of [W_ih | W_hh], so that the four pre-activations of a hidden unit meet in the workgroup's
// LDS reduction); the same dot products in the same order as linear_mfma_kernel (linear_mfma_core) and the cell of gridtd_fwd_lstm_kernel
// (lstm_cell): bit-identical traces.
// WHICH == 1, AdaLSTM (models/gridTDmodel.py:777-784, sentinel gate :982): workgroups 0 .. H/4 - 1 hold the cells of hidden units 4 j .. 4 j + 3;
// workgroups H/4 .. H/4 + H/16 - 1 the 16 sentinel-gate rows 4 H + 16 (j - H/4) .. of the UN-interleaved [.. ; x_gate | h_gate] - sigmoid(gate) goes
// to sg [B][H], the sentinel s = sigmoid(gate) tanh(c1) is formed by the attention kernel that reads it (the cell state comes from other workgroups).
// WHICH == 2, LanguageLSTM: cells + fc input hc = h2 + ctx_hat (:990), then xh1[b, t + 1] = [h2[b, t + 1] | glob[b] | emb[tok[b, t + 1]] | h1[b, t + 1]]:
// the workgroup's own four h2 columns from its registers, a slice of the other columns copied.
template <int RT, int WHICH>
__global__ __launch_bounds__(256) void gridtd_linear_lstm_kernel(GridFwd g, int t, const float* __restrict__ w_il, const float* __restrict__ b_il,
                                                                 const float* __restrict__ w_cat, const float* __restrict__ b_cat,
                                                                 float* __restrict__ sg, const float* __restrict__ glob,
                                                                 const float* __restrict__ emb, const long long* __restrict__ tok, int tok_ld) {
    __shared__ float red[4][RT][16][17];
    const int H = g.H, E = g.E;
    const int K = WHICH == 1 ? 2 * E + 2 * H : 3 * H;
    const float* x = WHICH == 1 ? g.xh1 + (long)t * K : g.xh2 + (long)t * K;
    const int n_cell = H / 4;                                   // workgroups that hold cells
    if (WHICH == 1 && (int)blockIdx.x >= n_cell) {              // sentinel-gate rows (workgroup-uniform branch)
        const int n0 = 4 * H + ((int)blockIdx.x - n_cell) * 16;
        linear_mfma_core<RT>(x, (long)g.T * K, w_cat, g.B, K, 5 * H, red, n0);
        for (int e = threadIdx.x; e < RT * 256; e += 256) {
            const int r = e >> 8, row = (e >> 4) & 15, col = e & 15;
            const int b = r * 16 + row, c = n0 - 4 * H + col;
            if (b >= g.B || c >= H) continue;
            float z = red4<RT>(red, r, row, col);
            if (b_cat) z += b_cat[n0 + col];
            sg[(long)b * H + c] = sigmoidf_(z);
        }
        return;
    }
    linear_mfma_core<RT>(x, (long)g.T * K, w_il, g.B, K, 4 * H, red, blockIdx.x * 16);
    float *hh = WHICH == 1 ? g.h1 : g.h2, *cc = WHICH == 1 ? g.c1 : g.c2;
    float *gg = WHICH == 1 ? g.g1 : g.g2, *ii = WHICH == 1 ? g.i1 : g.i2, *ff = WHICH == 1 ? g.f1 : g.f2, *oo = WHICH == 1 ? g.o1 : g.o2;
    for (int e = threadIdx.x; e < RT * 64; e += 256) {
        const int r = e >> 6, row = (e >> 2) & 15, u = e & 3;
        const int b = r * 16 + row, c = blockIdx.x * 4 + u;
        if (b >= g.B || c >= H) continue;
        float z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 4 * q + u;
            z[q] = red4<RT>(red, r, row, col);
            if (b_il) z[q] += b_il[blockIdx.x * 16 + col];
        }
        const long st0 = ((long)b * (g.T + 1) + t) * H, st1 = st0 + H, tr = ((long)b * g.T + t) * H;
        const LstmCell l = lstm_cell(z[0], z[1], z[2], z[3], cc[st0 + c]);
        const float cn = l.cn, hn = l.o * tanhf(cn);
        cc[st1 + c] = cn; hh[st1 + c] = hn;
        gg[tr + c] = z[2]; ii[tr + c] = l.i; ff[tr + c] = l.f;
        if (oo) oo[tr + c] = l.o;
        if (WHICH == 2) {
            g.hc[tr + c] = hn + g.ctx_hat[tr + c];
            if (t + 1 < g.T) g.xh1[((long)b * g.T + t + 1) * (2 * E + 2 * H) + c] = hn;
        }
    }
    if (WHICH == 2 && t + 1 < g.T) {        // the other columns H .. 2 E + 2 H of the next input row: this workgroup's slice, every image
        const int W1 = 2 * E + 2 * H, rest = W1 - H;
        const int per = (rest + (int)gridDim.x - 1) / (int)gridDim.x;
        const int c0 = H + blockIdx.x * per, c1 = min(W1, c0 + per);
        for (int e = threadIdx.x; e < g.B * per; e += 256) {
            const int b = e / per, c = c0 + e - b * per;
            if (c >= c1) continue;
            float v;
            if (c < H + E) v = glob[(long)b * E + (c - H)];
            else if (c < H + 2 * E) v = emb[tok[(long)b * tok_ld + t + 1] * E + (c - H - E)];
            else v = g.h1[((long)b * (g.T + 1) + t + 1) * H + (c - H - 2 * E)];
            g.xh1[((long)b * g.T + t + 1) * W1 + c] = v;
        }
    }
}

}  // namespace lrpx

using namespace lrpx;

static GridFwd to_fwd(const lrpx_gridtd_trace* t) {
    GridFwd g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P;
    g.xh1 = t->xh1; g.xh2 = t->xh2; g.h1 = t->h1; g.c1 = t->c1; g.h2 = t->h2; g.c2 = t->c2;
    g.g1 = t->g1; g.i1 = t->i1; g.f1 = t->f1; g.g2 = t->g2; g.i2 = t->i2; g.f2 = t->f2;
    g.s = t->s; g.ctx = t->ctx; g.ctx_hat = t->ctx_hat; g.hc = t->hc; g.alpha = t->alpha; g.beta = t->beta;
    g.o1 = t->o1; g.o2 = t->o2; g.sgate = t->sgate;
    return g;
}

static int check_trace(const lrpx_gridtd_trace* t) {
    LRPX_REQUIRE(t && t->B > 0 && t->T > 0 && t->H == 512 && t->E % 4 == 0 && t->P > 0 && t->P <= 256,
                 "gridtd: unsupported trace dims (H must be 512, P <= 256)");
    LRPX_REQUIRE(t->xh1 && t->xh2 && t->h1 && t->c1 && t->h2 && t->c2 && t->g1 && t->i1 && t->f1 && t->g2 && t->i2 &&
                     t->f2 && t->s && t->ctx && t->ctx_hat && t->hc && t->alpha && t->beta,
                 "gridtd: null trace tensor");
    return LRPX_OK;
}

// sg: the sentinel gate [B][H] of the fused step (null: the trace's s is already there)
static int gridtd_attention(const lrpx_gridtd_trace* tr, int t, const float* Vp, const float* att_img, const float* Wg, const float* Ws,
                            const float* bs, const float* wh, float* scratch, const float* sg, void* stream) {
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(Vp && att_img && Wg && Ws && bs && wh && scratch && t >= 0 && t < tr->T, "gridtd_fwd_attention: bad arguments");
    const GridFwd g = to_fwd(tr);
    hipLaunchKernelGGL(gridtd_fwd_att_scores_kernel, dim3(tr->B, (tr->P + ATT_PB - 1) / ATT_PB), dim3(256),
                       (size_t)2 * tr->H * sizeof(float), (hipStream_t)stream, g, t, att_img, Wg, Ws, bs, wh, scratch, sg);
    LRPX_TRY(check_launch("gridtd_fwd_att_scores"));
    hipLaunchKernelGGL(gridtd_fwd_att_context_kernel, dim3(tr->B, (tr->H + ATT_CB - 1) / ATT_CB), dim3(256),
                       (size_t)((2 * tr->P + 1 > 256 ? 2 * tr->P + 1 : 256) + 8) * sizeof(float), (hipStream_t)stream, g, t, Vp,
                       wh, scratch);
    return check_launch("gridtd_fwd_att_context");
}

static GridRel to_rel(const lrpx_gridtd_trace* t, const lrpx_gridtd_relstate* r) {
    GridRel g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P; g.lens = r->lens;
    g.xh1 = t->xh1; g.xh2 = t->xh2; g.h2 = t->h2; g.c1 = t->c1; g.c2 = t->c2;
    g.g1 = t->g1; g.i1 = t->i1; g.f1 = t->f1; g.g2 = t->g2; g.i2 = t->i2; g.f2 = t->f2;
    g.s = t->s; g.ctx = t->ctx; g.ctx_hat = t->ctx_hat; g.hc = t->hc; g.beta = t->beta;
    g.r_h2n = r->r_h2n; g.r_c2 = r->r_c2; g.r_c1 = r->r_c1; g.r_ch0 = r->r_ch0; g.r_h2p = r->r_h2p; g.r_glob = r->r_glob;
    g.A = r->A; g.rx = r->rx; g.wacc = r->wacc; g.r_words = r->r_words;
    return g;
}

static int check_rel(const lrpx_gridtd_trace* t, const lrpx_gridtd_relstate* r) {
    LRPX_TRY(check_trace(t));
    LRPX_REQUIRE(r && r->r_h2n && r->r_c2 && r->r_c1 && r->r_ch0 && r->r_h2p && r->r_glob && r->A && r->rx && r->wacc &&
                     r->r_words, "gridtd: null relevance-state tensor");
    return LRPX_OK;
}

// both entries of the pixel rule: `mean` - with r_avg / avg, the <true> instantiation of the kernel
static int launch_gridtd_rel_pix(bool mean, const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* Vp, const float* proj_pre,
                                 const float* r_avg, const float* avg, float* a_proj, const int32_t* rows, int n_rows, void* stream) {
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(Vp && proj_pre && a_proj && (!mean || (r_avg && avg)), "gridtd_rel_pix: null pointer");
    LRPX_REQUIRE(rows ? (n_rows > 0 && n_rows <= tr->B * tr->T) : n_rows == tr->B * tr->T, "gridtd_rel_pix: bad row list");
    const int kchunk = 28;
    const size_t lds = (size_t)tr->T * kchunk * sizeof(float);
    hipLaunchKernelGGL(mean ? gridtd_rel_pix_kernel<true> : gridtd_rel_pix_kernel<false>, dim3(n_rows, (tr->P + kchunk - 1) / kchunk),
                       dim3(256), lds, (hipStream_t)stream, to_rel(tr, rs), Vp, proj_pre, tr->alpha, a_proj, kchunk, rows, r_avg, avg);
    return check_launch("gridtd_rel_pix");
}

static GridGrad to_grad(const lrpx_gridtd_trace* t, const lrpx_gridtd_gradstate* r) {
    GridGrad g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P; g.lens = r->lens;
    g.c1 = t->c1; g.c2 = t->c2; g.g1 = t->g1; g.i1 = t->i1; g.f1 = t->f1; g.o1 = t->o1;
    g.g2 = t->g2; g.i2 = t->i2; g.f2 = t->f2; g.o2 = t->o2; g.sgate = t->sgate; g.beta = t->beta;
    g.d_h2n = r->d_h2n; g.d_c2 = r->d_c2; g.d_c1 = r->d_c1; g.d_ch0 = r->d_ch0; g.d_h2p = r->d_h2p; g.d_glob = r->d_glob;
    g.gates = r->gates; g.dx = r->dx; g.wacc = r->wacc; g.r_words = r->r_words;
    return g;
}

static int check_grad(const lrpx_gridtd_trace* t, const lrpx_gridtd_gradstate* r) {
    LRPX_TRY(check_trace(t));
    LRPX_REQUIRE(t->o1 && t->o2 && t->sgate, "gridtd_grad: the trace must carry o1/o2/sgate (gradient-explainer trace)");
    LRPX_REQUIRE(t->E == t->H, "gridtd_grad: embed_dim must equal hidden_dim");
    LRPX_REQUIRE(r && r->d_h2n && r->d_c2 && r->d_c1 && r->d_ch0 && r->d_h2p && r->d_glob && r->gates && r->dx && r->wacc &&
                     r->r_words, "gridtd_grad: null state tensor");
    return LRPX_OK;
}

template <int RT>
static int gridtd_fused_steps(const lrpx_gridtd_trace* tr, int t0, int t1, const lrpx_gridtd_step_args* a, hipStream_t st) {
    const GridFwd g = to_fwd(tr);
    const int H = tr->H;
    for (int t = t0; t < t1; ++t) {
        hipLaunchKernelGGL((gridtd_linear_lstm_kernel<RT, 1>), dim3(H / 4 + H / 16), dim3(256), 0, st, g, t, a->w_il1, a->b_il1, a->w_cat1,
                           a->b_cat1, a->zz1, a->glob, a->emb, a->tok, a->tok_ld);
        LRPX_TRY(check_launch("gridtd_linear_lstm1"));
        LRPX_TRY(gridtd_attention(tr, t, a->Vp, a->att_img, a->Wg, a->Ws, a->bs, a->wh, a->att_scratch, a->zz1, st));
        hipLaunchKernelGGL((gridtd_linear_lstm_kernel<RT, 2>), dim3(H / 4), dim3(256), 0, st, g, t, a->w_il2, a->b_il2, a->w_cat2, a->b_cat2,
                           a->zz1, a->glob, a->emb, a->tok, a->tok_ld);
        LRPX_TRY(check_launch("gridtd_linear_lstm2"));
    }
    return LRPX_OK;
}

extern "C" {

int lrpx_gridtd_fwd_pre(const lrpx_gridtd_trace* tr, int t, const float* glob, const float* emb, const long long* tok,
                        int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_fwd_pre", {glob, "glob"}, {emb, "emb"}, {tok, "tok"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(glob && emb && tok && t >= 0 && t < tr->T, "gridtd_fwd_pre: bad arguments");
    hipLaunchKernelGGL(gridtd_fwd_pre_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_fwd(tr), t, glob, emb,
                       tok, tok_ld);
    return check_launch("gridtd_fwd_pre");
}

int lrpx_gridtd_fwd_gate_input(const lrpx_gridtd_trace* tr, int t, float* xg, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_fwd_gate_input", {xg, "xg"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(xg && t >= 0 && t < tr->T, "gridtd_fwd_gate_input: bad arguments");
    hipLaunchKernelGGL(gridtd_gate_input_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_fwd(tr), t, xg);
    return check_launch("gridtd_fwd_gate_input");
}

int lrpx_gridtd_fwd_sentinel(const lrpx_gridtd_trace* tr, int t, const float* zg, int ldz, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_fwd_sentinel", {zg, "zg"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(zg && ldz >= tr->H && t >= 0 && t < tr->T, "gridtd_fwd_sentinel: bad arguments");
    hipLaunchKernelGGL(gridtd_sentinel_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_fwd(tr), t, zg, ldz);
    return check_launch("gridtd_fwd_sentinel");
}

int lrpx_gridtd_lrp_reweight(const lrpx_gridtd_trace* tr, int t, const float* pred, long ld, int V, const float* fc_w,
                             const unsigned char* skip, float* hcw, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_lrp_reweight", {pred, "pred"}, {fc_w, "fc_w"}, {skip, "skip"}, {hcw, "hcw"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(pred && fc_w && skip && hcw && V > 0 && ld >= V && t >= 0 && t < tr->T,
                 "gridtd_lrp_reweight: bad arguments");
    // the kernel is decoder_blocks.hip's: the two fc summands are h2[t + 1] and ctx_hat[t] of the trace.  Everything that entry refuses
    // has been refused above under this entry's own message (B > 0, H == 512 and both row strides >= H follow from check_trace)
    return lrpx_lrp_reweight_rows(pred, ld, V, tr->h2 + (long)(t + 1) * tr->H, (long)(tr->T + 1) * tr->H, tr->ctx_hat + (long)t * tr->H,
                                  (long)tr->T * tr->H, fc_w, skip, hcw, tr->B, tr->H, 0, stream);
}

int lrpx_gridtd_fwd_lstm(const lrpx_gridtd_trace* tr, int t, const float* zz, int ldz, int which, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_fwd_lstm", {zz, "zz"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(zz && (which == 1 || which == 2) && t >= 0 && t < tr->T, "gridtd_fwd_lstm: bad arguments");
    hipLaunchKernelGGL(gridtd_fwd_lstm_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_fwd(tr), t, zz, ldz,
                       which);
    return check_launch("gridtd_fwd_lstm");
}

int lrpx_gridtd_fwd_attention(const lrpx_gridtd_trace* tr, int t, const float* Vp, const float* att_img,
                              const float* Wg, const float* Ws, const float* bs, const float* wh, float* scratch,
                              void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_fwd_attention", {Vp, "Vp"}, {att_img, "att_img"}, {Wg, "Wg"}, {Ws, "Ws"}, {bs, "bs"}, {wh, "wh"}, {scratch, "scratch"});
    return gridtd_attention(tr, t, Vp, att_img, Wg, Ws, bs, wh, scratch, nullptr, stream);
}

int lrpx_gridtd_rel_init(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* fcw,
                         const float* logit, const long long* tok, int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_rel_init", {fcw, "fcw"}, {logit, "logit"}, {tok, "tok"});
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(fcw && logit && tok, "gridtd_rel_init: null pointer");
    hipLaunchKernelGGL(gridtd_rel_init_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_rel(tr, rs),
                       fcw, logit, tok, tok_ld);
    return check_launch("gridtd_rel_init");
}

int lrpx_gridtd_rel_step(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, int s, int phase, void* stream) {
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(s >= 0 && s < tr->T && phase >= 0 && phase <= 3, "gridtd_rel_step: bad step/phase");
    const GridRel g = to_rel(tr, rs);
    const dim3 grid(tr->B * tr->T), blk(256);
    if (phase == 0) hipLaunchKernelGGL(gridtd_rel_a_kernel, grid, blk, 0, (hipStream_t)stream, g, s);
    else if (phase == 1) hipLaunchKernelGGL(gridtd_rel_b_kernel, grid, blk, 0, (hipStream_t)stream, g, s);
    else if (phase == 2) hipLaunchKernelGGL(gridtd_rel_c_kernel, grid, blk, 0, (hipStream_t)stream, g, s);
    else hipLaunchKernelGGL(gridtd_rel_ca_kernel, grid, blk, 0, (hipStream_t)stream, g, s);       // 3: phase 2 of s + phase 0 of s + 1
    return check_launch("gridtd_rel_step");
}

int lrpx_gridtd_rel_glob(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* glob_pre,
                         float* a_glob, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_rel_glob", {glob_pre, "glob_pre"}, {a_glob, "a_glob"});
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(glob_pre && a_glob, "gridtd_rel_glob: null pointer");
    hipLaunchKernelGGL(gridtd_rel_glob_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_rel(tr, rs),
                       glob_pre, a_glob);
    return check_launch("gridtd_rel_glob");
}

int lrpx_gridtd_rel_pix_rows(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* Vp,
                             const float* proj_pre, float* a_proj, const int32_t* rows, int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_rel_pix_rows", {Vp, "Vp"}, {proj_pre, "proj_pre"}, {a_proj, "a_proj"}, {rows, "rows"});
    return launch_gridtd_rel_pix(false, tr, rs, Vp, proj_pre, nullptr, nullptr, a_proj, rows, n_rows, stream);
}

int lrpx_gridtd_rel_pix_rows_avg(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* Vp,
                                 const float* proj_pre, const float* r_avg, const float* avg, float* a_proj, const int32_t* rows,
                                 int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_rel_pix_rows_avg", {Vp, "Vp"}, {proj_pre, "proj_pre"}, {r_avg, "r_avg"}, {avg, "avg"},
                        {a_proj, "a_proj"}, {rows, "rows"});
    return launch_gridtd_rel_pix(true, tr, rs, Vp, proj_pre, r_avg, avg, a_proj, rows, n_rows, stream);
}

int lrpx_gridtd_rel_pix(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* Vp,
                        const float* proj_pre, float* a_proj, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_rel_pix", {Vp, "Vp"}, {proj_pre, "proj_pre"}, {a_proj, "a_proj"});
    LRPX_REQUIRE(tr, "gridtd_rel_pix: null trace");
    return lrpx_gridtd_rel_pix_rows(tr, rs, Vp, proj_pre, a_proj, nullptr, tr->B * tr->T, stream);
}

int lrpx_gridtd_grad_init(const lrpx_gridtd_trace* tr, const lrpx_gridtd_gradstate* gs, const float* fcw,
                          const long long* tok, int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_grad_init", {fcw, "fcw"}, {tok, "tok"});
    LRPX_TRY(check_grad(tr, gs));
    LRPX_REQUIRE(fcw && tok, "gridtd_grad_init: null pointer");
    hipLaunchKernelGGL(gridtd_grad_init_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_grad(tr, gs),
                       fcw, tok, tok_ld);
    return check_launch("gridtd_grad_init");
}

int lrpx_gridtd_grad_step(const lrpx_gridtd_trace* tr, const lrpx_gridtd_gradstate* gs, int s, int phase, void* stream) {
    LRPX_TRY(check_grad(tr, gs));
    LRPX_REQUIRE(s >= 0 && s < tr->T && phase >= 0 && phase <= 2, "gridtd_grad_step: bad step/phase");
    const GridGrad g = to_grad(tr, gs);
    const dim3 grid(tr->B * tr->T), blk(256);
    if (phase == 0) hipLaunchKernelGGL(gridtd_grad_a_kernel, grid, blk, 0, (hipStream_t)stream, g, s);
    else if (phase == 1) hipLaunchKernelGGL(gridtd_grad_b_kernel, grid, blk, 0, (hipStream_t)stream, g, s);
    else hipLaunchKernelGGL(gridtd_grad_c_kernel, grid, blk, 0, (hipStream_t)stream, g, s);
    return check_launch("gridtd_grad_step");
}

// ---- the host loops of the gridTD decoder in native code (round 5; as lrpx_aoa_fwd_steps / lrpx_aoa_rel_steps for the AoA decoder): every
// launch is one of the entry points above, what goes away is the interpreter between them (~4 us per call through ctypes against ~1.5 us
// from here): 7 x T + 5 x T calls per explanation - a third of the 5 ms one image costs through the drop-in class
int lrpx_gridtd_fwd_steps(const lrpx_gridtd_trace* tr, int t0, int t1, const lrpx_gridtd_step_args* a, void* stream) {
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(a && a->glob && a->emb && a->tok && a->w_cat1 && a->b_cat1 && a->w_cat2 && a->b_cat2 && a->Vp && a->att_img && a->Wg &&
                     a->Ws && a->bs && a->wh && a->zz1 && a->zz2 && a->att_scratch && t0 >= 0 && t0 <= t1 && t1 <= tr->T,
                 "gridtd_fwd_steps: bad arguments");
    const int B = tr->B, T = tr->T, H = tr->H, E = tr->E, W1 = 2 * E + 2 * H;
    // fused steps (4 launches instead of 7): interleaved gate rows given, <= 64 images, dims the matrix-core linear takes
    if (a->w_il1 && a->b_il1 && a->w_il2 && a->b_il2 && B <= 64 && W1 % 16 == 0 && H % 16 == 0 && t0 < t1) {
        LRPX_TRY(lrpx_gridtd_fwd_pre(tr, t0, a->glob, a->emb, a->tok, a->tok_ld, stream));      // (later rows: written by the step before)
        hipStream_t st = (hipStream_t)stream;
        return with_row_tiles(B, [&](auto rt) { return gridtd_fused_steps<decltype(rt)::value>(tr, t0, t1, a, st); });
    }
    for (int t = t0; t < t1; ++t) {
        LRPX_TRY(lrpx_gridtd_fwd_pre(tr, t, a->glob, a->emb, a->tok, a->tok_ld, stream));
        LRPX_TRY(lrpx_linear_small(tr->xh1 + (long)t * W1, (long)T * W1, a->w_cat1, a->b_cat1, a->zz1, 5 * H, B, W1, 5 * H, 0, stream));
        LRPX_TRY(lrpx_gridtd_fwd_lstm(tr, t, a->zz1, 5 * H, 1, stream));
        LRPX_TRY(lrpx_gridtd_fwd_attention(tr, t, a->Vp, a->att_img, a->Wg, a->Ws, a->bs, a->wh, a->att_scratch, stream));
        LRPX_TRY(lrpx_linear_small(tr->xh2 + (long)t * 3 * H, (long)T * 3 * H, a->w_cat2, a->b_cat2, a->zz2, 4 * H, B, 3 * H, 4 * H, 0, stream));
        LRPX_TRY(lrpx_gridtd_fwd_lstm(tr, t, a->zz2, 4 * H, 2, stream));
    }
    return LRPX_OK;
}

int lrpx_gridtd_rel_steps(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, int n_steps, const lrpx_conv_desc* dense2,
                          const lrpx_conv_desc* dense1, const int32_t* idx, int idx_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_gridtd_rel_steps", {idx, "idx"});
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(dense1 && dense2 && idx && n_steps >= 0 && n_steps <= tr->T && idx_ld >= tr->B * tr->T, "gridtd_rel_steps: bad arguments");
    lrpx_conv_desc d2 = *dense2, d1 = *dense1;
    for (int s = 0; s < n_steps; ++s) {
        d2.map2img = d1.map2img = idx + (long)s * idx_ld;      // row -> source row of the multiplicands at lock-step s
        if (s == 0) LRPX_TRY(lrpx_gridtd_rel_step(tr, rs, s, 0, stream));
        LRPX_TRY(lrpx_conv_mfma(&d2, stream));
        LRPX_TRY(lrpx_gridtd_rel_step(tr, rs, s, 1, stream));
        LRPX_TRY(lrpx_conv_mfma(&d1, stream));
        // the tail of lock-step s and the head of s + 1 in one launch
        LRPX_TRY(lrpx_gridtd_rel_step(tr, rs, s, s + 1 < n_steps ? 3 : 2, stream));
    }
    return LRPX_OK;
}

}  // extern "C"
