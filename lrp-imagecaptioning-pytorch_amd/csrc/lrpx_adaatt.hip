// The single-LSTM adaptive-attention model (models/adaptiveattention.py): decoder trace and LRP relevance recursion.
//
// Model (:101-135): x_t = [emb(word_t) | glob], one `AdaLSTM` cell on (x_t, h, c), sentinel s = sigmoid(x_gate(x_t) + h_gate(h_OLD)) tanh(c_t)
// (:48-53), `AdaptiveAttention` on (V, h_t, s_t) (:56-98, gridTD's module), scores fc(ctx_hat + h_t).  The recurrence reads h only - the
// attention feeds nothing back -, so under teacher forcing the input half of the five gate rows of every (image, word) is one GEMM, the
// serial part is ONE launch of K = H per time step (cell and sentinel in its epilogue), and the attention runs once over all B*T rows.
// Explainer (`ExplainAdaptiveAttention.explain_caption_wordt`, :679-771): sentinel and context take relevance at the explained word only
// (the context never feeds the LSTM), the gate rule divides by tanh OF the pre-activation (:737), the glob columns count at i == t only
// (:740-741), the two image-side rules divide by BIAS-FREE pre-activations (:536-537).
//
// Row layout of xh, [B][T][H + 2E]:  [h[t] | emb(word_t) | glob]  - the reference's xh = [emb | glob | h] (:688) with the h columns first,
// so that the columns of a lock-step s >= 1 that are ever read (h, emb) are the first H + E of the gate rule's output.
// Row r = b*T + t is the explanation of word t of image b; at lock-step s a row with t >= s works on time index i = t - s.
#include "common.h"
#include "conv_mfma.h"
#include "conv_launch.h"
#include "decoder_shared.h"

namespace lrpx {

struct AdaFwd {
    int B, T, H, E, P;
    float* xh;                                 // [B][T][H+2E]
    float *h, *c;                              // [B][T+1][H]
    float *g, *i, *f, *s, *ctx, *ctx_hat, *hc; // [B][T][H]
    float *alpha, *beta;                       // [B][T][P], [B][T]
    float *o, *sgate;                          // optional [B][T][H]
};

// gate rows interleaved in groups of 16: row 16 j + 5 u + q = gate q (i, f, g, o, sentinel gate) of hidden unit 3 j + u, u < 3; row 16 j + 15
// is padding (zero weights).  One workgroup of the recurrence owns the five rows of its three hidden units.
constexpr int ADA_UPG = 3;                                                       // hidden units per 16-row group
__host__ __device__ inline int ada_groups(int H) { return (H + ADA_UPG - 1) / ADA_UPG; }

// x columns of the input rows: xh[b, t][H:] = [emb[tok[b, t]] | glob[b]].  t < 0: every (image, word) row, grid B*T; t >= 0: the rows of
// step t, grid B, and the h columns too (xh[b, t][:H] = h[b, t]: the decoding loops reorder h between steps)
__global__ void adaatt_fwd_inputs_kernel(AdaFwd g, int t, const float* __restrict__ glob, const float* __restrict__ emb,
                                         const long long* __restrict__ tok, int tok_ld) {
    const int b = t < 0 ? blockIdx.x / g.T : blockIdx.x, tt = t < 0 ? blockIdx.x - b * g.T : t;
    const int H = g.H, E = g.E, W = H + 2 * E;
    float* dst = g.xh + ((long)b * g.T + tt) * W;
    const long long k = tok[(long)b * tok_ld + tt];
    for (int c = threadIdx.x + (t < 0 ? H : 0); c < W; c += blockDim.x) {
        float v;
        if (c < H) v = g.h[((long)b * (g.T + 1) + tt) * H + c];
        else if (c < H + E) v = emb[k * E + (c - H)];
        else v = glob[(long)b * E + (c - H - E)];
        dst[c] = v;
    }
}

// the cell and the sentinel from the five pre-activations of one hidden unit (:554-565, :603-604)
__device__ __forceinline__ void adaatt_cell(const AdaFwd& g, int b, int t, int c, const float (&z)[5]) {
    const int H = g.H;
    const long st0 = ((long)b * (g.T + 1) + t) * H, st1 = st0 + H, tr = ((long)b * g.T + t) * H;
    const LstmCell l = lstm_cell(z[0], z[1], z[2], z[3], g.c[st0 + c]);
    const float sg = sigmoidf_(z[4]);
    const float tc = tanhf(l.cn);
    const float hn = l.o * tc;
    g.c[st1 + c] = l.cn; g.h[st1 + c] = hn;
    g.g[tr + c] = z[2]; g.i[tr + c] = l.i; g.f[tr + c] = l.f;
    g.s[tr + c] = sg * tc;
    if (g.o) g.o[tr + c] = l.o;
    if (g.sgate) g.sgate[tr + c] = sg;
    if (t + 1 < g.T) g.xh[((long)b * g.T + t + 1) * (H + 2 * g.E) + c] = hn;         // the next step's h columns
}

// step t of the decoupled trace: z = zin[b, t] + [W_hh ; h_gate] h[b, t], then cell and sentinel.  w: (16 * groups, H) interleaved as above;
// zin: [B*T][16 * groups] in the same column order, biases included
template <int RT>
__global__ __launch_bounds__(256) void adaatt_rec_kernel(AdaFwd g, int t, const float* __restrict__ w, const float* __restrict__ zin) {
    __shared__ float red[4][RT][16][17];
    const int H = g.H, NR = 16 * ada_groups(H);
    linear_mfma_core<RT>(g.h + (long)t * H, (long)(g.T + 1) * H, w, g.B, H, NR, red, blockIdx.x * 16);
    for (int e = threadIdx.x; e < RT * 16 * ADA_UPG; e += 256) {
        const int r = e / (16 * ADA_UPG), row = (e / ADA_UPG) % 16, u = e % ADA_UPG;
        const int b = r * 16 + row, c = blockIdx.x * ADA_UPG + u;
        if (b >= g.B || c >= H) continue;
        const float* zi = zin + ((long)b * g.T + t) * NR + blockIdx.x * 16;
        float z[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int col = 5 * u + q;
            z[q] = red4<RT>(red, r, row, col) + zi[col];
        }
        adaatt_cell(g, b, t, c, z);
    }
}

// step t of the per-step path (the decoding loops): zz [B][5H] = [W_hh | W_ih ; h_gate | x_gate] xh[b, t] + biases, gates in blocks of H
__global__ void adaatt_fwd_cell_kernel(AdaFwd g, int t, const float* __restrict__ zz, int ldz) {
    const int b = blockIdx.x, H = g.H;
    const float* zr = zz + (long)b * ldz;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float z[5] = {zr[c], zr[H + c], zr[2 * H + c], zr[3 * H + c], zr[4 * H + c]};
        adaatt_cell(g, b, t, c, z);
    }
}

// the attention of decoder_shared.h on (h[t + 1], s[t]).  t < 0: every (image, word) row, grid.x = B*T; t >= 0: the rows of step t, grid.x = B.
// scr: [rows][3P]
__global__ __launch_bounds__(256) void adaatt_att_scores_kernel(AdaFwd g, int t, const float* __restrict__ att_img,
                                                                const float* __restrict__ Wg, const float* __restrict__ Ws,
                                                                const float* __restrict__ bs, const float* __restrict__ wh,
                                                                float* __restrict__ scr) {
    extern __shared__ float sm[];
    const int b = t < 0 ? blockIdx.x / g.T : blockIdx.x, tt = t < 0 ? blockIdx.x - b * g.T : t;
    const int H = g.H, P = g.P;
    float* hv = sm;           // H
    float* sv = hv + H;       // H
    const long st1 = ((long)b * (g.T + 1) + tt + 1) * H, tr = ((long)b * g.T + tt) * H;
    for (int c = threadIdx.x; c < H; c += 256) { hv[c] = g.h[st1 + c]; sv[c] = g.s[tr + c]; }
    __syncthreads();
    att_scores_block(hv, sv, H, P, b, blockIdx.y, att_img, Wg, Ws, bs, wh, scr + (long)blockIdx.x * 3 * P);
}

// ... and its context half; epilogue: ctx, ctx_hat = beta s + (1 - beta) ctx (:97) and the fc input hc = h[t + 1] + ctx_hat (:134)
__global__ __launch_bounds__(256) void adaatt_att_context_kernel(AdaFwd g, int t, const float* __restrict__ Vp,
                                                                 const float* __restrict__ wh, const float* __restrict__ scr) {
    extern __shared__ float sm[];
    const int b = t < 0 ? blockIdx.x / g.T : blockIdx.x, tt = t < 0 ? blockIdx.x - b * g.T : t;
    const int H = g.H, P = g.P, tid = threadIdx.x;
    const long row = (long)b * g.T + tt;
    float a;
    const float beta = att_context_block(scr + (long)blockIdx.x * 3 * P, sm, H, P, b, blockIdx.y, blockIdx.y == 0, Vp, wh,
                                         g.alpha + row * P, g.beta + row, a);
    const int c = blockIdx.y * ATT_CB + (tid & 31), part = tid >> 5;
    if (c < H && part == 0) {
        const long tr = row * H, st1 = ((long)b * (g.T + 1) + tt + 1) * H;
        const float ch = beta * g.s[tr + c] + (1.f - beta) * a;
        g.ctx[tr + c] = a; g.ctx_hat[tr + c] = ch;
        g.hc[tr + c] = g.h[st1 + c] + ch;
    }
}

// ------------------------------------------------------------------------------------------------
// relevance - models/adaptiveattention.py:679-771.  One block (256 threads) per row.
// ------------------------------------------------------------------------------------------------
struct AdaRel {
    int B, T, H, E, P;
    const int* lens;                      // [B] caption length per image (null: T)
    const float *h, *c, *g, *i, *f, *s, *ctx, *ctx_hat, *hc, *alpha, *beta;
    float *r_h, *r_c, *r_ctx;             // [rows][H]   (r_ctx: r_context / z~(ctx_t), the pixel rule's factor)
    float* r_glob;                        // [rows][E]
    float *A, *rx;                        // gate rule in [rows][H], out [rows][H+2E] = [h | emb | glob]
    float* r_words;                       // [rows][T]
};

__device__ __forceinline__ bool ada_row_active(const AdaRel& g, int b, int t, int s) {
    const int len = g.lens ? g.lens[b] : g.T;
    return t < len && t >= s;
}

// the cell split at time index i (:726-734) and the gate rule's prologue: r_c[i] and A = r_g / z~(tanh g[i])  (:737: tanh OF the pre-activation)
__device__ __forceinline__ void ada_cell_split(const AdaRel& g, int b, int i, long tr, int c, float r_h) {
    const int H = g.H;
    const long ti = ((long)b * g.T + i) * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H, sc0 = sc1 - H;
    const float rc = g.r_c[tr + c] + r_h;                                                            // :726
    const float cn = g.c[sc1 + c];
    const float tg = tanhf(g.g[ti + c]);
    const float rg = eps_id(rc, g.i[ti + c] * tg, cn);                                               // :727-730
    g.r_c[tr + c] = eps_id(rc, g.f[ti + c] * g.c[sc0 + c], cn);                                      // :731-734
    g.A[tr + c] = rg / stab_eps(tg);
}

// :700-724 - the one-hot relevance at the target logit through fc, split between h[t + 1] and ctx_hat[t], ctx_hat between context and
// sentinel, r_c[t + 1] = r_s - and the cell split of lock-step 0.  Rows behind an image's last word: zeros in A, r_ctx, r_glob, r_words
__global__ void adaatt_rel_init_kernel(AdaRel g, const float* __restrict__ fcw, const float* __restrict__ logit,
                                       const long long* __restrict__ tok, int tok_ld) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long tr = (long)row * H;
    for (int c = threadIdx.x; c < g.E; c += blockDim.x) g.r_glob[(long)row * g.E + c] = 0.f;
    for (int c = threadIdx.x; c < g.T; c += blockDim.x) g.r_words[(long)row * g.T + c] = 0.f;
    if (!ada_row_active(g, b, t, 0)) {
        for (int c = threadIdx.x; c < H; c += blockDim.x) { g.A[tr + c] = 0.f; g.r_ctx[tr + c] = 0.f; }
        return;
    }
    const long long k = tok[(long)b * tok_ld + t + 1];
    const float lg = logit[row];
    const float zt = stab_eps(lg);
    const long st1 = ((long)b * (g.T + 1) + t + 1) * H;
    const float beta = g.beta[row];
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float hc = g.hc[tr + c], ch = g.ctx_hat[tr + c], cx = g.ctx[tr + c];
        const float r_hc = (fcw[k * H + c] * hc / zt) * lg;                                          // :700-703
        const float r_h = eps_id(r_hc, g.h[st1 + c], hc);                                            // :705-708
        const float r_ch = eps_id(r_hc, ch, hc);                                                     // :710-713
        const float r_cx = eps_id(r_ch, (1.f - beta) * cx, ch);                                      // :714-717
        const float r_s = eps_id(r_ch, beta * g.s[tr + c], ch);                                      // :719-722
        g.r_ctx[tr + c] = r_cx / stab_eps(cx);                                                       // the pixel rule's factor (:756-759)
        g.r_h[tr + c] = r_h;
        g.r_c[tr + c] = r_s;                                                                         // :724
        ada_cell_split(g, b, t, tr, c, r_h);
    }
}

// behind the gate rule of lock-step s: r_h[i] = rx[:H] (:739), r_words[i] = sum rx[H:H+E] (:742, :764), r_glob = rx[H+E:] at s == 0 only
// (:740-741) - and the cell split of lock-step s + 1 (a thread owns the same channels in both: the r_h it writes is the one it reads)
__global__ __launch_bounds__(256) void adaatt_rel_ca_kernel(AdaRel g, int s) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, E = g.E;
    const long tr = (long)row * H;
    if (!ada_row_active(g, b, t, s)) {                 // (then not active at s + 1 either)
        for (int c = threadIdx.x; c < H; c += 256) g.A[tr + c] = 0.f;
        return;
    }
    const int i = t - s;
    const float* rx = g.rx + (long)row * (H + 2 * E);
    const bool nxt = ada_row_active(g, b, t, s + 1);
    for (int c = threadIdx.x; c < H; c += 256) {
        const float r_h = rx[c];
        g.r_h[tr + c] = r_h;
        if (nxt) ada_cell_split(g, b, i - 1, tr, c, r_h);
        else g.A[tr + c] = 0.f;
    }
    float acc = 0.f;
    for (int c = threadIdx.x; c < E; c += 256) {
        acc += rx[H + c];
        if (s == 0) g.r_glob[(long)row * E + c] = rx[H + E + c];
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) g.r_words[(long)row * g.T + i] = acc;
}

// :743-746 prologue: A_glob = r_glob / z~(glob_nb), glob_nb the BIAS-FREE pre-activation of global_img_feature_proj (:536-537)
__global__ void adaatt_rel_glob_kernel(AdaRel g, const float* __restrict__ glob_nb, float* __restrict__ Aglob) {
    const int row = blockIdx.x, b = row / g.T;
    for (int c = threadIdx.x; c < g.E; c += blockDim.x)
        Aglob[(long)row * g.E + c] = g.r_glob[(long)row * g.E + c] / stab_eps(glob_nb[(long)b * g.E + c]);
}

// :756-763: Aproj[row][k][c] = Vp[b][k][c] * alpha[b][t][k] * (r_ctx / z~(ctx_t))[row][c] / z~(proj_nb[b][k][c]) - the context takes
// relevance at the explained word only: no sum over time steps.  rowlist: workgroup x computes row rowlist[x], written as row x (compact)
__global__ __launch_bounds__(256) void adaatt_rel_pix_kernel(AdaRel g, const float* __restrict__ Vp, const float* __restrict__ proj_nb,
                                                             float* __restrict__ Aproj, int kchunk, const int* __restrict__ rowlist) {
    const int row = rowlist ? rowlist[blockIdx.x] : blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, P = g.P;
    const long orow = blockIdx.x;
    const bool act = ada_row_active(g, b, t, 0);
    const int k0 = blockIdx.y * kchunk, k1 = min(k0 + kchunk, P);
    for (int c = threadIdx.x; c < H; c += 256) {
        const float rc = act ? g.r_ctx[(long)row * H + c] : 0.f;
        for (int k = k0; k < k1; ++k) {
            const long pi = ((long)b * P + k) * H + c;
            Aproj[(orow * P + k) * H + c] = act ? Vp[pi] * (g.alpha[(long)row * P + k] * rc) / stab_eps(proj_nb[pi]) : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
static AdaFwd to_fwd(const lrpx_adaatt_trace* t) {
    AdaFwd g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P;
    g.xh = t->xh; g.h = t->h; g.c = t->c; g.g = t->g; g.i = t->i; g.f = t->f; g.s = t->s; g.ctx = t->ctx; g.ctx_hat = t->ctx_hat;
    g.hc = t->hc; g.alpha = t->alpha; g.beta = t->beta; g.o = t->o; g.sgate = t->sgate;
    return g;
}

static int check_trace(const lrpx_adaatt_trace* t) {
    LRPX_REQUIRE(t && t->B > 0 && t->T > 0 && t->H == 512 && t->E > 0 && t->E % 16 == 0 && t->P > 0 && t->P <= 256,
                 "adaatt: unsupported trace dims (H must be 512, E %% 16 == 0, P <= 256)");
    LRPX_REQUIRE(t->xh && t->h && t->c && t->g && t->i && t->f && t->s && t->ctx && t->ctx_hat && t->hc && t->alpha && t->beta,
                 "adaatt: null trace tensor");
    return LRPX_OK;
}

// images b0 .. b0 + nb - 1 of a trace
static lrpx_adaatt_trace slice(const lrpx_adaatt_trace* tr, int b0, int nb) {
    lrpx_adaatt_trace s = *tr;
    const long T = tr->T, H = tr->H, W = tr->H + 2L * tr->E;
    s.B = nb;
    s.xh += b0 * T * W;
    s.h += b0 * (T + 1) * H; s.c += b0 * (T + 1) * H;
    s.g += b0 * T * H; s.i += b0 * T * H; s.f += b0 * T * H; s.s += b0 * T * H;
    s.ctx += b0 * T * H; s.ctx_hat += b0 * T * H; s.hc += b0 * T * H;
    s.alpha += b0 * T * tr->P; s.beta += b0 * T;
    if (s.o) s.o += b0 * T * H;
    if (s.sgate) s.sgate += b0 * T * H;
    return s;
}

static int attention(const lrpx_adaatt_trace* tr, int t, const float* Vp, const float* att_img, const float* Wg, const float* Ws,
                     const float* bs, const float* wh, float* scratch, hipStream_t st) {
    const AdaFwd g = to_fwd(tr);
    const unsigned rows = t < 0 ? tr->B * tr->T : tr->B;
    hipLaunchKernelGGL(adaatt_att_scores_kernel, dim3(rows, (tr->P + ATT_PB - 1) / ATT_PB), dim3(256), (size_t)2 * tr->H * sizeof(float), st,
                       g, t, att_img, Wg, Ws, bs, wh, scratch);
    LRPX_TRY(check_launch("adaatt_att_scores"));
    hipLaunchKernelGGL(adaatt_att_context_kernel, dim3(rows, (tr->H + ATT_CB - 1) / ATT_CB), dim3(256),
                       (size_t)((2 * tr->P + 1 > 256 ? 2 * tr->P + 1 : 256) + 8) * sizeof(float), st, g, t, Vp, wh, scratch);
    return check_launch("adaatt_att_context");
}

static AdaRel to_rel(const lrpx_adaatt_trace* t, const lrpx_adaatt_relstate* r) {
    AdaRel g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P;
    g.lens = r->lens;
    g.h = t->h; g.c = t->c; g.g = t->g; g.i = t->i; g.f = t->f; g.s = t->s; g.ctx = t->ctx; g.ctx_hat = t->ctx_hat; g.hc = t->hc;
    g.alpha = t->alpha; g.beta = t->beta;
    g.r_h = r->r_h; g.r_c = r->r_c; g.r_ctx = r->r_ctx; g.r_glob = r->r_glob; g.A = r->A; g.rx = r->rx; g.r_words = r->r_words;
    return g;
}

static int check_rel(const lrpx_adaatt_trace* t, const lrpx_adaatt_relstate* r) {
    LRPX_TRY(check_trace(t));
    LRPX_REQUIRE(r && r->r_h && r->r_c && r->r_ctx && r->r_glob && r->A && r->rx && r->r_words, "adaatt: null relevance state tensor");
    return LRPX_OK;
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

int lrpx_adaatt_fwd_inputs(const lrpx_adaatt_trace* tr, const float* glob, const float* emb, const long long* tok, int tok_ld,
                           void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_fwd_inputs", {glob, "glob"}, {emb, "emb"}, {tok, "tok"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(glob && emb && tok && tok_ld >= tr->T, "adaatt_fwd_inputs: bad arguments");
    hipLaunchKernelGGL(adaatt_fwd_inputs_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_fwd(tr), -1, glob, emb, tok,
                       tok_ld);
    return check_launch("adaatt_fwd_inputs");
}

int lrpx_adaatt_fwd_recurrence(const lrpx_adaatt_trace* tr, const float* w_hh_il, const float* zin, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_fwd_recurrence", {w_hh_il, "w_hh_il"}, {zin, "zin"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(w_hh_il && zin, "adaatt_fwd_recurrence: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int H = tr->H, NG = ada_groups(H);
    // more than 64 images: slices of at most 64 through the same kernels (the recurrence is independent per image), so that an image's
    // trace does not depend on the batch it sits in
    for (int b0 = 0; b0 < tr->B; b0 += 64) {
        const lrpx_adaatt_trace sub = slice(tr, b0, tr->B - b0 < 64 ? tr->B - b0 : 64);
        const AdaFwd g = to_fwd(&sub);
        const float* z = zin + (long)b0 * tr->T * 16 * NG;
        for (int t = 0; t < tr->T; ++t) {
            with_row_tiles(sub.B, [&](auto rt) { hipLaunchKernelGGL((adaatt_rec_kernel<decltype(rt)::value>), dim3(NG), dim3(256), 0, st, g, t, w_hh_il, z); });
            LRPX_TRY(check_launch("adaatt_rec"));
        }
    }
    return LRPX_OK;
}

int lrpx_adaatt_fwd_attention_all(const lrpx_adaatt_trace* tr, const float* Vp, const float* att_img, const float* Wg, const float* Ws,
                                  const float* bs, const float* wh, float* scratch, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_fwd_attention_all", {Vp, "Vp"}, {att_img, "att_img"}, {Wg, "Wg"}, {Ws, "Ws"}, {bs, "bs"}, {wh, "wh"},
                        {scratch, "scratch"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(Vp && att_img && Wg && Ws && bs && wh && scratch, "adaatt_fwd_attention_all: null pointer");
    return attention(tr, -1, Vp, att_img, Wg, Ws, bs, wh, scratch, (hipStream_t)stream);
}

int lrpx_adaatt_fwd_pre(const lrpx_adaatt_trace* tr, int t, const float* glob, const float* emb, const long long* tok, int tok_ld,
                        void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_fwd_pre", {glob, "glob"}, {emb, "emb"}, {tok, "tok"});
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(glob && emb && tok && t >= 0 && t < tr->T && tok_ld > t, "adaatt_fwd_pre: bad arguments");
    hipLaunchKernelGGL(adaatt_fwd_inputs_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_fwd(tr), t, glob, emb, tok, tok_ld);
    return check_launch("adaatt_fwd_pre");
}

int lrpx_adaatt_fwd_step(const lrpx_adaatt_trace* tr, int t, const lrpx_adaatt_step_args* a, void* stream) {
    LRPX_TRY(check_trace(tr));
    LRPX_REQUIRE(a && a->w_cat && a->b_cat && a->Vp && a->att_img && a->Wg && a->Ws && a->bs && a->wh && a->zz && a->att_scratch && t >= 0 &&
                     t < tr->T, "adaatt_fwd_step: bad arguments");
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_fwd_step", {a->w_cat, "w_cat"}, {a->b_cat, "b_cat"}, {a->Vp, "Vp"}, {a->att_img, "att_img"},
                        {a->Wg, "Wg"}, {a->Ws, "Ws"}, {a->bs, "bs"}, {a->wh, "wh"}, {a->zz, "zz"}, {a->att_scratch, "att_scratch"});
    const int H = tr->H, W = H + 2 * tr->E;
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < tr->B; b0 += 64) {          // (the skinny linear takes 64 rows on the matrix cores: the same kernel for any batch)
        const int nb = tr->B - b0 < 64 ? tr->B - b0 : 64;
        LRPX_TRY(lrpx_linear_small(tr->xh + ((long)b0 * tr->T + t) * W, (long)tr->T * W, a->w_cat, a->b_cat, a->zz + (long)b0 * 5 * H, 5 * H, nb,
                                   W, 5 * H, 0, stream));
    }
    hipLaunchKernelGGL(adaatt_fwd_cell_kernel, dim3(tr->B), dim3(256), 0, st, to_fwd(tr), t, a->zz, 5 * H);
    LRPX_TRY(check_launch("adaatt_fwd_cell"));
    return attention(tr, t, a->Vp, a->att_img, a->Wg, a->Ws, a->bs, a->wh, a->att_scratch, st);
}

int lrpx_adaatt_rel_init(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, const float* fcw, const float* logit,
                         const long long* tok, int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_rel_init", {fcw, "fcw"}, {logit, "logit"}, {tok, "tok"});
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(fcw && logit && tok && tok_ld > tr->T, "adaatt_rel_init: bad arguments");
    hipLaunchKernelGGL(adaatt_rel_init_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_rel(tr, rs), fcw, logit, tok,
                       tok_ld);
    return check_launch("adaatt_rel_init");
}

int lrpx_adaatt_rel_steps(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, int n_steps, const lrpx_conv_desc* dense,
                          const int32_t* idx, int idx_ld, int cut_dead_columns, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_rel_steps", {idx, "idx"});
    LRPX_TRY(check_rel(tr, rs));
    const int H = tr->H, E = tr->E, W = H + 2 * E, rows = tr->B * tr->T;
    LRPX_REQUIRE(dense && idx && n_steps >= 0 && n_steps <= tr->T && idx_ld >= rows, "adaatt_rel_steps: bad arguments");
    LRPX_REQUIRE(dense->taps == 1 && dense->epi == EPI_REL && dense->in == rs->A && dense->out0 == rs->rx && !dense->out1 && dense->x == tr->xh &&
                     !dense->u && dense->cin == H && dense->n_oc == W && dense->oc_split == W && dense->n_maps == rows && dense->pix_per_map == 1 &&
                     !dense->f16x3 && !dense->bf16x6 && (H + E) % 32 == 0,
                 "adaatt_rel_steps: the gate rule is the fp32 epsilon rule A (rows x H) -> rx (rows x (H + 2E)) with x = the trace's xh");
    lrpx_conv_desc d = *dense;
    const AdaRel g = to_rel(tr, rs);
    for (int s = 0; s < n_steps; ++s) {
        d.map2img = idx + (long)s * idx_ld;                 // row -> source row of the multiplicand at lock-step s
        // the glob columns [H + E, H + 2E) are read at s == 0 only (:740-741): later lock-steps contract the first H + E columns (the weights
        // are packed per 32-column block, rows and the output keep their stride W: a live column's sum is the same either way)
        d.n_oc = (cut_dead_columns && s >= 1) ? H + E : W;
        LRPX_TRY(lrpx_conv_mfma(&d, stream));
        hipLaunchKernelGGL(adaatt_rel_ca_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, g, s);
        LRPX_TRY(check_launch("adaatt_rel_ca"));
    }
    return LRPX_OK;
}

int lrpx_adaatt_rel_glob(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, const float* glob_nb, float* a_glob, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_rel_glob", {glob_nb, "glob_nb"}, {a_glob, "a_glob"});
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(glob_nb && a_glob, "adaatt_rel_glob: null pointer");
    hipLaunchKernelGGL(adaatt_rel_glob_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_rel(tr, rs), glob_nb, a_glob);
    return check_launch("adaatt_rel_glob");
}

int lrpx_adaatt_rel_pix_rows(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, const float* Vp, const float* proj_nb,
                             float* a_proj, const int32_t* rows, int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaatt_rel_pix_rows", {Vp, "Vp"}, {proj_nb, "proj_nb"}, {a_proj, "a_proj"}, {rows, "rows"});
    LRPX_TRY(check_rel(tr, rs));
    LRPX_REQUIRE(Vp && proj_nb && a_proj && n_rows > 0 && n_rows <= tr->B * tr->T && (rows || n_rows == tr->B * tr->T),
                 "adaatt_rel_pix_rows: bad arguments (without a row list n_rows must be B*T)");
    const int kchunk = 28;
    hipLaunchKernelGGL(adaatt_rel_pix_kernel, dim3(n_rows, (tr->P + kchunk - 1) / kchunk), dim3(256), 0, (hipStream_t)stream, to_rel(tr, rs),
                       Vp, proj_nb, a_proj, kchunk, rows);
    return check_launch("adaatt_rel_pix");
}

}  // extern "C"
