// The single-LSTM adaptive-attention model (models/adaptiveattention.py): decoder back-pass of the gradient family -
// `ExplainAdaptiveGradient.explain_caption_wordt` (:965-1021); the decoder part of `ExplainiAdaptiveGuidedGradient` (:1100-1157) is the
// same function (its two masks select nothing: :1130 tests ReLU outputs for < 0, :1148 comes after d_average_img_feature is formed), and
// `ExplainAdaptiveGradCam` inherits it.  alpha, beta and the sentinel gate are constants.  Per explained word t of image b:
//
//     d_h   = fc.weight[caption[b, t+1]]                                   :987, :992
//     d_ctx = (1 - beta_t) d_h                                             :989
//     d_c   = beta_t d_h * sgate_t * (1 - tanh^2 c[t+1])                   :990-991
//     for i = t .. 0:                                                      :995-1010
//         tc  = tanh c[i+1];  d_c += d_h * o_i * (1 - tc^2)
//         G_i = [ d_c tanh(g_i) i_i (1 - i_i) | d_c c[i] f_i (1 - f_i) | d_c i_i (1 - tanh^2 g_i) | d_h tc o_i (1 - o_i) ]      (4H: i f g o)
//         d_c = d_c * f_i;   d_h = G_i W_hh
//         d_x = G_i W_ih;    r_words[i] = sum of d_x[:E];   d_glob += d_x[E:]
//
// Only d_h = G_i W_hh is serial.  By linearity r_words[i] = G_i . wsum (wsum[k] = sum_{e < E} W_ih[k, e]) and d_glob = (sum_i G_i) W_ih[:, E:],
// so a lock-step is ONE launch: the product over K = 4H on a transposed copy of W_hh ((H, 4H): row j = column j of W_hh) and, in its epilogue,
// the point-wise cell back-step of the workgroup's own 16 hidden units - the LSTM back-step is per hidden unit, the epilogue needs nothing
// from another workgroup.  G is ping-ponged between two buffers: every workgroup reads all 4H columns of the previous lock-step's.
// Row r = b*T + t runs in lock-step with all others: at lock-step s it works on time index i = t - s, active while s <= t < lens[b].
// Sums across workgroups go through per-workgroup partials added by one thread in a fixed order (no float atomics): bit-identical from
// run to run, and a row's values never depend on the batch it sits in (an MFMA row reads its own row of G only).
#include "common.h"
#include "conv_mfma.h"
#include "decoder_shared.h"

namespace lrpx {

constexpr int AG_UNITS = 16;          // hidden units per workgroup of the lock-step kernel = columns of one MFMA tile

struct AdaGrad {
    int B, T, H, P;
    const int* lens;                             // [B] caption length per image (null: T)
    const float *c;                              // [B][T+1][H]
    const float *g, *i, *f, *o, *sgate;          // [B][T][H]
    const float *alpha, *beta;                   // [B][T][P], [B][T]
    float *d_ctx, *d_c;                          // [rows][H]
    float *g0, *g1, *gsum;                       // [rows][4H]
    float *wpart;                                // [rows][T][H / 16]
    float *r_words;                              // [rows][T]
};

__device__ __forceinline__ bool ag_active(const AdaGrad& g, int b, int t, int s) {
    const int len = g.lens ? g.lens[b] : g.T;
    return t < len && t >= s;
}

// the cell back-step of hidden unit j at time index i (:996-1006): writes G_i, the row's sum of G and d_c[i]; returns the unit's share of
// G_i . wsum.  first: lock-step 0 (gsum is written, not added to)
__device__ __forceinline__ float ag_cell(const AdaGrad& g, int b, int i, long row, int j, float d_h, float d_c_in, float* __restrict__ Gout,
                                         const float* __restrict__ wsum, bool first) {
    const int H = g.H;
    const long ti = ((long)b * g.T + i) * H + j, c1 = ((long)b * (g.T + 1) + i + 1) * H + j, c0 = c1 - H;
    const float tc = tanhf(g.c[c1]);
    const float o = g.o[ti], ig = g.i[ti], fg = g.f[ti], tg = tanhf(g.g[ti]);
    const float d_c = d_c_in + d_h * o * (1.f - tc * tc);                                            // :997
    float G[4];
    G[0] = ((d_c * tg) * ig) * (1.f - ig);                                                           // :1000, :1002
    G[1] = ((d_c * g.c[c0]) * fg) * (1.f - fg);                                                      // :998, :1003
    G[2] = (d_c * ig) * (1.f - tg * tg);                                                             // :1001, :1005
    G[3] = ((d_h * tc) * o) * (1.f - o);                                                             // :996, :1004
    const long gr = row * 4 * H + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        Gout[gr + q * H] = G[q];
        g.gsum[gr + q * H] = first ? G[q] : g.gsum[gr + q * H] + G[q];
    }
    g.d_c[row * H + j] = d_c * fg;                                                                   // :999
    return (G[0] * wsum[j] + G[1] * wsum[H + j]) + (G[2] * wsum[2 * H + j] + G[3] * wsum[3 * H + j]);
}

// :987-992 and the cell back-step of lock-step 0 (i = t).  One block per row.  Rows behind an image's last word: exact zeros in d_ctx, d_c,
// both G buffers and gsum
__global__ __launch_bounds__(256) void adaptive_grad_init_kernel(AdaGrad g, const float* __restrict__ fcw, const long long* __restrict__ tok,
                                                                 int tok_ld, const float* __restrict__ wsum) {
    __shared__ float pu[512];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, NW = H / AG_UNITS;
    const long tr = (long)row * H;
    for (int c = threadIdx.x; c < 4 * H; c += 256) g.g1[(long)row * 4 * H + c] = 0.f;               // (never an unwritten value under the MFMAs)
    if (!ag_active(g, b, t, 0)) {
        for (int c = threadIdx.x; c < H; c += 256) { g.d_ctx[tr + c] = 0.f; g.d_c[tr + c] = 0.f; }
        for (int c = threadIdx.x; c < 4 * H; c += 256) { g.g0[(long)row * 4 * H + c] = 0.f; g.gsum[(long)row * 4 * H + c] = 0.f; }
        return;
    }
    const long long k = tok[(long)b * tok_ld + t + 1];
    const float beta = g.beta[row];
    const long s1 = ((long)b * (g.T + 1) + t + 1) * H;
    for (int c = threadIdx.x; c < H; c += 256) {
        const float d_h = fcw[k * H + c];                                                            // :987, :992
        g.d_ctx[tr + c] = d_h * (1.f - beta);                                                        // :989
        const float tcn = tanhf(g.c[s1 + c]);
        const float d_c = ((d_h * beta) * g.sgate[tr + c]) * (1.f - tcn * tcn);                      // :990-991
        pu[c] = ag_cell(g, b, t, row, c, d_h, d_c, g.g0, wsum, true);
    }
    __syncthreads();
    if (threadIdx.x < NW) {                                                                          // the partials the lock-step kernel's workgroups write
        float a = 0.f;
        for (int u = 0; u < AG_UNITS; ++u) a += pu[threadIdx.x * AG_UNITS + u];
        g.wpart[((long)row * g.T + t) * NW + threadIdx.x] = a;
    }
}

// lock-step s >= 1: d_h = G W_hh for the workgroup's 16 hidden units (blockIdx.x) of a tile of <= 16 RT rows (blockIdx.y), then their cell
// back-step at time index i = t - s.  w_hh_t: (H, 4H), row j = column j of W_hh.  Reads the G buffer lock-step s - 1 wrote, writes the other
template <int RT>
__global__ __launch_bounds__(256) void adaptive_grad_step_kernel(AdaGrad g, int s, const float* __restrict__ w_hh_t,
                                                                 const float* __restrict__ wsum) {
    __shared__ float red[4][RT][16][17];
    __shared__ float pu[RT * 16][AG_UNITS + 1];
    __shared__ int any;
    const int H = g.H, rows = g.B * g.T, r0 = blockIdx.y * (RT * 16), nr = min(RT * 16, rows - r0), NW = H / AG_UNITS;
    const int tid = threadIdx.x;
    if (tid == 0) any = 0;
    __syncthreads();
    if (tid < nr) {
        const int row = r0 + tid, b = row / g.T;
        if (ag_active(g, b, row - b * g.T, s)) any = 1;
    }
    __syncthreads();
    if (!any) return;                                                                                // a tile without an active row (uniform)
    const float* __restrict__ Gin = (s & 1) ? g.g0 : g.g1;
    float* __restrict__ Gout = (s & 1) ? g.g1 : g.g0;
    linear_mfma_core<RT>(Gin + (long)r0 * 4 * H, 4L * H, w_hh_t, nr, 4 * H, H, red, blockIdx.x * AG_UNITS);
    for (int e = tid; e < RT * 256; e += 256) {
        const int r = e >> 8, rr = (e >> 4) & 15, u = e & 15, lr = r * 16 + rr;
        float p = 0.f;
        if (lr < nr) {
            const int row = r0 + lr, b = row / g.T, t = row - b * g.T, j = blockIdx.x * AG_UNITS + u;
            if (ag_active(g, b, t, s)) {
                const float d_h = (red[0][r][rr][u] + red[1][r][rr][u]) + (red[2][r][rr][u] + red[3][r][rr][u]);        // :1007
                p = ag_cell(g, b, t - s, row, j, d_h, g.d_c[(long)row * H + j], Gout, wsum, false);
            }
        }
        pu[lr][u] = p;
    }
    __syncthreads();
    if (tid < nr) {
        const int row = r0 + tid, b = row / g.T, t = row - b * g.T;
        if (ag_active(g, b, t, s)) {
            float a = 0.f;
            for (int u = 0; u < AG_UNITS; ++u) a += pu[tid][u];
            g.wpart[((long)row * g.T + (t - s)) * NW + blockIdx.x] = a;
        }
    }
}

// r_words[row][i] = G_i . wsum (:1008, :1010, :1016): the H / 16 partials of every (row, i) in workgroup order; zeros behind word t, in the rows
// behind an image's last word and for time indices the n_steps lock-steps did not reach
__global__ void adaptive_grad_words_kernel(AdaGrad g, int n_steps) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)g.B * g.T * g.T) return;
    const int i = idx % g.T, row = idx / g.T, b = row / g.T, t = row - b * g.T, NW = g.H / AG_UNITS;
    float a = 0.f;
    if (ag_active(g, b, t, 0) && i <= t && t - i < n_steps) {
        const float* p = g.wpart + idx * NW;
        for (int w = 0; w < NW; ++w) a += p[w];
    }
    g.r_words[idx] = a;
}

// d_feat[x][k][:] = alpha[b][t][k] v1[row][:] + d_avg[row][:] / P for row = rowlist[x] (null: x) - :1013-1015 with the projector product
// taken out of the pixel loop (v1 = d_ctx W_proj: the term is rank-1 in the pixel index).  A row behind its image's last word: zeros
__global__ void adaptive_grad_pix_kernel(AdaGrad g, const float* __restrict__ v1, const float* __restrict__ d_avg, float* __restrict__ d_feat,
                                         int C4, long total, const int* __restrict__ rowlist) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;      // over (output rows) * P * C4
    if (idx >= total) return;
    const int c4 = idx % C4;
    const long rp = idx / C4;
    const int k = rp % g.P;
    const long row = rowlist ? rowlist[rp / g.P] : rp / g.P;
    const int b = row / g.T, t = row - (long)b * g.T;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (ag_active(g, b, t, 0)) {
        const float a = g.alpha[row * g.P + k], np = (float)g.P;
        const f32x4 x1 = reinterpret_cast<const f32x4*>(v1)[row * C4 + c4], x2 = reinterpret_cast<const f32x4*>(d_avg)[row * C4 + c4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = a * x1[e] + x2[e] / np;
    }
    reinterpret_cast<f32x4*>(d_feat)[idx] = o;
}

static AdaGrad to_agrad(const lrpx_adaatt_trace* t, const lrpx_adaptive_gradstate* r) {
    AdaGrad g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.P = t->P; g.lens = r->lens;
    g.c = t->c; g.g = t->g; g.i = t->i; g.f = t->f; g.o = t->o; g.sgate = t->sgate; g.alpha = t->alpha; g.beta = t->beta;
    g.d_ctx = r->d_ctx; g.d_c = r->d_c; g.g0 = r->g0; g.g1 = r->g1; g.gsum = r->gsum; g.wpart = r->wpart; g.r_words = r->r_words;
    return g;
}

// host side of every entry: a grad=True trace of the sizes the kernels are built for, and a complete state
static int check_agrad(const char* fn, const lrpx_adaatt_trace* t, const lrpx_adaptive_gradstate* r) {
    LRPX_REQUIRE(t, "%s: null trace", fn);
    LRPX_REQUIRE(t->B > 0 && t->T > 0 && t->H == 512 && t->E == t->H && t->P > 0 && t->P <= 256,
                 "%s: unsupported trace dims (H must be 512, E == H, T > 0, 0 < P <= 256)", fn);
    LRPX_REQUIRE(t->xh && t->h && t->c && t->g && t->i && t->f && t->s && t->ctx && t->ctx_hat && t->hc && t->alpha && t->beta,
                 "%s: null trace tensor", fn);
    LRPX_REQUIRE(t->o && t->sgate, "%s: the trace has no output gate / sentinel gate (o, sgate): not a gradient trace", fn);
    LRPX_REQUIRE(r, "%s: null gradient state", fn);
    LRPX_REQUIRE(r->d_ctx && r->d_c && r->g0 && r->g1 && r->gsum && r->wpart && r->r_words, "%s: null gradient state tensor", fn);
    return LRPX_OK;
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

int lrpx_adaptive_grad_init(const lrpx_adaatt_trace* tr, const lrpx_adaptive_gradstate* gs, const float* fcw, const long long* tok,
                            int tok_ld, const float* wsum, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaptive_grad_init", {fcw, "fcw"}, {tok, "tok"}, {wsum, "wsum"});
    LRPX_TRY(check_agrad("lrpx_adaptive_grad_init", tr, gs));
    LRPX_REQUIRE(fcw && tok && wsum, "lrpx_adaptive_grad_init: null pointer");
    LRPX_REQUIRE(tok_ld >= tr->T + 1, "lrpx_adaptive_grad_init: tok_ld must hold T + 1 ids");
    hipLaunchKernelGGL(adaptive_grad_init_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_agrad(tr, gs), fcw, tok, tok_ld,
                       wsum);
    return check_launch("adaptive_grad_init");
}

int lrpx_adaptive_grad_steps(const lrpx_adaatt_trace* tr, const lrpx_adaptive_gradstate* gs, int n_steps, const float* w_hh_t,
                             const float* wsum, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaptive_grad_steps", {w_hh_t, "w_hh_t"}, {wsum, "wsum"});
    LRPX_TRY(check_agrad("lrpx_adaptive_grad_steps", tr, gs));
    LRPX_REQUIRE(w_hh_t && wsum, "lrpx_adaptive_grad_steps: null pointer");
    LRPX_REQUIRE(n_steps >= 1 && n_steps <= tr->T, "lrpx_adaptive_grad_steps: n_steps must be in [1, T] (lock-step 0 is grad_init's)");
    hipStream_t st = (hipStream_t)stream;
    const AdaGrad g = to_agrad(tr, gs);
    const int rows = tr->B * tr->T, NW = tr->H / AG_UNITS;
    // row tiles of 32 (16 for <= 16 rows): 64-row tiles measured slower at every row count tried (160 .. 1280 rows: 1 % .. 27 % of the
    // back-pass) - half as many workgroups, each reading twice the rows of G; the results are the same bits either way
    for (int s = 1; s < n_steps; ++s) {
        if (rows <= 16) hipLaunchKernelGGL((adaptive_grad_step_kernel<1>), dim3(NW, 1), dim3(256), 0, st, g, s, w_hh_t, wsum);
        else hipLaunchKernelGGL((adaptive_grad_step_kernel<2>), dim3(NW, (rows + 31) / 32), dim3(256), 0, st, g, s, w_hh_t, wsum);
        LRPX_TRY(check_launch("adaptive_grad_step"));
    }
    const long total = (long)rows * tr->T;
    hipLaunchKernelGGL(adaptive_grad_words_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g, n_steps);
    return check_launch("adaptive_grad_words");
}

int lrpx_adaptive_grad_pix_rows(const lrpx_adaatt_trace* tr, const lrpx_adaptive_gradstate* gs, const float* v1, const float* d_avg,
                                float* d_feat, int C, const int32_t* rows, int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_adaptive_grad_pix_rows", {v1, "v1"}, {d_avg, "d_avg"}, {d_feat, "d_feat"}, {rows, "rows"});
    LRPX_TRY(check_agrad("lrpx_adaptive_grad_pix_rows", tr, gs));
    LRPX_REQUIRE(v1 && d_avg && d_feat && C > 0 && C % 4 == 0, "lrpx_adaptive_grad_pix_rows: bad arguments (C %% 4 == 0)");
    LRPX_REQUIRE(rows ? (n_rows > 0 && n_rows <= tr->B * tr->T) : n_rows == tr->B * tr->T,
                 "lrpx_adaptive_grad_pix_rows: bad row list (without a row list n_rows must be B*T)");
    const long total = (long)n_rows * tr->P * (C / 4);
    hipLaunchKernelGGL(adaptive_grad_pix_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, to_agrad(tr, gs), v1,
                       d_avg, d_feat, C / 4, total, rows);
    return check_launch("adaptive_grad_pix");
}

}  // extern "C"
