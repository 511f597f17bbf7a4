// The AoA decoder (models/aoamodel.py): forward trace (per step, fused, decoupled), LRP relevance (per step and the fused lock-step),
// gradient explainers, host loops.  What no model owns (the skinny linear, arg-max, re-weighting, ...) is in decoder_blocks.hip, reached
// through its C entry points; what the decoders share on the device is decoder_shared.h.
//
// Written as fused per-time-step kernels batched over all (image, word) rows: row r = b*T + t is the explanation of word t of image b;
// at lock-step s every row with t >= s works on time index i = t - s.
//
// Trace tensors are [B][T(+1)][...] fp32; token ids int64 (torch.long).
#include <math.h>

#include "common.h"
#include "conv_mfma.h"
#include "conv_launch.h"
#include "decoder_shared.h"

namespace lrpx {

// ================================================================================================
// AoA decoder (models/aoamodel.py): trace :990-1062, relevance :1064-1156
// ================================================================================================
struct AoaFwd {
    int B, T, H, E, P, NH;
    float *xh;                   // [B][T][E+2H] = [emb | glob | h_t]          (xt ++ ht[:T], :1075)
    float *h, *c;                // [B][T+1][H]
    float *g, *i, *f;            // [B][T][H]
    float *ctx, *lin, *c_aoa, *hc;   // [B][T][H]  context, decoder_aoa_linear(context), gated, fc input
    float *alpha;                // [B][T][NH][P]
    float *o, *sg;               // optional: [B][T][H] output gate, sigmoid(aoa gate)   (gradient explainers)
};

// xh[b,t] = [emb[tok[b,t]] | glob[b] | h[b,t]]   (:1030, :1075)
__global__ void aoa_fwd_pre_kernel(AoaFwd g, int t, const float* __restrict__ glob, const float* __restrict__ emb,
                                   const long long* __restrict__ tok, int tok_ld) {
    const int b = blockIdx.x, W = g.E + 2 * g.H;
    float* dst = g.xh + ((long)b * g.T + t) * W;
    const long st = ((long)b * (g.T + 1) + t) * g.H;
    const long long k = tok[(long)b * tok_ld + t];
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        float v;
        if (c < g.E) v = emb[k * g.E + c];
        else if (c < g.E + g.H) v = glob[(long)b * g.H + (c - g.E)];
        else v = g.h[st + (c - g.E - g.H)];
        dst[c] = v;
    }
}

__global__ void aoa_fwd_lstm_kernel(AoaFwd g, int t, const float* __restrict__ zz, int ldz) {
    const int b = blockIdx.x, H = g.H;
    const long st0 = ((long)b * (g.T + 1) + t) * H, st1 = st0 + H, tr = ((long)b * g.T + t) * H;
    const float* z = zz + (long)b * ldz;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float zg = z[2 * H + c];
        const LstmCell l = lstm_cell(z[c], z[H + c], zg, z[3 * H + c], g.c[st0 + c]);
        g.c[st1 + c] = l.cn; g.h[st1 + c] = l.o * tanhf(l.cn);
        g.g[tr + c] = zg; g.i[tr + c] = l.i; g.f[tr + c] = l.f;
        if (g.o) g.o[tr + c] = l.o;
    }
}

// MultiHeadedDotAttention.forward (models/aoamodel.py:77-108) for a single query per image; one block per
// (image, head).  qg: [B][2H] = [q_proj(h) | aoa_linear_gate(h)]
__global__ __launch_bounds__(256) void aoa_fwd_attention_kernel(AoaFwd g, int t, const float* __restrict__ qg, int ldq,
                                                                const float* __restrict__ key,
                                                                const float* __restrict__ value) {
    extern __shared__ float sm[];
    const int b = blockIdx.x, hd = blockIdx.y, H = g.H, P = g.P, dk = H / g.NH, tid = threadIdx.x;
    float* q = sm;          // dk
    float* sc = q + dk;     // P
    float* red = sc + P;    // 8
    for (int c = tid; c < dk; c += 256) q[c] = qg[(long)b * ldq + hd * dk + c];
    __syncthreads();
    const float inv = 1.f / sqrtf((float)dk);
    for (int k = tid; k < P; k += 256) {
        const float* kp = key + ((long)b * P + k) * H + hd * dk;
        float a = 0.f;
        for (int c = 0; c < dk; ++c) a += q[c] * kp[c];
        sc[k] = a * inv;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int k = tid; k < P; k += 256) m = fmaxf(m, sc[k]);
    m = block_max(m, red);
    float e = 0.f;
    for (int k = tid; k < P; k += 256) e += expf(sc[k] - m);
    const float denom = block_sum(e, red);
    __syncthreads();
    float* al = g.alpha + (((long)b * g.T + t) * g.NH + hd) * P;
    for (int k = tid; k < P; k += 256) { const float a = expf(sc[k] - m) / denom; sc[k] = a; al[k] = a; }
    __syncthreads();
    const long tr = ((long)b * g.T + t) * H;
    for (int c = tid; c < dk; c += 256) {
        float a = 0.f;
        for (int k = 0; k < P; ++k) a += sc[k] * value[((long)b * P + k) * H + hd * dk + c];
        g.ctx[tr + hd * dk + c] = a;
    }
}

// c_aoa = sigmoid(gate) * lin ; hc = c_aoa + h   (:1034-1038)
__global__ void aoa_fwd_post_kernel(AoaFwd g, int t, const float* __restrict__ qg, int ldq, const float* __restrict__ lin) {
    const int b = blockIdx.x, H = g.H;
    const long st1 = ((long)b * (g.T + 1) + t + 1) * H, tr = ((long)b * g.T + t) * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float l = lin[(long)b * H + c];
        const float sgv = sigmoidf_(qg[(long)b * ldq + H + c]);
        const float ca = sgv * l;
        g.lin[tr + c] = l; g.c_aoa[tr + c] = ca; g.hc[tr + c] = ca + g.h[st1 + c];
        if (g.sg) g.sg[tr + c] = sgv;
    }
}

// ---- the skinny linears of the AoA step with their point-wise neighbours in the epilogue ---------------------------------
// The bottom-up path is bound by the GPU's dispatch rate of dependent small kernels (~330 launches of 4 - 28 us per step of 640
// maps), so the seven launches of a decoder step become four: the gate linear applies the LSTM cell (its weight
// ROWS are interleaved - workgroup j holds the i, f, g, o rows of the hidden units 4j .. 4j+3 - so the four pre-activations of
// a unit meet in the workgroup's LDS reduction), decoder_aoa_linear applies the gated sum (fwd_post) and gathers the NEXT
// step's LSTM input row (fwd_pre).  The dot products run in the same order as in linear_mfma_kernel and the point-wise code is
// that of aoa_fwd_lstm / _post / _pre: results are bit-identical to the unfused step (token ids of the sampling goldens, traces).
// (linear_mfma_core, red4 and lstm_cell: decoder_shared.h; linear_mfma_kernel: decoder_blocks.hip)

// gate linear + LSTM cell (aoa_fwd_lstm_kernel).  w / bias: rows interleaved, row 16 j + 4 gate + u = original row gate * H + 4 j + u
template <int RT>
__global__ __launch_bounds__(256) void aoa_linear_lstm_kernel(AoaFwd g, int t, const float* __restrict__ w,
                                                              const float* __restrict__ bias) {
    __shared__ float red[4][RT][16][17];
    const int H = g.H, W = g.E + 2 * H;
    linear_mfma_core<RT>(g.xh + (long)t * W, (long)g.T * W, w, g.B, W, 4 * H, red, blockIdx.x * 16);
    for (int e = threadIdx.x; e < RT * 64; e += 256) {
        const int r = e >> 6, row = (e >> 2) & 15, u = e & 3;
        const int b = r * 16 + row, c = blockIdx.x * 4 + u;
        if (b >= g.B || c >= H) continue;
        float z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 4 * q + u;
            z[q] = red4<RT>(red, r, row, col);
            if (bias) z[q] += bias[blockIdx.x * 16 + col];
        }
        const long st0 = ((long)b * (g.T + 1) + t) * H, st1 = st0 + H, tr = ((long)b * g.T + t) * H;
        const LstmCell l = lstm_cell(z[0], z[1], z[2], z[3], g.c[st0 + c]);
        g.c[st1 + c] = l.cn; g.h[st1 + c] = l.o * tanhf(l.cn);
        g.g[tr + c] = z[2]; g.i[tr + c] = l.i; g.f[tr + c] = l.f;
        if (g.o) g.o[tr + c] = l.o;
    }
}

// decoder_aoa_linear + gated sum (aoa_fwd_post_kernel) + the next step's input row (aoa_fwd_pre_kernel for t + 1)
template <int RT>
__global__ __launch_bounds__(256) void aoa_linear_post_kernel(AoaFwd g, int t, const float* __restrict__ w,
                                                              const float* __restrict__ bias, const float* __restrict__ qg, int ldq,
                                                              const float* __restrict__ glob, const float* __restrict__ emb,
                                                              const long long* __restrict__ tok, int tok_ld) {
    __shared__ float red[4][RT][16][17];
    const int H = g.H, W = g.E + 2 * H;
    linear_mfma_core<RT>(g.ctx + (long)t * H, (long)g.T * H, w, g.B, H, H, red, blockIdx.x * 16);
    for (int e = threadIdx.x; e < RT * 256; e += 256) {
        const int r = e >> 8, row = (e >> 4) & 15, col = e & 15;
        const int b = r * 16 + row, c = blockIdx.x * 16 + col;
        if (b >= g.B || c >= H) continue;
        float l = red4<RT>(red, r, row, col);
        if (bias) l += bias[c];
        const long st1 = ((long)b * (g.T + 1) + t + 1) * H, tr = ((long)b * g.T + t) * H;
        const float sgv = sigmoidf_(qg[(long)b * ldq + H + c]);
        const float ca = sgv * l;
        g.lin[tr + c] = l; g.c_aoa[tr + c] = ca; g.hc[tr + c] = ca + g.h[st1 + c];
        if (g.sg) g.sg[tr + c] = sgv;
    }
    if (t + 1 < g.T) {        // xh[b, t+1] = [emb[tok[b, t+1]] | glob[b] | h[b, t+1]]: this workgroup's slice of the columns, every image
        const int per = (W + (int)gridDim.x - 1) / (int)gridDim.x;
        const int c0 = blockIdx.x * per, c1 = min(W, c0 + per);
        for (int e = threadIdx.x; e < g.B * per; e += 256) {
            const int b = e / per, c = c0 + e - b * per;
            if (c >= c1) continue;
            const long long k = tok[(long)b * tok_ld + t + 1];
            float v;
            if (c < g.E) v = emb[k * g.E + c];
            else if (c < g.E + H) v = glob[(long)b * H + (c - g.E)];
            else v = g.h[((long)b * (g.T + 1) + t + 1) * H + (c - g.E - H)];
            g.xh[((long)b * g.T + t + 1) * W + c] = v;
        }
    }
}

// ---- the teacher-forced trace with the recurrence DECOUPLED from what hangs off it (round 5) ------------------------------------
// In this model the LSTM input is x_t = [emb(word_t) | global feature] and its own h_{t-1} (models/aoamodel.py:1030-1033): the
// attention, the AoA gate and the scores READ h_t but never feed the recurrence.  Under teacher forcing every x_t is known up front,
// so the only sequential work is  z_t = Zin[t] + W_hh h_{t-1}  with  Zin = [emb | glob] W_ih^T + b  computed for all (image, word)
// rows in ONE GEMM, and q / gate linear, attention, decoder_aoa_linear, gated sum run once over all B*T rows afterwards: a step of
// the reference's loop (:1019-1052) costs one launch of K = 512 instead of four launches with K = 1536 in the first.
__global__ void aoa_fwd_inputs_kernel(AoaFwd g, const float* __restrict__ glob, const float* __restrict__ emb,
                                      const long long* __restrict__ tok, int tok_ld, float* __restrict__ xin) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, W = g.E + 2 * g.H, EH = g.E + g.H;
    float* dst = g.xh + (long)row * W;
    const long long k = tok[(long)b * tok_ld + t];
    for (int c = threadIdx.x; c < EH; c += blockDim.x) {
        const float v = c < g.E ? emb[k * g.E + c] : glob[(long)b * g.H + (c - g.E)];
        dst[c] = v;
        if (xin) xin[(long)row * EH + c] = v;
    }
}

// z = zin[b, t] + W_hh h[b, t]  ->  LSTM cell (the point-wise code of aoa_fwd_lstm_kernel).  w: (4H, H), rows interleaved as in
// aoa_linear_lstm_kernel; zin: [B*T][4H] in the same interleaved column order (bias included)
// zin == null: the input part comes from a per-MODEL table instead of a per-step GEMM - the embedding part of x_t W_ih^T depends on the
// token alone: tab[token] = emb[token] W_ie^T (V x 4H, computed once per engine), gimg[b] = glob[b] W_ig^T + bias (one small linear
// per trace): z = (W_hh h + tab[tok[b, t]]) + gimg[b]
template <int RT>
__global__ __launch_bounds__(256) void aoa_rec_lstm_kernel(AoaFwd g, int t, const float* __restrict__ w,
                                                           const float* __restrict__ zin, const float* __restrict__ tab,
                                                           const float* __restrict__ gimg, const long long* __restrict__ tok, int tok_ld) {
    __shared__ float red[4][RT][16][17];
    const int H = g.H;
    linear_mfma_core<RT>(g.h + (long)t * H, (long)(g.T + 1) * H, w, g.B, H, 4 * H, red, blockIdx.x * 16);
    for (int e = threadIdx.x; e < RT * 64; e += 256) {
        const int r = e >> 6, row = (e >> 2) & 15, u = e & 3;
        const int b = r * 16 + row, c = blockIdx.x * 4 + u;
        if (b >= g.B || c >= H) continue;
        const float* zi = zin ? zin + ((long)b * g.T + t) * 4 * H + blockIdx.x * 16
                              : tab + (long)tok[(long)b * tok_ld + t] * 4 * H + blockIdx.x * 16;
        const float* gi = zin ? nullptr : gimg + (long)b * 4 * H + blockIdx.x * 16;
        float z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 4 * q + u;
            z[q] = red4<RT>(red, r, row, col) + zi[col];
            if (gi) z[q] += gi[col];
        }
        const long st0 = ((long)b * (g.T + 1) + t) * H, st1 = st0 + H, tr = ((long)b * g.T + t) * H;
        const LstmCell l = lstm_cell(z[0], z[1], z[2], z[3], g.c[st0 + c]);
        g.c[st1 + c] = l.cn; g.h[st1 + c] = l.o * tanhf(l.cn);
        g.g[tr + c] = z[2]; g.i[tr + c] = l.i; g.f[tr + c] = l.f;
        if (g.o) g.o[tr + c] = l.o;
    }
}

// after the recurrence: hn[b, t] = h[b, t + 1] (contiguous rows for the q / gate GEMM), xh[b, t][E + H :] = h[b, t] (:1075)
__global__ __launch_bounds__(256) void aoa_fwd_gather_h_kernel(AoaFwd g, float* __restrict__ hn, unsigned* __restrict__ hn_amax) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, W = g.E + 2 * H;
    const long st0 = ((long)b * (g.T + 1) + t) * H;
    float m = 0.f;
    for (int c = threadIdx.x; c < H; c += 256) {
        g.xh[(long)row * W + g.E + H + c] = g.h[st0 + c];
        const float v = g.h[st0 + H + c];
        hn[(long)row * H + c] = v;
        m = fmaxf(m, fabsf(v));
    }
    if (hn_amax) {          // max|hn[row]|: the operand scale of the q / gate GEMM (what lrpx_amax_maps would read the row again for)
        m = block_max(m, red);
        if (threadIdx.x == 0) hn_amax[row] = __float_as_uint(m);
    }
}

// aoa_fwd_attention_kernel for every (image, word) row at once: block (row, head); qg: [B*T][ldq]
__global__ __launch_bounds__(64) void aoa_fwd_attention_all_kernel(AoaFwd g, const float* __restrict__ qg, int ldq,
                                                                   const float* __restrict__ key, const float* __restrict__ value,
                                                                   unsigned* __restrict__ ctx_amax) {
    extern __shared__ float sm[];
    const int row = blockIdx.x, b = row / g.T, hd = blockIdx.y, H = g.H, P = g.P, dk = H / g.NH, tid = threadIdx.x;
    float* q = sm;          // dk
    float* sc = q + dk;     // P
    for (int c = tid; c < dk; c += 64) q[c] = qg[(long)row * ldq + hd * dk + c];
    __syncthreads();
    const float inv = 1.f / sqrtf((float)dk);
    for (int k = tid; k < P; k += 64) {
        const float* kp = key + ((long)b * P + k) * H + hd * dk;
        float a = 0.f;
        for (int c = 0; c < dk; ++c) a += q[c] * kp[c];
        sc[k] = a * inv;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int k = tid; k < P; k += 64) m = fmaxf(m, sc[k]);
    m = wave_max(m);
    float e = 0.f;
    for (int k = tid; k < P; k += 64) e += expf(sc[k] - m);
    const float denom = wave_sum(e);
    float* al = g.alpha + ((long)row * g.NH + hd) * P;
    for (int k = tid; k < P; k += 64) { const float a = expf(sc[k] - m) / denom; sc[k] = a; al[k] = a; }
    __syncthreads();
    float mx = 0.f;
    for (int c = tid; c < dk; c += 64) {
        float a = 0.f;
        for (int k = 0; k < P; ++k) a += sc[k] * value[((long)b * P + k) * H + hd * dk + c];
        g.ctx[(long)row * H + hd * dk + c] = a;
        mx = fmaxf(mx, fabsf(a));
    }
    if (ctx_amax) {         // max|ctx[row]| over the heads (zero-initialised by the caller; non-negative floats order like unsigned integers)
        mx = wave_max(mx);
        if (tid == 0) atomicMax(&ctx_amax[row], __float_as_uint(mx));
    }
}

// aoa_fwd_post_kernel for every row: lin [B*T][H] = decoder_aoa_linear(ctx), qg [B*T][ldq] (gate in the second half)
__global__ __launch_bounds__(256) void aoa_fwd_post_all_kernel(AoaFwd g, const float* __restrict__ qg, int ldq, const float* __restrict__ lin,
                                                               unsigned* __restrict__ hc_amax) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long st1 = ((long)b * (g.T + 1) + t + 1) * H, tr = (long)row * H;
    float m = 0.f;
    for (int c = threadIdx.x; c < H; c += 256) {
        const float l = lin[tr + c];
        const float sgv = sigmoidf_(qg[(long)row * ldq + H + c]);
        const float ca = sgv * l;
        const float hcv = ca + g.h[st1 + c];
        g.lin[tr + c] = l; g.c_aoa[tr + c] = ca; g.hc[tr + c] = hcv;
        if (g.sg) g.sg[tr + c] = sgv;
        m = fmaxf(m, fabsf(hcv));
    }
    if (hc_amax) {          // max|hc[row]|: the operand scale of the (T, V) score GEMM
        m = block_max(m, red);
        if (threadIdx.x == 0) hc_amax[row] = __float_as_uint(m);
    }
}

// ---- AoA gradient explainers (models/aoamodel.py:1435-1499), all (image, word) rows in lock-step -------------------
struct AoaGrad {
    int B, T, H, E, P, NH;
    const int* lens;
    const float *c, *g, *i, *f, *o, *sg, *lin, *alpha;
    float *d_h, *d_c, *dA, *dB, *gates, *dx, *d_glob, *r_words;
};

__device__ __forceinline__ bool aoa_grow_active(const AoaGrad& g, int b, int t, int s) {
    const int len = g.lens ? g.lens[b] : g.T;
    return t < len && t >= s;
}

// :1461-1470: d_word_pred one-hot -> fc row; gradient into the gated sum  c_aoa = sigmoid(gate) * lin
__global__ void aoa_grad_init_kernel(AoaGrad g, const float* __restrict__ fcw, const long long* __restrict__ tok,
                                     int tok_ld) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long long k = tok[(long)b * tok_ld + t + 1];
    const long r = (long)row * H;          // trace tensors [B][T][H] are indexed by the same row
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float d = fcw[k * H + c], sgv = g.sg[r + c];
        g.d_h[r + c] = d; g.d_c[r + c] = 0.f; g.d_glob[r + c] = 0.f;
        g.dA[r + c] = d * sgv;
        g.dB[r + c] = d * g.lin[r + c] * (1.f - sgv) * sgv;
    }
    for (int c = threadIdx.x; c < g.T; c += blockDim.x) g.r_words[(long)row * g.T + c] = 0.f;
}

// phase 0 (:1474-1484): LSTM cell backward at time i = t - s -> gate gradients [i | f | g | o]
__global__ void aoa_grad_step0_kernel(AoaGrad g, int s) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long r = (long)row * H;
    float* gt = g.gates + (long)row * 4 * H;
    if (!aoa_grow_active(g, b, t, s)) {
        for (int c = threadIdx.x; c < 4 * H; c += blockDim.x) gt[c] = 0.f;
        return;
    }
    const int i = t - s;
    const long ti = ((long)b * g.T + i) * H, ci = ((long)b * (g.T + 1) + i) * H, ci1 = ci + H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float dh = g.d_h[r + c], tc = tanhf(g.c[ci1 + c]);
        const float iv = g.i[ti + c], fv = g.f[ti + c], gv = tanhf(g.g[ti + c]), ov = g.o[ti + c];
        const float dc = g.d_c[r + c] + dh * ov * (1.f - tc * tc);
        gt[c] = dc * gv * iv * (1.f - iv);
        gt[H + c] = dc * g.c[ci + c] * fv * (1.f - fv);
        gt[2 * H + c] = dc * iv * (1.f - gv * gv);
        gt[3 * H + c] = dh * tc * ov * (1.f - ov);
        g.d_c[r + c] = dc * fv;
    }
}

// phase 1 (:1485-1488): dx = gates @ [W_ih | W_hh] = [d_emb (E) | d_glob (H) | d_h (H)]
__global__ void aoa_grad_step1_kernel(AoaGrad g, int s) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, E = g.E;
    if (!aoa_grow_active(g, b, t, s)) return;
    const int i = t - s;
    const long r = (long)row * H;
    const float* dx = g.dx + (long)row * (E + 2 * H);
    __shared__ float red[4];
    float acc = 0.f;
    for (int c = threadIdx.x; c < E; c += blockDim.x) acc += dx[c];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) g.r_words[(long)row * g.T + i] = acc;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        g.d_glob[r + c] = dx[E + c];            // assignment, not accumulation (:1487)
        g.d_h[r + c] = dx[E + H + c];
    }
}

__global__ void aoa_grad_pix_kernel(const float* __restrict__ alpha, int T, int NH, int P, int head,
                                    const float* __restrict__ v1, const float* __restrict__ v2,
                                    float* __restrict__ d_feat, int C4, long total,
                                    const int* __restrict__ rowlist) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;     // over (output rows)*P*C4
    if (idx >= total) return;
    const int c4 = idx % C4;
    const long rp = idx / C4;
    const int p = rp % P;
    const long row = rowlist ? rowlist[rp / P] : rp / P;
    const float a = alpha[(row * NH + head) * P + p];
    const f32x4 x1 = reinterpret_cast<const f32x4*>(v1)[row * C4 + c4], x2 = reinterpret_cast<const f32x4*>(v2)[row * C4 + c4];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = a * x1[e] + x2[e];
    reinterpret_cast<f32x4*>(d_feat)[idx] = o;
}

struct AoaRel {
    int B, T, H, E, P, NH;
    const int* lens;
    const float *xh, *h, *c, *g, *i, *ctx, *lin, *c_aoa, *hc, *alpha;
    float *r_hn, *r_glob, *A, *rx, *r_words;     // [rows][H], [rows][H], [rows][H], [rows][E+2H], [rows][T]
};

__device__ __forceinline__ bool aoa_row_active(const AoaRel& g, int b, int t, int s) {
    const int len = g.lens ? g.lens[b] : g.T;
    return t < len && t >= s;
}

// :1081-1110 fc one-hot rule, split into h and context_aoa; A = r_caoa / z~(aoa_linear output) for the dense rule
__global__ void aoa_rel_init_kernel(AoaRel g, const float* __restrict__ fcw, const float* __restrict__ logit,
                                    const long long* __restrict__ tok, int tok_ld) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long long k = tok[(long)b * tok_ld + t + 1];
    const float lg = logit[row], zt = stab_eps(lg);
    const long tr = (long)row * H, st1 = ((long)b * (g.T + 1) + t + 1) * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float hc = g.hc[tr + c];
        const float r_hc = (fcw[k * H + c] * hc / zt) * lg;
        g.r_hn[tr + c] = eps_id(r_hc, g.h[st1 + c], hc);
        const float r_ca = eps_id(r_hc, g.c_aoa[tr + c], hc);
        g.A[tr + c] = r_ca / stab_eps(g.lin[tr + c]);
        g.r_glob[tr + c] = 0.f;
    }
    for (int c = threadIdx.x; c < g.T; c += blockDim.x) g.r_words[(long)row * g.T + c] = 0.f;
}

// lrp_mha (:812-862), single head: Aval[row][k][c] = (value*alpha / z~(ctx)) * r_ctx / z~(value)  inside head
// `head`, 0 elsewhere — the prologue of the v_proj dense rule (:1141-1144).  r_ctx: [rows][H]
__global__ __launch_bounds__(256) void aoa_rel_value_kernel(AoaRel g, const float* __restrict__ r_ctx,
                                                            const float* __restrict__ value, int head,
                                                            float* __restrict__ Aval, const int* __restrict__ rowlist, int head_only) {
    const int row = rowlist ? rowlist[blockIdx.x] : blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, P = g.P, dk = H / g.NH;
    const long orow = blockIdx.x;
    const int len = g.lens ? g.lens[b] : g.T;
    const bool act = t < len;
    const float* al = g.alpha + (((long)b * g.T + t) * g.NH + head) * P;
    if (head_only) {
        // only the head's dk columns are non-zero: Aval [rows][P][dk] - the v_proj rule then contracts over K = dk with the head's
        // dk rows of W_v instead of K = H with zeros in 7/8 of the operand (the same products in the same order: bit-identical)
        for (int j = threadIdx.x; j < P * dk; j += 256) {
            const int k = j / dk, c = head * dk + (j - k * dk);
            float v = 0.f;
            if (act) {
                const float val = value[((long)b * P + k) * H + c];
                const float rv = eps_id(r_ctx[(long)row * H + c], val * al[k], g.ctx[(long)row * H + c]);
                v = rv / stab_eps(val);
            }
            Aval[(orow * P + k) * dk + (c - head * dk)] = v;
        }
        return;
    }
    for (int j = threadIdx.x; j < P * H; j += 256) {
        const int k = j / H, c = j - k * H;
        float v = 0.f;
        if (act && c >= head * dk && c < (head + 1) * dk) {
            const float val = value[((long)b * P + k) * H + c];
            const float rv = eps_id(r_ctx[(long)row * H + c], val * al[k], g.ctx[(long)row * H + c]);
            v = rv / stab_eps(val);
        }
        Aval[(orow * P + k) * H + c] = v;
    }
}

// :1116-1120  r_c = r_h (assignment); g-gate path; A = r_g / z~(g)
__global__ void aoa_rel_a_kernel(AoaRel g, int s) {
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H;
    const long tr = (long)row * H;
    if (!aoa_row_active(g, b, t, s)) {
        for (int c = threadIdx.x; c < H; c += blockDim.x) g.A[tr + c] = 0.f;
        return;
    }
    const int i = t - s;
    const long ti = ((long)b * g.T + i) * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float rg = eps_id(g.r_hn[tr + c], g.i[ti + c] * tanhf(g.g[ti + c]), g.c[sc1 + c]);
        g.A[tr + c] = rg / stab_eps(g.g[ti + c]);
    }
}

// :1129-1133  r_xh = [emb | glob | h]
__global__ __launch_bounds__(256) void aoa_rel_c_kernel(AoaRel g, int s) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, E = g.E;
    if (!aoa_row_active(g, b, t, s)) return;
    const int i = t - s;
    const long tr = (long)row * H;
    const float* rx = g.rx + (long)row * (E + 2 * H);
    float acc = 0.f;
    for (int c = threadIdx.x; c < E; c += 256) acc += rx[c];
    for (int c = threadIdx.x; c < H; c += 256) {
        g.r_glob[tr + c] += rx[E + c];
        g.r_hn[tr + c] = rx[E + H + c];
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) g.r_words[(long)row * g.T + i] = acc;
}

// rel_c of lock-step s followed by rel_a of lock-step s + 1 for the same row (one launch instead of two; the same code, the
// element -> thread map of both parts is the same, so a thread reads back the r_hn it has just written)
__global__ __launch_bounds__(256) void aoa_rel_ca_kernel(AoaRel g, int s) {
    __shared__ float red[8];
    const int row = blockIdx.x, b = row / g.T, t = row - b * g.T, H = g.H, E = g.E;
    const long tr = (long)row * H;
    if (aoa_row_active(g, b, t, s)) {
        const int i = t - s;
        const float* rx = g.rx + (long)row * (E + 2 * H);
        float acc = 0.f;
        for (int c = threadIdx.x; c < E; c += 256) acc += rx[c];
        for (int c = threadIdx.x; c < H; c += 256) {
            g.r_glob[tr + c] += rx[E + c];
            g.r_hn[tr + c] = rx[E + H + c];
        }
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) g.r_words[(long)row * g.T + i] = acc;
    }
    if (s + 1 >= g.T) return;
    if (!aoa_row_active(g, b, t, s + 1)) {
        for (int c = threadIdx.x; c < H; c += 256) g.A[tr + c] = 0.f;
        return;
    }
    const int i = t - s - 1;
    const long ti = ((long)b * g.T + i) * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H;
    for (int c = threadIdx.x; c < H; c += 256) {
        const float rg = eps_id(g.r_hn[tr + c], g.i[ti + c] * tanhf(g.g[ti + c]), g.c[sc1 + c]);
        g.A[tr + c] = rg / stab_eps(g.g[ti + c]);
    }
}

// per-trace tables of the fused AoA lock-steps: what aoa_rel_a_kernel evaluates per (row, step) depends on (image, time index) only -
// q1 = i tanh(g) / z~(c[i + 1]) (eps_id's factor) and dg = z~(g) (:1116-1120) - and tmax[row] = t for a word the caption has, else -1
__global__ void aoa_rel_coef_kernel(AoaRel g, float* __restrict__ q1, float* __restrict__ dg, int* __restrict__ tmax) {
    const int row = blockIdx.x, b = row / g.T, i = row - b * g.T, H = g.H;
    const long ti = (long)row * H, sc1 = ((long)b * (g.T + 1) + i + 1) * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float gg = g.g[ti + c];
        q1[ti + c] = (g.i[ti + c] * tanhf(gg)) / stab_eps(g.c[sc1 + c]);
        dg[ti + c] = stab_eps(gg);
    }
    if (threadIdx.x == 0) tmax[row] = i < (g.lens ? g.lens[b] : g.T) ? i : -1;
}

// the same after the fused AoA lock-steps (dense_f16x3.hip, FUSE): r_words[row][i] = the four 128-column partial sums of the
// embedding part in a fixed order, then :1129-1132; rows behind an image's last word stay zero
__global__ void rel_words_norm_parts_kernel(float* __restrict__ r_words, const float* __restrict__ wpart, const int* __restrict__ lens,
                                            int rows, int T) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int b = row / T, t = row - b * T;
    const int len = lens ? lens[b] : T;
    float* rw = r_words + (long)row * T;
    if (t >= len) {
        for (int i = 0; i < T; ++i) rw[i] = 0.f;
        return;
    }
    float m = 0.f;
    for (int i = 0; i <= t; ++i) {
        const float* p = wpart + ((long)row * T + i) * 4;
        const float v = (p[0] + p[1]) + (p[2] + p[3]);
        rw[i] = v;
        m = fmaxf(m, fabsf(v));
    }
    for (int i = t + 1; i < T; ++i) rw[i] = 0.f;
    if (m > 0.f)
        for (int i = 0; i <= t; ++i) rw[i] /= m;
}


}  // namespace lrpx

using namespace lrpx;

static AoaFwd to_afwd(const lrpx_aoa_trace* t) {
    AoaFwd g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P; g.NH = t->NH;
    g.xh = t->xh; g.h = t->h; g.c = t->c; g.g = t->g; g.i = t->i; g.f = t->f;
    g.ctx = t->ctx; g.lin = t->lin; g.c_aoa = t->c_aoa; g.hc = t->hc; g.alpha = t->alpha;
    g.o = t->o; g.sg = t->sg;
    return g;
}

static int check_atrace(const lrpx_aoa_trace* t) {
    LRPX_REQUIRE(t && t->B > 0 && t->T > 0 && t->H == 512 && t->E % 4 == 0 && t->P > 0 && t->NH > 0 && t->H % t->NH == 0,
                 "aoa: unsupported trace dims (H must be 512)");
    LRPX_REQUIRE(t->xh && t->h && t->c && t->g && t->i && t->f && t->ctx && t->lin && t->c_aoa && t->hc && t->alpha,
                 "aoa: null trace tensor");
    return LRPX_OK;
}

static int to_agrad(const lrpx_aoa_trace* t, const lrpx_aoa_gradstate* r, AoaGrad* out) {
    LRPX_TRY(check_atrace(t));
    LRPX_REQUIRE(t->o && t->sg, "aoa gradient: the trace lacks the output gate / aoa gate (allocate it with grad=True)");
    LRPX_REQUIRE(r && r->d_h && r->d_c && r->dA && r->dB && r->gates && r->dx && r->d_glob && r->r_words,
                 "aoa gradient: null state tensor");
    AoaGrad g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P; g.NH = t->NH; g.lens = r->lens;
    g.c = t->c; g.g = t->g; g.i = t->i; g.f = t->f; g.o = t->o; g.sg = t->sg; g.lin = t->lin; g.alpha = t->alpha;
    g.d_h = r->d_h; g.d_c = r->d_c; g.dA = r->dA; g.dB = r->dB; g.gates = r->gates; g.dx = r->dx; g.d_glob = r->d_glob;
    g.r_words = r->r_words;
    *out = g;
    return LRPX_OK;
}

static AoaRel to_arel(const lrpx_aoa_trace* t, const lrpx_aoa_relstate* r) {
    AoaRel g;
    g.B = t->B; g.T = t->T; g.H = t->H; g.E = t->E; g.P = t->P; g.NH = t->NH; g.lens = r->lens;
    g.xh = t->xh; g.h = t->h; g.c = t->c; g.g = t->g; g.i = t->i; g.ctx = t->ctx; g.lin = t->lin; g.c_aoa = t->c_aoa;
    g.hc = t->hc; g.alpha = t->alpha;
    g.r_hn = r->r_hn; g.r_glob = r->r_glob; g.A = r->A; g.rx = r->rx; g.r_words = r->r_words;
    return g;
}

static int check_arel(const lrpx_aoa_trace* t, const lrpx_aoa_relstate* r) {
    LRPX_TRY(check_atrace(t));
    LRPX_REQUIRE(r && r->r_hn && r->r_glob && r->A && r->rx && r->r_words, "aoa: null relevance-state tensor");
    return LRPX_OK;
}

// The host loops of the AoA decoder in native code (lrpx_aoa_fwd_steps, lrpx_aoa_rel_steps).  Every launch is one of the entry points or
// one of the fused kernels above; what goes away is the
// interpreter between them: ~4 us per call through ctypes against ~1.5 us for a launch issued from here.  With a CNN stage
// behind it that is noise; the bottom-up path (no CNN, ~330 launches of 4 - 25 us per step of 640 maps) was bound by it.
template <int RT>
static int aoa_fused_steps(const lrpx_aoa_trace* tr, int t0, int t1, const lrpx_aoa_step_args* a, hipStream_t st) {
    const AoaFwd g = to_afwd(tr);
    const int H = tr->H, T = tr->T, B = tr->B;
    for (int t = t0; t < t1; ++t) {
        hipLaunchKernelGGL((aoa_linear_lstm_kernel<RT>), dim3(4 * H / 16), dim3(256), 0, st, g, t, a->w_cat_il, a->b_cat_il);
        LRPX_TRY(check_launch("aoa_linear_lstm"));
        LRPX_TRY(lrpx_linear_small(tr->h + (long)(t + 1) * H, (long)(T + 1) * H, a->w_qg, a->b_qg, a->qg, 2 * H, B, H, 2 * H, 0, st));
        LRPX_TRY(lrpx_aoa_fwd_attention(tr, t, a->qg, 2 * H, a->key, a->value, st));
        hipLaunchKernelGGL((aoa_linear_post_kernel<RT>), dim3(H / 16), dim3(256), 0, st, g, t, a->w_lin, a->b_lin, a->qg, 2 * H, a->glob,
                           a->emb, a->tok, a->tok_ld);
        LRPX_TRY(check_launch("aoa_linear_post"));
    }
    return LRPX_OK;
}

static int aoa_recurrence(const lrpx_aoa_trace* tr, const float* w_hh_il, const float* zin, const float* tab, const float* gimg,
                          const long long* tok, int tok_ld, hipStream_t st) {
    if (tr->B > 64) {
        // more than 64 images: slices of at most 64 through the SAME kernels (the recurrence is independent per image), so that an image's
        // trace does not depend on the batch it sits in (B = 65 used to leave the decoupled path altogether)
        const long T = tr->T, H = tr->H, W = tr->E + 2L * tr->H;
        for (int b0 = 0; b0 < tr->B; b0 += 64) {
            lrpx_aoa_trace sub = *tr;
            sub.B = tr->B - b0 < 64 ? tr->B - b0 : 64;
            sub.xh += b0 * T * W;
            sub.h += b0 * (T + 1) * H; sub.c += b0 * (T + 1) * H;
            sub.g += b0 * T * H; sub.i += b0 * T * H; sub.f += b0 * T * H;
            sub.ctx += b0 * T * H; sub.lin += b0 * T * H; sub.c_aoa += b0 * T * H; sub.hc += b0 * T * H;
            sub.alpha += b0 * T * tr->NH * (long)tr->P;
            if (sub.o) sub.o += b0 * T * H;
            if (sub.sg) sub.sg += b0 * T * H;
            LRPX_TRY(aoa_recurrence(&sub, w_hh_il, zin ? zin + b0 * T * 4 * H : nullptr, tab, gimg ? gimg + b0 * 4L * H : nullptr,
                                    tok ? tok + (long)b0 * tok_ld : nullptr, tok_ld, st));
        }
        return LRPX_OK;
    }
    const AoaFwd g = to_afwd(tr);
    const int H = tr->H, B = tr->B;
    for (int t = 0; t < tr->T; ++t) {
        with_row_tiles(B, [&](auto rt) { hipLaunchKernelGGL((aoa_rec_lstm_kernel<decltype(rt)::value>), dim3(4 * H / 16), dim3(256), 0, st, g, t, w_hh_il, zin, tab, gimg, tok, tok_ld); });
        LRPX_TRY(check_launch("aoa_rec_lstm"));
    }
    return LRPX_OK;
}

extern "C" {

int lrpx_aoa_fwd_pre(const lrpx_aoa_trace* tr, int t, const float* glob, const float* emb, const long long* tok,
                     int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_pre", {glob, "glob"}, {emb, "emb"}, {tok, "tok"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(glob && emb && tok && t >= 0 && t < tr->T, "aoa_fwd_pre: bad arguments");
    hipLaunchKernelGGL(aoa_fwd_pre_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_afwd(tr), t, glob, emb, tok,
                       tok_ld);
    return check_launch("aoa_fwd_pre");
}

int lrpx_aoa_fwd_lstm(const lrpx_aoa_trace* tr, int t, const float* zz, int ldz, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_lstm", {zz, "zz"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(zz && t >= 0 && t < tr->T, "aoa_fwd_lstm: bad arguments");
    hipLaunchKernelGGL(aoa_fwd_lstm_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_afwd(tr), t, zz, ldz);
    return check_launch("aoa_fwd_lstm");
}

int lrpx_aoa_fwd_attention(const lrpx_aoa_trace* tr, int t, const float* qg, int ldq, const float* key,
                           const float* value, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_attention", {qg, "qg"}, {key, "key"}, {value, "value"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(qg && key && value && t >= 0 && t < tr->T, "aoa_fwd_attention: bad arguments");
    const size_t lds = (size_t)(tr->H / tr->NH + tr->P + 8) * sizeof(float);
    hipLaunchKernelGGL(aoa_fwd_attention_kernel, dim3(tr->B, tr->NH), dim3(256), lds, (hipStream_t)stream, to_afwd(tr), t,
                       qg, ldq, key, value);
    return check_launch("aoa_fwd_attention");
}

int lrpx_aoa_fwd_post(const lrpx_aoa_trace* tr, int t, const float* qg, int ldq, const float* lin, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_post", {qg, "qg"}, {lin, "lin"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(qg && lin && t >= 0 && t < tr->T, "aoa_fwd_post: bad arguments");
    hipLaunchKernelGGL(aoa_fwd_post_kernel, dim3(tr->B), dim3(256), 0, (hipStream_t)stream, to_afwd(tr), t, qg, ldq, lin);
    return check_launch("aoa_fwd_post");
}

int lrpx_aoa_grad_init(const lrpx_aoa_trace* tr, const lrpx_aoa_gradstate* gs, const float* fcw, const long long* tok,
                       int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_grad_init", {fcw, "fcw"}, {tok, "tok"});
    AoaGrad g;
    LRPX_TRY(to_agrad(tr, gs, &g));
    LRPX_REQUIRE(fcw && tok, "aoa_grad_init: null pointer");
    hipLaunchKernelGGL(aoa_grad_init_kernel, dim3(g.B * g.T), dim3(256), 0, (hipStream_t)stream, g, fcw, tok, tok_ld);
    return check_launch("aoa_grad_init");
}

int lrpx_aoa_grad_step(const lrpx_aoa_trace* tr, const lrpx_aoa_gradstate* gs, int s, int phase, void* stream) {
    AoaGrad g;
    LRPX_TRY(to_agrad(tr, gs, &g));
    LRPX_REQUIRE(s >= 0 && s < g.T && (phase == 0 || phase == 1), "aoa_grad_step: bad step / phase");
    if (phase == 0) hipLaunchKernelGGL(aoa_grad_step0_kernel, dim3(g.B * g.T), dim3(256), 0, (hipStream_t)stream, g, s);
    else hipLaunchKernelGGL(aoa_grad_step1_kernel, dim3(g.B * g.T), dim3(256), 0, (hipStream_t)stream, g, s);
    return check_launch("aoa_grad_step");
}

int lrpx_aoa_grad_pix_rows(const lrpx_aoa_trace* tr, int head, const float* v1, const float* v2, float* d_feat, int C,
                           const int32_t* rows, int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_grad_pix_rows", {v1, "v1"}, {v2, "v2"}, {d_feat, "d_feat"}, {rows, "rows"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(v1 && v2 && d_feat && head >= 0 && head < tr->NH && C > 0 && C % 4 == 0, "aoa_grad_pix: bad arguments");
    LRPX_REQUIRE(rows ? (n_rows > 0 && n_rows <= tr->B * tr->T) : n_rows == tr->B * tr->T, "aoa_grad_pix: bad row list");
    const long total = (long)n_rows * tr->P * (C / 4);
    hipLaunchKernelGGL(aoa_grad_pix_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       tr->alpha, tr->T, tr->NH, tr->P, head, v1, v2, d_feat, C / 4, total, rows);
    return check_launch("aoa_grad_pix");
}

int lrpx_aoa_grad_pix(const lrpx_aoa_trace* tr, int head, const float* v1, const float* v2, float* d_feat, int C,
                      void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_grad_pix", {v1, "v1"}, {v2, "v2"}, {d_feat, "d_feat"});
    LRPX_REQUIRE(tr, "aoa_grad_pix: null trace");
    return lrpx_aoa_grad_pix_rows(tr, head, v1, v2, d_feat, C, nullptr, tr->B * tr->T, stream);
}

int lrpx_aoa_rel_init(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* fcw, const float* logit,
                      const long long* tok, int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_rel_init", {fcw, "fcw"}, {logit, "logit"}, {tok, "tok"});
    LRPX_TRY(check_arel(tr, rs));
    LRPX_REQUIRE(fcw && logit && tok, "aoa_rel_init: null pointer");
    hipLaunchKernelGGL(aoa_rel_init_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_arel(tr, rs), fcw,
                       logit, tok, tok_ld);
    return check_launch("aoa_rel_init");
}

int lrpx_aoa_rel_value_rows(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* r_ctx, const float* value,
                            int head, float* a_val, const int32_t* rows, int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_rel_value_rows", {r_ctx, "r_ctx"}, {value, "value"}, {a_val, "a_val"}, {rows, "rows"});
    LRPX_TRY(check_arel(tr, rs));
    LRPX_REQUIRE(r_ctx && value && a_val && head >= 0 && head < tr->NH, "aoa_rel_value: bad arguments");
    LRPX_REQUIRE(rows ? (n_rows > 0 && n_rows <= tr->B * tr->T) : n_rows == tr->B * tr->T, "aoa_rel_value: bad row list");
    hipLaunchKernelGGL(aoa_rel_value_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, to_arel(tr, rs),
                       r_ctx, value, head, a_val, rows, 0);
    return check_launch("aoa_rel_value");
}

int lrpx_aoa_rel_value_head(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* r_ctx, const float* value,
                            int head, float* a_val_head, const int32_t* rows, int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_rel_value_head", {r_ctx, "r_ctx"}, {value, "value"}, {a_val_head, "a_val_head"}, {rows, "rows"});
    LRPX_TRY(check_arel(tr, rs));
    LRPX_REQUIRE(r_ctx && value && a_val_head && head >= 0 && head < tr->NH && tr->H % tr->NH == 0, "aoa_rel_value_head: bad arguments");
    LRPX_REQUIRE(rows ? (n_rows > 0 && n_rows <= tr->B * tr->T) : n_rows == tr->B * tr->T, "aoa_rel_value_head: bad row list");
    hipLaunchKernelGGL(aoa_rel_value_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, to_arel(tr, rs),
                       r_ctx, value, head, a_val_head, rows, 1);
    return check_launch("aoa_rel_value_head");
}

int lrpx_aoa_rel_value(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* r_ctx, const float* value,
                       int head, float* a_val, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_rel_value", {r_ctx, "r_ctx"}, {value, "value"}, {a_val, "a_val"});
    LRPX_REQUIRE(tr, "aoa_rel_value: null trace");
    return lrpx_aoa_rel_value_rows(tr, rs, r_ctx, value, head, a_val, nullptr, tr->B * tr->T, stream);
}

int lrpx_aoa_rel_step(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, int s, int phase, void* stream) {
    LRPX_TRY(check_arel(tr, rs));
    LRPX_REQUIRE(s >= 0 && s < tr->T && (phase == 0 || phase == 1), "aoa_rel_step: bad step/phase");
    const AoaRel g = to_arel(tr, rs);
    if (phase == 0) hipLaunchKernelGGL(aoa_rel_a_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, g, s);
    else hipLaunchKernelGGL(aoa_rel_c_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, g, s);
    return check_launch("aoa_rel_step");
}

int lrpx_aoa_fwd_steps(const lrpx_aoa_trace* tr, int t0, int t1, const lrpx_aoa_step_args* a, void* stream) {
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(a && a->glob && a->emb && a->tok && a->w_cat && a->w_qg && a->w_lin && a->key && a->value && a->zz && a->qg &&
                     a->lin && t0 >= 0 && t0 <= t1 && t1 <= tr->T, "aoa_fwd_steps: bad arguments");
    const int B = tr->B, T = tr->T, H = tr->H, W = tr->E + 2 * tr->H;
    // fused steps (4 launches instead of 7): needs the interleaved gate rows, <= 64 images, dims the matrix-core linear takes
    if (a->w_cat_il && B <= 64 && W % 16 == 0 && H % 16 == 0 && t0 < t1) {
        LRPX_TRY(lrpx_aoa_fwd_pre(tr, t0, a->glob, a->emb, a->tok, a->tok_ld, stream));      // (later rows: gathered by the step before)
        hipStream_t st = (hipStream_t)stream;
        return with_row_tiles(B, [&](auto rt) { return aoa_fused_steps<decltype(rt)::value>(tr, t0, t1, a, st); });
    }
    for (int t = t0; t < t1; ++t) {
        LRPX_TRY(lrpx_aoa_fwd_pre(tr, t, a->glob, a->emb, a->tok, a->tok_ld, stream));
        LRPX_TRY(lrpx_linear_small(tr->xh + (long)t * W, (long)T * W, a->w_cat, a->b_cat, a->zz, 4 * H, B, W, 4 * H, 0, stream));
        LRPX_TRY(lrpx_aoa_fwd_lstm(tr, t, a->zz, 4 * H, stream));
        LRPX_TRY(lrpx_linear_small(tr->h + (long)(t + 1) * H, (long)(T + 1) * H, a->w_qg, a->b_qg, a->qg, 2 * H, B, H, 2 * H, 0, stream));
        LRPX_TRY(lrpx_aoa_fwd_attention(tr, t, a->qg, 2 * H, a->key, a->value, stream));
        LRPX_TRY(lrpx_linear_small(tr->ctx + (long)t * H, (long)T * H, a->w_lin, a->b_lin, a->lin, H, B, H, H, 0, stream));
        LRPX_TRY(lrpx_aoa_fwd_post(tr, t, a->qg, 2 * H, a->lin, stream));
    }
    return LRPX_OK;
}

int lrpx_aoa_fwd_inputs(const lrpx_aoa_trace* tr, const float* glob, const float* emb, const long long* tok, int tok_ld,
                        float* xin, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_inputs", {glob, "glob"}, {emb, "emb"}, {tok, "tok"}, {xin, "xin"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(glob && emb && tok, "aoa_fwd_inputs: null pointer");
    hipLaunchKernelGGL(aoa_fwd_inputs_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_afwd(tr), glob, emb, tok,
                       tok_ld, xin);
    return check_launch("aoa_fwd_inputs");
}

int lrpx_aoa_fwd_recurrence(const lrpx_aoa_trace* tr, const float* w_hh_il, const float* zin, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_recurrence", {w_hh_il, "w_hh_il"}, {zin, "zin"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(w_hh_il && zin && tr->H % 16 == 0, "aoa_fwd_recurrence: bad arguments (H %% 16)");
    return aoa_recurrence(tr, w_hh_il, zin, nullptr, nullptr, nullptr, 0, (hipStream_t)stream);
}

int lrpx_aoa_fwd_recurrence_tab(const lrpx_aoa_trace* tr, const float* w_hh_il, const float* tab, const float* gimg,
                                const long long* tok, int tok_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_recurrence_tab", {w_hh_il, "w_hh_il"}, {tab, "tab"}, {gimg, "gimg"}, {tok, "tok"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(w_hh_il && tab && gimg && tok && tok_ld >= tr->T && tr->H % 16 == 0,
                 "aoa_fwd_recurrence_tab: bad arguments (H %% 16)");
    return aoa_recurrence(tr, w_hh_il, nullptr, tab, gimg, tok, tok_ld, (hipStream_t)stream);
}

int lrpx_aoa_fwd_gather_h(const lrpx_aoa_trace* tr, float* hn, uint32_t* hn_amax, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_gather_h", {hn, "hn"}, {hn_amax, "hn_amax"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(hn, "aoa_fwd_gather_h: null pointer");
    hipLaunchKernelGGL(aoa_fwd_gather_h_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_afwd(tr), hn, hn_amax);
    return check_launch("aoa_fwd_gather_h");
}

int lrpx_aoa_fwd_attention_all(const lrpx_aoa_trace* tr, const float* qg, int ldq, const float* key, const float* value,
                               uint32_t* ctx_amax, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_attention_all", {qg, "qg"}, {key, "key"}, {value, "value"}, {ctx_amax, "ctx_amax"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(qg && key && value && tr->H % tr->NH == 0, "aoa_fwd_attention_all: bad arguments");
    const size_t lds = (size_t)(tr->H / tr->NH + tr->P) * sizeof(float);
    hipLaunchKernelGGL(aoa_fwd_attention_all_kernel, dim3(tr->B * tr->T, tr->NH), dim3(64), lds, (hipStream_t)stream, to_afwd(tr), qg,
                       ldq, key, value, ctx_amax);
    return check_launch("aoa_fwd_attention_all");
}

int lrpx_aoa_fwd_post_all(const lrpx_aoa_trace* tr, const float* qg, int ldq, const float* lin, uint32_t* hc_amax, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_fwd_post_all", {qg, "qg"}, {lin, "lin"}, {hc_amax, "hc_amax"});
    LRPX_TRY(check_atrace(tr));
    LRPX_REQUIRE(qg && lin, "aoa_fwd_post_all: null pointer");
    hipLaunchKernelGGL(aoa_fwd_post_all_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, to_afwd(tr), qg, ldq, lin, hc_amax);
    return check_launch("aoa_fwd_post_all");
}

int lrpx_aoa_rel_steps(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, int n_steps, const lrpx_conv_desc* dense,
                       const int32_t* idx, int idx_ld, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_rel_steps", {idx, "idx"});
    LRPX_TRY(check_arel(tr, rs));
    LRPX_REQUIRE(dense && idx && n_steps >= 0 && n_steps <= tr->T && idx_ld >= tr->B * tr->T, "aoa_rel_steps: bad arguments");
    lrpx_conv_desc d = *dense;
    const AoaRel g = to_arel(tr, rs);
    if (n_steps > 0) LRPX_TRY(lrpx_aoa_rel_step(tr, rs, 0, 0, stream));
    for (int s = 0; s < n_steps; ++s) {
        d.map2img = idx + (long)s * idx_ld;          // row -> source row of the multiplicand at lock-step s
        LRPX_TRY(lrpx_conv_mfma(&d, stream));
        if (s + 1 < n_steps) {                       // phase 1 of step s and phase 0 of step s + 1 in one launch
            hipLaunchKernelGGL(aoa_rel_ca_kernel, dim3(tr->B * tr->T), dim3(256), 0, (hipStream_t)stream, g, s);
            LRPX_TRY(check_launch("aoa_rel_ca"));
        } else {
            LRPX_TRY(lrpx_aoa_rel_step(tr, rs, s, 1, stream));
        }
    }
    return LRPX_OK;
}

int lrpx_aoa_rel_steps_fused(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const lrpx_conv_desc* dense, const int32_t* idx,
                             int idx_ld, float* a_alt, float* wpart, float* coef, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_aoa_rel_steps_fused", {idx, "idx"}, {a_alt, "a_alt"}, {wpart, "wpart"}, {coef, "coef"});
    LRPX_TRY(check_arel(tr, rs));
    const int T = tr->T, rows = tr->B * tr->T, H = tr->H;
    LRPX_REQUIRE(dense && idx && a_alt && wpart && coef && idx_ld >= rows, "aoa_rel_steps_fused: bad arguments");
    LRPX_REQUIRE((dense->f16x3 == 1 || (dense->f16x3 == 0 && !dense->bf16x6)) && dense->taps == 1 && dense->epi == EPI_REL && dense->in == rs->A && dense->x && !dense->u &&
                     dense->cin == H && tr->E == H && H == 512 && dense->n_oc == 3 * H && dense->oc_split == 3 * H && dense->n_maps == rows &&
                     dense->pix_per_map == 1, "aoa_rel_steps_fused: the fused lock-step is built for E = H = 512 on the f16x3 gate rule or (f16x3 = 0: weights "
                     "from lrpx_pack_weights, DENSE_T, kc = 32) on the fp32 MFMA");
    hipStream_t st = (hipStream_t)stream;
    LRPX_TRY(lrpx_aoa_rel_step(tr, rs, 0, 0, stream));                 // A of lock-step 0 (:1116-1120)
    ConvArgs a = {};
    a.wp = dense->wpacked; a.n_maps = rows; a.cin = H; a.n_oc = 3 * H; a.pix_per_map = 1; a.epi = EPI_REL; a.oc_split = 3 * H;
    a.X = dense->x; a.ksplit = 1;
    float *q1 = coef, *dg = coef + (size_t)rows * H;
    int* tmax = reinterpret_cast<int*>(coef + (size_t)2 * rows * H);
    hipLaunchKernelGGL(aoa_rel_coef_kernel, dim3(rows), dim3(256), 0, st, to_arel(tr, rs), q1, dg, tmax);
    LRPX_TRY(check_launch("aoa_rel_coef"));
    AoaStepFuse fz;
    fz.T = T; fz.tmax = tmax; fz.q1 = q1; fz.dg = dg; fz.r_glob = rs->r_glob; fz.wpart = wpart;
    float* buf[2] = {rs->A, a_alt};
    for (int s = 0; s < T; ++s) {
        a.in = buf[s & 1];
        a.map2img = idx + (long)s * idx_ld;        // row -> source row of the multiplicand at lock-step s
        fz.s = s; fz.A_next = buf[(s + 1) & 1];
        if (dense->f16x3) LRPX_TRY(launch_dense_small_f16x3_aoa_step(a, fz, st));
        else LRPX_TRY(launch_dense_ks_aoa_step(a, fz, st));
    }
    hipLaunchKernelGGL(rel_words_norm_parts_kernel, dim3((rows + 63) / 64), dim3(64), 0, st, rs->r_words, wpart, rs->lens, rows, T);
    return check_launch("rel_words_norm_parts");
}

}  // extern "C"
