// What the decoder files (decoder_blocks.hip: the model-agnostic kernels; decoder_gridtd.hip, decoder_aoa.hip, lrpx_adaatt.hip: one model
// each) share: the point-wise helpers, the LSTM cell, the wave / block reductions, the K loop of the skinny linears on the fp32 matrix cores
// with the sum of its four K-slices, the body of `AdaptiveAttention.forward` (models/gridTDmodel.py:71-103 and
// models/adaptiveattention.py:56-98 are the same module), and on the host the choice of the row tile.  One text, so the decoders round
// alike: a kernel that calls one of these forms the same sums in the same order as every other caller.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"
#include "conv_mfma.h"

namespace lrpx {

// host: the row tile RT (16 rows each) of the matrix-core kernels for B <= 64 rows; calls f(std::integral_constant<int, RT>{})
template <class F>
auto with_row_tiles(int B, F&& f) {
    if (B <= 16) return f(std::integral_constant<int, 1>{});
    if (B <= 32) return f(std::integral_constant<int, 2>{});
    if (B <= 48) return f(std::integral_constant<int, 3>{});
    return f(std::integral_constant<int, 4>{});
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float eps_id(float r, float x, float z) { return (x / stab_eps(z)) * r; }   // weight=eye rule

// The LSTM cell of every decoder (models/gridTDmodel.py:777-784, models/aoamodel.py:1030-1033, models/adaptiveattention.py:554-565) from the
// four pre-activations of one hidden unit and its old cell state: the gates and the new cell state; the caller forms h = o tanh(cn) and
// keeps what its trace wants (the g gate is traced as the pre-activation zg itself).
struct LstmCell { float i, f, o, cn; };
__device__ __forceinline__ LstmCell lstm_cell(float zi, float zf, float zg, float zo, float c_old) {
    const float i = sigmoidf_(zi), f = sigmoidf_(zf), o = sigmoidf_(zo);
    const float cn = f * c_old + i * tanhf(zg);
    return {i, f, o, cn};
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// block-wide reductions for 256-thread blocks (4 waves); `red` has >= 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The K loop of the skinny linears on the fp32 matrix cores (linear_mfma_kernel and the fused step kernels share it: the same dot products
// in the same order, bit-identical traces).  The 4 waves split K; a lane loads ONE float4 of its weight row and one of its x row per 16 k
// (lane = (feature or row) lane & 15, k quad lane >> 4: component j of the two float4s is the operand pair of MFMA j).
// Round 6: FOUR accumulators per row tile take the wave's k-steps in turn (k-step s -> accumulator s % 4): a sum of 2048 products is formed
// from 16 partial sums of 128 instead of 4 of 512 - the gate pre-activations of a gridTD trace moved from 8e-7 to 3e-7 of their fp64 values
// (what an fp32 CPU GEMM gives: tests/diag_t20_words.py), and with them the worst T = 20 r_words row of the goldens from 1.0e-5 to 1.4e-6 of
// fp64.  No faster: the kernel is at the rate its weights stream in (11 us per gridTD gate linear, 5 us of them the launch floor).
template <int RT>
__device__ __forceinline__ void linear_mfma_core(const float* __restrict__ x, long ldx, const float* __restrict__ w, int B, int K,
                                                 int N, float (&red)[4][RT][16][17], const int n0) {
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
    const int nl = lane & 15, kq = lane >> 4;
    const int kslice = ((K / 16 + 3) / 4) * 16;                        // K % 16 == 0 (host-checked)
    const int k_lo = wv_ * kslice, k_hi = min(K, k_lo + kslice);
    const float* __restrict__ wrow = w + (long)min(n0 + nl, N - 1) * K + kq * 4;
    const float* __restrict__ xrow[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) xrow[r] = x + (long)min(r * 16 + nl, B - 1) * ldx + kq * 4;
    constexpr int NA = 4;                                              // accumulators per row tile (k-step s -> accumulator s % NA)
    constexpr int NW = RT <= 2 ? 8 : 4;                                // k-steps of weights in flight per wave (16 measured no faster: the
                                                                       // kernel streams its 13 - 17 MB of fp32 weights at ~2.8 TB/s either way)
    constexpr int NX = 4;                                              // k-steps of x rows in flight (L2 hits)
    f32x4 acc[RT][NA];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int u = 0; u < NA; ++u) acc[r][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = k_lo; k0 < k_hi; k0 += 16 * NW) {
        f32x4 wq[NW];
#pragma unroll
        for (int u = 0; u < NW; ++u) wq[u] = *reinterpret_cast<const f32x4*>(wrow + min(k0 + 16 * u, k_hi - 16));   // (past the slice: re-read, MFMAs skipped)
#pragma unroll
        for (int v = 0; v < NW; v += NX) {
            f32x4 xq[RT][NX];
#pragma unroll
            for (int u = 0; u < NX; ++u)
#pragma unroll
                for (int r = 0; r < RT; ++r) xq[r][u] = *reinterpret_cast<const f32x4*>(xrow[r] + min(k0 + 16 * (v + u), k_hi - 16));
#pragma unroll
            for (int u = 0; u < NX; ++u) {
                if (k0 + 16 * (v + u) < k_hi) {                        // (wave-uniform)
#pragma unroll
                    for (int r = 0; r < RT; ++r)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[r][u % NA] = __builtin_amdgcn_mfma_f32_16x16x4f32(xq[r][u][j], wq[v + u][j], acc[r][u % NA], 0, 0, 0);
                }
            }
        }
    }
    // result layout: column (feature) lane & 15, rows 4 * (lane >> 4) + i
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wv_][r][4 * kq + i][nl] = (acc[r][0][i] + acc[r][1][i]) + (acc[r][2][i] + acc[r][3][i]);
    __syncthreads();
}

// ... and what every caller reads back: element (row tile r, row, col) of the product, the four K-slices summed in wave order
template <int RT>
__device__ __forceinline__ float red4(const float (&red)[4][RT][16][17], int r, int row, int col) {
    return (red[0][r][row][col] + red[1][r][row][col]) + (red[2][r][row][col] + red[3][r][row][col]);
}

// AdaptiveAttention.forward (models/gridTDmodel.py:71-103 = models/adaptiveattention.py:56-98), two kernels so that the rows fill the chip:
//  (1) scores: grid (rows, pixel blocks): h_proj[k] = W_g[k].h, s_proj[k] = W_s[k].s + b_s[k],
//      z[k] = w_h . tanh(att_img[k,:] + h_proj[k])   (ht_proj is broadcast along the row, :82);
//      att_img = W_v_proj(V)+b_v is time-invariant and precomputed.
//  (2) context: grid (rows, channel blocks): sentinel score, both softmaxes, context, c_hat.
// (latency-bound at B = 16: with 28 pixels / 128 channels per block the two kernels ran 30 + 29 us per time step on 112 / 64
// workgroups, each wave walking 7 pixels or each thread 98 pixels in sequence; now one pixel per wave and 8 pixel
// slices per channel)
constexpr int ATT_PB = 4;     // pixels per block in (1): one per wave
constexpr int ATT_CB = 32;    // channels per block in (2): 8 pixel slices x 32 channels per block

// (1) for pixel block `yblk` of image b: hv / sv [H] are the hidden state and the sentinel of the row (LDS), zsc its [z | h_proj | s_proj]
__device__ __forceinline__ void att_scores_block(const float* hv, const float* sv, int H, int P, int b, int yblk,
                                                 const float* __restrict__ att_img, const float* __restrict__ Wg,
                                                 const float* __restrict__ Ws, const float* __restrict__ bs,
                                                 const float* __restrict__ wh, float* __restrict__ zsc) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k0 = yblk * ATT_PB, k1 = min(k0 + ATT_PB, P);
    for (int k = k0 + wv; k < k1; k += 4) {
        float a = 0.f, c2 = 0.f;
        for (int c = lane; c < H; c += 64) { a += Wg[(long)k * H + c] * hv[c]; c2 += Ws[(long)k * H + c] * sv[c]; }
        a = wave_sum(a); c2 = wave_sum(c2);
        float z = 0.f;
        for (int j = lane; j < P; j += 64) z += wh[j] * tanhf(att_img[((long)b * P + k) * P + j] + a);
        z = wave_sum(z);
        if (lane == 0) { zsc[k] = z; zsc[P + k] = a; zsc[2 * P + k] = c2 + bs[k]; }
    }
}

// (2) for channel block `yblk` of image b: sc = the row's [z | h_proj | s_proj]; sm = (max(2P+1, 256) + 8) floats of LDS.  Every block forms
// both softmaxes; the block with `first` writes alpha_out [P] and *beta_out.  Returns beta; `ctx` is the context of channel
// yblk * ATT_CB + (tid & 31), valid in the threads tid < 32 (a sum of 8 pixel slices in slice order)
__device__ __forceinline__ float att_context_block(const float* __restrict__ sc, float* sm, int H, int P, int b, int yblk, bool first,
                                                   const float* __restrict__ Vp, const float* __restrict__ wh,
                                                   float* __restrict__ alpha_out, float* __restrict__ beta_out, float& ctx) {
    const int tid = threadIdx.x;
    float* zsc = sm;            // P+1
    float* alpha = zsc + P + 1; // P
    float* red = zsc + (2 * P + 1 > 256 ? 2 * P + 1 : 256);     // 8 (behind the 256 partial sums that reuse zsc / alpha)
    for (int k = tid; k < P; k += 256) zsc[k] = sc[k];
    {   // sentinel score = w_h . tanh(s_proj + h_proj)   (:94)
        float a = 0.f;
        for (int j = tid; j < P; j += 256) a += wh[j] * tanhf(sc[2 * P + j] + sc[P + j]);
        a = block_sum(a, red);
        if (tid == 0) zsc[P] = a;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int k = tid; k < P; k += 256) m = fmaxf(m, zsc[k]);
    m = block_max(m, red);
    float e = 0.f;
    for (int k = tid; k < P; k += 256) e += expf(zsc[k] - m);
    const float denom = block_sum(e, red);
    const float m2 = fmaxf(m, zsc[P]);
    float e2 = 0.f;
    for (int k = tid; k <= P; k += 256) e2 += expf(zsc[k] - m2);
    const float denom2 = block_sum(e2, red);
    const float beta = expf(zsc[P] - m2) / denom2;
    __syncthreads();
    for (int k = tid; k < P; k += 256) {
        const float a = expf(zsc[k] - m) / denom;
        alpha[k] = a;
        if (first) alpha_out[k] = a;
    }
    if (tid == 0 && first) *beta_out = beta;
    __syncthreads();
    // context for this block's 32 channels: thread = (pixel slice tid / 32, channel tid % 32) - 128-byte runs per slice -
    // partial sums through LDS, summed in slice order
    const int c = yblk * ATT_CB + (tid & 31), part = tid >> 5;
    float a = 0.f;
    if (c < H)
        for (int k = part; k < P; k += 8) a += Vp[((long)b * P + k) * H + c] * alpha[k];
    float* psum = zsc;                     // (P + 1 >= 8 * 32 floats are not needed any more: alpha is its own array)
    __syncthreads();
    psum[tid] = a;
    __syncthreads();
    if (part == 0) {
        a = psum[tid];
#pragma unroll
        for (int q = 1; q < 8; ++q) a += psum[q * 32 + tid];
    }
    ctx = a;
    return beta;
}

}  // namespace lrpx
