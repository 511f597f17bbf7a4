// Decoder-side kernels of the LRP hot path that no model owns: the skinny linear, the image-side constants, arg-max / beam selection,
// the LRP-inference re-weighting, and the point-wise and pixel-spread kernels the explainers of every model launch.  The models'
// own kernels and host loops are in decoder_gridtd.hip, decoder_aoa.hip and lrpx_adaatt.hip; they reach these through the C entry points.
//
// Everything here is small next to the VGG16 relevance pass (<1 % of the FLOPs), HBM / latency bound.
// Row r = b*T + t is the explanation of word t of image b.  Trace tensors are [B][T(+1)][...] fp32; token ids int64 (torch.long).
#include <math.h>

#include "common.h"
#include "decoder_shared.h"

namespace lrpx {

// ------------------------------------------------------------------------------------------------
// skinny linear: out[b][n] = act(sum_k x[b][k] * w[n][k] + bias[n]) for a handful of rows b.
// One wave per NPW output features; lanes split K in float4; rows live in register accumulators.
// Weight-read bound (each weight byte is read once per 16-row chunk, from L2).
// ------------------------------------------------------------------------------------------------
template <int NPW, int BCH>
__global__ __launch_bounds__(256) void linear_small_kernel(const float* __restrict__ x, long ldx,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, long ldo, int B, int K, int N,
                                                           int act) {
    // one workgroup per NPW output features; its 4 waves split K (a 16-row problem has too few outputs to fill the
    // chip with one wave per feature group, and one wave's serial K loop is a chain of L2 round trips)
    __shared__ float red[4][NPW * BCH];
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
    const int n0 = blockIdx.x * NPW;
    const int K4 = K >> 2;
    const int kq = (K4 + 3) / 4, k_lo = wv_ * kq, k_hi = min(K4, k_lo + kq);
    for (int b0 = 0; b0 < B; b0 += BCH) {
        float acc[NPW][BCH];
#pragma unroll
        for (int j = 0; j < NPW; ++j)
#pragma unroll
            for (int bb = 0; bb < BCH; ++bb) acc[j][bb] = 0.f;
        for (int k4 = k_lo + lane; k4 < k_hi; k4 += 64) {
            f32x4 wv[NPW];
#pragma unroll
            for (int j = 0; j < NPW; ++j) {
                const int n = min(n0 + j, N - 1);
                wv[j] = reinterpret_cast<const f32x4*>(w + (long)n * K)[k4];
            }
#pragma unroll
            for (int bb = 0; bb < BCH; ++bb) {
                const int b = min(b0 + bb, B - 1);
                const f32x4 xv = reinterpret_cast<const f32x4*>(x + (long)b * ldx)[k4];
#pragma unroll
                for (int j = 0; j < NPW; ++j)
                    acc[j][bb] += wv[j][0] * xv[0] + wv[j][1] * xv[1] + wv[j][2] * xv[2] + wv[j][3] * xv[3];
            }
        }
        __syncthreads();                 // (previous row chunk's reduction has been read)
#pragma unroll
        for (int j = 0; j < NPW; ++j)
#pragma unroll
            for (int bb = 0; bb < BCH; ++bb) {
                const float v = wave_sum(acc[j][bb]);
                if (lane == 0) red[wv_][j * BCH + bb] = v;
            }
        __syncthreads();
        if (threadIdx.x < NPW * BCH) {
            const int j = threadIdx.x / BCH, bb = threadIdx.x % BCH;
            const int n = n0 + j, b = b0 + bb;
            float v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
            if (n < N && b < B) {
                if (bias) v += bias[n];
                if (act == 1) v = v > 0.f ? v : 0.f;
                out[(long)b * ldo + n] = v;
            }
        }
    }
}

// (linear_mfma_core, the K loop of the skinny linears on the fp32 matrix cores: decoder_shared.h)
// The same skinny linear on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 products): M = 16 rows b per row tile,
// N = 16 output features per workgroup, the 4 waves split K.  A lane loads ONE float4 of its weight row and one of its x
// row per 16 k (lane = (feature or row) lane & 15, k quad lane >> 4: component j of the two float4s is the operand pair of
// MFMA j) - no cross-lane reduction at all: the VALU version spends 64 wave reductions (384 ds_bpermute) per wave and
// ran 22 us for a 16 x 1536 x 2560 problem (0.7 TB/s of weights).  The four K-slices meet in LDS, summed in wave order.
template <int RT>
__global__ __launch_bounds__(256) void linear_mfma_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out, long ldo,
                                                          int B, int K, int N, int act) {
    __shared__ float red[4][RT][16][17];
    const int n0 = blockIdx.x * 16;
    linear_mfma_core<RT>(x, ldx, w, B, K, N, red, n0);
    for (int e = threadIdx.x; e < RT * 256; e += 256) {
        const int r = e >> 8, row = (e >> 4) & 15, col = e & 15;
        const int b = r * 16 + row, n = n0 + col;
        if (b < B && n < N) {
            float v = red4<RT>(red, r, row, col);
            if (bias) v += bias[n];
            if (act == 1) v = v > 0.f ? v : 0.f;
            out[(long)b * ldo + n] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// image-side constants: avg over pixels, relu
// ------------------------------------------------------------------------------------------------
__global__ void mean_pixels_kernel(const float* __restrict__ f, float* __restrict__ avg, int P, int C, float scale) {
    // block = 64 channels x 4 pixel slices (a lone thread per channel walked the P pixels as a chain of dependent adds on
    // 32 workgroups: 76 us for 6 MB)
    __shared__ float part[4][64];
    const int b = blockIdx.y;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    float s = 0.f;
    if (c < C)
        for (int p = q; p < P; p += 4) s += f[((long)b * P + p) * C + c];
    part[q][threadIdx.x & 63] = s;
    __syncthreads();
    if (q == 0 && c < C) avg[(long)b * C + c] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x])) * scale;
}

__global__ void relu_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = fmaxf(x[i], 0.f);
}

// logit of the target word: dot(fc.weight[k], hc[b,t]) + fc.bias[k]   (one wave per row)
__global__ void target_logit_kernel(const float* __restrict__ hc, const float* __restrict__ fcw,
                                    const float* __restrict__ fcb, const long long* __restrict__ tok, int tok_ld,
                                    float* __restrict__ logit, int B, int T, int H) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B * T) return;
    const int b = row / T, t = row - b * T, lane = threadIdx.x & 63;
    const long long k = tok[(long)b * tok_ld + t + 1];
    float a = 0.f;
    for (int c = lane; c < H; c += 64) a += fcw[k * H + c] * hc[(long)row * H + c];
    a = wave_sum(a);
    if (lane == 0) logit[row] = a + fcb[k];
}

// argmax over the vocabulary (first maximum wins, like torch.argmax / topk(1)) — one block per row
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, long ld, int n,
                                                          long long* __restrict__ out) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const float* r = x + (long)blockIdx.x * ld;
    float best = -INFINITY; int idx = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) { const float v = r[i]; if (v > best) { best = v; idx = i; } }
    bv[threadIdx.x] = best; bi[threadIdx.x] = idx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float v = bv[threadIdx.x + s]; const int i2 = bi[threadIdx.x + s];
            if (v > bv[threadIdx.x] || (v == bv[threadIdx.x] && i2 < bi[threadIdx.x])) { bv[threadIdx.x] = v; bi[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = bi[0];
}

// ------------------------------------------------------------------------------------------------
// LRP-inference decoding (models/gridTDmodel.py:548-577, :631-702): per step the predicted word's logit is
// redistributed to the two fc summands, both relevance vectors become weights around 1, and the logits are
// recomputed from the re-weighted fc input.
// ------------------------------------------------------------------------------------------------
// get_lrp_weight_step (:548-577) + the re-weighted fc input (:687).  One block per image, H = 512, 256 threads.
// h / ctx: the two fc summands of row b (row strides ldh / ldc).  lsm: the AoA model hands the rule the log-softmax of
// the scores instead of the scores (models/aoamodel.py:721-723): relevance and stabilised output are log p(k).
__global__ __launch_bounds__(256) void lrp_reweight_kernel(const float* __restrict__ pred, long ld, int V,
                                                           const float* __restrict__ hrow, long ldh,
                                                           const float* __restrict__ crow, long ldc,
                                                           const float* __restrict__ fcw,
                                                           const unsigned char* __restrict__ skip,
                                                           float* __restrict__ hcw, int H, int lsm) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* r = pred + (long)b * ld;
    const float* hp = hrow + (long)b * ldh;
    const float* cp = crow + (long)b * ldc;
    float best = -INFINITY; int idx = 0x7fffffff;
    for (int i = tid; i < V; i += 256) { const float v = r[i]; if (v > best) { best = v; idx = i; } }
    bv[tid] = best; bi[tid] = idx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float v = bv[tid + s]; const int i2 = bi[tid + s];
            if (v > bv[tid] || (v == bv[tid] && i2 < bi[tid])) { bv[tid] = v; bi[tid] = i2; }
        }
        __syncthreads();
    }
    const int k = min(bi[0], V - 1);            // (all-NaN row: keep the index in range)
    float pk = bv[0];
    float* out = hcw + (long)b * H;
    if (skip[k]) {                                 // stop words and specials: both weights are 1 (:557-558)
        for (int c = tid; c < H; c += 256) out[c] = cp[c] * 1.f + 1.f * hp[c];
        return;
    }
    if (lsm) {                                     // log_softmax(pred)[k] = -log sum exp(pred - max)
        float se = 0.f;
        for (int i = tid; i < V; i += 256) se += expf(r[i] - pk);
        se = block_sum(se, red);
        pk = -logf(se);
        __syncthreads();
    }
    const float zt = stab_eps(pk);
    float rh[2], rc[2], mh = 0.f, mc = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = tid + j * 256;
        const float h2 = hp[c], ch = cp[c];
        const float hc = h2 + ch;
        const float r_hc = (fcw[(long)k * H + c] * hc / zt) * pk;     // one-hot epsilon rule through fc
        rh[j] = eps_id(r_hc, h2, hc);
        rc[j] = eps_id(r_hc, ch, hc);
        mh = fmaxf(mh, fabsf(rh[j])); mc = fmaxf(mc, fabsf(rc[j]));
    }
    mh = block_max(mh, red);
    __syncthreads();
    mc = block_max(mc, red);
    if (mh == 0.f) mh = 1.f;                       // LRPtools/utils.py:59
    if (mc == 0.f) mc = 1.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = tid + j * 256;
        const float w_h = rh[j] / mh + 1.f, w_c = rc[j] / mc + 1.f;
        out[c] = cp[c] * w_c + w_h * hp[c];
    }
}

// argmax of log_softmax(x) and its value (sample_next_word greedy, :522-526): one block per row
__global__ __launch_bounds__(256) void argmax_logprob_rows_kernel(const float* __restrict__ x, long ld, int n,
                                                                  long long* __restrict__ out, float* __restrict__ lp) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    __shared__ float red[8];
    const int tid = threadIdx.x;
    const float* r = x + (long)blockIdx.x * ld;
    float best = -INFINITY; int idx = 0x7fffffff;
    for (int i = tid; i < n; i += 256) { const float v = r[i]; if (v > best) { best = v; idx = i; } }
    bv[tid] = best; bi[tid] = idx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float v = bv[tid + s]; const int i2 = bi[tid + s];
            if (v > bv[tid] || (v == bv[tid] && i2 < bi[tid])) { bv[tid] = v; bi[tid] = i2; }
        }
        __syncthreads();
    }
    const float mx = bv[0];
    float se = 0.f;
    for (int i = tid; i < n; i += 256) se += expf(r[i] - mx);
    se = block_sum(se, red);
    if (tid == 0) { out[blockIdx.x] = min(bi[0], n - 1); lp[blockIdx.x] = -logf(se); }   // x[k] - mx = 0
}


// Beam-search step (GridTDModel.beam_search, models/gridTDmodel.py:437-444; AOAModel.beam_search): the k best of
// cum[r] + log_softmax(x[r])[w] over the n_rows live beams (flat index r * n + w, value).  One workgroup: row maxima and
// log-sum-exps, a per-thread top-k (k <= 4) over the flat range, then k rounds of a block-wide arg-max over the list heads
// (1024 threads: one workgroup has to walk n_rows x vocab scores three times, so the width of the group is the speed).
// Ties: lower flat index first.
// The selection is `beam_topk_block`: `beam_topk_kernel` (one image, the winners go to memory) and `beam_step_batch_kernel` (one workgroup
// per image, the winners stay in registers for the bookkeeping) call the same body - the same sums in the same order.  Every thread
// returns the k winners, best first: win_i[o] the flat index (BEAM_NONE where the range holds fewer than k scores), win_v[o] the score.
constexpr int BEAM_NONE = 0x7fffffff;
// What a selection does to log_softmax(x[r])[w] before the cumulative score is added.  `BeamPlain`: nothing - the beam search.
// `BeamDiverse` (diverse beam search, models/gridTDmodel.py:346-349): `diversity` comes off the columns of at most 8 word ids (-1: unused).
// Two types, so two instantiations of `beam_topk_block`: the plain one carries no trace of the other.
struct BeamPlain {
    __device__ __forceinline__ float operator()(float lp, int) const { return lp; }
};
struct BeamDiverse {
    int id[8];
    float diversity;
    __device__ __forceinline__ float operator()(float lp, int w) const {
        bool hit = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) hit |= w == id[q];
        return hit ? lp - diversity : lp;
    }
};
template <int KMAX, class ADJUST = BeamPlain>
__device__ __forceinline__ void beam_topk_block(const float* __restrict__ x, long ld, int n_rows, int n,
                                                const float* __restrict__ cum, int k, int (&win_i)[KMAX], float (&win_v)[KMAX],
                                                const ADJUST& adjust = ADJUST()) {
    constexpr int NT = 1024, NW = NT / 64;
    __shared__ float red[NW];
    __shared__ float lse[8];
    __shared__ float cv[NW];
    __shared__ int ci[NW];
    const int tid = threadIdx.x;
    for (int r = 0; r < n_rows; ++r) {
        const float* xr = x + (long)r * ld;
        float m = -INFINITY;
        for (int i = tid; i < n; i += NT) m = fmaxf(m, xr[i]);
        m = wave_max(m);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        m = red[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w]);
        float se = 0.f;
        for (int i = tid; i < n; i += NT) se += expf(xr[i] - m);
        se = wave_sum(se);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = se;
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += red[w];
            lse[r] = m + logf(t);
        }
    }
    __syncthreads();
    float bv[KMAX];
    int bi[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { bv[j] = -INFINITY; bi[j] = 0x7fffffff; }
    for (int r = 0; r < n_rows; ++r) {
        const float off = (cum ? cum[r] : 0.f), l = lse[r];
        const float* xr = x + (long)r * ld;
        for (int w = tid; w < n; w += NT) {
            float v = off + adjust(xr[w] - l, w);
            int vi = r * n + w;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {          // insertion into the sorted list (descending value, ascending index)
                const bool better = v > bv[j] || (v == bv[j] && vi < bi[j]);
                const float tv = better ? bv[j] : v; const int ti = better ? bi[j] : vi;
                bv[j] = better ? v : bv[j]; bi[j] = better ? vi : bi[j];
                v = tv; vi = ti;
            }
        }
    }
    // merge: k rounds of a block-wide arg-max over the heads of the 1024 sorted lists (value descending, flat index ascending on ties)
    int head = 0;
    for (int o = 0; o < k; ++o) {
        float v = -INFINITY; int vi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j == head) { v = bv[j]; vi = bi[j]; }
        float wv = v; int wi = vi;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(wv, off, 64); const int oi = __shfl_xor(wi, off, 64);
            const bool take = ov > wv || (ov == wv && oi < wi);
            wv = take ? ov : wv; wi = take ? oi : wi;
        }
        __syncthreads();                               // (cv / ci of the previous round have been read)
        if ((tid & 63) == 0) { cv[tid >> 6] = wv; ci[tid >> 6] = wi; }
        __syncthreads();
        float best = cv[0]; int bidx = ci[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const bool take = cv[w] > best || (cv[w] == best && ci[w] < bidx);
            best = take ? cv[w] : best; bidx = take ? ci[w] : bidx;
        }
        if (bidx != 0x7fffffff && vi == bidx) ++head;                       // the owner of the winner moves on to its next candidate
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j == o) { win_i[j] = bidx; win_v[j] = best; }
    }
}

template <int KMAX>
__global__ __launch_bounds__(1024) void beam_topk_kernel(const float* __restrict__ x, long ld, int n_rows, int n,
                                                         const float* __restrict__ cum, int k,
                                                         long long* __restrict__ out_idx, float* __restrict__ out_val) {
    int wi[KMAX];
    float wv[KMAX];
    beam_topk_block<KMAX>(x, ld, n_rows, n, cum, k, wi, wv);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) { out_idx[j] = wi[j] != BEAM_NONE ? wi[j] : 0; out_val[j] = wv[j]; }
    }
}

// one of four registers by a run-time s (an indexed register array would leave the registers)
template <typename T>
__device__ __forceinline__ T beam_pick(T a, T b, T c, T d, int s) {
    T r = a;
    r = s == 1 ? b : r;
    r = s == 2 ? c : r;
    r = s == 3 ? d : r;
    return r;
}

// One step of the reference's beam search (models/gridTDmodel.py:437-467) for N images, one workgroup per image, the state on the device
// (lrpx_beam_batch, include/lrpx.h).  Image i owns rows i k .. i k + k - 1, live rows first.  The selection is `beam_topk_block` over the
// image's live rows (step 0: row 0 alone with k candidates, :440-443); the bookkeeping - what `run_beam_search` (explainers/beam.py) does in
// Python lists - runs in every thread on the same registers: a candidate that is <end> is set aside and replaces the kept complete
// sequence only with a strictly greater score (candidates come best first, the reference keeps the first maximum, :469-470), the others
// are compacted to the front in their order.  Then thread c owns column c: it reads the k tokens of sequence position c (and the k values
// of every state tensor's feature c at time t + 1) into registers and writes them back permuted - no scratch buffer and no
// read-after-write hazard.  An image without live rows is a no-op.
template <int KMAX>
__global__ __launch_bounds__(1024) void beam_step_batch_kernel(const lrpx_beam_batch p, const float* __restrict__ x, long ld, int t) {
    constexpr int NT = 1024;
    static_assert(KMAX == 4, "beam_pick takes four registers");
    const int img = blockIdx.x, tid = threadIdx.x, k = p.k, V = p.V;
    const int nl = p.n_live[img];
    if (nl == 0) return;
    const bool had = p.best_len[img] > 0;
    const float had_score = p.best_score[img];
    const long r0 = (long)img * k;
    const int kc = t == 0 ? k : nl;
    int wi[KMAX];
    float wv[KMAX];
    beam_topk_block<KMAX>(x + r0 * ld, ld, t == 0 ? 1 : nl, V, p.cum + r0, kc, wi, wv);
    const int end = p.end_ids ? p.end_ids[img] : p.end_id;
    int src[KMAX], word[KMAX];
    float sc[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { src[j] = 0; word[j] = p.start_id; sc[j] = 0.f; }
    int nn = 0, done_src = -1;
    float best_score = had_score;
    bool has = had;
#pragma unroll
    for (int o = 0; o < KMAX; ++o) {
        const int flat = wi[o] != BEAM_NONE ? wi[o] : 0;
        const int b = flat / V, w = flat - b * V;
        if (o >= kc) {
        } else if (w == end) {
            if (!has || wv[o] > best_score) { has = true; best_score = wv[o]; done_src = b; }
        } else {
#pragma unroll
            for (int j = 0; j < KMAX; ++j) if (j == nn) { src[j] = b; word[j] = w; sc[j] = wv[o]; }
            ++nn;
        }
    }
    __syncthreads();                                   // (every thread has read cum, n_live and the kept score)
    if (const int c = tid; c <= t) {                  // one thread per sequence position: t < LRPX_BEAM_MAX_STEPS = NT
        long long v[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) v[j] = j < k ? p.toks[(r0 + j) * p.tok_ld + c] : 0;
        if (done_src >= 0) p.best[(long)img * p.best_ld + c] = beam_pick(v[0], v[1], v[2], v[3], done_src);
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j < nn) p.toks[(r0 + j) * p.tok_ld + c] = beam_pick(v[0], v[1], v[2], v[3], src[j]);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s >= p.n_state) continue;
        float* st = p.state[s] + (long)(t + 1) * p.state_w;
        for (int c = tid; c < p.state_w; c += NT) {
            float v[KMAX];
#pragma unroll
            for (int j = 0; j < KMAX; ++j) v[j] = j < k ? st[(r0 + j) * p.state_ld + c] : 0.f;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) if (j < nn) st[(r0 + j) * p.state_ld + c] = beam_pick(v[0], v[1], v[2], v[3], src[j]);
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) {
                p.toks[(r0 + j) * p.tok_ld + t + 1] = j < nn ? word[j] : p.start_id;      // rows that are not live carry a valid id
                if (j < nn) p.cum[r0 + j] = sc[j];
            }
        p.n_live[img] = nn;
        if (done_src >= 0) {
            p.best[(long)img * p.best_ld + t + 1] = end;
            p.best_len[img] = t + 2;
            p.best_score[img] = best_score;
        }
        if (nn == 0) atomicSub(p.live_images, 1);
    }
}

// the result of a batched beam search after `steps` steps: out[i] = [length, tokens ...] - the kept complete sequence, or live sequence 0
// cut to 20 tokens (:472)
__global__ __launch_bounds__(256) void beam_result_batch_kernel(const lrpx_beam_batch p, int steps, long long* __restrict__ out, int out_ld) {
    const int img = blockIdx.x;
    const int bl = p.best_len[img];
    const int len = bl > 0 ? bl : min(steps + 1, 20);
    const long long* from = bl > 0 ? p.best + (long)img * p.best_ld : p.toks + (long)img * p.k * p.tok_ld;
    long long* o = out + (long)img * out_ld;
    if (threadIdx.x == 0) o[0] = len;
    for (int c = threadIdx.x; c < len; c += 256) o[1 + c] = from[c];
}

// One step of the reference's diverse beam search (models/gridTDmodel.py:337-381) for N images, one workgroup per image (lrpx_dbs_batch,
// include/lrpx.h).  The image's G groups run in sequence in the launch - group g + 1 needs the outcome of group g twice: the `break`
// (:365-366: a group whose last beam completes ends the step for the later ones) and the penalty set (the distinct input words of groups
// 0 and 1, :377-380).  The first is a register every thread computes alike, the second eight ids in LDS that thread 0 keeps.  A group's
// selection is `beam_topk_block<BeamDiverse>` over its live rows; bookkeeping and the re-order are those of `beam_step_batch_kernel`, on
// the group's own sequence buffer (a group that was passed over is shorter than the step count).  A passed-over group keeps everything;
// its input word and its state move from time t to time t + 1, where the next decoder step reads them.
template <int KMAX>
__global__ __launch_bounds__(1024) void dbs_step_batch_kernel(const lrpx_dbs_batch p, const float* __restrict__ x, long ld, int t) {
    constexpr int NT = 1024;
    static_assert(KMAX == 4, "beam_pick takes four registers");
    const int img = blockIdx.x, tid = threadIdx.x, k = p.k, G = p.G, V = p.V;
    const int end = p.end_ids ? p.end_ids[img] : p.end_id;
    __shared__ int pen_id[8];                             // the penalty set (-1: unused), kept by thread 0 between the groups
    if (tid < 8) pen_id[tid] = -1;
    __syncthreads();
    int n_pen = 0, live_before = 0, live_after = 0;
    bool broken = false;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
        const int grp = img * G + g;
        const long r0 = (long)grp * k;
        const int nl = p.n_live[grp];
        if (nl == 0) continue;                             // :340-341
        ++live_before;
        // a group that is passed over (`broken`) runs the tail below as the identity from time t: the same input words, the same state
        const bool sel = !broken;
        const int sl = p.seq_len[grp];
        int src[KMAX], word[KMAX];
        float sc[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) { src[j] = j; word[j] = p.start_id; sc[j] = 0.f; }
        int nn = k, ns = 0, done_src = -1;
        float best_score = 0.f;
        if (sel) {
            bool has = p.best_len[grp] > 0;
            best_score = p.best_score[grp];
            const int kc = t == 0 ? k : nl;
            int wi[KMAX];
            float wv[KMAX];
            BeamDiverse pen;                               // (read from LDS: eight vector registers, the scalar file is full)
#pragma unroll
            for (int q = 0; q < 8; ++q) pen.id[q] = pen_id[q];
            pen.diversity = p.diversity;
            beam_topk_block<KMAX, BeamDiverse>(x + r0 * ld, ld, t == 0 ? 1 : nl, V, p.cum + r0, kc, wi, wv, pen);
            nn = 0;
#pragma unroll
            for (int o = 0; o < KMAX; ++o) {
                const int flat = wi[o] != BEAM_NONE ? wi[o] : 0;
                const int b = flat / V, w = flat - b * V;
                if (o >= kc) {
                } else if (w == end) {
                    if (!has || wv[o] > best_score) { has = true; best_score = wv[o]; done_src = b; }
                } else {
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) if (j == nn) { src[j] = b; word[j] = w; sc[j] = wv[o]; }
                    ++nn;
                }
            }
            // the last beam completed: `seqs[g]` stays what :357 made it - row 0 is candidate 0 with its <end> (the fallback reads it, :389)
            ns = nn > 0 ? nn : 1;
            if (nn == 0) { const int flat = wi[0] != BEAM_NONE ? wi[0] : 0; src[0] = flat / V; word[0] = flat - src[0] * V; }
            if (g < 2 && nn > 0 && tid == 0) {             // :377-380: the distinct input words of this group join the penalty set
                for (int j = 0; j < nl; ++j) {
                    const int w = (int)p.toks[(r0 + j) * p.tok_ld + t];
                    bool known = false;
                    for (int q = 0; q < n_pen; ++q) known |= pen_id[q] == w;
                    if (!known) pen_id[n_pen++] = w;       // at most 2 groups x 4 live rows
                }
            }
        }
        __syncthreads();                                   // (every thread has read cum, n_live, seq_len, the kept score and the set)
        if (const int c = tid; c < sl && sel) {           // one thread per sequence position: sl <= t + 1 <= LRPX_BEAM_MAX_STEPS = NT
            long long v[KMAX];
#pragma unroll
            for (int j = 0; j < KMAX; ++j) v[j] = j < k ? p.seqs[(r0 + j) * p.seq_ld + c] : 0;
            if (done_src >= 0) p.best[(long)grp * p.best_ld + c] = beam_pick(v[0], v[1], v[2], v[3], done_src);
#pragma unroll
            for (int j = 0; j < KMAX; ++j) if (j < ns) p.seqs[(r0 + j) * p.seq_ld + c] = beam_pick(v[0], v[1], v[2], v[3], src[j]);
        }
        const long from = (long)(sel ? t + 1 : t) * p.state_w, to = (long)(t + 1) * p.state_w;
#pragma unroll 1
        for (int s = 0; s < p.n_state; ++s) {
            float* st = p.state[s];
            for (int c = tid; c < p.state_w; c += NT) {
                float v[KMAX];
#pragma unroll
                for (int j = 0; j < KMAX; ++j) v[j] = j < k ? st[(r0 + j) * p.state_ld + from + c] : 0.f;
#pragma unroll
                for (int j = 0; j < KMAX; ++j) if (j < nn) st[(r0 + j) * p.state_ld + to + c] = beam_pick(v[0], v[1], v[2], v[3], src[j]);
            }
        }
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < k) {
                    long long* tk = p.toks + (r0 + j) * p.tok_ld + t;
                    tk[1] = !sel ? tk[0] : j < nn ? word[j] : p.start_id;                 // rows that are not live carry a valid id
                    if (j < ns) p.seqs[(r0 + j) * p.seq_ld + sl] = word[j];
                    if (sel && j < nn) p.cum[r0 + j] = sc[j];
                }
            if (sel) {
                p.n_live[grp] = nn;
                p.seq_len[grp] = sl + 1;
            }
            if (done_src >= 0) {
                p.best[(long)grp * p.best_ld + sl] = end;
                p.best_len[grp] = sl + 1;
                p.best_score[grp] = best_score;
            }
        }
        if (nn > 0) ++live_after; else broken = true;
    }
    if (tid == 0 && live_before > 0 && live_after == 0) atomicSub(p.live_images, 1);
}

// the result of a batched diverse beam search: out[i G + g] = [length, tokens ...] - the group's kept complete sequence, or sequence row
// 0 of the image's GROUP 0 cut to 20 tokens (:389)
__global__ __launch_bounds__(256) void dbs_result_batch_kernel(const lrpx_dbs_batch p, long long* __restrict__ out, int out_ld) {
    const int grp = blockIdx.x, g0 = grp / p.G * p.G;
    const int bl = p.best_len[grp];
    const int len = bl > 0 ? bl : min(p.seq_len[g0], 20);
    const long long* from = bl > 0 ? p.best + (long)grp * p.best_ld : p.seqs + (long)g0 * p.k * p.seq_ld;
    long long* o = out + (long)grp * out_ld;
    if (threadIdx.x == 0) o[0] = len;
    for (int c = threadIdx.x; c < len; c += 256) o[1 + c] = from[c];
}

// softmax(x[r])[ids[r]] per row (the reference's `torch.softmax(scores, dim=-1)[word]`, evaluation.py:122, :149, :252): one block per row,
// the reduction shape of argmax_logprob_rows_kernel
__global__ __launch_bounds__(256) void softmax_pick_rows_kernel(const float* __restrict__ x, long ld, int n, const long long* __restrict__ ids,
                                                                float* __restrict__ out) {
    __shared__ float red[8];
    const int tid = threadIdx.x;
    const float* r = x + (long)blockIdx.x * ld;
    float m = -INFINITY;
    for (int i = tid; i < n; i += 256) m = fmaxf(m, r[i]);
    m = block_max(m, red);
    float se = 0.f;
    for (int i = tid; i < n; i += 256) se += expf(r[i] - m);
    se = block_sum(se, red);
    if (tid == 0) {
        const long long id = ids[blockIdx.x];
        out[blockIdx.x] = (id >= 0 && id < n) ? expf(r[id] - m) / se : NAN;
    }
}

// word ablation (evaluation.py:242-247): row r holds a caption prefix of t + 1 tokens and the relevance of its words; the kdel most
// relevant of the positions 1 .. t (<start> is never a candidate; ties: lower position) are dropped, the others keep their order.
// One wave per row: kdel rounds of an arg-max over the positions (lane p - 1, p + 63, ...).
__global__ __launch_bounds__(64) void delete_topk_tokens_kernel(const long long* __restrict__ caps, int cap_ld, const float* __restrict__ rw,
                                                                int rw_ld, const int* __restrict__ ts, int kdel,
                                                                long long* __restrict__ out, int out_ld, int* __restrict__ out_len,
                                                                int* __restrict__ deleted) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int t = max(0, min(ts[row], min(cap_ld, min(rw_ld, out_ld)) - 1));      // (a t past a row's end never leaves the row)
    const long long* cp = caps + (long)row * cap_ld;
    const float* rp = rw + (long)row * rw_ld;
    int gone[LRPX_DELETE_MAX];
#pragma unroll
    for (int d = 0; d < LRPX_DELETE_MAX; ++d) gone[d] = -1;
#pragma unroll
    for (int d = 0; d < LRPX_DELETE_MAX; ++d) {
        if (d >= kdel) continue;
        float bv = -INFINITY; int bi = BEAM_NONE;
        for (int pos = 1 + lane; pos <= t; pos += 64) {
            bool taken = false;
#pragma unroll
            for (int e = 0; e < LRPX_DELETE_MAX; ++e) taken = taken || gone[e] == pos;
            const float v = rp[pos];
            if (!taken && (bi == BEAM_NONE || v > bv)) { bv = v; bi = pos; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64); const int oi = __shfl_xor(bi, off, 64);
            const bool take = oi != BEAM_NONE && (bi == BEAM_NONE || ov > bv || (ov == bv && oi < bi));
            bv = take ? ov : bv; bi = take ? oi : bi;
        }
#pragma unroll
        for (int e = 0; e < LRPX_DELETE_MAX; ++e) if (e == d) gone[e] = bi == BEAM_NONE ? -1 : bi;
        if (lane == 0 && deleted) deleted[(long)row * kdel + d] = bi == BEAM_NONE ? -1 : bi;
    }
    int n_gone = 0;
#pragma unroll
    for (int e = 0; e < LRPX_DELETE_MAX; ++e) n_gone += gone[e] >= 0;
    for (int pos = lane; pos <= t; pos += 64) {
        int before = 0; bool taken = false;
#pragma unroll
        for (int e = 0; e < LRPX_DELETE_MAX; ++e) { before += gone[e] >= 0 && gone[e] < pos; taken = taken || gone[e] == pos; }
        if (!taken) out[(long)row * out_ld + pos - before] = cp[pos];
    }
    if (lane == 0) out_len[row] = t + 1 - n_gone;
}


// U[row][c] = r_avg / (P * z~(avg))  — the eye rule of :1121-1124 folded into the projector GEMM's bracket
__global__ void gridtd_rel_u_kernel(const float* __restrict__ r_avg, const float* __restrict__ avg,
                                    float* __restrict__ U, int T, int C, int P) {
    const int row = blockIdx.x, b = row / T;
    for (int c = threadIdx.x; c < C; c += blockDim.x)
        U[(long)row * C + c] = r_avg[(long)row * C + c] / ((float)P * stab_eps(avg[(long)b * C + c]));
}


// :1129-1132  r_words / max|r_words|
__global__ void rel_words_norm_kernel(float* __restrict__ r_words, int rows, int T) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int t = row % T;
    float m = 0.f;
    for (int i = 0; i <= t; ++i) m = fmaxf(m, fabsf(r_words[(long)row * T + i]));
    if (m > 0.f)
        for (int i = 0; i <= t; ++i) r_words[(long)row * T + i] /= m;
}


// Aproj[row][k][c] = sum_{i<=t} alpha[b][i][k] * wacc[row][i][c]   (:1642-1643 summed over i)
__global__ __launch_bounds__(256) void spread_pixels_kernel(const float* __restrict__ wacc, const float* __restrict__ alpha,
                                                            const int* __restrict__ lens, float* __restrict__ Aproj,
                                                            int T, int H, int P, int kchunk,
                                                            const int* __restrict__ rowlist) {
    const int row = rowlist ? rowlist[blockIdx.x] : blockIdx.x, b = row / T, t = row - b * T;
    const long orow = blockIdx.x;
    const int len = lens ? lens[b] : T;
    const int k0 = blockIdx.y * kchunk, k1 = min(k0 + kchunk, P);
    extern __shared__ float al[];
    const int n = t < len ? t + 1 : 0;
    for (int j = threadIdx.x; j < n * kchunk; j += 256) {
        const int i = j / kchunk, kk = j - i * kchunk;
        al[j] = (k0 + kk < P) ? alpha[((long)b * T + i) * P + k0 + kk] : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 256)
        for (int k = k0; k < k1; ++k) {
            float a = 0.f;
            for (int i = n - 1; i >= 0; --i) a += al[i * kchunk + (k - k0)] * wacc[((long)row * T + i) * H + c];
            Aproj[(orow * P + k) * H + c] = a;
        }
}

__global__ void scale_kernel(const float* __restrict__ x, float* __restrict__ y, long n, float alpha) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = x[i] * alpha;
}

__global__ void positive_mask_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = x[i] > 0.f ? 1.f : 0.f;
}


__global__ void keep_cols_kernel(float* __restrict__ x, int ncol, int lo, int hi, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = idx % ncol;
    if (c < lo || c >= hi) x[idx] = 0.f;
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

int lrpx_linear_small(const float* x, long ldx, const float* w, const float* bias, float* out, long ldo, int B, int K,
                      int N, int act, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_linear_small", {x, "x"}, {w, "w"}, {bias, "bias"}, {out, "out"});
    LRPX_REQUIRE(x && w && out && B > 0 && N > 0 && K > 0 && K % 4 == 0 && ldx % 4 == 0, "linear_small: bad arguments");
    if (K % 16 == 0 && B <= 64) {
        const dim3 grid((N + 15) / 16);
        hipStream_t st = (hipStream_t)stream;
        with_row_tiles(B, [&](auto rt) { hipLaunchKernelGGL((linear_mfma_kernel<decltype(rt)::value>), grid, dim3(256), 0, st, x, ldx, w, bias, out, ldo, B, K, N, act); });
        return check_launch("linear_small");
    }
    hipLaunchKernelGGL((linear_small_kernel<4, 16>), dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, w,
                       bias, out, ldo, B, K, N, act);
    return check_launch("linear_small");
}

int lrpx_mean_pixels(const float* f, float* avg, int B, int P, int C, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_mean_pixels", {f, "f"}, {avg, "avg"});
    LRPX_REQUIRE(f && avg && B > 0, "mean_pixels: bad arguments");
    hipLaunchKernelGGL(mean_pixels_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, f, avg, P, C,
                       1.0f / (float)P);
    return check_launch("mean_pixels");
}

int lrpx_relu(const float* x, float* y, long n, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_relu", {x, "x"}, {y, "y"});
    LRPX_REQUIRE(x && y && n > 0, "relu: bad arguments");
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    return check_launch("relu");
}

int lrpx_argmax_rows(const float* x, long ld, int rows, int n, long long* out, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_argmax_rows", {x, "x"}, {out, "out"});
    LRPX_REQUIRE(x && out && rows > 0 && n > 0, "argmax_rows: bad arguments");
    hipLaunchKernelGGL(argmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, ld, n, out);
    return check_launch("argmax_rows");
}

int lrpx_lrp_reweight_rows(const float* pred, long ld, int V, const float* h, long ldh, const float* ctx, long ldc,
                           const float* fc_w, const unsigned char* skip, float* hcw, int rows, int H, int log_softmax,
                           void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_lrp_reweight_rows", {pred, "pred"}, {h, "h"}, {ctx, "ctx"}, {fc_w, "fc_w"}, {skip, "skip"}, {hcw, "hcw"});
    LRPX_REQUIRE(pred && h && ctx && fc_w && skip && hcw && rows > 0 && V > 0 && ld >= V && H == 512 && ldh >= H &&
                     ldc >= H, "lrp_reweight_rows: bad arguments (H must be 512)");
    hipLaunchKernelGGL(lrp_reweight_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, pred, ld, V, h, ldh, ctx, ldc,
                       fc_w, skip, hcw, H, log_softmax ? 1 : 0);
    return check_launch("lrp_reweight_rows");
}

int lrpx_argmax_logprob_rows(const float* x, long ld, int rows, int n, long long* out, float* logprob, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_argmax_logprob_rows", {x, "x"}, {out, "out"}, {logprob, "logprob"});
    LRPX_REQUIRE(x && out && logprob && rows > 0 && n > 0, "argmax_logprob_rows: bad arguments");
    hipLaunchKernelGGL(argmax_logprob_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, ld, n, out,
                       logprob);
    return check_launch("argmax_logprob_rows");
}

int lrpx_beam_topk(const float* x, long ld, int n_rows, int n, const float* cum, int k, long long* out_idx, float* out_val,
                   void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_beam_topk", {x, "x"}, {cum, "cum"}, {out_idx, "out_idx"}, {out_val, "out_val"});
    LRPX_REQUIRE(x && out_idx && out_val && n_rows > 0 && n_rows <= 8 && n > 0 && k > 0 && k <= 4 && (long)n_rows * n < 0x7fffffffL,
                 "beam_topk: bad arguments (at most 8 live beams, k <= 4)");
    hipLaunchKernelGGL((beam_topk_kernel<4>), dim3(1), dim3(1024), 0, (hipStream_t)stream, x, ld, n_rows, n, cum, k, out_idx,
                       out_val);
    return check_launch("beam_topk");
}

int lrpx_beam_step_batch(const lrpx_beam_batch* p, const float* x, long ld, int t, void* stream) {
    LRPX_REQUIRE(p, "beam_step_batch: null state");
    LRPX_REQUIRE(p->k >= 1 && p->k <= 4 && p->N >= 1 && p->V >= 1 && (long)p->k * p->V < 0x7fffffffL,
                 "beam_step_batch: bad arguments (beam size 1..4, N >= 1, V >= 1; got k = %d, N = %d, V = %d)", p->k, p->N, p->V);
    LRPX_REQUIRE(p->T >= 1 && p->T <= LRPX_BEAM_MAX_STEPS, "beam_step_batch: max_cap_length %d outside 1..%d (one thread per sequence position)",
                 p->T, LRPX_BEAM_MAX_STEPS);
    LRPX_REQUIRE(t >= 0 && t < p->T && p->tok_ld > p->T && p->best_ld > p->T && ld >= p->V, "beam_step_batch: step %d of %d, or a row stride shorter than its rows", t, p->T);
    LRPX_REQUIRE(x && p->toks && p->cum && p->n_live && p->best && p->best_len && p->best_score && p->live_images, "beam_step_batch: null pointer");
    LRPX_REQUIRE(p->n_state >= 0 && p->n_state <= 4 && (p->n_state == 0 || (p->state_w >= 1 && p->state_ld >= (long)(p->T + 1) * p->state_w)),
                 "beam_step_batch: at most 4 state tensors (rows, T + 1, width)");
    for (int s = 0; s < p->n_state; ++s) LRPX_REQUIRE(p->state[s], "beam_step_batch: null state tensor %d", s);
#define LRPX_BEAM_PTRS {x, "x"}, {p->end_ids, "end_ids"}, {p->toks, "toks"}, {p->cum, "cum"}, {p->n_live, "n_live"}, {p->best, "best"},         \
                       {p->best_len, "best_len"}, {p->best_score, "best_score"}, {p->live_images, "live_images"}, {p->n_state > 0 ? p->state[0] : nullptr, "state[0]"},    \
                       {p->n_state > 1 ? p->state[1] : nullptr, "state[1]"}, {p->n_state > 2 ? p->state[2] : nullptr, "state[2]"},               \
                       {p->n_state > 3 ? p->state[3] : nullptr, "state[3]"}
    if (t == 0) {      // the first step of a search looks at every pointer; the later ones only under LRPX_CHECK_PTRS=1, like their neighbours
        LRPX_CHECK_PTRS("lrpx_beam_step_batch", LRPX_BEAM_PTRS);
    } else {
        LRPX_CHECK_PTRS_OPT("lrpx_beam_step_batch", LRPX_BEAM_PTRS);
    }
#undef LRPX_BEAM_PTRS
    hipLaunchKernelGGL((beam_step_batch_kernel<4>), dim3(p->N), dim3(1024), 0, (hipStream_t)stream, *p, x, ld, t);
    return check_launch("beam_step_batch");
}

int lrpx_beam_result_batch(const lrpx_beam_batch* p, int steps, long long* out, int out_ld, void* stream) {
    LRPX_REQUIRE(p && out, "beam_result_batch: null pointer");
    LRPX_CHECK_PTRS("lrpx_beam_result_batch", {out, "out"}, {p->toks, "toks"}, {p->best, "best"}, {p->best_len, "best_len"});
    LRPX_REQUIRE(p->k >= 1 && p->k <= 4 && p->N >= 1 && p->T >= 1 && p->T <= LRPX_BEAM_MAX_STEPS && steps >= 1 && steps <= p->T &&
                     p->tok_ld > p->T && p->best_ld > p->T && out_ld >= p->T + 2 && p->toks && p->best && p->best_len,
                 "beam_result_batch: bad arguments (out rows hold the length and T + 1 tokens)");
    hipLaunchKernelGGL(beam_result_batch_kernel, dim3(p->N), dim3(256), 0, (hipStream_t)stream, *p, steps, out, out_ld);
    return check_launch("beam_result_batch");
}

// the shape of a diverse beam search's state: G = k groups of k beams, at most 16 rows per image, one thread per sequence position
static int dbs_check_shape(const lrpx_dbs_batch* p, const char* who) {
    LRPX_REQUIRE(p, "%s: null state", who);
    LRPX_REQUIRE(p->k >= 1 && p->k <= 4 && p->G == p->k && p->N >= 1 && p->V >= 1 && (long)p->k * p->V < 0x7fffffffL &&
                     (long)p->N * p->G * p->k < 0x7fffffffL,
                 "%s: bad arguments (beam size 1..4, as many groups as beams, N >= 1, V >= 1; got k = %d, G = %d, N = %d, V = %d)", who,
                 p->k, p->G, p->N, p->V);
    LRPX_REQUIRE(p->T >= 1 && p->T <= LRPX_BEAM_MAX_STEPS, "%s: max_cap_length %d outside 1..%d (one thread per sequence position)", who,
                 p->T, LRPX_BEAM_MAX_STEPS);
    LRPX_REQUIRE(p->tok_ld > p->T && p->seq_ld > p->T && p->best_ld > p->T, "%s: a row stride shorter than T + 1 = %d", who, p->T + 1);
    LRPX_REQUIRE(p->toks && p->seqs && p->cum && p->n_live && p->seq_len && p->best && p->best_len && p->best_score && p->live_images,
                 "%s: null pointer", who);
    return LRPX_OK;
}

int lrpx_dbs_step_batch(const lrpx_dbs_batch* p, const float* x, long ld, int t, void* stream) {
    if (const int rc = dbs_check_shape(p, "dbs_step_batch")) return rc;
    LRPX_REQUIRE(x && t >= 0 && t < p->T && ld >= p->V, "dbs_step_batch: null scores, step %d of %d, or a row stride shorter than V", t, p->T);
    LRPX_REQUIRE(p->diversity == p->diversity, "dbs_step_batch: diversity is NaN");
    LRPX_REQUIRE(p->n_state >= 0 && p->n_state <= 4 && (p->n_state == 0 || (p->state_w >= 1 && p->state_ld >= (long)(p->T + 1) * p->state_w)),
                 "dbs_step_batch: at most 4 state tensors (rows, T + 1, width)");
    for (int s = 0; s < p->n_state; ++s) LRPX_REQUIRE(p->state[s], "dbs_step_batch: null state tensor %d", s);
#define LRPX_DBS_PTRS {x, "x"}, {p->end_ids, "end_ids"}, {p->toks, "toks"}, {p->seqs, "seqs"}, {p->cum, "cum"}, {p->n_live, "n_live"},          \
                      {p->seq_len, "seq_len"}, {p->best, "best"}, {p->best_len, "best_len"}, {p->best_score, "best_score"},                     \
                      {p->live_images, "live_images"}, {p->n_state > 0 ? p->state[0] : nullptr, "state[0]"},                                    \
                      {p->n_state > 1 ? p->state[1] : nullptr, "state[1]"}, {p->n_state > 2 ? p->state[2] : nullptr, "state[2]"},               \
                      {p->n_state > 3 ? p->state[3] : nullptr, "state[3]"}
    if (t == 0) {      // the first step of a search looks at every pointer; the later ones only under LRPX_CHECK_PTRS=1, like their neighbours
        LRPX_CHECK_PTRS("lrpx_dbs_step_batch", LRPX_DBS_PTRS);
    } else {
        LRPX_CHECK_PTRS_OPT("lrpx_dbs_step_batch", LRPX_DBS_PTRS);
    }
#undef LRPX_DBS_PTRS
    hipLaunchKernelGGL((dbs_step_batch_kernel<4>), dim3(p->N), dim3(1024), 0, (hipStream_t)stream, *p, x, ld, t);
    return check_launch("dbs_step_batch");
}

int lrpx_dbs_result_batch(const lrpx_dbs_batch* p, long long* out, int out_ld, void* stream) {
    if (const int rc = dbs_check_shape(p, "dbs_result_batch")) return rc;
    LRPX_REQUIRE(out && out_ld >= p->T + 2, "dbs_result_batch: out rows hold the length and T + 1 tokens");
    LRPX_CHECK_PTRS("lrpx_dbs_result_batch", {out, "out"}, {p->seqs, "seqs"}, {p->seq_len, "seq_len"}, {p->best, "best"},
                    {p->best_len, "best_len"});
    hipLaunchKernelGGL(dbs_result_batch_kernel, dim3(p->N * p->G), dim3(256), 0, (hipStream_t)stream, *p, out, out_ld);
    return check_launch("dbs_result_batch");
}

int lrpx_softmax_pick_rows(const float* x, long ld, int rows, int n, const long long* ids, float* out, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_softmax_pick_rows", {x, "x"}, {ids, "ids"}, {out, "out"});
    LRPX_REQUIRE(x && ids && out && rows > 0 && n > 0 && ld >= n, "softmax_pick_rows: bad arguments");
    hipLaunchKernelGGL(softmax_pick_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, ld, n, ids, out);
    return check_launch("softmax_pick_rows");
}

int lrpx_delete_topk_tokens(const long long* caps, int cap_ld, const float* r_words, int rw_ld, const int32_t* t, int rows, int kdel,
                            long long* out, int out_ld, int32_t* out_len, int32_t* deleted, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_delete_topk_tokens", {caps, "caps"}, {r_words, "r_words"}, {t, "t"}, {out, "out"}, {out_len, "out_len"},
                        {deleted, "deleted"});
    LRPX_REQUIRE(caps && r_words && t && out && out_len && rows > 0 && kdel >= 0 && kdel <= LRPX_DELETE_MAX && cap_ld >= 1 && rw_ld >= 1 &&
                     out_ld >= 1, "delete_topk_tokens: bad arguments (at most %d deletions)", LRPX_DELETE_MAX);
    hipLaunchKernelGGL(delete_topk_tokens_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, caps, cap_ld, r_words, rw_ld, t, kdel, out,
                       out_ld, out_len, deleted);
    return check_launch("delete_topk_tokens");
}

int lrpx_target_logit(const float* hc, const float* fcw, const float* fcb, const long long* tok, int tok_ld,
                      float* logit, int B, int T, int H, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_target_logit", {hc, "hc"}, {fcw, "fcw"}, {fcb, "fcb"}, {tok, "tok"}, {logit, "logit"});
    LRPX_REQUIRE(hc && fcw && fcb && tok && logit, "target_logit: null pointer");
    hipLaunchKernelGGL(target_logit_kernel, dim3((B * T + 3) / 4), dim3(256), 0, (hipStream_t)stream, hc, fcw, fcb, tok,
                       tok_ld, logit, B, T, H);
    return check_launch("target_logit");
}

int lrpx_rel_avg_u(const float* r_avg, const float* avg, float* u, int rows, int T, int C, int P, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_rel_avg_u", {r_avg, "r_avg"}, {avg, "avg"}, {u, "u"});
    LRPX_REQUIRE(r_avg && avg && u && rows > 0, "rel_avg_u: bad arguments");
    hipLaunchKernelGGL(gridtd_rel_u_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, r_avg, avg, u, T, C, P);
    return check_launch("rel_avg_u");
}

int lrpx_rel_words_norm(float* r_words, int rows, int T, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_rel_words_norm", {r_words, "r_words"});
    LRPX_REQUIRE(r_words && rows > 0 && T > 0, "rel_words_norm: bad arguments");
    hipLaunchKernelGGL(rel_words_norm_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, r_words, rows, T);
    return check_launch("rel_words_norm");
}

int lrpx_spread_pixels_rows(const float* wacc, const float* alpha, const int32_t* lens, float* a_proj, int B, int T, int H,
                            int P, const int32_t* rows, int n_rows, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_spread_pixels_rows", {wacc, "wacc"}, {alpha, "alpha"}, {lens, "lens"}, {a_proj, "a_proj"}, {rows, "rows"});
    LRPX_REQUIRE(wacc && alpha && a_proj && B > 0 && T > 0, "spread_pixels: bad arguments");
    LRPX_REQUIRE(rows ? (n_rows > 0 && n_rows <= B * T) : n_rows == B * T, "spread_pixels: bad row list");
    const int kchunk = 28;
    hipLaunchKernelGGL(spread_pixels_kernel, dim3(n_rows, (P + kchunk - 1) / kchunk), dim3(256),
                       (size_t)T * kchunk * sizeof(float), (hipStream_t)stream, wacc, alpha, lens, a_proj, T, H, P, kchunk, rows);
    return check_launch("spread_pixels");
}

int lrpx_spread_pixels(const float* wacc, const float* alpha, const int32_t* lens, float* a_proj, int B, int T, int H,
                       int P, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_spread_pixels", {wacc, "wacc"}, {alpha, "alpha"}, {lens, "lens"}, {a_proj, "a_proj"});
    return lrpx_spread_pixels_rows(wacc, alpha, lens, a_proj, B, T, H, P, nullptr, B * T, stream);
}

int lrpx_scale(const float* x, float* y, long n, float alpha, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_scale", {x, "x"}, {y, "y"});
    LRPX_REQUIRE(x && y && n > 0, "scale: bad arguments");
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n, alpha);
    return check_launch("scale");
}

int lrpx_positive_mask(const float* x, float* y, long n, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_positive_mask", {x, "x"}, {y, "y"});
    LRPX_REQUIRE(x && y && n > 0, "positive_mask: bad arguments");
    hipLaunchKernelGGL(positive_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    return check_launch("positive_mask");
}

int lrpx_keep_cols(float* x, long rows, int ncol, int lo, int hi, void* stream) {
    LRPX_CHECK_PTRS_OPT("lrpx_keep_cols", {x, "x"});
    LRPX_REQUIRE(x && rows > 0 && ncol > 0 && lo >= 0 && hi <= ncol && lo < hi, "keep_cols: bad arguments");
    const long total = rows * ncol;
    hipLaunchKernelGGL(keep_cols_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ncol,
                       lo, hi, total);
    return check_launch("keep_cols");
}

}  // extern "C"
