// The one kernel of the runtime-geometry contraction engine (conv_geom.h) and its launch.  Classes, taps, staging, gather, stage loop and
// epilogue are written here once; the arithmetic - fp32 MFMA (CgF32, conv_geom.hip) or the exact bf16 split (CgB6, conv_geom_b6.hip) - is
// a policy that holds
//   ROWB            bytes per pixel row of the LDS A tile
//   BFrag, NB       a lane's 16 bytes of a packed B fragment and the fragments per stage: a (column block, tap, chunk) of the packed
//                   weights is NB contiguous 1 KiB fragments of 64 lanes x 16 bytes
//   store_a         the gathered float4 of channels c4 .. c4 + 3 of the chunk into the pixel's LDS row
//   mma             the MFMAs of one stage from the A rows at `ap` (this lane's row + 16 (lane >> 5) bytes) and the stage's B fragments
// The transposed direction takes the operands of a BATCHED relevance pass, each optional:
//   map2img   the relevance operand and the output are per MAP, x and q per IMAGE map2img[m]  (NULL: map m on image m)
//   q         per-image multiplier of the relevance operand, applied while the A tile is gathered: S = R * q[img] never exists
//   addend    out = x * acc + addend  (the two relevances that meet at a block's input)
// The general alpha-beta rule (AB) is the same transposed kernel with a DUAL-coefficient A gather: the contraction runs
// over the stacked index kappa in [0, 2 kr) against the weight rows [W+ ; W-] (packed as one tensor of 2 kr rows), and the operand is
// A(kappa) = (R[c] * qh[c]) * sh with c = kappa mod kr and (qh, sh) = (q, scale) below kr, (q2, scale2) from kr on.  kr % 4 == 0, so a
// thread's float4 never straddles the halves, wherever the boundary falls in a chunk.
// The gradient chain (AB = 3) is the transposed kernel with the raw weights and an operand shaped while it is gathered:
// A = scale[c] * (mask[img] > 0 ? (clamp ? max(in, 0) : in) : 0), each of the three optional, and the epilogue out = acc + addend: no
// multiplicand, p.x is never read.
// The blocked forward (BLOCKED, forward direction only): the sums of the plain forward in a blocked order.  Z+ is a sum of
// terms of one sign, so every add into the running sum rounds at the sum's full size; the policy's cross products collect in an
// accumulator of their own and the main one is flushed into a second level every CG_FLUSH stages, which leaves (stages / CG_FLUSH) + 2
// CG_FLUSH roundings of full size per output where the plain forward has 12 per stage.
// POOL (the dual-coefficient gather only): the conv sits directly under a 2x2 / stride-2 max-pool and `in` is the relevance
// BEHIND that pool, (n maps, (OH / 2) (OW / 2), kr): the staged element reads it at (sy >> 1, sx >> 1), inside the pooled map's bounds, and
// q / q2 - which carry the pool's winner factor - at (sy, sx).  The relevance at the conv's own resolution never exists.
#pragma once
#include "conv_geom.h"

namespace lrpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct CgParams {
    const float* in;
    const char* wp;
    const float* bias;
    const float* x;
    const float* q;
    const float* addend;
    const int32_t* map2img;
    float* out;
    int n, H, W, OH, OW, kh, kw, sh, sw, ph, pw, K, n_oc, nchunk, taps;
    // AB only: row length of in / q / q2 (K = kr or 2 kr), the second half's coefficient and the two scalars
    int kr;
    const float* q2;
    float scale, scale2;
    // AB = 3 only: per-image ReLU mask (indexed like q), per-channel factor (K floats), clamp the operand at 0 first
    const float* mask;
    const float* chscale;
    int clamp;
};

// The second level of the blocked forward: present in the BLOCKED instantiation alone, an empty object in every other
template <bool ON>
struct CgSecondLevel {
    f32x16 hi;
    __device__ __forceinline__ CgSecondLevel() {
#pragma unroll
        for (int e = 0; e < 16; ++e) hi[e] = 0.f;
    }
    __device__ __forceinline__ void flush(f32x16& acc) {
        hi = hi + acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    }
    __device__ __forceinline__ void join(f32x16& acc, const f32x16& lo) const { acc = hi + (acc + lo); }
};
template <>
struct CgSecondLevel<false> {};

// DIR = LRPX_GEOM_FWD: output pixels are the (OH, OW) map, sources the (H, W) map.
// DIR = LRPX_GEOM_BWD: output pixels are the (H, W) map in sub-pixel classes (blockIdx.z), sources the (OH, OW) map.
// AB (transposed direction only) 1: the dual-coefficient gather;  2: the same, with the policy's cross products in an accumulator of their
// own (CgB6 over both halves, K = 2 kr);  3: the gradient chain's gather and epilogue.  POOL, BLOCKED: above.
template <typename Arith, int DIR, int AB, bool POOL = false, bool BLOCKED = false>
__global__ __launch_bounds__(256) void conv_geom_kernel(const CgParams p) {
    static_assert(!POOL || (DIR == LRPX_GEOM_BWD && (AB == 1 || AB == 2)), "the pooled operand belongs to the dual-coefficient gather");
    typedef typename Arith::BFrag BFrag;
    constexpr int NB = Arith::NB;
    constexpr bool DUAL = AB == 1 || AB == 2, GRAD = AB == 3;
    constexpr int CG_FLUSH = 8;                     // BLOCKED: stages per block of the main accumulator
    static_assert(!BLOCKED || (DIR == LRPX_GEOM_FWD && AB == 0), "the blocked order belongs to the forward direction");
    __shared__ __attribute__((aligned(16))) char a_lds[CG_TM * Arith::ROWB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;

    // the class of this workgroup: output rows ch, ch + cs_h, ..., columns cw, cw + cs_w, ...
    const int ch = DIR == LRPX_GEOM_BWD ? (int)blockIdx.z / p.sw : 0, cw = DIR == LRPX_GEOM_BWD ? (int)blockIdx.z % p.sw : 0;
    const int cs_h = DIR == LRPX_GEOM_BWD ? p.sh : 1, cs_w = DIR == LRPX_GEOM_BWD ? p.sw : 1;
    const int OY = DIR == LRPX_GEOM_BWD ? p.H : p.OH, OX = DIR == LRPX_GEOM_BWD ? p.W : p.OW;     // output map
    const int SY = DIR == LRPX_GEOM_BWD ? p.OH : p.H, SX = DIR == LRPX_GEOM_BWD ? p.OW : p.W;     // source map
    // POOL: the map `in` is stored at, and the part of the source map its windows cover - a last odd row / column lies under no window,
    // its operand is zero (the winner factor in q / q2 is) and nothing of it is read
    const int PY = SY >> 1, PX = SX >> 1;
    const int SYg = POOL ? SY & ~1 : SY, SXg = POOL ? SX & ~1 : SX;
    const int Hc = ch < OY ? (OY - ch + cs_h - 1) / cs_h : 0, Wc = cw < OX ? (OX - cw + cs_w - 1) / cs_w : 0;
    const long npix = (long)p.n * Hc * Wc;
    const long pix0 = (long)blockIdx.x * CG_TM;
    if (pix0 >= npix) return;                      // the grid is sized for the largest class

    // the taps that reach this class: r = r0 + i * rstep < kh, s = s0 + j * sstep < kw
    int r0 = 0, s0 = 0, nr = p.kh, ns = p.kw, yb = 0, xb = 0;
    if (DIR == LRPX_GEOM_BWD) {
        r0 = (ch + p.ph) % p.sh;
        s0 = (cw + p.pw) % p.sw;
        nr = r0 < p.kh ? (p.kh - r0 + p.sh - 1) / p.sh : 0;
        ns = s0 < p.kw ? (p.kw - s0 + p.sw - 1) / p.sw : 0;
        yb = (ch + p.ph) / p.sh;                   // source row of tap r0 for class row 0: oh = hi + yb - i
        xb = (cw + p.pw) / p.sw;
    }
    const int nst = nr * ns * p.nchunk;            // 0: no tap reaches the class, its pixels are x * 0 + addend

    // staging: thread -> pixel rows (tid >> 3) and (tid >> 3) + 32 of the tile, channels 4 (tid & 7) .. + 3 of the chunk
    const int c4 = 4 * (tid & 7);
    int pn[2], pim[2], phi[2], pwi[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long q = pix0 + (tid >> 3) + 32 * i;
        if (q < npix) {
            const long m = q / ((long)Hc * Wc);
            const int rem = (int)(q - m * Hc * Wc);
            pn[i] = (int)m;
            pim[i] = (DIR == LRPX_GEOM_BWD && p.map2img) ? p.map2img[m] : (int)m;
            phi[i] = rem / Wc;
            pwi[i] = rem - phi[i] * Wc;
        } else {
            pn[i] = -1;
            pim[i] = phi[i] = pwi[i] = 0;
        }
    }
    const int ocb = blockIdx.y * 2 + wn;
    const bool active = ocb * 32 < p.n_oc;          // a wave whose 32 columns lie beyond n_oc only helps staging

    f32x4 ra[2];
    BFrag bcur[NB], bnext[NB];
    f32x16 acc, acc_lo;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = acc_lo[e] = 0.f;
    f32x16& lo = AB == 2 || BLOCKED ? acc_lo : acc;  // where the policy's cross products collect (CgB6)
    CgSecondLevel<BLOCKED> second;
#pragma unroll
    for (int g = 0; g < NB; ++g) bcur[g] = bnext[g] = BFrag{0, 0, 0, 0};

    auto load_stage = [&](int st, BFrag* b) {
        const int t = st / p.nchunk, chunk = st - t * p.nchunk;
        const int i = t / ns, j = t - i * ns;
        const int kc = chunk * CG_KC + c4;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int sy = DIR == LRPX_GEOM_BWD ? phi[u] + yb - i : phi[u] * p.sh - p.ph + i;
            const int sx = DIR == LRPX_GEOM_BWD ? pwi[u] + xb - j : pwi[u] * p.sw - p.pw + j;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (pn[u] >= 0 && sy >= 0 && sy < SYg && sx >= 0 && sx < SXg && kc < p.K) {
                const long pix = (long)sy * SX + sx;
                const bool neg = DUAL && kc >= p.kr;                 // the W- half of the stacked contraction
                const int c = neg ? kc - p.kr : kc, ld = DUAL ? p.kr : p.K;
                if (!POOL)
                    v = *reinterpret_cast<const f32x4*>(p.in + ((long)pn[u] * SY * SX + pix) * ld + c);
                else        // sy < SY & ~1 and sx < SX & ~1 here: (sy >> 1, sx >> 1) lies inside the pooled map
                    v = *reinterpret_cast<const f32x4*>(p.in + ((long)pn[u] * PY * PX + (long)(sy >> 1) * PX + (sx >> 1)) * ld + c);
                if (DIR == LRPX_GEOM_BWD && !GRAD && p.q) {
                    const f32x4 qv = *reinterpret_cast<const f32x4*>((neg ? p.q2 : p.q) + ((long)pim[u] * SY * SX + pix) * ld + c);
                    v = v * qv;
                }
                if (DUAL) v = v * (neg ? p.scale2 : p.scale);      // (R q) s in this order: s = 1 leaves the preset's operand
                if (GRAD) {                                        // clamp, mask, scale in this order, all in fp32
                    if (p.clamp)
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    if (p.mask) {
                        const f32x4 mv = *reinterpret_cast<const f32x4*>(p.mask + ((long)pim[u] * SY * SX + pix) * ld + c);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = mv[e] <= 0.f ? 0.f : v[e];
                    }
                    if (p.chscale) v = v * *reinterpret_cast<const f32x4*>(p.chscale + c);
                }
            }
            ra[u] = v;
        }
        if (active) {
            const int r = DIR == LRPX_GEOM_BWD ? r0 + i * p.sh : i, s = DIR == LRPX_GEOM_BWD ? s0 + j * p.sw : j;
            const char* bp = p.wp + (((long)ocb * p.taps + (r * p.kw + s)) * p.nchunk + chunk) * (NB * 1024) + lane * 16;
#pragma unroll
            for (int g = 0; g < NB; ++g) b[g] = *reinterpret_cast<const BFrag*>(bp + g * 1024);
        }
    };

    if (nst > 0) load_stage(0, bcur);
    for (int st = 0; st < nst; ++st) {
        __syncthreads();                            // the previous stage's fragments have been read
#pragma unroll
        for (int u = 0; u < 2; ++u) Arith::store_a(a_lds + ((tid >> 3) + 32 * u) * Arith::ROWB, c4, ra[u]);
        __syncthreads();
        if (st + 1 < nst) load_stage(st + 1, bnext);   // in flight under this stage's MFMAs
        if (active) Arith::mma(a_lds + (wm * 32 + (lane & 31)) * Arith::ROWB + 16 * (lane >> 5), bcur, acc, lo);
#pragma unroll
        for (int g = 0; g < NB; ++g) bcur[g] = bnext[g];
        if constexpr (BLOCKED)
            if (st % CG_FLUSH == CG_FLUSH - 1) second.flush(acc);
    }

    if (AB == 2) acc = acc + acc_lo;
    if constexpr (BLOCKED) second.join(acc, acc_lo);
    // epilogue: accumulator register e of lane l is tile row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
    const int oc = ocb * 32 + (lane & 31);
    if (oc >= p.n_oc) return;
    const float bias = (DIR == LRPX_GEOM_FWD && p.bias) ? p.bias[oc] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const long q = pix0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (q >= npix) continue;
        const long m = q / ((long)Hc * Wc);
        const int rem = (int)(q - m * Hc * Wc);
        const int hi = rem / Wc, wi = rem - hi * Wc;
        const long pix = (long)(ch + hi * cs_h) * OX + (cw + wi * cs_w);
        const long off = (m * OY * OX + pix) * p.n_oc + oc;
        if (DIR == LRPX_GEOM_FWD) {
            p.out[off] = acc[e] + bias;
        } else if (GRAD) {
            float v = nst > 0 ? acc[e] : 0.f;
            if (p.addend) v += p.addend[off];
            p.out[off] = v;
        } else {
            const long img = p.map2img ? p.map2img[m] : m;
            float v = nst > 0 ? acc[e] * p.x[(img * OY * OX + pix) * p.n_oc + oc] : 0.f;
            if (p.addend) v += p.addend[off];
            p.out[off] = v;
        }
    }
}

// Check the descriptor (`ab`: the dual-coefficient entries, d = &ab->base; `gr`: the gradient entries, d = &gr->base, AB = 3) and launch its direction: conv_geom_kernel<Arith, FWD, 0> on
// ceil(output pixels / CG_TM) tiles, or <Arith, BWD, AB, POOL> on the tiles of the largest class, (0, 0), for each of the sh * sw classes.
template <typename Arith, int AB, bool POOL = false, bool BLOCKED = false>
int conv_geom_run(const lrpx_conv_geom_ex_desc* d, const lrpx_conv_geom_ab_desc* ab, void* stream, const char* fn,
                  const lrpx_conv_geom_grad_desc* gr = nullptr) {
    LRPX_TRY(conv_geom_check(d, fn, ab, gr));
    const CgParams p = {d->in, (const char*)d->wpacked, d->bias, d->x, d->q, d->addend, d->map2img, d->out, d->n, d->h, d->w, d->oh, d->ow,
                        d->kh, d->kw, d->sh, d->sw, d->ph, d->pw, d->k, d->n_oc, (int)ceil_div(d->k, CG_KC), d->kh * d->kw,
                        ab ? ab->kr : 0, ab ? ab->q2 : nullptr, ab ? ab->scale : 0.f, ab ? ab->scale2 : 0.f,
                        gr ? gr->mask : nullptr, gr ? gr->scale : nullptr, gr ? gr->clamp : 0};
    const unsigned gy = (unsigned)ceil_div(d->n_oc, CG_TN);
    if (d->dir == LRPX_GEOM_FWD) {
        const long pix_out = (long)d->n * d->oh * d->ow;
        hipLaunchKernelGGL((conv_geom_kernel<Arith, LRPX_GEOM_FWD, 0, false, BLOCKED>), dim3((unsigned)ceil_div(pix_out, CG_TM), gy, 1), dim3(256), 0,
                           (hipStream_t)stream, p);
    } else {
        const long pc = (long)d->n * ceil_div(d->h, d->sh) * ceil_div(d->w, d->sw);
        hipLaunchKernelGGL((conv_geom_kernel<Arith, LRPX_GEOM_BWD, AB, POOL>), dim3((unsigned)ceil_div(pc, CG_TM), gy, (unsigned)(d->sh * d->sw)),
                           dim3(256), 0, (hipStream_t)stream, p);
    }
    return check_launch(fn);
}

}  // namespace lrpx
