// The runtime-geometry contraction engine (conv_geom.h) with the operands of a BATCHED relevance pass: lrpx_conv_geom_ex.
// Same tiling, packed weights and arithmetic as lrpx_conv_geom (conv_geom.hip: fp32 operands, fp32 accumulation on
// v_mfma_f32_32x32x2_f32, one fmaf chain per output over (tap, channel)); the transposed direction additionally takes
//   map2img   the relevance operand and the output are per MAP, x and q per IMAGE map2img[m]  (NULL: map m on image m)
//   q         per-image multiplier of the relevance operand, applied while the A tile is gathered: S = R * q[img] never exists
//   addend    out = x * acc + addend  (the two relevances that meet at a block's input)
// The forward direction is the plain convolution; the trace stacks [W | W+] along the output columns to get the conv's output
// and Z+ from one gather of the A tile.
// The general alpha-beta rule (lrpx_conv_geom_ab) is the same transposed kernel with a DUAL-coefficient A gather:
// the contraction runs over the stacked index kappa in [0, 2 kr) against the weight rows [W+ ; W-] (packed by lrpx_conv_geom_pack as
// one tensor of 2 kr rows), and the operand is A(kappa) = (R[c] * qh[c]) * sh with c = kappa mod kr and (qh, sh) = (q, scale) below kr,
// (q2, scale2) from kr on.  kr % 4 == 0, so a thread's float4 never straddles the halves, wherever the boundary falls in a chunk.
#include "conv_geom.h"

namespace lrpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct CgxParams {
    const float* in;
    const float* wp;
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
};

// DIR = LRPX_GEOM_FWD: output pixels are the (OH, OW) map, sources the (H, W) map.
// DIR = LRPX_GEOM_BWD: output pixels are the (H, W) map in sub-pixel classes (blockIdx.z), sources the (OH, OW) map.
// AB (transposed direction only): the dual-coefficient gather described at the top of the file.
template <int DIR, bool AB = false>
__global__ __launch_bounds__(256) void conv_geom_ex_kernel(const CgxParams p) {
    __shared__ __attribute__((aligned(16))) float a_lds[CG_TM * CG_LDA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;

    const int ch = DIR == LRPX_GEOM_BWD ? (int)blockIdx.z / p.sw : 0, cw = DIR == LRPX_GEOM_BWD ? (int)blockIdx.z % p.sw : 0;
    const int cs_h = DIR == LRPX_GEOM_BWD ? p.sh : 1, cs_w = DIR == LRPX_GEOM_BWD ? p.sw : 1;
    const int OY = DIR == LRPX_GEOM_BWD ? p.H : p.OH, OX = DIR == LRPX_GEOM_BWD ? p.W : p.OW;     // output map
    const int SY = DIR == LRPX_GEOM_BWD ? p.OH : p.H, SX = DIR == LRPX_GEOM_BWD ? p.OW : p.W;     // source map
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

    f32x4 ra[2], bcur[4], bnext[4];
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) bcur[g] = bnext[g] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto load_stage = [&](int st, f32x4* b) {
        const int t = st / p.nchunk, chunk = st - t * p.nchunk;
        const int i = t / ns, j = t - i * ns;
        const int kc = chunk * CG_KC + c4;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int sy = DIR == LRPX_GEOM_BWD ? phi[u] + yb - i : phi[u] * p.sh - p.ph + i;
            const int sx = DIR == LRPX_GEOM_BWD ? pwi[u] + xb - j : pwi[u] * p.sw - p.pw + j;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (pn[u] >= 0 && sy >= 0 && sy < SY && sx >= 0 && sx < SX && kc < p.K) {
                const long pix = (long)sy * SX + sx;
                const bool neg = AB && kc >= p.kr;                 // the W- half of the stacked contraction
                const int c = neg ? kc - p.kr : kc, ld = AB ? p.kr : p.K;
                v = *reinterpret_cast<const f32x4*>(p.in + ((long)pn[u] * SY * SX + pix) * ld + c);
                if (DIR == LRPX_GEOM_BWD && p.q) {
                    const f32x4 qv = *reinterpret_cast<const f32x4*>((neg ? p.q2 : p.q) + ((long)pim[u] * SY * SX + pix) * ld + c);
                    v = v * qv;
                }
                if (AB) v = v * (neg ? p.scale2 : p.scale);        // (R q) s in this order: s = 1 leaves the preset's operand
            }
            ra[u] = v;
        }
        if (active) {
            const int r = DIR == LRPX_GEOM_BWD ? r0 + i * p.sh : i, s = DIR == LRPX_GEOM_BWD ? s0 + j * p.sw : j;
            const float* bp = p.wp + (((long)ocb * p.taps + (r * p.kw + s)) * p.nchunk + chunk) * CG_FRAG + lane * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const f32x4*>(bp + g * 256);
        }
    };

    if (nst > 0) load_stage(0, bcur);
    for (int st = 0; st < nst; ++st) {
        __syncthreads();                            // the previous stage's fragments have been read
#pragma unroll
        for (int u = 0; u < 2; ++u)
            *reinterpret_cast<f32x4*>(a_lds + ((tid >> 3) + 32 * u) * CG_LDA + c4) = ra[u];
        __syncthreads();
        if (st + 1 < nst) load_stage(st + 1, bnext);   // in flight under this stage's MFMAs
        if (active) {
            const float* ap = a_lds + (wm * 32 + (lane & 31)) * CG_LDA + 4 * (lane >> 5);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 8 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bcur[g][e], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) bcur[g] = bnext[g];
    }

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
        } else {
            const long img = p.map2img ? p.map2img[m] : m;
            float v = nst > 0 ? acc[e] * p.x[(img * OY * OX + pix) * p.n_oc + oc] : 0.f;
            if (p.addend) v += p.addend[off];
            p.out[off] = v;
        }
    }
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

int lrpx_conv_geom_ex(const lrpx_conv_geom_ex_desc* d, void* stream) {
    LRPX_REQUIRE(d, "conv_geom_ex: null descriptor");
    LRPX_REQUIRE(d->in && d->wpacked && d->out, "conv_geom_ex: null pointer");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->dir == LRPX_GEOM_BWD, "conv_geom_ex: unknown direction %d", d->dir);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->x, "conv_geom_ex: the transposed direction needs the multiplicand x");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_BWD || (!d->x && !d->q && !d->addend && !d->map2img),
                 "conv_geom_ex: x, q, addend and map2img belong to the transposed direction");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || !d->bias, "conv_geom_ex: bias belongs to the forward direction");
    LRPX_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->oh > 0 && d->ow > 0 && d->k > 0 && d->n_oc > 0, "conv_geom_ex: bad sizes");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->n_img > 0, "conv_geom_ex: the transposed direction needs n_img > 0 (the images x / q hold)");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->map2img || d->n_img == d->n, "conv_geom_ex: without map2img there is one map per image (n = %d, n_img = %d)", d->n, d->n_img);
    LRPX_REQUIRE(d->kh > 0 && d->kw > 0 && d->kh * d->kw <= 1024 && d->sh > 0 && d->sw > 0 && d->ph >= 0 && d->pw >= 0,
                 "conv_geom_ex: bad window (kernel %dx%d stride %dx%d padding %dx%d)", d->kh, d->kw, d->sh, d->sw, d->ph, d->pw);
    LRPX_REQUIRE(d->h + 2 * d->ph >= d->kh && d->w + 2 * d->pw >= d->kw && d->oh == (d->h + 2 * d->ph - d->kh) / d->sh + 1 &&
                     d->ow == (d->w + 2 * d->pw - d->kw) / d->sw + 1,
                 "conv_geom_ex: output %dx%d is not what input %dx%d gives", d->oh, d->ow, d->h, d->w);
    LRPX_REQUIRE(d->k % 4 == 0 && ((uintptr_t)d->in & 15) == 0 && ((uintptr_t)d->wpacked & 15) == 0 && ((uintptr_t)d->q & 15) == 0,
                 "conv_geom_ex: the contraction channels (%d) must be a multiple of 4 and in / q / wpacked 16-byte aligned", d->k);
    const long pix_in = (long)d->n * d->h * d->w, pix_out = (long)d->n * d->oh * d->ow;
    LRPX_REQUIRE(pix_in < (1L << 31) && pix_out < (1L << 31), "conv_geom_ex: more than 2^31 pixels");
    LRPX_CHECK_PTRS("lrpx_conv_geom_ex", {d->in, "in"}, {d->wpacked, "wpacked"}, {d->bias, "bias"}, {d->x, "x"}, {d->q, "q"},
                    {d->addend, "addend"}, {d->map2img, "map2img"}, {d->out, "out"});
    CgxParams p = {d->in, d->wpacked, d->bias, d->x, d->q, d->addend, d->map2img, d->out, d->n, d->h, d->w, d->oh, d->ow,
                   d->kh, d->kw, d->sh, d->sw, d->ph, d->pw, d->k, d->n_oc, (int)ceil_div(d->k, CG_KC), d->kh * d->kw,
                   0, nullptr, 0.f, 0.f};
    const unsigned gy = (unsigned)ceil_div(d->n_oc, CG_TN);
    LRPX_REQUIRE(gy < 65536 && d->sh * d->sw < 65536, "conv_geom_ex: too many output channels or stride classes");
    hipStream_t st = (hipStream_t)stream;
    if (d->dir == LRPX_GEOM_FWD) {
        hipLaunchKernelGGL((conv_geom_ex_kernel<LRPX_GEOM_FWD>), dim3((unsigned)ceil_div(pix_out, CG_TM), gy, 1), dim3(256), 0, st, p);
    } else {
        // class (0, 0) holds the most pixels
        const long pc = (long)d->n * ceil_div(d->h, d->sh) * ceil_div(d->w, d->sw);
        hipLaunchKernelGGL((conv_geom_ex_kernel<LRPX_GEOM_BWD>), dim3((unsigned)ceil_div(pc, CG_TM), gy, (unsigned)(d->sh * d->sw)),
                           dim3(256), 0, st, p);
    }
    return check_launch("conv_geom_ex");
}

int lrpx_conv_geom_ab(const lrpx_conv_geom_ab_desc* a, void* stream) {
    LRPX_TRY(conv_geom_ab_check(a, "lrpx_conv_geom_ab"));
    const lrpx_conv_geom_ex_desc* d = &a->base;
    CgxParams p = {d->in, d->wpacked, nullptr, d->x, d->q, d->addend, d->map2img, d->out, d->n, d->h, d->w, d->oh, d->ow,
                   d->kh, d->kw, d->sh, d->sw, d->ph, d->pw, d->k, d->n_oc, (int)ceil_div(d->k, CG_KC), d->kh * d->kw,
                   a->kr, a->q2, a->scale, a->scale2};
    const long pc = (long)d->n * ceil_div(d->h, d->sh) * ceil_div(d->w, d->sw);      // class (0, 0) holds the most pixels
    hipLaunchKernelGGL((conv_geom_ex_kernel<LRPX_GEOM_BWD, true>),
                       dim3((unsigned)ceil_div(pc, CG_TM), (unsigned)ceil_div(d->n_oc, CG_TN), (unsigned)(d->sh * d->sw)), dim3(256), 0,
                       (hipStream_t)stream, p);
    return check_launch("conv_geom_ab");
}

}  // extern "C"
