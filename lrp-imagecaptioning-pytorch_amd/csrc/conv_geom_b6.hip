// The batched runtime-geometry contraction (conv_geom_ex.hip) in the exact arithmetic of conv mode 1: lrpx_conv_geom_ex_b6.
// Every fp32 operand is split exactly into three bf16 planes (conv_bf16x6.h: split3) and the six plane products with i + j <= 2 run
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, small terms first: 12 MFMAs of 32 cycles per (tap, 32-channel chunk) stage in
// place of 16 fp32 MFMAs of 64.  Tile, stages, gather indices, sub-pixel classes, masking, operands and epilogue are those of
// conv_geom_ex_kernel; what differs:
//   A   the gathered float4 (times q, in fp32) is split between the global load and the LDS store.  LDS row of a pixel:
//       [k-step 2][plane 3][16 bf16] = 192 B + 16 B pad, so a lane's fragment of a plane (A[row l & 31][k = 8 (l >> 5) + j]) is one
//       ds_read_b128 and the 16 rows of a phase, 13 sixteen-byte slots apart, land in 16 distinct 4-bank groups (13 is odd)
//   B   split at pack time (lrpx_conv_geom_pack_bf16x3): [n_oc / 32][taps][K / 32][k-step 2][plane 3][64 lanes][8 bf16]; element j of
//       lane l is W[k = 32 chunk + 16 ks + 8 (l >> 5) + j][column 32 ocb + (l & 31)], zero beyond K and n_oc: a fragment is one
//       contiguous 1 KiB load
// The general alpha-beta rule (lrpx_conv_geom_ab_b6): the dual-coefficient A gather of conv_geom_ex.hip, (R q) s in
// fp32, THEN split3 - over the stacked rows [W+ ; W-] packed by lrpx_conv_geom_pack_bf16x3 as one tensor of 2 kr rows.
// split3 of +-inf leaves NaN in the lower planes: an overflowing in * q gives NaN here where the fp32 kernel gives inf.
#include "conv_geom.h"
#include "conv_bf16x6.h"

namespace lrpx {

constexpr int CG6_ROWB = 208;                    // bytes per pixel row of the LDS A tile
constexpr int CG6_FRAGB = 2 * 3 * 1024;          // bytes per (column block, tap, chunk) of the packed image
inline size_t conv_geom_b6_bytes(int n_oc, int k, int taps) {
    return (size_t)ceil_div(n_oc, 32) * taps * ceil_div(k, CG_KC) * CG6_FRAGB;
}

struct Cg6Params {
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
};

// one thread per element of [ocb][tap][chunk][k-step][lane][j]; it writes the element's three planes
__global__ void conv_geom_pack_bf16x3_kernel(const float* __restrict__ w, unsigned short* __restrict__ packed, long total, int cin,
                                             int taps, int K, int n_oc, int nchunk, int dir) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63), ks = (int)((idx >> 9) & 1);
    const long frag = idx >> 10;                 // (ocb, tap, chunk)
    long rest = frag;
    const int chunk = (int)(rest % nchunk);
    rest /= nchunk;
    const int tap = (int)(rest % taps);
    const int ocb = (int)(rest / taps);
    const int k = chunk * CG_KC + 16 * ks + 8 * (lane >> 5) + j;
    const int col = ocb * 32 + (lane & 31);
    float v = 0.f;
    if (k < K && col < n_oc) {
        const long co = dir == LRPX_GEOM_FWD ? col : k, ci = dir == LRPX_GEOM_FWD ? k : col;
        v = w[(co * cin + ci) * taps + tap];
    }
    unsigned short p[3];
    split3(v, p[0], p[1], p[2]);
    unsigned short* dst = packed + ((frag * 2 + ks) * 3) * 512 + lane * 8 + j;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) dst[pl * 512] = p[pl];
}

// DIR = LRPX_GEOM_FWD: output pixels are the (OH, OW) map, sources the (H, W) map.
// DIR = LRPX_GEOM_BWD: output pixels are the (H, W) map in sub-pixel classes (blockIdx.z), sources the (OH, OW) map.
// AB (transposed direction only) 1: the dual-coefficient gather over the W+ half alone (K = kr);  2: over both halves (K = 2 kr), with the
// cross products in an accumulator of their own.
template <int DIR, int AB = 0>
__global__ __launch_bounds__(256) void conv_geom_b6_kernel(const Cg6Params p) {
    __shared__ __attribute__((aligned(16))) char a_lds[CG_TM * CG6_ROWB];
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

    f32x4 ra[2];
    u32x4 bcur[6], bnext[6];                        // [k-step][plane]
    f32x16 acc, acc_lo;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = acc_lo[e] = 0.f;
    // AB = 2: the five cross products (2^-8 of a term and below) collect in an accumulator of their own, joined to the a0 b0 sums once at
    // the end.  The W+ and W- sums cancel, so the running sum is large against the result, and every MFMA that adds into it rounds at
    // the running sum's size: two per stage then, not twelve.  Otherwise this is the one accumulator of the parent - AB = 1 sums in the
    // parent's order, so that scale 1 gives the parent's bytes.
    f32x16& lo = AB == 2 ? acc_lo : acc;
#pragma unroll
    for (int g = 0; g < 6; ++g) bcur[g] = bnext[g] = u32x4{0, 0, 0, 0};

    auto load_stage = [&](int st, u32x4* b) {
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
            const char* bp = p.wp + (((long)ocb * p.taps + (r * p.kw + s)) * p.nchunk + chunk) * CG6_FRAGB + lane * 16;
#pragma unroll
            for (int g = 0; g < 6; ++g) b[g] = *reinterpret_cast<const u32x4*>(bp + g * 1024);
        }
    };

    // this thread's 4 channels in the LDS row: k-step c4 / 16, bf16 c4 % 16 .. + 3 of each plane
    const int a_dst = (c4 >> 4) * 96 + (c4 & 15) * 2;
    if (nst > 0) load_stage(0, bcur);
    for (int st = 0; st < nst; ++st) {
        __syncthreads();                            // the previous stage's fragments have been read
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            unsigned short p0[4], p1[4], p2[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split3(ra[u][e], p0[e], p1[e], p2[e]);
            char* d = a_lds + ((tid >> 3) + 32 * u) * CG6_ROWB + a_dst;
            *reinterpret_cast<u32x2*>(d) = u32x2{p0[0] | ((unsigned)p0[1] << 16), p0[2] | ((unsigned)p0[3] << 16)};
            *reinterpret_cast<u32x2*>(d + 32) = u32x2{p1[0] | ((unsigned)p1[1] << 16), p1[2] | ((unsigned)p1[3] << 16)};
            *reinterpret_cast<u32x2*>(d + 64) = u32x2{p2[0] | ((unsigned)p2[1] << 16), p2[2] | ((unsigned)p2[3] << 16)};
        }
        __syncthreads();
        if (st + 1 < nst) load_stage(st + 1, bnext);   // in flight under this stage's MFMAs
        if (active) {
            const char* ap = a_lds + (wm * 32 + (lane & 31)) * CG6_ROWB + 16 * (lane >> 5);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ap + ks * 96);
                const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap + ks * 96 + 32);
                const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(ap + ks * 96 + 64);
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, bcur[3 * ks]);
                const bf16x8 b1 = __builtin_bit_cast(bf16x8, bcur[3 * ks + 1]);
                const bf16x8 b2 = __builtin_bit_cast(bf16x8, bcur[3 * ks + 2]);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, lo, 0, 0, 0);        // small terms first
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, lo, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, lo, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, lo, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, lo, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < 6; ++g) bcur[g] = bnext[g];
    }

    if (AB == 2) acc = acc + acc_lo;
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

size_t lrpx_conv_geom_packed_bf16x3_bytes(int n_oc, int k, int taps) {
    if (n_oc <= 0 || k <= 0 || taps <= 0) return 0;
    return conv_geom_b6_bytes(n_oc, k, taps);
}

int lrpx_conv_geom_pack_bf16x3(const float* w, int cout, int cin, int kh, int kw, int dir, void* packed, void* stream) {
    LRPX_REQUIRE(w && packed, "conv_geom_pack_bf16x3: null pointer");
    LRPX_REQUIRE(cout > 0 && cin > 0 && kh > 0 && kw > 0 && kh * kw <= 1024, "conv_geom_pack_bf16x3: bad shape (%d,%d,%d,%d)", cout, cin, kh,
                 kw);
    LRPX_REQUIRE(dir == LRPX_GEOM_FWD || dir == LRPX_GEOM_BWD, "conv_geom_pack_bf16x3: unknown direction %d", dir);
    LRPX_REQUIRE(((uintptr_t)packed & 15) == 0, "conv_geom_pack_bf16x3: packed must be 16-byte aligned");
    LRPX_CHECK_PTRS("lrpx_conv_geom_pack_bf16x3", {w, "w"}, {packed, "packed"});
    const int K = dir == LRPX_GEOM_FWD ? cin : cout, n_oc = dir == LRPX_GEOM_FWD ? cout : cin, taps = kh * kw;
    const long total = (long)(conv_geom_b6_bytes(n_oc, K, taps) / 6);       // elements: three 2-byte planes each
    LRPX_REQUIRE(ceil_div(total, 256) < (1L << 31), "conv_geom_pack_bf16x3: weight tensor too large");
    hipLaunchKernelGGL(conv_geom_pack_bf16x3_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (unsigned short*)packed, total, cin, taps, K, n_oc, (int)ceil_div(K, CG_KC), dir);
    return check_launch("conv_geom_pack_bf16x3");
}

int lrpx_conv_geom_ex_b6(const lrpx_conv_geom_ex_desc* d, void* stream) {
    LRPX_REQUIRE(d, "conv_geom_ex_b6: null descriptor");
    LRPX_REQUIRE(d->in && d->wpacked && d->out, "conv_geom_ex_b6: null pointer");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->dir == LRPX_GEOM_BWD, "conv_geom_ex_b6: unknown direction %d", d->dir);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->x, "conv_geom_ex_b6: the transposed direction needs the multiplicand x");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_BWD || (!d->x && !d->q && !d->addend && !d->map2img),
                 "conv_geom_ex_b6: x, q, addend and map2img belong to the transposed direction");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || !d->bias, "conv_geom_ex_b6: bias belongs to the forward direction");
    LRPX_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->oh > 0 && d->ow > 0 && d->k > 0 && d->n_oc > 0, "conv_geom_ex_b6: bad sizes");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->n_img > 0, "conv_geom_ex_b6: the transposed direction needs n_img > 0 (the images x / q hold)");
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->map2img || d->n_img == d->n,
                 "conv_geom_ex_b6: without map2img there is one map per image (n = %d, n_img = %d)", d->n, d->n_img);
    LRPX_REQUIRE(d->kh > 0 && d->kw > 0 && d->kh * d->kw <= 1024 && d->sh > 0 && d->sw > 0 && d->ph >= 0 && d->pw >= 0,
                 "conv_geom_ex_b6: bad window (kernel %dx%d stride %dx%d padding %dx%d)", d->kh, d->kw, d->sh, d->sw, d->ph, d->pw);
    LRPX_REQUIRE(d->h + 2 * d->ph >= d->kh && d->w + 2 * d->pw >= d->kw && d->oh == (d->h + 2 * d->ph - d->kh) / d->sh + 1 &&
                     d->ow == (d->w + 2 * d->pw - d->kw) / d->sw + 1,
                 "conv_geom_ex_b6: output %dx%d is not what input %dx%d gives", d->oh, d->ow, d->h, d->w);
    LRPX_REQUIRE(d->k % 4 == 0 && ((uintptr_t)d->in & 15) == 0 && ((uintptr_t)d->wpacked & 15) == 0 && ((uintptr_t)d->q & 15) == 0,
                 "conv_geom_ex_b6: the contraction channels (%d) must be a multiple of 4 and in / q / wpacked 16-byte aligned", d->k);
    const long pix_in = (long)d->n * d->h * d->w, pix_out = (long)d->n * d->oh * d->ow;
    LRPX_REQUIRE(pix_in < (1L << 31) && pix_out < (1L << 31), "conv_geom_ex_b6: more than 2^31 pixels");
    LRPX_CHECK_PTRS("lrpx_conv_geom_ex_b6", {d->in, "in"}, {d->wpacked, "wpacked"}, {d->bias, "bias"}, {d->x, "x"}, {d->q, "q"},
                    {d->addend, "addend"}, {d->map2img, "map2img"}, {d->out, "out"});
    Cg6Params p = {d->in, (const char*)d->wpacked, d->bias, d->x, d->q, d->addend, d->map2img, d->out, d->n, d->h, d->w, d->oh, d->ow,
                   d->kh, d->kw, d->sh, d->sw, d->ph, d->pw, d->k, d->n_oc, (int)ceil_div(d->k, CG_KC), d->kh * d->kw,
                   0, nullptr, 0.f, 0.f};
    const unsigned gy = (unsigned)ceil_div(d->n_oc, CG_TN);
    LRPX_REQUIRE(gy < 65536 && d->sh * d->sw < 65536, "conv_geom_ex_b6: too many output channels or stride classes");
    hipStream_t st = (hipStream_t)stream;
    if (d->dir == LRPX_GEOM_FWD) {
        hipLaunchKernelGGL((conv_geom_b6_kernel<LRPX_GEOM_FWD>), dim3((unsigned)ceil_div(pix_out, CG_TM), gy, 1), dim3(256), 0, st, p);
    } else {
        // class (0, 0) holds the most pixels
        const long pc = (long)d->n * ceil_div(d->h, d->sh) * ceil_div(d->w, d->sw);
        hipLaunchKernelGGL((conv_geom_b6_kernel<LRPX_GEOM_BWD>), dim3((unsigned)ceil_div(pc, CG_TM), gy, (unsigned)(d->sh * d->sw)),
                           dim3(256), 0, st, p);
    }
    return check_launch("conv_geom_ex_b6");
}

int lrpx_conv_geom_ab_b6(const lrpx_conv_geom_ab_desc* a, void* stream) {
    LRPX_TRY(conv_geom_ab_check(a, "lrpx_conv_geom_ab_b6"));
    const lrpx_conv_geom_ex_desc* d = &a->base;
    Cg6Params p = {d->in, (const char*)d->wpacked, nullptr, d->x, d->q, d->addend, d->map2img, d->out, d->n, d->h, d->w, d->oh, d->ow,
                   d->kh, d->kw, d->sh, d->sw, d->ph, d->pw, d->k, d->n_oc, (int)ceil_div(d->k, CG_KC), d->kh * d->kw,
                   a->kr, a->q2, a->scale, a->scale2};
    const long pc = (long)d->n * ceil_div(d->h, d->sh) * ceil_div(d->w, d->sw);      // class (0, 0) holds the most pixels
    const dim3 grid((unsigned)ceil_div(pc, CG_TM), (unsigned)ceil_div(d->n_oc, CG_TN), (unsigned)(d->sh * d->sw));
    if (a->q2) {
        hipLaunchKernelGGL((conv_geom_b6_kernel<LRPX_GEOM_BWD, 2>), grid, dim3(256), 0, (hipStream_t)stream, p);
    } else {
        hipLaunchKernelGGL((conv_geom_b6_kernel<LRPX_GEOM_BWD, 1>), grid, dim3(256), 0, (hipStream_t)stream, p);
    }
    return check_launch("conv_geom_ab_b6");
}

}  // extern "C"
