// Runtime-geometry convolution engine (conv_geom_kernel.h; fp32 MFMA in conv_geom.hip, exact bf16 split in conv_geom_b6.hip): tile
// constants, the packed weight index, the descriptor refusals shared by its five entries.
//
// One implicit-GEMM kernel family for any kernel size / stride / zero padding (dilation 1, groups 1), NHWC fp32:
//   FWD  out[n,oh,ow,co] = sum in[n, oh*sh-ph+r, ow*sw-pw+s, ci] * w[co,ci,r,s] (+ bias[co])
//   BWD  out[n,h,w,ci]   = x[n,h,w,ci] * sum s_in[n,oh,ow,co] * w[co,ci,r,s]   over (r,s,oh,ow) with oh*sh-ph+r = h, ow*sw-pw+s = w
// A workgroup of 4 waves owns CG_TM pixels x CG_TN channels (waves 2 x 2, one 32x32 accumulator each) and walks
// (tap, K chunk of CG_KC channels) stages: the gathered A tile goes through LDS (zero-filled outside the map and beyond K),
// the B fragments come straight from the packed weights.  BWD tiles the output by sub-pixel class (h mod sh, w mod sw): a
// workgroup's pixels share one class and it visits only the taps that reach it.
#pragma once
#include <cmath>

#include "common.h"

namespace lrpx {

constexpr int CG_TM = 64;    // pixels per workgroup
constexpr int CG_TN = 64;    // output channels per workgroup (two 32-wide MFMA column blocks)
constexpr int CG_KC = 32;    // contraction channels per stage

// Both packed weight images are [n_oc / 32][taps][K / CG_KC] fragments of 1024 elements, zero-padded in both channel axes; the
// arithmetic (CgF32 in conv_geom.hip, CgB6 in conv_geom_b6.hip) orders the elements of a fragment.
inline size_t conv_geom_frags(int n_oc, int k, int taps) { return (size_t)ceil_div(n_oc, 32) * taps * ceil_div(k, CG_KC); }

// What a pack kernel needs: w (cout, cin, kh, kw) as nn.Conv2d stores it.  FWD: K = cin, columns = cout; BWD: K = cout, columns = cin.
struct CgPack {
    const float* w;
    long total;              // elements of the image: 1024 per fragment
    int cin, taps, K, n_oc, nchunk, dir;
};

// The weight in contraction row `kk` of its chunk and column `cl` of its column block of fragment `frag` = (ocb, tap, chunk); zero
// beyond K and n_oc.
__device__ __forceinline__ float conv_geom_weight(const CgPack& a, long frag, int kk, int cl) {
    const int chunk = (int)(frag % a.nchunk);
    frag /= a.nchunk;
    const int tap = (int)(frag % a.taps);
    const int ocb = (int)(frag / a.taps);
    const int k = chunk * CG_KC + kk;
    const int col = ocb * 32 + cl;
    if (k >= a.K || col >= a.n_oc) return 0.f;
    const long co = a.dir == LRPX_GEOM_FWD ? col : k, ci = a.dir == LRPX_GEOM_FWD ? k : col;
    return a.w[(co * a.cin + ci) * a.taps + tap];
}

// The refusals of the two packers and the kernel's argument; `fn` names the entry in the message and in the pointer check.
inline int conv_geom_pack_check(const float* w, int cout, int cin, int kh, int kw, int dir, const void* packed, const char* fn, CgPack* a) {
    LRPX_REQUIRE(w && packed, "%s: null pointer", fn);
    LRPX_REQUIRE(cout > 0 && cin > 0 && kh > 0 && kw > 0 && kh * kw <= 1024, "%s: bad shape (%d,%d,%d,%d)", fn, cout, cin, kh, kw);
    LRPX_REQUIRE(dir == LRPX_GEOM_FWD || dir == LRPX_GEOM_BWD, "%s: unknown direction %d", fn, dir);
    LRPX_CHECK_PTRS(fn, {w, "w"}, {packed, "packed"});
    const int K = dir == LRPX_GEOM_FWD ? cin : cout, n_oc = dir == LRPX_GEOM_FWD ? cout : cin, taps = kh * kw;
    *a = {w, (long)conv_geom_frags(n_oc, K, taps) * 1024, cin, taps, K, n_oc, (int)ceil_div(K, CG_KC), dir};
    LRPX_REQUIRE(ceil_div(a->total, 256) < (1L << 31), "%s: weight tensor too large", fn);
    return LRPX_OK;
}

// What the dual-coefficient transposed entries (lrpx_conv_geom_ab, lrpx_conv_geom_ab_b6) add to conv_geom_check: the transposed direction
// alone, q required, and the second coefficient's refusals.
inline int conv_geom_ab_check(const lrpx_conv_geom_ab_desc* a, const char* fn) {
    const lrpx_conv_geom_ex_desc* d = &a->base;
    LRPX_REQUIRE(d->dir == LRPX_GEOM_BWD, "%s: the transposed direction only (dir %d): the forward direction has no coefficients", fn, d->dir);
    LRPX_REQUIRE(d->x && d->q, "%s: the transposed direction needs the multiplicand x and the coefficient q", fn);
    LRPX_REQUIRE(a->kr > 0, "%s: bad sizes", fn);
    LRPX_REQUIRE(a->kr % 4 == 0 && ((uintptr_t)a->q2 & 15) == 0,
                 "%s: the relevance channels kr (%d) must be a multiple of 4 and in / q / q2 / wpacked 16-byte aligned", fn, a->kr);
    LRPX_REQUIRE(d->k == a->kr || d->k == 2 * a->kr, "%s: k (%d) is kr (%d, the W+ half alone) or 2 kr (the rows [W+ ; W-])", fn, d->k, a->kr);
    LRPX_REQUIRE((d->k == 2 * a->kr) == (a->q2 != nullptr), "%s: q2 goes with k = 2 kr: null where the W- half is contracted, or given without it", fn);
    LRPX_REQUIRE(std::isfinite(a->scale) && std::isfinite(a->scale2) && (a->q2 || a->scale2 == 0.f),
                 "%s: scale / scale2 must be finite (%g, %g) and scale2 zero without q2", fn, (double)a->scale, (double)a->scale2);
    return LRPX_OK;
}

// What the pooled-operand entries (lrpx_conv_geom_ab_pool, lrpx_conv_geom_ab_pool_b6) check before conv_geom_check sees their ab part:
// the one pool the gather is written for, and a pooled map that is not empty.
inline int conv_geom_pool_check(const lrpx_conv_geom_ab_pool_desc* a, const char* fn) {
    LRPX_REQUIRE(a, "%s: null descriptor", fn);
    LRPX_REQUIRE(a->pool == 2, "%s: pool must be 2 (kernel = stride = 2, no padding, floor mode), got %d", fn, a->pool);
    LRPX_REQUIRE(a->ab.base.oh >= 2 && a->ab.base.ow >= 2, "%s: the conv's output %dx%d leaves the pool no window", fn, a->ab.base.oh,
                 a->ab.base.ow);
    return LRPX_OK;
}

// What the gradient entries (lrpx_conv_geom_grad, lrpx_conv_geom_grad_b6) add to conv_geom_check: the transposed direction alone, no
// multiplicand, coefficient or bias, and the refusals of mask / scale / clamp.
inline int conv_geom_grad_check(const lrpx_conv_geom_grad_desc* g, const char* fn) {
    const lrpx_conv_geom_ex_desc* d = &g->base;
    LRPX_REQUIRE(d->dir == LRPX_GEOM_BWD, "%s: the transposed direction only (dir %d): the gradient of a conv's input", fn, d->dir);
    LRPX_REQUIRE(!d->x && !d->q && !d->bias, "%s: x, q and bias must be null: the gradient has no multiplicand, coefficient or bias", fn);
    LRPX_REQUIRE(((uintptr_t)g->mask & 15) == 0 && ((uintptr_t)g->scale & 15) == 0, "%s: mask and scale must be 16-byte aligned", fn);
    LRPX_REQUIRE(g->clamp == 0 || g->clamp == 1, "%s: clamp is 0 or 1 (%d)", fn, g->clamp);
    return LRPX_OK;
}

// The refusals shared by lrpx_conv_geom, _ex, _ex_b6, _ab, _ab_b6, _grad and _grad_b6 (d = &ab->base, d = &gr->base).  `fn` names the entry in the message
// and in the pointer check, which comes last: it asks the runtime.
inline int conv_geom_check(const lrpx_conv_geom_ex_desc* d, const char* fn, const lrpx_conv_geom_ab_desc* ab = nullptr,
                           const lrpx_conv_geom_grad_desc* gr = nullptr) {
    LRPX_REQUIRE(d, "%s: null descriptor", fn);
    LRPX_REQUIRE(d->in && d->wpacked && d->out, "%s: null pointer", fn);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->dir == LRPX_GEOM_BWD, "%s: unknown direction %d", fn, d->dir);
    if (ab) LRPX_TRY(conv_geom_ab_check(ab, fn));
    if (gr) LRPX_TRY(conv_geom_grad_check(gr, fn));
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->x || gr, "%s: the transposed direction needs the multiplicand x", fn);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_BWD || (!d->x && !d->q && !d->addend && !d->map2img),
                 "%s: x, q, addend and map2img belong to the transposed direction", fn);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || !d->bias, "%s: bias belongs to the forward direction", fn);
    LRPX_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->oh > 0 && d->ow > 0 && d->k > 0 && d->n_oc > 0, "%s: bad sizes", fn);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->n_img > 0, "%s: the transposed direction needs n_img > 0 (the images x / q hold)", fn);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_FWD || d->map2img || d->n_img == d->n, "%s: without map2img there is one map per image (n = %d, n_img = %d)",
                 fn, d->n, d->n_img);
    LRPX_REQUIRE(d->kh > 0 && d->kw > 0 && d->kh * d->kw <= 1024 && d->sh > 0 && d->sw > 0 && d->ph >= 0 && d->pw >= 0,
                 "%s: bad window (kernel %dx%d stride %dx%d padding %dx%d)", fn, d->kh, d->kw, d->sh, d->sw, d->ph, d->pw);
    LRPX_REQUIRE(d->h + 2 * d->ph >= d->kh && d->w + 2 * d->pw >= d->kw && d->oh == (d->h + 2 * d->ph - d->kh) / d->sh + 1 &&
                     d->ow == (d->w + 2 * d->pw - d->kw) / d->sw + 1,
                 "%s: output %dx%d is not what input %dx%d gives", fn, d->oh, d->ow, d->h, d->w);
    LRPX_REQUIRE(d->k % 4 == 0 && ((uintptr_t)d->in & 15) == 0 && ((uintptr_t)d->wpacked & 15) == 0 && ((uintptr_t)d->q & 15) == 0,
                 "%s: the contraction channels (%d) must be a multiple of 4 and in / q / wpacked 16-byte aligned", fn, d->k);
    const long pix_in = (long)d->n * d->h * d->w, pix_out = (long)d->n * d->oh * d->ow;
    LRPX_REQUIRE(pix_in < (1L << 31) && pix_out < (1L << 31), "%s: more than 2^31 pixels", fn);
    LRPX_REQUIRE(ceil_div(d->n_oc, CG_TN) < 65536 && d->sh * d->sw < 65536, "%s: too many output channels or stride classes", fn);
    LRPX_CHECK_PTRS(fn, {d->in, "in"}, {d->wpacked, "wpacked"}, {d->bias, "bias"}, {d->x, "x"}, {d->q, "q"}, {ab ? ab->q2 : nullptr, "q2"},
                    {d->addend, "addend"}, {d->map2img, "map2img"}, {d->out, "out"}, {gr ? gr->mask : nullptr, "mask"},
                    {gr ? gr->scale : nullptr, "scale"});
    return LRPX_OK;
}

}  // namespace lrpx
