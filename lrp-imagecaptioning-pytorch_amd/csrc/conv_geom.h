// Runtime-geometry convolution engine on the fp32 MFMA (conv_geom.hip): tile constants and the packed weight layout.
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
constexpr int CG_LDA = 36;   // floats per pixel row of the LDS A tile: 16 consecutive rows of a b128 read cover all 64 banks

// Packed weights: [n_oc / 32][taps][K / CG_KC][CG_KC / 8][64 lanes][4], zero-padded in both channel axes.  Element e of lane l in
// k-step group g of a chunk is B[k = chunk * 32 + 8 g + 4 (l >> 5) + e][column = 32 ocb + (l & 31)]: the operand of the e-th
// v_mfma_f32_32x32x2_f32 of that group, so a wave's fragment is one contiguous 1 KiB float4 load.
constexpr int CG_FRAG = CG_KC * 32;      // floats per (column block, tap, chunk)
inline size_t conv_geom_floats(int n_oc, int k, int taps) {
    return (size_t)ceil_div(n_oc, 32) * taps * ceil_div(k, CG_KC) * CG_FRAG;
}

// The refusals of the dual-coefficient transposed entries (lrpx_conv_geom_ab, lrpx_conv_geom_ab_b6): those of lrpx_conv_geom_ex for the
// transposed direction plus the second coefficient's.  `fn` names the entry in the message and in the pointer check.
inline int conv_geom_ab_check(const lrpx_conv_geom_ab_desc* a, const char* fn) {
    LRPX_REQUIRE(a, "%s: null descriptor", fn);
    const lrpx_conv_geom_ex_desc* d = &a->base;
    LRPX_REQUIRE(d->in && d->wpacked && d->out, "%s: null pointer", fn);
    LRPX_REQUIRE(d->dir == LRPX_GEOM_BWD, "%s: the transposed direction only (dir %d): the forward direction has no coefficients", fn, d->dir);
    LRPX_REQUIRE(d->x && d->q, "%s: the transposed direction needs the multiplicand x and the coefficient q", fn);
    LRPX_REQUIRE(!d->bias, "%s: bias belongs to the forward direction", fn);
    LRPX_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->oh > 0 && d->ow > 0 && d->k > 0 && d->n_oc > 0 && a->kr > 0, "%s: bad sizes", fn);
    LRPX_REQUIRE(d->n_img > 0, "%s: the transposed direction needs n_img > 0 (the images x / q / q2 hold)", fn);
    LRPX_REQUIRE(d->map2img || d->n_img == d->n, "%s: without map2img there is one map per image (n = %d, n_img = %d)", fn, d->n, d->n_img);
    LRPX_REQUIRE(d->kh > 0 && d->kw > 0 && d->kh * d->kw <= 1024 && d->sh > 0 && d->sw > 0 && d->ph >= 0 && d->pw >= 0,
                 "%s: bad window (kernel %dx%d stride %dx%d padding %dx%d)", fn, d->kh, d->kw, d->sh, d->sw, d->ph, d->pw);
    LRPX_REQUIRE(d->h + 2 * d->ph >= d->kh && d->w + 2 * d->pw >= d->kw && d->oh == (d->h + 2 * d->ph - d->kh) / d->sh + 1 &&
                     d->ow == (d->w + 2 * d->pw - d->kw) / d->sw + 1,
                 "%s: output %dx%d is not what input %dx%d gives", fn, d->oh, d->ow, d->h, d->w);
    LRPX_REQUIRE(a->kr % 4 == 0 && ((uintptr_t)d->in & 15) == 0 && ((uintptr_t)d->wpacked & 15) == 0 && ((uintptr_t)d->q & 15) == 0 &&
                     ((uintptr_t)a->q2 & 15) == 0,
                 "%s: the relevance channels kr (%d) must be a multiple of 4 and in / q / q2 / wpacked 16-byte aligned", fn, a->kr);
    LRPX_REQUIRE(d->k == a->kr || d->k == 2 * a->kr, "%s: k (%d) is kr (%d, the W+ half alone) or 2 kr (the rows [W+ ; W-])", fn, d->k, a->kr);
    LRPX_REQUIRE((d->k == 2 * a->kr) == (a->q2 != nullptr), "%s: q2 goes with k = 2 kr: null where the W- half is contracted, or given without it", fn);
    LRPX_REQUIRE(std::isfinite(a->scale) && std::isfinite(a->scale2) && (a->q2 || a->scale2 == 0.f),
                 "%s: scale / scale2 must be finite (%g, %g) and scale2 zero without q2", fn, (double)a->scale, (double)a->scale2);
    const long pix_in = (long)d->n * d->h * d->w, pix_out = (long)d->n * d->oh * d->ow;
    LRPX_REQUIRE(pix_in < (1L << 31) && pix_out < (1L << 31), "%s: more than 2^31 pixels", fn);
    LRPX_REQUIRE(ceil_div(d->n_oc, CG_TN) < 65536 && d->sh * d->sw < 65536, "%s: too many output channels or stride classes", fn);
    LRPX_CHECK_PTRS(fn, {d->in, "in"}, {d->wpacked, "wpacked"}, {d->x, "x"}, {d->q, "q"}, {a->q2, "q2"}, {d->addend, "addend"},
                    {d->map2img, "map2img"}, {d->out, "out"});
    return LRPX_OK;
}

}  // namespace lrpx
