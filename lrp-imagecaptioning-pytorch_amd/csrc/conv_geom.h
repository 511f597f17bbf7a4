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

}  // namespace lrpx
