// Conv2d relevance at any kernel size / stride / padding: the fp32 entries of the runtime-geometry contraction engine
// (conv_geom_kernel.h) and their packer.  Arithmetic grade of conv mode 0 and of the general alpha-beta path: fp32 operands, fp32
// accumulation on v_mfma_f32_32x32x2_f32, one fmaf chain per output over (tap, channel).  The signed-input / alpha / beta / bias handling
// stays outside (lrpx_nchw_to_nhwc_posneg, weight stacks built by the caller, lrpx_divide_stab / lrpx_divide_alpha_beta,
// lrpx_fold_halves): lrpx_conv_geom is a plain convolution (+ bias) and a plain transposed convolution (* x), lrpx_conv_geom_ex the same
// with the operands of a batched relevance pass, lrpx_conv_geom_ab its transposed direction with two coefficients, lrpx_conv_geom_grad
// the transposed direction of the gradient chain (raw weights, the operand clamped / masked / scaled in the gather, no multiplicand).
#include "conv_geom_kernel.h"

namespace lrpx {

// A   LDS row of a pixel: the chunk's 32 floats + 4 of padding (CG_LDA = 36 floats), so that 16 consecutive rows of a b128 read cover
//     all 64 banks.
// B   packed weights: [n_oc / 32][taps][K / CG_KC][CG_KC / 8][64 lanes][4], zero-padded in both channel axes.  Element e of lane l in
//     k-step group g of a chunk is B[k = chunk * 32 + 8 g + 4 (l >> 5) + e][column = 32 ocb + (l & 31)]: the operand of the e-th
//     v_mfma_f32_32x32x2_f32 of that group, so a wave's fragment is one contiguous 1 KiB float4 load.
struct CgF32 {
    static constexpr int CG_LDA = 36;
    static constexpr int ROWB = CG_LDA * 4;
    typedef f32x4 BFrag;
    static constexpr int NB = 4;
    static __device__ __forceinline__ void store_a(char* row, int c4, f32x4 v) { *reinterpret_cast<f32x4*>(row + c4 * 4) = v; }
    static __device__ __forceinline__ void mma(const char* ap, const BFrag* b, f32x16& acc, f32x16&) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 32 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b[g][e], acc, 0, 0, 0);
        }
    }
};

// one thread per element of [ocb][tap][chunk][g][lane][e]
__global__ void conv_geom_pack_kernel(const CgPack a, float* __restrict__ packed) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.total) return;
    const int e = (int)(idx & 3), lane = (int)((idx >> 2) & 63), g = (int)((idx >> 8) & 3);
    packed[idx] = conv_geom_weight(a, idx >> 10, 8 * g + 4 * (lane >> 5) + e, lane & 31);
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

size_t lrpx_conv_geom_packed_floats(int n_oc, int k, int taps) {
    if (n_oc <= 0 || k <= 0 || taps <= 0) return 0;
    return conv_geom_frags(n_oc, k, taps) * 1024;
}

int lrpx_conv_geom_pack(const float* w, int cout, int cin, int kh, int kw, int dir, float* packed, void* stream) {
    CgPack a;
    LRPX_TRY(conv_geom_pack_check(w, cout, cin, kh, kw, dir, packed, "lrpx_conv_geom_pack", &a));
    hipLaunchKernelGGL(conv_geom_pack_kernel, dim3((unsigned)ceil_div(a.total, 256)), dim3(256), 0, (hipStream_t)stream, a, packed);
    return check_launch("lrpx_conv_geom_pack");
}

// the batched kernel without the batched operands: one map per image, no q, no addend
int lrpx_conv_geom(const lrpx_conv_geom_desc* d, void* stream) {
    LRPX_REQUIRE(d, "lrpx_conv_geom: null descriptor");
    const lrpx_conv_geom_ex_desc e = {d->in, d->wpacked, d->bias, d->x, nullptr, nullptr, nullptr, d->out, d->dir, d->n, d->n, d->h, d->w,
                                      d->oh, d->ow, d->kh, d->kw, d->sh, d->sw, d->ph, d->pw, d->k, d->n_oc};
    return conv_geom_run<CgF32, 0>(&e, nullptr, stream, "lrpx_conv_geom");
}

int lrpx_conv_geom_ex(const lrpx_conv_geom_ex_desc* d, void* stream) { return conv_geom_run<CgF32, 0>(d, nullptr, stream, "lrpx_conv_geom_ex"); }

int lrpx_conv_geom_ab(const lrpx_conv_geom_ab_desc* a, void* stream) {
    LRPX_REQUIRE(a, "lrpx_conv_geom_ab: null descriptor");
    return conv_geom_run<CgF32, 1>(&a->base, a, stream, "lrpx_conv_geom_ab");
}

int lrpx_conv_geom_ab_pool(const lrpx_conv_geom_ab_pool_desc* a, void* stream) {
    LRPX_TRY(conv_geom_pool_check(a, "lrpx_conv_geom_ab_pool"));
    return conv_geom_run<CgF32, 1, true>(&a->ab.base, &a->ab, stream, "lrpx_conv_geom_ab_pool");
}

int lrpx_conv_geom_grad(const lrpx_conv_geom_grad_desc* g, void* stream) {
    LRPX_REQUIRE(g, "lrpx_conv_geom_grad: null descriptor");
    return conv_geom_run<CgF32, 3>(&g->base, nullptr, stream, "lrpx_conv_geom_grad", g);
}

}  // extern "C"
