// The runtime-geometry contraction engine (conv_geom_kernel.h) in the exact arithmetic of conv mode 1: lrpx_conv_geom_ex_b6,
// lrpx_conv_geom_ab_b6 and their packer.  Every fp32 operand is split exactly into three bf16 planes (conv_bf16x6.h: split3) and the six
// plane products with i + j <= 2 run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, small terms first: 12 MFMAs of 32 cycles per
// (tap, 32-channel chunk) stage in place of 16 fp32 MFMAs of 64.  Tile, stages, gather indices, sub-pixel classes, masking, operands and
// epilogue are the shared kernel's, so the zero pattern is that of conv mode 0; the alpha-beta gather forms (R q) s in fp32, THEN splits.
// split3 of +-inf leaves NaN in the lower planes: an overflowing in * q gives NaN here where the fp32 kernel gives inf.
#include "conv_geom_kernel.h"
#include "conv_bf16x6.h"

namespace lrpx {

// A   the gathered float4 (times q, in fp32) is split between the global load and the LDS store.  LDS row of a pixel:
//     [k-step 2][plane 3][16 bf16] = 192 B + 16 B pad, so a lane's fragment of a plane (A[row l & 31][k = 8 (l >> 5) + j]) is one
//     ds_read_b128 and the 16 rows of a phase, 13 sixteen-byte slots apart, land in 16 distinct 4-bank groups (13 is odd)
// B   split at pack time (lrpx_conv_geom_pack_bf16x3): [n_oc / 32][taps][K / 32][k-step 2][plane 3][64 lanes][8 bf16]; element j of
//     lane l is W[k = 32 chunk + 16 ks + 8 (l >> 5) + j][column 32 ocb + (l & 31)], zero beyond K and n_oc: a fragment is one
//     contiguous 1 KiB load
struct CgB6 {
    static constexpr int ROWB = 208;
    typedef u32x4 BFrag;                            // [k-step][plane]
    static constexpr int NB = 6;
    // this thread's 4 channels in the LDS row: k-step c4 / 16, bf16 c4 % 16 .. + 3 of each plane
    static __device__ __forceinline__ void store_a(char* row, int c4, f32x4 v) {
        unsigned short p0[4], p1[4], p2[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) split3(v[e], p0[e], p1[e], p2[e]);
        char* d = row + (c4 >> 4) * 96 + (c4 & 15) * 2;
        *reinterpret_cast<u32x2*>(d) = u32x2{p0[0] | ((unsigned)p0[1] << 16), p0[2] | ((unsigned)p0[3] << 16)};
        *reinterpret_cast<u32x2*>(d + 32) = u32x2{p1[0] | ((unsigned)p1[1] << 16), p1[2] | ((unsigned)p1[3] << 16)};
        *reinterpret_cast<u32x2*>(d + 64) = u32x2{p2[0] | ((unsigned)p2[1] << 16), p2[2] | ((unsigned)p2[3] << 16)};
    }
    // `lo` is `acc` itself (one accumulator, summed in this order) or, for the dual-coefficient contraction over both halves, an
    // accumulator of its own for the five cross products (2^-8 of a term and below), joined to the a0 b0 sums once at the end.  There
    // the W+ and W- sums cancel, so the running sum is large against the result, and every MFMA that adds into it rounds at the running
    // sum's size: two per stage then, not twelve.
    static __device__ __forceinline__ void mma(const char* ap, const BFrag* b, f32x16& acc, f32x16& lo) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ap + ks * 96);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap + ks * 96 + 32);
            const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(ap + ks * 96 + 64);
            const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[3 * ks]);
            const bf16x8 b1 = __builtin_bit_cast(bf16x8, b[3 * ks + 1]);
            const bf16x8 b2 = __builtin_bit_cast(bf16x8, b[3 * ks + 2]);
            lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, lo, 0, 0, 0);        // small terms first
            lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, lo, 0, 0, 0);
            lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, lo, 0, 0, 0);
            lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, lo, 0, 0, 0);
            lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, lo, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
        }
    }
};

// one thread per element of [ocb][tap][chunk][k-step][lane][j]; it writes the element's three planes
__global__ void conv_geom_pack_bf16x3_kernel(const CgPack a, unsigned short* __restrict__ packed) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.total) return;
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63), ks = (int)((idx >> 9) & 1);
    const long frag = idx >> 10;
    unsigned short p[3];
    split3(conv_geom_weight(a, frag, 16 * ks + 8 * (lane >> 5) + j, lane & 31), p[0], p[1], p[2]);
    unsigned short* dst = packed + ((frag * 2 + ks) * 3) * 512 + lane * 8 + j;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) dst[pl * 512] = p[pl];
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

size_t lrpx_conv_geom_packed_bf16x3_bytes(int n_oc, int k, int taps) {
    if (n_oc <= 0 || k <= 0 || taps <= 0) return 0;
    return conv_geom_frags(n_oc, k, taps) * CgB6::NB * 1024;
}

int lrpx_conv_geom_pack_bf16x3(const float* w, int cout, int cin, int kh, int kw, int dir, void* packed, void* stream) {
    CgPack a;
    LRPX_REQUIRE(((uintptr_t)packed & 15) == 0, "lrpx_conv_geom_pack_bf16x3: packed must be 16-byte aligned");
    LRPX_TRY(conv_geom_pack_check(w, cout, cin, kh, kw, dir, packed, "lrpx_conv_geom_pack_bf16x3", &a));
    hipLaunchKernelGGL(conv_geom_pack_bf16x3_kernel, dim3((unsigned)ceil_div(a.total, 256)), dim3(256), 0, (hipStream_t)stream, a,
                       (unsigned short*)packed);
    return check_launch("lrpx_conv_geom_pack_bf16x3");
}

int lrpx_conv_geom_ex_b6(const lrpx_conv_geom_ex_desc* d, void* stream) { return conv_geom_run<CgB6, 0>(d, nullptr, stream, "lrpx_conv_geom_ex_b6"); }

// the forward direction alone, its sums in the blocked order (conv_geom_kernel.h): the Z+ / Z- of the alpha-beta coefficients
int lrpx_conv_geom_ex_b6_blocked(const lrpx_conv_geom_ex_desc* d, void* stream) {
    LRPX_REQUIRE(d && d->dir == LRPX_GEOM_FWD, "lrpx_conv_geom_ex_b6_blocked: the forward direction only");
    return conv_geom_run<CgB6, 0, false, true>(d, nullptr, stream, "lrpx_conv_geom_ex_b6_blocked");
}

// the W+ half alone sums in lrpx_conv_geom_ex_b6's order, so that scale 1 gives its bytes
int lrpx_conv_geom_ab_b6(const lrpx_conv_geom_ab_desc* a, void* stream) {
    LRPX_REQUIRE(a, "lrpx_conv_geom_ab_b6: null descriptor");
    return a->q2 ? conv_geom_run<CgB6, 2>(&a->base, a, stream, "lrpx_conv_geom_ab_b6") : conv_geom_run<CgB6, 1>(&a->base, a, stream, "lrpx_conv_geom_ab_b6");
}

int lrpx_conv_geom_ab_pool_b6(const lrpx_conv_geom_ab_pool_desc* a, void* stream) {
    LRPX_TRY(conv_geom_pool_check(a, "lrpx_conv_geom_ab_pool_b6"));
    return a->ab.q2 ? conv_geom_run<CgB6, 2, true>(&a->ab.base, &a->ab, stream, "lrpx_conv_geom_ab_pool_b6")
                    : conv_geom_run<CgB6, 1, true>(&a->ab.base, &a->ab, stream, "lrpx_conv_geom_ab_pool_b6");
}

// clamp, mask and scale are applied in fp32 before the split: the operand is lrpx_conv_geom_grad's
int lrpx_conv_geom_grad_b6(const lrpx_conv_geom_grad_desc* g, void* stream) {
    LRPX_REQUIRE(g, "lrpx_conv_geom_grad_b6: null descriptor");
    return conv_geom_run<CgB6, 3>(&g->base, nullptr, stream, "lrpx_conv_geom_grad_b6", g);
}

}  // extern "C"
