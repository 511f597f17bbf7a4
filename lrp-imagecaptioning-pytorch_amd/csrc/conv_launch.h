// Launch helpers for the conv_mfma kernel family and the row type of the kernel list (conv_kernels.def).
#pragma once
#include "common.h"
#include "conv_mfma.h"

namespace lrpx {

template <int HW, int KC, int MT, int NWN, int TAPS, int EPI>
int launch_conv_cfg(const ConvArgs& a, hipStream_t stream) {
    using C = ConvCfg<HW, KC, MT, NWN, TAPS>;
    long m_tiles;
    if (TAPS == 9) m_tiles = ceil_div((long)a.n_maps * HW, C::R);
    else m_tiles = ceil_div((long)a.n_maps * a.pix_per_map, C::PIX);
    const int n_blocks = (int)ceil_div(a.n_oc, 32 * NWN);
    const long grid = ceil_div(m_tiles, 8) * 8 * n_blocks;
    if (grid <= 0 || grid > 0x7fffffffL) {
        set_error("conv_mfma: grid %ld out of range", grid);
        return LRPX_EINVAL;
    }
    auto kern = conv_mfma_kernel<HW, KC, MT, NWN, TAPS, EPI>;
    static LdsOnce attr_once;
    LRPX_TRY(reserve_lds_once(attr_once, kern, C::LDS_BYTES, "conv_mfma"));
    const int ks = a.ksplit > 1 ? a.ksplit : 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid, ks), dim3(C::NT), C::LDS_BYTES, stream, a, (int)m_tiles, n_blocks);
    return check_launch("conv_mfma");
}

// one row of conv_kernels.def: a fixed-geometry conv kernel (launch_<name> = an instantiation of launch_conv_cfg / launch_conv_bf16x6 /
// launch_conv_f16x3 / launch_conv_wino_b6, defined in the generated conv_inst_<unit>.hip) and the descriptors that run on it
enum ConvFamily : int { FAM_FP32, FAM_B6, FAM_H3, FAM_H8 };
enum ConvVariant : int { VAR_DIRECT, VAR_POOL, VAR_WINO_OWN, VAR_WINO_SHARE };
constexpr int OC_ANY = 0x7fffffff;
struct ConvKernel {
    const char* name;
    int (*launch)(const ConvArgs&, hipStream_t);
    int family, hw, epi, variant, oc_min, oc_max;
};

// dense relevance GEMMs with many rows on the fp16 matrix cores (dense_f16x3.hip)
int launch_dense_f16x3(const ConvArgs& a, hipStream_t s);
int launch_dense_bf16x6(const ConvArgs& a, hipStream_t s);      // dense_f16x3.hip, B6: exact bf16 splits, REL epilogue
int launch_dense_small_f16x3(const ConvArgs& a, hipStream_t s);     // few rows: whole K per workgroup, row scales found in-kernel
// lock-step s of the AoA decoder relevance fused into that GEMM (dense_f16x3.hip, FUSE): rows are (image, word) pairs, row = image * T + word
struct AoaStepFuse {
    int T = 0, s = 0;
    const int* tmax = nullptr;                                   // [rows] word index t of the row if its caption has that word, else -1
    const float *q1 = nullptr, *dg = nullptr;                    // [B][T][H]: i tanh(g) / z~(c next), z~(g)  (decoder_aoa.hip, aoa_rel_coef_kernel)
    float* A_next = nullptr;                                     // [rows][H] GEMM input of lock-step s + 1 (the OTHER buffer than `in`)
    float* r_glob = nullptr;                                     // [rows][H], accumulated
    float* wpart = nullptr;                                      // [rows][T][4] partial sums of r_words
};
int launch_dense_small_f16x3_aoa_step(const ConvArgs& a, const AoaStepFuse& fz, hipStream_t s);
int launch_dense_ks_aoa_step(const ConvArgs& a, const AoaStepFuse& fz, hipStream_t s);      // dense_small.hip: the same step on the fp32 MFMA (exact modes)

// few-row dense GEMMs (dense_small.hip)
bool dense_small_fits(const ConvArgs& a);
int launch_dense_small(const ConvArgs& a, hipStream_t s);

// host-side entry used by the C ABI and by the VGG16 / decoder chains (conv_dispatch.hip): conv_select, then the launch
int conv_dispatch(const lrpx_conv_desc* d, hipStream_t stream, int f16_ksplit = 1);

}  // namespace lrpx
