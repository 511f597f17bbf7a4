// The VGG16 encoder chains (forward trace, LRP relevance, image gradients) of liblrpx; their convs go through conv_dispatch.hip.
//
// Reference behaviour reproduced (paths relative to the reference repo):
//   forward  : models/gridTDmodel.py:40-43 Encoder.forward over vgg16.features[0:-1] (models/vgg.py:62-81)
//              + LRPtools/lrp_wrapper.py:24-25 save_input_hook (every leaf keeps its input)
//   relevance: LRPtools/lrp_wrapper.py:63-87 compute_lrp -> per leaf, in reverse order,
//              Conv2d alpha1beta0 (lrp_modules.py:124-150), ReLU identity (:42-46), MaxPool2d (:182-195)
#include <atomic>
#include <cstdlib>

#include "conv_launch.h"
#include "conv_f16x3.h"
#include "blocked.h"

namespace lrpx {

// ------------------------------------------------------------------------------------------------
// VGG16 geometry (cfg 'D' without the last pool)
// ------------------------------------------------------------------------------------------------
struct VggLayer { int conv; int hw; int cin; int cout; };   // conv: 1 conv3x3, 0 maxpool; hw = input size
static constexpr VggLayer kVgg[17] = {
    {1, 224, 3, 64},   {1, 224, 64, 64},   {0, 224, 64, 64},
    {1, 112, 64, 128}, {1, 112, 128, 128}, {0, 112, 128, 128},
    {1, 56, 128, 256}, {1, 56, 256, 256},  {1, 56, 256, 256}, {0, 56, 256, 256},
    {1, 28, 256, 512}, {1, 28, 512, 512},  {1, 28, 512, 512}, {0, 28, 512, 512},
    {1, 14, 512, 512}, {1, 14, 512, 512},  {1, 14, 512, 512}};
static const int kNL = 17;
static inline int cin_pad(int l) { return l == 0 ? 8 : kVgg[l].cin; }   // image is kept NHWC with 8 channels

// K ranges per tile of a forward-trace conv on the split-product kernels: a property of the LAYER (its map size) and of the
// arithmetic, never of the batch size - an image gets the same activations, pool winners and maps whatever batch it sits in
// (test_forward_features_vs_fp64_...).
//  * 14 x 14, both arithmetics: 8.  The grid fills the chip: 16 images are 112 workgroups of 32 K-chunks each (207 -> 112 + 45 us
//    per layer); an accumulator carries 36 k-steps instead of 288.  A chain of N MFMA accumulations rounds like a sequential
//    fp32 sum (tools/micro/mfma_round.hip, profiles/r03_mfma_round.txt: rms 3.6e-7 of the result at N = 288, 6.5e-8 in 8
//    blocks): f16x3 features 2.9e-6 -> 2.0e-6 of their maximum from an fp64 forward.
//  * f16x3, 28 x 28: unsplit.  Four ranges give features 1.6e-6 from fp64, but their partial sums are 4 x 51 MB per layer and 16
//    images: +0.3 ms per forward pass for a gain that no parity test can see (the AoA r_words rows sit at 1.0 - 1.2 of the
//    reference's own fp64 distance either way, bound 3).
//  * exact bf16 splits (bf16x6), 28 x 28: 4 and 56 x 56: 2.  An accumulator of this kernel is rounded six times per k-step (six
//    MFMAs), against three on the fp16 split products: unsplit, the exact-split forward sits 2.7e-6 of the feature maximum from
//    an fp64 evaluation where the fp16 forward sits at 2.1e-6 and oneDNN at 7.6e-7 (tools/dbg/fwd_f64_probe.py), and one
//    well-conditioned r_words row of the T = 20 fixture left the 1e-5 bound (1.6e-5).  Partial sums over <= 72 k-steps, added
//    pairwise by fwd_dual_finish; +0.5 ms per 16 images.
static constexpr int fwd_ksplit(bool f16x3, bool bf16x6, int hw) {
    if (!f16x3 && !bf16x6) return 1;
    return hw == 14 ? 8 : (f16x3 ? 1 : (hw == 28 ? 4 : (hw == 56 ? 2 : 1)));
}
// every split divides the layer's K-chunks, and its partial sums fit the scratch region of the trace (xz[1]: 224 x 224 x 64 per image)
static constexpr bool fwd_ksplit_fits() {
    for (int l = 1; l < kNL; ++l)
        for (int f16 = 0; f16 < 2; ++f16) {
            const int ks = fwd_ksplit(f16, !f16, kVgg[l].hw);
            if (kVgg[l].conv && ks > 1 && ((kVgg[l].cin / 16) % ks != 0 || (long)ks * kVgg[l].hw * kVgg[l].hw * 2 * kVgg[l].cout > 224L * 224 * 64)) return false;
        }
    return true;
}
static_assert(fwd_ksplit_fits(), "forward K split: ranges must divide cin / 16 and the partial sums must fit the trace's scratch region");

int first_layer_pack(const float* w, float* w6, int cout, int plain, hipStream_t s);
int first_layer_relevance(const float* S, const float* w6, const float* X8, const int* map2img, float* out, int n_maps,
                          int cin, int plain, int s_chunked, hipStream_t s);
int fwd_dual_finish(const float* part, int nsplit, const float* bias, float* act, float* zpos, int n_img, long pix_per_img,
                    int cout, unsigned* amax, hipStream_t s);
int first_layer_pack_mfma(const float* w, float* packed, int plain, hipStream_t s);
int first_layer_relevance_mfma(const float* S, const float* packed, const float* X8, const int* map2img,
                               const unsigned* s_amax, float* out, int n_maps, int plain, int s_layout, hipStream_t s);

int guided_gate(const float* g, const float* y, const int* map2img, float* out, int n_maps, long per, int plain,
                hipStream_t s);
int rel_mul_finish(const float* part, int nsplit, const float* x, const int* map2img, float* out, int n_maps, long per_map, hipStream_t s);
int maxpool_guided_bwd(const float* x, const float* g_out, const int* map2img, float* g_in, int n_maps, int ho, int wo,
                       int c, int plain, unsigned* amax, hipStream_t s);

// PROCESS DEFAULTS of the matrix-core mode of the fused chains (lrpx_set_conv_mode: 0 fp32 MFMA, 1 bf16x6 (conv_bf16x6.h),
// 2 f16x3 (conv_f16x3.h), 3 = 2 with fp8 cross products in the relevance pass) and of the forward-trace switch
// (lrpx_set_forward_f16).  Atomics: a setter racing with a call on another thread yields one of the two values, never a
// torn one; callers that need a mode of their own pass it per call (lrpx_vgg16_opts, the *_ex entry points) and are not
// affected by the setters at all.
// Round 6: the process default is mode 1 - operands split EXACTLY into three bf16 parts (24 significand bits, fp32's exponent range),
// six products, fp32 accumulate: arithmetic no narrower than the reference's fp32 convolutions (LRPtools/lrp_modules.py:124-150,
// utils.py:21-31).  The faster modes 2 / 3 (fp16 split products behind per-map power-of-two scales; 22 / ~15 effective operand bits)
// meet the 1e-4 contract on every tested input but are OPT-IN: lrpx_set_conv_mode, lrpx_vgg16_opts.conv_mode, or LRPX_CONV_MODE in the
// environment (read once, at load).
static int initial_mode() {
    const char* v = getenv("LRPX_CONV_MODE");
    if (!v || !*v) return 1;
    const int m = atoi(v);
    return m < 0 ? 0 : (m > 3 ? 3 : m);
}
static std::atomic<int> g_default_mode{initial_mode()};
// Round 6: the forward trace runs on the EXACT kernels in every conv mode by default (fp32 MFMA for conv1_1, exact bf16 splits above).
// The fp16 split-product forward (one power-of-two scale per image: inputs more than ~2^29 below the image's maximum flush, a
// receptive field made of such inputs gets Z+ = 0 and its relevance is dropped where the reference redistributes it -
// tests/test_gpu_range.py) is an explicit opt-in: lrpx_set_forward_f16(1), lrpx_vgg16_opts.forward_f16, LRPX_FORWARD_F16=1.
static int initial_fwd_f16() {
    const char* v = getenv("LRPX_FORWARD_F16");
    return (v && *v) ? (atoi(v) ? 1 : 0) : 0;
}
static std::atomic<int> g_default_fwd_f16{initial_fwd_f16()};

// what one call runs with: resolved once at entry from its opts (or the process defaults)
struct VggCtx { int mode, fwd_f16; };
static VggCtx resolve_ctx(const lrpx_vgg16_opts* o) {
    VggCtx c;
    c.mode = (o && o->conv_mode >= 0) ? (o->conv_mode > 3 ? 3 : o->conv_mode) : g_default_mode.load(std::memory_order_relaxed);
    c.fwd_f16 = (o && o->forward_f16 >= 0) ? (o->forward_f16 ? 1 : 0) : g_default_fwd_f16.load(std::memory_order_relaxed);
    return c;
}

// legacy profiling switch (lrpx_vgg16_layer_timing): per THREAD, so that two host threads driving two streams never share
// an event table; it routes the thread's next plain lrpx_vgg16_relevance calls through opts.layer_ms
static thread_local int tl_timing = 0;
static thread_local float tl_ms[17];

// relevance convs that can run on conv_wino_b6.h: long K on 56 / 28 / 14-pixel maps, not under a pool (conv3_1/2, conv4_1/2, conv5_1/2/3)
static bool wino_layer(int l) {
    return l > 0 && kVgg[l].conv && kVgg[l].hw <= 56 && kVgg[l].cin % 64 == 0 && !(l + 1 < kNL && !kVgg[l + 1].conv);
}

// ---- the packed blob: ONE list of its regions, in blob order (a new pack is one line here) -----------------------
// vgg_packed_layout() and lrpx_vgg16_pack() both walk it; the chains address a region by its name and layer (VggPacked::at).
enum PackLayers { L_CONV, L_UPPER, L_WINO, L_ONCE };   // every conv; the convs above conv1_1; wino_layer(); once, filled with conv1_1
enum PackSrc { SRC_NONE, SRC_DUAL, SRC_SCALED, SRC_RAW, SRC_BIAS };   // the dual rows wd, the scaled rows wr, W itself (lrpx_vgg16_pack); the bias
// fp32 fragments (K-chunk of the layer: lrpx_conv_kc), bf16x3, f16x2, f16f8, Winograd bf16x3; the first layer's direct-conv weights and
// their matrix-core form; plain floats: `floats` of them, or one per output channel where that is 0.  X(name, layers, source, format, pack mode, floats)
enum PackFmt { FMT_FP32, FMT_BF16X3, FMT_F16X2, FMT_F16F8, FMT_WINO, FMT_FIRST_VALU, FMT_FIRST_MFMA, FMT_FLOATS };
#define LRPX_VGG_REGIONS(X)                                                                  \
    X(fwd, L_CONV, SRC_DUAL, FMT_FP32, LRPX_PACK_FWD, 0)                                     \
    X(bwd, L_CONV, SRC_SCALED, FMT_FP32, LRPX_PACK_BWD_POS, 0)                              /* conv1_1: LRPX_PACK_BWD_FIRST */ \
    X(bias, L_CONV, SRC_BIAS, FMT_FLOATS, 0, 0)                                              \
    X(bwdp, L_UPPER, SRC_RAW, FMT_FP32, LRPX_PACK_BWD_PLAIN, 0)                              \
    X(bwd6, L_UPPER, SRC_SCALED, FMT_BF16X3, LRPX_PACK_BWD_POS, 0)                           \
    X(bwdp6, L_UPPER, SRC_RAW, FMT_BF16X3, LRPX_PACK_BWD_PLAIN, 0)                           \
    X(bwdh, L_UPPER, SRC_SCALED, FMT_F16X2, LRPX_PACK_BWD_POS, 0)                            \
    X(fwdh, L_UPPER, SRC_DUAL, FMT_F16X2, LRPX_PACK_FWD, 0)                                  \
    X(bwdph, L_UPPER, SRC_RAW, FMT_F16X2, LRPX_PACK_BWD_PLAIN, 0)                            \
    X(bwd8, L_UPPER, SRC_SCALED, FMT_F16F8, LRPX_PACK_BWD_POS, 0)                            \
    X(bwdp8, L_UPPER, SRC_RAW, FMT_F16F8, LRPX_PACK_BWD_PLAIN, 0)                            \
    X(fwd6, L_UPPER, SRC_DUAL, FMT_BF16X3, LRPX_PACK_FWD, 0)                                 \
    X(fwdh0, L_ONCE, SRC_DUAL, FMT_F16X2, LRPX_PACK_FWD, 0)                                 /* conv1_1 forward on the fp16 matrix cores */ \
    X(first6, L_ONCE, SRC_SCALED, FMT_FIRST_VALU, LRPX_PACK_BWD_POS, 64 * 9 * 6)            /* direct-conv weights of the first layer's rule */ \
    X(first6p, L_ONCE, SRC_RAW, FMT_FIRST_VALU, LRPX_PACK_BWD_PLAIN, 64 * 9 * 6)            /* ... and of its plain transposed conv (guided backprop) */ \
    X(first16, L_ONCE, SRC_SCALED, FMT_FIRST_MFMA, LRPX_PACK_BWD_POS, 16 + 2 * 9 * 64 * 4)  /* first layer's rule on the matrix cores (header + A fragments) */ \
    X(first16p, L_ONCE, SRC_RAW, FMT_FIRST_MFMA, LRPX_PACK_BWD_PLAIN, 16 + 2 * 9 * 64 * 4)  /* ... and its plain transposed conv */ \
    X(chs, L_CONV, SRC_NONE, FMT_FLOATS, 0, 0)                                              /* per-output-channel balance factors rs_l[c] of conv l (powers of two, see lrpx_vgg16_pack) */ \
    X(spread, L_ONCE, SRC_NONE, FMT_FLOATS, 0, 32)                                          /* [17] per conv layer: largest ratio of row maxima max|W[c,:]| inside one 16-row K slice (lrpx_vgg16_row_spread) */ \
    X(bwdw6, L_WINO, SRC_SCALED, FMT_WINO, LRPX_PACK_BWD_POS, 0)                            /* Winograd F(2x2,3x3) form of bwd6 (lrpx_pack_weights_wino_b6) */ \
    X(scratch, L_ONCE, SRC_NONE, FMT_FLOATS, 0, 512 * 512 * 9 * 3)                          /* scaled weight copies while packing: cout*cin*9 + 2*cout*2*cin*9 floats of the largest layer */
#define X(name, ...) R_##name,
enum PackId { LRPX_VGG_REGIONS(X) R_COUNT };
#undef X
#define X(name, ...) {__VA_ARGS__},
static constexpr struct PackRegion { int layers, src, fmt, mode; size_t floats; } kRegions[R_COUNT] = {LRPX_VGG_REGIONS(X)};
#undef X

static bool region_has(const PackRegion& r, int l) {
    return r.layers == L_ONCE ? l == 0 : (r.layers == L_WINO ? wino_layer(l) : (kVgg[l].conv && (l > 0 || r.layers == L_CONV)));
}
// The floats that region r takes for layer l and, with a destination, its pack from `src` (status in *rc): each format's size formula
// next to its packer.  A weight pack feeds a GEMM of n_oc output channels over k from a source matrix of rows x cols x 9 taps: the conv
// (LRPX_PACK_FWD) or its transpose.  conv1_1: its image is [x+ | x-] in 8 channels (one 16-channel K-chunk on the fp16 matrix cores), its
// transposed conv is padded to 32 output channels and takes LRPX_PACK_BWD_FIRST
static size_t region_floats(const PackRegion& r, int l, const float* src = nullptr, float* dst = nullptr, void* stream = nullptr, int* rc = nullptr) {
    const VggLayer& L = kVgg[l];
    const bool fwd = r.mode == LRPX_PACK_FWD, plain = r.mode == LRPX_PACK_BWD_PLAIN;
    const int n_oc = fwd ? 2 * L.cout : (l > 0 ? L.cin : 32), k = !fwd ? L.cout : (l > 0 ? L.cin : (r.fmt == FMT_FP32 ? cin_pad(0) : 16));
    const int rows = fwd ? 2 * L.cout : L.cout, cols = (fwd && l == 0) ? 2 * L.cin : L.cin, kc = lrpx_conv_kc(L.hw, 9, k);
    const size_t plain_floats = r.floats ? r.floats : (size_t)L.cout;
    switch (r.fmt) {
        case FMT_FP32: if (dst) *rc = lrpx_pack_weights(src, rows, cols, 9, (l == 0 && !fwd && !plain) ? LRPX_PACK_BWD_FIRST : r.mode, kc, dst, stream);
            return lrpx_packed_floats(n_oc, k, 9, kc);
        case FMT_BF16X3: if (dst) *rc = lrpx_pack_weights_bf16x3(src, rows, cols, 9, r.mode, dst, stream);
            return lrpx_packed_bf16x3_bytes(n_oc, k, 9) / sizeof(float);
        case FMT_F16X2: if (dst) *rc = lrpx_pack_weights_f16x2(src, rows, cols, 9, r.mode, dst, stream);
            return lrpx_packed_f16x2_bytes(n_oc, k, 9) / sizeof(float);
        case FMT_F16F8: if (dst) *rc = lrpx_pack_weights_f16f8(src, rows, cols, r.mode, dst, stream);
            return lrpx_packed_f16f8_bytes(n_oc, k) / sizeof(float);
        case FMT_WINO: if (dst) *rc = lrpx_pack_weights_wino_b6(src, rows, cols, r.mode, dst, stream);
            return lrpx_packed_wino_b6_bytes(n_oc, k) / sizeof(float);
        case FMT_FIRST_VALU: if (dst) *rc = first_layer_pack(src, dst, L.cout, plain, (hipStream_t)stream); return r.floats;
        case FMT_FIRST_MFMA: if (dst) *rc = first_layer_pack_mfma(src, dst, plain, (hipStream_t)stream); return r.floats;
        default:      // (of the sources, only the bias is copied as it is)
            if (dst && hipMemcpyAsync(dst, src, plain_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
                set_error("vgg16_pack: bias copy failed");
                *rc = LRPX_ELAUNCH;
            }
            return plain_floats;
    }
}

struct VggPacked {   // offsets in floats into the packed blob (0: the layer has no such region)
    size_t off[R_COUNT][17], total;
    size_t at(int region, int l = 0) const { return off[region][l]; }
};
// regions that follow each other in the list and are not L_ONCE lie layer by layer: [fwd .. fwd6] of conv1_1, of conv1_2, ...
static VggPacked make_packed_layout() {
    VggPacked p = {};
    size_t off = 0;
    for (int r = 0, end; r < R_COUNT; r = end) {
        for (end = r + 1; kRegions[r].layers != L_ONCE && end < R_COUNT && kRegions[end].layers != L_ONCE;) ++end;
        for (int l = 0; l < kNL; ++l)
            for (int e = r; e < end; ++e)
                if (region_has(kRegions[e], l)) { p.off[e][l] = off; off += region_floats(kRegions[e], l); }
    }
    p.total = off;
    return p;
}
static const VggPacked& vgg_packed_layout() { static const VggPacked p = make_packed_layout(); return p; }   // (once: every chain call asks for it)

// ---- what a conv mode is to the chains: one row per resolved mode (a new arithmetic is one row here) ----------
struct ConvArith { int f16x3, bf16x6, pack; };   // lrpx_conv_desc.f16x3 / .bf16x6 and the region that holds the weights
struct ModeRow {
    ConvArith rel, plain, fwd;   // the relevance convs (rows rs W+), the plain transposed convs of the image-gradient chains (W itself), the exact forward
    bool amax;         // operands sit behind per-map power-of-two scales: max|S| words per (layer, map) behind the R buffer
    bool blocked;      // every S tensor of the relevance chain and the multiplicands are BLOCKED (blocked.h), the kernels accumulate channels x pixels
    bool fused;        // relevance: the fused flow (relevance_fused), else round 1's (relevance_rel)
    bool lowres;       // gradient chains: a conv under a pool takes the gradient at the pool's OUTPUT resolution (vgg16_backprop), else a pool-backward kernel
    bool first_mfma;   // conv1_1 on the matrix cores (S in 32-channel chunks), else the direct fp32 VALU conv (16-channel chunks): Chain::first_layer
};
static constexpr ModeRow kModes[4] = {
    {{0, 0, R_bwd}, {0, 0, R_bwdp}, {0, 0, R_fwd}, false, false, false, false, false},      // 0: fp32 MFMA
    // 1 (round 6): exact bf16 splits on the conv_f16x3.h tiling (B6): no operand scales, hence no amax words; pools folded into the staging as in mode 3
    {{0, 1, R_bwd6}, {0, 1, R_bwdp6}, {0, 1, R_fwd6}, false, false, true, true, false},
    {{1, 0, R_bwdh}, {1, 0, R_bwdph}, {0, 1, R_fwd6}, true, false, true, false, true},      // 2: fp16 split products
    {{2, 0, R_bwd8}, {2, 0, R_bwdp8}, {0, 1, R_fwd6}, true, true, true, true, true},        // 3: ... with the cross products on the fp8 matrix cores
};
// the forward trace runs on the EXACT kernels (fp32 MFMA for conv1_1; above it the mode's, round 6: conv1_2 too) unless forward_f16
// comes with mode 2 / 3: the fp16 split products then, conv1_1 included
static ConvArith fwd_arith(const VggCtx& cx, int l) {
    if (cx.fwd_f16 && cx.mode >= 2) return {1, 0, l > 0 ? R_fwdh : R_fwdh0};
    return l > 0 ? kModes[cx.mode].fwd : kModes[0].fwd;
}

// ---- channel balance of the Z+ / relevance side (round 5) ----------------------------------------------------------------------
// The relevance step of conv l contracts over ITS output channels c:  R_in[i] = x_i * sum_{c,taps} S_c W+[c,i],  S_c = R_c / Z+_c
// (LRPtools/lrp_modules.py:124-150, utils.py:16-31).  A channel whose weights are small against its bias - common in trained
// networks: models/vgg.py:86-94 loads pretrained weights - has activations ~ b_c but Z+_c ~ |W_c|: S_c ~ 1/|W_c| is huge exactly
// where W+[c,:] is tiny.  In fp32 (the reference) the product is harmless; operands split into fp16 halves behind ONE scale per map
// / per layer hold ~2^17 of range at full precision, and the huge S planes push every ordinary entry out of it (measured: 7e-2 of
// max|R| on a chain with log-normal channel scales, tests/test_gpu_vgg.py::test_chain_hostile_weights_all_modes).
// Cure, exact in every mode: the Z+ half of the forward weights and every alpha1beta0 relevance pack carry row c multiplied by
//     rs_l[c] = 2^(e_max - e_c),   e_c = floor(log2 max_{i,taps} W+[c,i])   (first layer: max |W|; a row without positive
// weights: 1).  The trace then holds Z'_c = rs_c Z+_c, every S the chain forms is S'_c = S_c / rs_c, and S'_c (rs_c W+[c,i]) is
// the reference's product bit for bit (powers of two).  Where Z+ == 0 the reference divides by 1e-7 (utils.py:16-18); there every
// product x_i W+[c,i] of the window is zero, so the value of S at such a pixel never reaches R_in, scaled or not.
// one workgroup per weight row: m[c] = max over the row of w+ (first layer: |w|), ma[c] = max |w|   (coalesced; a lone thread per row
// walking 4 608 strided floats took 0.6 ms per layer)
__global__ __launch_bounds__(256) void row_max_kernel(const float* __restrict__ w, int per_row, int use_abs, float* __restrict__ m_out,
                                                      float* __restrict__ ma_out) {
    __shared__ float r1[4], r2[4];
    const int c = blockIdx.x;
    float m = 0.f, ma = 0.f;
    for (int j = threadIdx.x; j < per_row; j += 256) {
        const float x = w[(long)c * per_row + j];
        m = fmaxf(m, use_abs ? fabsf(x) : fmaxf(x, 0.f));
        ma = fmaxf(ma, fabsf(x));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); ma = fmaxf(ma, __shfl_xor(ma, o, 64)); }
    if ((threadIdx.x & 63) == 0) { r1[threadIdx.x >> 6] = m; r2[threadIdx.x >> 6] = ma; }
    __syncthreads();
    if (threadIdx.x == 0) {
        m_out[c] = fmaxf(fmaxf(r1[0], r1[1]), fmaxf(r1[2], r1[3]));
        ma_out[c] = fmaxf(fmaxf(r2[0], r2[1]), fmaxf(r2[2], r2[3]));
    }
}

// rs[c] = 2^(e_max - e_c) from the row maxima; spread = the largest ratio of |w| row maxima inside one 16-row K slice
__global__ __launch_bounds__(512) void row_scale_kernel(const float* __restrict__ m_in, const float* __restrict__ ma_in, int cout,
                                                        float* __restrict__ rs, float* __restrict__ spread) {
    __shared__ float sh[512];
    __shared__ float sa[512];
    const int c = threadIdx.x;
    const float m = c < cout ? m_in[c] : 0.f;
    // spread of the PLAIN weights' row maxima inside a 16-row K slice (the block the fp6 cross-term operands share one scale over):
    // what the image-gradient chains' mode-3 kernels are sensitive to (they multiply with W itself, rows unbalanced)
    sa[c] = c < cout ? ma_in[c] : 0.f;
    __syncthreads();
    if (c == 0) {
        float worst = 1.f;
        for (int g0 = 0; g0 < cout; g0 += 16) {
            float hi = 0.f, lo = 3.0e38f;
            for (int k = g0; k < min(g0 + 16, cout); ++k) { hi = fmaxf(hi, sa[k]); if (sa[k] > 0.f) lo = fminf(lo, sa[k]); }
            if (hi > 0.f && lo < 3.0e38f) worst = fmaxf(worst, hi / lo);
        }
        *spread = worst;
    }
    __syncthreads();
    // d = 2^floor(log2 m) for a normal m (the exponent field alone); 0 for rows without a usable weight
    const unsigned eb = __float_as_uint(m) & 0x7f800000u;
    const float d = (eb != 0u && eb != 0x7f800000u) ? __uint_as_float(eb) : 0.f;
    sh[c] = c < cout ? d : 0.f;
    __syncthreads();
    for (int o = 256; o > 0; o >>= 1) {
        if (c < o) sh[c] = fmaxf(sh[c], sh[c + o]);
        __syncthreads();
    }
    const float dmax = sh[0];
    if (c < cout) rs[c] = (d > 0.f && dmax > 0.f) ? dmax / d : 1.f;
}

__global__ void scale_rows_kernel(const float* __restrict__ w, const float* __restrict__ rs, float* __restrict__ wr,
                                  int per_row, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < total) wr[idx] = w[idx] * rs[idx / per_row];
}

// wd (2 cout, cin2, 9): rows [0, cout) = W (the activation half), rows [cout, 2 cout) = the Z half, rs_c W+ (first layer, cin2 =
// 2 cin, input channels [x+ | x-]: [W | W] above, [rs W+ | rs W-] below) - packed with LRPX_PACK_FWD this is the LRPX_PACK_FWD_DUAL
// (_FIRST) layout with the balanced Z half
__global__ void dual_rows_kernel(const float* __restrict__ w, const float* __restrict__ rs, float* __restrict__ wd, int cout,
                                 int cin, int first, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cin2 = first ? 2 * cin : cin;
    const int t = idx % 9;
    const int ci2 = (idx / 9) % cin2;
    const int oc = idx / (9L * cin2);
    const int co = oc < cout ? oc : oc - cout, ci = ci2 < cin ? ci2 : ci2 - cin;
    float x = w[((long)co * cin + ci) * 9 + t];
    if (oc >= cout) {
        x *= rs[co];
        x = (!first || ci2 < cin) ? fmaxf(x, 0.f) : fminf(x, 0.f);
    }
    wd[idx] = x;
}

struct VggTrace {   // offsets in floats; act[l] = input of layer l, act[17] = encoder output
    size_t act[18], zpos[17], xz[17], xzp[17], am[17], famax, total;   // famax: [18][n_img] max of act[l] per image (f16x3 forward)
    // xz[l]: multiplicand of conv l's fused relevance step = act[l] / safe(Z+ of the conv below): directly below
    //        (zpos[l-1]) or under a pool (zpos[l-2] at the window's winner, lrpx_pool_winner);
    //        xz[1] (n_img x 224*224*64 floats, the largest) doubles as the SCRATCH of the K-split forward layers while
    //        lrpx_vgg16_forward runs: the xz tensors are only valid after lrpx_vgg16_trace_derive, its last step;
    // xzp[l]: the same multiplicand in the BLOCKED layout (blocked.h; one block set per image) for the mode-3 kernels;
    // am[lp]: winner positions of pool lp (bytes, stored in a float-aligned region)
};
static VggTrace vgg_trace_layout(int n_img) {
    VggTrace t;
    size_t off = 0;
    for (int l = 0; l <= kNL; ++l) {
        int hw, c;
        if (l < kNL) { hw = kVgg[l].hw; c = cin_pad(l); }
        else { hw = 14; c = 512; }
        t.act[l] = off;
        off += (size_t)n_img * hw * hw * c;
    }
    for (int l = 0; l < kNL; ++l) {
        t.zpos[l] = off;
        if (kVgg[l].conv) off += (size_t)n_img * kVgg[l].hw * kVgg[l].hw * kVgg[l].cout;
    }
    for (int l = 0; l < kNL; ++l) {
        t.xz[l] = t.xzp[l] = t.am[l] = 0;
        if (l >= 1 && kVgg[l].conv) {
            t.xz[l] = off;
            off += (size_t)n_img * kVgg[l].hw * kVgg[l].hw * kVgg[l].cin;
            t.xzp[l] = off;
            if (l >= 3) off += (size_t)n_img * (size_t)blk_floats((long)kVgg[l].hw * kVgg[l].hw, kVgg[l].cin);
        }
        if (!kVgg[l].conv) {
            t.am[l] = off;
            off += ((size_t)n_img * (kVgg[l].hw / 2) * (kVgg[l].hw / 2) * kVgg[l].cin + 3) / 4;
        }
    }
    t.famax = off;
    off += (size_t)18 * n_img;
    t.total = off;
    return t;
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

int lrpx_set_bf16x6(int enable) {
    if (enable >= 0) return g_default_mode.exchange(enable ? 1 : 0) >= 1;
    return g_default_mode.load() >= 1;
}

int lrpx_set_forward_f16(int enable) {
    if (enable >= 0) return g_default_fwd_f16.exchange(enable ? 1 : 0);
    return g_default_fwd_f16.load();
}

int lrpx_set_conv_mode(int mode) {
    if (mode >= 0) return g_default_mode.exchange(mode > 3 ? 3 : mode);
    return g_default_mode.load();
}

int lrpx_vgg16_resolve_opts(const lrpx_vgg16_opts* opts, int* conv_mode, int* forward_f16) {
    const VggCtx c = resolve_ctx(opts);
    if (conv_mode) *conv_mode = c.mode;
    if (forward_f16) *forward_f16 = c.fwd_f16;
    return LRPX_OK;
}

size_t lrpx_vgg16_packed_bytes(void) { return vgg_packed_layout().total * sizeof(float); }
size_t lrpx_vgg16_trace_bytes(int n_img) { return vgg_trace_layout(n_img).total * sizeof(float); }
size_t lrpx_vgg16_workspace_bytes(int n_maps) {
    // two ping-pong S buffers (largest: 224*224*64 per map) + one R buffer in front of a pool (112*112*64)
    // + per-(layer, map) max|S| words of the f16x3 relevance pass
    return ((size_t)2 * 224 * 224 * 64 + (size_t)112 * 112 * 64 + 32) * (size_t)n_maps * sizeof(float);
}

int lrpx_vgg16_pack(const float* const* w, const float* const* b, void* packed, void* stream) {
    LRPX_REQUIRE(w && b && packed, "vgg16_pack: null pointer");
    LRPX_CHECK_PTRS("lrpx_vgg16_pack", {packed, "packed"});
    for (int i = 0; i < 13; ++i) LRPX_CHECK_PTRS("lrpx_vgg16_pack", {w[i], "w[i]"}, {b[i], "b[i]"});
    const VggPacked& p = vgg_packed_layout();
    float* base = (float*)packed;
    int ci = 0;
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < kNL; ++l) {
        if (!kVgg[l].conv) continue;
        const VggLayer& L = kVgg[l];
        LRPX_REQUIRE(w[ci] && b[ci], "vgg16_pack: null weight %d", ci);
        // channel balance (see row_scale_kernel): rs, wr = rs W (every row), wd = [W ; rs W+] for the forward packs
        float* rs = base + p.at(R_chs, l);
        float* wr = base + p.at(R_scratch);
        float* wd = wr + (size_t)L.cout * L.cin * 9;
        const int first = l == 0, cin2 = first ? 2 * L.cin : L.cin;
        float* rmax = wr;                                    // (row maxima: 2 x cout floats at the head of the scratch, consumed before wr is written)
        hipLaunchKernelGGL(row_max_kernel, dim3(L.cout), dim3(256), 0, st, w[ci], L.cin * 9, first, rmax, rmax + L.cout);
        LRPX_TRY(check_launch("vgg16_pack: row maxima"));
        hipLaunchKernelGGL(row_scale_kernel, dim3(1), dim3(512), 0, st, rmax, rmax + L.cout, L.cout, rs, base + p.at(R_spread) + l);
        LRPX_TRY(check_launch("vgg16_pack: row scales"));
        const long n_w = (long)L.cout * L.cin * 9, n_d = (long)2 * L.cout * cin2 * 9;
        hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((n_w + 255) / 256)), dim3(256), 0, st, w[ci], rs, wr, L.cin * 9, n_w);
        LRPX_TRY(check_launch("vgg16_pack: scaled rows"));
        hipLaunchKernelGGL(dual_rows_kernel, dim3((unsigned)((n_d + 255) / 256)), dim3(256), 0, st, w[ci], rs, wd, L.cout, L.cin, first, n_d);
        LRPX_TRY(check_launch("vgg16_pack: dual rows"));
        // every region of this layer that has a source, in list order: they write disjoint parts of the blob from sources that are complete by now
        // (SRC_RAW: the image-gradient chains - guided backprop, plain gradient - take W itself)
        const float* srcs[] = {nullptr, wd, wr, w[ci], b[ci]};
        for (int r = 0, rc = LRPX_OK; r < R_COUNT; ++r)
            if (kRegions[r].src != SRC_NONE && region_has(kRegions[r], l)) { region_floats(kRegions[r], l, srcs[kRegions[r].src], base + p.at(r, l), stream, &rc); LRPX_TRY(rc); }
        ++ci;
    }
    return LRPX_OK;
}

// pools_done: the forward pass already wrote the pooled multiplicands (its pools run pool_winner_blk, which reads the activations once
// for the pooled activations, the winners and the multiplicand - see lrpx_vgg16_forward_ex)
static int trace_derive_impl(void* trace, int n_img, void* stream, bool pools_done) {
    LRPX_REQUIRE(trace && n_img > 0, "vgg16_trace_derive: bad arguments");
    const VggTrace t = vgg_trace_layout(n_img);
    float* tr = (float*)trace;
    for (int l = 1; l < kNL; ++l) {
        if (!t.xz[l]) continue;
        if (pools_done && !kVgg[l - 1].conv) continue;
        // l >= 3: the blocked copy the mode-3 relevance kernels multiply with (one block set per image) is written in the same pass
        // (conv1_2's kernel takes NHWC)
        const int pix = kVgg[l].hw * kVgg[l].hw;
        if (kVgg[l - 1].conv) {
            // multiplicand of the fused step  S_{l-1} = x_l * convT(S_l, W+) / safe(Z+_{l-1})   (lrp_modules.py:124-150
            // for conv l, then utils.py:16-18 safe_divide of the conv below)
            if (l >= 3)
                LRPX_TRY(divide_safe_blk(tr + t.act[l], tr + t.zpos[l - 1], tr + t.xz[l], tr + t.xzp[l], n_img, pix, kVgg[l].cin, (hipStream_t)stream));
            else
                LRPX_TRY(divide_stab_amax(tr + t.act[l], tr + t.zpos[l - 1], nullptr, tr + t.xz[l], n_img, (long)pix * kVgg[l].cin, STAB_SAFE0, nullptr, (hipStream_t)stream));
        } else {
            // a pool lies below: max / safe(Z+_{l-2} at the winner) + the winner positions (lrp_modules.py:182-195)
            LRPX_TRY(pool_winner_blk(tr + t.act[l - 1], tr + t.zpos[l - 2], tr + t.xz[l], (uint8_t*)(tr + t.am[l - 1]), tr + t.xzp[l],
                                     n_img, kVgg[l].hw, kVgg[l].hw, kVgg[l].cin, (hipStream_t)stream));
        }
    }
    return LRPX_OK;
}

int lrpx_vgg16_trace_derive(void* trace, int n_img, void* stream) {
    LRPX_CHECK_PTRS("lrpx_vgg16_trace_derive", {trace, "trace"});
    return trace_derive_impl(trace, n_img, stream, false);
}

int lrpx_vgg16_trace_layout(int n_img, size_t* act_off, size_t* zpos_off) {
    LRPX_REQUIRE(n_img > 0 && act_off && zpos_off, "vgg16_trace_layout: bad arguments");
    const VggTrace t = vgg_trace_layout(n_img);
    for (int l = 0; l <= kNL; ++l) act_off[l] = t.act[l];
    for (int l = 0; l < kNL; ++l) zpos_off[l] = kVgg[l].conv ? t.zpos[l] : 0;
    return LRPX_OK;
}

const float* lrpx_vgg16_trace_features(const void* trace, int n_img) {
    return (const float*)trace + vgg_trace_layout(n_img).act[kNL];
}

const float* lrpx_vgg16_row_spread(const void* packed) {
    return packed ? (const float*)packed + vgg_packed_layout().at(R_spread) : nullptr;
}

const float* lrpx_vgg16_channel_scales(const void* packed, int layer, int* n_channels) {
    if (!packed || layer < 0 || layer >= kNL || !kVgg[layer].conv) return nullptr;
    if (n_channels) *n_channels = kVgg[layer].cout;
    return (const float*)packed + vgg_packed_layout().at(R_chs, layer);
}

int lrpx_vgg16_forward(const void* packed, const float* img_nchw, int n_img, void* trace, float* feat_nhwc,
                       void* stream) {
    return lrpx_vgg16_forward_ex(packed, img_nchw, n_img, trace, feat_nhwc, nullptr, stream);
}

int lrpx_vgg16_forward_ex(const void* packed, const float* img_nchw, int n_img, void* trace, float* feat_nhwc,
                          const lrpx_vgg16_opts* opts, void* stream) {
    LRPX_CHECK_PTRS("lrpx_vgg16_forward_ex", {packed, "packed"}, {img_nchw, "img_nchw"}, {trace, "trace"}, {feat_nhwc, "feat_nhwc"});
    LRPX_REQUIRE(packed && img_nchw && trace && n_img > 0, "vgg16_forward: bad arguments");
    const VggCtx cx = resolve_ctx(opts);      // this call's values
    const bool f16 = fwd_arith(cx, 0).f16x3;
    const VggPacked& p = vgg_packed_layout();
    const VggTrace t = vgg_trace_layout(n_img);
    const float* pk = (const float*)packed;
    float* tr = (float*)trace;
    // fp16 split products (conv_f16x3.h): operand scale = max of the layer input per image
    unsigned* fam = reinterpret_cast<unsigned*>(tr + t.famax);
    if (f16) LRPX_TRY(clear_async(fam, (size_t)18 * n_img * sizeof(unsigned), (hipStream_t)stream));
    // the signed image is kept split into x+ / x- (channels 0-2 / 3-5 of 8): Z of the first conv needs both
    LRPX_TRY(lrpx_nchw_to_nhwc_posneg(img_nchw, tr + t.act[0], n_img, 3, 224 * 224, 8, stream));
    bool pools_fused = false, pools_plain = false;
    for (int l = 0; l < kNL; ++l) {
        const VggLayer& L = kVgg[l];
        if (L.conv) {
            const ConvArith a = fwd_arith(cx, l);
            lrpx_conv_desc d = {};
            d.in = tr + t.act[l]; d.wpacked = pk + p.at(a.pack, l); d.f16x3 = a.f16x3; d.bf16x6 = a.bf16x6;
            d.n_maps = n_img; d.hw = L.hw; d.cin = cin_pad(l); d.n_oc = 2 * L.cout; d.taps = 9;
            d.epi = EPI_FWD_DUAL; d.oc_split = L.cout; d.bias = pk + p.at(R_bias, l);
            d.out0 = tr + t.act[l + 1]; d.out1 = tr + t.zpos[l];
            if (f16) {
                // a max-pool keeps the maximum of its input; the epilogue records the per-image maximum of the activations, the next conv's scale
                d.in_amax = fam + (size_t)((l == 0 || kVgg[l - 1].conv) ? l : l - 1) * n_img;
                d.out0_amax = fam + (size_t)(l + 1) * n_img;
            }
            if (f16 && l == 0) {
                // conv1_1 on the fp16 matrix cores too (the fp32 MFMA kernel: 0.67 ms per 16 images for 15 GFLOP and 0.4 GB -
                // neither its matrix nor its memory time): the signed image [x+ | x- | 0] padded to one 16-channel
                // K-chunk (51 MB per 16 images, in the scratch region of the trace), scale = max|pixel| per image
                float* img16 = tr + t.xz[1];
                LRPX_TRY(lrpx_nchw_to_nhwc_posneg(img_nchw, img16, n_img, 3, 224 * 224, 16, stream));
                LRPX_TRY(lrpx_amax_maps(img16, n_img, (long)224 * 224 * 16, fam, stream));
                d.in = img16; d.cin = 16;
            }
            const int fwd_ks = fwd_ksplit(d.f16x3, d.bf16x6, L.hw);
            if (fwd_ks > 1) {
                // K-SPLIT: blockIdx.y takes one of fwd_ks contiguous K ranges per tile through the PLAIN epilogue (partial sums behind
                // each other in the xz[1] region of the trace - SCRATCH during the forward pass: lrpx_vgg16_trace_derive below
                // rewrites it after the last layer), then one pass adds the splits pairwise in a fixed order, applies bias / ReLU
                // and (f16x3) records the per-image maximum: what the FWD_DUAL epilogue does.
                float* part = tr + t.xz[1];
                unsigned* act_amax = d.out0_amax;
                d.epi = EPI_PLAIN; d.bias = nullptr; d.oc_split = 2 * L.cout;
                d.out0 = part; d.out1 = nullptr; d.out0_amax = nullptr;
                LRPX_TRY(conv_dispatch(&d, (hipStream_t)stream, fwd_ks));
                LRPX_TRY(fwd_dual_finish(part, fwd_ks, pk + p.at(R_bias, l), tr + t.act[l + 1], tr + t.zpos[l], n_img,
                                         (long)L.hw * L.hw, L.cout, act_amax, (hipStream_t)stream));
                continue;
            }
            LRPX_TRY(conv_dispatch(&d, (hipStream_t)stream));
        } else if (l >= 2 && l + 1 < kNL && t.xz[l + 1] && kVgg[l - 1].conv && L.cin % 16 == 0) {
            // a pool whose output a relevance layer multiplies with: ONE pass over the activations writes the pooled activations,
            // the winner positions and the multiplicand max / safe(Z+ at the winner) (NHWC + blocked) - what maxpool_fwd here and
            // pool_winner in lrpx_vgg16_trace_derive did in two (the larger tensor read twice: 4 x ~20 us per 16 images)
            LRPX_TRY(pool_winner_blk(tr + t.act[l], tr + t.zpos[l - 1], tr + t.xz[l + 1], (uint8_t*)(tr + t.am[l]), tr + t.xzp[l + 1],
                                     n_img, L.hw / 2, L.hw / 2, L.cin, (hipStream_t)stream, tr + t.act[l + 1]));
            pools_fused = true;
        } else {
            LRPX_TRY(lrpx_maxpool2x2_fwd(tr + t.act[l], tr + t.act[l + 1], n_img, L.hw, L.hw, L.cin, stream));
            pools_plain = true;
        }
    }
    LRPX_TRY(trace_derive_impl(trace, n_img, stream, pools_fused && !pools_plain));
    if (feat_nhwc) {
        if (hipMemcpyAsync(feat_nhwc, tr + t.act[kNL], (size_t)n_img * 196 * 512 * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
            set_error("vgg16_forward: feature copy failed");
            return LRPX_ELAUNCH;
        }
    }
    return LRPX_OK;
}

}  // extern "C"

// per-call HIP events around the conv launches of one relevance pass (opts.layer_ms)
struct LayerTimer {
    hipEvent_t ev[17][2];
    bool made = false, valid[17] = {};
    int begin() {
        for (auto& pair : ev)
            for (hipEvent_t& e : pair)
                if (hipEventCreate(&e) != hipSuccess) { set_error("vgg16_relevance: hipEventCreate failed"); return LRPX_ELAUNCH; }
        made = true;
        return LRPX_OK;
    }
    // the launches of layer l, between the layer's two events where begin() made them
    template <class F> int timed(int l, hipStream_t st, F launches) {
        if (made) (void)hipEventRecord(ev[l][0], st);
        LRPX_TRY(launches());
        if (made) { (void)hipEventRecord(ev[l][1], st); valid[l] = true; }
        return LRPX_OK;
    }
    // waits for the recorded events.  (Out of line, as it always was: the library's list of exported symbols has it.)
    __attribute__((noinline)) int finish(float* ms17) {
        int rc = LRPX_OK;
        for (int l = 0; l < 17; ++l) {
            ms17[l] = 0.f;
            if (valid[l] && (hipEventSynchronize(ev[l][1]) != hipSuccess || hipEventElapsedTime(&ms17[l], ev[l][0], ev[l][1]) != hipSuccess)) {
                set_error("vgg16_relevance: event query failed");
                rc = LRPX_ELAUNCH;
            }
        }
        return rc;
    }
    ~LayerTimer() {
        for (auto& pair : ev)
            for (hipEvent_t e : pair) if (made) (void)hipEventDestroy(e);
    }
};

// what the backward chains of one call work on
namespace {
struct Chain {
    const ModeRow& m;
    const VggPacked& p;
    const VggTrace t;
    const float *pk, *tr;      // the blob, the trace
    const int32_t* map2img;
    int n_img, n_maps;
    float *buf[2], *R;         // the workspace: two ping-pong buffers for S (the gradient), the R buffer in front of a pool and, behind it,
    unsigned* amax;            // in the modes with operand scales: amax[l * n_maps + n] = bits of the maximum over map n of the tensor
    hipStream_t st;            // that conv layer l consumes, recorded by whoever writes that tensor
    Chain(const lrpx_vgg16_opts* opts, const void* packed, const void* trace, int n_img_, const int32_t* map2img_, int n_maps_, void* workspace, void* stream)
        : m(kModes[resolve_ctx(opts).mode]), p(vgg_packed_layout()), t(vgg_trace_layout(n_img_)), pk((const float*)packed), tr((const float*)trace),
          map2img(map2img_), n_img(n_img_), n_maps(n_maps_), st((hipStream_t)stream) {
        const size_t sbuf = (size_t)224 * 224 * 64 * n_maps;
        buf[0] = (float*)workspace; buf[1] = buf[0] + sbuf; R = buf[0] + 2 * sbuf;
        amax = m.amax ? reinterpret_cast<unsigned*>(R + (size_t)112 * 112 * 64 * n_maps) : nullptr;
    }
    // the head of the descriptor of conv layer l's transposed conv on `in`.  unpool: under a pool, `in` is the low-resolution tensor that the
    // conv above the pool wrote, unpooled while staged
    lrpx_conv_desc desc(int l, const ConvArith& a, const float* in, bool unpool) const {
        const VggLayer& L = kVgg[l];
        lrpx_conv_desc d = {};
        d.in = in; d.wpacked = pk + p.at(a.pack, l); d.f16x3 = a.f16x3; d.bf16x6 = a.bf16x6;
        d.n_maps = n_maps; d.hw = L.hw; d.cin = L.cout; d.taps = 9; d.map2img = map2img; d.n_oc = L.cin; d.oc_split = L.cin;
        if (amax) d.in_amax = amax + (size_t)l * n_maps;
        // the maps of one image (the words of its caption) usually follow each other: tile-order hint for the
        // multiplicand reuse in L2 (a wrong guess only costs the reuse; the fp32 kernels take none)
        d.tile_group = (n_maps % n_img == 0) ? n_maps / n_img : 0;
        if (unpool && l + 1 < kNL && !kVgg[l + 1].conv) d.pool_am = (const uint8_t*)(tr + t.am[l + 1]);
        return d;
    }
    // conv1_1's step of a chain, 3 output channels (first_layer.hip): 16x16x32 MFMAs on the split halves of S in the split-product modes (S comes
    // with its per-map maximum), the direct fp32 VALU conv otherwise.  S of the fused relevance flow comes in channel chunks
    int first_layer(const float* S, float* out_nchw, int plain) const {      // plain: the transposed conv with W itself (the image-gradient chains)
        const int s_layout = (!plain && m.fused) ? 1 : 0;
        if (m.first_mfma)
            return first_layer_relevance_mfma(S, pk + p.at(plain ? R_first16p : R_first16), tr + t.act[0], map2img, amax, out_nchw, n_maps, plain, s_layout, st);
        return first_layer_relevance(S, pk + p.at(plain ? R_first6p : R_first6), tr + t.act[0], map2img, out_nchw, n_maps, kVgg[0].cout, plain, s_layout, st);
    }
};
}  // namespace

// Mode 0 keeps round 1's relevance flow: EPI_REL with the division in the epilogue + maxpool_relevance kernels
static int relevance_rel(const Chain& c, const float* r_feat_nhwc, float* out_nchw, LayerTimer& timer) {
    const VggTrace& t = c.t;
    int cur = 0, cur_chunked = 0;   // S[cur] is stored in K-chunks (written so by the pool kernel for the 224^2 / 112^2 layers)
    // S_16 = R_feat / safe(Z+_16)
    LRPX_TRY(divide_stab_amax(r_feat_nhwc, c.tr + t.zpos[16], c.map2img, c.buf[cur], c.n_maps, (long)196 * 512, STAB_SAFE, nullptr, c.st));
    for (int l = kNL - 1; l > 0; --l) {
        const VggLayer& L = kVgg[l];
        if (!L.conv) continue;   // pools are handled together with the conv above them
        lrpx_conv_desc d = c.desc(l, c.m.rel, c.buf[cur], false);
        d.epi = EPI_REL; d.x = c.tr + t.act[l]; d.in_chunked = cur_chunked;
        cur_chunked = 0;
        const bool pool_below = !kVgg[l - 1].conv;
        // ReLU passes relevance through (lrp_modules.py:42-46): fuse the next layer's S = R / safe(Z+)
        if (!pool_below) { d.out1 = c.buf[cur ^ 1]; d.zdiv = c.tr + t.zpos[l - 1]; d.stab = STAB_SAFE; }
        // a pool lies below: R at the pool output, then the Pool2d rule + division by Z+ of the conv under it
        else d.out0 = c.R;
        LRPX_TRY(timer.timed(l, c.st, [&] { return conv_dispatch(&d, c.st); }));
        if (pool_below) {
            // wide maps: hand the conv below its input in K-chunks (32-byte pixel slices would drag every 128-byte
            // line through the fabric four times: measured L2 hit 36 %, 3x the unique bytes on conv1_2)
            const int below_hw = 2 * L.hw;
            const int chunk = below_hw < 112 ? 0 : lrpx_conv_kc(below_hw, 9, L.cin);
            LRPX_TRY(maxpool_relevance_amax(c.tr + t.act[l - 1], c.R, c.tr + t.zpos[l - 2], c.map2img, nullptr, c.buf[cur ^ 1],
                                            c.n_maps, L.hw, L.hw, L.cin, chunk, nullptr, c.st));
            cur_chunked = chunk ? 1 : 0;
        }
        cur ^= 1;
    }
    return timer.timed(0, c.st, [&] { return c.first_layer(c.buf[cur], out_nchw, 0); });
}

// Modes 1 - 3 share the FUSED flow: REL_MUL epilogues on the precomputed multiplicands x / safe(Z+), convs under a pool unpool while they
// stage, no pool kernels, no unpooled tensors
static int relevance_fused(const Chain& c, const float* r_feat_nhwc, float* out_nchw, LayerTimer& timer) {
    const ModeRow& m = c.m;
    const VggTrace& t = c.t;
    int cur = 0, cur_chunked = 0;   // S[cur] is stored in K-chunks (conv2_2's output in the NHWC modes)
    if (c.amax) LRPX_TRY(clear_async(c.amax, (size_t)kNL * c.n_maps * sizeof(unsigned), c.st));
    // S_16 = R_feat / safe(Z+_16)
    if (m.blocked)
        LRPX_TRY(divide_stab_blocked(r_feat_nhwc, c.tr + t.zpos[16], c.map2img, c.buf[cur], c.n_maps, 196, 512, c.amax + (size_t)16 * c.n_maps, c.st));
    else
        LRPX_TRY(divide_stab_amax(r_feat_nhwc, c.tr + t.zpos[16], c.map2img, c.buf[cur], c.n_maps, (long)196 * 512, STAB_SAFE0,
                                  c.amax ? c.amax + (size_t)16 * c.n_maps : nullptr, c.st));
    for (int l = kNL - 1; l > 0; --l) {
        const VggLayer& L = kVgg[l];
        if (!L.conv) continue;   // pools are handled together with the conv above them
        lrpx_conv_desc d = c.desc(l, m.rel, c.buf[cur], true);
        d.epi = EPI_REL_MUL; d.in_chunked = cur_chunked;
        cur_chunked = 0;
        // x / safe(Z+) precomputed: of the conv below (ReLU passes relevance through, lrp_modules.py:42-46) or, where a pool lies below,
        // max / safe(Z+ at the winner), which turns the accumulator straight into S of the conv under the pool (at the winners).
        // blocked: in (1), x (2), out (4); conv1_2 (l == 1): blocked input only (see conv_f16x3.h, TR)
        d.x = c.tr + ((m.blocked && l != 1) ? t.xzp[l] : t.xz[l]); d.out1 = c.buf[cur ^ 1];
        if (m.blocked) d.blocked = l == 1 ? 1 : 7;
        if (c.amax) d.out1_amax = c.amax + (size_t)(kVgg[l - 1].conv ? l - 1 : l - 2) * c.n_maps;
        if (m.rel.bf16x6 && wino_layer(l)) d.wpacked_wino = c.pk + c.p.at(R_bwdw6, l);      // (used where lrpx_set_b6_wino / LRPX_B6_WINO has the bit of L.hw)
        // the first-layer kernel walks S in channel chunks (MFMA version: 32 = whole 128-byte lines per pixel; VALU: 16)
        if (l == 1) d.out_chunk = m.first_mfma ? 32 : 16;
        // conv2_2 -> conv2_1, NHWC: S in 16-channel chunks, the K-chunk of the consumer (64-byte slices of 512-byte NHWC pixels
        // drag every 128-byte line through the fabric twice: FETCH 3.1x the tensor; chunked: conv2_1 1.44 -> 1.37 ms)
        if (l == 4 && !m.blocked) { d.out_chunk = 16; cur_chunked = 1; }
        // (14 x 14 on the Winograd kernel: one launch of 8 x ceil(49 n_maps / 64) workgroups, no K split)
        constexpr int rel_ks = 2;
        static_assert((512 / 16) % rel_ks == 0, "the K ranges must divide the K-chunks of the 14 x 14 layers");
        if (m.rel.bf16x6 && L.hw == 14 && !(d.wpacked_wino && (b6_wino_bits() & 4))) {
            // the 14 x 14 relevance layers of mode 1 K-split in two: partial sums into the R buffer (unused in the fused flow), then
            // out = multiplicand * (pairwise sum) in rel_mul_finish.  At 320 maps the layers cost the same (1 120 -> 2 240 workgroups on 512 slots:
            // the shorter tail pays for the extra pass: 3.67 -> 3.64 ms over the three layers); a chain of 20 maps - the drop-in's one image - ran
            // them on 72 workgroups with 288-step K loops: 319 -> 190 us each, 4.24 -> 3.86 ms per chain.  A LAYER property, never the batch's:
            // an image's maps are the same bits in every batch (tests/test_gpu_gridtd.py::test_one_image_alone_equals...).  Four ranges: +0.3 ms at 320 maps.
            lrpx_conv_desc dk = d;
            dk.epi = EPI_PLAIN; dk.x = nullptr; dk.out0 = c.R; dk.out1 = nullptr; dk.pool_am = nullptr; dk.map2img = nullptr; dk.tile_group = 0;
            LRPX_TRY(timer.timed(l, c.st, [&] {
                LRPX_TRY(conv_dispatch(&dk, c.st, rel_ks));
                return rel_mul_finish(c.R, rel_ks, c.tr + t.xz[l], c.map2img, c.buf[cur ^ 1], c.n_maps, (long)196 * L.cin, c.st);
            }));
        } else {
            LRPX_TRY(timer.timed(l, c.st, [&] { return conv_dispatch(&d, c.st); }));
        }
        cur ^= 1;
    }
    return timer.timed(0, c.st, [&] { return c.first_layer(c.buf[cur], out_nchw, 0); });
}

// guided backprop (plain = 0) or the plain autograd gradient (plain = 1) of the encoder output w.r.t. the image
static int vgg16_backprop(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc, const int32_t* map2img, int n_maps,
                          void* workspace, float* out_nchw, int plain, const lrpx_vgg16_opts* opts, void* stream) {
    LRPX_REQUIRE(packed && trace && d_feat_nhwc && workspace && out_nchw && n_maps > 0 && n_img > 0, "vgg16_guided_backprop: bad arguments");
    LRPX_CHECK_PTRS(plain ? "lrpx_vgg16_gradient" : "lrpx_vgg16_guided_backprop", {packed, "packed"}, {trace, "trace"}, {d_feat_nhwc, "d_feat_nhwc"},
                    {map2img, "map2img"}, {workspace, "workspace"}, {out_nchw, "out_nchw"});
    LRPX_REQUIRE(map2img || n_maps == n_img, "vgg16_guided_backprop: map2img is required when n_maps != n_img");
    const Chain c(opts, packed, trace, n_img, map2img, n_maps, workspace, stream);
    const VggTrace& t = c.t;
    int cur = 0;
    // hook of the last ReLU (the encoder ends with one): clamp(d,0) * [features > 0]
    LRPX_TRY(guided_gate(d_feat_nhwc, c.tr + t.act[kNL], map2img, c.buf[cur], n_maps, (long)196 * 512, plain, c.st));
    // fp16 split-product kernels: operand scale = per-map maximum of the incoming gradient, recorded by whoever writes that tensor (the
    // GUIDED epilogue of the conv above, the pool backward kernel); only the first tensor costs a streaming read of its own
    unsigned* gam = c.amax;
    if (gam) {
        LRPX_TRY(clear_async(gam, (size_t)kNL * n_maps * sizeof(unsigned), c.st));
        LRPX_TRY(lrpx_amax_maps(c.buf[cur], n_maps, (long)196 * 512, gam + (size_t)16 * n_maps, c.st));
    }
    for (int l = kNL - 1; l > 0; --l) {
        const VggLayer& L = kVgg[l];
        if (!L.conv) continue;
        lrpx_conv_desc d = c.desc(l, c.m.plain, c.buf[cur], c.m.lowres);
        const bool hook = kVgg[l - 1].conv || c.m.lowres;
        if (hook) {
            // ReLU hook of conv l-1 fused - or a pool lies below and the conv under it routes the gradient, which it receives at the pool's OUTPUT
            // resolution, to the windows' arg-max while staging (the winner bytes of the trace, as the relevance chain): no pool-backward kernel, no 4x
            // tensor.  The pool backward's gate [max > 0] (and the guided clamp) is the same hook on the pool's OUTPUT (= this conv's input, act[l])
            d.epi = EPI_GUIDED; d.x = c.tr + t.act[l]; d.out0 = c.buf[cur ^ 1];
            d.relu = plain ? 2 : 0;
            if (gam) d.out0_amax = gam + (size_t)(kVgg[l - 1].conv ? l - 1 : l - 2) * n_maps;
        } else {
            d.epi = EPI_PLAIN; d.out0 = c.R;      // ... else the gradient at the pool's output, then the pool backward kernel
        }
        LRPX_TRY(conv_dispatch(&d, c.st));
        if (!hook)
            LRPX_TRY(maxpool_guided_bwd(c.tr + t.act[l - 1], c.R, map2img, c.buf[cur ^ 1], n_maps, L.hw, L.hw, L.cin, plain,
                                        gam ? gam + (size_t)(l - 2) * n_maps : nullptr, c.st));
        cur ^= 1;
    }
    return c.first_layer(c.buf[cur], out_nchw, 1);      // (W itself in both chains: conv1_1 has no ReLU below it)
}

extern "C" {

int lrpx_vgg16_relevance(const void* packed, const void* trace, int n_img, const float* r_feat_nhwc,
                         const int32_t* map2img, int n_maps, void* workspace, float* out_nchw, void* stream) {
    lrpx_vgg16_opts o = {-1, -1, tl_ms};       // legacy per-thread profiling switch: this call records and waits for its own events
    return lrpx_vgg16_relevance_ex(packed, trace, n_img, r_feat_nhwc, map2img, n_maps, workspace, out_nchw, tl_timing ? &o : nullptr, stream);
}

int lrpx_vgg16_relevance_ex(const void* packed, const void* trace, int n_img, const float* r_feat_nhwc, const int32_t* map2img, int n_maps,
                            void* workspace, float* out_nchw, const lrpx_vgg16_opts* opts, void* stream) {
    LRPX_CHECK_PTRS("lrpx_vgg16_relevance_ex", {packed, "packed"}, {trace, "trace"}, {r_feat_nhwc, "r_feat_nhwc"}, {map2img, "map2img"}, {workspace, "workspace"}, {out_nchw, "out_nchw"});
    LRPX_REQUIRE(packed && trace && r_feat_nhwc && workspace && out_nchw && n_maps > 0 && n_img > 0, "vgg16_relevance: bad arguments");
    LRPX_REQUIRE(map2img || n_maps == n_img, "vgg16_relevance: map2img is required when n_maps != n_img");
    const Chain c(opts, packed, trace, n_img, map2img, n_maps, workspace, stream);
    float* layer_ms = opts ? opts->layer_ms : nullptr;      // host [17]: per-layer HIP-event times of THIS call (events live and die inside the call)
    LayerTimer timer;
    if (layer_ms) LRPX_TRY(timer.begin());
    LRPX_TRY(c.m.fused ? relevance_fused(c, r_feat_nhwc, out_nchw, timer) : relevance_rel(c, r_feat_nhwc, out_nchw, timer));
    if (layer_ms) LRPX_TRY(timer.finish(layer_ms));
    return LRPX_OK;
}

int lrpx_vgg16_layer_timing(int enable, float* ms17) {
    if (ms17)
        for (int l = 0; l < kNL; ++l) ms17[l] = tl_ms[l];
    if (enable >= 0) {
        tl_timing = enable ? 1 : 0;
        if (enable)
            for (int l = 0; l < kNL; ++l) tl_ms[l] = 0.f;
    }
    return LRPX_OK;
}

int lrpx_vgg16_guided_backprop(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc,
                               const int32_t* map2img, int n_maps, void* workspace, float* out_nchw, void* stream) {
    return vgg16_backprop(packed, trace, n_img, d_feat_nhwc, map2img, n_maps, workspace, out_nchw, 0, nullptr, stream);
}

int lrpx_vgg16_guided_backprop_ex(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc, const int32_t* map2img,
                                  int n_maps, void* workspace, float* out_nchw, const lrpx_vgg16_opts* opts, void* stream) {
    return vgg16_backprop(packed, trace, n_img, d_feat_nhwc, map2img, n_maps, workspace, out_nchw, 0, opts, stream);
}

int lrpx_vgg16_gradient(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc,
                        const int32_t* map2img, int n_maps, void* workspace, float* out_nchw, void* stream) {
    return vgg16_backprop(packed, trace, n_img, d_feat_nhwc, map2img, n_maps, workspace, out_nchw, 1, nullptr, stream);
}

int lrpx_vgg16_gradient_ex(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc, const int32_t* map2img,
                           int n_maps, void* workspace, float* out_nchw, const lrpx_vgg16_opts* opts, void* stream) {
    return vgg16_backprop(packed, trace, n_img, d_feat_nhwc, map2img, n_maps, workspace, out_nchw, 1, opts, stream);
}

}  // extern "C"
