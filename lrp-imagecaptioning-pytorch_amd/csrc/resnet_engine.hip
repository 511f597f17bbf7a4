// Elementwise kernels of the batched bottleneck-ResNet encoder engine (ops.ResNetEncoder).  All NHWC fp32, one pass each.
//   trace (once per image)
//     lrpx_resnet_bn_act_coef   eval-mode BN affine (+ ReLU) of a conv's output and the conv's relevance coefficient
//                               q = safe_divide(|y w|, |y w| + |b|) / safe(Z+)      LRPtools/lrp_modules.py:210-215, utils.py:16-18
//     lrpx_resnet_coef_neg      the second coefficient of the general alpha-beta rule, qn = (the same fraction) / safe(Z-), from
//                               [y | Z-]: made at the first alpha-beta call after a forward, not by the trace      
//     lrpx_resnet_add_relu_coef Add + ReLU and the two split coefficients of the Add rule      lrp_modules.py:262-275
//     lrpx_resnet_maxpool_fwd   MaxPool2d of any window                                        models/resnet.py:168
//   relevance (per map, the per-image operands through map2img)
//     lrpx_resnet_add_split     R1 = R c1[img], R2 = R c2[img]: the Add rule behind the block's final ReLU (identity rule)
//     lrpx_resnet_maxpool_rel   the Pool2d rule as a gather per input pixel (the logic of lrpx_maxpool_rule)   lrp_modules.py:182-195
//                               (resnet_maxpool_gather_kernel<false>)
//     lrpx_resnet_stem_fold     [x+ convT | x- convT] halves of the stem's rule joined into the NCHW result    lrp_modules.py:81-84
//   gradient chain (per map)
//     lrpx_resnet_relu_grad     ReLU backward at a block's output, with guided backprop's clamp on request
//     lrpx_resnet_maxpool_grad  MaxPool2d backward: the same gather without the division and the x factor (resnet_maxpool_gather_kernel<true>)
// No kernel uses atomics: a map's result does not depend on the other maps of the call.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)   // expression-by-expression arithmetic, as the reference's elementwise ops evaluate it

namespace lrpx {

static constexpr float kEps = 0.01f;      // LRPtools/utils.py:10 EPSILON
static constexpr float kZEps = 1e-7f;     // LRPtools/utils.py:11 Z_EPSILON

// the BatchNorm fraction safe_divide(|y w|, |y w| + |b|) over safe(z): a conv's relevance coefficient, z = Z+ (q) or Z- (qn)
__device__ __forceinline__ float bn_coef(float y, float wc, float bc, float z) {
    const float xw = fabsf(y * wc);                                   // lrp_modules.py:212
    const float den = xw + fabsf(bc);
    const float frac = xw / (den + kZEps * (den == 0.f ? 1.f : 0.f)); // safe_divide, :214
    return frac / (z + kZEps * (z == 0.f ? 1.f : 0.f));               // S = R / safe(Z), utils.py:28
}

// yz: rows of `ld` floats, the conv's output y in columns [0, c), Z of its rule in [c, 2c) (the stacked forward contraction)
__global__ void resnet_bn_act_coef_kernel(const float* __restrict__ yz, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                          float* __restrict__ act, float* __restrict__ q, long rows, int c, int relu) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * c) return;
    const long r = i / c;
    const int ch = (int)(i - r * c);
    const float y = yz[r * ld + ch], z = yz[r * ld + c + ch];
    const float wc = w[ch], bc = b[ch];
    const float a = y * wc + bc;
    act[i] = relu ? fmaxf(a, 0.f) : a;
    q[i] = bn_coef(y, wc, bc, z);
}

// yz: the conv's output y in columns [0, c), Z- of the general rule in [c, 2c): the coefficient half of the kernel above
__global__ void resnet_coef_neg_kernel(const float* __restrict__ yz, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                       float* __restrict__ qn, long rows, int c) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * c) return;
    const long r = i / c;
    const int ch = (int)(i - r * c);
    qn[i] = bn_coef(yz[r * ld + ch], w[ch], b[ch], yz[r * ld + c + ch]);
}

__global__ void resnet_add_relu_coef_kernel(const float* __restrict__ x1, const float* __restrict__ x2, float* __restrict__ out,
                                            float* __restrict__ c1, float* __restrict__ c2, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = x1[i], b = x2[i];
    float s = a + b;
    out[i] = fmaxf(s, 0.f);
    const float half = s == 0.f ? 0.5f : 0.f;                         // out_mask (:264-265)
    s += kEps * (s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f));             // :267
    float v1 = a / s, v2 = b / s;                                     // :270-271 without the map's factor
    if (v1 != v1 || s == 0.f) v1 = 0.f;                               // :272-273 (0 / 0); x1 = -x2 != 0 has no finite rule: 0
    if (v2 != v2 || s == 0.f) v2 = 0.f;
    c1[i] = v1 + half;                                                // :274-275
    c2[i] = v2 + half;
}

struct RnPoolGeom { int H, W, OH, OW, kh, kw, sh, sw, ph, pw; };

// one thread per output element; padding is skipped (-inf), the FIRST maximum in (kernel row, kernel column) order wins like ATen
__global__ void resnet_maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n, int c, RnPoolGeom g) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * g.OH * g.OW * c) return;
    const int ch = (int)(i % c);
    long rest = i / c;
    const int ow = (int)(rest % g.OW);
    rest /= g.OW;
    const int oh = (int)(rest % g.OH);
    const long img = rest / g.OH;
    const int h0 = max(oh * g.sh - g.ph, 0), h1 = min(oh * g.sh - g.ph + g.kh, g.H);
    const int w0 = max(ow * g.sw - g.pw, 0), w1 = min(ow * g.sw - g.pw + g.kw, g.W);
    const float* xp = x + img * g.H * g.W * c + ch;
    float m = -INFINITY;
    for (int ih = h0; ih < h1; ++ih)
        for (int iw = w0; iw < w1; ++iw) {
            const float v = xp[((long)ih * g.W + iw) * c];
            if (v > m || v != v) m = v;
        }
    y[i] = m;
}

// one thread per INPUT element of a map: visits the windows that contain it in ascending (oh, ow) order, repeats the forward scan of
// each and adds up the term of every window it wins, x through map2img (maxpool_rule_kernel of lrpx_rules.hip in NHWC).
// GRAD false, the Pool2d rule: term R_out / safe(max), result x * sum.  GRAD true, MaxPool2d backward: term g_out, result the sum.
template <bool GRAD>
__global__ void resnet_maxpool_gather_kernel(const float* __restrict__ x, const float* __restrict__ r_out, const int32_t* __restrict__ map2img,
                                             float* __restrict__ r_in, long n_maps, int c, RnPoolGeom g) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_maps * g.H * g.W * c) return;
    const int ch = (int)(i % c);
    long rest = i / c;
    const int w = (int)(rest % g.W);
    rest /= g.W;
    const int h = (int)(rest % g.H);
    const long m = rest / g.H;
    const long img = map2img ? map2img[m] : m;
    const int oh_lo = max(0, (h + g.ph - g.kh + g.sh) / g.sh), oh_hi = min(g.OH - 1, (h + g.ph) / g.sh);
    const int ow_lo = max(0, (w + g.pw - g.kw + g.sw) / g.sw), ow_hi = min(g.OW - 1, (w + g.pw) / g.sw);
    const float* xp = x + img * g.H * g.W * c + ch;
    const float* rp = r_out + m * g.OH * g.OW * c + ch;
    const int p = h * g.W + w;
    float grad = 0.f;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        const int h0 = max(oh * g.sh - g.ph, 0), h1 = min(oh * g.sh - g.ph + g.kh, g.H);
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
            const int w0 = max(ow * g.sw - g.pw, 0), w1 = min(ow * g.sw - g.pw + g.kw, g.W);
            int win = h0 * g.W + w0;
            float mx = -INFINITY;
            for (int ih = h0; ih < h1; ++ih)
                for (int iw = w0; iw < w1; ++iw) {
                    const float v = xp[((long)ih * g.W + iw) * c];
                    if (v > mx || v != v) {
                        mx = v;
                        win = ih * g.W + iw;
                    }
                }
            if (win == p) {
                const float r = rp[((long)oh * g.OW + ow) * c];
                grad += GRAD ? r : r / (mx + kZEps * (mx == 0.f ? 1.f : 0.f));
            }
        }
    }
    r_in[i] = GRAD ? grad : xp[(long)p * c] * grad;
}

__global__ void resnet_relu_grad_kernel(const float* __restrict__ g, const float* __restrict__ act, const int32_t* __restrict__ map2img,
                                        float* __restrict__ out, long n_maps, long per, int clamp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_maps * per) return;
    const long m = i / per;
    const long j = (map2img ? (long)map2img[m] : m) * per + (i - m * per);
    float v = g[i];
    if (clamp) v = fmaxf(v, 0.f);
    out[i] = act[j] > 0.f ? v : 0.f;
}

__global__ void resnet_add_split_kernel(const float* __restrict__ r, const float* __restrict__ c1, const float* __restrict__ c2,
                                        const int32_t* __restrict__ map2img, float* __restrict__ r1, float* __restrict__ r2,
                                        long n_maps, long per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_maps * per) return;
    const long m = i / per;
    const long j = (map2img ? (long)map2img[m] : m) * per + (i - m * per);
    const float v = r[i];
    r1[i] = v * c1[j];
    r2[i] = v * c2[j];
}

// r_split (n_maps, pix, ld) -> out (n_maps, cin, pix) = columns [0, cin) + columns [half, half + cin)
__global__ void resnet_stem_fold_kernel(const float* __restrict__ r_split, float* __restrict__ out, long n_maps, int cin, int half, int ld,
                                        long pix) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_maps * cin * pix) return;
    const long p = i % pix;
    const long rest = i / pix;
    const int ch = (int)(rest % cin);
    const long m = rest / cin;
    const float* rp = r_split + (m * pix + p) * ld;
    out[i] = rp[ch] + rp[half + ch];
}

static bool pool_geom_ok(int h, int w, int oh, int ow, int kh, int kw, int sh, int sw, int ph, int pw) {
    return h > 0 && w > 0 && oh > 0 && ow > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0 && 2 * ph <= kh && 2 * pw <= kw &&
           (long)(oh - 1) * sh < h + ph && (long)(ow - 1) * sw < w + pw;      // every window starts inside the image or its left padding
}

static inline unsigned blocks_of(long total) { return (unsigned)ceil_div(total, 256); }

// what lrpx_resnet_add_split and lrpx_resnet_relu_grad refuse alike; `fn` is the entry's name in the messages
static int per_map_ok(const char* fn, int n_maps, int n_img, long per_map, const int32_t* map2img) {
    LRPX_REQUIRE(n_maps > 0 && n_img > 0 && per_map > 0 && n_maps * per_map < (1L << 38), "%s: bad sizes", fn);
    LRPX_REQUIRE(map2img || n_maps == n_img, "%s: without map2img there is one map per image", fn);
    return LRPX_OK;
}

// the two pool gathers (`what` = "rel" | "grad"): refusals, pointer check, launch
template <bool GRAD>
static int maxpool_gather(const char* what, const float* x, const float* r_out, const int32_t* map2img, float* r_in, int n_maps, int n_img,
                          int h, int w, int oh, int ow, int c, int kh, int kw, int sh, int sw, int ph, int pw, void* stream) {
    LRPX_REQUIRE(x && r_out && r_in, "resnet_maxpool_%s: null pointer", what);
    LRPX_REQUIRE(n_maps > 0 && n_img > 0 && c > 0 && pool_geom_ok(h, w, oh, ow, kh, kw, sh, sw, ph, pw),
                 "resnet_maxpool_%s: bad sizes or window (maps %d images %d c %d, %dx%d -> %dx%d, kernel %dx%d stride %dx%d padding %dx%d)",
                 what, n_maps, n_img, c, h, w, oh, ow, kh, kw, sh, sw, ph, pw);
    LRPX_REQUIRE(map2img || n_maps == n_img, "resnet_maxpool_%s: without map2img there is one map per image", what);
    LRPX_REQUIRE((long)n_maps * h * w * c < (1L << 38), "resnet_maxpool_%s: tensor too large", what);
    LRPX_CHECK_PTRS(GRAD ? "lrpx_resnet_maxpool_grad" : "lrpx_resnet_maxpool_rel", {x, "x"}, {r_out, GRAD ? "g_out" : "r_out"},
                    {map2img, "map2img"}, {r_in, GRAD ? "g_in" : "r_in"});
    const RnPoolGeom g = {h, w, oh, ow, kh, kw, sh, sw, ph, pw};
    hipLaunchKernelGGL(resnet_maxpool_gather_kernel<GRAD>, dim3(blocks_of((long)n_maps * h * w * c)), dim3(256), 0, (hipStream_t)stream, x,
                       r_out, map2img, r_in, (long)n_maps, c, g);
    return check_launch(GRAD ? "resnet_maxpool_grad" : "resnet_maxpool_rel");
}

}  // namespace lrpx

using namespace lrpx;

extern "C" {

int lrpx_resnet_bn_act_coef(const float* yz, int ld, const float* w, const float* b, float* act, float* q, long rows, int c, int relu,
                            void* stream) {
    LRPX_REQUIRE(yz && w && b && act && q, "resnet_bn_act_coef: null pointer");
    LRPX_REQUIRE(rows > 0 && c > 0 && ld >= 2 * c && rows * (long)ld < (1L << 38), "resnet_bn_act_coef: bad sizes (rows %ld, c %d, ld %d)", rows, c, ld);
    LRPX_CHECK_PTRS("lrpx_resnet_bn_act_coef", {yz, "yz"}, {w, "w"}, {b, "b"}, {act, "act"}, {q, "q"});
    hipLaunchKernelGGL(resnet_bn_act_coef_kernel, dim3(blocks_of(rows * c)), dim3(256), 0, (hipStream_t)stream, yz, ld, w, b, act, q, rows, c,
                       relu ? 1 : 0);
    return check_launch("resnet_bn_act_coef");
}

int lrpx_resnet_coef_neg(const float* yz, int ld, const float* w, const float* b, float* qn, long rows, int c, void* stream) {
    LRPX_REQUIRE(yz && w && b && qn, "resnet_coef_neg: null pointer");
    LRPX_REQUIRE(rows > 0 && c > 0 && ld >= 2 * c && rows * (long)ld < (1L << 38), "resnet_coef_neg: bad sizes (rows %ld, c %d, ld %d)", rows, c, ld);
    LRPX_CHECK_PTRS("lrpx_resnet_coef_neg", {yz, "yz"}, {w, "w"}, {b, "b"}, {qn, "qn"});
    hipLaunchKernelGGL(resnet_coef_neg_kernel, dim3(blocks_of(rows * c)), dim3(256), 0, (hipStream_t)stream, yz, ld, w, b, qn, rows, c);
    return check_launch("resnet_coef_neg");
}

int lrpx_resnet_add_relu_coef(const float* x1, const float* x2, float* out, float* c1, float* c2, long n, void* stream) {
    LRPX_REQUIRE(x1 && x2 && out && c1 && c2, "resnet_add_relu_coef: null pointer");
    LRPX_REQUIRE(n > 0 && n < (1L << 38), "resnet_add_relu_coef: bad size %ld", n);
    LRPX_CHECK_PTRS("lrpx_resnet_add_relu_coef", {x1, "x1"}, {x2, "x2"}, {out, "out"}, {c1, "c1"}, {c2, "c2"});
    hipLaunchKernelGGL(resnet_add_relu_coef_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, x1, x2, out, c1, c2, n);
    return check_launch("resnet_add_relu_coef");
}

int lrpx_resnet_maxpool_fwd(const float* x, float* y, int n, int h, int w, int oh, int ow, int c, int kh, int kw, int sh, int sw, int ph,
                            int pw, void* stream) {
    LRPX_REQUIRE(x && y, "resnet_maxpool_fwd: null pointer");
    LRPX_REQUIRE(n > 0 && c > 0 && pool_geom_ok(h, w, oh, ow, kh, kw, sh, sw, ph, pw),
                 "resnet_maxpool_fwd: bad sizes or window (n %d c %d, %dx%d -> %dx%d, kernel %dx%d stride %dx%d padding %dx%d)", n, c, h, w, oh,
                 ow, kh, kw, sh, sw, ph, pw);
    LRPX_REQUIRE((long)n * h * w * c < (1L << 38), "resnet_maxpool_fwd: tensor too large");
    LRPX_CHECK_PTRS("lrpx_resnet_maxpool_fwd", {x, "x"}, {y, "y"});
    const RnPoolGeom g = {h, w, oh, ow, kh, kw, sh, sw, ph, pw};
    hipLaunchKernelGGL(resnet_maxpool_fwd_kernel, dim3(blocks_of((long)n * oh * ow * c)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n, c, g);
    return check_launch("resnet_maxpool_fwd");
}

int lrpx_resnet_maxpool_rel(const float* x, const float* r_out, const int32_t* map2img, float* r_in, int n_maps, int n_img, int h, int w,
                            int oh, int ow, int c, int kh, int kw, int sh, int sw, int ph, int pw, void* stream) {
    return maxpool_gather<false>("rel", x, r_out, map2img, r_in, n_maps, n_img, h, w, oh, ow, c, kh, kw, sh, sw, ph, pw, stream);
}

int lrpx_resnet_add_split(const float* r, const float* c1, const float* c2, const int32_t* map2img, float* r1, float* r2, int n_maps,
                          int n_img, long per_map, void* stream) {
    LRPX_REQUIRE(r && c1 && c2 && r1 && r2, "resnet_add_split: null pointer");
    LRPX_TRY(per_map_ok("resnet_add_split", n_maps, n_img, per_map, map2img));
    LRPX_CHECK_PTRS("lrpx_resnet_add_split", {r, "r"}, {c1, "c1"}, {c2, "c2"}, {map2img, "map2img"}, {r1, "r1"}, {r2, "r2"});
    hipLaunchKernelGGL(resnet_add_split_kernel, dim3(blocks_of(n_maps * per_map)), dim3(256), 0, (hipStream_t)stream, r, c1, c2, map2img, r1,
                       r2, (long)n_maps, per_map);
    return check_launch("resnet_add_split");
}

int lrpx_resnet_relu_grad(const float* g, const float* act, const int32_t* map2img, float* out, int n_maps, int n_img, long per_map,
                          int clamp, void* stream) {
    LRPX_REQUIRE(g && act && out, "resnet_relu_grad: null pointer");
    LRPX_TRY(per_map_ok("resnet_relu_grad", n_maps, n_img, per_map, map2img));
    LRPX_REQUIRE(clamp == 0 || clamp == 1, "resnet_relu_grad: clamp is 0 or 1 (%d)", clamp);
    LRPX_CHECK_PTRS("lrpx_resnet_relu_grad", {g, "g"}, {act, "act"}, {map2img, "map2img"}, {out, "out"});
    hipLaunchKernelGGL(resnet_relu_grad_kernel, dim3(blocks_of(n_maps * per_map)), dim3(256), 0, (hipStream_t)stream, g, act, map2img, out,
                       (long)n_maps, per_map, clamp);
    return check_launch("resnet_relu_grad");
}

int lrpx_resnet_maxpool_grad(const float* x, const float* g_out, const int32_t* map2img, float* g_in, int n_maps, int n_img, int h, int w,
                             int oh, int ow, int c, int kh, int kw, int sh, int sw, int ph, int pw, void* stream) {
    return maxpool_gather<true>("grad", x, g_out, map2img, g_in, n_maps, n_img, h, w, oh, ow, c, kh, kw, sh, sw, ph, pw, stream);
}

int lrpx_resnet_stem_fold(const float* r_split, float* out, int n_maps, int cin, int half, int ld, long pix, void* stream) {
    LRPX_REQUIRE(r_split && out, "resnet_stem_fold: null pointer");
    LRPX_REQUIRE(n_maps > 0 && cin > 0 && half >= cin && ld >= half + cin && pix > 0 && n_maps * pix * ld < (1L << 38), "resnet_stem_fold: bad sizes");
    LRPX_CHECK_PTRS("lrpx_resnet_stem_fold", {r_split, "r_split"}, {out, "out"});
    hipLaunchKernelGGL(resnet_stem_fold_kernel, dim3(blocks_of((long)n_maps * cin * pix)), dim3(256), 0, (hipStream_t)stream, r_split, out,
                       (long)n_maps, cin, half, ld, pix);
    return check_launch("resnet_stem_fold");
}

}  // extern "C"
