/* lrpx — C ABI of the MI355X-native LRP relevance-propagation hot path.
 *
 * Drop-in boundary for SunJiamei/LRP-imagecaptioning-pytorch.  The reference is pure Python; these
 * are the entry points its Python would bind (ctypes) in place of the ATen op
 * clusters of its LRP path.  Each function cites the reference interface it replaces
 * (paths relative to the reference repo).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (or int32 where stated), owned by the caller
 *     (PyTorch's allocator); the library never frees or retains a caller pointer beyond the call
 *     and never allocates device memory (one 4-byte flag word of lrpx_check excepted): workspaces
 *     are caller-provided, sizes come from *_bytes().
 *   - `stream` is a hipStream_t passed as void*; all calls are asynchronous w.r.t. the host.
 *   - internal activation layout is pixel-major NHWC: a [map*H*W][C] row-major matrix.
 *   - return value: 0 = ok, otherwise an LRPX_E* code; lrpx_last_error_string() describes it.
 */
#ifndef LRPX_H
#define LRPX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    LRPX_OK = 0,
    LRPX_EINVAL = 1,      /* bad shape / null pointer / unsupported configuration */
    LRPX_EARCH = 2,       /* device is not gfx950 */
    LRPX_ELAUNCH = 3,     /* hip launch / runtime failure */
    LRPX_ENONFINITE = 4,  /* NaN/Inf found by lrpx_check_finite (the reference's inline asserts) */
    LRPX_EZERO = 5        /* all-zero relevance (reference: `assert sample.grad.sum()!=0`, lrp_wrapper.py:81) */
};

/* The runtime-geometry conv engine and the general MaxPool2d rule (lrpx_conv_geom, lrpx_conv_geom_pack,
 * lrpx_conv_geom_packed_floats, lrpx_maxpool_rule) came WITHOUT a new version number: a caller detects them by the presence
 * of the symbols (dlsym / hasattr on the loaded library).
 * The same holds for the batched ResNet engine's entries (lrpx_conv_geom_ex, lrpx_resnet_*) and their conv mode 1 siblings
 * (lrpx_conv_geom_packed_bf16x3_bytes, lrpx_conv_geom_pack_bf16x3, lrpx_conv_geom_ex_b6), and for the general alpha-beta rule on
 * that engine (lrpx_conv_geom_ab, lrpx_conv_geom_ab_b6, lrpx_resnet_coef_neg), and for its gradient chain (lrpx_conv_geom_grad,
 * lrpx_conv_geom_grad_b6, lrpx_resnet_relu_grad, lrpx_resnet_maxpool_grad), and for the alpha-beta rule under a 2x2 max-pool
 * (lrpx_conv_geom_ab_pool, lrpx_conv_geom_ab_pool_b6, lrpx_vgg16_ab_coef, lrpx_conv_geom_ex_b6_blocked).
 * 101: the alpha-beta Conv2d rule (LRPX_PACK_*_PN*, lrpx_divide_alpha_beta, lrpx_maxpool2x2_relevance_ab); 100 before it */
int lrpx_version(void);
const char* lrpx_last_error_string(void);
/* "" for a release build.  Otherwise the list of timing-experiment / profiling switches the library was compiled with
 * (-DLRPX_EXPERIMENTS with -DLRPXH_EXP=.. / -DLRPX_EPI_EXP=.. / ..., make STAMP=1): such a build computes WRONG results by
 * design (or carries profiling atomics) and must never serve a caller - tests/test_abi.py and smoke() assert "". */
const char* lrpx_build_flags(void);

/* ---- weight packing ------------------------------------------------------------------------- */
enum {
    LRPX_PACK_FWD_DUAL = 0,  /* conv fwd: channels [0,cout) = W, [cout,2cout) = clamp(W,min=0)  (PosNetConv weights, LRPtools/lrp_modules.py:66-67) */
    LRPX_PACK_BWD_POS = 1,   /* relevance pass: transposed conv with clamp(W,min=0)            (lrp_modules.py:136-138 through autograd) */
    LRPX_PACK_BWD_FIRST = 2, /* first layer: out 0..cin-1 = W+ , cin..2cin-1 = W-  (signed inputs, lrp_modules.py:78-84) */
    LRPX_PACK_BWD_PLAIN = 3, /* transposed conv with W (guided backprop, models/gridTDmodel.py:1702-1723) */
    LRPX_PACK_DENSE_T = 4,   /* dense: out = in @ W      W is (k, n)   (epsilon rule W^T contraction, gridTDmodel.py:744-765) */
    LRPX_PACK_DENSE = 5,     /* dense: out = in @ W^T    W is (n, k)   (nn.Linear forward) */
    LRPX_PACK_FWD = 6,       /* conv fwd, plain W only */
    LRPX_PACK_FWD_DUAL_FIRST = 7, /* first conv: the signed input is stored split, channels [0,cin) = x+, [cin,2cin) = x-;
                                  plain part = W on both, Z part = W+ on x+ and W- on x-  (Z = conv(x+,W+)+conv(x-,W-),
                                  lrp_modules.py:81-84) */
    /* The general alpha-beta rule  R = alpha * lrp_backward(PosNetConv) - beta * lrp_backward(NegNetConv)  (lrp_modules.py:124-150,
     * the two nets at :56-122).  Its two forward convs and its two transposed convs are ONE contraction each with the second
     * net stacked along the channel axis: Z = [Z+ | Z-] are 2 cout output channels, and with S2 = [alpha S+ | -beta S-]
     * (lrpx_divide_alpha_beta) the relevance is x * convT(S2, [W+ ; W-]) with K = 2 cout.  fp32 packer only. */
    LRPX_PACK_FWD_PN = 8,        /* x >= 0, k = cin: channels [0,cout) = W+ (Z+ = conv(x,W+), :66-67), [cout,2cout) = W- (Z- = conv(x,W-), :104-105) */
    LRPX_PACK_FWD_PN_FIRST = 9,  /* input split [x+ | x-], k = 2cin: [0,cout) = W+ on x+ and W- on x- (Z+, :81-84),
                                    [cout,2cout) = W- on x+ and W+ on x- (Z-, :116-121) */
    LRPX_PACK_BWD_PN = 10,       /* k = 2cout, oc = cin, taps flipped: rows [0,cout) (alpha S+) carry W+, rows [cout,2cout) (-beta S-) carry W- */
    LRPX_PACK_BWD_PN_FIRST = 11  /* as BWD_PN with oc = 2cin for the split multiplicand [x+ | x-]: W+ where (row in the S+ half) ==
                                    (column in the x+ half), W- otherwise; lrpx_fold_halves joins the halves */
};
/* number of floats of the packed image: n_oc/k padded to multiples of 32 / kc */
size_t lrpx_packed_floats(int n_oc, int k, int taps, int kc);
/* w: conv (cout,cin,3,3) or dense matrix; kc = K-chunk the consuming kernel will use (lrpx_conv_kc) */
int lrpx_pack_weights(const float* w, int cout, int cin, int taps, int mode, int kc, float* packed, void* stream);
/* bf16x3 split of the same fragment layout for the fp32-accurate bf16 path (lrpx_conv_desc.bf16x6): every weight is
 * stored as three bf16 planes w = w0 + w1 + w2; modes BWD_POS / BWD_PLAIN / FWD; 3x3 kernels (taps = 9) or - round 6 - a dense
 * (cout, cin) matrix (taps = 1; BWD_PLAIN = the transposed product of the epsilon rules, as lrpx_pack_weights_f16x2) */
size_t lrpx_packed_bf16x3_bytes(int n_oc, int k, int taps);
int lrpx_pack_weights_bf16x3(const float* w, int cout, int cin, int taps, int mode, void* packed, void* stream);
/* f16x2 split for the fp16 matrix-core path (lrpx_conv_desc.f16x3): the layer's weights are scaled by a power of two
 * 2^kW (max|w| * 2^kW in [2^14, 2^15)) and stored as two fp16 planes w * 2^kW ~= hi + lo (22 significand bits); a
 * 64-byte header carries 2^-kW for the consumer's epilogue.  Same modes as lrpx_pack_weights_bf16x3. */
size_t lrpx_packed_f16x2_bytes(int n_oc, int k, int taps);
int lrpx_pack_weights_f16x2(const float* w, int cout, int cin, int taps, int mode, void* packed, void* stream);
/* weights for lrpx_conv_desc.f16x3 = 2 (fp16 hi.hi product + the two cross products on the narrow-format matrix cores;
 * the symbol keeps its round-1 name): scaled into [2^14, 2^15), stored per tap row as fp16 hi planes + block-scaled fp6
 * e2m3 fields of (w - hi)*2^11 and w with one E8M0 exponent per (output channel, tap, 16 channels) in the operand
 * layout of v_mfma_f32_32x32x64_f8f6f4 (K = 3 taps + a zero slot, x 16 channels).  3x3 kernels, modes BWD_POS / BWD_PLAIN */
size_t lrpx_packed_f16f8_bytes(int n_oc, int k);
int lrpx_pack_weights_f16f8(const float* w, int cout, int cin, int mode, void* packed, void* stream);
/* Winograd F(2x2,3x3) form of the same relevance weights (modes BWD_POS / BWD_PLAIN, 3x3 kernels): for each of the 16 transform
 * positions U = G g G^T evaluated in fp64, rounded once to fp32 and stored as three bf16 planes (16/9 of the bf16x3 image);
 * lrpx_conv_desc.wpacked_wino */
size_t lrpx_packed_wino_b6_bytes(int n_oc, int k);
int lrpx_pack_weights_wino_b6(const float* w, int cout, int cin, int mode, void* packed, void* stream);
/* which bf16x6 REL_MUL convs with wpacked_wino run on the Winograd kernel: bit 0 = 56 x 56, bit 1 = 28 x 28, bit 2 = 14 x 14 maps.
 * Bit 3 (8) = the Winograd kernel stages its patches the way it always did: every thread fetches all four columns of its patch.  Without the
 * bit a thread fetches its tile's own two columns and takes the outer two from the neighbouring lanes of its wave (column sharing): the same
 * bits, fewer bytes through the vector-memory path, measured NOT faster and kept for A/B.
 * Process-wide; initial value from LRPX_B6_WINO (default 15: all three map sizes, own-fetch staging).  bits < 0 only queries.  Returns the previous
 * value.  0 = the direct kernels, bit for bit what the library computed before the Winograd kernel existed */
int lrpx_set_b6_wino(int bits);
/* K-chunk used by lrpx_conv_mfma for a given image width / taps / input channels */
int lrpx_conv_kc(int hw, int taps, int cin);

/* ---- the contraction engine ------------------------------------------------------------------ */
enum { LRPX_EPI_FWD_DUAL = 0, LRPX_EPI_REL = 1, LRPX_EPI_FIRST = 2, LRPX_EPI_PLAIN = 3, LRPX_EPI_GUIDED = 4,
       LRPX_EPI_REL_MUL = 5 /* out1 (or out0; exactly one of them) = x * acc: the rule with the next layer's division folded into the
                               multiplicand (x = X for R, x = X / safe(Z_below) for S_next); the f16x3 epilogue */ };
enum { LRPX_STAB_NONE = 0, LRPX_STAB_SAFE = 1, LRPX_STAB_EPS = 2 };

typedef struct lrpx_conv_desc {
    const float* in;      /* [n_maps*pix_per_map][cin], or channel-chunked [cin/kc][n_maps*pix_per_map][kc] if in_chunked */
    const float* wpacked; /* from lrpx_pack_weights with kc = lrpx_conv_kc(hw,taps,cin) */
    int n_maps, hw, cin, n_oc, taps, pix_per_map;
    int epi, stab, oc_split, relu;
    int in_chunked;       /* input stored in K-chunks of lrpx_conv_kc(hw,taps,cin) channels (see lrpx_maxpool2x2_relevance) */
    int bf16x6;           /* 1: contraction on the bf16 matrix cores with exact 3-way operand splits and the 6 leading
                             partial products (fp32 accuracy, 2.67x less matrix-pipe time); wpacked must come from
                             lrpx_pack_weights_bf16x3; 3x3 convs, cin %% 16 == 0.  Epilogues: REL (conv_bf16x6.h) and - round 6,
                             on the conv_f16x3.h tiling - FWD_DUAL, GUIDED, bias-free PLAIN at hw <= 56 and REL_MUL (x = the precomputed
                             multiplicand; with pool_am the input is the relevance at the pool's output and is unpooled while staged).
                             FWD_DUAL needs oc_split %% 32 == 0 (a 32-channel block goes to out0 or to out1 as a whole; every VGG16
                             layer): any other oc_split is LRPX_EINVAL.  No operand scales: in_amax / out1_amax unused.
                             taps = 1 (round 6): the (word, pixel) epsilon rules of the decoders (gridTDmodel.py:1125-1128, aoamodel.py:1135-1148)
                             in the same exact arithmetic - REL epilogue with x, map2img and ONE of out0 / out1 (+ zdiv), optional u;
                             cin %% 32 == 0, oc_split %% 4 == 0, 16-byte aligned operands, any number of rows (one kernel: a row's sum
                             never depends on the batch).  What the host layer uses while the conv mode is 0 / 1 */
    const float* bias;
    const float* x;
    const float* u;
    const float* zdiv;
    const int32_t* map2img;
    float* out0;
    float* out1;
    int f16x3;            /* 1: contraction on the fp16 matrix cores: operands scaled into the fp16 range (per map /
                             per layer, powers of two) and split in two halves, 3 partial products, fp32 accumulate
                             (22-bit operands: below the rounding of the fp32 accumulation itself; half the matrix
                             time of bf16x6).  wpacked from lrpx_pack_weights_f16x2; needs in_amax; REL_MUL or FWD_DUAL epilogue,
                             3x3 convs, cin %% 16 == 0.
                             2: as 1, but the two cross products hi*lo + lo*hi (2^-11 of the result) run on the fp6 matrix
                             cores (e2m3, one block exponent per 16-channel slice; rounds 1-2: fp8 e4m3) - error 2^-15 of a
                             product, random sign: the maps move by < 1e-5 of their maximum; wpacked from
                             lrpx_pack_weights_f16f8; REL_MUL, GUIDED or PLAIN epilogue */
    int out_chunk;        /* REL_MUL: > 0 writes the output channel-chunked [C/out_chunk][n_maps*pixels][out_chunk] (16 / 32) */
    const uint32_t* in_amax;  /* f16x3: [n_maps] float bits of max|in| per map (lrpx_amax_maps, or a producer's out1_amax) */
    uint32_t* out1_amax;      /* f16x3 + out1: max|out1| per map is atomicMax-ed into it (zero it first); may be null */
    uint32_t* out0_amax;      /* f16x3 + FWD_DUAL: max of out0 (the activations) per map is atomicMax-ed into it; may be null */
    const uint8_t* pool_am;   /* f16x3, or bf16x6 with REL_MUL: the conv sits under a 2x2 max-pool and `in` is the relevance at the pool's
                                 OUTPUT [n_maps][hw/2*hw/2][cin]; pool_am [n_img][hw/2*hw/2][cin] = window position
                                 (0..3, row-major) of each maximum (lrpx_pool_winner): Pool2d.propagate_relevance
                                 (lrp_modules.py:182-195) is applied while the operand is staged */
    int tile_group;           /* f16x3 / bf16x6 REL_MUL, performance hint only (results do not depend on it): maps [k*g, (k+1)*g) share an
                                 image (the g words of a caption): their tiles of the same image rows are scheduled next to
                                 each other on one XCD, so the per-image multiplicand `x` is fetched from HBM once, not g
                                 times.  0 / 1: plain order.  Needs n_maps %% g == 0 and map-aligned tiles (hw >= 56) */
    int blocked;              /* bit 0 (1): `in`, bit 1 (2): `x`, bit 2 (4): the output are in the BLOCKED layout (lrpx_nhwc_to_blocked
                                 below): [16-channel chunk][32-pixel block][4-channel part][pixel][4] - `in` / out: ONE block set over
                                 all n_maps * pixels, `x`: one block set per image.  f16x3 = 2 with REL_MUL (the relevance chain of conv
                                 mode 3) REQUIRES 7; its 224 x 224 kernel 1 (x and the output stay NHWC); every other kernel 0 */
    const void* wpacked_wino; /* optional, bf16x6 with REL_MUL, no pool_am, hw 56 / 28 / 14, n_oc %% 64 == 0, NHWC `in`: the same weights from
                                 lrpx_pack_weights_wino_b6.  Where lrpx_set_b6_wino has the bit of hw set the conv runs as Winograd F(2x2,3x3)
                                 on the exact splits (16 instead of 36 six-product multiplications per 2x2 outputs and channel pair; fp32
                                 grade like the direct kernel, other rounding); tile_group is ignored there */
} lrpx_conv_desc;
/* 3x3/pad-1 convolution (taps=9, square hw x hw maps) or dense GEMM (taps=1) on the fp32 MFMA with
 * the fused epilogues of the relevance rules.  Replaces F.conv2d / conv backward inside
 * LRPtools/utils.py:21-31 `lrp_backward` and torch.matmul/sum inside `lrp_linear_eps`.
 * taps = 9 is built for hw = 224, 112, 56, 28 and 14 only: any other hw is LRPX_EINVAL, in every arithmetic (before the kernel list of
 * csrc/conv_kernels.def, bf16x6 PLAIN and Winograd descriptors with another hw <= 56 ran a kernel compiled for 14 x 14 maps). */
int lrpx_conv_mfma(const lrpx_conv_desc* d, void* stream);
/* Which kernel lrpx_conv_mfma would run for *d: exactly its validation and selection, pure host code - nothing is launched or cleared, no
 * pointer is dereferenced or queried (pointers only need to be non-null where the descriptor needs them).  Writes
 * "<name> ks=<K split> tg=<tile group>" into buf (len bytes, truncated), <name> = the row of csrc/conv_kernels.def (the launcher launch_<name>; b6_<hw>_wino_share = the Winograd kernel
 * with column-sharing staging, lrpx_set_b6_wino bit 8 clear) or one of dense_bf16x6,
 * dense_f16x3, dense_small_f16x3, dense_small; the selection reads lrpx_set_b6_wino.  LRPX_EINVAL + lrpx_last_error_string() where
 * lrpx_conv_mfma refuses the descriptor. */
int lrpx_conv_kernel_name(const lrpx_conv_desc* d, char* buf, int len);

/* ---- the contraction engine at any conv geometry (csrc/conv_geom_kernel.h, fp32 entries in csrc/conv_geom.hip; the ResNet encoders' 7x7 s2, 1x1, 1x1 s2, 3x3 s2) ------ */
enum { LRPX_GEOM_FWD = 0,   /* out[n,oh,ow,co] = sum in[n, oh*sh-ph+r, ow*sw-pw+s, ci] * w[co,ci,r,s] (+ bias[co]) */
       LRPX_GEOM_BWD = 1 }; /* the transposed conv autograd runs inside lrp_backward (LRPtools/utils.py:21-31), times x:
                               out[n,h,w,ci] = x[n,h,w,ci] * sum in[n,oh,ow,co] * w[co,ci,r,s] over oh*sh-ph+r = h, ow*sw-pw+s = w */
typedef struct lrpx_conv_geom_desc {
    const float* in;       /* FWD: [n*h*w][k];  BWD: [n*oh*ow][k] (S of the rule).  16-byte aligned, k %% 4 == 0 */
    const float* wpacked;  /* lrpx_conv_geom_pack of the same direction */
    const float* bias;     /* FWD only, [n_oc], may be NULL */
    const float* x;        /* BWD only, [n*h*w][n_oc]: the multiplicand of the epilogue */
    float* out;            /* FWD: [n*oh*ow][n_oc];  BWD: [n*h*w][n_oc] */
    int dir;               /* LRPX_GEOM_FWD / LRPX_GEOM_BWD */
    int n, h, w, oh, ow;   /* h x w: the conv's INPUT map, oh x ow = (h + 2 ph - kh) / sh + 1, ... its output map, in both directions */
    int kh, kw, sh, sw, ph, pw;   /* dilation 1, groups 1, zero padding */
    int k, n_oc;           /* contraction channels (row length of `in`) and output channels (row length of out / x); any n_oc */
} lrpx_conv_geom_desc;
/* fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulation: the arithmetic grade of conv mode 0.  BWD tiles the output by sub-pixel
 * class (h mod sh, w mod sw) and visits only the taps that reach a class; pixels no window covers are exact zeros. */
int lrpx_conv_geom(const lrpx_conv_geom_desc* d, void* stream);
/* floats of the packed image for n_oc output channels, k contraction channels, taps = kh * kw */
size_t lrpx_conv_geom_packed_floats(int n_oc, int k, int taps);
/* w: (cout, cin, kh, kw) as nn.Conv2d stores it (the caller stacks W+ / W- along either channel axis first).
 * FWD: k = cin, n_oc = cout;  BWD: k = cout, n_oc = cin. */
int lrpx_conv_geom_pack(const float* w, int cout, int cin, int kh, int kw, int dir, float* packed, void* stream);

/* ---- the same engine with the operands of a BATCHED relevance pass (csrc/conv_geom.hip; ops.ResNetEncoder) ----
 * The kernel, packed weights (lrpx_conv_geom_pack) and arithmetic of lrpx_conv_geom, which is this entry without q, addend and map2img.  FWD is the plain convolution: the trace stacks
 * [W | W+] along the output columns (the caller, before packing) and gets the conv's output and Z+ of its rule from ONE gather of
 * the input tile.  BWD answers for the transposed conv inside lrp_backward (LRPtools/utils.py:21-31) with the division
 * S = R / safe(Z) (utils.py:28) and the BatchNorm rule above the conv (lrp_modules.py:210-215) folded into a per-image multiplier:
 *   out[m,h,w,ci] = x[img,h,w,ci] * sum (in[m,oh,ow,co] * q[img,oh,ow,co]) * w[co,ci,r,s]  (+ addend[m,h,w,ci]),  img = map2img[m]. */
typedef struct lrpx_conv_geom_ex_desc {
    const float* in;       /* FWD: [n*h*w][k];  BWD: [n*oh*ow][k], the relevance at the conv's output, per MAP.  16-byte aligned, k %% 4 == 0 */
    const float* wpacked;  /* lrpx_conv_geom_pack of the same direction */
    const float* bias;     /* FWD only, [n_oc], may be NULL */
    const float* x;        /* BWD only, [n_img*h*w][n_oc]: the multiplicand of the epilogue, per IMAGE */
    const float* q;        /* BWD only, may be NULL, [n_img*oh*ow][k], 16-byte aligned: multiplies `in` while the tile is gathered */
    const float* addend;   /* BWD only, may be NULL, [n*h*w][n_oc]: added after the multiplication by x (also where no tap reaches) */
    const int32_t* map2img;/* BWD only, [n] image of each map, every entry in [0, n_img) - the CALLER validates it, the kernel trusts
                              it;  NULL: map m reads image m (then n_img == n) */
    float* out;            /* FWD: [n*oh*ow][n_oc];  BWD: [n*h*w][n_oc] */
    int dir;               /* LRPX_GEOM_FWD / LRPX_GEOM_BWD */
    int n, n_img;          /* n: images (FWD) / maps (BWD);  n_img: images behind x and q (BWD; ignored by FWD) */
    int h, w, oh, ow;      /* as lrpx_conv_geom_desc: the conv's INPUT map and its output map, in both directions */
    int kh, kw, sh, sw, ph, pw;   /* dilation 1, groups 1, zero padding */
    int k, n_oc;           /* contraction channels (row length of `in` / q) and output channels (row length of out / x / addend) */
} lrpx_conv_geom_ex_desc;
/* fp32 MFMA, fp32 accumulation (the grade of conv mode 0); no atomics: a map's result does not depend on the other maps. */
int lrpx_conv_geom_ex(const lrpx_conv_geom_ex_desc* d, void* stream);

/* ---- the batched engine in the exact arithmetic of conv mode 1 (csrc/conv_geom_b6.hip; ops.ResNetEncoder(conv_mode=1))
 * Every fp32 operand is split exactly into three bf16 planes; the six plane products with i + j <= 2 run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation, small terms first: fp32-grade results in 12 bf16 MFMAs per (tap, 32-channel chunk)
 * where lrpx_conv_geom_ex issues 16 fp32 ones.  Detected by the presence of the symbols, like the other ResNet entries. */
/* bytes of the bf16x3 image: ceil(n_oc / 32) * taps * ceil(k / 32) * 2 k-steps * 3 planes * 1024 */
size_t lrpx_conv_geom_packed_bf16x3_bytes(int n_oc, int k, int taps);
/* as lrpx_conv_geom_pack (the caller stacks W+ / W- first); packed: lrpx_conv_geom_packed_bf16x3_bytes bytes, 16-byte aligned */
int lrpx_conv_geom_pack_bf16x3(const float* w, int cout, int cin, int kh, int kw, int dir, void* packed, void* stream);
/* lrpx_conv_geom_ex with `wpacked` the bf16x3 image of the same direction: same descriptor, same refusals, same tiling and masking,
 * no atomics.  An in * q that overflows to +-inf comes out NaN here (the lower planes of inf are NaN), inf there. */
int lrpx_conv_geom_ex_b6(const lrpx_conv_geom_ex_desc* d, void* stream);
/* The forward direction of lrpx_conv_geom_ex_b6 (dir = LRPX_GEOM_FWD only, else LRPX_EINVAL) with its sums in a BLOCKED order: the cross
 * products of the split collect in an accumulator of their own and the main accumulator is flushed into a second level every 8
 * (tap, chunk) stages.  Z+ of a conv is a sum of terms of one sign: the plain forward rounds 12 times per stage at the running sum's
 * full size, this one (stages / 8) + 16 times per output.  Same descriptor, packs, tiling and refusals; other bits than the plain
 * forward's.  What lrpx_vgg16_ab_coef's input is made with. */
int lrpx_conv_geom_ex_b6_blocked(const lrpx_conv_geom_ex_desc* d, void* stream);

/* ---- the transposed direction of both engines with TWO coefficients: the general alpha-beta rule without bias on the batched engine
 * (LRPtools/lrp_modules.py:124-150; ops.ResNetEncoder.relevance_alpha_beta).  For a conv with a non-negative input
 *   R_in = x ( convT(alpha R qp, W+) + convT(-beta R qn, W-) ),   qp = f / safe(conv(x, W+)),  qn = f / safe(conv(x, W-)),
 * f the BatchNorm fraction above the conv.  One contraction over the stacked index kappa in [0, 2 kr) against the rows [W+ ; W-]:
 *   out[m,h,w,ci] = x[img,h,w,ci] * sum_kappa A(kappa) * w2[kappa,ci,r,s]  (+ addend[m,h,w,ci]),   img = map2img[m],
 *   A(kappa) = (in[m,oh,ow,c] * qh[img,oh,ow,c]) * sh,  c = kappa mod kr,  (qh, sh) = (q, scale) for kappa < kr, (q2, scale2) above,
 * formed in fp32, in that order, while the A tile is gathered (scale 1 is the operand of lrpx_conv_geom_ex bit for bit); S never
 * exists.  alpha and beta are launch arguments: nothing per image depends on them.  Tiling, stages, sub-pixel classes, masking and the
 * epilogue are those of lrpx_conv_geom_ex / _ex_b6; no atomics, a map's result does not depend on the other maps of the call. */
typedef struct lrpx_conv_geom_ab_desc {
    lrpx_conv_geom_ex_desc base; /* dir = LRPX_GEOM_BWD only; in / q have row length kr (not k); q is required; bias NULL.
                                    k = 2 kr: wpacked is lrpx_conv_geom_pack(_bf16x3) of the (2 kr, n_oc, kh, kw) tensor [W+ ; W-].
                                    k = kr: the W+ half alone (beta == 0): wpacked as for lrpx_conv_geom_ex, q2 NULL, scale2 0 */
    const float* q2;             /* [n_img*oh*ow][kr], 16-byte aligned: the coefficient of the second half; required iff k = 2 kr */
    float scale, scale2;         /* finite: alpha and -beta */
    int kr;                      /* relevance channels (the conv's cout), a multiple of 4 */
} lrpx_conv_geom_ab_desc;
int lrpx_conv_geom_ab(const lrpx_conv_geom_ab_desc* d, void* stream);      /* fp32 MFMA, the arithmetic of lrpx_conv_geom_ex */
/* exact bf16 split (split3 after both multiplications); the cross products collect in an accumulator of their own, joined to the
 * a0 b0 sums once per output: W+ against W- cancels, and fewer roundings at the running sum's size keep the result fp32 grade */
int lrpx_conv_geom_ab_b6(const lrpx_conv_geom_ab_desc* d, void* stream);

/* ---- the same two entries for a conv that sits directly under a 2x2 / stride-2 max-pool (VGG16's conv1_2, 2_2, 3_3, 4_3;
 * ops.Vgg16.relevance_alpha_beta(conv_mode=1)).  The Pool2d rule (lrp_modules.py:182-195) hands a window's relevance to
 * its first maximum, R where that maximum is non-zero and 0 where the whole window is zero: a per-image 0 / 1 factor, folded into q / q2
 * by lrpx_vgg16_ab_coef.  `in` is the relevance BEHIND the pool,
 *   in [n * (oh / 2) * (ow / 2)][kr],   A(kappa) = (in[m, oh' >> 1, ow' >> 1, c] * qh[img, oh', ow', c]) * sh,
 * read inside the pooled map's bounds: a last odd row / column of the conv's output lies under no window and contributes zero.  The
 * relevance at the conv's own resolution never exists.  Everything else - stacked K, scale / scale2, x, addend, map2img, k = kr with q2
 * NULL, arithmetic, tiling, refusals - is lrpx_conv_geom_ab's / _ab_b6's; no atomics, no workspace. */
typedef struct lrpx_conv_geom_ab_pool_desc {
    lrpx_conv_geom_ab_desc ab;   /* as above, but ab.base.in at the pooled resolution */
    int pool;                    /* 2: kernel = stride = 2, no padding, floor mode.  Anything else is LRPX_EINVAL */
} lrpx_conv_geom_ab_pool_desc;
int lrpx_conv_geom_ab_pool(const lrpx_conv_geom_ab_pool_desc* d, void* stream);     /* fp32 MFMA */
int lrpx_conv_geom_ab_pool_b6(const lrpx_conv_geom_ab_pool_desc* d, void* stream);  /* exact bf16 split */
/* The per-image coefficients of those entries on VGG16 (once per forward, independent of alpha and beta).  zz [n_img*oh*ow][2c] =
 * [Z+ | Z-], the rows of one stacked forward contraction;  qp, qn [n_img*oh*ow][c]:
 *   qp = win / safe(Z+),  qn = win / safe(Z-),  safe(z) = z + 1e-7 (z == 0)  (LRPtools/utils.py:28), IEEE division of 1.
 * xpool NULL: win = 1.  xpool [n_img*oh*ow][c], the input of the 2x2 max-pool above the conv (the conv's ReLU output): win = 1 at the
 * FIRST maximum of the pixel's window (row-major, strict >) if that maximum != 0, else 0; 0 for pixels no window covers (odd oh / ow).
 * c % 4 == 0, all pointers 16-byte aligned; 64-bit indices, no atomics. */
int lrpx_vgg16_ab_coef(const float* zz, const float* xpool, float* qp, float* qn, int n_img, int oh, int ow, int c, void* stream);

/* ---- the transposed direction of both engines for the GRADIENT chain through conv -> BatchNorm (eval) -> ReLU
 * (ops.ResNetEncoder.gradient / guided_backprop): plain autograd (ExplainGridTDGradient.explain_cnn,
 * models/gridTDmodel.py:1510-1521) and guided backprop (:1677-1691).  wpacked is the transposed pack of the RAW weights W (K = cout):
 *   out[m,h,w,ci] = sum A[m,oh,ow,co] * w[co,ci,r,s]  (+ addend[m,h,w,ci]),   img = map2img[m],
 *   A = scale[co] * (mask[img,oh,ow,co] > 0 ? (clamp ? max(in, 0) : in) : 0)
 * formed in fp32 in the order clamp, mask, scale while the A tile is gathered (the b6 entry splits afterwards).  mask is the ReLU's
 * OUTPUT (or input: only its sign is read; NaN passes), scale the BatchNorm factor gamma / sqrt(var + eps).  There is no multiplicand:
 * x is never read, and a stride class no tap reaches is addend or 0.  No divisions.  Tiling, stages, sub-pixel classes and zero
 * pattern are those of lrpx_conv_geom_ex / _ex_b6: with mask all positive, scale NULL and clamp 0 the result is lrpx_conv_geom_ex's with
 * q = 1 and x = 1, byte for byte.  Detected by the presence of the symbols, like the other ResNet entries. */
typedef struct lrpx_conv_geom_grad_desc {
    lrpx_conv_geom_ex_desc base; /* dir = LRPX_GEOM_BWD only; x, q, bias NULL; in (n maps, OH OW, k) -> out (n, H W, n_oc);
                                    addend, map2img, n_img as lrpx_conv_geom_ex */
    const float* mask;           /* (n_img, OH OW, k) or NULL; 16-byte aligned */
    const float* scale;          /* (k) or NULL; 16-byte aligned */
    int clamp;                   /* 0 / 1 */
} lrpx_conv_geom_grad_desc;
int lrpx_conv_geom_grad(const lrpx_conv_geom_grad_desc* d, void* stream);     /* fp32 MFMA */
int lrpx_conv_geom_grad_b6(const lrpx_conv_geom_grad_desc* d, void* stream);  /* exact bf16 split; wpacked from lrpx_conv_geom_pack_bf16x3 */

/* ---- elementwise / layout kernels -------------------------------------------------------------- */
/* NHWC <-> BLOCKED (csrc/blocked.h): n_groups tensors of pix_per_group pixels x c channels (c %% 16 == 0), each its own block set
 * of lrpx_blocked_floats(pix_per_group, c) floats: element (pixel p, channel ch) at (ch / 16) * CS + (p / 32) * 512 + ((ch % 16) / 4)
 * * 128 + (p % 32) * 4 + ch % 4, CS = ceil(pix / 32) * 512.  An S tensor of the mode-3 chain is ONE group of n_maps * pixels; the
 * per-image multiplicands are n_img groups. */
size_t lrpx_blocked_floats(long n_pix, int c);
int lrpx_nhwc_to_blocked(const float* src, float* dst, long n_groups, int pix_per_group, int c, void* stream);
int lrpx_blocked_to_nhwc(const float* src, float* dst, long n_groups, int pix_per_group, int c, void* stream);
/* (n,c,h,w) -> [n*h*w][c_pad] with zero padding channels; and back (first c of c_src channels) */
int lrpx_nchw_to_nhwc(const float* src, float* dst, int n, int c, int hw_pix, int c_pad, void* stream);
int lrpx_nhwc_to_nchw(const float* src, float* dst, int n, int c, int hw_pix, int c_src, void* stream);
/* signed image -> [n*h*w][c_pad]: channels [0,c) = max(x,0), [c,2c) = min(x,0), rest 0 */
int lrpx_nchw_to_nhwc_posneg(const float* src, float* dst, int n, int c, int hw_pix, int c_pad, void* stream);
/* MaxPool2d(2,2) forward on NHWC (models/vgg.py:67) */
int lrpx_maxpool2x2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
/* Pool2d.propagate_relevance (LRPtools/lrp_modules.py:182-195) fused with the division by the
 * conv layer below:  r_in = x * [argmax] * (r_out / safe(max));  s_out = r_in / safe(zdiv).
 * x, zdiv: per IMAGE (n_img,2h,2w,c); r_out: per MAP (n_maps,h,w,c); outputs per map at 2h x 2w.
 * r_in / s_out may be null (skip).  zdiv may be null (then s_out = r_in).
 * s_chunk > 0: s_out is written channel-chunked [c/s_chunk][n_maps*2h*2w][s_chunk] (s_chunk = 8), the layout
 * lrpx_conv_mfma reads with in_chunked=1: whole 128-byte lines per chunk instead of 32-byte slices of every pixel. */
int lrpx_maxpool2x2_relevance(const float* x, const float* r_out, const float* zdiv, const int32_t* map2img,
                              float* r_in, float* s_out, int n_maps, int h_out, int w_out, int c, int s_chunk,
                              void* stream);
/* s[n,p,c] = r[n,p,c] / stab(z[img(n),p,c])   (LRPtools/utils.py:16-18 safe_divide with broadcast) */
int lrpx_divide_stab(const float* r, const float* z, const int32_t* map2img, float* s, int n_maps, long pix_c,
                     int stab, void* stream);
/* The divisions of the general alpha-beta Conv2d rule in one pass (lrp_modules.py:136-147: safe_divide of the incoming relevance by
 * the outputs of PosNetConv and of NegNetConv, then `alpha * R_pos - beta * R_neg` - the two factors are folded into S here):
 *   s2[n,p,0..c) = alpha * (r[n,p,:] / safe(zpos[img(n),p,:])),   s2[n,p,c..2c) = -beta * (r[n,p,:] / safe(zneg[img(n),p,:]))
 * r: [n_maps*pix][c]; zpos / zneg: [n_img*pix][c] per IMAGE (map2img, null = identity); s2: [n_maps*pix][2c]; c % 4 == 0.
 * safe(z) = z + 1e-7 [z == 0] (LRPtools/utils.py:16-18); IEEE division.  Element indices are 64-bit. */
int lrpx_divide_alpha_beta(const float* r, const float* zpos, const float* zneg, const int32_t* map2img, float* s2,
                           int n_maps, int pix, int c, float alpha, float beta, void* stream);
/* lrpx_maxpool2x2_relevance with the two divisors of the alpha-beta rule of the conv below the pool: the Pool2d rule
 * (lrp_modules.py:182-195; first maximum wins, an all-zero window sends r_out / 1e-7 * 0 = 0 to its first pixel) followed by
 * lrpx_divide_alpha_beta, without the full-resolution relevance ever reaching memory.
 * x, zpos, zneg: per IMAGE (n_img,2h,2w,c); r_out: per MAP (n_maps,h,w,c); s2: (n_maps,2h,2w,2c). */
int lrpx_maxpool2x2_relevance_ab(const float* x, const float* r_out, const float* zpos, const float* zneg,
                                 const int32_t* map2img, float* s2, int n_maps, int h_out, int w_out, int c, float alpha,
                                 float beta, void* stream);
/* Per image, for a 2x2 max-pool with input x (n,2h,2w,c) sitting on a conv with Z+ = z (n,2h,2w,c):
 *   am[n,h,w,c]  = window position (0..3, row-major, first maximum wins as in max_pool2d's backward)
 *   xzw[n,h,w,c] = max / safe(z at the winner): the multiplicand that turns the accumulator of the conv ABOVE the pool
 *                  straight into S = R / Z+ of the conv BELOW it at the winner (Pool2d rule + safe_divide fused). */
int lrpx_pool_winner(const float* x, const float* z, float* xzw, uint8_t* am, int n, int h_out, int w_out, int c,
                     void* stream);
/* the Pool2d rule as a scatter for a conv that does not unpool while staging: s_hi (n_maps, 2*h_out, 2*w_out, c) =
 * s_lo (n_maps, h_out, w_out, c) at the winner positions `am` (per image, from lrpx_pool_winner), 0 elsewhere */
int lrpx_unpool_winner(const float* s_lo, const uint8_t* am, const int32_t* map2img, float* s_hi, int n_maps, int h_out,
                       int w_out, int c, void* stream);
/* amax[n] = float bits of max |s[n,:]| (zeroes amax first): the per-map operand scale of the f16x3 convolution */
int lrpx_amax_maps(const float* s, int n_maps, long per, uint32_t* amax, void* stream);
/* running sum over the maps of one image: out[b,t] = sum_{t'<=t} in[b,t']  (the reference's
 * `sample.grad` accumulation, LRPtools/lrp_wrapper.py:64-82); per = floats per map, any positive count (float4 accesses where it is
 * a multiple of four, as for 224 x 224 and 448 x 448 maps; element by element otherwise - the same sums).  lrpx_scatter_maps and
 * lrpx_accumulate likewise. */
int lrpx_cumsum_maps(const float* in, float* out, int n_img, int t_per_img, long per, void* stream);
/* Captions of unequal length (the reference explains whatever length its beam search returns, models/gridTDmodel.py:935-937,
 * 1147-1153): `in` holds only the VALID (image, word) maps, image b's lens[b] maps starting at map offs[b]; `out` is the padded
 * [n_img][t_per_img] layout - the valid maps (accumulate = 1: their running sums, as lrpx_cumsum_maps) and exact zeros behind
 * an image's last word. */
int lrpx_scatter_maps(const float* in, float* out, int n_img, int t_per_img, const int32_t* lens, const int32_t* offs,
                      long per, int accumulate, void* stream);
/* dst[0 .. bytes) = 0 on `stream` (hipMemsetAsync).  The host layer clears its scratch through the library, not through the
 * framework, so that a recorded step (lrp_amd._lib.Recording: the calls of one eager run, replayed without the interpreter's
 * per-launch cost) contains EVERY device operation of the step. */
int lrpx_zero(void* dst, size_t bytes, void* stream);

/* dst[r][0..width) = src[rows[r]][0..width) for 4-byte items (per-row operands of the compacted (word, pixel) rules) */
int lrpx_gather_rows(const void* src, const int32_t* rows, void* dst, int n_rows, int width, void* stream);
/* dst += src  (the `.grad` accumulation of autograd that compute_lrp relies on, lrp_wrapper.py:80-82) */
int lrpx_accumulate(float* dst, const float* src, long n, void* stream);
/* out[row][c] = in[row][c] + in[row][half + c]: joins the x+ / x- halves of a split relevance tensor
 * (R = x+ * convT(S,W+) + x- * convT(S,W-), lrp_modules.py:56-84, for signed layer inputs) */
int lrpx_fold_halves(const float* in, float* out, long rows, int half, void* stream);
/* NaN/Inf + all-zero check of a buffer (the asserts of lrp_modules.py:154-155, lrp_wrapper.py:81);
 * synchronises the stream.  flags: bit0 = fail on non-finite, bit1 = fail on all-zero */
int lrpx_check(const float* buf, long n, int flags, void* stream);

/* THREADING.  Every entry point is thread-compatible: calls on different host threads / streams with different caller
 * buffers never share mutable state.  What the library keeps is (a) the one-time kernel-attribute initialisation of each
 * kernel instantiation (std::call_once), (b) the 4-byte flag word of lrpx_check behind a mutex, (c) the thread-local
 * error string, (d) the PROCESS DEFAULTS set by lrpx_set_conv_mode / lrpx_set_forward_f16 / lrpx_set_bf16x6 (atomics).
 * A caller that wants a mode of its own - or that runs while another thread changes the defaults - passes it per call in
 * an lrpx_vgg16_opts to the *_ex entry points; such a call never reads the defaults. */
typedef struct lrpx_vgg16_opts {
    int conv_mode;     /* 0 fp32 MFMA, 1 bf16x6, 2 f16x3, 3 fp16 + fp6 cross products; < 0: the process default */
    int forward_f16;   /* forward trace on the fp16 split-product kernels: 0 / 1; < 0: the process default */
    float* layer_ms;   /* lrpx_vgg16_relevance_ex only, may be NULL.  HOST array of 17 floats: the call records HIP events of
                          its own around every conv launch, WAITS for them and stores the milliseconds per VGG16 layer index
                          (0 for pools / the first layer); the events are created and destroyed inside the call */
} lrpx_vgg16_opts;
/* the values a call with `opts` (NULL: none) would run with - host logic only, no device access */
int lrpx_vgg16_resolve_opts(const lrpx_vgg16_opts* opts, int* conv_mode, int* forward_f16);

/* Process-wide DEFAULT for lrpx_vgg16_relevance: 1 (default) runs the relevance passes of the 56/28/14-pixel layers on
 * the bf16 matrix cores with exact operand splits (fp32 accuracy, see lrpx_conv_desc.bf16x6), 0 keeps the fp32 MFMA
 * everywhere; a negative value only queries.  Returns the previous setting. */
int lrpx_set_bf16x6(int enable);
/* Matrix-core mode of the fused VGG16 chains: 0 fp32 MFMA, 1 bf16x6 (exact 3-way bf16 splits of both operands, six products, fp32
 * accumulate: 24 significand bits and fp32's exponent range per operand - THE DEFAULT since round 6, arithmetic no narrower than the
 * reference's fp32 convolutions, LRPtools/lrp_modules.py:124-150), 2 f16x3 (fp16 split products behind per-map power-of-two
 * scales: 22 operand bits, fp16's exponent range below the map maximum), 3 = 2 with the cross products of the relevance pass on the fp6
 * matrix cores (lrpx_conv_desc.f16x3 = 2).  Modes 2 / 3 are opt-in speed modes (1.6x / 2.0 - 2.2x the maps/s of mode 1, inside the 1e-4
 * contract on every tested input of natural range).  RANGE CONTRACT of modes 2 / 3: the relevance operand S = R / Z+ of a layer is scaled by
 * ONE power of two per map into the fp16 range; entries more than ~2^29 below the map's maximum flush to zero and entries below ~2^-15 of it
 * lose bits, so a map whose layer activations differ by more than ~2^16 BETWEEN REGIONS of one image (S = R / Z+ then spans that range the
 * other way) is rounded against its largest region: tests/test_gpu_range.py pins 1e-2-grade maps on a 2^33 range, where modes 0 / 1 keep 1e-4.  LRPX_CONV_MODE in the environment sets the initial default (read once at load).
 * Negative: query only.  Returns the previous mode. */
int lrpx_set_conv_mode(int mode);
/* 1 (conv modes 2 / 3 only): the forward trace of conv1_1..conv5_3 also runs on the fp16 split-product kernels (operand scale =
 * per-image maximum of the layer input).  RANGE CONTRACT of that switch: inputs more than ~2^29 below their image's maximum
 * flush to zero; a receptive field made only of such inputs gets Z+ = 0 and the relevance arriving there is dropped, where the
 * reference (LRPtools/utils.py:16-18 stabilises exact zeros only) redistributes it (tests/test_gpu_range.py).
 * 0 (THE DEFAULT since round 6, every conv mode): exact kernels - fp32 MFMA for conv1_1, exact bf16 splits (fp32's exponent
 * range) above; conv mode 0: fp32 MFMA throughout.  LRPX_FORWARD_F16 in the environment sets the initial default.
 * Negative: query.  Returns the previous value. */
int lrpx_set_forward_f16(int enable);

/* ---- device-side consumers of the relevance maps (evaluation.py) -------------------------- */
/* (n,c,hw) -> (n,hw): mode 0 mean over channels (evaluation.py:134), 1 mean of max(x,0) (:410-412), 2 mean of max(-x,0) (:406-408) */
int lrpx_spatial_reduce(const float* maps, int n, int c, long hw, int mode, float* out, void* stream);
/* `_project_maxabs` (evaluation.py:338-343): every map divided by its max |x| in place (all-zero maps stay zero) */
int lrpx_project_maxabs(float* x, int n, long per, void* stream);
/* `block_image` (evaluation.py:57-80): sums over patch x patch squares, mask = 0 on the k squares with the largest sum
 * (ties: lower index first), 1 elsewhere; spatial, mask: (n,h,w) */
int lrpx_patch_mask(const float* spatial, int n, int h, int w, int patch, int k, float* mask, void* stream);
/* `_calculate_overlaped_pixels` (evaluation.py:313-336) for every threshold: boxes [n][4] = x0,y0,x1,y1 (pixels),
 * out[n][nthr] = sum of the relevance > thr inside the box / sum of the relevance > thr (0 if that is 0, capped at 1) */
int lrpx_bbox_ratio(const float* spatial, int n, int h, int w, const int32_t* boxes, const float* thresholds, int nthr,
                    float* out, void* stream);
/* tpfp statistics (evaluation.py:506-513): out[n][4] = mean, mean |x|, mean of the positive entries (0 if none), max */
int lrpx_map_stats(const float* spatial, int n, long per, float* out4, void* stream);

/* np.quantile(map, q) ('linear' method) of every (H*W) map: the 100-point quantiles of the tpfp statistics
 * (evaluation.py:451, :510, :543).  spatial (n, per) floats, q (nq) doubles in [0,1], out (n, nq).
 * `workspace`: lrpx_map_quantiles_workspace(n, per) bytes of device memory (sorted copy + sort scratch; 0 = the
 * shape is unsupported, n*per must stay below 2^31). */
size_t lrpx_map_quantiles_workspace(int n, long per);
int lrpx_map_quantiles(const float* spatial, int n, long per, const double* q, int nq, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
/* `LRPutil.heatmap(LRPutil.gamma(hm))` (LRPtools/utils.py:67-145) as the explainers' visualize_explanations call it
 * (models/gridTDmodel.py:1196-1198): gamma correction with the map's own max |x|, sum over the channels, projection to
 * [0, 255] with the summed map's max |x|, colour-map lookup.  maps (n,c,hw) -> out (n,hw,3); lut [nlut][3] (the
 * colour map sampled at its nlut = 256 entries); tmp: n*hw floats of scratch. */
int lrpx_heatmap(const float* maps, int n, int c, long hw, float gamma, const float* lut, int nlut, float* tmp, float* out,
                 void* stream);

/* ---- VGG16 encoder: trace + relevance chain ------------------------------------------------------ */
/* bytes of the packed-weight blob / per-batch trace / relevance workspace */
size_t lrpx_vgg16_packed_bytes(void);
size_t lrpx_vgg16_trace_bytes(int n_img);
size_t lrpx_vgg16_workspace_bytes(int n_maps);
/* w[13], b[13]: device pointers to the conv weights (cout,cin,3,3) / biases in layer order */
int lrpx_vgg16_pack(const float* const* w, const float* const* b, void* packed, void* stream);
/* Per-layer timing of lrpx_vgg16_relevance for profiling, per calling THREAD: enable = 1 makes this thread's following
 * plain lrpx_vgg16_relevance calls behave like lrpx_vgg16_relevance_ex with opts.layer_ms (events of their own, the
 * call waits for them); ms17 (may be null) receives the milliseconds per VGG16 layer index of this thread's last such
 * call.  enable < 0: query only.  (Kept for callers of the round-1 ABI; new code passes opts.layer_ms.) */
int lrpx_vgg16_layer_timing(int enable, float* ms17);
/* recompute the trace tensors derived from the saved activations (x / safe(Z+_below), the multiplicand of the fused
 * conv->conv relevance step); lrpx_vgg16_forward calls it, callers that overwrite activations in the trace must too */
int lrpx_vgg16_trace_derive(void* trace, int n_img, void* stream);
/* Encoder.forward (models/gridTDmodel.py:40-43) + the per-layer inputs `save_input_hook` keeps
 * (LRPtools/lrp_wrapper.py:24-25) + Z+ of every conv.  img: (n_img,3,224,224) NCHW.
 * feat_nhwc: (n_img,196,512) encoder output (may be null: it also lives in the trace). */
int lrpx_vgg16_forward(const void* packed, const float* img_nchw, int n_img, void* trace, float* feat_nhwc,
                       void* stream);
/* compute_lrp (LRPtools/lrp_wrapper.py:63-87) for N maps sharing n_img traces: r_feat (N,196,512) NHWC
 * relevance at the encoder output -> out (N,3,224,224) NCHW.  map2img[N] int32 (null: identity, then
 * n_maps == n_img).  `trace` must come from lrpx_vgg16_forward with the same n_img. */
int lrpx_vgg16_relevance(const void* packed, const void* trace, int n_img, const float* r_feat_nhwc,
                         const int32_t* map2img, int n_maps, void* workspace, float* out_nchw, void* stream);
/* offsets (in floats) of the per-layer tensors inside a trace made for n_img images: act_off[18]
 * (act[l] = NHWC input of leaf l in forward order conv,conv,pool,...; act[0] is the image stored split
 * [x+|x-|0 0] with 8 channels; act[17] = encoder output) and zpos_off[17] (Z+ of conv l, 0 for pools).
 * This is what `module.input` is to the reference's hooks (lrp_wrapper.py:24-25). */
int lrpx_vgg16_trace_layout(int n_img, size_t* act_off, size_t* zpos_off);
/* pointer to the encoder output features (n_img,196,512) inside a trace */
const float* lrpx_vgg16_trace_features(const void* trace, int n_img);
/* Channel balance of the Z+ / relevance side: conv layer `layer` (0..16, a conv of cfg 'D') keeps its Z+ in the trace as
 * Z'_c = rs[c] * conv(X, W+)_c and every alpha1beta0 relevance pack carries rs[c] * W+[c,:], rs[c] = 2^(e_max - e_c), e_c = floor(log2
 * max W+[c,:]) (exact powers of two: S'_c (rs_c W+[c,i]) is the reference's product S_c W+[c,i] of LRPtools/lrp_modules.py:124-150 bit
 * for bit).  It keeps the operands of the split-product modes inside fp16's range when a channel's weights are small against its bias
 * (trained weights, models/vgg.py:86-94).  Returns the DEVICE pointer of rs inside `packed` (n_channels floats), null for a pool. */
const float* lrpx_vgg16_channel_scales(const void* packed, int layer, int* n_channels);
/* DEVICE pointer of 17 floats inside `packed` (index = layer; pools: unset): the largest ratio of row maxima max|W[c,:,:,:]| inside one
 * 16-row slice of a conv layer's weights.  The image-gradient chains (guided backprop / plain gradient) multiply with W itself; in conv
 * mode 3 the cross terms of their operands are fp6 fields that share ONE scale per 16-channel slice, so a slice whose rows differ by
 * 2^6 and more loses the cross terms of its small rows (measured on log-normal channel scales: 1.1e-4 of max|gradient|, fp16 split
 * products 4e-6).  A caller that wants the 1e-4 grade on any weights runs those chains in conv mode 2 when a layer exceeds ~64
 * (lrp_amd.ops.Vgg16 does).  The relevance chain is not affected: its rows are balanced (lrpx_vgg16_channel_scales). */
const float* lrpx_vgg16_row_spread(const void* packed);


/* ---- small dense / utility kernels of the decoders ----------------------------------------------- */
/* out[b][n] = act(sum_k x[b][k] w[n][k] + bias[n]); w in nn.Linear layout (N,K); a few rows b (weight-read bound).
 * act: 0 none, 1 relu.  ldx/ldo = row strides in floats.  (nn.Linear / LSTMCell matmuls of
 * models/gridTDmodel.py:773-797, :980-990 at batch size B) */
int lrpx_linear_small(const float* x, long ldx, const float* w, const float* bias, float* out, long ldo, int B, int K,
                      int N, int act, void* stream);
/* avg[b][c] = mean_p f[b][p][c]   (nn.AdaptiveAvgPool2d(1), models/gridTDmodel.py:38,42) */
int lrpx_mean_pixels(const float* f, float* avg, int B, int P, int C, void* stream);
int lrpx_relu(const float* x, float* y, long n, void* stream);
/* first maximum per row -> int64 (torch.argmax / topk(1), models/gridTDmodel.py:499, :849) */
int lrpx_argmax_rows(const float* x, long ld, int rows, int n, long long* out, void* stream);
/* greedy `sample_next_word` (models/gridTDmodel.py:522-526): argmax of log_softmax(x[r]) and its value */
int lrpx_argmax_logprob_rows(const float* x, long ld, int rows, int n, long long* out, float* logprob, void* stream);
/* logit[b*T+t] = fc.weight[tok[b][t+1]] . hc[b][t] + fc.bias[...]  (the one entry of `predictions`
 * that explain_caption_wordt reads, models/gridTDmodel.py:1027,1034) */
int lrpx_target_logit(const float* hc, const float* fcw, const float* fcb, const long long* tok, int tok_ld,
                      float* logit, int B, int T, int H, void* stream);

/* ---- gridTD decoder: trace (get_hidden_parameters, models/gridTDmodel.py:933-1012) ------------------ */
typedef struct lrpx_gridtd_trace {
    int B, T, H, E, P;
    float *xh1, *xh2;                   /* [B][T][2E+2H] = x1t ++ h1t ; [B][T][3H] = x2t ++ h2t  (:1025-1026) */
    float *h1, *c1, *h2, *c2;           /* [B][T+1][H] */
    float *g1, *i1, *f1, *g2, *i2, *f2; /* [B][T][H]  g = pre-activation, i/f = activations (:1002-1009) */
    float *s, *ctx, *ctx_hat, *hc;      /* [B][T][H]  hc = h2[t+1] + ctx_hat[t] (fc input) */
    float *alpha, *beta;                /* [B][T][P], [B][T] */
    float *o1, *o2, *sgate;             /* [B][T][H] output gates + sentinel gate: only the gradient explainers'
                                           trace keeps them (models/gridTDmodel.py:1323-1422); may be null */
} lrpx_gridtd_trace;
/* per step t: build xh1 ; LSTM point-wise (which = 1 AdaLSTM incl. sentinel, 2 LanguageLSTM) ; adaptive attention */
int lrpx_gridtd_fwd_pre(const lrpx_gridtd_trace* tr, int t, const float* glob, const float* emb, const long long* tok,
                        int tok_ld, void* stream);
int lrpx_gridtd_fwd_lstm(const lrpx_gridtd_trace* tr, int t, const float* zz, int ldz, int which, void* stream);
/* LRP-inference decoding, `GridTDModel.sample_lrp` / `forwardlrp_context` (models/gridTDmodel.py:631-702, :579-630).
 * Their forward differs from the model's own in one place: the sentinel gate sees the NEW h1 (:672, :610).
 *   fwd_gate_input: xg[b] = [h2_old | glob | emb | h1_new]  ((B, 2E+2H) floats), the input of x_gate|h_gate;
 *   fwd_sentinel:   s[b,t] = sigmoid(zg[b]) * tanh(c1_new)  with zg = [x_gate|h_gate] xg + biases, (B, ldz);
 *   lrp_reweight:   `get_lrp_weight_step` (:548-577) for step t: k = argmax pred[b]; unless skip[k] (stop words and
 *                   special tokens), R = pred[b][k] goes back through fc (epsilon rule) to h2 + ctx_hat and is split
 *                   between the two; both vectors are normalised to weights x / max|x| + 1 (LRPtools/utils.py:55-64);
 *                   hcw[b] = ctx_hat * w_ctx + w_h2 * h2, the re-weighted fc input (:687).  skip: V bytes. */
int lrpx_gridtd_fwd_gate_input(const lrpx_gridtd_trace* tr, int t, float* xg, void* stream);
int lrpx_gridtd_fwd_sentinel(const lrpx_gridtd_trace* tr, int t, const float* zg, int ldz, void* stream);
int lrpx_gridtd_lrp_reweight(const lrpx_gridtd_trace* tr, int t, const float* pred, long ld, int V, const float* fc_w,
                             const unsigned char* skip, float* hcw, void* stream);
/* the same rule on plain rows: h / ctx = the two fc summands of row r (row strides ldh / ldc, H = 512).  log_softmax = 1
 * is `AOAModel.get_lrp_weight_step` as `AOAModel.sample_lrp` calls it (models/aoamodel.py:597-626, :721-723): the rule
 * sees log_softmax(pred), i.e. the relevance sent back through fc is log p(k). */
int lrpx_lrp_reweight_rows(const float* pred, long ld, int V, const float* h, long ldh, const float* ctx, long ldc,
                           const float* fc_w, const unsigned char* skip, float* hcw, int rows, int H, int log_softmax,
                           void* stream);
/* one beam-search step (GridTDModel.beam_search, models/gridTDmodel.py:437-444; AOAModel.beam_search): the k <= 4 best of
 * cum[r] + log_softmax(x[r,:n])[w] over the n_rows <= 8 live beams; out_idx[j] = r * n + w (int64), out_val[j] the score,
 * best first (ties: lower flat index).  cum may be NULL (zeros). */
int lrpx_beam_topk(const float* x, long ld, int n_rows, int n, const float* cum, int k, long long* out_idx, float* out_val,
                   void* stream);
/* The same beam search for N images at once with its state on the device: no device -> host read per step.  Image i owns rows
 * i k .. i k + k - 1 of the decoder trace (k = beam size <= 4), its live rows first, in the order the reference keeps them.
 *   toks       [N k][tok_ld] int64, tok_ld >= T + 1: the live sequences; column t is the decoder's input of step t.  The caller fills ALL of
 *              it with start_id: a row that is not live carries a valid id for the embedding gather, and is never read by a selection
 *   cum        [N k] cumulative scores (zeros), n_live [N] (k), best [N][best_ld >= T + 1] / best_len [N] (zeros) / best_score [N]: the
 *              best complete sequence so far - a later one replaces it only with a strictly greater score (the reference takes the
 *              first maximum in order of completion, :469-470)
 *   live_images  one int, N at the start: the images with n_live > 0 (a caller may poll it to stop early; the result does not depend on it)
 *   end_id / end_ids   the <end> id, or one per image (device, may be NULL)
 *   state      up to 4 tensors [N k][T + 1][state_w] (row stride state_ld floats): the LSTM state the decoder step t wrote at time t + 1
 * lrpx_beam_step_batch, after the decoder step t and its scores x [N k][ld >= V]: selection (the arithmetic of lrpx_beam_topk: step 0
 * row 0 alone with k candidates, else n_live rows and n_live candidates, flat index r V + w, ties to the lower index), the bookkeeping
 * (:447-467: append the word, set <end> candidates aside in ascending candidate index, compact the survivors in their order), toks
 * column t + 1, cum, and the state at time t + 1 gathered by the survivors' parents - ONE launch, one workgroup per image.  An image whose
 * n_live is 0 is not touched.  The first step (t = 0) validates every pointer, the later ones under LRPX_CHECK_PTRS=1.
 * lrpx_beam_result_batch after `steps` steps: out[i] = [length, tokens ...] (out_ld >= T + 2 int64) - the best complete sequence, or
 * live sequence 0 cut to 20 tokens (:472); incl. <start>.
 * T = max_cap_length <= LRPX_BEAM_MAX_STEPS: the kernel keeps one thread per sequence position; larger values are LRPX_EINVAL. */
#define LRPX_BEAM_MAX_STEPS 1024
typedef struct lrpx_beam_batch {
    int N, k, V, T;
    int start_id, end_id;
    const int32_t* end_ids;
    long long* toks;
    long long* best;
    float *cum, *best_score;
    int32_t *n_live, *best_len, *live_images;
    float* state[4];
    long state_ld;
    int tok_ld, best_ld, state_w, n_state;
} lrpx_beam_batch;
int lrpx_beam_step_batch(const lrpx_beam_batch* p, const float* x, long ld, int t, void* stream);
int lrpx_beam_result_batch(const lrpx_beam_batch* p, int steps, long long* out, int out_ld, void* stream);
/* Diverse beam search (GridTDModel.diverse_beam_search, models/gridTDmodel.py:304-398; the other four model classes run the same
 * algorithm on their own step) for N images at once, its state on the device.  Image i owns G k rows of the decoder trace: G = k = beam
 * size <= 4 groups of k beams, group g the rows (i G + g) k .. + k - 1, live rows first.  One launch per decoder step, one workgroup per
 * image, the groups in sequence inside it:
 *   - a group without live beams is passed over (:340-341);
 *   - scores cum[r] + ((x[r][w] - lse[r]) - diversity), the subtraction only for the columns w that are among the distinct INPUT words
 *     of this step of groups 0 and 1, as far as these selected earlier in this step (:346-349, :377-380; at most 8 ids);
 *   - selection and bookkeeping as lrpx_beam_step_batch (t = 0: row 0 alone with k candidates);
 *   - a group whose last live beam completes ends the step for the groups after it (the `break`, :365-366): they keep sequences, scores
 *     and input words, and their state tensors are carried from time t to time t + 1.
 * So a group's sequences are not as long as the step count: seqs [N G k][seq_ld >= T + 1] int64 with seq_len [N G] (the caller fills
 * column 0 with start_id and seq_len with 1), while toks [N G k][tok_ld >= T + 1] holds only the decoder's inputs (column t = the input
 * of step t; the caller fills ALL of it with start_id).  cum [N G k] zeros, n_live [N G] = k, best [N G][best_ld >= T + 1] / best_len
 * (zeros) / best_score [N G] per group as in lrpx_beam_batch, live_images one int = N (images with a live group).  When a group's last
 * beam completes, its sequence row 0 becomes candidate 0 of that step, <end> included (what `seqs[g][0]` holds after :357).
 * lrpx_dbs_result_batch: out[i G + g] = [length, tokens ...] (out_ld >= T + 2) - group g's best complete sequence, or, where it has
 * none, the first 20 tokens of sequence row 0 of GROUP 0 (:389: `seqs[0][0][:20]`).
 * T <= LRPX_BEAM_MAX_STEPS.  The first step (t = 0) validates every pointer, the later ones under LRPX_CHECK_PTRS=1. */
typedef struct lrpx_dbs_batch {
    int N, k, G, V, T;
    int start_id, end_id;
    float diversity;
    const int32_t* end_ids;
    long long* toks;
    long long* seqs;
    long long* best;
    float *cum, *best_score;
    int32_t *n_live, *seq_len, *best_len, *live_images;
    float* state[4];
    long state_ld;
    int tok_ld, seq_ld, best_ld, state_w, n_state;
} lrpx_dbs_batch;
int lrpx_dbs_step_batch(const lrpx_dbs_batch* p, const float* x, long ld, int t, void* stream);
int lrpx_dbs_result_batch(const lrpx_dbs_batch* p, long long* out, int out_ld, void* stream);
/* out[r] = softmax(x[r,:n])[ids[r]] (evaluation.py:122, :149, :252: the score of one word); an id outside [0, n) gives NaN */
int lrpx_softmax_pick_rows(const float* x, long ld, int rows, int n, const long long* ids, float* out, void* stream);
/* word ablation (evaluation.py:242-247): row r is a caption prefix caps[r][0 .. t[r]] (column 0 = <start>) with the relevance of its
 * words r_words[r][0 .. t[r]].  The kdel <= LRPX_DELETE_MAX positions 1 + topk(r_words[r][1 : t + 1], kdel) are dropped (position 0 is never
 * a candidate; ties: lower position; fewer than kdel candidates: all of them), the others keep their order: out[r][0 .. out_len[r] - 1].
 * deleted (may be NULL): [rows][kdel] the dropped positions, most relevant first, -1 where there was none. */
#define LRPX_DELETE_MAX 4
int lrpx_delete_topk_tokens(const long long* caps, int cap_ld, const float* r_words, int rw_ld, const int32_t* t, int rows, int kdel,
                            long long* out, int out_ld, int32_t* out_len, int32_t* deleted, void* stream);
/* scratch: [B][3*P] floats (scores, W_g h, W_s s) */
int lrpx_gridtd_fwd_attention(const lrpx_gridtd_trace* tr, int t, const float* Vp, const float* att_img,
                              const float* Wg, const float* Ws, const float* bs, const float* wh, float* scratch,
                              void* stream);

/* ---- gridTD decoder: relevance (explain_caption_wordt, models/gridTDmodel.py:1014-1135) -------------- */
typedef struct lrpx_gridtd_relstate {
    const int32_t* lens;                /* [B] words per image (null: T) */
    float *r_h2n, *r_c2, *r_c1, *r_ch0, *r_h2p; /* [B*T][H] */
    float* r_glob;                      /* [B*T][E] */
    float *A, *rx;                      /* dense-rule input [B*T][H] / output [B*T][2E+2H] */
    float* wacc;                        /* [B*T][T][H] */
    float* r_words;                     /* [B*T][T] */
} lrpx_gridtd_relstate;
/* decoder steps t0 <= t < t1 of get_hidden_parameters (models/gridTDmodel.py:952-1012) in ONE call - fwd_pre, the AdaLSTM gate linear,
 * its cell + sentinel, the adaptive attention, the LanguageLSTM linear, its cell - the `for t in range(...)` loop with its host side in
 * native code (the same launches as the per-step entry points: bit-identical) */
typedef struct lrpx_gridtd_step_args {
    const float *glob, *emb;            /* relu(global_img_feature_proj(avg)) [B][E], embedding table */
    const long long* tok; int tok_ld;   /* token ids [B][tok_ld] */
    const float *w_cat1, *b_cat1;       /* [AdaLSTM W_ih | W_hh ; x_gate | h_gate] (5H x (2E+2H)) and bias */
    const float *w_cat2, *b_cat2;       /* LanguageLSTM [W_ih | W_hh] (4H x 3H) and its bias (the explainers' quirk or the model's) */
    const float *Vp, *att_img;          /* relu(img_projector(features)) [B][P][H]; W_v_proj(Vp) + b [B][P][P] */
    const float *Wg, *Ws, *bs, *wh;     /* AdaAttention W_g_proj, W_s_proj (+ bias), w_h */
    float *zz1, *zz2, *att_scratch;     /* scratch [B][5H], [B][4H], [B][3P] */
    /* optional (all four or none): the first 4H rows of w_cat1 / w_cat2 and their biases with the gate rows INTERLEAVED - row 16 j + 4 gate + u =
     * row gate * H + 4 j + u - for the fused step (gate linear + LSTM cell in one launch, the next input row behind the second: 4 launches per
     * time step instead of 7, bit-identical traces; <= 64 images) */
    const float *w_il1, *b_il1, *w_il2, *b_il2;
} lrpx_gridtd_step_args;
int lrpx_gridtd_fwd_steps(const lrpx_gridtd_trace* tr, int t0, int t1, const lrpx_gridtd_step_args* a, void* stream);

int lrpx_gridtd_rel_init(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* fcw,
                         const float* logit, const long long* tok, int tok_ld, void* stream);
/* lock-step s, phase 0: LanguageLSTM cell split (:1061-1069) -> A ; 1: after its dense rule (:1074-1105) -> A ;
 * 2: after the AdaLSTM dense rule (:1110-1115) ; 3: phase 2 of lock-step s and phase 0 of lock-step s + 1 in one launch */
int lrpx_gridtd_rel_step(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, int s, int phase, void* stream);
/* lock-steps 0 <= s < n_steps of explain_caption_wordt's `for i in range(t+1)[::-1]` (models/gridTDmodel.py:1060-1113) in ONE call: phase 0,
 * the LanguageLSTM dense rule `dense2`, phase 1, the AdaLSTM dense rule `dense1`, phase 2 (lrpx_conv_mfma descriptors whose map2img is
 * replaced by idx + s * idx_ld: row -> source row of the multiplicand at lock-step s) */
int lrpx_gridtd_rel_steps(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, int n_steps, const lrpx_conv_desc* dense2,
                          const lrpx_conv_desc* dense1, const int32_t* idx, int idx_ld, void* stream);
int lrpx_gridtd_rel_glob(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* glob_pre,
                         float* a_glob, void* stream);
int lrpx_rel_avg_u(const float* r_avg, const float* avg, float* u, int rows, int T, int C, int P, void* stream);
int lrpx_gridtd_rel_pix(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* Vp,
                        const float* proj_pre, float* a_proj, void* stream);
/* the same for the n_rows (image, word) rows listed in `rows` (row = image * T + word) only, written COMPACTLY: a_proj
 * [n_rows][P][H] - padded words of captions shorter than T then cost nothing in the (word, pixel) rules and in the VGG16
 * chain.  rows = null: all B*T rows (n_rows must be B*T). */
int lrpx_gridtd_rel_pix_rows(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* Vp,
                             const float* proj_pre, float* a_proj, const int32_t* rows, int n_rows, void* stream);
/* the same with the mean-of-projected-features term of the bottom-up model (models/gridTDmodel.py:1912-1915: the global feature is
 * relu(global_img_feature_proj(mean_k Vp[k])), so its relevance returns UNDER the projector rule): r_avg [B*T][H] is the relevance of
 * that mean (indexed by the full row, also with a row list), avg [B][H] the mean itself;
 * a_proj[row][k][c] = Vp[b][k][c] * (sum_i alpha[b][i][k] wacc[row][i][c] + r_avg[row][c] / (P z~(avg[b][c]))) / z~(proj_pre[b][k][c]) */
int lrpx_gridtd_rel_pix_rows_avg(const lrpx_gridtd_trace* tr, const lrpx_gridtd_relstate* rs, const float* Vp,
                                 const float* proj_pre, const float* r_avg, const float* avg, float* a_proj, const int32_t* rows,
                                 int n_rows, void* stream);
int lrpx_rel_words_norm(float* r_words, int rows, int T, void* stream);

/* ---- single-LSTM adaptive-attention decoder (models/adaptiveattention.py): trace (get_hidden_parameters, :626-677) ---------------- */
typedef struct lrpx_adaatt_trace {
    int B, T, H, E, P;
    float* xh;                          /* [B][T][H+2E] = [h[t] | emb(word_t) | glob]: the reference's xht (:688) with the h columns FIRST */
    float *h, *c;                       /* [B][T+1][H]; row 0 must be zero (init_hidden_state, :123-126) */
    float *g, *i, *f;                   /* [B][T][H]  g = pre-activation, i / f = activations (:672-674) */
    float *s, *ctx, *ctx_hat, *hc;      /* [B][T][H]  hc = h[t+1] + ctx_hat[t] (fc input, :663) */
    float *alpha, *beta;                /* [B][T][P], [B][T] */
    float *o, *sgate;                   /* optional [B][T][H]: output gate, sentinel gate (the gradient explainers' trace); may be null */
} lrpx_adaatt_trace;
/* The teacher-forced trace, decoupled: the recurrence reads h only (the attention feeds nothing back).
 *   fwd_inputs:        the x columns [emb | glob] of every (image, word) row of xh; the caller then forms
 *                      zin [B*T][NR] = xh[:, H:] Wx_il^T + b_il for all rows with lrpx_linear_small (K = 2E);
 *   fwd_recurrence:    T dependent launches of K = H: z = zin[b, t] + Wh_il h[b, t], LSTM cell (:554-565) and sentinel
 *                      s = sigmoid(z_gate) tanh(c_t) (:603-604) in the epilogue; writes the h columns of xh[b, t + 1].  B > 64 runs in slices;
 *   fwd_attention_all: AdaptiveAttention (:56-98) on (h[t+1], s[t]) of every row, ctx_hat and hc = h[t+1] + ctx_hat (two launches);
 *                      att_img [B][P][P] = W_v_proj(Vp) + b; scratch [B*T][3P].
 * Interleaved gate rows (Wx_il (NR, 2E), Wh_il (NR, H), b_il, zin columns), NR = 16 * ceil(H / 3): row 16 j + 5 u + q = gate q (i, f, g, o of
 * the LSTM, then the sentinel gate: [W_ih ; x_gate] / [W_hh ; h_gate] / b_ih + b_hh ; b_x + b_h) of hidden unit 3 j + u, u < 3; rows
 * 16 j + 15 and the rows of units >= H are zero. */
int lrpx_adaatt_fwd_inputs(const lrpx_adaatt_trace* tr, const float* glob, const float* emb, const long long* tok, int tok_ld,
                           void* stream);
int lrpx_adaatt_fwd_recurrence(const lrpx_adaatt_trace* tr, const float* w_hh_il, const float* zin, void* stream);
int lrpx_adaatt_fwd_attention_all(const lrpx_adaatt_trace* tr, const float* Vp, const float* att_img, const float* Wg, const float* Ws,
                                  const float* bs, const float* wh, float* scratch, void* stream);
/* Per-step entries (the decoding loops): fwd_pre writes row xh[b, t] = [h[b, t] | emb[tok[b][t]] | glob[b]]; fwd_step runs the gate
 * linear over the whole row (w_cat (5H, H+2E) = [W_hh | W_ih ; h_gate | x_gate], gates in blocks of H, b_cat its bias), cell + sentinel,
 * and the attention of step t.  Values equal the decoupled trace's to rounding (one dot product over [h | x] instead of two). */
typedef struct lrpx_adaatt_step_args {
    const float *w_cat, *b_cat;
    const float *Vp, *att_img;          /* relu(img_projector(features)) [B][P][H]; W_v_proj(Vp) + b [B][P][P] */
    const float *Wg, *Ws, *bs, *wh;     /* AdaAttention W_g_proj, W_s_proj (+ bias), w_h */
    float *zz, *att_scratch;            /* scratch [B][5H], [B][3P] */
} lrpx_adaatt_step_args;
int lrpx_adaatt_fwd_pre(const lrpx_adaatt_trace* tr, int t, const float* glob, const float* emb, const long long* tok, int tok_ld,
                        void* stream);
int lrpx_adaatt_fwd_step(const lrpx_adaatt_trace* tr, int t, const lrpx_adaatt_step_args* a, void* stream);

/* ---- single-LSTM adaptive-attention decoder: relevance (explain_caption_wordt, models/adaptiveattention.py:679-771) ---------------- */
typedef struct lrpx_adaatt_relstate {
    const int32_t* lens;                /* [B] words per image (null: T) */
    float *r_h, *r_c, *r_ctx;           /* [B*T][H]; r_ctx = r_context / z~(ctx_t), the factor of the pixel rule */
    float* r_glob;                      /* [B*T][E] */
    float *A, *rx;                      /* gate-rule input [B*T][H] / output [B*T][H+2E] = [h | emb | glob] */
    float* r_words;                     /* [B*T][T] */
} lrpx_adaatt_relstate;
/* :700-724 and the cell split of lock-step 0 (:726-734): fc rule from the target logit onto h[t+1] + ctx_hat[t], split by identity rules,
 * ctx_hat split into context ((1 - beta) ctx) and sentinel (beta s) - at the explained word only -, r_c[t+1] = r_s + r_h[t+1],
 * A = r_g / z~(tanh g[t]).  Rows behind an image's last word: zeros in A, r_ctx, r_glob, r_words. */
int lrpx_adaatt_rel_init(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, const float* fcw, const float* logit,
                         const long long* tok, int tok_ld, void* stream);
/* lock-steps 0 <= s < n_steps (:725-742) in one call; per lock-step the gate rule `dense` (an lrpx_conv_mfma descriptor: fp32, taps 1,
 * EPI_REL, in = A, x = tr->xh, out0 = rx, cin = H, n_oc = oc_split = H + 2E; weights [W_hh^g | W_ih^g] packed DENSE_T; map2img is
 * replaced by idx + s * idx_ld: row -> source row of the multiplicand) and one point-wise launch: r_h[i] = rx[:H], r_words[i] =
 * sum rx[H:H+E], r_glob = rx[H+E:] at s == 0 only (:740-741), then the cell split of lock-step s + 1.  Inactive rows: zeros in A, nothing
 * else touched.  cut_dead_columns != 0: lock-steps s >= 1 contract the first H + E columns only (the glob columns are never read
 * there); every column that is read is bit-identical to the full-width contraction. */
int lrpx_adaatt_rel_steps(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, int n_steps, const lrpx_conv_desc* dense,
                          const int32_t* idx, int idx_ld, int cut_dead_columns, void* stream);
/* a_glob[row][e] = r_glob[row][e] / z~(glob_nb[b][e]), glob_nb = W_gp avg WITHOUT the bias (:536-537, :743-746) */
int lrpx_adaatt_rel_glob(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, const float* glob_nb, float* a_glob, void* stream);
/* a_proj[x][k][c] = Vp[b][k][c] * alpha[b][t][k] * r_ctx[row][c] / z~(proj_nb[b][k][c]) for row = rows[x] (null: x, n_rows = B*T), written
 * compactly [n_rows][P][H]; proj_nb = the projector's pre-activation WITHOUT the bias (:751-763) */
int lrpx_adaatt_rel_pix_rows(const lrpx_adaatt_trace* tr, const lrpx_adaatt_relstate* rs, const float* Vp, const float* proj_nb,
                             float* a_proj, const int32_t* rows, int n_rows, void* stream);

/* ---- single-LSTM adaptive-attention decoder: gradient explainers (ExplainAdaptiveGradient.explain_caption_wordt,
 *      models/adaptiveattention.py:965-1021; the guided class's decoder part, :1100-1157, is the same function and Grad-CAM inherits it).
 *      The trace is an lrpx_adaatt_trace WITH o and sgate.  Only d_h = G_i W_hh is serial: r_words[i] = G_i . wsum with
 *      wsum[k] = sum_{e < E} W_ih[k][e], and d_glob = (sum_i G_i) W_ih[:, E:] - the caller's GEMM on gsum (csrc/lrpx_adaatt_grad.hip). -- */
typedef struct lrpx_adaptive_gradstate {
    const int32_t* lens;                /* [B] words per image (null: T) */
    float *d_ctx, *d_c;                 /* [B*T][H]: (1 - beta_t) d_h (:989); the running cell gradient */
    float *g0, *g1;                     /* [B*T][4H]: the gate gradients G_i (order i f g o) of even / odd lock-steps */
    float* gsum;                        /* [B*T][4H]: sum_i G_i */
    float* wpart;                       /* [B*T][T][H / 16]: per-workgroup partials of G_i . wsum */
    float* r_words;                     /* [B*T][T] (not normalised: lrpx_rel_words_norm) */
} lrpx_adaptive_gradstate;
/* :987-992 and the cell back-step of lock-step 0 (time index i = t): d_ctx, d_c, G_t into g0, gsum = G_t, the partials of r_words[t]; g1 is
 * cleared.  Rows behind an image's last word: exact zeros in d_ctx, d_c, g0, g1, gsum.  wsum: [4H].  tok_ld >= T + 1. */
int lrpx_adaptive_grad_init(const lrpx_adaatt_trace* tr, const lrpx_adaptive_gradstate* gs, const float* fcw, const long long* tok,
                            int tok_ld, const float* wsum, void* stream);
/* lock-steps 1 <= s < n_steps in one call, one launch each (row b*T + t works on time index i = t - s while s <= t < lens[b]):
 * d_h = G_{i+1} w_hh_t^T on the fp32 matrix cores (w_hh_t (H, 4H): row j = column j of W_hh) with the cell back-step (:996-1006) of the
 * workgroup's 16 hidden units in the epilogue - G_i into the other G buffer, d_c, gsum += G_i, its partial of G_i . wsum -; then one launch
 * that adds the partials in workgroup order into r_words (zeros behind word t and in inactive rows).  1 <= n_steps <= T. */
int lrpx_adaptive_grad_steps(const lrpx_adaatt_trace* tr, const lrpx_adaptive_gradstate* gs, int n_steps, const float* w_hh_t,
                             const float* wsum, void* stream);
/* d_feat[x][k][:] = alpha[b][t][k] v1[row][:] + d_avg[row][:] / P for row = rows[x] (null: x, n_rows must be B*T), written compactly
 * [n_rows][P][C] (:1013-1015; v1 = d_ctx W_proj [B*T][C], d_avg = d_glob W_gp [B*T][C]); zeros for a row behind its image's last word.
 * C % 4 == 0. */
int lrpx_adaptive_grad_pix_rows(const lrpx_adaatt_trace* tr, const lrpx_adaptive_gradstate* gs, const float* v1, const float* d_avg,
                                float* d_feat, int C, const int32_t* rows, int n_rows, void* stream);

/* ---- AoA decoder: trace (get_hidden_parameters, models/aoamodel.py:990-1062) -------------------------- */
typedef struct lrpx_aoa_trace {
    int B, T, H, E, P, NH;
    float* xh;                     /* [B][T][E+2H] = xt ++ ht[:T]  (:1075) */
    float *h, *c;                  /* [B][T+1][H] */
    float *g, *i, *f;              /* [B][T][H] */
    float *ctx, *lin, *c_aoa, *hc; /* [B][T][H]: context, decoder_aoa_linear(context), gated, fc input */
    float* alpha;                  /* [B][T][NH][P] */
    float *o, *sg;                 /* optional (gradient explainers, :1309-1376): [B][T][H] output gate, sigmoid(aoa gate) */
} lrpx_aoa_trace;
int lrpx_aoa_fwd_pre(const lrpx_aoa_trace* tr, int t, const float* glob, const float* emb, const long long* tok,
                     int tok_ld, void* stream);
int lrpx_aoa_fwd_lstm(const lrpx_aoa_trace* tr, int t, const float* zz, int ldz, void* stream);
/* qg: [B][2H] = [q_proj(h_t) | decoder_aoa_linear_gate(h_t)]; key/value: [B][P][H]  (MultiHeadedDotAttention, :77-108) */
int lrpx_aoa_fwd_attention(const lrpx_aoa_trace* tr, int t, const float* qg, int ldq, const float* key,
                           const float* value, void* stream);
int lrpx_aoa_fwd_post(const lrpx_aoa_trace* tr, int t, const float* qg, int ldq, const float* lin, void* stream);
/* decoder steps t0 <= t < t1 of get_hidden_parameters (models/aoamodel.py:1020-1052) in ONE call: per step fwd_pre, LSTM gate
 * linear, fwd_lstm, [q | aoa gate] linear, fwd_attention, decoder_aoa_linear, fwd_post - the `for t in range(...)` loop of
 * the reference (:1019) with its host side in native code */
typedef struct lrpx_aoa_step_args {
    const float *glob, *emb;            /* global image feature [B][H], embedding table */
    const long long* tok; int tok_ld;   /* token ids [B][tok_ld] (teacher forcing: the caption incl. <start>) */
    const float *w_cat, *b_cat;         /* LSTM [W_ih | W_hh] (4H x (E+2H)) and its bias (the explainers' quirk or the model's) */
    const float *w_cat_il, *b_cat_il;   /* optional: the same with the gate rows interleaved (row 16 j + 4 gate + u = row gate * H + 4 j + u):
                                           the steps then run fused, 4 launches instead of 7 (gate linear + LSTM cell; aoa_linear + gated
                                           sum + the next step's input row); results are bit-identical */
    const float *w_qg, *b_qg;           /* [q_proj ; decoder_aoa_linear_gate] (2H x H) */
    const float *w_lin, *b_lin;         /* decoder_aoa_linear (H x H) */
    const float *key, *value;           /* [B][P][H] */
    float *zz, *qg, *lin;               /* scratch [B][4H], [B][2H], [B][H] */
} lrpx_aoa_step_args;
int lrpx_aoa_fwd_steps(const lrpx_aoa_trace* tr, int t0, int t1, const lrpx_aoa_step_args* a, void* stream);
/* The teacher-forced trace with the recurrence decoupled from what hangs off it: in this model the LSTM reads x_t = [emb(word_t) |
 * global feature] and its own h_{t-1} only (models/aoamodel.py:1030-1033); attention, AoA gate and scores read h_t and feed nothing
 * back.  So: (1) lrpx_aoa_fwd_inputs gathers x_t of every (image, word) row (into xh and, contiguous, into xin [B*T][E+H]); the caller
 * forms zin = xin W_ih^T + b for all rows in one GEMM (columns in the interleaved gate order of w_cat_il above); (2)
 * lrpx_aoa_fwd_recurrence runs the T dependent steps  z = zin[t] + W_hh h_{t-1} -> LSTM cell, ONE launch of K = H each (w_hh_il:
 * (4H, H), rows interleaved); (3) lrpx_aoa_fwd_gather_h writes hn [B*T][H] = h_t rows and the h part of xh; the q / gate linear,
 * lrpx_aoa_fwd_attention_all, decoder_aoa_linear and lrpx_aoa_fwd_post_all then run ONCE over all B*T rows (qg [B*T][ldq] =
 * [q_proj(h_t) | aoa_linear_gate(h_t)], lin [B*T][H]).  Same trace tensors as the stepwise entry points (values equal to rounding:
 * z is (x W_ih^T + b) + W_hh h instead of one dot product over [x | h]). */
int lrpx_aoa_fwd_inputs(const lrpx_aoa_trace* tr, const float* glob, const float* emb, const long long* tok, int tok_ld,
                        float* xin, void* stream);
int lrpx_aoa_fwd_recurrence(const lrpx_aoa_trace* tr, const float* w_hh_il, const float* zin, void* stream);
/* the same with the input part from tables instead of a GEMM per trace: the embedding part of x_t W_ih^T depends on the token alone -
 * tab [V][4H] = embedding W_ie^T (interleaved gate order; once per MODEL), gimg [B][4H] = glob W_ig^T + bias (one small linear per
 * trace): z = (W_hh h + tab[tok[b, t]]) + gimg[b].  xin of lrpx_aoa_fwd_inputs may then be null. */
int lrpx_aoa_fwd_recurrence_tab(const lrpx_aoa_trace* tr, const float* w_hh_il, const float* tab, const float* gimg,
                                const long long* tok, int tok_ld, void* stream);
/* hn_amax / ctx_amax / hc_amax (optional, [B*T] words): float bits of max|row| of hn / ctx / hc, recorded by the kernel that writes
 * the row - the operand scales of the GEMMs that read it (ctx_amax must come zeroed: its 8 heads meet in an atomic maximum) */
int lrpx_aoa_fwd_gather_h(const lrpx_aoa_trace* tr, float* hn, uint32_t* hn_amax, void* stream);
int lrpx_aoa_fwd_attention_all(const lrpx_aoa_trace* tr, const float* qg, int ldq, const float* key, const float* value,
                               uint32_t* ctx_amax, void* stream);
int lrpx_aoa_fwd_post_all(const lrpx_aoa_trace* tr, const float* qg, int ldq, const float* lin, uint32_t* hc_amax, void* stream);

/* ---- AoA decoder: gradient explainers (ExplainAOAGradient.explain_caption_wordt, models/aoamodel.py:1435-1499;
 *      inherited unchanged by the guided / Grad-CAM variants) --------------------------------------------------- */
typedef struct lrpx_aoa_gradstate {
    const int32_t* lens;
    float *d_h, *d_c;              /* [B*T][H] */
    float *dA, *dB;                /* [B*T][H]: gradient into decoder_aoa_linear / decoder_aoa_linear_gate outputs (:1468-1470) */
    float *gates, *dx;             /* [B*T][4H] LSTM gate gradients / [B*T][E+2H] = gates @ [W_ih | W_hh] */
    float *d_glob;                 /* [B*T][H]   (assignment quirk :1487: the i = 0 step survives) */
    float* r_words;                /* [B*T][T] */
} lrpx_aoa_gradstate;
/* seed: d_h = fc.weight[target], dA, dB from the saved gate / linear outputs; needs tr->o and tr->sg */
int lrpx_aoa_grad_init(const lrpx_aoa_trace* tr, const lrpx_aoa_gradstate* gs, const float* fcw, const long long* tok,
                       int tok_ld, void* stream);
/* lock-step s (time index i = t - s): phase 0 LSTM cell backward -> gates; phase 1 after dx = gates @ [W_ih|W_hh] */
int lrpx_aoa_grad_step(const lrpx_aoa_trace* tr, const lrpx_aoa_gradstate* gs, int s, int phase, void* stream);
/* d_feat[row][p][:] = alpha[b,t,head,p] * v1[row][:] + v2[row][:]  (gradient_mha :1415-1433 folded through v_proj and
 * the projector: both are rank-1 in the pixel index) */
int lrpx_aoa_grad_pix(const lrpx_aoa_trace* tr, int head, const float* v1, const float* v2, float* d_feat, int C,
                      void* stream);
int lrpx_aoa_grad_pix_rows(const lrpx_aoa_trace* tr, int head, const float* v1, const float* v2, float* d_feat, int C,
                           const int32_t* rows, int n_rows, void* stream);   /* compact output for the listed rows */
/* x[row][c] = 0 for c outside [lo, hi)  (only one head passes gradient, :1428) */
int lrpx_keep_cols(float* x, long rows, int ncol, int lo, int hi, void* stream);

/* ---- AoA decoder: relevance (explain_caption_wordt :1064-1156, lrp_mha :812-862) ----------------------- */
typedef struct lrpx_aoa_relstate {
    const int32_t* lens;
    float *r_hn, *r_glob;          /* [B*T][H] */
    float *A, *rx;                 /* dense-rule input [B*T][H] / output [B*T][E+2H] */
    float* r_words;                /* [B*T][T] */
} lrpx_aoa_relstate;
int lrpx_aoa_rel_init(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* fcw, const float* logit,
                      const long long* tok, int tok_ld, void* stream);
int lrpx_aoa_rel_value(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* r_ctx, const float* value,
                       int head, float* a_val, void* stream);
int lrpx_aoa_rel_value_rows(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* r_ctx, const float* value,
                            int head, float* a_val, const int32_t* rows, int n_rows, void* stream);   /* compact a_val */
/* the same, only the head's H / NH non-zero columns: a_val_head [n_rows][P][H/NH] (rows = null: all B*T rows).  `lrp_mha` passes
 * relevance through ONE head (models/aoamodel.py:848-860), so the v_proj rule behind it contracts over that head's H/NH rows of W_v
 * (lrpx_pack_weights_f16x2 of the row slice) instead of over H with zeros in 7/8 of the operand: an eighth of the matrix work and of
 * the operand traffic, the same products in the same order (bit-identical). */
int lrpx_aoa_rel_value_head(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const float* r_ctx, const float* value,
                            int head, float* a_val_head, const int32_t* rows, int n_rows, void* stream);
/* lock-step s: phase 0 g-gate split (:1116-1120) -> A ; phase 1 after the LSTM dense rule (:1129-1133) */
int lrpx_aoa_rel_step(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, int s, int phase, void* stream);
/* lock-steps 0 <= s < n_steps of explain_caption_wordt's `for i in range(t+1)[::-1]` (models/aoamodel.py:1114-1134) in ONE
 * call: phase 0, the LSTM dense rule `dense` (an lrpx_conv_mfma descriptor whose map2img is replaced by idx + s * idx_ld:
 * row -> source row of its multiplicand), phase 1 */
int lrpx_aoa_rel_steps(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, int n_steps, const lrpx_conv_desc* dense,
                       const int32_t* idx, int idx_ld, void* stream);
/* All T lock-steps with ONE launch each: the step's point-wise code (:1116-1120 of the next step, :1129-1133 of this one) runs in the
 * epilogue of the gate rule's GEMM, r_xh is never stored.  `dense` as above (in = rs->A, no addend; E = H = 512) and either on the fp16
 * split products (f16x3 = 1: csrc/dense_f16x3.hip, FUSE) or - round 6, the exact arithmetic of the default mode - on the fp32 MFMA with K split
 * over four waves (f16x3 = 0, wpacked from lrpx_pack_weights(DENSE_T, kc = 32): csrc/dense_small.hip, dense_ks_kernel<REL, FUSE>); a_alt: a second [B*T][H] buffer (the steps ping-pong between rs->A and it);
 * wpart: [B*T][T][4] scratch for the partial sums of r_words; coef: [2 * B*T*H + B*T] floats of scratch (per-trace coefficient tables of
 * :1116-1120 and the rows' last active step).  rs->r_words comes out NORMALISED (lrpx_rel_words_norm included); rs->rx
 * and rs->r_hn are not used.  Values equal to the two-launch steps up to the summation order of r_words. */
int lrpx_aoa_rel_steps_fused(const lrpx_aoa_trace* tr, const lrpx_aoa_relstate* rs, const lrpx_conv_desc* dense, const int32_t* idx,
                             int idx_ld, float* a_alt, float* wpart, float* coef, void* stream);

/* ---- gridTD guided backprop, decoder side (ExplainiGridTDGuidedGradient.explain_caption_wordt,
 *      models/gridTDmodel.py:1588-1675): BPTT with alpha/beta constant ------------------------------------ */
typedef struct lrpx_gridtd_gradstate {
    const int32_t* lens;
    float *d_h2n, *d_c2, *d_c1, *d_ch0, *d_h2p; /* [B*T][H] */
    float* d_glob;                      /* [B*T][E] */
    float *gates, *dx;                  /* gate-gradient rows [B*T][4H] (GEMM input) / GEMM output [B*T][3H] */
    float* wacc;                        /* [B*T][T][H]  d_context per time step */
    float* r_words;                     /* [B*T][T] */
} lrpx_gridtd_gradstate;
int lrpx_gridtd_grad_init(const lrpx_gridtd_trace* tr, const lrpx_gridtd_gradstate* gs, const float* fcw,
                          const long long* tok, int tok_ld, void* stream);
/* phase 0: LanguageLSTM cell backward -> gates ; 1: after gates @ [W_ih|W_hh] -> AdaLSTM cell backward -> gates ;
 * 2: after gates @ W_ih of the AdaLSTM */
int lrpx_gridtd_grad_step(const lrpx_gridtd_trace* tr, const lrpx_gridtd_gradstate* gs, int s, int phase, void* stream);
/* a_proj[row][k][:] = sum_{i<=t} alpha[b][i][k] * wacc[row][i][:]   (:1642-1643) */
int lrpx_spread_pixels(const float* wacc, const float* alpha, const int32_t* lens, float* a_proj, int B, int T, int H,
                       int P, void* stream);
int lrpx_spread_pixels_rows(const float* wacc, const float* alpha, const int32_t* lens, float* a_proj, int B, int T, int H,
                            int P, const int32_t* rows, int n_rows, void* stream);   /* compact a_proj for the listed rows */
int lrpx_scale(const float* x, float* y, long n, float alpha, void* stream);
int lrpx_positive_mask(const float* x, float* y, long n, void* stream);   /* y = [x > 0]  (:1674) */

/* ---- VGG16 guided backprop (explain_cnn, models/gridTDmodel.py:1677-1723) ------------------------------ */
/* d_feat (N,196,512) NHWC gradient at the encoder output -> (N,3,224,224) NCHW image gradient with the guided
 * ReLU rule clamp(g,min=0)*[relu_out>0] at every ReLU.  Same trace / workspace as lrpx_vgg16_relevance. */
int lrpx_vgg16_guided_backprop(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc,
                               const int32_t* map2img, int n_maps, void* workspace, float* out_nchw, void* stream);
/* ExplainGridTDGradient.explain_cnn (models/gridTDmodel.py:1507-1521): the plain autograd gradient of the encoder
 * output w.r.t. the image, `image_feature.backward(d_img_feature)`; same arguments as the guided variant. */
int lrpx_vgg16_gradient(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc,
                        const int32_t* map2img, int n_maps, void* workspace, float* out_nchw, void* stream);
/* ExplainGridTDGradCam.grad_cam (models/gridTDmodel.py:1760-1771): feats (n_img,P,C) NHWC, grads (rows,P,C) ->
 * cam (rows,P) = relu(sum_c feats_c * mean_p grads_c) / (max + 1e-6); P <= 256. */
int lrpx_gradcam(const float* feats, const float* grads, const int32_t* map2img, float* cam, int rows, int P, int C,
                 void* stream);

/* ---- rules of the layers the VGG16 path never reaches (ResNet encoders), csrc/lrpx_rules.hip ---- */
/* Linear.propagate_relevance, epsilon rule (LRPtools/lrp_modules.py:9-37).  x [n_rows][n_in] is the layer's SAVED input
 * and is mutated in place like the reference's (:14): exact zeros become RELEVANCE_RECT = -1e-6.  Z = x W^T; with
 * bias == NULL (ignore_bias, the preset of lrp_wrapper.py:7-12) Z += 0.01 sign(Z), exact zeros -> 0.01; otherwise
 * Z += bias (:20-21).  r_in = x * ((r_out / Z) W).  w [n_out][n_in] as nn.Linear stores it; s_ws: workspace of
 * n_rows * n_out floats (S = r_out / Z).  Any sizes. */
int lrpx_linear_eps_rule(float* x, const float* w, const float* bias, const float* r_out, float* s_ws, float* r_in,
                         int n_rows, int n_in, int n_out, void* stream);
/* BatchNorm2d / BatchNorm1d.propagate_relevance, method != 'identity' (LRPtools/lrp_modules.py:197-246):
 * r_in = safe_divide(|x w|, |x w| + |b|) * r_out with w = gamma / sqrt(var + eps), b = beta - mean gamma / sqrt(var + eps).
 * The result has n_outer * channels * inner elements, element e in channel (e / inner) % channels.  broadcast_x = 0: x and
 * r_out have the same shape (BatchNorm2d on (N,C,H,W): n_outer = N, inner = H*W).  broadcast_x = 1 (n_outer = 1): x and
 * r_out hold `inner` elements and are indexed by e % inner - what the reference's `[:, None, None]` indexing makes of a
 * (N,C) or (1,C,L) input of BatchNorm1d (:236-238): a (C, N, C) / (C, C, L) result. */
int lrpx_batchnorm_rule(const float* x, const float* r_out, const float* gamma, const float* beta, const float* mean,
                        const float* var, float eps, float* r_in, long n_outer, int channels, long inner, int broadcast_x,
                        void* stream);
/* Add.propagate_relevance (LRPtools/lrp_modules.py:256-280): r_k = r_out x_k / (x1 + x2 + 0.01 sign(x1 + x2)), NaN -> 0,
 * plus r_out / 2 each where x1 + x2 == 0.  Non-finite results (x1 == -x2 != 0) are left for lrpx_check, as the reference's
 * asserts (:276-279) catch them. */
int lrpx_add_rule(const float* x1, const float* x2, const float* r_out, float* r1, float* r2, long n, void* stream);
/* Pool2d.propagate_relevance for nn.AvgPool2d (LRPtools/lrp_modules.py:176-177,182-195; table entry :327): Z = avgpool(x),
 * S = r_out / (Z + 1e-7 [Z == 0]) (utils.py:16-18), r_in = x * avgpool^T(S).  x / r_in: (planes, h, w), r_out: (planes, oh, ow) with
 * planes = N * C of the module's NCHW tensors; s_ws: planes * oh * ow floats of scratch.  Window bounds, divisor
 * (count_include_pad, divisor_override > 0, ceil_mode through oh / ow) and summation orders follow ATen's CPU kernels:
 * bit-exact against the reference. */
int lrpx_avgpool_rule(const float* x, const float* r_out, float* s_ws, float* r_in, long planes, int h, int w, int oh, int ow,
                      int kh, int kw, int sh, int sw, int ph, int pw, int count_include_pad, int divisor_override, void* stream);
/* Pool2d.propagate_relevance for nn.MaxPool2d of any kernel / stride / padding / ceil_mode, dilation 1 (LRPtools/lrp_modules.py:174-175,
 * 182-195): Z = maxpool(x), S = r_out / (Z + 1e-7 [Z == 0]), r_in = x * maxpool^T(S).  x / r_in: (planes, h, w), r_out: (planes, oh, ow),
 * planes = N * C of the module's NCHW tensors (ceil_mode travels in oh / ow).  Padding is -inf; a window's winner is its FIRST
 * maximum in ATen's scan order (kernel rows outer, columns inner; a NaN wins); an input pixel that wins several overlapping windows
 * collects all of them, added in ascending (oh, ow) order as ATen's backward does.  Written as a gather per input pixel over the
 * windows that contain it: no atomics, no workspace. */
int lrpx_maxpool_rule(const float* x, const float* r_out, float* r_in, long planes, int h, int w, int oh, int ow, int kh, int kw,
                      int sh, int sw, int ph, int pw, void* stream);
/* ---- elementwise kernels of the batched bottleneck-ResNet engine (csrc/resnet_engine.hip; NHWC fp32, one pass each) -----------
 * Trace, once per image.  yz: `rows` pixel rows of `ld` >= 2c floats, columns [0,c) the conv's output y, [c,2c) Z of its rule
 * (conv(x,W+); the stem: conv(x+,W+) + conv(x-,W-), lrp_modules.py:81-84).  w / b [c]: the folded eval-mode BatchNorm scale and
 * shift (lrp_modules.py:210-211).  act [rows][c] = y w + b (relu != 0: max(., 0), models/resnet.py:122-131);  q [rows][c] =
 * safe_divide(|y w|, |y w| + |b|) / (Z + 1e-7 [Z == 0]): BatchNorm2d.propagate_relevance (:212-215) times the divisor of
 * utils.safe_divide inside lrp_backward (utils.py:16-18,28) - everything between R at the BN's output and S of the conv. */
int lrpx_resnet_bn_act_coef(const float* yz, int ld, const float* w, const float* b, float* act, float* q, long rows, int c, int relu,
                            void* stream);
/* The second coefficient of the general alpha-beta rule (lrpx_conv_geom_ab): yz columns [0,c) the conv's output y, [c,2c) Z- =
 * conv(x,W-) (the stem: conv(x+,W-) + conv(x-,W+));  qn [rows][c] = safe_divide(|y w|, |y w| + |b|) / (Z- + 1e-7 [Z- == 0]), the
 * fraction evaluated as lrpx_resnet_bn_act_coef evaluates it.  Independent of alpha / beta: once per image. */
int lrpx_resnet_coef_neg(const float* yz, int ld, const float* w, const float* b, float* qn, long rows, int c, void* stream);
/* out = max(x1 + x2, 0) (models/resnet.py:137-138) and the coefficients of Add.propagate_relevance (lrp_modules.py:262-275):
 * c_k = x_k / (x1 + x2 + 0.01 sign(x1 + x2)), NaN -> 0, + 0.5 where x1 + x2 == 0, so that R_k = R c_k.  (x1 == -x2 != 0, where the
 * reference's result is non-finite and its asserts fire, gives 0.5.)  n elements each. */
int lrpx_resnet_add_relu_coef(const float* x1, const float* x2, float* out, float* c1, float* c2, long n, void* stream);
/* nn.MaxPool2d forward on NHWC (models/resnet.py:168,225): x [n][h*w][c] -> y [n][oh*ow][c]; padding is -inf, a NaN wins. */
int lrpx_resnet_maxpool_fwd(const float* x, float* y, int n, int h, int w, int oh, int ow, int c, int kh, int kw, int sh, int sw, int ph,
                            int pw, void* stream);
/* Relevance, per map; per-image operands are read from image map2img[m] (int32 [n_maps], entries in [0, n_img) validated by the
 * caller; NULL: n_maps == n_img, map m on image m).
 * Pool2d.propagate_relevance for nn.MaxPool2d (lrp_modules.py:182-195) in NHWC: x [n_img][h*w][c], r_out [n_maps][oh*ow][c] ->
 * r_in [n_maps][h*w][c].  A gather per input element with the winner logic of lrpx_maxpool_rule (first maximum, kernel rows outer;
 * windows added in ascending (oh, ow) order); the winners are recomputed from x, no atomics, no workspace. */
int lrpx_resnet_maxpool_rel(const float* x, const float* r_out, const int32_t* map2img, float* r_in, int n_maps, int n_img, int h, int w,
                            int oh, int ow, int c, int kh, int kw, int sh, int sw, int ph, int pw, void* stream);
/* Add.propagate_relevance (lrp_modules.py:262-275) behind the block's final ReLU (identity rule, :42-46): r1 = r c1[img],
 * r2 = r c2[img] with the coefficients of lrpx_resnet_add_relu_coef; r / r1 / r2 [n_maps][per_map], c1 / c2 [n_img][per_map]. */
int lrpx_resnet_add_split(const float* r, const float* c1, const float* c2, const int32_t* map2img, float* r1, float* r2, int n_maps,
                          int n_img, long per_map, void* stream);
/* the stem's signed-input rule R = x+ convT(S,W+) + x- convT(S,W-) (lrp_modules.py:81-84,136-138): r_split [n_maps][pix][ld]
 * holds the two terms in columns [0,cin) and [half, half+cin), half + cin <= ld (the layout of lrpx_nchw_to_nhwc_posneg: half = cin);
 * out [n_maps][cin][pix] (NCHW) = their sum. */
int lrpx_resnet_stem_fold(const float* r_split, float* out, int n_maps, int cin, int half, int ld, long pix, void* stream);
/* Gradient chain, per map, per-image operands through map2img as above.
 * ReLU backward at a block's output: out = (clamp ? max(g, 0) : g) * (act[img] > 0); g / out [n_maps][per_map], act [n_img][per_map]
 * the ReLU's output.  clamp 1 is guided backprop at this ReLU.  out may be g. */
int lrpx_resnet_relu_grad(const float* g, const float* act, const int32_t* map2img, float* out, int n_maps, int n_img, long per_map,
                          int clamp, void* stream);
/* nn.MaxPool2d backward in NHWC: x [n_img][h*w][c] the pool's input, g_out [n_maps][oh*ow][c] -> g_in [n_maps][h*w][c]: each window's
 * gradient goes to its first maximum (kernel rows outer, a NaN wins) - the gather and winner logic of lrpx_resnet_maxpool_rel without
 * the division and without the x factor; windows added in ascending (oh, ow) order, no atomics, no workspace. */
int lrpx_resnet_maxpool_grad(const float* x, const float* g_out, const int32_t* map2img, float* g_in, int n_maps, int n_img, int h, int w,
                             int oh, int ow, int c, int kh, int kw, int sh, int sw, int ph, int pw, void* stream);
/* max |a - b| into one device float (Dropout.propagate_relevance's check, LRPtools/lrp_modules.py:251; NaN counts as inf) */
int lrpx_max_abs_diff(const float* a, const float* b, long n, float* out_dev, void* stream);

/* Guided-Grad-CAM (ExplainGridTDGuidedGradCam.explain_cnn, models/gridTDmodel.py:1814-1836; AoA: models/aoamodel.py:1729-1751):
 * out[n][c] = guided[n][c] * E_n with E_n = expand_m cam_n expand_m^T, the (hw x hw) `skimage.transform.pyramid_expand(cam,
 * upscale = hw / p)` of the (p x p) Grad-CAM heat map cam_n.  guided / out: (rows, channels, hw, hw); cam: (rows, p*p);
 * expand_m: (hw, p) row-major, Gaussian smoothing x bilinear resize as ONE matrix (both steps are linear and separable;
 * built on the host by lrp_amd.ops.pyramid_expand_matrix). */
int lrpx_guided_gradcam(const float* guided, const float* cam, const float* expand_m, float* out, int rows, int p, int hw,
                        int channels, void* stream);
/* Feature-resolution heat maps at image size (attention maps evaluation.py:198-211, :390-400, :483-494, :744-750; 2-D Grad-CAM maps
 * :125-132, :401-407, :496-501): out_n = E_n = expand_m a_n expand_m^T, the factor lrpx_guided_gradcam multiplies by, bit for bit.
 * maps: (rows, heads, p*p); a_n is head `head` (>= 0) or, head == -1, the mean over the heads (fp32 sum in head order, one division;
 * heads == 1 copies).  normalize == 1: every map divided by its max |E| as lrpx_project_maxabs would (same bits; all-zero maps stay
 * zero); out (rows, hw, hw) is written exactly once either way.  p in 2..32, hw a multiple of p, (hw * 4 * ceil(p / 4) + p*p + 16)
 * floats of LDS at most 64 KiB; anything else, a bad head / heads and null pointers are LRPX_EINVAL before any launch. */
int lrpx_expand_maps(const float* maps, const float* expand_m, float* out, int rows, int heads, int head, int p, int hw, int normalize,
                     void* stream);

/* ---- the VGG16 chains with a per-call context (see THREADING above): same arguments + opts (NULL = process defaults) -- */
int lrpx_vgg16_forward_ex(const void* packed, const float* img_nchw, int n_img, void* trace, float* feat_nhwc,
                          const lrpx_vgg16_opts* opts, void* stream);
int lrpx_vgg16_relevance_ex(const void* packed, const void* trace, int n_img, const float* r_feat_nhwc,
                            const int32_t* map2img, int n_maps, void* workspace, float* out_nchw,
                            const lrpx_vgg16_opts* opts, void* stream);
int lrpx_vgg16_guided_backprop_ex(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc,
                                  const int32_t* map2img, int n_maps, void* workspace, float* out_nchw,
                                  const lrpx_vgg16_opts* opts, void* stream);
int lrpx_vgg16_gradient_ex(const void* packed, const void* trace, int n_img, const float* d_feat_nhwc,
                           const int32_t* map2img, int n_maps, void* workspace, float* out_nchw,
                           const lrpx_vgg16_opts* opts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
