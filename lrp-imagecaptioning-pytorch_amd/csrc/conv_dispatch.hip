// Conv dispatch of liblrpx: which kernel a descriptor runs on (conv_select: host code, no HIP call) and its launch (conv_dispatch).
// The fixed-geometry conv kernels are the rows of conv_kernels.def; this file holds no device code.
#include "conv_launch.h"

namespace lrpx {

#define UNIT(unit, header)
#define LRPX_STAMP_READER(unit)
#define LRPX_STAMP_READER_X6
#define K(name, ...) int launch_##name(const ConvArgs& a, hipStream_t s);      // defined in conv_inst_<unit>.hip
#include "conv_kernels.def"
#undef K
#define K(name, family, hw, epi, variant, oc_min, oc_max, ...) {#name, launch_##name, family, hw, epi, variant, oc_min, oc_max},
static constexpr ConvKernel kConvKernels[] = {
#include "conv_kernels.def"
};
#undef K
static constexpr int kNumConvKernels = sizeof(kConvKernels) / sizeof(kConvKernels[0]);

static constexpr bool row_takes(const ConvKernel& k, int family, int hw, int epi, int variant, int n_oc) {
    return k.family == family && k.hw == hw && k.epi == epi && k.variant == variant && k.oc_min <= n_oc && n_oc <= k.oc_max;
}
// no descriptor matches two rows: rows with the same (family, hw, epilogue, variant) have disjoint channel ranges
static constexpr bool rows_disjoint() {
    for (int i = 0; i < kNumConvKernels; ++i)
        for (int j = i + 1; j < kNumConvKernels; ++j) {
            const ConvKernel &p = kConvKernels[i], &q = kConvKernels[j];
            if (p.family == q.family && p.hw == q.hw && p.epi == q.epi && p.variant == q.variant && p.oc_min <= q.oc_max && q.oc_min <= p.oc_max) return false;
        }
    return true;
}
static_assert(rows_disjoint(), "conv_kernels.def: two rows take the same descriptor");

// the dense GEMMs (taps = 1) that do not run on a conv kernel: dense_f16x3.hip, dense_small.hip.  conv_select names them itself, before
// it looks at the list: only their name and launcher are used, the predicate fields mean nothing
static constexpr ConvKernel kDenseBf16x6{"dense_bf16x6", launch_dense_bf16x6, FAM_B6, 0, EPI_REL, VAR_DIRECT, 1, OC_ANY};
static constexpr ConvKernel kDenseF16x3{"dense_f16x3", launch_dense_f16x3, FAM_H3, 0, EPI_REL, VAR_DIRECT, 1, OC_ANY};
static constexpr ConvKernel kDenseSmallF16x3{"dense_small_f16x3", launch_dense_small_f16x3, FAM_H3, 0, EPI_REL, VAR_DIRECT, 1, OC_ANY};
static constexpr ConvKernel kDenseSmall{"dense_small", launch_dense_small, FAM_FP32, 0, EPI_REL, VAR_DIRECT, 1, OC_ANY};

struct ConvChoice {
    ConvArgs a;
    const ConvKernel* k = nullptr;
    int matches = 0;             // rows of the list that take the descriptor (1, or 0 on the dense routes)
    size_t clear_bytes = 0;      // atomic K split: a.out0 is zeroed before the launch
};

// validation and selection: fills c or refuses (LRPX_EINVAL + last-error text).  Touches no memory behind the descriptor's pointers.
static int conv_select(const lrpx_conv_desc* d, int f16_ksplit, ConvChoice& c) {
    LRPX_REQUIRE(d && d->in && d->wpacked && (d->out0 || d->out1), "conv_mfma: null pointer");
    LRPX_REQUIRE(d->taps == 9 || d->taps == 1, "conv_mfma: taps must be 9 or 1");
    LRPX_REQUIRE(d->taps == 1 || d->hw == 224 || d->hw == 112 || d->hw == 56 || d->hw == 28 || d->hw == 14,
                 "conv_mfma: hw=%d: the 3x3 kernels are built for 224 / 112 / 56 / 28 / 14-pixel maps", d->hw);
    LRPX_REQUIRE(d->n_maps > 0 && d->cin > 0 && d->n_oc > 0 && d->n_oc % 32 == 0, "conv_mfma: bad sizes (n_oc %% 32)");
    const int kc = (d->bf16x6 || d->f16x3) ? 16 : lrpx_conv_kc(d->hw, d->taps, d->cin);
    LRPX_REQUIRE(kc > 0 && d->cin % kc == 0, "conv_mfma: cin=%d is not a multiple of the K-chunk %d", d->cin, kc);
    ConvArgs& a = c.a;
    a.in = d->in; a.wp = d->wpacked; a.n_maps = d->n_maps; a.cin = d->cin; a.n_oc = d->n_oc;
    a.pix_per_map = d->taps == 9 ? d->hw * d->hw : d->pix_per_map;
    a.in_chunk_stride = d->in_chunked ? (long)d->n_maps * a.pix_per_map * kc : 0;
    a.epi = d->epi; a.stab = d->stab; a.oc_split = d->oc_split; a.relu = d->relu;
    a.bias = d->bias; a.X = d->x; a.U = d->u; a.Zdiv = d->zdiv; a.map2img = d->map2img;
    a.out0 = d->out0; a.out1 = d->out1;
    a.in_amax = d->in_amax; a.out1_amax = d->out1_amax; a.pool_am = d->pool_am; a.out0_amax = d->out0_amax;
    a.out_chunk = d->epi == EPI_REL_MUL ? d->out_chunk : 0;
    a.tile_group = ((d->f16x3 || (d->bf16x6 && (d->epi == EPI_REL_MUL || d->epi == EPI_GUIDED))) && d->tile_group > 1 && d->n_maps % d->tile_group == 0) ? d->tile_group : 0;
    a.ksplit = 1;
    // many rows (the (word, pixel) rules of the decoders): split products on the fp16 matrix cores (dense_f16x3.hip);
    // `wpacked` is then an lrpx_pack_weights_f16x2 blob (taps = 1) and `in_amax` holds max|in| per map
    // ... or, with operands split EXACTLY into three bf16 parts (the default arithmetic of the path: nothing narrower than fp32), on the
    // bf16 matrix cores: `wpacked` from lrpx_pack_weights_bf16x3 (taps = 1), no in_amax, any number of rows
    if (d->taps == 1 && d->bf16x6) {
        LRPX_REQUIRE(!d->f16x3 && d->epi == EPI_REL && d->x && d->pix_per_map > 0, "conv_mfma: the dense bf16x6 GEMM is built for the REL epilogue (x, pix_per_map)");
        c.k = &kDenseBf16x6;
        return LRPX_OK;
    }
    if (d->taps == 1 && d->f16x3 && d->epi == EPI_PLAIN) {
        // out0 = in W^T + bias on the fp16 matrix cores (the (T,V) scores of a trace): weights from lrpx_pack_weights_f16x2(PACK_FWD,
        // taps = 1), in_amax = max|in| per map (rows of a map share one operand scale; pix_per_map = 1: per row)
        LRPX_REQUIRE(d->f16x3 == 1 && d->in_amax && d->pix_per_map > 0 && d->out0 && !d->out1,
                     "conv_mfma: the dense f16x3 PLAIN GEMM needs in_amax, pix_per_map and out0");
        c.k = &kDenseF16x3;
        return LRPX_OK;
    }
    if (d->taps == 1 && d->f16x3) {
        LRPX_REQUIRE(d->f16x3 == 1 && d->epi == EPI_REL && d->x && d->pix_per_map > 0,
                     "conv_mfma: the dense f16x3 GEMMs are built for the REL / PLAIN epilogues (REL needs x, pix_per_map)");
        // few rows (the lock-step gate rules): whole K per workgroup, per-row operand scales found while staging
        if ((long)d->n_maps * d->pix_per_map <= 4096 && d->cin <= 1024 && !d->out1) {
            c.k = &kDenseSmallF16x3;
            return LRPX_OK;
        }
        LRPX_REQUIRE(d->in_amax, "conv_mfma: the many-row dense f16x3 GEMM needs in_amax (max|in| per map)");
        LRPX_REQUIRE(!d->out1 || d->zdiv || d->stab == STAB_NONE, "conv_mfma: REL out1 needs zdiv");
        c.k = &kDenseF16x3;
        return LRPX_OK;
    }
    // few rows (the decoder's lock-step rules): 32-row tiles, whole K per workgroup (dense_small.hip)
    if (d->taps == 1 && dense_small_fits(a)) {
        LRPX_REQUIRE(d->epi != EPI_REL || d->x, "conv_mfma: REL needs x");
        c.k = &kDenseSmall;
        return LRPX_OK;
    }
    // dense GEMMs with few rows are latency-bound by one wave's serial MFMA chain over K: split K over blockIdx.y and
    // add the partial results atomically (outputs zeroed first).  Only where the epilogue is linear in the accumulator.
    if (d->taps == 1 && (long)d->n_maps * a.pix_per_map <= 2048 && d->cin >= 4 * kc && !d->out1 &&
        ((d->epi == EPI_REL) || (d->epi == EPI_PLAIN && !d->relu))) {
        a.ksplit = d->cin / kc >= 16 ? 4 : 2;
        c.clear_bytes = (size_t)d->n_maps * a.pix_per_map * d->oc_split * sizeof(float);
    }
    LRPX_REQUIRE(a.pix_per_map > 0, "conv_mfma: pix_per_map must be positive");
    LRPX_REQUIRE((long)a.n_maps * a.pix_per_map < 0x7fffffffL, "conv_mfma: too many pixels for 32-bit indexing");
    switch (d->epi) {
        case EPI_FWD_DUAL: LRPX_REQUIRE(d->out0 && d->out1 && 2 * d->oc_split <= d->n_oc, "conv_mfma: FWD_DUAL needs out0,out1"); break;
        case EPI_REL: LRPX_REQUIRE(d->x && (d->out0 || d->out1) && (!d->out1 || d->zdiv || d->stab == STAB_NONE), "conv_mfma: REL needs x and (out0|out1,zdiv)"); break;
        case EPI_FIRST: LRPX_REQUIRE(d->x && d->out0, "conv_mfma: FIRST needs x,out0"); break;
        case EPI_PLAIN: LRPX_REQUIRE(d->out0, "conv_mfma: PLAIN needs out0"); break;
        case EPI_GUIDED: LRPX_REQUIRE(d->out0 && d->x, "conv_mfma: GUIDED needs x,out0"); break;
        case EPI_REL_MUL: LRPX_REQUIRE(d->x && (d->f16x3 || d->bf16x6) && (!d->out0 != !d->out1), "conv_mfma: REL_MUL is the epilogue of the split-product kernels (f16x3 / bf16x6; needs x and exactly one of out0 / out1)"); break;
        default: LRPX_REQUIRE(false, "conv_mfma: epilogue %d not built", d->epi);
    }
    const int family = d->f16x3 ? (d->f16x3 == 2 ? FAM_H8 : FAM_H3) : (d->bf16x6 ? FAM_B6 : FAM_FP32);
    int variant = VAR_DIRECT;
    if (d->f16x3) {
        LRPX_REQUIRE(d->taps == 9 && d->cin % 16 == 0 && d->in_amax && !d->bf16x6 &&
                         ((d->epi == EPI_REL_MUL && d->x) || (d->epi == EPI_GUIDED && d->f16x3 == 2 && d->x) ||
                          ((d->epi == EPI_FWD_DUAL || d->epi == EPI_GUIDED || (d->epi == EPI_PLAIN && !d->relu && !d->bias)) &&
                           !d->pool_am)),
                     "conv_mfma: f16x3 needs a 3x3 conv, cin %% 16 == 0, in_amax and the REL_MUL (with x), FWD_DUAL, GUIDED "
                     "or bias-free PLAIN epilogue");
        LRPX_REQUIRE(d->f16x3 != 2 || d->epi == EPI_REL_MUL || d->epi == EPI_GUIDED || d->epi == EPI_PLAIN,
                     "conv_mfma: the f16+f8 kernels (f16x3 = 2) are built for the REL_MUL, GUIDED and PLAIN epilogues");
        // the mode-3 relevance kernels (f16x3 = 2, REL_MUL) take `in` in the BLOCKED layout (blocked.h, lrpx_nhwc_to_blocked) and, except the
        // 224 x 224 one (conv1_2: NHWC multiplicand, NHWC / channel-chunked output for the first-layer kernel), x and the output too;
        // everything else takes NHWC
        if (d->f16x3 == 2 && d->epi == EPI_REL_MUL) {
            if (d->hw == 224)
                LRPX_REQUIRE(d->blocked == 1 && !d->in_chunked, "conv_mfma: the 224x224 f16x3 = 2 REL_MUL kernel takes `in` blocked (blocked = 1), x / out NHWC");
            else
                LRPX_REQUIRE(d->blocked == 7 && d->oc_split % 16 == 0 && !d->in_chunked && !d->out_chunk,
                             "conv_mfma: f16x3 = 2 with REL_MUL takes in / x / out in the blocked layout (blocked = 7, oc_split %% 16 == 0, no chunk options)");
        } else {
            LRPX_REQUIRE(d->blocked == 0, "conv_mfma: only the f16x3 = 2 REL_MUL kernels take the blocked layout");
        }
        if (d->pool_am) variant = VAR_POOL;
    } else if (d->bf16x6) {
        LRPX_REQUIRE(d->taps == 9 && d->cin % 16 == 0, "conv_mfma: bf16x6 needs a 3x3 conv, cin %% 16 == 0");
        LRPX_REQUIRE(d->blocked == 0 && (!d->pool_am || d->epi == EPI_REL_MUL || d->epi == EPI_GUIDED),
                     "conv_mfma: bf16x6 takes NHWC tensors; pool_am needs the REL_MUL or GUIDED epilogue");
        if (d->epi == EPI_PLAIN)
            LRPX_REQUIRE(d->hw <= 56 && !d->relu && !d->bias, "conv_mfma: the bf16x6 PLAIN kernels are built for 56 / 28 / 14-pixel maps, no bias / ReLU (the K-split forward)");
        // (the act | Z+ halves of a tile's 32-channel output blocks must not straddle oc_split)
        if (d->epi == EPI_FWD_DUAL)
            LRPX_REQUIRE(d->oc_split % 32 == 0, "conv_mfma: the bf16x6 FWD_DUAL kernels need oc_split %% 32 == 0 (oc_split=%d)", d->oc_split);
        if (d->pool_am) {
            // the conv sits under a 2x2 max-pool: `in` at the pool's output resolution, unpooled while staged (conv_f16x3.h, POOL + B6)
            variant = VAR_POOL;
        } else if (d->epi == EPI_REL_MUL && d->wpacked_wino && !d->in_chunked && d->n_oc % 64 == 0 && d->hw <= 56 &&
                   (b6_wino_bits() & (d->hw == 56 ? 1 : (d->hw == 28 ? 2 : 4)))) {
            // Winograd F(2x2,3x3) on the same exact splits (conv_wino_b6.h): chosen by the layer's map size, never by the batch.
            // LRPX_B6_WINO / lrpx_set_b6_wino bit 8 (on by default): every staging thread fetches its whole patch; off: column sharing
            a.wp = reinterpret_cast<const float*>(d->wpacked_wino);
            variant = (b6_wino_bits() & 8) ? VAR_WINO_OWN : VAR_WINO_SHARE;
        }
    } else if (d->taps == 1) {
        LRPX_REQUIRE(d->epi == EPI_REL || d->epi == EPI_PLAIN, "conv_mfma: dense supports REL / PLAIN epilogues only");
    }
    if (family != FAM_FP32) {
        // (internal: K split of the PLAIN epilogue, partial sums per split behind each other in out0)
        a.ksplit = (d->epi == EPI_PLAIN && f16_ksplit > 1 && (d->cin / 16) % f16_ksplit == 0) ? f16_ksplit : 1;
        // the kernels index pool_am with 32-bit element offsets (image * pooled pixels * channels)
        LRPX_REQUIRE(variant != VAR_POOL || (long)d->n_maps * (d->hw / 2) * (d->hw / 2) * d->cin < 0x7fffffffL,
                     "conv_mfma: too many (image, pooled pixel, channel) elements for the pooled-input kernel");
    }
    // (the fp32 kernels never read pool_am: it does not select among them)
    const int hw = d->taps == 9 ? d->hw : 0;
    for (const ConvKernel& k : kConvKernels)
        if (row_takes(k, family, hw, d->epi, variant, d->n_oc)) {
            c.k = &k;
            ++c.matches;
        }
    static const char* const fam_name[] = {"fp32", "bf16x6", "f16x3", "f16+f8"};
    static const char* const epi_name[] = {"FWD_DUAL", "REL", "FIRST", "PLAIN", "GUIDED", "REL_MUL"};
    LRPX_REQUIRE(c.matches > 0, "conv_mfma: no %s%s %s kernel built for hw=%d n_oc=%d",
                 variant == VAR_POOL ? "pooled-input " : (variant == VAR_DIRECT ? "" : "Winograd "), fam_name[family], epi_name[d->epi], d->hw, d->n_oc);
    // (cannot happen: rows_disjoint above.  Kept as the run-time face of that assertion for tests/test_conv_table_host.py)
    LRPX_REQUIRE(c.matches == 1, "conv_mfma: %d rows of conv_kernels.def take hw=%d n_oc=%d", c.matches, d->hw, d->n_oc);
    return LRPX_OK;
}

int conv_dispatch(const lrpx_conv_desc* d, hipStream_t s, int f16_ksplit) {
    ConvChoice c;
    LRPX_TRY(conv_select(d, f16_ksplit, c));
    if (c.clear_bytes) LRPX_TRY(clear_async(c.a.out0, c.clear_bytes, s));
    return c.k->launch(c.a, s);
}

}  // namespace lrpx

extern "C" {

int lrpx_conv_kc(int hw, int taps, int cin) {
    if (taps == 1) return 32;
    (void)cin;
    if (hw >= 112) return 8;    // two LDS buffers of (rows+halo) x (W+2) pixels must fit: narrower chunks on wide maps
    return 16;
}

int lrpx_conv_mfma(const lrpx_conv_desc* d, void* stream) {
    LRPX_REQUIRE(d, "conv_mfma: null descriptor");
    LRPX_CHECK_PTRS("lrpx_conv_mfma", {d->in, "in"}, {d->wpacked, "wpacked"}, {d->bias, "bias"}, {d->x, "x"}, {d->u, "u"}, {d->zdiv, "zdiv"},
                    {d->map2img, "map2img"}, {d->out0, "out0"}, {d->out1, "out1"}, {d->in_amax, "in_amax"}, {d->out1_amax, "out1_amax"},
                    {d->out0_amax, "out0_amax"}, {d->pool_am, "pool_am"});
    return lrpx::conv_dispatch(d, (hipStream_t)stream);
}

int lrpx_conv_kernel_name(const lrpx_conv_desc* d, char* buf, int len) {
    LRPX_REQUIRE(d && buf && len > 0, "conv_kernel_name: null argument");
    lrpx::ConvChoice c;
    LRPX_TRY(lrpx::conv_select(d, 1, c));
    snprintf(buf, len, "%s ks=%d tg=%d", c.k->name, c.a.ksplit, c.a.tile_group);
    return LRPX_OK;
}

}  // extern "C"
