// Winograd F(2x2, 3x3) relevance conv on the exact bf16 splits (conv mode 1, REL_MUL epilogue).
//
//   Y = A^T [ (G g G^T) (.) (B^T d B) ] A        per 2x2 output tile and channel pair: 16 multiplications instead of 36
//
// The 16 element-wise products are 16 GEMMs  M[xi][tile][ci] = sum_co V[xi][tile][co] U[xi][co][ci]  (xi = 4 i + j), each
// computed exactly like the direct kernel computes its one GEMM: both operands are fp32 values split EXACTLY into three bf16
// planes, the six leading plane products run on v_mfma_f32_32x32x16_bf16 (smallest terms first), fp32 accumulation.
//   * U = G g G^T is evaluated in fp64, rounded ONCE to fp32 and split at pack time (lrpx_pack_weights_wino_b6);
//   * V = B^T d B is evaluated in fp32 (+-1 coefficients only: one add per element and stage) by the whole workgroup
//     while it stages a 16-channel K-chunk, and kept in LDS as fp32 (64 KiB per chunk, double buffered); a wave owns
//     two of the 16 xi, so every V element is read - and split into its planes - by exactly one wave;
//   * GEMM rows are the 2x2 tiles of all maps flattened (tile T = map * (HW/2)^2 + ty * HW/2 + tx): fragments may straddle
//     maps and the last workgroup is ragged; a tile's sums never depend on its neighbours or on the batch.
// Workgroup: 8 waves, 64 tiles x 64 output channels x 16 xi; wave w accumulates xi = 2w, 2w+1 (2 row x 2 channel fragments
// each: 128 accumulator registers).  The output transform exchanges M through LDS (the V buffers, after the K loop), then
// out = x * Y as in epi_finish<EPI_REL_MUL> (NHWC or channel-chunked output, map2img for the multiplicand).
// B fragments stream from L2: 32 B/clk/CU, sustainable only while the CUs of an XCD walk the same 64-channel slice
// (16 xi x K x 64 x 6 B = 3.1 MB at K = 512): workgroups are ordered XCD-contiguous in bands of 32 row blocks.
// Patch and B loads are buffer loads without control flow around them, so that every s_waitcnt counts them: the patch loads of the
// next chunk go out between the chunk's two xi steps and are waited for by the commit alone (profiles/wino_wait_isa.txt).
#pragma once
#include "conv_bf16x6.h"

namespace lrpx {

constexpr int WINO_KQ = 1088;              // bytes per (xi, 4-channel quad) plane: 64 tiles x 16 B + 64 B (conflict-free float4 commits)
constexpr int WINO_XI = 4 * WINO_KQ;       // bytes per xi
constexpr int WINO_BUF = 16 * WINO_XI;     // bytes per V buffer
constexpr int WINO_LDS = 2 * WINO_BUF;     // 139 264 B: one workgroup per CU
constexpr int WINO_MROW = 33;              // floats per (xi, tile) row of the M exchange
constexpr unsigned WINO_OOB = 0x7fff0000u; // patch-load offset of what is not fetched: beyond the end of every workgroup's buffer resource

// 8 fp32 -> three bf16x8 planes, v == p0 + p1 + p2 exactly
__device__ __forceinline__ void wino_split8(const f32x4 q0, const f32x4 q1, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        unsigned short s0, s1, s2;
        split3(e < 4 ? q0[e & 3] : q1[e & 3], s0, s1, s2);
        p0[e] = (short)s0; p1[e] = (short)s1; p2[e] = (short)s2;
    }
}

// x - y, x + y and fma(x, s, y) (s = +-1: y +- x, one rounding, the bits of the add) on the channel pairs of a quad: v_pk_add_f32 / v_pk_fma_f32
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 wino_sub(const f32x4 x, const f32x4 y) {
    const f32x2 lo = __builtin_shufflevector(x, x, 0, 1) - __builtin_shufflevector(y, y, 0, 1);
    const f32x2 hi = __builtin_shufflevector(x, x, 2, 3) - __builtin_shufflevector(y, y, 2, 3);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}
__device__ __forceinline__ f32x4 wino_add(const f32x4 x, const f32x4 y) {
    const f32x2 lo = __builtin_shufflevector(x, x, 0, 1) + __builtin_shufflevector(y, y, 0, 1);
    const f32x2 hi = __builtin_shufflevector(x, x, 2, 3) + __builtin_shufflevector(y, y, 2, 3);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}
__device__ __forceinline__ f32x4 wino_fma(const f32x4 x, const float s, const f32x4 y) {
    const f32x2 ss = {s, s};
    const f32x2 lo = __builtin_elementwise_fma(__builtin_shufflevector(x, x, 0, 1), ss, __builtin_shufflevector(y, y, 0, 1));
    const f32x2 hi = __builtin_elementwise_fma(__builtin_shufflevector(x, x, 2, 3), ss, __builtin_shufflevector(y, y, 2, 3));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}

// SHARE: a staging thread fetches only its tile's own two patch columns and takes the two outer ones from the lanes that own them
// (lane -/+ 4: the same channel quad of the tile to the left / right); false = every thread fetches its four columns (LRPX_B6_WINO bit 8,
// the default: the shared form moves fewer bytes and is not faster).  Both stage the same bits.
template <int HW, bool SHARE>
__global__ __launch_bounds__(512) void conv_wino_b6_kernel(ConvArgs a, int total_tiles, int m_blocks, int n_blocks) {
    constexpr int TW = HW / 2, TPM = TW * TW, P = HW * HW;
    constexpr int BAND = 32;
    extern __shared__ __attribute__((aligned(16))) char ldsw[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;

    // XCD-contiguous order: the 32 row blocks of a band run the same channel slice at the same time on one XCD
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int mb8 = (m_blocks + 7) >> 3;
    const int band = idx / (BAND * n_blocks), rem = idx - band * (BAND * n_blocks);
    const int band_rows = min(BAND, mb8 - band * BAND);
    const int nblk = rem / band_rows;
    const int mblk = (band * BAND + rem - nblk * band_rows) * 8 + xcd;
    if (mblk >= m_blocks) return;
    const int row0 = mblk * 64;
    const int nchunk = a.cin / 16;

    // ---- staging: thread = (tile, 4-channel quad, half of the transform rows); three patch rows x four columns each ----
    // rv[0..2] = patch rows (a, b, c) with V rows  a - c  and  c + sgn b:  half 0 (i = 0, 1): a, b, c = d0, d1, d2, sgn = +1
    // (d0 - d2, d1 + d2);  half 1 (i = 2, 3): a, b, c = d2, d3, d1, sgn = -1 (d2 - d1, d1 - d3) - one code path, no selects
    const int seg = tid & 3, stile = (tid >> 2) & 63;
    const int half = wave >> 2;
    const float sgn = half ? -1.f : 1.f;
    unsigned smask = 0;
    bool take_l = false, take_r = false;     // SHARE: patch column 0 / 3 comes from lane - 4 / lane + 4
    int srow[3];                             // patch row of slot a, b, c (wave-uniform)
    // The patch loads are raw buffer loads through a resource that starts at the workgroup's first map and ends with the tensor
    // (at most WINO_OOB bytes: the launcher checks that a workgroup's maps fit): a thread issues all twelve of them, every chunk, with
    // no branch around them, so that the compiler counts them in its vmcnt waits.  What a thread must not fetch (zero padding,
    // ragged tail, SHARE: the columns it is given) has the offset WINO_OOB: the range check answers with the exact zero, forms no
    // address and touches no memory.  Every other offset is that of an element of `in`.
    const int n0 = row0 / TPM;
    unsigned voff[3][4];
    {
        const int T = row0 + stile;
        const int n = T / TPM, t = T - n * TPM;
        const int ty = t / TW, tx = t - ty * TW;
        const int y0 = 2 * ty - 1, x0 = 2 * tx - 1;
#pragma unroll
        for (int r = 0; r < 3; ++r) srow[r] = half ? (r == 2 ? 1 : r + 2) : r;
        if (T < total_tiles) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (y0 + srow[r] >= 0 && y0 + srow[r] < HW && x0 + c >= 0 && x0 + c < HW) smask |= 1u << (r * 4 + c);
            if (SHARE) {
                // lanes -/+ 4 hold tiles T -/+ 1 (same half, so the same patch rows) if they are in this wave; inside a tile row
                // they are this map's tiles tx -/+ 1, whose own columns 2 / 1 are this patch's columns 0 / 3.  At the ends of
                // the wave and of the tile row the thread keeps its own fetch (or the zero padding) under smask.
                take_l = (stile & 15) != 0 && tx != 0;
                take_r = (stile & 15) != 15 && tx != TW - 1 && T + 1 < total_tiles;
                if (take_l) smask &= ~0x111u;
                if (take_r) smask &= ~0x888u;
            }
        }
        // under smask the pixel lies in map n >= n0 of the tensor: the offset is >= 0 and below WINO_OOB
        const int sbase = (((n - n0) * HW + y0) * HW + x0) * a.cin + seg * 4;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                voff[r][c] = (smask & (1u << (r * 4 + c))) ? (unsigned)(sbase + (srow[r] * HW + c) * a.cin) * 4u : WINO_OOB;
    }
    const long left = (long)(a.n_maps - n0) * P * a.cin * 4;
    const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.in) + (long)n0 * P * a.cin, 0, (int)(left < (long)WINO_OOB ? left : (long)WINO_OOB), 0x00020000);
    // SHARE: the exchange overwrites columns 0 / 3 of the lanes that are given them; the next chunk's loads put their zeros back
    f32x4 rv[3][4];
#define LRPXW_ISSUE(CHUNK)                                                                                          \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 4; ++c)                      \
        rv[r][c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, voff[r][c], (CHUNK) * 64, 0));
    // ds_bpermute moves a dword between lanes without a VALU slot (DPP row shifts stop at 16 lanes = 4 tiles); one select per dword.
    // (the element goes through a scalar: __builtin_bit_cast straight on rv[r][c][e] reads element 0 of the vector)
    const int lane_l = ((lane - 4) & 63) * 4, lane_r = ((lane + 4) & 63) * 4;
#define LRPXW_SHARE()                                                                                               \
    if (SHARE) {                                                                                                    \
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int e = 0; e < 4; ++e) {                \
            const float ml = rv[r][2][e], mr = rv[r][1][e];                                                         \
            const float fl = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(lane_l, __builtin_bit_cast(int, ml))); \
            const float fr = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(lane_r, __builtin_bit_cast(int, mr))); \
            rv[r][0][e] = take_l ? fl : rv[r][0][e];                                                                \
            rv[r][3][e] = take_r ? fr : rv[r][3][e];                                                                \
        }                                                                                                           \
    }
    // stage 1 (rows): t_0 = d0 - d2, t_1 = d1 + d2, t_2 = d2 - d1, t_3 = d1 - d3; stage 2 (columns) alike.  Channel pairs: packed fp32
#define LRPXW_COMMIT(BUFIDX)                                                                                        \
    {                                                                                                               \
        LRPXW_SHARE()                                                                                               \
        char* vb = ldsw + (BUFIDX) * WINO_BUF + (half * 8) * WINO_XI + seg * WINO_KQ + stile * 16;                  \
        _Pragma("unroll") for (int ii = 0; ii < 2; ++ii) {                                                          \
            f32x4 t[4];                                                                                             \
            _Pragma("unroll") for (int c = 0; c < 4; ++c)                                                           \
                t[c] = ii == 0 ? wino_sub(rv[0][c], rv[2][c]) : wino_fma(rv[1][c], sgn, rv[2][c]);                  \
            *reinterpret_cast<f32x4*>(vb + (ii * 4 + 0) * WINO_XI) = wino_sub(t[0], t[2]);                          \
            *reinterpret_cast<f32x4*>(vb + (ii * 4 + 1) * WINO_XI) = wino_add(t[1], t[2]);                          \
            *reinterpret_cast<f32x4*>(vb + (ii * 4 + 2) * WINO_XI) = wino_sub(t[2], t[1]);                          \
            *reinterpret_cast<f32x4*>(vb + (ii * 4 + 3) * WINO_XI) = wino_sub(t[1], t[3]);                          \
        }                                                                                                           \
    }

    LRPXW_ISSUE(0)

    f32x16 acc[2][2][2];     // [xi of the wave][row fragment][channel fragment]
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[x][rt][nb][e] = 0.f;

    // B fragments [ocb][xi][k-step][plane][64 lanes][16 B]: the fragments of channel block nb are re-loaded for the next
    // (xi, k-step) as soon as its MFMAs are issued, i.e. half a step ahead
    // (buffer loads as well: the lane's 16 B in the one address register, fragment and plane in the scalar offset - flat loads
    // keep four 64-bit addresses in registers that the kernel does not have; the launcher checks that the packed weights stay below 2 GiB)
    const int ocb_stride = 16 * nchunk * 192;
    const int last_step = 2 * nchunk - 1;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, n_blocks * 2 * ocb_stride * 16, 0x00020000);
    const unsigned wlane = lane * 16;
    auto boff = [&](int step, int nb) -> unsigned {
        const int s = min(step, last_step);
        const int xi = 2 * wave + (s & 1), ks = s >> 1;
        return (unsigned)((nblk * 2 + nb) * ocb_stride + (xi * nchunk + ks) * 192) * 16u;
    };
#define LRPXW_BLOAD(STEP, NB)                                                                                       \
    _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                                   \
        bq[NB][p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, boff(STEP, NB) + p * 1024, 0));
    u32x4 bq[2][3];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) LRPXW_BLOAD(0, nb)

    LRPXW_COMMIT(0)
    __syncthreads();

    // one xi step of a chunk: read and split the wave's A fragments, 24 MFMAs; the B fragments of a channel block are re-loaded for
    // the next step as soon as its MFMAs are issued
#define LRPXW_STEP(CHUNK, X, VBUF)                                                                                  \
    {                                                                                                               \
        const char* vx = (VBUF) + (2 * wave + (X)) * WINO_XI + (2 * lh) * WINO_KQ + li * 16;                        \
        bf16x8 ap[2][3];                                                                                            \
        _Pragma("unroll") for (int rt = 0; rt < 2; ++rt) {                                                          \
            const f32x4 q0 = *reinterpret_cast<const f32x4*>(vx + rt * 512);                                        \
            const f32x4 q1 = *reinterpret_cast<const f32x4*>(vx + rt * 512 + WINO_KQ);                              \
            wino_split8(q0, q1, ap[rt][0], ap[rt][1], ap[rt][2]);                                                   \
        }                                                                                                           \
        _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) {                                                          \
            const bf16x8 b0 = __builtin_bit_cast(bf16x8, bq[nb][0]);                                                \
            const bf16x8 b1 = __builtin_bit_cast(bf16x8, bq[nb][1]);                                                \
            const bf16x8 b2 = __builtin_bit_cast(bf16x8, bq[nb][2]);                                                \
            _Pragma("unroll") for (int rt = 0; rt < 2; ++rt) {                                                      \
                f32x16 c = acc[X][rt][nb];                                                                          \
                /* smallest terms first */                                                                          \
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[rt][2], b0, c, 0, 0, 0);                             \
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[rt][1], b1, c, 0, 0, 0);                             \
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[rt][0], b2, c, 0, 0, 0);                             \
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[rt][1], b0, c, 0, 0, 0);                             \
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[rt][0], b1, c, 0, 0, 0);                             \
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[rt][0], b0, c, 0, 0, 0);                             \
                acc[X][rt][nb] = c;                                                                                 \
            }                                                                                                       \
            LRPXW_BLOAD(2 * (CHUNK) + (X) + 1, nb)                                                                  \
            __builtin_amdgcn_sched_barrier(0); /* the reload stays here in the queue of loads */                    \
        }                                                                                                           \
    }

    // Steady state.  The loads retire in the order of their issue, which the scheduling barriers pin:
    //   B of the second step (6, issued during the first step), the 12 patch loads of chunk + 1, B of the next chunk's first step (6).
    // So no wait in front of MFMAs retires a patch load of its own chunk (the second step's waits end at vmcnt(15), the next chunk's
    // first step finds the patch loads retired by the commit), and the patch loads have the second step's 24 MFMAs to come back.  rv is
    // dead during the first step.  The last chunk, which stages nothing, is peeled off, so that the loop has no branch in it.
    for (int chunk = 0; chunk + 1 < nchunk; ++chunk) {
        const char* vbuf = ldsw + (chunk & 1) * WINO_BUF;
        LRPXW_STEP(chunk, 0, vbuf)
        LRPXW_ISSUE(chunk + 1)
        __builtin_amdgcn_sched_barrier(0);
        LRPXW_STEP(chunk, 1, vbuf)      // (ends with a scheduling barrier: the transform and its waits stay behind the MFMAs)
        LRPXW_COMMIT((chunk + 1) & 1)
        __syncthreads();
    }
    {
        const char* vbuf = ldsw + ((nchunk - 1) & 1) * WINO_BUF;
        LRPXW_STEP(nchunk - 1, 0, vbuf)
        LRPXW_STEP(nchunk - 1, 1, vbuf)
        __syncthreads();
    }
#undef LRPXW_STEP
#undef LRPXW_BLOAD
#undef LRPXW_ISSUE
#undef LRPXW_SHARE
#undef LRPXW_COMMIT

    // ---- output transform Y = A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]) through LDS, then out = x * Y ----
    float* ms = reinterpret_cast<float*>(ldsw);
    const float* __restrict__ X = a.X;
    float* __restrict__ ob = a.out1 ? a.out1 : a.out0;
    const int ncol = a.oc_split;
    const int ch = a.out_chunk;
    const int ostr = ch > 0 ? ch : ncol;
    const long total_pix = (long)a.n_maps * P;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    ms[((2 * wave + x) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * WINO_MROW + li] = acc[x][rt][nb][e];
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int pr = tid + it * 512;
                const int c = pr & 31, tl = pr >> 5;
                float m[16];
#pragma unroll
                for (int xi = 0; xi < 16; ++xi) m[xi] = ms[(xi * 32 + tl) * WINO_MROW + c];
                float s0[4], s1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s0[j] = (m[j] + m[4 + j]) + m[8 + j];
                    s1[j] = (m[4 + j] - m[8 + j]) - m[12 + j];
                }
                const float y00 = (s0[0] + s0[1]) + s0[2], y01 = (s0[1] - s0[2]) - s0[3];
                const float y10 = (s1[0] + s1[1]) + s1[2], y11 = (s1[1] - s1[2]) - s1[3];
                const int T = row0 + rt * 32 + tl;
                const int oc = (nblk * 2 + nb) * 32 + c;
                if (T < total_tiles && oc < ncol) {
                    const int n = T / TPM, t = T - n * TPM;
                    const int ty = t / TW, tx = t - ty * TW;
                    const long img = a.map2img ? a.map2img[n] : n;
                    const int p = (2 * ty) * HW + 2 * tx;
                    const float* xp = X + (img * P + p) * ncol + oc;
                    const long obase = ch > 0 ? (long)(oc / ch) * total_pix * ch + (oc % ch) : (long)oc;
                    float* op = ob + ((long)n * P + p) * ostr + obase;
                    const float x00 = xp[0], x01 = xp[ncol], x10 = xp[(long)HW * ncol], x11 = xp[(long)(HW + 1) * ncol];
                    __builtin_nontemporal_store(x00 * y00, &op[0]);
                    __builtin_nontemporal_store(x01 * y01, &op[ostr]);
                    __builtin_nontemporal_store(x10 * y10, &op[(long)HW * ostr]);
                    __builtin_nontemporal_store(x11 * y11, &op[(long)(HW + 1) * ostr]);
                }
            }
            __syncthreads();
        }
}

template <int HW, bool SHARE>
int launch_conv_wino_b6(const ConvArgs& a, hipStream_t stream) {
    constexpr int TPM = (HW / 2) * (HW / 2);
    const long total_tiles = (long)a.n_maps * TPM;
    const long m_blocks = ceil_div(total_tiles, 64);
    const int n_blocks = a.n_oc / 64;
    const long grid = ceil_div(m_blocks, 8) * 8 * n_blocks;
    if (grid <= 0 || grid > 0x7fffffffL || a.n_oc % 64 != 0) {
        set_error("conv_wino_b6: grid %ld out of range or n_oc %d not a multiple of 64", grid, a.n_oc);
        return LRPX_EINVAL;
    }
    // the kernel's 32-bit buffer offsets: the maps that a workgroup's 64 tiles touch (at most 64 / TPM + 2), and the packed weights
    const long span = (long)(64 / TPM + 2) * HW * HW * a.cin * 4, wbytes = (long)n_blocks * 2 * 16 * (a.cin / 16) * 192 * 16;
    if (span >= (long)WINO_OOB || wbytes > 0x7fffffffL) {
        set_error("conv_wino_b6: %ld B of maps per workgroup or %ld B of packed weights are beyond the kernel's 32-bit offsets", span, wbytes);
        return LRPX_EINVAL;
    }
    auto kern = conv_wino_b6_kernel<HW, SHARE>;
    static LdsOnce attr_once;
    LRPX_TRY(reserve_lds_once(attr_once, kern, WINO_LDS, "conv_wino_b6"));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), WINO_LDS, stream, a, (int)total_tiles, (int)m_blocks, n_blocks);
    return check_launch("conv_wino_b6");
}

}  // namespace lrpx
