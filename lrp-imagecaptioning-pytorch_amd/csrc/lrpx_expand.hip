// Guided-Grad-CAM combination (ExplainGridTDGuidedGradCam.explain_cnn, models/gridTDmodel.py:1814-1836;
// ExplainAOAGuidedGradCam.explain_cnn, models/aoamodel.py:1729-1751):
//     guided_results = guided_gradient * pyramid_expand(cam, upscale = 16)          (cam: 14x14 Grad-CAM heat map)
// skimage.transform.pyramid_expand (scikit-image, un-vendored dependency of the reference; absent from this image) is
// `resize(order=1, mode='reflect')` followed by a Gaussian smoothing with sigma = 2 * upscale / 6, truncate 4 - both
// linear and separable, so the whole expansion is E = M cam M^T with one (HW x p) matrix M = Gauss (HW x HW) . Bilinear
// (HW x p) that the host builds once (ops.pyramid_expand_matrix).  One workgroup per map: tmp = M cam (HW x p, LDS), then
// every pixel E[y][x] = sum_j tmp[y][j] M[x][j] times the three channels of the guided gradient.  HBM-bound: reads and
// writes the maps once (1.2 MB per map).
#include "common.h"

namespace lrpx {

typedef float f32x4x __attribute__((ext_vector_type(4)));

template <int PMAX>
__global__ __launch_bounds__(256) void guided_gradcam_kernel(const float* __restrict__ g, const float* __restrict__ cam,
                                                             const float* __restrict__ M, float* __restrict__ out,
                                                             int p, int hw, int channels) {
    extern __shared__ float lds[];
    float* Ms = lds;                    // [hw][p]
    float* tmp = lds + hw * p;          // [hw][p]   tmp[y][j] = sum_i M[y][i] cam[i][j]
    float* cs = tmp + hw * p;           // [p][p]
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int e = tid; e < hw * p; e += 256) Ms[e] = M[e];
    for (int e = tid; e < p * p; e += 256) cs[e] = cam[(long)n * p * p + e];
    __syncthreads();
    for (int e = tid; e < hw * p; e += 256) {
        const int y = e / p, j = e - y * p;
        float s = 0.f;
        for (int i = 0; i < p; ++i) s = fmaf(Ms[y * p + i], cs[i * p + j], s);
        tmp[e] = s;
    }
    __syncthreads();
    const long per = (long)hw * hw;
    const float* gn = g + (long)n * channels * per;
    float* on = out + (long)n * channels * per;
    for (long q = tid; q < per; q += 256) {
        const int y = (int)(q / hw), x = (int)(q - (long)y * hw);
        float ev = 0.f;
        for (int j = 0; j < p; ++j) ev = fmaf(tmp[y * p + j], Ms[x * p + j], ev);
        for (int c = 0; c < channels; ++c) on[c * per + q] = gn[c * per + q] * ev;
    }
}

// A feature-resolution heat map (attention weights of one decoder step, a 2-D Grad-CAM map) at image size: out = E = M a M^T, optionally
// divided by max |E| (`_project_maxabs`, evaluation.py:338-343).  `a` is one head of (heads, p*p) or the mean over the heads.  One
// workgroup of 1024 threads per map: lane x = tid & 255 keeps row x of M in registers (p <= 32) and walks the rows y = tid >> 8, + 4, ...;
// tmp[y][.] = (M a)[y][.] is an LDS broadcast (one address per wave, ds_read_b128), the store of a wave is 256 contiguous bytes.
// Both fmaf chains run in the order of guided_gradcam_kernel above (i ascending, then j ascending), so E has its bits.  normalize: pass 1
// forms E in registers for max |E| alone, pass 2 forms it again and stores E / m - `out` is written once, nothing is read back.
// PQ = ceil(p / 4): the quads below the last are unguarded, the last one is guarded per element (a padded fmaf(0, 0, ev) would turn
// an ev of -0 into +0).
constexpr int EXPAND_NT = 1024;          // threads of a workgroup: 256 columns x 4 row phases

template <int PQ>
__device__ __forceinline__ float expand_pixel(const float* __restrict__ trow, const float (&mr)[4 * PQ], int p) {
    const f32x4x* t4 = reinterpret_cast<const f32x4x*>(trow);
    float ev = 0.f;
#pragma unroll
    for (int q = 0; q < PQ - 1; ++q) {
        const f32x4x t = t4[q];
        ev = fmaf(t.x, mr[4 * q], ev); ev = fmaf(t.y, mr[4 * q + 1], ev);
        ev = fmaf(t.z, mr[4 * q + 2], ev); ev = fmaf(t.w, mr[4 * q + 3], ev);
    }
    const f32x4x t = t4[PQ - 1];
    constexpr int b = 4 * (PQ - 1);
    ev = fmaf(t.x, mr[b], ev);
    if (b + 1 < p) ev = fmaf(t.y, mr[b + 1], ev);
    if (b + 2 < p) ev = fmaf(t.z, mr[b + 2], ev);
    if (b + 3 < p) ev = fmaf(t.w, mr[b + 3], ev);
    return ev;
}

template <int PQ>
__global__ __launch_bounds__(EXPAND_NT) void expand_maps_kernel(const float* __restrict__ maps, const float* __restrict__ M,
                                                          float* __restrict__ out, int heads, int head, int p, int hw, int normalize) {
    extern __shared__ float lds[];
    constexpr int ts = 4 * PQ;          // row stride of tmp: 16-byte rows
    float* tmp = lds;                   // [hw][ts]   tmp[y][j] = sum_i M[y][i] a[i][j]
    float* cs = tmp + hw * ts;          // [p][p]
    float* red = cs + p * p;            // [16]
    const int n = blockIdx.x, tid = threadIdx.x, pp = p * p;
    const float* src = maps + (long)n * heads * pp;
    for (int e = tid; e < pp; e += EXPAND_NT) {
        float v;
        if (head >= 0) v = src[head * pp + e];
        else {                          // np.mean(axis = 0) of an (NH, P) fp32 array: heads added in order, one division
            v = src[e];
            for (int h = 1; h < heads; ++h) v += src[h * pp + e];
            if (heads > 1) v = v / (float)heads;
        }
        cs[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < hw * p; e += EXPAND_NT) {
        const int y = e / p, j = e - y * p;
        float s = 0.f;
        for (int i = 0; i < p; ++i) s = fmaf(M[y * p + i], cs[i * p + j], s);
        tmp[y * ts + j] = s;
    }
    __syncthreads();
    const int lx = tid & 255, y0 = tid >> 8;
    float m = 0.f;
    if (normalize) {
        for (int x0 = 0; x0 < hw; x0 += 256) {
            const int x = x0 + lx;
            if (x < hw) {
                float mr[4 * PQ];
#pragma unroll
                for (int j = 0; j < 4 * PQ; ++j) mr[j] = j < p ? M[x * p + j] : 0.f;
                for (int y = y0; y < hw; y += EXPAND_NT / 256) m = fmaxf(m, fabsf(expand_pixel<PQ>(tmp + y * ts, mr, p)));
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        m = red[0];
#pragma unroll
        for (int w = 1; w < EXPAND_NT / 64; ++w) m = fmaxf(m, red[w]);
    }
    float* on = out + (long)n * hw * hw;
    for (int x0 = 0; x0 < hw; x0 += 256) {
        const int x = x0 + lx;
        if (x < hw) {
            float mr[4 * PQ];
#pragma unroll
            for (int j = 0; j < 4 * PQ; ++j) mr[j] = j < p ? M[x * p + j] : 0.f;
            for (int y = y0; y < hw; y += EXPAND_NT / 256) {
                const float ev = expand_pixel<PQ>(tmp + y * ts, mr, p);
                on[(long)y * hw + x] = m != 0.f ? ev / m : ev;          // all-zero map (`np.zeros(x.shape)`), or no normalisation: E itself
            }
        }
    }
}

}  // namespace lrpx

using namespace lrpx;

extern "C" int lrpx_guided_gradcam(const float* guided, const float* cam, const float* expand_m, float* out, int rows, int p,
                                   int hw, int channels, void* stream) {
    LRPX_REQUIRE(guided && cam && expand_m && out && rows > 0 && p > 0 && p <= 32 && hw > 0 && channels > 0,
                 "guided_gradcam: bad arguments");
    const int lds = (2 * hw * p + p * p) * (int)sizeof(float);
    LRPX_REQUIRE(lds <= 64 * 1024, "guided_gradcam: hw * p too large for the LDS image (%d bytes)", lds);
    hipLaunchKernelGGL((guided_gradcam_kernel<32>), dim3(rows), dim3(256), lds, (hipStream_t)stream, guided, cam, expand_m,
                       out, p, hw, channels);
    return check_launch("guided_gradcam");
}

template <int PQ>
static void launch_expand_maps(const float* maps, const float* expand_m, float* out, int rows, int heads, int head, int p, int hw,
                               int normalize, int lds, hipStream_t stream) {
    hipLaunchKernelGGL((expand_maps_kernel<PQ>), dim3(rows), dim3(EXPAND_NT), lds, stream, maps, expand_m, out, heads, head, p, hw, normalize);
}

extern "C" int lrpx_expand_maps(const float* maps, const float* expand_m, float* out, int rows, int heads, int head, int p, int hw,
                                int normalize, void* stream) {
    LRPX_REQUIRE(maps && expand_m && out, "expand_maps: null pointer");
    LRPX_REQUIRE(rows > 0 && heads > 0 && head >= -1 && head < heads, "expand_maps: bad rows / heads / head (%d, %d, %d)", rows, heads, head);
    LRPX_REQUIRE(p >= 2 && p <= 32 && hw > 0 && hw % p == 0, "expand_maps: p must be 2..32 and hw a multiple of p (p %d, hw %d)", p, hw);
    LRPX_REQUIRE(normalize == 0 || normalize == 1, "expand_maps: normalize must be 0 or 1");
    const int pq = (p + 3) / 4;
    const long lds = ((long)hw * 4 * pq + p * p + 16) * (long)sizeof(float);
    LRPX_REQUIRE(lds <= 64 * 1024, "expand_maps: hw * p too large for the LDS image (%ld bytes)", lds);
    LRPX_CHECK_PTRS("lrpx_expand_maps", {maps, "maps"}, {expand_m, "expand_m"}, {out, "out"});
    hipStream_t st = (hipStream_t)stream;
    switch (pq) {
        case 1: launch_expand_maps<1>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
        case 2: launch_expand_maps<2>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
        case 3: launch_expand_maps<3>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
        case 4: launch_expand_maps<4>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
        case 5: launch_expand_maps<5>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
        case 6: launch_expand_maps<6>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
        case 7: launch_expand_maps<7>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
        default: launch_expand_maps<8>(maps, expand_m, out, rows, heads, head, p, hw, normalize, (int)lds, st); break;
    }
    return check_launch("expand_maps");
}
