// Shared host-side helpers of liblrpx: error reporting and launch checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <initializer_list>
#include <mutex>

#include "../../include/lrpx.h"

#include "build_guard.h"

namespace lrpx {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return LRPX_ELAUNCH;
    }
    return LRPX_OK;
}

#define LRPX_REQUIRE(cond, ...)          \
    do {                                 \
        if (!(cond)) {                   \
            lrpx::set_error(__VA_ARGS__); \
            return LRPX_EINVAL;          \
        }                                \
    } while (0)

#define LRPX_TRY(expr)               \
    do {                             \
        int rc__ = (expr);           \
        if (rc__ != LRPX_OK) return rc__; \
    } while (0)

// ---- caller pointers ------------------------------------------------------------------------------------------
// The C ABI takes raw device pointers; a pageable host pointer (a CPU tensor's data_ptr) handed to a kernel is a GPU page fault, not
// an error code.  check_dev_ptrs asks the runtime what each non-null pointer is (hipPointerGetAttributes, ~1 us each): device /
// managed memory of the CURRENT device or pinned host memory pass; anything else returns LRPX_EINVAL with the entry point and the
// argument's name in lrpx_last_error_string().  The heavy entry points (milliseconds of work: the VGG16 chains, the packers, the
// layout converters, the rule classes' kernels) validate on every call; the microsecond-scale decoder steps only when
// LRPX_CHECK_PTRS=1 is in the environment (latched at first use).
struct PtrArg { const void* p; const char* name; };
int check_dev_ptrs(const char* fn, std::initializer_list<PtrArg> args);     // (lrpx_core.hip)
bool ptr_checks_all();
#define LRPX_CHECK_PTRS(fn, ...) LRPX_TRY(lrpx::check_dev_ptrs(fn, {__VA_ARGS__}))
#define LRPX_CHECK_PTRS_OPT(fn, ...)                                                   \
    do {                                                                               \
        if (lrpx::ptr_checks_all()) LRPX_TRY(lrpx::check_dev_ptrs(fn, {__VA_ARGS__})); \
    } while (0)

// elementwise producers of S that also record max|S| per map for an f16x3 consumer (lrpx_core.hip)
int maxpool_relevance_amax(const float* x, const float* r_out, const float* zdiv, const int32_t* map2img, float* r_in,
                           float* s_out, int n_maps, int h_out, int w_out, int c, int s_chunk, unsigned* amax,
                           hipStream_t stream);
int divide_stab_amax(const float* r, const float* z, const int32_t* map2img, float* s, int n_maps, long pix_c, int stab,
                     unsigned* amax, hipStream_t stream);
int pool_winner_blk(const float* x, const float* z, float* xzw, uint8_t* am, float* xzw_blk, int n, int h_out, int w_out, int c, hipStream_t stream,
                    float* y_pool = nullptr);     // y_pool: also the pooled activations (the forward pass)
int divide_safe_blk(const float* r, const float* z, float* s, float* s_blk, int n_img, int pix, int c, hipStream_t stream);
int divide_stab_blocked(const float* r, const float* z, const int32_t* map2img, float* s_blk, int n_maps, int pix, int c,
                        unsigned* amax, hipStream_t stream);

// max|x| over a flat tensor, atomically max-ed into *out as float bits (lrpx_core.hip)
int amax_flat(const float* x, long n, unsigned* out, hipStream_t stream);

// zero `bytes` bytes at dst on the stream (lrpx_core.hip): every clear of the library goes through here - hipMemsetAsync, a kernel while
// the stream is being captured into a HIP graph
int clear_async(void* dst, size_t bytes, hipStream_t stream);

// hipFuncAttributeMaxDynamicSharedMemorySize of one kernel instantiation.  HIP function attributes are PER DEVICE, and one
// host process may drive several GPUs from several threads (include/lrpx.h THREADING), so the attribute is set exactly once
// per (instantiation, device ordinal) even when several host threads make their first launch of it at the same time
// (no globals except an init-once cache behind a mutex).  `LdsOnce` is the caller's function-local static
// (one per template instantiation).
struct LdsOnce {
    static constexpr int MAX_DEV = 64;
    std::once_flag once[MAX_DEV];
    hipError_t res[MAX_DEV] = {};
};
template <typename K>
inline int reserve_lds_once(LdsOnce& st, K kern, int bytes, const char* what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LdsOnce::MAX_DEV) {
        set_error("%s: cannot identify the current device", what);
        return LRPX_ELAUNCH;
    }
    std::call_once(st.once[dev], [&] {
        st.res[dev] = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    });
    if (st.res[dev] != hipSuccess) {
        set_error("%s: cannot reserve %d bytes of LDS on device %d", what, bytes, dev);
        return LRPX_ELAUNCH;
    }
    return LRPX_OK;
}

// The two dispatch switches that tests use as seams (both values of each are reachable by descriptor anyway): ONE getenv pass per
// process, latched on first use.  Every other former LRPX_* A/B switch is frozen at the value all measurements in DESIGN.md
// were taken with (table in DESIGN.md, "Frozen runtime switches"); setting such a name in the environment changes nothing.
struct Switches {
    int dense_n256;      // LRPX_DENSE_N256 (default 1): 128 x 256 tiles with the waves side by side for the many-row dense f16x3 GEMM
    int b6_wino;         // LRPX_B6_WINO (bit mask, default 15): conv-mode-1 relevance convs that are not under a pool on the Winograd F(2x2,3x3) kernel
                         // (conv_wino_b6.h) at 56 x 56 (1), 28 x 28 (2), 14 x 14 (4); needs lrpx_conv_desc.wpacked_wino.  lrpx_set_b6_wino overrides it.
                         // 8: every staging thread fetches its whole patch (legacy staging); without it the outer columns come from the neighbouring lanes (same bits, not faster)
};
const Switches& switches();      // (lrpx_core.hip)
int b6_wino_bits();              // switches().b6_wino unless lrpx_set_b6_wino moved it (lrpx_core.hip)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

}  // namespace lrpx
