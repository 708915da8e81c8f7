// Internal helpers shared by the HIP translation units of libgvcnn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "gvcnn_hip.h"

#define GV_HIP_CHECK(expr)                           \
    do {                                             \
        hipError_t _e = (expr);                      \
        if (_e != hipSuccess) return (int)_e;        \
    } while (0)

#define GV_LAUNCH_CHECK()                            \
    do {                                             \
        hipError_t _e = hipGetLastError();           \
        if (_e != hipSuccess) return (int)_e;        \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting and one process may drive several GPUs
// (model.pin_device): remember its outcome per device, not per process.
struct GvPerDeviceOnce {
    std::atomic<signed char> state[64] = {};                     // 0 = not tried, 1 = ok, -1 = failed
    template <typename F>
    bool ok(F&& set) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
        signed char v = state[dev].load(std::memory_order_acquire);
        if (v == 0) {
            v = set() == hipSuccess ? 1 : -1;
            state[dev].store(v, std::memory_order_release);
        }
        return v > 0;
    }
};
// true when `kernel` may be launched with `bytes` of dynamic LDS on the current device
#define GV_BIG_LDS_OK(kernel, bytes)                                                                              \
    ([&] {                                                                                                        \
        static GvPerDeviceOnce once_;                                                                             \
        return once_.ok([&] {                                                                                     \
            return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                       (int)(bytes));                                                             \
        });                                                                                                       \
    }())

#if defined(__HIPCC__)
// Launch Kernel with `lds` bytes of dynamic LDS.  Above 64 KB the kernel's limit is raised first (to the CU's 160 KB; the
// outcome is remembered per kernel and device).  GV_OK, GV_E_UNSUPPORTED where the device refuses the limit, else the
// launch's HIP error.
template <auto Kernel, typename... Args>
int gv_launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
    if (lds > 64 * 1024) {
        if (!GV_BIG_LDS_OK(Kernel, 160 * 1024)) return GV_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
#endif

// the 16-bit storage types: T the type a stored element stands for
#define GV_LP_DISPATCH(dtype, CALL)                       \
    do {                                                  \
        if ((dtype) == GV_BF16) { using T = __bf16; CALL; }   \
        if ((dtype) == GV_F16) { using T = _Float16; CALL; }  \
        return GV_E_UNSUPPORTED;                          \
    } while (0)
// every storage type: E the element type in HBM, T the type it stands for
#define GV_ST_DISPATCH(dtype, CALL)                                                   \
    do {                                                                              \
        if ((dtype) == GV_F32) { using E = float; using T = float; CALL; }            \
        if ((dtype) == GV_BF16) { using E = unsigned short; using T = __bf16; CALL; } \
        if ((dtype) == GV_F16) { using E = unsigned short; using T = _Float16; CALL; } \
        return GV_E_UNSUPPORTED;                                                      \
    } while (0)
// a dtype (without GV_ACCUM_* bits) that GV_ST_DISPATCH serves
static inline bool gv_storage_type(int dtype) { return dtype == GV_F32 || dtype == GV_BF16 || dtype == GV_F16; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Every pooling window must hold at least one valid tap (else an average divides 0 by 0 and a max writes -inf / a 0xff
// argmax byte): the last window starts inside the image and the padding is smaller than the window.
static inline bool gv_pool_geometry_ok(const gv_pool_desc* d) {
    return d->pad_t < d->kh && d->pad_l < d->kw && (int64_t)(d->oh - 1) * d->stride - d->pad_t < d->ih &&
           (int64_t)(d->ow - 1) * d->stride - d->pad_l < d->iw;
}

// Exact division of a 31-bit dividend by a constant (Granlund-Montgomery, 31-bit precision): q = hi32(m * mul) >> sh.
struct GvFastDiv {
    unsigned mul;
    int sh;                                                      // -1: divisor 1 (q = m)
    int d;
};
static inline GvFastDiv gv_fast_div(int d) {
    GvFastDiv f;
    f.d = d;
    if (d <= 1) { f.mul = 0; f.sh = -1; return f; }
    int l = 0;
    while ((1ll << l) < d) ++l;                                  // l = ceil(log2 d) >= 1
    f.mul = (unsigned)(((1ull << (31 + l)) + (unsigned)d - 1) / (unsigned)d);
    f.sh = l - 1;
    return f;
}
#if defined(__HIPCC__)
__device__ __forceinline__ int gv_div(int m, const GvFastDiv& f) {
    return f.sh < 0 ? m : (int)(__umulhi((unsigned)m, f.mul) >> f.sh);
}
#endif

static inline int gv_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline bool gv_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
// rows of p (stride ld elements) can be walked in 16-byte accesses of n elements; nullptr: an operand that is not used
static inline bool gv_vec_ok(const void* p, int ld, int n) { return p == nullptr || (gv_aligned16(p) && ld % n == 0); }
// workgroups of 256 threads for a grid-stride loop over `total` items: at most 16 per CU, the loop strides the rest
static inline unsigned gv_grid_for(int64_t total) {
    const int64_t b = (total + 255) / 256, cap = 256 * 16;
    return (unsigned)(b < cap ? (b > 0 ? b : 1) : cap);
}

// ---- where a filter-gradient launch puts its partial tiles ------------------------------------------------------
// A filter gradient splits the pixel axis over workgroups ("slices"); every slice produces a partial of each
// element of dW it owns.  Two ways to combine them:
//   part == nullptr   fp32 atomic adds into dw (the order the slices arrive in decides the rounding: two runs differ in
//                     the last bits) — or, with ONE slice, the plain sum: a single adder per element;
//   part != nullptr   slice s STORES its partials into part + s * stride (an image of dW per slice), and a second launch
//                     (gv_dw_finish) adds the slices in index order into dw: the same bits every run, whatever the
//                     dispatch order.  (gv_conv2d_wgrad_ws; reference: the deterministic CPU gradients of
//                     utils/train_utils.py:217-259.)
struct GvDw {
    float* dw;
    float* part;
    size_t stride;                                               // elements between two slices' images (multiple of 4)
    size_t cap_bytes;                                            // host side: size of the workspace behind `part`
};
static inline GvDw gv_dw_plain(float* dw) { return GvDw{dw, nullptr, 0, 0}; }
// The slices a launch may use with this sink: a workspace holds cap_bytes / image slices; without room for two the
// launch runs un-split (one adder per element is deterministic as well).
static inline int64_t gv_dw_clamp(const GvDw& o, size_t elems, int64_t splits) {
    if (!o.part) return splits;
    const int64_t cap = (int64_t)(o.cap_bytes / (((elems + 3) / 4 * 4) * sizeof(float)));
    return cap < 2 ? 1 : (splits < cap ? splits : cap);
}
// The slice plan of a launch: `units` of work along the split axis (pixels, or strip stages) go to `splits` slices of
// `per` units each, the last one ragged.  Enough slices that `tiles` workgroups per slice fill `target_wgs`, but at least
// `min_units` a slice, at most `max_splits` slices (0: no such cap) and what the sink holds; `per` is then rounded up to
// `granule` and the slices counted again.  `per` is only ever rounded UP after gv_dw_clamp, so the slices never
// outnumber what the clamp allowed: splits <= gv_dw_clamp(o, elems, ...) — the workspace holds every slice's image.
struct GvSlices {
    int64_t splits, per;
};
static inline GvSlices gv_dw_plan(const GvDw& o, size_t elems, int64_t units, int64_t tiles, int64_t target_wgs,
                                  int64_t min_units, int64_t granule, int64_t max_splits) {
    int64_t splits = (target_wgs + tiles - 1) / tiles;
    const int64_t most = (units + min_units - 1) / min_units;
    if (splits > most) splits = most;
    if (splits < 1) splits = 1;
    if (max_splits && splits > max_splits) splits = max_splits;
    splits = gv_dw_clamp(o, elems, splits);
    int64_t per = (units + splits - 1) / splits;
    per = (per + granule - 1) / granule * granule;
    return GvSlices{(units + per - 1) / per, per};
}
// The sink the KERNEL gets for `splits` slices (the plain one for a single slice) ...
static inline GvDw gv_dw_sink(const GvDw& o, size_t elems, int64_t splits) {
    if (!o.part || splits <= 1) return GvDw{o.dw, nullptr, 0, 0};
    return GvDw{o.dw, o.part, (elems + 3) / 4 * 4, o.cap_bytes};
}
// ... and the launch that follows it: dw[i] += part[0][i] + part[1][i] + ... in slice order (nothing to do for a plain sink)
int gv_dw_finish(const GvDw& o, size_t elems, int64_t splits, hipStream_t st);      // train.hip
#if defined(__HIPCC__)
__device__ __forceinline__ void gv_dw_put(const GvDw& o, int64_t slice, size_t idx, float v) {
    if (o.part) o.part[(size_t)slice * o.stride + idx] = v;      // (wave-uniform branch)
    else atomicAdd(&o.dw[idx], v);
}
// The tap-per-workgroup kernels (conv_wgrad2_f32, conv_wgrad_lp) take one argument list: the layer, `per`
// pixels a slice, the sink.
template <auto Kernel, typename E>
int gv_wgrad_launch(dim3 grid, const gv_conv_desc* d, const E* x, const E* dz, int dz_ld, int64_t per, const GvDw& sink,
                    hipStream_t st) {
    return gv_launch<Kernel>(grid, dim3(256), 0, st, x, d->x_ld, dz, dz_ld, d->nb, d->ih, d->iw, d->cin, d->kh, d->kw,
                             d->stride, d->pad_t, d->pad_l, d->oh, d->ow, d->cout, (int64_t)d->nb * d->oh * d->ow, per, sink);
}
#endif

// Bijective XCD-aware remap of a 1-D grid: blocks with equal (bid % 8) share an XCD (and its
// L2) under round-robin dispatch, so give each XCD one contiguous chunk of logical tile ids.
// Placement only changes speed, never results.
__device__ __forceinline__ int gv_xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// sum over the 64 lanes of a wave, valid in lane 0: a fixed tree, so the same bits every run
__device__ __forceinline__ float gv_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
