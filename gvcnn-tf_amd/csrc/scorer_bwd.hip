// scorer_bwd.hip — the gradient of the loss with respect to the grouping module's scores (per-shape form with
// mean_score weights, include/gvcnn_hip.h), down to the V Dense(1) scorer layers and the raw-tap activations.
//
//   w_g = mean_{v in M_g} s_v,  W = sum_g w_g,  S = sum_g w_g D_g / W
//   dL/dw_g = (1/W) sum_e dS_e (D_{g,e} - S_e)                       gv_group_weight_bwd_per_shape
//   dL/ds_v = dL/dw_{g(v)} / |M_{g(v)}|
//   dL/dr_b = dL/ds_b * sign(r_b) / (1 + |r_b|)^2                     gv_view_score_bwd
//   dbias_v = sum_n dr_{n,v},  dkernel_v[c] = sum_n dr_{n,v} mean_p raw[n,v,p,c],  draw[b,p,c] (+)= dr_b k_v[c] / hw
//
// The binning g(v) is piecewise constant: a constant of the backward pass, no straight-through term.  Every reduction
// is a fixed tree (wave shuffles, LDS, partials stored per workgroup and added in index order): no float atomics, two
// runs give the same bits.
#include <math.h>

#include "gv_common.h"
#include "group_table.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

constexpr int kGwChunk = 256;                         // element vectors per workgroup of group_weight_bwd (one per thread)

// Workgroup (chunk, n): ws[n][chunk][g] = sum over the chunk's elements of dS_e (D_{g,e} - S_e), S recomputed in
// registers from the forward kernel's group table and D_g (group_table.h; first pass over the groups), D_g formed a
// second time for the difference (the V vectors of a thread come from cache then).  Empty groups: 0 (their weight is 0
// in this form, so the fill value never enters S).
template <typename T, int VEC, typename E>
__global__ __launch_bounds__(256) void group_weight_bwd_kernel(const E* __restrict__ F, const float* __restrict__ dS, int V,
                                                               int64_t E_, int64_t view_stride, int64_t shape_stride,
                                                               const int* __restrict__ scheme, int G,
                                                               const float* __restrict__ weight, int mode,
                                                               float* __restrict__ ws) {
    using A = Px<E, T, VEC>;
    GROUP_TABLE_SHARED(tab);
    __shared__ float s_part[64][4];
    const int n = blockIdx.y;
    group_table_load<256>(tab, scheme + (size_t)n * G * V, weight + (size_t)n * G, G, V, true);
    const float wsum = *tab.W;
    const int64_t eg = E_ / VEC;
    const int64_t idx = (int64_t)blockIdx.x * kGwChunk + threadIdx.x;
    const bool live = idx < eg;                                   // (the last chunk is ragged: idle threads add 0)
    const int64_t e = live ? idx * VEC : 0;
    const E* base = F + (size_t)n * shape_stride + e;
    float s[VEC], ds[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = ds[k] = 0.f;
    if (live) {
        for (int g = 0; g < G; ++g) {
            const unsigned long long m = tab.mask[g];
            if (m == 0) continue;
            float d[VEC];
            pooled_group<A>(base, view_stride, m, mode, d);
            const float w = tab.w[g];
#pragma unroll
            for (int k = 0; k < VEC; ++k) s[k] = __fadd_rn(s[k], __fmul_rn(w, d[k]));
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) s[k] = wsum != 0.f ? __fdiv_rn(s[k], wsum) : 0.f;
        const float* g_ = dS + (size_t)n * E_ + e;
        if constexpr (VEC >= 4) {
#pragma unroll
            for (int q = 0; q < VEC / 4; ++q) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(g_ + 4 * q);
                ds[4 * q] = t[0]; ds[4 * q + 1] = t[1]; ds[4 * q + 2] = t[2]; ds[4 * q + 3] = t[3];
            }
        } else {
            ds[0] = g_[0];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int g = 0; g < G; ++g) {                                 // (the mask is uniform: no divergence around the shuffles)
        const unsigned long long m = tab.mask[g];
        float t = 0.f;
        if (m != 0) {
            if (live) {
                float d[VEC];
                pooled_group<A>(base, view_stride, m, mode, d);
#pragma unroll
                for (int k = 0; k < VEC; ++k) t += ds[k] * (d[k] - s[k]);
            }
            t = gv_wave_sum(t);
        }
        if (lane == 0) s_part[g][wave] = t;
    }
    __syncthreads();
    if (threadIdx.x < G) {
        const float* p = s_part[threadIdx.x];
        ws[((size_t)n * gridDim.x + blockIdx.x) * G + threadIdx.x] = (p[0] + p[1]) + (p[2] + p[3]);
    }
}

// dw[n][g] = (sum of the chunks in ascending order) / W; 0 for an empty group and for W = 0
__global__ __launch_bounds__(64) void group_weight_bwd_finish(const float* __restrict__ ws, int chunks,
                                                              const int* __restrict__ scheme, int V, int G,
                                                              const float* __restrict__ weight, float* __restrict__ dw) {
    GROUP_TABLE_SHARED(tab);
    const int n = blockIdx.x, g = threadIdx.x;
    group_table_load<64>(tab, scheme + (size_t)n * G * V, weight + (size_t)n * G, G, V, true);
    if (g >= G) return;
    const float wsum = *tab.W;
    float t = 0.f;
    for (int c = 0; c < chunks; ++c) t += ws[((size_t)n * chunks + c) * G + g];
    dw[(size_t)n * G + g] = (tab.mask[g] != 0 && wsum != 0.f) ? t / wsum : 0.f;
}

// dL/dr of image (n, v): the members of v's group are counted from gidx; a view in no group (gidx outside [0, G):
// status bits 1 / 2 of the assignment) and r = 0 get 0.  fp64: a handful of operations per image, and the raw-tap term
// built from it is then one rounding away from the exact value.
__device__ __forceinline__ double score_dr(const float* __restrict__ r_img, const int* __restrict__ gidx,
                                           const float* __restrict__ dw, int G, int V, int n, int v) {
    const int* gi = gidx + (size_t)n * V;
    const int g = gi[v];
    if (g < 0 || g >= G) return 0.0;
    int cnt = 0;
    for (int u = 0; u < V; ++u) cnt += gi[u] == g ? 1 : 0;
    const float r = r_img[(size_t)n * V + v];
    if (r == 0.f || r != r) return 0.0;
    const double q = 1.0 + fabs((double)r);                       // (1 - s)^2 = 1 / (1 + |r|)^2, without the cancellation
    const double d = (double)dw[(size_t)n * G + g] / (double)cnt / (q * q);     // of 1 - s as s -> 1
    return r < 0.f ? -d : d;
}

// dbias[v] = sum_n dr_{n,v}, n ascending; one thread per view
__global__ void score_dbias_kernel(const float* __restrict__ r_img,
                                   const int* __restrict__ gidx, const float* __restrict__ dw, int G, int V, int N,
                                   float* __restrict__ dbias) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    double t = 0.0;
    for (int n = 0; n < N; ++n) t += score_dr(r_img, gidx, dw, G, V, n, v);
    dbias[v] = (float)t;
}

// dkernel[v][c] = (1/hw) sum_n dr_{n,v} sum_p raw[n,v,p,c].  Workgroup (channel chunk, view): 8 channel vectors x 32
// pixel lanes; a thread adds its pixels of one image (p ascending), scales by dr, goes on to the next image (n
// ascending); the 32 pixel lanes meet in a fixed LDS tree.
template <typename T, int VEC, typename E>
__global__ __launch_bounds__(256) void score_dkernel_kernel(const E* __restrict__ raw, int N, int V, int hw, int cr,
                                                            int raw_ld, const float* __restrict__ r_img,
                                                            const int* __restrict__ gidx, const float* __restrict__ dw,
                                                            int G, float* __restrict__ dkernel) {
    __shared__ float s_dr[256];
    __shared__ float s_red[32][8][VEC + 1];
    const int v = blockIdx.y;
    const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int c0 = (blockIdx.x * 8 + cl) * VEC;
    const bool live = c0 < cr;                                    // (cr is a multiple of VEC on the vector path)
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int n0 = 0; n0 < N; n0 += 256) {
        __syncthreads();
        if (n0 + (int)threadIdx.x < N)
            s_dr[threadIdx.x] = (float)score_dr(r_img, gidx, dw, G, V, n0 + threadIdx.x, v);
        __syncthreads();
        const int nn = min(256, N - n0);
        if (!live) continue;
        for (int i = 0; i < nn; ++i) {
            const float dr = s_dr[i];
            if (dr == 0.f) continue;                              // (uniform over the workgroup; adds nothing)
            const E* xb = raw + ((size_t)(n0 + i) * V + v) * hw * raw_ld + c0;
            float a[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < 8; ++k) a[u][k] = 0.f;
            int p = pl;
            for (; p + 96 < hw; p += 128) {                       // four loads in flight, each into its own partial sum
                float x[4][8];
#pragma unroll
                for (int u = 0; u < 4; ++u) load_v<T, VEC>(xb + (size_t)(p + 32 * u) * raw_ld, x[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int k = 0; k < VEC; ++k) a[u][k] += x[u][k];
            }
            for (; p < hw; p += 32) {
                float x[8];
                load_v<T, VEC>(xb + (size_t)p * raw_ld, x);
#pragma unroll
                for (int k = 0; k < VEC; ++k) a[0][k] += x[k];
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += dr * ((a[0][k] + a[1][k]) + (a[2][k] + a[3][k]));
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) s_red[pl][cl][k] = acc[k];
    __syncthreads();
    for (int half = 16; half > 0; half >>= 1) {
        if (pl < half) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) s_red[pl][cl][k] += s_red[pl + half][cl][k];
        }
        __syncthreads();
    }
    if (pl == 0 && live) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) dkernel[(size_t)v * cr + c0 + k] = s_red[0][cl][k] / (float)hw;
    }
}

// draw[b][p][c] (+)= dr_b k_v[c] / hw.  Workgroup (pixel slab, image); the term depends on (b, c) only: a thread forms
// it once per channel vector (fp64, so the stored value is ONE rounding of the exact one) and walks the pixels.
template <typename T, int VEC, typename E>
__global__ __launch_bounds__(256) void score_draw_kernel(int V, int hw, int cr, const float* __restrict__ kernel,
                                                         const float* __restrict__ r_img, const int* __restrict__ gidx,
                                                         const float* __restrict__ dw, int G, E* __restrict__ draw,
                                                         int draw_ld, int accumulate, int slab) {
    const int b = blockIdx.y, n = b / V, v = b - n * V;
    const double dr = score_dr(r_img, gidx, dw, G, V, n, v);       // (every thread: V cached loads)
    if (accumulate && dr == 0.0) return;                          // adds nothing
    const int cv = cr / VEC;
    const int p0 = blockIdx.x * slab, p1 = min(hw, p0 + slab);
    E* db = draw + (size_t)b * hw * draw_ld;
    const float* kv = kernel + (size_t)v * cr;
    const double scale = dr / (double)hw;
    // threads along the channel vectors first (contiguous stores), the rest of the workgroup along the pixels
    int tc = 1;
    while (tc < cv && tc < 256) tc <<= 1;
    const int tp = 256 / tc;
    const int ci = threadIdx.x % tc, pi = threadIdx.x / tc;
    for (int c = ci; c < cv; c += tc) {
        double t[8];
#pragma unroll
        for (int k = 0; k < VEC; ++k) t[k] = scale * (double)kv[c * VEC + k];
        if (!accumulate) {
            float f[8];
#pragma unroll
            for (int k = 0; k < VEC; ++k) f[k] = (float)t[k];
            for (int p = p0 + pi; p < p1; p += tp) store_v<T, VEC>(db + (size_t)p * draw_ld + c * VEC, f);
        } else {
            for (int p = p0 + pi; p < p1; p += tp) {
                float f[8];
                load_v<T, VEC>(db + (size_t)p * draw_ld + c * VEC, f);
#pragma unroll
                for (int k = 0; k < VEC; ++k) f[k] = (float)((double)f[k] + t[k]);
                store_v<T, VEC>(db + (size_t)p * draw_ld + c * VEC, f);
            }
        }
    }
}

template <typename T, int VEC, typename E>
int group_weight_bwd_launch(const void* F, const float* dS, int V, int N, int64_t E_, int64_t vs, int64_t ss,
                            const int* scheme, int G, const float* weight, int mode, float* dw, float* ws,
                            hipStream_t st) {
    const int64_t chunks = (E_ / VEC + kGwChunk - 1) / kGwChunk;
    hipLaunchKernelGGL((group_weight_bwd_kernel<T, VEC, E>), dim3((unsigned)chunks, (unsigned)N), dim3(256), 0, st,
                       (const E*)F, dS, V, E_, vs, ss, scheme, G, weight, mode, ws);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_weight_bwd_finish, dim3((unsigned)N), dim3(64), 0, st, ws, (int)chunks, scheme, V, G, weight,
                       dw);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

template <typename T, int VEC, typename E>
int score_bwd_launch(const void* raw, int N, int V, int hw, int cr, int raw_ld, const float* kernel, const float* r_img,
                     const int* gidx, const float* dw, int G, float* dkernel, void* draw,
                     int draw_ld, int accumulate, hipStream_t st) {
    const int chunks = (cr / VEC + 7) / 8;
    hipLaunchKernelGGL((score_dkernel_kernel<T, VEC, E>), dim3((unsigned)chunks, (unsigned)V), dim3(256), 0, st,
                       (const E*)raw, N, V, hw, cr, raw_ld, r_img, gidx, dw, G, dkernel);
    GV_LAUNCH_CHECK();
    if (draw) {
        // pixel slabs: enough workgroups per image to fill the chip at small batches, whole rows of work at large ones
        int slabs = (int)((2048 + (int64_t)N * V - 1) / ((int64_t)N * V));
        if (slabs > hw) slabs = hw;
        if (slabs > 65535) slabs = 65535;
        const int slab = (hw + slabs - 1) / slabs;
        slabs = (hw + slab - 1) / slab;
        hipLaunchKernelGGL((score_draw_kernel<T, VEC, E>), dim3((unsigned)slabs, (unsigned)(N * V)), dim3(256), 0, st, V, hw,
                           cr, kernel, r_img, gidx, dw, G, (E*)draw, draw_ld, accumulate, slab);
        GV_LAUNCH_CHECK();
    }
    return GV_OK;
}

// chunks of the SCALAR path: the most any path of this call uses
int64_t gw_chunks_max(int64_t E_) { return (E_ + kGwChunk - 1) / kGwChunk; }

}  // namespace

extern "C" int64_t gv_group_weight_bwd_workspace_bytes(int32_t num_shapes, int64_t E, int32_t num_groups) {
    if (num_shapes <= 0 || E <= 0 || num_groups <= 0) return GV_E_BADARG;
    if (num_groups > 64 || num_shapes > 65535) return GV_E_UNSUPPORTED;
    return (int64_t)num_shapes * gw_chunks_max(E) * num_groups * (int64_t)sizeof(float);
}

extern "C" int gv_group_weight_bwd_per_shape(const void* F, const float* dS, int32_t num_views, int32_t num_shapes,
                                             int64_t E, int64_t view_stride, int64_t shape_stride,
                                             const int32_t* scheme, int32_t num_groups, const float* weight,
                                             int32_t mode, float* dw, void* ws, int64_t ws_bytes, int32_t dtype,
                                             void* stream) {
    if (dtype != GV_F32 && dtype != GV_BF16 && dtype != GV_F16) return GV_E_UNSUPPORTED;
    if (!F || !dS || !scheme || !weight || !dw || !ws) return GV_E_BADARG;
    if (num_views <= 0 || num_shapes <= 0 || E <= 0 || num_groups <= 0 || view_stride < 0 || shape_stride < 0)
        return GV_E_BADARG;
    if (mode != GV_VIEWPOOL_MAX && mode != GV_VIEWPOOL_MEAN) return GV_E_BADARG;
    if (num_views > 64 || num_groups > 64 || num_shapes > 65535) return GV_E_UNSUPPORTED;
    if (gw_chunks_max(E) > 0x7fffffff) return GV_E_UNSUPPORTED;
    if (ws_bytes < gv_group_weight_bwd_workspace_bytes(num_shapes, E, num_groups)) return GV_E_BADARG;
    if (((uintptr_t)ws) & 3u) return GV_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int vw = dtype == GV_F32 ? 4 : 8;
    const bool vec = E % vw == 0 && view_stride % vw == 0 && shape_stride % vw == 0 && gv_aligned16(F) && gv_aligned16(dS);
#define GW_ARGS F, dS, num_views, num_shapes, E, view_stride, shape_stride, scheme, num_groups, weight, mode, dw, (float*)ws, st
    if (dtype == GV_F32)
        return vec ? group_weight_bwd_launch<float, 4, float>(GW_ARGS) : group_weight_bwd_launch<float, 1, float>(GW_ARGS);
    if (dtype == GV_BF16)
        return vec ? group_weight_bwd_launch<__bf16, 8, unsigned short>(GW_ARGS)
                   : group_weight_bwd_launch<__bf16, 1, unsigned short>(GW_ARGS);
    return vec ? group_weight_bwd_launch<_Float16, 8, unsigned short>(GW_ARGS)
               : group_weight_bwd_launch<_Float16, 1, unsigned short>(GW_ARGS);
#undef GW_ARGS
}

extern "C" int gv_view_score_bwd(const void* raw, int32_t nb, int32_t hw, int32_t cr, int32_t raw_ld,
                                 const float* kernel, const float* r_img, const int32_t* gidx,
                                 const float* dw, int32_t num_groups, int32_t num_views, float* dkernel, float* dbias,
                                 void* draw, int32_t draw_ld, int32_t accumulate, int32_t dtype, void* stream) {
    if (dtype != GV_F32 && dtype != GV_BF16 && dtype != GV_F16) return GV_E_UNSUPPORTED;
    if (!raw || !kernel || !r_img || !gidx || !dw || !dkernel || !dbias) return GV_E_BADARG;
    if (nb <= 0 || hw <= 0 || cr <= 0 || raw_ld < cr || num_groups <= 0 || num_views <= 0 || nb % num_views != 0)
        return GV_E_BADARG;
    if (draw && draw_ld < cr) return GV_E_BADARG;
    if (accumulate != 0 && accumulate != 1) return GV_E_BADARG;
    if (num_views > 64 || num_groups > 64 || nb > 65535) return GV_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int N = nb / num_views, V = num_views;
    hipLaunchKernelGGL(score_dbias_kernel, dim3(1), dim3(64), 0, st, r_img, gidx, dw, num_groups, V, N, dbias);
    GV_LAUNCH_CHECK();
    const int vw = dtype == GV_F32 ? 4 : 8;
    const bool vec = cr % vw == 0 && gv_vec_ok(raw, raw_ld, vw) && gv_vec_ok(draw, draw_ld, vw);
#define SB_ARGS raw, N, V, hw, cr, raw_ld, kernel, r_img, gidx, dw, num_groups, dkernel, draw, draw_ld, accumulate, st
    if (dtype == GV_F32) return vec ? score_bwd_launch<float, 4, float>(SB_ARGS) : score_bwd_launch<float, 1, float>(SB_ARGS);
    if (dtype == GV_BF16)
        return vec ? score_bwd_launch<__bf16, 8, unsigned short>(SB_ARGS) : score_bwd_launch<__bf16, 1, unsigned short>(SB_ARGS);
    return vec ? score_bwd_launch<_Float16, 8, unsigned short>(SB_ARGS) : score_bwd_launch<_Float16, 1, unsigned short>(SB_ARGS);
#undef SB_ARGS
}
