// grouping.hip — the grouping module of nets/model.py on device, forward and backward (the scorer partial and the view
// pool + fusion with its backward for every storage type; the rest is fp32).
//
//   scorer            model.py:144-147   GAP -> Dense(1) per view -> batch mean -> sigmoid(log|.|)
//   group assignment  model.py:16-41     bin = (int)(score * 10f) ; weight = 1 + count
//   view pooling      model.py:44-74     per group: max over its views, ones when empty
//   group fusion      model.py:77-102    sum_g w_g D_g / sum_g w_g          (the group table and D_g: group_table.h)
//   classifier        model.py:163-164   GAP -> Dense(C)
//
// The reference computes scheme/weight with host numpy between two partial_run calls
// (train.py:270-288): scores D2H, Python loops, scheme/weight H2D.  Here they stay on device.
// The pooling + fusion kernel is a single pass over the V view descriptors: every descriptor
// element is read exactly once (the algorithmic minimum; the TF graph makes >= 3 passes).
#include <math.h>

#include "gv_common.h"
#include "group_table.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

__device__ __forceinline__ int view_of_image(int b, int num_views, int num_shapes, int order) {
    return order == GV_ORDER_SHAPE_MAJOR ? b % num_views : b / num_shapes;
}

// x[0] * k[0] + x[1] * k[1] + ... of one N-element chunk, left to right; k (16-byte aligned) is read in quads
template <int N>
__device__ __forceinline__ float chunk_dot(const float (&x)[8], const float* __restrict__ k) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
        const f32x4 kq = *reinterpret_cast<const f32x4*>(k + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) t = q + e == 0 ? x[0] * kq[0] : t + x[4 * q + e] * kq[e];
    }
    return t;
}

// nets/model.py:144-145: r_img[b] = (1/hw) * sum_{p,c} raw[b,p,c] * k[v(b)][c] + bias[v(b)]; one workgroup per image,
// fixed reduction tree => bitwise reproducible.  E the element type of the raw map in HBM, T the type it stands for.
template <typename E, typename T>
__global__ __launch_bounds__(256) void view_score_partial(const E* __restrict__ raw, int hw, int cr, int raw_ld,
                                                          const float* __restrict__ kernel, const float* __restrict__ bias,
                                                          int num_views, int num_shapes, int order,
                                                          float* __restrict__ r_img) {
    constexpr int N = 16 / sizeof(E);               // elements of a 16-byte chunk
    const int b = blockIdx.x;
    const int v = view_of_image(b, num_views, num_shapes, order);
    const float* kv = kernel + (size_t)v * cr;
    const E* xb = raw + (size_t)b * hw * raw_ld;
    float s = 0.f;
    if (cr % N == 0 && raw_ld % N == 0 && ((((uintptr_t)raw) | ((uintptr_t)kernel)) & 15) == 0) {
        const int cg = cr / N;
        const int total = hw * cg;
        // four chunks in flight per thread, each into its own partial sum (one load at a time left this 85 MB read
        // latency-bound: 69 us for the raw tap of 384 views, 1.2 TB/s); the order of the additions is fixed, so every rank
        // of a sharded job still computes the same bits
        float sp[4] = {0.f, 0.f, 0.f, 0.f};
        int i = threadIdx.x;
        for (; i + 3 * 256 < total; i += 4 * 256) {
            u32x4 q[4];
            int gq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ii = i + u * 256;
                const int p = ii / cg;
                gq[u] = ii - p * cg;
                q[u] = *reinterpret_cast<const u32x4*>(xb + (size_t)p * raw_ld + N * gq[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float x[8];
                unpackq<E, T>(q[u], x);
                sp[u] += chunk_dot<N>(x, kv + N * gq[u]);
            }
        }
        for (; i < total; i += 256) {
            const int p = i / cg, g = i - p * cg;
            float x[8];
            unpackq<E, T>(*reinterpret_cast<const u32x4*>(xb + (size_t)p * raw_ld + N * g), x);
            if constexpr (sizeof(E) == 4) {
                sp[0] += chunk_dot<N>(x, kv + N * g);
            } else {                                // (16-bit storage adds a tail chunk's products to sp[0] one by one)
#pragma unroll
                for (int e = 0; e < N; ++e) sp[0] += x[e] * kv[N * g + e];
            }
        }
        s = (sp[0] + sp[1]) + (sp[2] + sp[3]);
    } else {
        const int total = hw * cr;
        for (int i = threadIdx.x; i < total; i += 256) {
            const int p = i / cr, c = i - p * cr;
            s += up<T>(xb[(size_t)p * raw_ld + c]) * kv[c];
        }
    }
    __shared__ float part[4];
    s = gv_wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) r_img[b] = (part[0] + part[1] + part[2] + part[3]) / (float)hw + bias[v];
}

// sigmoid(log|r|) (model.py:147); r == 0 -> log = -inf -> score 0
__device__ __forceinline__ float view_score(float r) {
    const float lg = logf(fabsf(r));
    return 1.0f / (1.0f + expf(-lg));
}

// score[v] = sigmoid(log(|mean_n r_img[b(n,v)]|)); one thread per view, n ascending.
__global__ void view_score_finalize_f32(const float* __restrict__ r_img, int num_shapes, int num_views,
                                        int order, float* __restrict__ scores) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= num_views) return;
    float s = 0.f;
    for (int n = 0; n < num_shapes; ++n)
        s += r_img[order == GV_ORDER_SHAPE_MAJOR ? n * num_views + v : v * num_shapes + n];
    scores[v] = view_score(s / (float)num_shapes);
}

// sigmoid(log|r|) per image (the paper's per-shape scorer; model.py:147 without the batch mean of :146)
__global__ void view_score_per_shape_f32(const float* __restrict__ r_img, int nb, float* __restrict__ scores) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    scores[b] = view_score(r_img[b]);
}

// One workgroup per scheme (a batch-level call has one, a per-shape call one per shape).  Integer path: must be bit-exact
// with numpy's int(np.float32(score) * 10).  Status bits: 1 a bin outside [0, G), 2 a NaN score; or_status: the word was
// cleared before the launch and every workgroup ORs its bits in, else the one workgroup overwrites it.
__global__ __launch_bounds__(64) void group_assign_kernel(const float* __restrict__ scores, int V, int G, int num_bins,
                                                          int weight_mode, int* __restrict__ gidx,
                                                          int* __restrict__ scheme, float* __restrict__ weight,
                                                          int* __restrict__ status, int or_status) {
    __shared__ int s_gidx[64];
    __shared__ float s_score[64];
    __shared__ int s_status;
    const int n = blockIdx.x, t = threadIdx.x;
    scores += (size_t)n * V;
    gidx += (size_t)n * V;
    scheme += (size_t)n * G * V;
    weight += (size_t)n * G;
    if (t == 0) s_status = 0;
    __syncthreads();
    if (t < V) {
        const float sc = scores[t];
        const float prod = __fmul_rn(sc, (float)num_bins);   // one IEEE fp32 multiply, no contraction
        int b = (int)prod;                                   // truncation toward zero
        if (sc != sc) { atomicOr(&s_status, 2); b = -1; }
        else if (b >= G || b < 0 || prod >= 2147483648.0f) { atomicOr(&s_status, 1); if (prod >= 2147483648.0f) b = 0x7fffffff; }
        s_gidx[t] = b;
        s_score[t] = sc;
        gidx[t] = b;
    }
    __syncthreads();
    for (int i = t; i < G * V; i += 64) {
        const int g = i / V, v = i - g * V;
        scheme[i] = (s_gidx[v] == g) ? 1 : 0;
    }
    for (int g = t; g < G; g += 64) {
        int cnt = 0;
        float sum = 0.f;
        for (int v = 0; v < V; ++v)
            if (s_gidx[v] == g) { ++cnt; sum = __fadd_rn(sum, s_score[v]); }      // view order: reproducible
        // GV_WEIGHT_COUNT: model.py:32 `sum = 1`
        weight[g] = weight_mode == GV_WEIGHT_COUNT ? (float)(1 + cnt) : (cnt ? __fdiv_rn(sum, (float)cnt) : 0.f);
    }
    if (t == 0) {
        if (!or_status) *status = s_status;
        else if (s_status) atomicOr(status, s_status);
    }
}

__global__ void group_weight_kernel(const int* __restrict__ scheme, int G, int V, float* __restrict__ weight) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    int cnt = 1;                                              // model.py:32 `sum = 1`
    for (int v = 0; v < V; ++v) cnt += (scheme[g * V + v] == 1) ? 1 : 0;   // model.py:34
    weight[g] = (float)cnt;
}

// Fused view pooling + group fusion.  Thread per (shape n, VEC consecutive descriptor elements).
// Group membership is turned into per-group 64-bit view masks held in LDS; each view of each
// group is loaded once, so a one-hot scheme costs exactly V loads per output element.
// Order of the fp32 operations (numpy float32 reproduces it bit for bit): D_g and wsum as group_table.h forms them;
// S = fl(w_g * D_g) added in ascending g, one division by wsum.  The
// header's __fmul_rn / __fadd_rn are plain operators that hipcc contracts into one FMA by default, wherever they are called
// from (render.hip), so the kernel body turns contraction off and spells the fusion with plain operators: the product is
// rounded before it is added, as tf.multiply + tf.add_n round it.
// 16-bit storage: one rounding of D and of S into the storage type, each from the unrounded fp32 value.
template <class A>
__global__ __launch_bounds__(256) void view_pool_fuse(const typename A::elem* __restrict__ F, int V, int N, int64_t E,
                                                      int64_t view_stride, int64_t shape_stride,
                                                      const int* __restrict__ scheme, int G,
                                                      const float* __restrict__ weight, int mode, float fill,
                                                      typename A::elem* __restrict__ D, typename A::elem* __restrict__ S,
                                                      int64_t scheme_stride, int64_t weight_stride) {
#pragma clang fp contract(off)
    constexpr int VEC = A::N;
    GROUP_TABLE_SHARED(tab);
    const int n = blockIdx.y;                       // one shape per grid row: its own scheme when strides != 0
    group_table_load<256>(tab, scheme + (size_t)n * scheme_stride, weight + (size_t)n * weight_stride, G, V, false);
    const float wsum = *tab.W;
    const int64_t eg = E / VEC;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < eg;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = idx * VEC;
        const typename A::elem* base = F + (size_t)n * shape_stride + e;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int g = 0; g < G; ++g) {
            const unsigned long long m = tab.mask[g];
            float d[VEC];
            if (m == 0) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) d[k] = fill;
            } else {
                pooled_group<A>(base, view_stride, m, mode, d);
            }
            if (D) A::store(D + ((size_t)g * N + n) * E + e, 0, 0, 0, d);
            const float w = tab.w[g];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + w * d[k];   // multiply, add_n: two roundings (contraction is off)
        }
        if (S) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = wsum != 0.f ? __fdiv_rn(acc[k], wsum) : 0.f;   // tf.div
            A::store(S + (size_t)n * E + e, 0, 0, 0, acc);
        }
    }
}

// The backward of view_pool_fuse (nets/model.py:44-102):
// dF[v] += w_g/sum(w) * dS / (#views of g tied at the maximum) for every view of g attaining the maximum
// (tf.reduce_max splits the gradient equally among ties); mean pooling: w_g/sum(w) * dS / |g|.
// F and dF in the storage type (SE the element in HBM, T the type it stands for), dS in fp32.
template <typename SE, typename T>
__global__ __launch_bounds__(256) void view_pool_fuse_bwd_t(
    const SE* __restrict__ F, const float* __restrict__ dS, int V, int N, int64_t E, int64_t view_stride,
    int64_t shape_stride, const int* __restrict__ scheme, int G, const float* __restrict__ weight, int mode,
    SE* __restrict__ dF, int64_t scheme_stride, int64_t weight_stride) {
    GROUP_TABLE_SHARED(tab);
    const int n = blockIdx.y;                       // one shape per grid row: its own scheme when strides != 0
    group_table_load<256>(tab, scheme + (size_t)n * scheme_stride, weight + (size_t)n * weight_stride, G, V, false);
    const float wsum = *tab.W;
    if (wsum == 0.f) return;                       // (per-shape, mean-score weights) S = 0 for this shape: no gradient
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const size_t base = (size_t)n * shape_stride + e;
        const float ds = dS[(size_t)n * E + e];
        for (int g = 0; g < G; ++g) {
            const unsigned long long m0 = tab.mask[g];
            if (m0 == 0) continue;
            const float coef = tab.w[g] / wsum * ds;
            if (mode == GV_VIEWPOOL_MEAN) {
                const float each = coef / (float)__popcll(m0);
                for (unsigned long long m = m0; m; m &= m - 1) {
                    const size_t a = base + (size_t)(__ffsll((long long)m) - 1) * view_stride;
                    dF[a] = down<T>(up<T>(dF[a]) + each);
                }
            } else {
                float best = -INFINITY;
                for (unsigned long long m = m0; m; m &= m - 1)
                    best = fmaxf(best, up<T>(F[base + (size_t)(__ffsll((long long)m) - 1) * view_stride]));
                int ties = 0;
                for (unsigned long long m = m0; m; m &= m - 1)
                    ties += up<T>(F[base + (size_t)(__ffsll((long long)m) - 1) * view_stride]) == best;
                const float each = coef / (float)ties;
                for (unsigned long long m = m0; m; m &= m - 1) {
                    const size_t a = base + (size_t)(__ffsll((long long)m) - 1) * view_stride;
                    if (up<T>(F[a]) == best) dF[a] = down<T>(up<T>(dF[a]) + each);
                }
            }
        }
    }
}

// y[n][c] = x[n][:] . kernel[:, c] + bias[c]; one workgroup per (n, c) pair group.
__global__ __launch_bounds__(256) void dense_f32(const float* __restrict__ x, int f,
                                                 const float* __restrict__ kernel,
                                                 const float* __restrict__ bias, int c,
                                                 float* __restrict__ y) {
    const int n = blockIdx.x;
    const int cc = blockIdx.y;
    const float* xr = x + (size_t)n * f;
    float s = 0.f;
    for (int i = threadIdx.x; i < f; i += 256) s += xr[i] * kernel[(size_t)i * c + cc];
    __shared__ float part[4];
    s = gv_wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) y[(size_t)n * c + cc] = part[0] + part[1] + part[2] + part[3] + bias[cc];
}

}  // namespace

extern "C" int gv_view_score_partial(const void* raw, int32_t nb, int32_t hw, int32_t cr,
                                     int32_t raw_ld, const float* kernel, const float* bias,
                                     int32_t num_views, int32_t order, float* r_img, int32_t dtype,
                                     void* stream) {
    if (!raw || !kernel || !bias || !r_img || nb <= 0 || hw <= 0 || cr <= 0 || raw_ld < cr ||
        num_views <= 0 || nb % num_views != 0)
        return GV_E_BADARG;
    if (order != GV_ORDER_SHAPE_MAJOR && order != GV_ORDER_VIEW_MAJOR) return GV_E_BADARG;
    GV_ST_DISPATCH(dtype, return (gv_launch<view_score_partial<E, T>>(dim3(nb), dim3(256), 0, (hipStream_t)stream, (const E*)raw,
                                                                      hw, cr, raw_ld, kernel, bias, num_views, nb / num_views,
                                                                      order, r_img)));
}

extern "C" int gv_view_score_finalize(const float* r_img, int32_t num_shapes, int32_t num_views,
                                      int32_t order, float* scores, void* stream) {
    if (!r_img || !scores || num_shapes <= 0 || num_views <= 0) return GV_E_BADARG;
    if (order != GV_ORDER_SHAPE_MAJOR && order != GV_ORDER_VIEW_MAJOR) return GV_E_BADARG;
    hipLaunchKernelGGL(view_score_finalize_f32, dim3((num_views + 63) / 64), dim3(64), 0,
                       (hipStream_t)stream, r_img, num_shapes, num_views, order, scores);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

// the checks of both assign entry points are done: one workgroup per scheme
static int assign_launch(const float* scores, int num_schemes, int V, int G, int num_bins, int weight_mode, int32_t* gidx,
                         int32_t* scheme, float* weight, int32_t* status, int or_status, void* stream) {
    hipLaunchKernelGGL(group_assign_kernel, dim3(num_schemes), dim3(64), 0, (hipStream_t)stream, scores, V, G, num_bins,
                       weight_mode, gidx, scheme, weight, status, or_status);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_group_assign(const float* scores, int32_t num_views, int32_t num_groups,
                               int32_t num_bins, int32_t* gidx, int32_t* scheme, float* weight,
                               int32_t* status, void* stream) {
    if (!scores || !gidx || !scheme || !weight || !status) return GV_E_BADARG;
    if (num_views <= 0 || num_groups <= 0 || num_bins <= 0) return GV_E_BADARG;
    if (num_views > 64 || num_groups > 64) return GV_E_UNSUPPORTED;
    return assign_launch(scores, 1, num_views, num_groups, num_bins, GV_WEIGHT_COUNT, gidx, scheme, weight, status, 0, stream);
}

extern "C" int gv_group_weight(const int32_t* scheme, int32_t num_groups, int32_t num_views,
                               float* weight, void* stream) {
    if (!scheme || !weight || num_groups <= 0 || num_views <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(group_weight_kernel, dim3((num_groups + 63) / 64), dim3(64), 0,
                       (hipStream_t)stream, scheme, num_groups, num_views, weight);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

static int pool_fuse_launch(const void* F, int32_t num_views, int32_t num_shapes, int64_t E, int64_t view_stride,
                            int64_t shape_stride, const int32_t* scheme, int32_t num_groups, const float* weight,
                            int32_t mode, float empty_fill, void* D, void* S, int32_t dtype, void* stream,
                            int64_t scheme_stride, int64_t weight_stride) {
    if (!F || !scheme || !weight || (!D && !S)) return GV_E_BADARG;
    if (num_views <= 0 || num_shapes <= 0 || E <= 0 || num_groups <= 0 || view_stride < 0 ||
        shape_stride < 0)
        return GV_E_BADARG;
    if (mode != GV_VIEWPOOL_MAX && mode != GV_VIEWPOOL_MEAN) return GV_E_BADARG;
    if (num_views > 64 || num_groups > 64 || num_shapes > 65535) return GV_E_UNSUPPORTED;
    const int quad = dtype == GV_F32 ? 4 : 8;
    const bool vec = (E % quad == 0) && (view_stride % quad == 0) && (shape_stride % quad == 0) &&
                     gv_aligned16(F) && (!D || gv_aligned16(D)) && (!S || gv_aligned16(S));
    const int64_t per_shape = vec ? E / quad : E;
    int64_t bx = (per_shape + 255) / 256;
    if (bx > 1024) bx = 1024;
    const dim3 grid((unsigned)bx, (unsigned)num_shapes);
    const int64_t ne = E;                                        // (GV_ST_DISPATCH names the element type E)
#define GV_FUSE(NN)                                                                                                       \
    return (gv_launch<view_pool_fuse<Px<E, T, NN>>>(grid, dim3(256), 0, (hipStream_t)stream, (const E*)F, num_views,      \
                                                     num_shapes, ne, view_stride, shape_stride, scheme, num_groups, weight, \
                                                     mode, empty_fill, (E*)D, (E*)S, scheme_stride, weight_stride))
    if (vec) GV_ST_DISPATCH(dtype, GV_FUSE(16 / sizeof(E)));
    GV_ST_DISPATCH(dtype, GV_FUSE(1));
#undef GV_FUSE
}

extern "C" int gv_view_pool_fuse_fwd(const void* F, int32_t num_views, int32_t num_shapes, int64_t E,
                                     int64_t view_stride, int64_t shape_stride,
                                     const int32_t* scheme, int32_t num_groups, const float* weight,
                                     int32_t mode, float empty_fill, void* D, void* S, int32_t dtype,
                                     void* stream) {
    return pool_fuse_launch(F, num_views, num_shapes, E, view_stride, shape_stride, scheme, num_groups, weight, mode,
                            empty_fill, D, S, dtype, stream, 0, 0);
}

extern "C" int gv_view_pool_fuse_fwd_per_shape(const void* F, int32_t num_views, int32_t num_shapes, int64_t E,
                                               int64_t view_stride, int64_t shape_stride, const int32_t* scheme,
                                               int32_t num_groups, const float* weight, int32_t mode,
                                               float empty_fill, void* D, void* S, int32_t dtype, void* stream) {
    return pool_fuse_launch(F, num_views, num_shapes, E, view_stride, shape_stride, scheme, num_groups, weight, mode,
                            empty_fill, D, S, dtype, stream, (int64_t)num_groups * num_views, num_groups);
}

// per_shape: every shape has its own scheme ([num_groups][num_views]) and weights ([num_groups]); else one for the batch
extern "C" int gv_view_pool_fuse_bwd_t(const void* F, const float* dS, int32_t num_views, int32_t num_shapes,
                                       int64_t n_elem, int64_t view_stride, int64_t shape_stride, const int32_t* scheme,
                                       int32_t num_groups, const float* weight, int32_t mode, void* dF,
                                       int32_t per_shape, int32_t dtype, void* stream) {
    if (!gv_storage_type(dtype)) return GV_E_UNSUPPORTED;
    if (!F || !dS || !scheme || !weight || !dF) return GV_E_BADARG;
    if (num_views <= 0 || num_shapes <= 0 || n_elem <= 0 || num_groups <= 0) return GV_E_BADARG;
    if (num_views > 64 || num_groups > 64 || num_shapes > 65535) return GV_E_UNSUPPORTED;
    const int64_t ss = per_shape ? (int64_t)num_groups * num_views : 0, ws = per_shape ? num_groups : 0;
    int64_t bx = (n_elem + 255) / 256;
    if (bx > 1024) bx = 1024;
    const dim3 grid((unsigned)bx, (unsigned)num_shapes);
    GV_ST_DISPATCH(dtype, {
        hipLaunchKernelGGL((view_pool_fuse_bwd_t<E, T>), grid, dim3(256), 0, (hipStream_t)stream, (const E*)F, dS, num_views,
                           num_shapes, n_elem, view_stride, shape_stride, scheme, num_groups, weight, mode, (E*)dF, ss, ws);
        GV_LAUNCH_CHECK();
        return GV_OK;
    });
}

extern "C" int gv_view_pool_fuse_bwd(const float* F, const float* dS, int32_t num_views, int32_t num_shapes,
                                     int64_t E, int64_t view_stride, int64_t shape_stride,
                                     const int32_t* scheme, int32_t num_groups, const float* weight,
                                     int32_t mode, float* dF, void* stream) {
    return gv_view_pool_fuse_bwd_t(F, dS, num_views, num_shapes, E, view_stride, shape_stride, scheme, num_groups, weight,
                                   mode, dF, 0, GV_F32, stream);
}

extern "C" int gv_view_pool_fuse_bwd_per_shape(const float* F, const float* dS, int32_t num_views,
                                               int32_t num_shapes, int64_t E, int64_t view_stride,
                                               int64_t shape_stride, const int32_t* scheme, int32_t num_groups,
                                               const float* weight, int32_t mode, float* dF, void* stream) {
    return gv_view_pool_fuse_bwd_t(F, dS, num_views, num_shapes, E, view_stride, shape_stride, scheme, num_groups, weight,
                                   mode, dF, 1, GV_F32, stream);
}

extern "C" int gv_view_score_per_shape(const float* r_img, int32_t nb, float* scores, void* stream) {
    if (!r_img || !scores || nb <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(view_score_per_shape_f32, dim3((nb + 255) / 256), dim3(256), 0, (hipStream_t)stream, r_img, nb,
                       scores);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_group_assign_per_shape(const float* scores, int32_t num_shapes, int32_t num_views,
                                         int32_t num_groups, int32_t num_bins, int32_t weight_mode, int32_t* gidx,
                                         int32_t* scheme, float* weight, int32_t* status, void* stream) {
    if (!scores || !gidx || !scheme || !weight || !status) return GV_E_BADARG;
    if (num_shapes <= 0 || num_views <= 0 || num_groups <= 0 || num_bins <= 0) return GV_E_BADARG;
    if (weight_mode != GV_WEIGHT_COUNT && weight_mode != GV_WEIGHT_MEAN_SCORE) return GV_E_BADARG;
    if (num_views > 64 || num_groups > 64) return GV_E_UNSUPPORTED;
    GV_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    return assign_launch(scores, num_shapes, num_views, num_groups, num_bins, weight_mode, gidx, scheme, weight, status, 1,
                         stream);
}

// eval.py:94-99: argmax, correct count, confusion matrix; one thread per shape
__global__ void eval_metrics_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, int n,
                                    int c, long long* __restrict__ prediction, int* __restrict__ confusion,
                                    int* __restrict__ correct) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* row = logits + (size_t)i * c;
    int best = 0;
    float bv = row[0];
    for (int k = 1; k < c; ++k)
        if (row[k] > bv) { bv = row[k]; best = k; }               // strict >: the first maximum wins
    prediction[i] = best;
    const long long l = labels[i];
    if (l >= 0 && l < c) {
        atomicAdd(&confusion[(size_t)l * c + best], 1);
        if (l == best) atomicAdd(correct, 1);
    }
}

extern "C" int gv_eval_metrics(const float* logits, const int64_t* labels, int32_t n, int32_t c,
                               int64_t* prediction, int32_t* confusion, int32_t* correct, void* stream) {
    if (!logits || !labels || !prediction || !confusion || !correct || n <= 0 || c <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(eval_metrics_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, logits,
                       (const long long*)labels, n, c, (long long*)prediction, confusion, correct);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_dense_fwd(const float* x, int32_t n, int32_t f, const float* kernel,
                            const float* bias, int32_t c, float* y, void* stream) {
    if (!x || !kernel || !bias || !y || n <= 0 || f <= 0 || c <= 0) return GV_E_BADARG;
    if (c > 65535) return GV_E_UNSUPPORTED;
    hipLaunchKernelGGL(dense_f32, dim3(n, c), dim3(256), 0, (hipStream_t)stream, x, f, kernel, bias, c, y);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
