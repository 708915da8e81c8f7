// The group table of one shape and the pooled descriptor of one group: the two things the head's kernels must agree on
// to the bit (grouping.hip: view_pool_fuse and its backward; scorer_bwd.hip: the weight gradient, which recomputes S;
// explain.hip: the backward's coefficients).
// Everything sits in the including file's unnamed namespace: each translation unit has its own copy.
#pragma once
#include "gv_common.h"
#include "lp_elem.h"

namespace {

// Scheme rows as 64-bit masks of views [64], the group weights [64], and W = their fp32 sum in ascending g
// (tf.reduce_sum(group_weight_list)), in LDS.  V, G <= 64 (the entry points check).  Three objects, each addressed from
// its own base (one struct base costs an address subtraction per group in the kernels' element loops).
struct GroupTable {
    unsigned long long* mask;
    float* w;
    float* W;
};
#define GROUP_TABLE_SHARED(t)                                                                                            \
    __shared__ unsigned long long t##_mask[64];                                                                          \
    __shared__ float t##_w[64];                                                                                          \
    __shared__ float t##_W;                                                                                              \
    const GroupTable t = {t##_mask, t##_w, &t##_W}

// Fill `t` (LDS) from one shape's scheme [G][V] and weight [G]; every thread of the workgroup calls it, and the table is
// complete when it returns.  empty_zero: the weight of a group without views counts as 0 (the mean_score form, where
// such a group has no score to average).  THREADS: the workgroup's size where the kernel fixes it (0: blockDim.x).
template <int THREADS = 0>
__device__ __forceinline__ void group_table_load(const GroupTable& t, const int* __restrict__ scheme,
                                                 const float* __restrict__ weight, int G, int V, bool empty_zero) {
    for (int g = threadIdx.x; g < G; g += THREADS ? THREADS : (int)blockDim.x) {
        unsigned long long m = 0;
        for (int v = 0; v < V; ++v)
            if (scheme[g * V + v] != 0) m |= 1ull << v;
        t.mask[g] = m;
        t.w[g] = (empty_zero && m == 0) ? 0.f : weight[g];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ws = 0.f;
        for (int g = 0; g < G; ++g) ws = ws + t.w[g];
        *t.W = ws;
    }
    __syncthreads();
}

// D_g of one element vector (A: a Px accessor of lp_elem.h; base: the vector in view 0): the group's first view, the
// others folded in in ascending v (maximum or sum), one division by the count for the mean.  m != 0.
template <class A>
__device__ __forceinline__ void pooled_group(const typename A::elem* base, int64_t view_stride, unsigned long long m,
                                             int mode, float (&d)[A::N]) {
    const int cnt = __popcll(m);
    int v = __ffsll((long long)m) - 1;
    m &= m - 1;
    A::load(base + (size_t)v * view_stride, 0, 0, 0, d);
    while (m) {
        v = __ffsll((long long)m) - 1;
        m &= m - 1;
        float x[A::N];
        A::load(base + (size_t)v * view_stride, 0, 0, 0, x);
#pragma unroll
        for (int k = 0; k < A::N; ++k) d[k] = mode == GV_VIEWPOOL_MAX ? fmaxf(d[k], x[k]) : d[k] + x[k];
    }
    if (mode == GV_VIEWPOOL_MEAN) {
        const float c = (float)cnt;
#pragma unroll
        for (int k = 0; k < A::N; ++k) d[k] = d[k] / c;
    }
}

}  // namespace
