// point_math.h — the arithmetic the point-cloud files share that is not the grid (point_grid.h includes it): each piece is
// a clause of a bit-exact contract (include/gvcnn_hip.h, "points in"), so it is written once.  The block scan (cell_base_kernel,
// scan_kernel, offsets_kernel), the tree sum (tree_kernel of point_clean.hip, sum_kernel<C> of point_register.hip) and the
// Jacobi rotation (rotate of point_normals.hip, rotate4 of point_register.hip).
#pragma once
#include <math.h>

#include "gv_common.h"

// every step of the contracts' arithmetic rounds on its own, here and in the file that includes this one
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                                          // threads of every kernel but the scan
constexpr int TB = 256;                                          // leaves of one workgroup tree (= NT)
constexpr int MAX_GRID_X = 2048;                                 // workgroups along x; the loops stride the rest

inline int64_t round16(int64_t x) { return (x + 15) / 16 * 16; }

inline unsigned grid_x(long long items) {
    const long long b = (items + NT - 1) / NT;
    return (unsigned)(b < 1 ? 1 : b > MAX_GRID_X ? MAX_GRID_X : b);
}

// The exclusive prefix of v over the N threads of the workgroup (s: N values of LDS), and their sum in `total`.  Every
// thread calls it; s may be reused once it returns.
template <class T, int N>
__device__ __forceinline__ T block_exclusive_scan(T* s, T v, T& total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < N; o <<= 1) {
        const T add = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const T before = s[tid] - v;
    total = s[N - 1];
    __syncthreads();
    return before;
}

__host__ __device__ inline int blocks_of(int x) { return (x + TB - 1) / TB; }

// Cloud m (first point v0) keeps its level-0 partials of channel c from part1 + c * plane + (v0 >> 8) + m and its level-1
// partials from part2 + (m * C + c) * TB.  tree_layout: part2 (a byte offset, as part1) and, returned, the end of both.
inline int64_t tree_plane(int32_t n, int64_t total_points) { return total_points / TB + n + 2; }

inline int64_t tree_layout(int64_t part1, int32_t n, int64_t total_points, int C, int64_t& part2) {
    part2 = part1 + round16(tree_plane(n, total_points) * C * 8);
    return part2 + round16((int64_t)n * TB * C * 8);
}

// One level of the tree sums of cloud m (P points from v0), C channels at once: aligned blocks of TB values, adjacent
// pairs level by level (b_t = a_2t + a_2t+1, zeros past the end), one partial per block and channel.  Level 0 reads
// leaf(i, x) (x arrives zeroed), level 1 the partials of level 0, level 2 those of level 1 (at most TB: one block) and
// hands the totals to finish(c, total) in threads c < C.  sh: C * TB doubles of LDS.
template <int C, class Leaf, class Finish>
__device__ __forceinline__ void tree_level(int level, int m, long long v0, int P, double* part1, long long plane,
                                           double* part2, double* sh, Leaf leaf, Finish finish) {
    const int tid = threadIdx.x;
    const int c1 = blocks_of(P), c2 = blocks_of(c1);
    const int count = level == 0 ? P : level == 1 ? c1 : c2;
    double* p1 = part1 + (v0 >> 8) + m;                          // channel c: + c * plane
    double* p2 = part2 + (long long)m * C * TB;                  // channel c: + c * TB
    for (int b = blockIdx.x; b < blocks_of(count); b += gridDim.x) {
        const int idx = b * TB + tid;
        double x[C];
        for (int c = 0; c < C; ++c) x[c] = 0.0;
        if (idx < count) {
            if (level == 0) leaf(idx, x);
            else
                for (int c = 0; c < C; ++c) x[c] = level == 1 ? p1[c * plane + idx] : p2[c * TB + idx];
        }
        for (int c = 0; c < C; ++c) sh[c * TB + tid] = x[c];
        __syncthreads();
        for (int stride = 1; stride < TB; stride <<= 1) {
            if ((tid & (2 * stride - 1)) == 0)
                for (int c = 0; c < C; ++c) sh[c * TB + tid] = sh[c * TB + tid] + sh[c * TB + tid + stride];
            __syncthreads();
        }
        if (tid < C) {
            const double v = sh[tid * TB];
            if (level == 0) p1[tid * plane + b] = v;
            else if (level == 1) p2[tid * TB + b] = v;
            else finish(tid, v);
        }
        __syncthreads();
    }
}

// the three levels of KERNEL(args..., level) over n clouds of at most max_points points: level is the kernel's LAST parameter
template <auto KERNEL, class... Args>
inline void launch_tree(int32_t n, int32_t max_points, hipStream_t st, const Args&... args) {
    const long long b1 = ((long long)max_points + TB - 1) / TB, b2 = (b1 + TB - 1) / TB;
    const unsigned gx[3] = {grid_x(b1 * NT), grid_x(b2 * NT), 1u};
    for (int level = 0; level < 3; ++level)
        hipLaunchKernelGGL(KERNEL, dim3(gx[level], (unsigned)n), dim3(TB), 0, st, args..., level);
}

// The rotation that annihilates a_pq of a symmetric matrix (a_pq != 0): its cosine, sine and the shift h of the two
// diagonal entries (a_pp - h, a_qq + h).  Contract formulas, in their order.
__device__ __forceinline__ void jacobi_csh(double app, double aqq, double apq, double& c, double& s, double& h) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    c = 1.0 / __builtin_sqrt(t * t + 1.0);
    s = t * c;
    h = t * apq;
}

// the plane rotation of the pair (x, y): columns p and q of a row
__device__ __forceinline__ void rotate_pair(double c, double s, double& xp, double& yq) {
    const double x = xp, y = yq;
    xp = c * x - s * y;
    yq = s * x + c * y;
}

}  // namespace
