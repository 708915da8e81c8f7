// point_grid.h — the uniform search grid over a batch of point clouds and the exact k-nearest walk through it, shared by
// point_normals.hip (normal estimation), point_clean.hip (outlier selection, voxel selection, compaction) and
// point_register.hip (the nearest target point of a moved source point).  What they share that is not the grid (the block
// scan, the tree sum, the Jacobi rotation) is point_math.h's.
//
//   build_grid   bbox_kernel        one workgroup per cloud: offsets check, bounding box, cells per axis G.
//                cell_base_kernel   one workgroup: exclusive scan of the clouds' G^3 -> where each cloud's cells start in
//                                   the workspace.
//                bin_kernel<false>  a thread per point: its cell's counter + 1 (integer atomics).
//                alloc_kernel       a thread per cell: takes count slots of its cloud's id range from the cloud's cursor
//                                   (an integer atomic: WHERE a cell's ids lie is arbitrary).
//                bin_kernel<true>   a thread per point: its id into its cell's range.
//   ring_walk    Chebyshev rings of cells around a point's own; every candidate goes to visit(j, d2); the walk stops
//                only when every point it has not seen is PROVABLY farther than the caller's k-th key (ring_bound; ties
//                included), so the k smallest keys never depend on the grid.  ring_walk_from: the same walk around a
//                cell the caller names (cell3_clamped: a query that may lie outside the cloud's box).
//   insert_key   the k smallest keys (bits(d2) << 32 | id) kept sorted in an LDS column of the thread.
//   nearest_keys the k_eff smallest keys of a point of the cloud, itself included or not (GV_LAUNCH_BY_K: the kernel<K>).
//   check_common, check_sizes   the argument clauses the entry points and the size queries share, in the ABI's order.
#pragma once
#include "point_math.h"

namespace {

typedef unsigned long long u64;

constexpr int SCAN_T = 1024;
constexpr int MAX_CLOUD = 1 << 24;                               // points of a cloud: ids fit the splatter's 24 bits
constexpr int MAX_G = 128;                                       // cells per axis
constexpr u64 NO_KEY = ~0ull;

struct CloudGrid {                                               // per cloud, written by bbox_kernel (64 bytes)
    float mn[3], mx[3];                                          // bounding box
    float inv[3];                                                // cells per unit length, 0 on an axis without extent
    int G;                                                       // cells per axis
    int status;                                                  // GV_RENDER_*
    int cursor;                                                  // next free slot of the cloud's id range (alloc_kernel)
    long long cell_base;                                         // first cell in cell_count / cell_end
};

// largest g with g^3 <= x, at most MAX_G
__host__ __device__ inline int icbrt(long long x) {
    int g = 0;
    while (g < MAX_G && (long long)(g + 1) * (g + 1) * (g + 1) <= x) ++g;
    return g;
}

// Cells per axis of a cloud of P points.  Auto: about two points per cell by volume, G^3 <= max(P / 2, 1).  A hint h:
// min(h, the largest G with G^3 <= max(4 P, 1)), which keeps the cells of a batch within 4 * total_points + n whatever h.
__host__ __device__ inline int cells_per_axis(long long P, int hint) {
    const int g = icbrt(hint <= 0 ? P / 2 : 4 * P), g1 = g < 1 ? 1 : g;
    return hint <= 0 || g1 < hint ? g1 : hint;
}

// the cells a batch can need: the workspace holds two int32 per cell
inline int64_t cell_capacity(int32_t n, int64_t total_points, int32_t hint) {
    if (hint <= 0 || hint > MAX_G) return total_points / 2 + n;  // (a hint out of range is refused: the layout stays defined)
    const int64_t by_hint = (int64_t)n * hint * hint * hint, by_points = 4 * total_points + n;
    return by_hint < by_points ? by_hint : by_points;
}

struct GridWs {
    int64_t grids, ids, cell_count, cell_end, cells, bytes;      // byte offsets; cells: capacity in cells
};

inline GridWs grid_ws_layout(int32_t n, int64_t total_points, int32_t hint) {
    GridWs L;
    L.cells = cell_capacity(n, total_points, hint);
    L.grids = 0;
    L.ids = round16((int64_t)n * (int64_t)sizeof(CloudGrid));
    L.cell_count = L.ids + round16(total_points * 4);
    L.cell_end = L.cell_count + round16(L.cells * 4);
    L.bytes = L.cell_end + round16(L.cells * 4);
    return L;
}

struct GridArgs {
    const float* pts;
    const long long* poff;
    CloudGrid* grid;
    int* ids;                                                    // [total_points]: a cloud's ids, cell by cell
    int* cell_count;
    int* cell_end;                                               // after bin_kernel<true>: one past the cell's last slot
    int* status;
    long long total_points, cells;
    int n, hint;
};

inline void grid_args(GridArgs& a, const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                      int32_t hint, void* workspace, const GridWs& L, int32_t* status) {
    char* ws = static_cast<char*>(workspace);
    a.pts = points;
    a.poff = (const long long*)point_offsets;
    a.grid = reinterpret_cast<CloudGrid*>(ws + L.grids);
    a.ids = reinterpret_cast<int*>(ws + L.ids);
    a.cell_count = reinterpret_cast<int*>(ws + L.cell_count);
    a.cell_end = reinterpret_cast<int*>(ws + L.cell_end);
    a.status = status;
    a.total_points = total_points;
    a.cells = L.cells;
    a.n = n;
    a.hint = hint;
}

// the clauses of the sizes (all a size query has), in the ABI's order; total_b, max_b: the target batch of a registration
inline int check_sizes(int32_t n, int64_t total, int32_t max_points, int32_t grid_cells, int64_t total_b = 0, int32_t max_b = 0) {
    if (n <= 0 || total < 0 || max_points < 0 || grid_cells < 0 || grid_cells > MAX_G || total_b < 0 || max_b < 0)
        return GV_E_BADARG;
    return n > 65535 || max_points > MAX_CLOUD || max_b > MAX_CLOUD ? GV_E_UNSUPPORTED : GV_OK;
}

// The argument clauses every call shares, in the ABI's order: null pointers and sizes (GV_E_BADARG), limits
// (GV_E_UNSUPPORTED), the workspace's size (GV_E_BADARG; need: what the call's layout asks for), alignment (GV_E_ALIGN).
// A call checks its own values before (registration: that its target is there) and the alignment of its own pointers after.
inline int check_common(const void* points, const void* offsets, int32_t n, int64_t total, int32_t max_points,
                        int32_t grid_cells, const void* workspace, int64_t workspace_bytes, int64_t need,
                        const void* points_b = nullptr, const void* offsets_b = nullptr, int64_t total_b = 0, int32_t max_b = 0) {
    if (!points || !offsets || !workspace) return GV_E_BADARG;
    const int rc = check_sizes(n, total, max_points, grid_cells, total_b, max_b);
    if (rc != GV_OK) return rc;
    if (workspace_bytes < need) return GV_E_BADARG;
    const uintptr_t by8 = (uintptr_t)offsets | (uintptr_t)offsets_b, by4 = (uintptr_t)points | (uintptr_t)points_b;
    return !gv_aligned16(workspace) || (by8 & 7u) || (by4 & 3u) ? GV_E_ALIGN : GV_OK;
}

struct CloudSpan { long long v0; int P; };                       // a cloud's first point in the packed arrays, its points

__device__ __forceinline__ CloudSpan cloud_span(const long long* poff, int m) {
    return {poff[m] - poff[0], (int)(poff[m + 1] - poff[m])};
}

__device__ __forceinline__ bool no_points(int st) {              // the statuses whose cloud has no output
    st &= 0xFF;
    return st == GV_RENDER_EMPTY || st == GV_RENDER_TOO_LARGE || st == GV_RENDER_BAD_OFFSETS;
}

// the cell of coordinate x on an axis: monotone in x (each step is), the same wherever it is computed
__device__ __forceinline__ int cell_of(float x, float mn, float inv, int G) {
    return min((int)((x - mn) * inv), G - 1);
}

__device__ __forceinline__ void cell3(const CloudGrid& g, const float* p, int c[3]) {
    for (int a = 0; a < 3; ++a) c[a] = cell_of(p[a], g.mn[a], g.inv[a], g.G);
}

// cell_of for a coordinate that may lie outside the cloud's box (a query from another cloud): the nearest cell of the
// axis.  The clamp is in float, before the conversion, so neither a negative nor a huge (x - mn) * inv reaches the cast
// (fmaxf turns the NaN of inf * 0 into 0).  Inside the box it is cell_of: min((int)t, G - 1) == (int)min(t, G - 1), t >= 0.
__device__ __forceinline__ int cell_of_clamped(float x, float mn, float inv, int G) {
    return (int)fminf(fmaxf((x - mn) * inv, 0.0f), (float)(G - 1));
}

__device__ __forceinline__ void cell3_clamped(const CloudGrid& g, const float* p, int c[3]) {
    for (int a = 0; a < 3; ++a) c[a] = cell_of_clamped(p[a], g.mn[a], g.inv[a], g.G);
}

// ---- bounding box, grid size ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void bbox_kernel(GridArgs a) {
    __shared__ float s_red[6][NT];
    const int m = blockIdx.x, tid = threadIdx.x;
    const long long v0 = a.poff[m] - a.poff[0], v1 = a.poff[m + 1] - a.poff[0];
    int st = GV_RENDER_OK;
    if (v0 < 0 || v1 < v0 || v1 > a.total_points) st = GV_RENDER_BAD_OFFSETS;
    else if (v1 - v0 > MAX_CLOUD) st = GV_RENDER_TOO_LARGE;
    else if (v1 == v0) st = GV_RENDER_EMPTY;
    CloudGrid g = {};
    if (st == GV_RENDER_OK) {                                    // (uniform)
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (long long i = v0 + tid; i < v1; i += NT)
            for (int c = 0; c < 3; ++c) {
                const float p = a.pts[i * 3 + c];
                mn[c] = fminf(mn[c], p);
                mx[c] = p != p ? INFINITY : fmaxf(mx[c], p);     // (fmaxf would drop a NaN: it must not pass unseen)
            }
        for (int c = 0; c < 3; ++c) {
            s_red[c][tid] = mn[c];
            s_red[3 + c][tid] = mx[c];
        }
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (tid < s)
                for (int c = 0; c < 3; ++c) {
                    s_red[c][tid] = fminf(s_red[c][tid], s_red[c][tid + s]);
                    s_red[3 + c][tid] = fmaxf(s_red[3 + c][tid], s_red[3 + c][tid + s]);
                }
            __syncthreads();
        }
        g.G = cells_per_axis(v1 - v0, a.hint);
        for (int c = 0; c < 3; ++c) {
            g.mn[c] = s_red[c][0];
            g.mx[c] = s_red[3 + c][0];
            const float ext = g.mx[c] - g.mn[c];
            if (!(ext >= 0.0f && ext < INFINITY)) st = GV_RENDER_NONFINITE;      // a NaN / inf point, or a box past fp32
            const float inv = ext > 0.0f ? (float)g.G / ext : 0.0f;
            g.inv[c] = inv < INFINITY ? inv : 0.0f;              // (an extent in the denormals: one cell on this axis)
        }
    }
    if (st != GV_RENDER_OK) g.G = 0;
    g.status = st;
    if (tid == 0) {
        a.grid[m] = g;
        a.status[m] = st;
    }
}

// exclusive scan of the clouds' cell counts (one workgroup).  A cloud whose cells would pass the workspace's capacity
// (offsets that overlap: the clouds then hold more than total_points points) is refused as GV_RENDER_BAD_OFFSETS.
__global__ __launch_bounds__(SCAN_T) void cell_base_kernel(GridArgs a) {
    __shared__ long long s[SCAN_T];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int b = 0; b < a.n; b += SCAN_T) {
        const int i = b + tid;
        long long v = 0;
        if (i < a.n) {
            const long long G = a.grid[i].G;
            v = G * G * G;
        }
        long long total;
        const long long before = block_exclusive_scan<long long, SCAN_T>(s, v, total);
        if (i < a.n) {
            const long long base = carry + before;
            a.grid[i].cell_base = base;
            if (base + v > a.cells) {
                a.grid[i].G = 0;
                a.grid[i].status = GV_RENDER_BAD_OFFSETS;
                a.status[i] = GV_RENDER_BAD_OFFSETS;
            }
        }
        carry += total;
    }
}

// ---- binning --------------------------------------------------------------------------------------------------------
template <bool SCATTER>
__global__ __launch_bounds__(NT) void bin_kernel(GridArgs a) {
    const int m = blockIdx.y;
    const CloudGrid g = a.grid[m];
    if (g.status != GV_RENDER_OK) return;
    const auto [v0, P] = cloud_span(a.poff, m);
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        int c[3];
        cell3(g, a.pts + (v0 + i) * 3, c);
        const long long cell = g.cell_base + ((long long)c[2] * g.G + c[1]) * g.G + c[0];
        if (SCATTER) a.ids[v0 + atomicAdd(&a.cell_end[cell], 1)] = i;
        else atomicAdd(&a.cell_count[cell], 1);
    }
}

// every non-empty cell takes its slots from the cloud's cursor: cell_end starts as the cell's first slot
__global__ __launch_bounds__(NT) void alloc_kernel(GridArgs a) {
    const int m = blockIdx.y;
    CloudGrid& g = a.grid[m];
    if (g.status != GV_RENDER_OK) return;
    const long long cells = (long long)g.G * g.G * g.G;
    for (long long c = (long long)blockIdx.x * NT + threadIdx.x; c < cells; c += (long long)gridDim.x * NT) {
        const int cnt = a.cell_count[g.cell_base + c];
        a.cell_end[g.cell_base + c] = cnt ? atomicAdd(&g.cursor, cnt) : 0;
    }
}

// bounding boxes, statuses and the binned ids of the batch.  max_points sizes the launches only: every kernel strides
// what its grid does not cover.
inline int build_grid(const GridArgs& a, int32_t max_points, hipStream_t st) {
    const long long G = cells_per_axis(max_points, a.hint);
    const dim3 by_point(grid_x(max_points), (unsigned)a.n), by_cell(grid_x(G * G * G), (unsigned)a.n);
    GV_HIP_CHECK(hipMemsetAsync(a.cell_count, 0, (size_t)a.cells * 4, st));
    hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)a.n), dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(cell_base_kernel, dim3(1), dim3(SCAN_T), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(bin_kernel<false>, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(alloc_kernel, by_cell, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(bin_kernel<true>, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

// ---- query ----------------------------------------------------------------------------------------------------------
// A lower bound of the squared distance from point p (cell c) to any point in a cell outside the block of Chebyshev
// radius r around c; +inf when the block holds the whole grid.  A point in a cell >= h on an axis has fl(fl(x - mn) *
// inv) >= h, so x - mn >= (h / inv) (1 - 2^-23) in real numbers; a point in a cell <= l has x - mn < ((l + 1) / inv)
// (1 + 2^-23).  The margin taken is 2^-18, in fp64 from the exact u = x_p - mn.
// Neither inequality speaks of p, so the bound holds for ANY cell c, p's own or not, and for a p outside the box with its
// clamped cell: beyond the upper face c = G - 1 and the first branch is skipped, while in the second u only grew past
// the box (a larger, still true, bound); beyond the lower face c = 0, the second is skipped and -u > 0 adds to the first.
__device__ __forceinline__ double ring_bound(const CloudGrid& g, const float* p, const int c[3], int r) {
    double D = INFINITY;
    for (int a = 0; a < 3; ++a) {
        if (g.inv[a] == 0.0f) continue;                          // one occupied cell on this axis: nothing beyond it
        const double u = (double)p[a] - (double)g.mn[a], cs = 1.0 / (double)g.inv[a];
        if (c[a] + r + 1 <= g.G - 1) D = fmin(D, fmax((double)(c[a] + r + 1) * cs * (1.0 - 0x1p-18) - u, 0.0));
        if (c[a] - r - 1 >= 0) D = fmin(D, fmax(u - (double)(c[a] - r) * cs * (1.0 + 0x1p-18), 0.0));
    }
    return D * D;
}

// `key` into the column of the keff smallest keys so far (keys[r * NT], ascending); worst: the column's last entry
__device__ __forceinline__ void insert_key(u64* keys, int keff, u64 key, u64& worst) {
    if (key >= worst) return;
    int t = keff - 1;                                            // sorted insert from the end
    while (t > 0) {
        const u64 prev = keys[(t - 1) * NT];
        if (prev < key) break;
        keys[t * NT] = prev;
        --t;
    }
    keys[t * NT] = key;
    worst = keys[(keff - 1) * NT];
}

// Every point j of the cloud that can be among the nearest of point pi, ring by ring: visit(j, d2) with the contract's
// fp32 d2 (pi itself included, d2 = 0).  kth() is the caller's k-th smallest key so far, NO_KEY while it has fewer.
// c: the cell the rings are centred on, any cell of the grid (ring_bound holds for each; the nearest is the fastest).
template <class Visit, class Kth>
__device__ __forceinline__ void ring_walk_from(const GridArgs& a, const CloudGrid& g, long long v0, const float pi[3],
                                               const int c[3], Visit visit, Kth kth) {
    const int G = g.G;
    auto cell_points = [&](long long cell) {
        const int end = a.cell_end[cell], beg = end - a.cell_count[cell];
        for (int q = beg; q < end; ++q) {
            const int j = a.ids[v0 + q];
            const float* pj = a.pts + (v0 + j) * 3;
            const float dx = pj[0] - pi[0], dy = pj[1] - pi[1], dz = pj[2] - pi[2];
            visit(j, (dx * dx + dy * dy) + dz * dz);
        }
    };
    for (int r = 0;; ++r) {                                      // the shell of Chebyshev radius r, clipped to the grid
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, G - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, G - 1);
        const int xl = c[0] - r, xh = c[0] + r;
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const long long row = g.cell_base + ((long long)z * G + y) * G;
                if (abs(z - c[2]) == r || abs(y - c[1]) == r) {  // a row of the shell's z or y faces: whole
                    for (int x = max(xl, 0); x <= min(xh, G - 1); ++x) cell_points(row + x);
                } else {                                         // any other (r >= 1): its two ends
                    if (xl >= 0) cell_points(row + xl);
                    if (xh <= G - 1) cell_points(row + xh);
                }
            }
        const double B = ring_bound(g, pi, c, r);
        if (B == INFINITY) break;                                // every cell has been seen
        // fp32 d2 of an unseen point >= B (1 - 2^-22) unless B is near the underflow of a square; the strict <
        // leaves a tie with the k-th key to the next ring
        const u64 worst = kth();
        if (worst != NO_KEY && B > 1e-30 && (double)__uint_as_float((unsigned)(worst >> 32)) < B * (1.0 - 0x1p-18)) break;
    }
}

// the walk of a point of the cloud itself, around its own cell
template <class Visit, class Kth>
__device__ __forceinline__ void ring_walk(const GridArgs& a, const CloudGrid& g, long long v0, const float pi[3], Visit visit,
                                          Kth kth) {
    int c[3];
    cell3(g, pi, c);
    ring_walk_from(a, g, v0, pi, c, visit, kth);
}

// the keff smallest keys of point pi (id i) of the cloud into the thread's column; SKIP_SELF: over j != i
template <bool SKIP_SELF>
__device__ __forceinline__ void nearest_keys(const GridArgs& a, const CloudGrid& g, long long v0, int i, const float pi[3],
                                             u64* keys, int keff) {
    for (int r = 0; r < keff; ++r) keys[r * NT] = NO_KEY;
    u64 worst = NO_KEY;
    ring_walk(
        a, g, v0, pi,
        [&](int j, float d2) {
            if (!SKIP_SELF || j != i) insert_key(keys, keff, ((u64)__float_as_uint(d2) << 32) | (unsigned)j, worst);
        },
        [&]() { return worst; });
}

// kernel<K>(args) for the smallest K in 8 / 16 / 32 that holds k keys (K sizes the LDS columns), a thread per point
#define GV_LAUNCH_BY_K(kernel, k, by_point, st, args) \
    hipLaunchKernelGGL(((k) <= 8 ? kernel<8> : (k) <= 16 ? kernel<16> : kernel<32>), by_point, dim3(NT), 0, st, args)

}  // namespace
