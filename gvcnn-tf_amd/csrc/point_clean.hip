// point_clean.hip — cleaning a batch of raw point clouds on the device: statistical outlier selection, voxel selection
// and the one compaction both feed (the contract is in include/gvcnn_hip.h, "points in", cleaning;
// tests/points_clean_oracle.py restates it in numpy).  The search grid, the exact k-nearest collector and the call
// prologue are point_grid.h's; the tree sum and the block scan are point_math.h's.
//
//   gv_points_outlier_select   build_grid          bounding boxes, statuses, binned ids (point_grid.h).
//                              mean_kernel<K>      a thread per point, in cell order: nearest_keys over j != i, then the
//                                                  fp64 mean of their distances in rank order.
//                              tree_kernel x 6     tree_level<1> with the leaves m (-> mu), then (m - mu)^2 (-> sigma, T).
//                              keep_kernel         a thread per point: m_i <= T; the cloud's stats.
//   gv_points_voxel_select     bbox + cell_base    (the same bounding-box pass; the grid itself is not needed)
//                              voxel_setup_kernel  a thread per cloud: voxel size, passthrough clauses, fixed-point scale.
//                              voxel_insert_kernel a thread per point: its voxel key into the cloud's open-addressing
//                                                  table (atomicCAS), integer sums / count / lowest id of the voxel
//                                                  (integer atomics: WHICH slot a voxel has is arbitrary, what it holds
//                                                  is not).
//                              voxel_best_kernel   a thread per point: smallest key (bits(d2 to the centroid) << 32 | id).
//                              voxel_final_kernel  a thread per point: keep / centroid / index at the lowest member id.
//   gv_points_compact          scan_kernel         one workgroup per cloud: exclusive scan of keep in id order, counts.
//                              offsets_kernel      one workgroup: the new point_offsets (both: block_exclusive_scan).
//                              gather_kernel       a thread per point: points (or centroids), normals[index], index.
//
// No floating-point atomics anywhere; nothing in a result depends on the grid, the batch or the schedule.
#include "point_grid.h"

namespace {

constexpr u64 GOLD = 0x9E3779B97F4A7C15ull;
constexpr float TOO_FINE = 2097152.0f;                           // 2^21 cells on an axis

struct VoxelCloud {                                              // per cloud, written by voxel_setup_kernel
    double s;                                                    // fixed-point scale 2^(29 - E)
    float h;                                                     // voxel size
    int pass;                                                    // 1: the cloud goes through unchanged
    int shift;                                                   // 64 - log2(capacity of the cloud's table)
    unsigned mask;                                               // capacity - 1
};

struct CleanWs {
    GridWs grid;
    int64_t extra;                                               // where the operation's own arrays start
    // outlier selection
    int64_t mean, part1, part2, cstat;
    // voxel selection
    int64_t vcloud, voxel, slot, keys, best, minid, cnt, sums;
    int64_t slots, bytes;
};

CleanWs clean_layout(int32_t n, int64_t total_points, int32_t hint) {
    CleanWs L;
    L.grid = grid_ws_layout(n, total_points, hint);
    L.extra = L.grid.bytes;
    L.mean = L.extra;
    L.part1 = L.mean + round16(total_points * 8);
    L.cstat = tree_layout(L.part1, n, total_points, 1, L.part2);
    const int64_t outlier_end = L.cstat + round16((int64_t)n * 4 * 8);
    L.slots = 4 * total_points;                                  // a cloud of P points: slots [4 v0, 4 v0 + capacity)
    L.vcloud = L.extra;
    L.voxel = L.vcloud + round16((int64_t)n * (int64_t)sizeof(VoxelCloud));
    L.slot = L.voxel + round16((int64_t)n * 4);
    L.keys = L.slot + round16(total_points * 4);
    L.best = L.keys + L.slots * 8;
    L.minid = L.best + L.slots * 8;
    L.cnt = L.minid + L.slots * 4;
    L.sums = L.cnt + L.slots * 4;
    const int64_t voxel_end = L.sums + 3 * L.slots * 8;
    L.bytes = outlier_end > voxel_end ? outlier_end : voxel_end;
    return L;
}

// ---- statistical outlier selection ----------------------------------------------------------------------------------
struct OArgs : GridArgs {
    int k;
    double ratio;                                                // (double)std_ratio
    double* mean;                                                // [total_points], by id
    double* part1;                                               // the tree's partials (tree_layout, one channel)
    double* part2;
    double* cstat;                                               // [n, 4]: -, mu, sigma, T
    int* keep;
    float* mean_dist;
    double* stats;
};

template <int K>
__global__ __launch_bounds__(NT) void mean_kernel(OArgs a) {
    __shared__ u64 s_keys[K * NT];                               // rank-major: a thread's column is s_keys[r * NT + tid]
    const int m = blockIdx.y, tid = threadIdx.x;
    const CloudGrid g = a.grid[m];
    if (g.status != GV_RENDER_OK) return;
    const auto [v0, P] = cloud_span(a.poff, m);
    const int keff = min(a.k, P - 1);
    u64* keys = s_keys + tid;
    for (int s = blockIdx.x * NT + tid; s < P; s += gridDim.x * NT) {
        const int i = a.ids[v0 + s];
        double mi = 0.0;
        if (keff > 0) {                                          // (uniform)
            const float* pp = a.pts + (v0 + i) * 3;
            const float pi[3] = {pp[0], pp[1], pp[2]};
            nearest_keys<true>(a, g, v0, i, pi, keys, keff);
            for (int r = 0; r < keff; ++r)
                mi = mi + __builtin_sqrt((double)__uint_as_float((unsigned)(keys[r * NT] >> 32)));
            mi = mi / (double)keff;
        }
        a.mean[v0 + i] = mi;
        if (a.mean_dist) a.mean_dist[v0 + i] = (float)mi;
    }
}

// one level (point_math.h) of the tree sums of cloud m: mode 0 T(m) -> mu = T / P, mode 1 T((m - mu)^2) -> sigma, threshold
__global__ __launch_bounds__(TB) void tree_kernel(OArgs a, int mode, int level) {
    __shared__ double s[TB];
    const int m = blockIdx.y;
    if (a.grid[m].status != GV_RENDER_OK) return;
    const CloudSpan sp = cloud_span(a.poff, m);
    if (sp.P < 2) return;
    const double* mean = a.mean + sp.v0;
    double* out = a.cstat + m * 4;                               // -, mu, sigma, T
    const double mu = out[1];
    tree_level<1>(
        level, m, sp.v0, sp.P, a.part1, 0, a.part2, s,                  // (one channel: no plane stride)
        [&](int i, double x[1]) {
            const double e = mean[i] - mu;                       // (mode 0: mu is still 0)
            x[0] = mode == 0 ? mean[i] : e * e;
        },
        [&](int, double total) {
            if (mode == 0) {
                out[1] = total / (double)sp.P;
            } else {
                const double sigma = __builtin_sqrt(total / (double)(sp.P - 1));
                out[2] = sigma;
                out[3] = mu + a.ratio * sigma;
            }
        });
}

__global__ __launch_bounds__(NT) void keep_kernel(OArgs a) {
    const int m = blockIdx.y;
    const CloudGrid& g = a.grid[m];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (g.status != GV_RENDER_OK && g.status != GV_RENDER_NONFINITE) {
        if (first && a.stats) a.stats[m * 3] = a.stats[m * 3 + 1] = a.stats[m * 3 + 2] = 0.0;
        return;
    }
    const auto [v0, P] = cloud_span(a.poff, m);
    const bool select = g.status == GV_RENDER_OK && P >= 2;
    const double T = a.cstat[m * 4 + 3];
    if (first) {
        if (g.status == GV_RENDER_NONFINITE) a.status[m] = GV_RENDER_NONFINITE | GV_POINTS_CLEAN_PASSTHROUGH;
        if (a.stats)
            for (int c = 0; c < 3; ++c) a.stats[m * 3 + c] = select ? a.cstat[m * 4 + 1 + c] : 0.0;
    }
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        a.keep[v0 + i] = select ? (a.mean[v0 + i] <= T ? 1 : 0) : 1;
        if (a.mean_dist && g.status == GV_RENDER_NONFINITE) a.mean_dist[v0 + i] = 0.0f;
    }
}

// ---- voxel selection ------------------------------------------------------------------------------------------------
struct VArgs : GridArgs {
    VoxelCloud* vcloud;
    const float* voxel;                                          // [n], the caller's sizes (device copy)
    int relative;
    int* slot;                                                   // [total_points]: a point's slot in its cloud's table
    u64* keys;                                                   // tables: cloud m owns slots [4 v0, 4 v0 + capacity)
    u64* best;
    int* minid;
    int* cnt;
    u64* sums;                                                   // [3][slots], int64 sums through unsigned adds
    long long slots;
    int* keep;
    float* centroids;
    int* index;
};

__global__ __launch_bounds__(NT) void voxel_setup_kernel(VArgs a) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= a.n) return;
    const CloudGrid g = a.grid[m];
    VoxelCloud vc = {};
    if (g.status == GV_RENDER_NONFINITE) vc.pass = 1;
    if (g.status == GV_RENDER_OK) {
        const int P = cloud_span(a.poff, m).P;
        float ext[3], big = 0.0f;
        for (int c = 0; c < 3; ++c) {
            ext[c] = g.mx[c] - g.mn[c];
            big = fmaxf(big, ext[c]);
        }
        const float h = a.relative ? a.voxel[m] * big : a.voxel[m];
        bool bad = !(h > 0.0f && h < INFINITY);
        if (!bad)
            for (int c = 0; c < 3; ++c) bad |= !(ext[c] / h < TOO_FINE);
        vc.h = h;
        vc.pass = bad;
        int E = 0;
        if (big > 0.0f) (void)frexpf(big, &E);
        vc.s = big > 0.0f ? ldexp(1.0, 29 - E) : 1.0;
        int L = 2;
        while ((1ll << L) < 2ll * P + 1) ++L;                    // capacity 2^L >= 2 P + 1, at most 4 P
        vc.shift = 64 - L;
        vc.mask = (1u << L) - 1u;
    }
    a.vcloud[m] = vc;
    if (vc.pass) a.status[m] = g.status | GV_POINTS_CLEAN_PASSTHROUGH;
}

// the centroid of the voxel in slot `at` of cloud g, and its member count
__device__ __forceinline__ void centroid_of(const VArgs& a, const CloudGrid& g, const VoxelCloud& vc, long long at, float cf[3]) {
    const double nv = (double)a.cnt[at];
    for (int c = 0; c < 3; ++c) {
        const double S = (double)(long long)a.sums[c * a.slots + at];
        cf[c] = (float)((double)g.mn[c] + (S / nv) / vc.s);
    }
}

__global__ __launch_bounds__(NT) void voxel_insert_kernel(VArgs a) {
    const int m = blockIdx.y;
    const CloudGrid g = a.grid[m];
    const VoxelCloud vc = a.vcloud[m];
    if (g.status != GV_RENDER_OK || vc.pass) return;
    const auto [v0, P] = cloud_span(a.poff, m);
    const long long base = 4 * v0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        const float* p = a.pts + (v0 + i) * 3;
        float t[3];
        u64 key = 0;
        for (int c = 2; c >= 0; --c) {
            t[c] = p[c] - g.mn[c];
            key = (key << 21) | (u64)(unsigned)(int)(t[c] / vc.h);
        }
        unsigned s = (unsigned)((key * GOLD) >> vc.shift) & vc.mask;
        int found = -1;
        for (unsigned probe = 0; probe <= vc.mask; ++probe) {    // bounded by the capacity: it never spins
            const u64 old = atomicCAS(&a.keys[base + s], NO_KEY, key);
            if (old == NO_KEY || old == key) {
                found = (int)s;
                break;
            }
            s = (s + 1u) & vc.mask;
        }
        a.slot[v0 + i] = found;
        if (found < 0) {                                         // (a table fuller than its capacity: not reachable)
            atomicOr(&a.status[m], GV_POINTS_CLEAN_TABLE_FULL);
            continue;
        }
        const long long at = base + found;
        for (int c = 0; c < 3; ++c) atomicAdd(&a.sums[c * a.slots + at], (u64)__builtin_llrint((double)t[c] * vc.s));
        atomicAdd(&a.cnt[at], 1);
        atomicMin(&a.minid[at], i);
    }
}

__global__ __launch_bounds__(NT) void voxel_best_kernel(VArgs a) {
    const int m = blockIdx.y;
    const CloudGrid g = a.grid[m];
    const VoxelCloud vc = a.vcloud[m];
    if (g.status != GV_RENDER_OK || vc.pass) return;
    const auto [v0, P] = cloud_span(a.poff, m);
    const long long base = 4 * v0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        const int s = a.slot[v0 + i];
        if (s < 0) continue;
        float cf[3];
        centroid_of(a, g, vc, base + s, cf);
        const float* p = a.pts + (v0 + i) * 3;
        const float dx = p[0] - cf[0], dy = p[1] - cf[1], dz = p[2] - cf[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        atomicMin(&a.best[base + s], ((u64)__float_as_uint(d2) << 32) | (unsigned)i);
    }
}

__global__ __launch_bounds__(NT) void voxel_final_kernel(VArgs a) {
    const int m = blockIdx.y;
    const CloudGrid g = a.grid[m];
    const VoxelCloud vc = a.vcloud[m];
    if (g.status != GV_RENDER_OK && g.status != GV_RENDER_NONFINITE) return;
    const auto [v0, P] = cloud_span(a.poff, m);
    const long long base = 4 * v0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        const long long o = v0 + i;
        const float* p = a.pts + o * 3;
        float cf[3] = {0.0f, 0.0f, 0.0f};
        int keep = 0, index = -1;
        if (vc.pass) {
            keep = 1, index = i;
            cf[0] = p[0], cf[1] = p[1], cf[2] = p[2];
        } else {
            const int s = a.slot[o];
            if (s >= 0 && a.minid[base + s] == i) {
                keep = 1, index = (int)(unsigned)a.best[base + s];
                centroid_of(a, g, vc, base + s, cf);
            }
        }
        a.keep[o] = keep;
        a.index[o] = index;
        a.centroids[o * 3] = cf[0];
        a.centroids[o * 3 + 1] = cf[1];
        a.centroids[o * 3 + 2] = cf[2];
    }
}

// ---- compaction -----------------------------------------------------------------------------------------------------
struct CArgs {
    const float* pts;
    const long long* poff;
    const int* keep;
    const float* selected;                                       // the points to write (centroids), or NULL: pts
    const int* index;                                            // the member whose normal a kept point takes, or NULL: itself
    const float* normals;
    const int* status;
    int* rank;                                                   // [total_points]: kept points of the cloud before this one
    float* out_points;
    float* out_normals;
    int* out_index;
    long long* out_offsets;
    int* counts;
    long long total_points;
    int n;
};

// the cloud's range, or false when it has no output (its status says so, or its offsets cannot be trusted)
__device__ __forceinline__ bool cloud_range(const CArgs& a, int m, long long& v0, int& P) {
    v0 = a.poff[m] - a.poff[0];
    const long long v1 = a.poff[m + 1] - a.poff[0];
    P = 0;
    if (no_points(a.status[m]) || v0 < 0 || v1 <= v0 || v1 > a.total_points || v1 - v0 > MAX_CLOUD) return false;
    P = (int)(v1 - v0);
    return true;
}

__global__ __launch_bounds__(NT) void scan_kernel(CArgs a) {
    __shared__ int s[NT];
    const int m = blockIdx.x, tid = threadIdx.x;
    long long v0;
    int P, carry = 0;
    cloud_range(a, m, v0, P);                                    // (P = 0 without output)
    for (int b = 0; b < P; b += NT) {
        const int i = b + tid, k = i < P && a.keep[v0 + i] != 0;
        int total;
        const int before = block_exclusive_scan<int, NT>(s, k, total);
        if (i < P) a.rank[v0 + i] = carry + before;
        carry += total;
    }
    if (tid == 0) a.counts[m] = carry;
}

__global__ __launch_bounds__(SCAN_T) void offsets_kernel(CArgs a) {
    __shared__ long long s[SCAN_T];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int b = 0; b < a.n; b += SCAN_T) {
        const int i = b + tid;
        const long long v = i < a.n ? a.counts[i] : 0;
        long long total;
        const long long before = block_exclusive_scan<long long, SCAN_T>(s, v, total);
        if (i < a.n) a.out_offsets[i] = carry + before;
        carry += total;
    }
    if (tid == 0) a.out_offsets[a.n] = carry;
}

__global__ __launch_bounds__(NT) void gather_kernel(CArgs a) {
    const int m = blockIdx.y;
    long long v0;
    int P;
    if (!cloud_range(a, m, v0, P)) return;
    const long long o0 = a.out_offsets[m];
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        if (a.keep[v0 + i] == 0) continue;
        const long long d = o0 + a.rank[v0 + i];
        if (d >= a.total_points) continue;                       // (clouds that overlap: never past the output buffers)
        const float* p = (a.selected ? a.selected : a.pts) + (v0 + i) * 3;
        int src = a.index ? a.index[v0 + i] : i;
        if (src < 0 || src >= P) src = i;
        a.out_points[d * 3] = p[0];
        a.out_points[d * 3 + 1] = p[1];
        a.out_points[d * 3 + 2] = p[2];
        a.out_index[d] = src;
        if (a.out_normals) {
            const float* g = a.normals + (v0 + src) * 3;
            a.out_normals[d * 3] = g[0];
            a.out_normals[d * 3 + 1] = g[1];
            a.out_normals[d * 3 + 2] = g[2];
        }
    }
}

}  // namespace

extern "C" int64_t gv_points_clean_workspace_bytes(int32_t n, int64_t total_points, int32_t grid_cells) {
    const int rc = check_sizes(n, total_points, 0, grid_cells);
    return rc != GV_OK ? rc : clean_layout(n, total_points, grid_cells).bytes;
}

extern "C" int gv_points_outlier_select(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                                        int32_t max_points, int32_t k, float std_ratio, int32_t grid_cells, int32_t* keep,
                                        float* mean_dist, double* stats, void* workspace, int64_t workspace_bytes,
                                        int32_t* status, void* stream) {
    if (!keep || !status) return GV_E_BADARG;
    if (k < 1 || k > 32 || !(std_ratio >= 0.0f && std_ratio < INFINITY)) return GV_E_BADARG;
    const CleanWs L = clean_layout(n, total_points, grid_cells);
    const int rc = check_common(points, point_offsets, n, total_points, max_points, grid_cells, workspace, workspace_bytes, L.bytes);
    if (rc != GV_OK) return rc;
    if ((((uintptr_t)keep | (uintptr_t)mean_dist | (uintptr_t)status) & 3u) || ((uintptr_t)stats & 7u)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    OArgs a;
    grid_args(a, points, point_offsets, n, total_points, grid_cells, workspace, L.grid, status);
    a.k = k;
    a.ratio = (double)std_ratio;
    a.mean = reinterpret_cast<double*>(ws + L.mean);
    a.part1 = reinterpret_cast<double*>(ws + L.part1);
    a.part2 = reinterpret_cast<double*>(ws + L.part2);
    a.cstat = reinterpret_cast<double*>(ws + L.cstat);
    a.keep = keep;
    a.mean_dist = mean_dist;
    a.stats = stats;
    const int g = build_grid(a, max_points, st);
    if (g != GV_OK) return g;
    GV_HIP_CHECK(hipMemsetAsync(a.cstat, 0, (size_t)n * 4 * 8, st));
    const dim3 by_point(grid_x(max_points), (unsigned)n);
    GV_LAUNCH_BY_K(mean_kernel, k, by_point, st, a);
    GV_LAUNCH_CHECK();
    for (int mode = 0; mode < 2; ++mode) {
        launch_tree<tree_kernel>(n, max_points, st, a, mode);
        GV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(keep_kernel, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_points_voxel_select(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                                      int32_t max_points, const float* voxel, int32_t relative, int32_t grid_cells,
                                      int32_t* keep, float* centroids, int32_t* index, void* workspace,
                                      int64_t workspace_bytes, int32_t* status, void* stream) {
    if (!voxel || !keep || !centroids || !index || !status) return GV_E_BADARG;
    if (relative != 0 && relative != 1) return GV_E_BADARG;
    const CleanWs L = clean_layout(n, total_points, grid_cells);
    const int rc = check_common(points, point_offsets, n, total_points, max_points, grid_cells, workspace, workspace_bytes, L.bytes);
    if (rc != GV_OK) return rc;
    if (((uintptr_t)keep | (uintptr_t)centroids | (uintptr_t)index | (uintptr_t)status) & 3u) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    VArgs a;
    grid_args(a, points, point_offsets, n, total_points, grid_cells, workspace, L.grid, status);
    a.vcloud = reinterpret_cast<VoxelCloud*>(ws + L.vcloud);
    a.voxel = reinterpret_cast<const float*>(ws + L.voxel);
    a.relative = relative;
    a.slot = reinterpret_cast<int*>(ws + L.slot);
    a.keys = reinterpret_cast<u64*>(ws + L.keys);
    a.best = reinterpret_cast<u64*>(ws + L.best);
    a.minid = reinterpret_cast<int*>(ws + L.minid);
    a.cnt = reinterpret_cast<int*>(ws + L.cnt);
    a.sums = reinterpret_cast<u64*>(ws + L.sums);
    a.slots = L.slots;
    a.keep = keep;
    a.centroids = centroids;
    a.index = index;
    GV_HIP_CHECK(hipMemcpyAsync(ws + L.voxel, voxel, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (L.slots) {                                               // (a batch of empty clouds has no table)
        GV_HIP_CHECK(hipMemsetAsync(a.keys, 0xFF, (size_t)L.slots * 16, st));             // keys and best: NO_KEY
        GV_HIP_CHECK(hipMemsetAsync(a.minid, 0x7F, (size_t)L.slots * 4, st));             // above every id
        GV_HIP_CHECK(hipMemsetAsync(a.cnt, 0, (size_t)L.slots * 28, st));                 // counts and sums
    }
    hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)n), dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(cell_base_kernel, dim3(1), dim3(SCAN_T), 0, st, a);                // (overlapping offsets refused)
    GV_LAUNCH_CHECK();
    const dim3 by_point(grid_x(max_points), (unsigned)n);
    hipLaunchKernelGGL(voxel_setup_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(voxel_insert_kernel, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(voxel_best_kernel, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(voxel_final_kernel, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_points_compact(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                                 int32_t max_points, const int32_t* keep, const float* selected, const int32_t* index,
                                 const float* normals, const int32_t* status, float* out_points, float* out_normals,
                                 int32_t* out_index, int64_t* out_offsets, int32_t* counts, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    if (!keep || !status || !out_points || !out_index || !out_offsets || !counts) return GV_E_BADARG;
    if ((normals != nullptr) != (out_normals != nullptr)) return GV_E_BADARG;
    // (one int32 per point: less than the size query answers for any grid_cells)
    const int rc = check_common(points, point_offsets, n, total_points, max_points, 0, workspace, workspace_bytes,
                                round16(total_points * 4));
    if (rc != GV_OK) return rc;
    if ((((uintptr_t)keep | (uintptr_t)selected | (uintptr_t)index | (uintptr_t)normals | (uintptr_t)status |
          (uintptr_t)out_points | (uintptr_t)out_normals | (uintptr_t)out_index | (uintptr_t)counts) & 3u) ||
        ((uintptr_t)out_offsets & 7u))
        return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    CArgs a;
    a.pts = points;
    a.poff = (const long long*)point_offsets;
    a.keep = keep;
    a.selected = selected;
    a.index = index;
    a.normals = normals;
    a.status = status;
    a.rank = static_cast<int*>(workspace);
    a.out_points = out_points;
    a.out_normals = out_normals;
    a.out_index = out_index;
    a.out_offsets = (long long*)out_offsets;
    a.counts = counts;
    a.total_points = total_points;
    a.n = n;
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n), dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(SCAN_T), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(gather_kernel, dim3(grid_x(max_points), (unsigned)n), dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
