// point_normals.hip — per-point normals of a batch of point clouds: exact k nearest neighbours within the cloud, the fp64
// covariance of the neighbourhood, its smallest eigenvector by cyclic Jacobi, a sign convention (the contract is in
// include/gvcnn_hip.h, "points in", normal estimation; tests/point_normals_oracle.py restates it in numpy).
//
//   gv_points_estimate_normals   build_grid         bounding boxes, statuses and the binned ids of the batch (point_grid.h,
//                                                   shared with point_clean.hip: five launches).
//                                query_kernel<K>    a thread per point, in cell order (neighbouring lanes walk the same
//                                                   cells): ring_walk over Chebyshev rings of cells around the point's own,
//                                                   the k_eff smallest keys (bits(d2) << 32 | id) kept sorted in an LDS
//                                                   column of the thread; then covariance, Jacobi and the sign in fp64
//                                                   registers.
//
// Nothing in the result depends on the grid: keys are unique, so the k_eff smallest are the same set in the same order
// whatever the order candidates arrive in, and a ring walk stops only when every point it has not seen is PROVABLY
// farther than the k-th key (ring_bound in point_grid.h; ties included).  No floating-point atomics anywhere.
#include "point_grid.h"

namespace {

constexpr int SWEEPS = 6;                                        // Jacobi sweeps (contract)

struct NArgs : GridArgs {
    int k, orient;
    double vp[3];
    float* normals;
    int* neighbours;
    float* variation;
};

// ---- covariance, Jacobi, sign ---------------------------------------------------------------------------------------
// one Jacobi rotation of the pair (p, q) of a symmetric 3x3; r the third index.  Contract formulas, in their order.
__device__ __forceinline__ void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                       double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
    x = v0p, y = v0q;
    v0p = c * x - s * y;
    v0q = s * x + c * y;
    x = v1p, y = v1q;
    v1p = c * x - s * y;
    v1q = s * x + c * y;
    x = v2p, y = v2q;
    v2p = c * x - s * y;
    v2q = s * x + c * y;
}

// the "none" rule: the component of largest magnitude becomes positive (the first of x, y, z on a tie)
__device__ __forceinline__ bool flip_none(const double n[3]) {
    const double ax = fabs(n[0]), ay = fabs(n[1]), az = fabs(n[2]);
    const double lead = (ax >= ay && ax >= az) ? n[0] : (ay >= az ? n[1] : n[2]);
    return lead < 0.0;
}

// normal and variation of point i from its sorted keys (column `keys`, stride NT); false: a degenerate neighbourhood
__device__ __forceinline__ bool normal_of(const NArgs& a, const CloudGrid& g, long long v0, const float* pi, const u64* keys, int keff,
                          float nf[3], float& var) {
    nf[0] = nf[1] = nf[2] = 0.0f;
    var = 0.0f;
    if (keff < 3) return false;
    const double p[3] = {(double)pi[0], (double)pi[1], (double)pi[2]};
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    for (int r = 0; r < keff; ++r) {
        const float* q = a.pts + (v0 + (long long)(unsigned)keys[r * NT]) * 3;
        m0 = m0 + ((double)q[0] - p[0]);
        m1 = m1 + ((double)q[1] - p[1]);
        m2 = m2 + ((double)q[2] - p[2]);
    }
    const double kd = (double)keff;
    m0 = m0 / kd, m1 = m1 / kd, m2 = m2 / kd;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int r = 0; r < keff; ++r) {
        const float* q = a.pts + (v0 + (long long)(unsigned)keys[r * NT]) * 3;
        const double e0 = ((double)q[0] - p[0]) - m0, e1 = ((double)q[1] - p[1]) - m1, e2 = ((double)q[2] - p[2]) - m2;
        a00 = a00 + e0 * e0;
        a01 = a01 + e0 * e1;
        a02 = a02 + e0 * e2;
        a11 = a11 + e1 * e1;
        a12 = a12 + e1 * e2;
        a22 = a22 + e2 * e2;
    }
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int s = 0; s < SWEEPS; ++s) {
        rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);           // (0, 1), third index 2
        rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);           // (0, 2), third index 1
        rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);           // (1, 2), third index 0
    }
    // l0 <= l1 <= l2, ties by column index: column c0 holds the smallest
    const int c0 = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);
    const double l0 = c0 == 0 ? a00 : c0 == 1 ? a11 : a22;
    const double ra = c0 == 0 ? a11 : a00, rb = c0 == 2 ? a11 : a22;             // the other two, in column order
    const double l1 = ra <= rb ? ra : rb, l2 = ra <= rb ? rb : ra;
    if (l2 == 0.0 || l1 <= 1e-12 * l2) return false;
    double n[3] = {c0 == 0 ? v00 : c0 == 1 ? v01 : v02, c0 == 0 ? v10 : c0 == 1 ? v11 : v12,
                   c0 == 0 ? v20 : c0 == 1 ? v21 : v22};
    bool flip;
    if (a.orient == GV_NORMALS_ORIENT_NONE) {
        flip = flip_none(n);
    } else {
        double w[3];
        for (int c = 0; c < 3; ++c)
            w[c] = a.orient == GV_NORMALS_ORIENT_OUTWARD ? p[c] - 0.5 * ((double)g.mn[c] + (double)g.mx[c]) : a.vp[c] - p[c];
        const double d = (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2];
        flip = d == 0.0 ? flip_none(n) : d < 0.0;
    }
    for (int c = 0; c < 3; ++c) nf[c] = (float)(flip ? -n[c] : n[c]);
    var = (float)(l0 / ((l0 + l1) + l2));
    return true;
}

// ---- query ----------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(NT) void query_kernel(NArgs a) {
    __shared__ u64 s_keys[K * NT];                               // rank-major: a thread's column is s_keys[r * NT + tid]
    const int m = blockIdx.y, tid = threadIdx.x;
    const CloudGrid g = a.grid[m];
    if (g.status != GV_RENDER_OK && g.status != GV_RENDER_NONFINITE) return;     // no points, or none that can be trusted
    const long long v0 = a.poff[m] - a.poff[0];
    const int P = (int)(a.poff[m + 1] - a.poff[m]);
    const int keff = min(a.k, P);
    u64* keys = s_keys + tid;
    bool degenerate = false;
    for (int s = blockIdx.x * NT + tid; s < P; s += gridDim.x * NT) {
        float nf[3] = {0.0f, 0.0f, 0.0f}, var = 0.0f;
        int i = s;
        bool ok = false;
        if (g.status == GV_RENDER_OK) {                          // (uniform)
            i = a.ids[v0 + s];
            const float* pp = a.pts + (v0 + i) * 3;
            const float pi[3] = {pp[0], pp[1], pp[2]};
            for (int r = 0; r < keff; ++r) keys[r * NT] = NO_KEY;
            u64 worst = NO_KEY;
            ring_walk(
                a, g, v0, pi,
                [&](int j, float d2) { insert_key(keys, keff, ((u64)__float_as_uint(d2) << 32) | (unsigned)j, worst); },
                [&]() { return worst; });
            ok = normal_of(a, g, v0, pi, keys, keff, nf, var);
            degenerate |= !ok;
        }
        const long long o = v0 + i;
        a.normals[o * 3] = nf[0];
        a.normals[o * 3 + 1] = nf[1];
        a.normals[o * 3 + 2] = nf[2];
        if (a.variation) a.variation[o] = var;
        if (a.neighbours)
            for (int r = 0; r < a.k; ++r)
                a.neighbours[o * a.k + r] = (g.status == GV_RENDER_OK && r < keff) ? (int)(unsigned)keys[r * NT] : -1;
    }
    if (degenerate) atomicOr(&a.status[m], GV_POINTS_DEGENERATE_NORMAL);
}

}  // namespace

extern "C" int64_t gv_points_normals_workspace_bytes(int32_t n, int64_t total_points, int32_t grid_cells) {
    if (n <= 0 || total_points < 0 || grid_cells < 0 || grid_cells > MAX_G) return GV_E_BADARG;
    if (n > 65535) return GV_E_UNSUPPORTED;
    return grid_ws_layout(n, total_points, grid_cells).bytes;
}

extern "C" int gv_points_estimate_normals(const float* points, const int64_t* point_offsets, int32_t n,
                                          int64_t total_points, int32_t max_points, int32_t k, int32_t orient,
                                          const float* viewpoint, int32_t grid_cells, float* normals, int32_t* neighbours,
                                          float* variation, void* workspace, int64_t workspace_bytes, int32_t* status,
                                          void* stream) {
    if (!points || !point_offsets || !normals || !workspace || !status) return GV_E_BADARG;
    if (n <= 0 || total_points < 0 || max_points < 0 || k < 3 || k > 32 || grid_cells < 0 || grid_cells > MAX_G)
        return GV_E_BADARG;
    if (orient != GV_NORMALS_ORIENT_NONE && orient != GV_NORMALS_ORIENT_OUTWARD && orient != GV_NORMALS_ORIENT_VIEWPOINT)
        return GV_E_BADARG;
    if (orient == GV_NORMALS_ORIENT_VIEWPOINT &&
        !(viewpoint && isfinite(viewpoint[0]) && isfinite(viewpoint[1]) && isfinite(viewpoint[2])))
        return GV_E_BADARG;
    if (n > 65535 || max_points > MAX_CLOUD) return GV_E_UNSUPPORTED;
    const GridWs L = grid_ws_layout(n, total_points, grid_cells);
    if (workspace_bytes < L.bytes) return GV_E_BADARG;
    if (!gv_aligned16(workspace) || ((uintptr_t)point_offsets & 7u) ||
        (((uintptr_t)points | (uintptr_t)normals | (uintptr_t)neighbours | (uintptr_t)variation | (uintptr_t)status) & 3u))
        return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    NArgs a;
    grid_args(a, points, point_offsets, n, total_points, grid_cells, workspace, L, status);
    a.k = k;
    a.orient = orient;
    for (int c = 0; c < 3; ++c) a.vp[c] = orient == GV_NORMALS_ORIENT_VIEWPOINT ? (double)viewpoint[c] : 0.0;
    a.normals = normals;
    a.neighbours = neighbours;
    a.variation = variation;
    const int rc = build_grid(a, max_points, st);
    if (rc != GV_OK) return rc;
    const dim3 by_point(grid_x(max_points), (unsigned)n);
    if (k <= 8) hipLaunchKernelGGL(query_kernel<8>, by_point, dim3(NT), 0, st, a);
    else if (k <= 16) hipLaunchKernelGGL(query_kernel<16>, by_point, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(query_kernel<32>, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
