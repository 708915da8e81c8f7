// point_normals.hip — per-point normals of a batch of point clouds: exact k nearest neighbours within the cloud, the fp64
// covariance of the neighbourhood, its smallest eigenvector by cyclic Jacobi, a sign convention (the contract is in
// include/gvcnn_hip.h, "points in", normal estimation; tests/point_normals_oracle.py restates it in numpy).
//
//   gv_points_estimate_normals   build_grid         bounding boxes, statuses and the binned ids of the batch (point_grid.h,
//                                                   shared with point_clean.hip and point_register.hip: five launches).
//                                query_kernel<K>    a thread per point, in cell order (neighbouring lanes walk the same
//                                                   cells): nearest_keys (point_grid.h), the k_eff smallest keys (bits(d2)
//                                                   << 32 | id) sorted in an LDS column of the thread; then covariance,
//                                                   Jacobi (the rotation is point_math.h's) and the sign in fp64 registers.
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
// one Jacobi rotation (point_math.h) of the pair (p, q) of a symmetric 3x3; r the third index
__device__ __forceinline__ void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                       double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    double c, s, h;
    jacobi_csh(app, aqq, apq, c, s, h);
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    rotate_pair(c, s, arp, arq);
    rotate_pair(c, s, v0p, v0q);
    rotate_pair(c, s, v1p, v1q);
    rotate_pair(c, s, v2p, v2q);
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
    const auto [v0, P] = cloud_span(a.poff, m);
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
            nearest_keys<false>(a, g, v0, i, pi, keys, keff);
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
    const int rc = check_sizes(n, total_points, 0, grid_cells);
    return rc != GV_OK ? rc : grid_ws_layout(n, total_points, grid_cells).bytes;
}

extern "C" int gv_points_estimate_normals(const float* points, const int64_t* point_offsets, int32_t n,
                                          int64_t total_points, int32_t max_points, int32_t k, int32_t orient,
                                          const float* viewpoint, int32_t grid_cells, float* normals, int32_t* neighbours,
                                          float* variation, void* workspace, int64_t workspace_bytes, int32_t* status,
                                          void* stream) {
    if (!normals || !status || k < 3 || k > 32) return GV_E_BADARG;
    if (orient != GV_NORMALS_ORIENT_NONE && orient != GV_NORMALS_ORIENT_OUTWARD && orient != GV_NORMALS_ORIENT_VIEWPOINT)
        return GV_E_BADARG;
    if (orient == GV_NORMALS_ORIENT_VIEWPOINT &&
        !(viewpoint && isfinite(viewpoint[0]) && isfinite(viewpoint[1]) && isfinite(viewpoint[2])))
        return GV_E_BADARG;
    const GridWs L = grid_ws_layout(n, total_points, grid_cells);
    const int rc0 = check_common(points, point_offsets, n, total_points, max_points, grid_cells, workspace, workspace_bytes, L.bytes);
    if (rc0 != GV_OK) return rc0;
    if (((uintptr_t)normals | (uintptr_t)neighbours | (uintptr_t)variation | (uintptr_t)status) & 3u) return GV_E_ALIGN;
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
    GV_LAUNCH_BY_K(query_kernel, k, by_point, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
