// point_register.hip — rigid point-to-point ICP for a batch of (source cloud, target cloud) pairs, entirely on the stream
// (the contract is in include/gvcnn_hip.h, "points in", registration; tests/points_register_oracle.py restates it in
// numpy).  The grid, the exact nearest walk and the call prologue are point_grid.h's; the tree sum (zeros for rejected
// pairs), several channels to a workgroup, and the Jacobi rotation are point_math.h's, shared with the cleaning and the normals.
//
//   gv_points_register   build_grid x 2        the target's grid (it does not move: built once) and the source's (its
//                                              status, and the cell order the nearest kernel visits the points in).
//                        begin_kernel          a thread per pair: status byte, initial transform, the pair's state.
//     per round          nearest_kernel        a thread per source point: moved by the pair's (R, t) in fp64, rounded
//                                              once; ring_walk_from around the clamped cell in the TARGET's grid; the one
//                                              smallest key (bits(d2) << 32 | id) in a register.
//                        sum_kernel<8> x 3     count, sum p, sum y, sum d2 over the inliers (tree_level<8>, three levels).
//                        decide_kernel         a thread per pair: non-finite / few pairs / rmse / converged; centroids.
//                        sum_kernel<9> x 3     H = sum (p - cp)(y - cy)^T about those centroids.
//                        solve_kernel          a thread per pair: Horn's 4x4 matrix, cyclic Jacobi, quaternion -> (R, t).
//                        finish_kernel         a thread per pair: transforms, rmse, inliers, used, status.
//                        apply_kernel          a thread per source point: moved points, rotated normals, correspondence.
//
// The host enqueues every round; a pair that has stopped is a device flag its threads return on.  No floating-point
// atomics anywhere; nothing in a result depends on the grid, the batch or the schedule.
#include "point_grid.h"

namespace {

constexpr int SWEEPS = 8;                                        // Jacobi sweeps of the 4x4 (contract)
constexpr int C1 = 8, C2 = 9, CMAX = 9;                          // channels of the two passes

struct PairState {                                               // per pair
    double T[12];                                                // (R | t), row-major 3x4
    double cen[6];                                               // cp, cy of the round
    double rmse, prev;
    int inliers, used, flags, done;                              // flags: GV_POINTS_ICP_*; done: no further round
    int byte, pad;                                               // the pair's GV_RENDER_* byte
};

struct RegWs {
    GridWs tgrid, sgrid;
    int64_t t0, s0;                                              // where the two grids start
    int64_t state, init, sstatus, tstatus, match, d2, part1, part2, tot, bytes;
};

RegWs reg_layout(int32_t n, int64_t total_source, int64_t total_target, int32_t hint) {
    RegWs L;
    L.tgrid = grid_ws_layout(n, total_target, hint);
    L.sgrid = grid_ws_layout(n, total_source, hint);
    L.t0 = 0;
    L.s0 = L.tgrid.bytes;
    L.state = L.s0 + L.sgrid.bytes;
    L.init = L.state + round16((int64_t)n * (int64_t)sizeof(PairState));
    L.sstatus = L.init + (int64_t)n * 16 * 8;
    L.tstatus = L.sstatus + round16((int64_t)n * 4);
    L.match = L.tstatus + round16((int64_t)n * 4);
    L.d2 = L.match + round16(total_source * 4);
    L.part1 = L.d2 + round16(total_source * 4);
    L.tot = tree_layout(L.part1, n, total_source, CMAX, L.part2);
    L.bytes = L.tot + round16((int64_t)n * CMAX * 8);
    return L;
}

struct RArgs {
    GridArgs s, t;                                               // source and target: points, offsets, grids
    PairState* state;
    const double* init;                                          // [n, 16] in the workspace, or NULL
    const float* normals;
    int* match;                                                  // [total_source], by source id
    float* d2;
    double* part1;                                               // [C][plane]
    double* part2;                                               // [n][C][TB]
    double* tot;                                                 // [n][CMAX]
    long long plane;
    float max_d2;
    double tol;
    int cell_order;
    double* transforms;
    double* rmse;
    int* inliers;
    int* used;
    int* corr;
    float* moved;
    float* moved_normals;
    int* status;
};

int g_cell_order = 1;                                            // gv_points_register_set_cell_order: speed alone

__device__ __forceinline__ void move_point(const double* T, const float* p, float q[3]) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    for (int c = 0; c < 3; ++c) q[c] = (float)(((T[c * 4] * x + T[c * 4 + 1] * y) + T[c * 4 + 2] * z) + T[c * 4 + 3]);
}

__global__ __launch_bounds__(NT) void begin_kernel(RArgs a) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= a.s.n) return;
    const int sb = a.s.grid[m].status, tb = a.t.grid[m].status;
    PairState ps = {};
    for (int c = 0; c < 3; ++c)
        for (int d = 0; d < 4; ++d) ps.T[c * 4 + d] = a.init ? a.init[m * 16 + c * 4 + d] : (c == d ? 1.0 : 0.0);
    ps.byte = sb != GV_RENDER_OK ? sb : tb;
    ps.done = ps.byte != GV_RENDER_OK;
    a.state[m] = ps;
}

// ---- nearest --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void nearest_kernel(RArgs a) {
    const int m = blockIdx.y;
    PairState& ps = a.state[m];
    if (ps.done) return;                                         // (uniform)
    const CloudGrid g = a.t.grid[m];
    double T[12];
    for (int c = 0; c < 12; ++c) T[c] = ps.T[c];
    const auto [vs, P] = cloud_span(a.s.poff, m);
    const long long vt = cloud_span(a.t.poff, m).v0;
    bool bad = false;
    for (int s = blockIdx.x * NT + threadIdx.x; s < P; s += gridDim.x * NT) {
        // the cell order of the source at its ORIGINAL positions: a rigid motion keeps neighbours neighbours
        const int i = a.cell_order ? a.s.ids[vs + s] : s;
        float q[3];
        move_point(T, a.s.pts + (vs + i) * 3, q);
        if (!(fabsf(q[0]) < INFINITY && fabsf(q[1]) < INFINITY && fabsf(q[2]) < INFINITY)) {
            bad = true;
            a.match[vs + i] = -1;                                // (the sums of this round still run: a NaN d2 is no
            a.d2[vs + i] = NAN;                                  // inlier, so no leaf reads the match)
            continue;
        }
        int c[3];
        cell3_clamped(g, q, c);
        u64 best = NO_KEY;
        ring_walk_from(
            a.t, g, vt, q, c,
            [&](int j, float d2) {
                const u64 key = ((u64)__float_as_uint(d2) << 32) | (unsigned)j;
                best = key < best ? key : best;
            },
            [&]() { return best; });
        a.match[vs + i] = (int)(unsigned)best;
        a.d2[vs + i] = __uint_as_float((unsigned)(best >> 32));
    }
    if (bad) atomicOr(&ps.flags, GV_POINTS_ICP_NONFINITE);
}

// ---- sums -----------------------------------------------------------------------------------------------------------
// the leaf values of source id i of pair m, written over the zeros x arrives with (tree_level): left alone unless i is an inlier
template <int C>
__device__ __forceinline__ void leaf(const RArgs& a, const PairState& ps, long long vs, long long vt, int i, double x[C]) {
    const float d2 = a.d2[vs + i];
    if (!(d2 <= a.max_d2)) return;
    const float* p = a.s.pts + (vs + i) * 3;
    const float* y = a.t.pts + (vt + a.match[vs + i]) * 3;
    if (C == C1) {
        x[0] = 1.0;
        for (int c = 0; c < 3; ++c) {
            x[1 + c] = (double)p[c];
            x[4 + c] = (double)y[c];
        }
        x[7] = (double)d2;
    } else {
        double ep[3], ey[3];
        for (int c = 0; c < 3; ++c) {
            ep[c] = (double)p[c] - ps.cen[c];
            ey[c] = (double)y[c] - ps.cen[3 + c];
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) x[r * 3 + c] = ep[r] * ey[c];
    }
}

// one level (point_math.h) of the tree sums of pair m over its source points, C channels at once
template <int C>
__global__ __launch_bounds__(TB) void sum_kernel(RArgs a, int level) {
    __shared__ double sh[C * TB];
    const int m = blockIdx.y;
    const PairState& ps = a.state[m];
    if (ps.done) return;                                         // (uniform)
    const CloudSpan sp = cloud_span(a.s.poff, m);
    const long long vt = cloud_span(a.t.poff, m).v0;
    tree_level<C>(
        level, m, sp.v0, sp.P, a.part1, a.plane, a.part2, sh, [&](int i, double x[C]) { leaf<C>(a, ps, sp.v0, vt, i, x); },
        [&](int c, double total) { a.tot[m * CMAX + c] = total; });
}

// ---- the round's decision -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void decide_kernel(RArgs a, int round) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= a.s.n) return;
    PairState& ps = a.state[m];
    if (ps.done) return;
    ps.used = round;
    if (ps.flags & GV_POINTS_ICP_NONFINITE) {
        ps.inliers = 0;
        ps.rmse = 0.0;
        ps.done = 1;
        return;
    }
    const double* tot = a.tot + m * CMAX;
    const double cnt = tot[0];
    ps.inliers = (int)cnt;
    if (cnt < 3.0) {
        ps.flags |= GV_POINTS_ICP_FEW_PAIRS;
        ps.rmse = cnt > 0.0 ? __builtin_sqrt(tot[7] / cnt) : 0.0;
        ps.done = 1;
        return;
    }
    const double rmse = __builtin_sqrt(tot[7] / cnt);
    ps.rmse = rmse;
    if (round > 1 && fabs(ps.prev - rmse) <= a.tol) {
        ps.flags |= GV_POINTS_ICP_CONVERGED;
        ps.done = 1;
        return;
    }
    ps.prev = rmse;
    for (int c = 0; c < 6; ++c) ps.cen[c] = tot[1 + c] / cnt;
}

// ---- Horn's closed form ---------------------------------------------------------------------------------------------
// one Jacobi rotation (point_math.h) of the pair (P, Q) of the symmetric 4x4 A (both triangles kept) and of V
template <int P, int Q>
__device__ __forceinline__ void rotate4(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    double c, s, h;
    jacobi_csh(A[P][P], A[Q][Q], apq, c, s, h);
    A[P][P] = A[P][P] - h;
    A[Q][Q] = A[Q][Q] + h;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        rotate_pair(c, s, A[r][P], A[r][Q]);
        A[P][r] = A[r][P];
        A[Q][r] = A[r][Q];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) rotate_pair(c, s, V[i][P], V[i][Q]);
}

__global__ __launch_bounds__(NT) void solve_kernel(RArgs a) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= a.s.n) return;
    PairState& ps = a.state[m];
    if (ps.done) return;
    const double* H = a.tot + m * CMAX;
    const double h00 = H[0], h01 = H[1], h02 = H[2], h10 = H[3], h11 = H[4], h12 = H[5], h20 = H[6], h21 = H[7], h22 = H[8];
    double A[4][4], V[4][4];
    A[0][0] = (h00 + h11) + h22;
    A[1][1] = (h00 - h11) - h22;
    A[2][2] = (h11 - h00) - h22;
    A[3][3] = (h22 - h00) - h11;
    A[0][1] = A[1][0] = h12 - h21;
    A[0][2] = A[2][0] = h20 - h02;
    A[0][3] = A[3][0] = h01 - h10;
    A[1][2] = A[2][1] = h01 + h10;
    A[1][3] = A[3][1] = h20 + h02;
    A[2][3] = A[3][2] = h12 + h21;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        rotate4<0, 1>(A, V);
        rotate4<0, 2>(A, V);
        rotate4<0, 3>(A, V);
        rotate4<1, 2>(A, V);
        rotate4<1, 3>(A, V);
        rotate4<2, 3>(A, V);
    }
    // the column of the largest eigenvalue, the lower column on a tie
    double best = A[0][0], e[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (A[c][c] > best) {
            best = A[c][c];
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = V[i][c];
        }
    const double lead = e[0] != 0.0 ? e[0] : e[1] != 0.0 ? e[1] : e[2] != 0.0 ? e[2] : e[3];
    if (lead < 0.0)
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = -e[i];
    const double nn = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3];
    const double len = __builtin_sqrt(nn);
    const double w = e[0] / len, x = e[1] / len, y = e[2] / len, z = e[3] / len;
    double R[9];
    R[0] = ((w * w + x * x) - y * y) - z * z;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = ((w * w - x * x) + y * y) - z * z;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = ((w * w - x * x) - y * y) + z * z;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ps.T[c * 4] = R[c * 3];
        ps.T[c * 4 + 1] = R[c * 3 + 1];
        ps.T[c * 4 + 2] = R[c * 3 + 2];
        ps.T[c * 4 + 3] = ps.cen[3 + c] - ((R[c * 3] * ps.cen[0] + R[c * 3 + 1] * ps.cen[1]) + R[c * 3 + 2] * ps.cen[2]);
    }
}

// ---- outputs --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void finish_kernel(RArgs a) {
    const int m = blockIdx.x * NT + threadIdx.x;
    if (m >= a.s.n) return;
    const PairState& ps = a.state[m];
    for (int c = 0; c < 12; ++c) a.transforms[m * 16 + c] = ps.T[c];
    for (int c = 12; c < 16; ++c) a.transforms[m * 16 + c] = c == 15 ? 1.0 : 0.0;
    if (a.rmse) a.rmse[m] = ps.rmse;
    if (a.inliers) a.inliers[m] = ps.inliers;
    if (a.used) a.used[m] = ps.used;
    a.status[m] = ps.byte | ps.flags;
}

__global__ __launch_bounds__(NT) void apply_kernel(RArgs a) {
    const int m = blockIdx.y;
    if (no_points(a.s.grid[m].status)) return;                   // (its offsets cannot be trusted, or it has no points)
    const PairState& ps = a.state[m];
    double T[12];
    for (int c = 0; c < 12; ++c) T[c] = ps.T[c];
    const bool matched = ps.used > 0 && !(ps.flags & GV_POINTS_ICP_NONFINITE);
    const auto [vs, P] = cloud_span(a.s.poff, m);
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        const long long o = vs + i;
        float q[3];
        move_point(T, a.s.pts + o * 3, q);
        a.moved[o * 3] = q[0];
        a.moved[o * 3 + 1] = q[1];
        a.moved[o * 3 + 2] = q[2];
        if (a.moved_normals) {
            const float* g = a.normals + o * 3;
            const double x = (double)g[0], y = (double)g[1], z = (double)g[2];
            for (int c = 0; c < 3; ++c) a.moved_normals[o * 3 + c] = (float)((T[c * 4] * x + T[c * 4 + 1] * y) + T[c * 4 + 2] * z);
        }
        if (a.corr) a.corr[o] = matched && a.d2[o] <= a.max_d2 ? a.match[o] : -1;
    }
}

}  // namespace

// tuning hook (not part of the drop-in surface): 1 = the nearest kernel visits the source points in the cell order of
// the source's grid, 0 = in id order.  The results are the same.
extern "C" void gv_points_register_set_cell_order(int on) { g_cell_order = on != 0; }

extern "C" int64_t gv_points_register_workspace_bytes(int32_t n, int64_t total_source, int64_t total_target, int32_t grid_cells) {
    const int rc = check_sizes(n, total_source, 0, grid_cells, total_target, 0);
    return rc != GV_OK ? rc : reg_layout(n, total_source, total_target, grid_cells).bytes;
}

extern "C" int gv_points_register(const float* source, const int64_t* source_offsets, const float* target,
                                  const int64_t* target_offsets, int32_t n, int64_t total_source, int64_t total_target,
                                  int32_t max_source, int32_t max_target, const float* source_normals, const double* init,
                                  int32_t iterations, float max_distance, double tolerance, int32_t grid_cells,
                                  double* transforms, double* rmse, int32_t* inliers, int32_t* used, int32_t* correspondence,
                                  float* moved, float* moved_normals, void* workspace, int64_t workspace_bytes,
                                  int32_t* status, void* stream) {
    if (!target || !target_offsets || !transforms || !moved || !status) return GV_E_BADARG;
    if ((source_normals != nullptr) != (moved_normals != nullptr)) return GV_E_BADARG;
    if (iterations < 1 || !(max_distance >= 0.0f) || !(tolerance >= 0.0)) return GV_E_BADARG;
    const RegWs L = reg_layout(n, total_source, total_target, grid_cells);
    const int rc0 = check_common(source, source_offsets, n, total_source, max_source, grid_cells, workspace, workspace_bytes, L.bytes,
                                 target, target_offsets, total_target, max_target);
    if (rc0 != GV_OK) return rc0;
    if ((((uintptr_t)init | (uintptr_t)transforms | (uintptr_t)rmse) & 7u) ||
        (((uintptr_t)source_normals | (uintptr_t)inliers | (uintptr_t)used | (uintptr_t)correspondence | (uintptr_t)moved |
          (uintptr_t)moved_normals | (uintptr_t)status) & 3u))
        return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    RArgs a;
    grid_args(a.t, target, target_offsets, n, total_target, grid_cells, ws + L.t0, L.tgrid, reinterpret_cast<int*>(ws + L.tstatus));
    grid_args(a.s, source, source_offsets, n, total_source, grid_cells, ws + L.s0, L.sgrid, reinterpret_cast<int*>(ws + L.sstatus));
    a.state = reinterpret_cast<PairState*>(ws + L.state);
    a.init = init ? reinterpret_cast<const double*>(ws + L.init) : nullptr;
    a.normals = source_normals;
    a.match = reinterpret_cast<int*>(ws + L.match);
    a.d2 = reinterpret_cast<float*>(ws + L.d2);
    a.part1 = reinterpret_cast<double*>(ws + L.part1);
    a.part2 = reinterpret_cast<double*>(ws + L.part2);
    a.tot = reinterpret_cast<double*>(ws + L.tot);
    a.plane = tree_plane(n, total_source);
    a.max_d2 = max_distance * max_distance;
    a.tol = tolerance;
    a.cell_order = g_cell_order;
    a.transforms = transforms;
    a.rmse = rmse;
    a.inliers = inliers;
    a.used = used;
    a.corr = correspondence;
    a.moved = moved;
    a.moved_normals = moved_normals;
    a.status = status;
    if (init) GV_HIP_CHECK(hipMemcpyAsync(ws + L.init, init, (size_t)n * 16 * 8, hipMemcpyHostToDevice, st));
    int rc = build_grid(a.t, max_target, st);
    if (rc != GV_OK) return rc;
    rc = build_grid(a.s, max_source, st);
    if (rc != GV_OK) return rc;
    const dim3 by_pair((unsigned)((n + NT - 1) / NT)), by_point(grid_x(max_source), (unsigned)n);
    hipLaunchKernelGGL(begin_kernel, by_pair, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    for (int round = 1; round <= iterations; ++round) {
        hipLaunchKernelGGL(nearest_kernel, by_point, dim3(NT), 0, st, a);
        GV_LAUNCH_CHECK();
        launch_tree<sum_kernel<C1>>(n, max_source, st, a);
        GV_LAUNCH_CHECK();
        hipLaunchKernelGGL(decide_kernel, by_pair, dim3(NT), 0, st, a, round);
        GV_LAUNCH_CHECK();
        launch_tree<sum_kernel<C2>>(n, max_source, st, a);
        GV_LAUNCH_CHECK();
        hipLaunchKernelGGL(solve_kernel, by_pair, dim3(NT), 0, st, a);
        GV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(finish_kernel, by_pair, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(apply_kernel, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
