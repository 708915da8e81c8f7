// point_normals.hip — per-point normals of a batch of point clouds: exact k nearest neighbours within the cloud, the fp64
// covariance of the neighbourhood, its smallest eigenvector by cyclic Jacobi, a sign convention (the contract is in
// include/gvcnn_hip.h, "points in", normal estimation; tests/point_normals_oracle.py restates it in numpy).
//
//   gv_points_estimate_normals   bbox_kernel        one workgroup per cloud: offsets check, bounding box, cells per axis G.
//                                cell_base_kernel   one workgroup: exclusive scan of the clouds' G^3 -> where each cloud's
//                                                   cells start in the workspace.
//                                bin_kernel<false>  a thread per point: its cell's counter + 1 (integer atomics).
//                                alloc_kernel       a thread per cell: takes count slots of its cloud's id range from the
//                                                   cloud's cursor (an integer atomic: WHERE a cell's ids lie is arbitrary).
//                                bin_kernel<true>   a thread per point: its id into its cell's range.
//                                query_kernel<K>    a thread per point, in cell order (neighbouring lanes walk the same
//                                                   cells): Chebyshev rings of cells around the point's own, the k_eff
//                                                   smallest keys (bits(d2) << 32 | id) kept sorted in an LDS column of the
//                                                   thread; then covariance, Jacobi and the sign in fp64 registers.
//
// Nothing in the result depends on the grid: keys are unique, so the k_eff smallest are the same set in the same order
// whatever the order candidates arrive in, and a ring walk stops only when every point it has not seen is PROVABLY
// farther than the k-th key (ring_bound below; ties included).  No floating-point atomics anywhere.
#include <math.h>

#include "gv_common.h"

// every step of the contract's arithmetic rounds on its own (fp32 distances, fp64 covariance and Jacobi)
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int NT = 256;                                          // threads of every kernel but the scan
constexpr int SCAN_T = 1024;
constexpr int MAX_CLOUD = 1 << 24;                               // points of a cloud: ids fit the splatter's 24 bits
constexpr int MAX_G = 128;                                       // cells per axis
constexpr int MAX_GRID_X = 2048;                                 // workgroups along x; the loops stride the rest
constexpr int SWEEPS = 6;                                        // Jacobi sweeps (contract)
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
    if (hint <= 0) return total_points / 2 + n;
    const int64_t by_hint = (int64_t)n * hint * hint * hint, by_points = 4 * total_points + n;
    return by_hint < by_points ? by_hint : by_points;
}

struct NormalsWs {
    int64_t grids, ids, cell_count, cell_end, cells, bytes;      // byte offsets; cells: capacity in cells
};

inline int64_t round16(int64_t x) { return (x + 15) / 16 * 16; }

NormalsWs ws_layout(int32_t n, int64_t total_points, int32_t hint) {
    NormalsWs L;
    L.cells = cell_capacity(n, total_points, hint);
    L.grids = 0;
    L.ids = round16((int64_t)n * (int64_t)sizeof(CloudGrid));
    L.cell_count = L.ids + round16(total_points * 4);
    L.cell_end = L.cell_count + round16(L.cells * 4);
    L.bytes = L.cell_end + round16(L.cells * 4);
    return L;
}

struct NArgs {
    const float* pts;
    const long long* poff;
    CloudGrid* grid;
    int* ids;                                                    // [total_points]: a cloud's ids, cell by cell
    int* cell_count;
    int* cell_end;                                               // after scatter_kernel: one past the cell's last slot
    int* status;
    long long total_points, cells;
    int n, k, orient, hint;
    double vp[3];
    float* normals;
    int* neighbours;
    float* variation;
};

// the cell of coordinate x on an axis: monotone in x (each step is), the same wherever it is computed
__device__ __forceinline__ int cell_of(float x, float mn, float inv, int G) {
    return min((int)((x - mn) * inv), G - 1);
}

__device__ __forceinline__ void cell3(const CloudGrid& g, const float* p, int c[3]) {
    for (int a = 0; a < 3; ++a) c[a] = cell_of(p[a], g.mn[a], g.inv[a], g.G);
}

// ---- bounding box, grid size ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void bbox_kernel(NArgs a) {
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
__global__ __launch_bounds__(SCAN_T) void cell_base_kernel(NArgs a) {
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
        s[tid] = v;
        __syncthreads();
        for (int o = 1; o < SCAN_T; o <<= 1) {
            const long long add = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (i < a.n) {
            const long long base = carry + s[tid] - v;
            a.grid[i].cell_base = base;
            if (base + v > a.cells) {
                a.grid[i].G = 0;
                a.grid[i].status = GV_RENDER_BAD_OFFSETS;
                a.status[i] = GV_RENDER_BAD_OFFSETS;
            }
        }
        carry += s[SCAN_T - 1];
        __syncthreads();
    }
}

// ---- binning --------------------------------------------------------------------------------------------------------
template <bool SCATTER>
__global__ __launch_bounds__(NT) void bin_kernel(NArgs a) {
    const int m = blockIdx.y;
    const CloudGrid g = a.grid[m];
    if (g.status != GV_RENDER_OK) return;
    const long long v0 = a.poff[m] - a.poff[0];
    const int P = (int)(a.poff[m + 1] - a.poff[m]);
    for (int i = blockIdx.x * NT + threadIdx.x; i < P; i += gridDim.x * NT) {
        int c[3];
        cell3(g, a.pts + (v0 + i) * 3, c);
        const long long cell = g.cell_base + ((long long)c[2] * g.G + c[1]) * g.G + c[0];
        if (SCATTER) a.ids[v0 + atomicAdd(&a.cell_end[cell], 1)] = i;
        else atomicAdd(&a.cell_count[cell], 1);
    }
}

// every non-empty cell takes its slots from the cloud's cursor: cell_end starts as the cell's first slot
__global__ __launch_bounds__(NT) void alloc_kernel(NArgs a) {
    const int m = blockIdx.y;
    CloudGrid& g = a.grid[m];
    if (g.status != GV_RENDER_OK) return;
    const long long cells = (long long)g.G * g.G * g.G;
    for (long long c = (long long)blockIdx.x * NT + threadIdx.x; c < cells; c += (long long)gridDim.x * NT) {
        const int cnt = a.cell_count[g.cell_base + c];
        a.cell_end[g.cell_base + c] = cnt ? atomicAdd(&g.cursor, cnt) : 0;
    }
}

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
// A lower bound of the squared distance from point p (cell c) to any point in a cell outside the block of Chebyshev
// radius r around c; +inf when the block holds the whole grid.  A point in a cell >= h on an axis has fl(fl(x - mn) *
// inv) >= h, so x - mn >= (h / inv) (1 - 2^-23) in real numbers; a point in a cell <= l has x - mn < ((l + 1) / inv)
// (1 + 2^-23).  The margin taken is 2^-18, in fp64 from the exact u = x_p - mn.
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

template <int K>
__global__ __launch_bounds__(NT) void query_kernel(NArgs a) {
    __shared__ u64 s_keys[K * NT];                               // rank-major: a thread's column is s_keys[r * NT + tid]
    const int m = blockIdx.y, tid = threadIdx.x;
    const CloudGrid g = a.grid[m];
    if (g.status != GV_RENDER_OK && g.status != GV_RENDER_NONFINITE) return;     // no points, or none that can be trusted
    const long long v0 = a.poff[m] - a.poff[0];
    const int P = (int)(a.poff[m + 1] - a.poff[m]);
    const int keff = min(a.k, P), G = g.G;
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
            int c[3];
            cell3(g, pi, c);
            for (int r = 0; r < keff; ++r) keys[r * NT] = NO_KEY;
            u64 worst = NO_KEY;
            auto visit = [&](long long cell) {                  // every point of a cell against the k_eff best so far
                const int end = a.cell_end[cell], beg = end - a.cell_count[cell];
                for (int q = beg; q < end; ++q) {
                    const int j = a.ids[v0 + q];
                    const float* pj = a.pts + (v0 + j) * 3;
                    const float dx = pj[0] - pi[0], dy = pj[1] - pi[1], dz = pj[2] - pi[2];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const u64 key = ((u64)__float_as_uint(d2) << 32) | (unsigned)j;
                    if (key >= worst) continue;
                    int t = keff - 1;                            // sorted insert from the end
                    while (t > 0) {
                        const u64 prev = keys[(t - 1) * NT];
                        if (prev < key) break;
                        keys[t * NT] = prev;
                        --t;
                    }
                    keys[t * NT] = key;
                    worst = keys[(keff - 1) * NT];
                }
            };
            for (int r = 0;; ++r) {                              // the shell of Chebyshev radius r, clipped to the grid
                const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, G - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, G - 1);
                const int xl = c[0] - r, xh = c[0] + r;
                for (int z = z0; z <= z1; ++z)
                    for (int y = y0; y <= y1; ++y) {
                        const long long row = g.cell_base + ((long long)z * G + y) * G;
                        if (abs(z - c[2]) == r || abs(y - c[1]) == r) {          // a row of the shell's z or y faces: whole
                            for (int x = max(xl, 0); x <= min(xh, G - 1); ++x) visit(row + x);
                        } else {                                                 // any other (r >= 1): its two ends
                            if (xl >= 0) visit(row + xl);
                            if (xh <= G - 1) visit(row + xh);
                        }
                    }
                const double B = ring_bound(g, pi, c, r);
                if (B == INFINITY) break;                        // every cell has been seen
                // fp32 d2 of an unseen point >= B (1 - 2^-22) unless B is near the underflow of a square; the strict <
                // leaves a tie with the k-th key to the next ring
                if (worst != NO_KEY && B > 1e-30 && (double)__uint_as_float((unsigned)(worst >> 32)) < B * (1.0 - 0x1p-18))
                    break;
            }
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

unsigned grid_x(long long items) {
    const long long b = (items + NT - 1) / NT;
    return (unsigned)(b < 1 ? 1 : b > MAX_GRID_X ? MAX_GRID_X : b);
}

}  // namespace

extern "C" int64_t gv_points_normals_workspace_bytes(int32_t n, int64_t total_points, int32_t grid_cells) {
    if (n <= 0 || total_points < 0 || grid_cells < 0 || grid_cells > MAX_G) return GV_E_BADARG;
    if (n > 65535) return GV_E_UNSUPPORTED;
    return ws_layout(n, total_points, grid_cells).bytes;
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
    const NormalsWs L = ws_layout(n, total_points, grid_cells);
    if (workspace_bytes < L.bytes) return GV_E_BADARG;
    if (!gv_aligned16(workspace) || ((uintptr_t)point_offsets & 7u) ||
        (((uintptr_t)points | (uintptr_t)normals | (uintptr_t)neighbours | (uintptr_t)variation | (uintptr_t)status) & 3u))
        return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    NArgs a;
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
    a.k = k;
    a.orient = orient;
    a.hint = grid_cells;
    for (int c = 0; c < 3; ++c) a.vp[c] = orient == GV_NORMALS_ORIENT_VIEWPOINT ? (double)viewpoint[c] : 0.0;
    a.normals = normals;
    a.neighbours = neighbours;
    a.variation = variation;
    // max_points sizes the launches only: every kernel strides what its grid does not cover
    const long long G = cells_per_axis(max_points, grid_cells);
    const dim3 by_point(grid_x(max_points), (unsigned)n), by_cell(grid_x(G * G * G), (unsigned)n);
    GV_HIP_CHECK(hipMemsetAsync(a.cell_count, 0, (size_t)L.cells * 4, st));
    hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)n), dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(cell_base_kernel, dim3(1), dim3(SCAN_T), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(bin_kernel<false>, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(alloc_kernel, by_cell, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(bin_kernel<true>, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    if (k <= 8) hipLaunchKernelGGL(query_kernel<8>, by_point, dim3(NT), 0, st, a);
    else if (k <= 16) hipLaunchKernelGGL(query_kernel<16>, by_point, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(query_kernel<32>, by_point, dim3(NT), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
