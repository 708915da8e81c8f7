// render.hip — multi-view rasteriser: a batch of triangle meshes -> the backbone's input views [N, V, H, W, 3] on the
// device (the rendering contract is in include/gvcnn_hip.h, "meshes in").
//
//   gv_render_prepare   normalise_kernel   one workgroup per mesh: bbox midpoint c, radius r, scale = fit / r, status.
//                       bin_kernel<false>  grid (triangle chunks, view, mesh): every thread sets up its triangles for
//                                          the view (vertex transform, snap, orientation, pixel-centre bbox) and counts
//                                          them into the image's 16x16-pixel tiles with LDS atomics; the workgroup then
//                                          adds its nonzero tile counts to the global counters (one atomic per
//                                          workgroup and tile, never per fragment).  View 0 also writes every triangle's
//                                          flat shading factor (world-space normal, view independent).
//                       scan_images_kernel one workgroup: exclusive scan of the per-image pair totals, the grand total.
//                       scan_tiles_kernel  one workgroup per image: tile list starts = image base + scan of its tiles.
//   gv_render_draw      bin_kernel<true>   the same setup and the same LDS counts; each workgroup reserves a run of
//                                          every tile list it feeds (one atomic per workgroup and tile) and places its
//                                          triangle ids there through LDS cursors.  List order is scheduling dependent;
//                                          nothing downstream depends on it.
//                       raster_kernel      one workgroup per tile (256 threads = 16 x 16 pixels): the tile's list is
//                                          streamed through LDS 256 setups at a time; each pixel keeps the smallest
//                                          64-bit key (Z << 32 | triangle id) in a register and writes its outputs once.
//
// No thread walks more than one tile's pixels: a triangle that covers the whole screen sits in every tile list it
// touches and each tile's threads test it against their own pixel.  The triangle setup is a pure function of (mesh,
// view, triangle), recomputed where needed (count, scatter, raster), so the bins hold 4-byte ids only.
#include <math.h>

#include "gv_common.h"

// Every fp32 step rounds on its own, so numpy float32 reproduces it.  hipcc contracts a * b + c into one FMA by default,
// the header's __fmul_rn / __fadd_rn included (they are plain operators there): this file turns contraction off and
// spells each step with the helpers below.  The one fused step, the quantised output, is an explicit fmaf.  Division is
// IEEE (HIP's default); the square root is __builtin_sqrtf, correctly rounded (__fsqrt_rn is the native approximation).
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

typedef unsigned long long u64;

constexpr int TS = 16;                                           // tile edge in pixels
constexpr int RT = 256;                                          // threads of every kernel but the scans
constexpr int SCAN_T = 1024;                                     // threads of the scan kernels
constexpr int CHUNK = 1024;                                      // triangles per binning workgroup and pass
constexpr int MAX_SIDE = 512;
constexpr int MAX_TILES = (MAX_SIDE / TS) * (MAX_SIDE / TS);     // 1024
constexpr int MAX_TRIS = 1 << 24;
// snapped coordinates are clamped to +-2^18 (+-1024 pixels; a vertex of the unit sphere lands inside the image): a
// triangle then spans at most 2^19 per axis, twice its area is below 2^38 and e0*Z0 + e1*Z1 + e2*Z2 <= area * (2^24-1)
// stays below 2^62, whatever the input
constexpr float SNAP_LIM = 262144.0f;
constexpr u64 BG_KEY = ~0ull;

struct MeshXf {                                                  // per mesh, written by normalise_kernel
    float cx, cy, cz, scale;
    int status, pad0, pad1, pad2;
};

struct Args {                                                    // everything a triangle setup needs
    const float* verts;
    const long long* voff;
    const int* tris;
    const long long* toff;
    const float* cams;                                           // [V, 3, 3]
    const float* rots;                                           // [N, 3, 3] or null
    const MeshXf* xf;
    int V, H, W, tiles_x, tiles_y, persp;
    float k, D, da, db, cxs, cys;                                // projection constants, image centre
};

struct Tri {
    int x0, y0, x1, y1, x2, y2;
    unsigned z0, z1, z2;
    int px0, px1, py0, py1;
    long long area;
};

__device__ __forceinline__ float dot3(const float* r, float a, float b, float c) {
    return add_rn(add_rn(mul_rn(r[0], a), mul_rn(r[1], b)), mul_rn(r[2], c));
}

// normalised (and rotated) world position w of a vertex
__device__ __forceinline__ void world(const MeshXf& x, const float* M, const float* p, float w[3]) {
    const float u0 = mul_rn(add_rn(p[0], -x.cx), x.scale);
    const float u1 = mul_rn(add_rn(p[1], -x.cy), x.scale);
    const float u2 = mul_rn(add_rn(p[2], -x.cz), x.scale);
    if (M) {
        w[0] = dot3(M, u0, u1, u2);
        w[1] = dot3(M + 3, u0, u1, u2);
        w[2] = dot3(M + 6, u0, u1, u2);
    } else {
        w[0] = u0;
        w[1] = u1;
        w[2] = u2;
    }
}

__device__ __forceinline__ int snap(float s) {
    return (int)rintf(fminf(fmaxf(mul_rn(s, 256.0f), -SNAP_LIM), SNAP_LIM));
}

// camera transform, projection, 1/256-pixel snap, 24-bit depth
__device__ __forceinline__ void project(const Args& a, const float* C, const float w[3], int& X, int& Y, unsigned& Z) {
    const float q0 = dot3(C, w[0], w[1], w[2]), q1 = dot3(C + 3, w[0], w[1], w[2]), q2 = dot3(C + 6, w[0], w[1], w[2]);
    float sx, sy, t;
    if (a.persp) {
        const float z = add_rn(q2, a.D);
        sx = add_rn(a.cxs, __fdiv_rn(mul_rn(q0, a.k), z));
        sy = add_rn(a.cys, -__fdiv_rn(mul_rn(q1, a.k), z));
        t = add_rn(a.da, -__fdiv_rn(a.db, z));
    } else {
        sx = add_rn(a.cxs, mul_rn(q0, a.k));
        sy = add_rn(a.cys, -mul_rn(q1, a.k));
        t = mul_rn(add_rn(q2, 1.0f), 0.5f);
    }
    X = snap(sx);
    Y = snap(sy);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    Z = (unsigned)rintf(mul_rn(t, 16777215.0f));
}

__device__ __forceinline__ bool load_tri(const Args& a, int m, int t, const float*& p0, const float*& p1,
                                         const float*& p2) {
    const long long tb = a.toff[m] - a.toff[0], vb = a.voff[m] - a.voff[0];
    const long long nv = a.voff[m + 1] - a.voff[m];
    if (t < 0 || t >= a.toff[m + 1] - a.toff[m]) return false;   // a tile-list slot a matching prepare never wrote
    const int* ix = a.tris + (tb + t) * 3;
    const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return false;
    p0 = a.verts + (vb + i0) * 3;
    p1 = a.verts + (vb + i1) * 3;
    p2 = a.verts + (vb + i2) * 3;
    return true;
}

// setup of triangle t of mesh m in view v: false when it covers no pixel centre (zero area, off screen, bad index)
__device__ bool tri_setup(const Args& a, int m, int v, int t, Tri& T) {
    const float *p0, *p1, *p2;
    if (!load_tri(a, m, t, p0, p1, p2)) return false;
    const MeshXf x = a.xf[m];
    const float* M = a.rots ? a.rots + (size_t)m * 9 : nullptr;
    const float* C = a.cams + (size_t)v * 9;
    float w[3];
    world(x, M, p0, w);
    project(a, C, w, T.x0, T.y0, T.z0);
    world(x, M, p1, w);
    project(a, C, w, T.x1, T.y1, T.z1);
    world(x, M, p2, w);
    project(a, C, w, T.x2, T.y2, T.z2);
    long long area = (long long)(T.x1 - T.x0) * (T.y2 - T.y0) - (long long)(T.y1 - T.y0) * (T.x2 - T.x0);
    if (area == 0) return false;
    if (area < 0) {                                              // orient to positive area
        int s = T.x1; T.x1 = T.x2; T.x2 = s;
        s = T.y1; T.y1 = T.y2; T.y2 = s;
        const unsigned z = T.z1; T.z1 = T.z2; T.z2 = z;
        area = -area;
    }
    T.area = area;
    const int xmin = min(T.x0, min(T.x1, T.x2)), xmax = max(T.x0, max(T.x1, T.x2));
    const int ymin = min(T.y0, min(T.y1, T.y2)), ymax = max(T.y0, max(T.y1, T.y2));
    // pixel centres 256 i + 128 inside [min, max]
    T.px0 = max((xmin + 127) >> 8, 0);
    T.px1 = min((xmax - 128) >> 8, a.W - 1);
    T.py0 = max((ymin + 127) >> 8, 0);
    T.py1 = min((ymax - 128) >> 8, a.H - 1);
    return T.px0 <= T.px1 && T.py0 <= T.py1;
}

// flat shading factor of a triangle (winding-defined world normal)
__device__ float shade_factor(const MeshXf& x, const float* M, const float* p0, const float* p1, const float* p2,
                              float3 light, float ambient, int two_sided) {
    float w0[3], w1[3], w2[3];
    world(x, M, p0, w0);
    world(x, M, p1, w1);
    world(x, M, p2, w2);
    const float a0 = add_rn(w1[0], -w0[0]), a1 = add_rn(w1[1], -w0[1]), a2 = add_rn(w1[2], -w0[2]);
    const float b0 = add_rn(w2[0], -w0[0]), b1 = add_rn(w2[1], -w0[1]), b2 = add_rn(w2[2], -w0[2]);
    const float n0 = add_rn(mul_rn(a1, b2), -mul_rn(a2, b1));
    const float n1 = add_rn(mul_rn(a2, b0), -mul_rn(a0, b2));
    const float n2 = add_rn(mul_rn(a0, b1), -mul_rn(a1, b0));
    const float nl = add_rn(add_rn(mul_rn(n0, light.x), mul_rn(n1, light.y)), mul_rn(n2, light.z));
    const float nn = add_rn(add_rn(mul_rn(n0, n0), mul_rn(n1, n1)), mul_rn(n2, n2));
    const float s = nn > 0.0f ? __fdiv_rn(nl, __builtin_sqrtf(nn)) : 0.0f;
    const float h = two_sided ? fabsf(s) : mul_rn(add_rn(s, 1.0f), 0.5f);
    return add_rn(ambient, mul_rn(add_rn(1.0f, -ambient), h));
}

// ---- normalisation -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void normalise_kernel(const float* __restrict__ verts, const long long* __restrict__ voff,
                                                       const long long* __restrict__ toff, long long total_verts,
                                                       long long total_tris, float fit, MeshXf* __restrict__ xf,
                                                       int* __restrict__ status) {
    __shared__ float s_red[6][RT];
    const int m = blockIdx.x, tid = threadIdx.x;
    const long long v0 = voff[m] - voff[0], v1 = voff[m + 1] - voff[0];
    const long long t0 = toff[m] - toff[0], t1 = toff[m + 1] - toff[0];
    int st = GV_RENDER_OK;
    if (v0 < 0 || v1 < v0 || v1 > total_verts || t0 < 0 || t1 < t0 || t1 > total_tris) st = GV_RENDER_BAD_OFFSETS;
    else if (t1 - t0 > MAX_TRIS) st = GV_RENDER_TOO_LARGE;
    else if (t1 == t0 || v1 == v0) st = GV_RENDER_EMPTY;
    MeshXf x = {0.f, 0.f, 0.f, 0.f, st, 0, 0, 0};
    if (st == GV_RENDER_OK) {                                    // (uniform)
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (long long i = v0 + tid; i < v1; i += RT)
            for (int c = 0; c < 3; ++c) {
                const float p = verts[i * 3 + c];
                mn[c] = fminf(mn[c], p);
                mx[c] = fmaxf(mx[c], p);
            }
        for (int c = 0; c < 3; ++c) {
            s_red[c][tid] = mn[c];
            s_red[3 + c][tid] = mx[c];
        }
        __syncthreads();
        for (int s = RT / 2; s > 0; s >>= 1) {
            if (tid < s)
                for (int c = 0; c < 3; ++c) {
                    s_red[c][tid] = fminf(s_red[c][tid], s_red[c][tid + s]);
                    s_red[3 + c][tid] = fmaxf(s_red[3 + c][tid], s_red[3 + c][tid + s]);
                }
            __syncthreads();
        }
        x.cx = mul_rn(add_rn(s_red[0][0], s_red[3][0]), 0.5f);
        x.cy = mul_rn(add_rn(s_red[1][0], s_red[4][0]), 0.5f);
        x.cz = mul_rn(add_rn(s_red[2][0], s_red[5][0]), 0.5f);
        __syncthreads();
        float r2 = 0.0f;                                         // max of the squared distances: sqrt is monotone
        for (long long i = v0 + tid; i < v1; i += RT) {
            const float dx = add_rn(verts[i * 3], -x.cx), dy = add_rn(verts[i * 3 + 1], -x.cy);
            const float dz = add_rn(verts[i * 3 + 2], -x.cz);
            r2 = fmaxf(r2, add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));
        }
        s_red[0][tid] = r2;
        __syncthreads();
        for (int s = RT / 2; s > 0; s >>= 1) {
            if (tid < s) s_red[0][tid] = fmaxf(s_red[0][tid], s_red[0][tid + s]);
            __syncthreads();
        }
        const float r = __builtin_sqrtf(s_red[0][0]);
        if (!isfinite(r)) x.status = GV_RENDER_NONFINITE;
        else if (r == 0.0f) x.status = GV_RENDER_ZERO_RADIUS;
        else {
            x.scale = __fdiv_rn(fit, r);
            if (!isfinite(x.scale)) x.status = GV_RENDER_NONFINITE;
        }
    }
    if (tid == 0) {
        xf[m] = x;
        status[m] = x.status;
    }
}

// ---- binning: count (SCATTER = false) and scatter (SCATTER = true) --------------------------------------------------
template <bool SCATTER>
__global__ __launch_bounds__(RT) void bin_kernel(Args a, int* __restrict__ tile_count, long long* __restrict__ image_total,
                                                 float* __restrict__ shade, float3 light, float ambient, int two_sided,
                                                 const long long* __restrict__ tile_start, int* __restrict__ tile_fill,
                                                 int* __restrict__ bins, long long cap) {
    __shared__ int s_cnt[MAX_TILES];
    __shared__ long long s_base[SCATTER ? MAX_TILES : 1];
    __shared__ long long s_sum[RT / 64];
    const int m = blockIdx.z, v = blockIdx.y, tid = threadIdx.x;
    if (a.xf[m].status != GV_RENDER_OK) return;                  // (uniform)
    const int nt = (int)(a.toff[m + 1] - a.toff[m]);
    const int T = a.tiles_x * a.tiles_y;
    const long long img = (long long)m * a.V + v;
    const int stride = gridDim.x * CHUNK;
    for (int c0 = blockIdx.x * CHUNK; c0 < nt; c0 += stride) {
        for (int i = tid; i < T; i += RT) s_cnt[i] = 0;
        __syncthreads();
        for (int t = c0 + tid; t < min(c0 + CHUNK, nt); t += RT) {
            if (!SCATTER && v == 0) {
                const float *p0, *p1, *p2;
                if (load_tri(a, m, t, p0, p1, p2))
                    shade[a.toff[m] - a.toff[0] + t] = shade_factor(a.xf[m], a.rots ? a.rots + (size_t)m * 9 : nullptr,
                                                                    p0, p1, p2, light, ambient, two_sided);
            }
            Tri q;
            if (!tri_setup(a, m, v, t, q)) continue;
            for (int ty = q.py0 >> 4; ty <= q.py1 >> 4; ++ty)
                for (int tx = q.px0 >> 4; tx <= q.px1 >> 4; ++tx) atomicAdd(&s_cnt[ty * a.tiles_x + tx], 1);
        }
        __syncthreads();
        long long local = 0;
        for (int i = tid; i < T; i += RT) {
            const int c = s_cnt[i];
            if (!c) continue;
            if (SCATTER) {
                s_base[i] = tile_start[img * T + i] + atomicAdd(&tile_fill[img * T + i], c);
                s_cnt[i] = 0;                                    // now the workgroup's cursor into its run
            } else {
                atomicAdd(&tile_count[img * T + i], c);
                local += c;
            }
        }
        if (!SCATTER) {
            for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
            if ((tid & 63) == 0) s_sum[tid >> 6] = local;
            __syncthreads();
            if (tid == 0) {
                const long long s = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
                if (s) atomicAdd((u64*)&image_total[img], (u64)s);
            }
        } else {
            __syncthreads();
            for (int t = c0 + tid; t < min(c0 + CHUNK, nt); t += RT) {
                Tri q;
                if (!tri_setup(a, m, v, t, q)) continue;
                for (int ty = q.py0 >> 4; ty <= q.py1 >> 4; ++ty)
                    for (int tx = q.px0 >> 4; tx <= q.px1 >> 4; ++tx) {
                        const int i = ty * a.tiles_x + tx;
                        const long long pos = s_base[i] + atomicAdd(&s_cnt[i], 1);
                        if (pos < cap) bins[pos] = t;
                    }
            }
        }
        __syncthreads();                                         // s_cnt / s_sum are reused by the next chunk
    }
}

// exclusive scan of the per-image totals (one workgroup); *total = their sum
__global__ __launch_bounds__(SCAN_T) void scan_images_kernel(const long long* __restrict__ image_total, long long nimg,
                                                             long long* __restrict__ image_base,
                                                             long long* __restrict__ total) {
    __shared__ long long s[SCAN_T];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (long long b = 0; b < nimg; b += SCAN_T) {
        const long long i = b + tid;
        const long long v = i < nimg ? image_total[i] : 0;
        s[tid] = v;
        __syncthreads();
        for (int o = 1; o < SCAN_T; o <<= 1) {
            const long long add = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (i < nimg) image_base[i] = carry + s[tid] - v;
        carry += s[SCAN_T - 1];
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// tile list starts of one image: image base + exclusive scan of its tile counts (T <= 1024)
__global__ __launch_bounds__(SCAN_T) void scan_tiles_kernel(const int* __restrict__ tile_count,
                                                            const long long* __restrict__ image_base, int T,
                                                            long long* __restrict__ tile_start) {
    __shared__ long long s[SCAN_T];
    const int tid = threadIdx.x;
    const long long img = blockIdx.x;
    const long long v = tid < T ? tile_count[img * T + tid] : 0;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {
        const long long add = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    if (tid < T) tile_start[img * T + tid] = image_base[img] + s[tid] - v;
}

// ---- raster + resolve ----------------------------------------------------------------------------------------------
struct LTri {                                                    // one setup in LDS (64 bytes)
    int x0, y0, x1, y1, x2, y2;
    unsigned z0, z1, z2;
    int bx, by;                                                  // px0 | px1 << 16, py0 | py1 << 16
    int id;                                                      // triangle id | owned-edge bits << 24
    long long area;
    int pad0, pad1;
};

// the top-left rule.  Positive area in the y-down frame means clockwise on screen: a top edge runs left to right
// (dy == 0, dx > 0) and a left edge runs upwards (dy < 0); those edges own the pixel centres on them
__device__ __forceinline__ int owns(int ax, int ay, int bx, int by) {
    const int dx = bx - ax, dy = by - ay;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 1 : 0;
}
__device__ __forceinline__ long long edge(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

template <int OUT>
__global__ __launch_bounds__(RT) void raster_kernel(Args a, const float* __restrict__ shade,
                                                    const int* __restrict__ tile_count,
                                                    const long long* __restrict__ tile_start,
                                                    const int* __restrict__ bins, long long cap, float3 color,
                                                    float3 background, void* __restrict__ out, int* __restrict__ face_id,
                                                    unsigned* __restrict__ depth) {
    __shared__ LTri s_tri[RT];
    const int T = a.tiles_x * a.tiles_y;
    const int tile = blockIdx.x, v = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    const long long img = (long long)m * a.V + v;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int px = tx * TS + (tid & (TS - 1)), py = ty * TS + (tid >> 4);
    const int PX = px * 256 + 128, PY = py * 256 + 128;
    u64 best = BG_KEY;
    if (a.xf[m].status == GV_RENDER_OK) {
        const long long start = tile_start[img * T + tile];
        const long long end = min(start + (long long)tile_count[img * T + tile], cap);
        for (long long c0 = start; c0 < end; c0 += RT) {
            const int n = (int)min((long long)RT, end - c0);
            if (tid < n) {
                const int t = bins[c0 + tid];
                Tri q;
                LTri& L = s_tri[tid];
                if (tri_setup(a, m, v, t, q)) {
                    L.x0 = q.x0; L.y0 = q.y0; L.x1 = q.x1; L.y1 = q.y1; L.x2 = q.x2; L.y2 = q.y2;
                    L.z0 = q.z0; L.z1 = q.z1; L.z2 = q.z2;
                    L.bx = q.px0 | (q.px1 << 16);
                    L.by = q.py0 | (q.py1 << 16);
                    L.id = t | (owns(q.x1, q.y1, q.x2, q.y2) << 24) | (owns(q.x2, q.y2, q.x0, q.y0) << 25) |
                           (owns(q.x0, q.y0, q.x1, q.y1) << 26);
                    L.area = q.area;
                } else {
                    L.bx = 1;                                    // empty range: px0 = 1 > px1 = 0
                    L.by = 0;
                }
            }
            __syncthreads();
            for (int i = 0; i < n; ++i) {
                const LTri& L = s_tri[i];
                if (px < (L.bx & 0xffff) || px > (L.bx >> 16) || py < (L.by & 0xffff) || py > (L.by >> 16)) continue;
                const long long e0 = edge(L.x1, L.y1, L.x2, L.y2, PX, PY);
                const long long e1 = edge(L.x2, L.y2, L.x0, L.y0, PX, PY);
                const long long e2 = edge(L.x0, L.y0, L.x1, L.y1, PX, PY);
                const bool in = (e0 > 0 || (e0 == 0 && (L.id >> 24 & 1))) && (e1 > 0 || (e1 == 0 && (L.id >> 25 & 1))) &&
                                (e2 > 0 || (e2 == 0 && (L.id >> 26 & 1)));
                if (!in) continue;
                const u64 num = (u64)e0 * L.z0 + (u64)e1 * L.z1 + (u64)e2 * L.z2;
                // exact early-out: Z = num div area >= bestZ + 1 exactly when num >= (bestZ + 1) * area (< 2^62)
                if (best != BG_KEY && num >= ((best >> 32) + 1) * (u64)L.area) continue;
                const u64 Z = num / (u64)L.area;
                const u64 key = (Z << 32) | (unsigned)(L.id & 0xffffff);
                best = key < best ? key : best;
            }
            __syncthreads();
        }
    }
    if (px >= a.W || py >= a.H) return;
    const size_t p = ((size_t)img * a.H + py) * a.W + px;
    float c0 = background.x, c1 = background.y, c2 = background.z;
    if (best != BG_KEY) {
        const int id = (int)(best & 0xffffffffu);
        const float f = shade[a.toff[m] - a.toff[0] + id];
        c0 = mul_rn(color.x, f);
        c1 = mul_rn(color.y, f);
        c2 = mul_rn(color.z, f);
    }
    if (face_id) face_id[p] = best == BG_KEY ? -1 : (int)(best & 0xffffffffu);
    if (depth) depth[p] = best == BG_KEY ? 0xFFFFFFFFu : (unsigned)(best >> 32);
    if (OUT == GV_RENDER_OUT_F32) {
        float* o = static_cast<float*>(out) + p * 3;
        o[0] = add_rn(c0, -0.5f);
        o[1] = add_rn(c1, -0.5f);
        o[2] = add_rn(c2, -0.5f);
    } else {
        const float cs[3] = {c0, c1, c2};
        unsigned char u[3];
        for (int c = 0; c < 3; ++c)
            u[c] = (unsigned char)fminf(fmaxf(floorf(add_rn(mul_rn(cs[c], 255.0f), 0.5f)), 0.0f), 255.0f);
        if (OUT == GV_RENDER_OUT_U8) {
            unsigned char* o = static_cast<unsigned char*>(out) + p * 3;
            o[0] = u[0];
            o[1] = u[1];
            o[2] = u[2];
        } else {
            float* o = static_cast<float*>(out) + p * 3;
            // what gv_preprocess_views computes from the PNG bytes (its u8 * (1/255) - 0.5 compiles to one FMA)
            for (int c = 0; c < 3; ++c) o[c] = __builtin_fmaf((float)u[c], 1.0f / 255.0f, -0.5f);
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct WsLayout {
    int64_t xf, shade, tile_count, tile_fill, tile_start, image_total, image_base, bytes;
};

WsLayout ws_layout(int32_t n, int32_t v, int32_t h, int32_t w, int64_t total_tris) {
    const int64_t T = (int64_t)((h + TS - 1) / TS) * ((w + TS - 1) / TS);
    const int64_t nimg = (int64_t)n * v;
    WsLayout L;
    int64_t o = 0;
    L.xf = o;          o += round_up((int64_t)n * sizeof(MeshXf), 256);
    L.shade = o;       o += round_up((total_tris > 0 ? total_tris : 1) * 4, 256);
    L.tile_count = o;  o += round_up(nimg * T * 4, 256);
    L.tile_fill = o;   o += round_up(nimg * T * 4, 256);
    L.tile_start = o;  o += round_up(nimg * T * 8, 256);
    L.image_total = o; o += round_up(nimg * 8, 256);
    L.image_base = o;  o += round_up(nimg * 8, 256);
    L.bytes = o;
    return L;
}

bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the checks every entry point shares
int check_common(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
                 int32_t n, int64_t total_verts, int64_t total_tris, int32_t max_tris, const gv_render_desc* d,
                 const float* cameras, const void* workspace, int64_t workspace_bytes) {
    if (!verts || !vert_offsets || !tris || !tri_offsets || !d || !cameras || !workspace) return GV_E_BADARG;
    if (n <= 0 || total_verts < 0 || total_tris < 0 || max_tris < 0) return GV_E_BADARG;
    if (d->height <= 0 || d->width <= 0 || d->num_views <= 0 || (d->flags & ~(GV_RENDER_PERSPECTIVE | GV_RENDER_TWO_SIDED)))
        return GV_E_BADARG;
    if (!(d->fit > 0.0f && d->fit <= 1.0f) || !(d->ambient >= 0.0f && d->ambient <= 1.0f)) return GV_E_BADARG;
    if (!(d->proj_scale > 0.0f) || !isfinite(d->proj_scale)) return GV_E_BADARG;
    if ((d->flags & GV_RENDER_PERSPECTIVE) &&
        !(d->persp_dist > 1.0f && isfinite(d->persp_dist) && isfinite(d->depth_a) && isfinite(d->depth_b)))
        return GV_E_BADARG;
    if (!finite3(d->light) || !finite3(d->color) || !finite3(d->background)) return GV_E_BADARG;
    if (d->height > MAX_SIDE || d->width > MAX_SIDE || d->num_views > 64 || n > 65535 || max_tris > MAX_TRIS)
        return GV_E_UNSUPPORTED;
    if (workspace_bytes < ws_layout(n, d->num_views, d->height, d->width, total_tris).bytes) return GV_E_BADARG;
    if (!gv_aligned16(workspace)) return GV_E_ALIGN;
    return GV_OK;
}

Args make_args(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
               const gv_render_desc* d, const float* cameras, const float* rotations, const MeshXf* xf) {
    Args a;
    a.verts = verts;
    a.voff = (const long long*)vert_offsets;
    a.tris = tris;
    a.toff = (const long long*)tri_offsets;
    a.cams = cameras;
    a.rots = rotations;
    a.xf = xf;
    a.V = d->num_views;
    a.H = d->height;
    a.W = d->width;
    a.tiles_x = (d->width + TS - 1) / TS;
    a.tiles_y = (d->height + TS - 1) / TS;
    a.persp = (d->flags & GV_RENDER_PERSPECTIVE) ? 1 : 0;
    a.k = d->proj_scale;
    a.D = d->persp_dist;
    a.da = d->depth_a;
    a.db = d->depth_b;
    a.cxs = (float)d->width * 0.5f;                              // exact: w <= 512
    a.cys = (float)d->height * 0.5f;
    return a;
}

dim3 bin_grid(int32_t max_tris, int32_t v, int32_t n) {
    const int chunks = max_tris > 0 ? (max_tris + CHUNK - 1) / CHUNK : 1;
    return dim3((unsigned)chunks, (unsigned)v, (unsigned)n);
}

}  // namespace

extern "C" int64_t gv_render_workspace_bytes(int32_t n, int32_t num_views, int32_t height, int32_t width,
                                             int64_t total_tris) {
    if (n <= 0 || num_views <= 0 || height <= 0 || width <= 0 || total_tris < 0) return GV_E_BADARG;
    if (height > MAX_SIDE || width > MAX_SIDE || num_views > 64 || n > 65535) return GV_E_UNSUPPORTED;
    return ws_layout(n, num_views, height, width, total_tris).bytes;
}

extern "C" int64_t gv_render_bins_bytes(int64_t total) {
    if (total < 0) return GV_E_BADARG;
    return round_up((total > 0 ? total : 1) * 4, 256);
}

extern "C" int gv_render_prepare(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                                 const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                                 int32_t max_tris, const gv_render_desc* desc, const float* cameras,
                                 const float* rotations, void* workspace, int64_t workspace_bytes, int64_t* pair_total,
                                 int32_t* status, void* stream) {
    if (!pair_total || !status) return GV_E_BADARG;
    const int rc = check_common(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc,
                                cameras, workspace, workspace_bytes);
    if (rc != GV_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const WsLayout L = ws_layout(n, desc->num_views, desc->height, desc->width, total_tris);
    char* ws = static_cast<char*>(workspace);
    MeshXf* xf = reinterpret_cast<MeshXf*>(ws + L.xf);
    const Args a = make_args(verts, vert_offsets, tris, tri_offsets, desc, cameras, rotations, xf);
    const int T = a.tiles_x * a.tiles_y;
    const long long nimg = (long long)n * desc->num_views;
    GV_HIP_CHECK(hipMemsetAsync(ws + L.tile_count, 0, (size_t)nimg * T * 4, st));
    GV_HIP_CHECK(hipMemsetAsync(ws + L.image_total, 0, (size_t)nimg * 8, st));
    hipLaunchKernelGGL(normalise_kernel, dim3(n), dim3(RT), 0, st, verts, (const long long*)vert_offsets,
                       (const long long*)tri_offsets, (long long)total_verts, (long long)total_tris, desc->fit, xf,
                       status);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(bin_kernel<false>, bin_grid(max_tris, desc->num_views, n), dim3(RT), 0, st, a,
                       reinterpret_cast<int*>(ws + L.tile_count), reinterpret_cast<long long*>(ws + L.image_total),
                       reinterpret_cast<float*>(ws + L.shade), make_float3(desc->light[0], desc->light[1], desc->light[2]),
                       desc->ambient, (desc->flags & GV_RENDER_TWO_SIDED) ? 1 : 0, nullptr, nullptr, nullptr, 0ll);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_images_kernel, dim3(1), dim3(SCAN_T), 0, st,
                       reinterpret_cast<const long long*>(ws + L.image_total), nimg,
                       reinterpret_cast<long long*>(ws + L.image_base), (long long*)pair_total);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)nimg), dim3(SCAN_T), 0, st,
                       reinterpret_cast<const int*>(ws + L.tile_count),
                       reinterpret_cast<const long long*>(ws + L.image_base), T,
                       reinterpret_cast<long long*>(ws + L.tile_start));
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_render_draw(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                              const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                              int32_t max_tris, const gv_render_desc* desc, const float* cameras, const float* rotations,
                              void* workspace, int64_t workspace_bytes, void* bins, int64_t bins_bytes, int64_t total,
                              int32_t output, void* out, int32_t* face_id, uint32_t* depth, void* stream) {
    if (!bins || !out || total < 0) return GV_E_BADARG;
    if (output != GV_RENDER_OUT_F32_QUANTIZED && output != GV_RENDER_OUT_F32 && output != GV_RENDER_OUT_U8)
        return GV_E_BADARG;
    const int rc = check_common(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc,
                                cameras, workspace, workspace_bytes);
    if (rc != GV_OK) return rc;
    if (bins_bytes < gv_render_bins_bytes(total)) return GV_E_BADARG;
    if (!gv_aligned16(bins) || (output != GV_RENDER_OUT_U8 && ((uintptr_t)out & 3u))) return GV_E_ALIGN;
    if (((uintptr_t)face_id & 3u) || ((uintptr_t)depth & 3u)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const WsLayout L = ws_layout(n, desc->num_views, desc->height, desc->width, total_tris);
    char* ws = static_cast<char*>(workspace);
    const MeshXf* xf = reinterpret_cast<const MeshXf*>(ws + L.xf);
    const Args a = make_args(verts, vert_offsets, tris, tri_offsets, desc, cameras, rotations, xf);
    const int T = a.tiles_x * a.tiles_y;
    const long long nimg = (long long)n * desc->num_views;
    const long long cap = bins_bytes / 4;
    GV_HIP_CHECK(hipMemsetAsync(ws + L.tile_fill, 0, (size_t)nimg * T * 4, st));
    hipLaunchKernelGGL(bin_kernel<true>, bin_grid(max_tris, desc->num_views, n), dim3(RT), 0, st, a, nullptr, nullptr,
                       nullptr, make_float3(0.f, 0.f, 0.f), 0.f, 0, reinterpret_cast<const long long*>(ws + L.tile_start),
                       reinterpret_cast<int*>(ws + L.tile_fill), static_cast<int*>(bins), cap);
    GV_LAUNCH_CHECK();
    const float3 color = make_float3(desc->color[0], desc->color[1], desc->color[2]);
    const float3 bg = make_float3(desc->background[0], desc->background[1], desc->background[2]);
    const dim3 grid((unsigned)T, (unsigned)desc->num_views, (unsigned)n);
    const float* shade = reinterpret_cast<const float*>(ws + L.shade);
    const int* tc = reinterpret_cast<const int*>(ws + L.tile_count);
    const long long* ts = reinterpret_cast<const long long*>(ws + L.tile_start);
    const int* b = static_cast<const int*>(bins);
    if (output == GV_RENDER_OUT_F32_QUANTIZED)
        hipLaunchKernelGGL(raster_kernel<GV_RENDER_OUT_F32_QUANTIZED>, grid, dim3(RT), 0, st, a, shade, tc, ts, b, cap,
                           color, bg, out, face_id, depth);
    else if (output == GV_RENDER_OUT_F32)
        hipLaunchKernelGGL(raster_kernel<GV_RENDER_OUT_F32>, grid, dim3(RT), 0, st, a, shade, tc, ts, b, cap, color, bg,
                           out, face_id, depth);
    else
        hipLaunchKernelGGL(raster_kernel<GV_RENDER_OUT_U8>, grid, dim3(RT), 0, st, a, shade, tc, ts, b, cap, color, bg,
                           out, face_id, depth);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
