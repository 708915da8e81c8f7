// render.hip — multi-view rasteriser: a batch of triangle meshes -> the backbone's input views [N, V, H, W, 3] on the
// device (the rendering contract is in include/gvcnn_hip.h, "meshes in").
//
//   gv_render_prepare   normalise_kernel       (render_common.h, as the scans) one workgroup per mesh: bbox midpoint c,
//                                              radius r, scale = fit / r, status.
//                       tile_bin_kernel<false> (render_tiles.h, over MeshPrim<LS>) grid (triangle chunks, view, mesh): every
//                                              thread sets up its triangles for the view (vertex transform, snap,
//                                              orientation, pixel-centre bbox) and counts them into the image's
//                                              16x16-pixel tiles.  View 0 also writes every triangle's flat shading factor
//                                              (world-space normal, view independent).
//                       scan_images_kernel     one workgroup: exclusive scan of the per-image pair totals, the grand total.
//                       scan_tiles_kernel      one workgroup per image: tile list starts = image base + scan of its tiles.
//   gv_render_draw      tile_bin_kernel<true>  the same setup; places the triangle ids in the tile lists.
//                       raster_kernel          one workgroup per tile (256 threads = 16 x 16 pixels): the tile's list is
//                                              streamed through LDS 256 setups at a time; each pixel keeps the smallest
//                                              64-bit key (Z << 32 | triangle id) in a register and writes its outputs once.
//
// gv_render_prepare_ss / gv_render_draw_ss: the same launches with S x S samples per pixel (S = 1 << LS = 1, 2, 4; LS is a
// template parameter of tri_setup, MeshPrim and raster_kernel; LS = 0 is the code behind the original pair).  The
// triangle's box is taken over the sample grid, so binning depends on S; a raster thread still owns one pixel and keeps
// its S * S keys in registers, and resolves them to the pixel in the same launch.
//
// Smooth shading (gv_render_vertex_normals, then gv_render_draw_smooth in place of the draw call):
//   vertex_normals_kernel  one thread per (normal table, vertex): gathers the face vectors of the vertex's corners over a
//                          host-built CSR in ascending triangle order and normalises the sum.
//   raster_kernel<.., SM = true>  the same raster loop; the resolve recomputes the winning triangle's setup and edge
//                          functions per covered sample, interpolates the three vertex normals and shades the sample
//                          (smooth_colour, the reflection model of render_common.h).  SM = false is the flat code, instantiated from the same source as before.
//
// No thread walks more than one tile's pixels: a triangle that covers the whole screen sits in every tile list it
// touches and each tile's threads test it against their own pixel.  The triangle setup is a pure function of (mesh,
// view, triangle), recomputed where needed (count, scatter, raster), so the bins hold 4-byte ids only.
#include <math.h>

// the fp32 discipline (mul_rn / add_rn, no contraction), MeshXf, world, project, snap, dot3, the reflection model, the pixel
// store, normalise_kernel, the binning kernel and the two scan kernels are shared with render_points.hip
#include "render_tiles.h"

#pragma clang fp contract(off)

namespace {

struct Args : View {                                             // everything a triangle setup needs
    const float* verts;
    const long long* voff;
    const int* tris;
    const long long* toff;
    const float* cams;                                           // [V, 3, 3]
    const float* rots;                                           // [N, 3, 3] or null
    const MeshXf* xf;
};

struct Tri {
    int x0, y0, x1, y1, x2, y2;
    unsigned z0, z1, z2;
    int px0, px1, py0, py1;
    long long area;
    int flip;                                                    // vertices 1 and 2 were swapped (smooth shading)
};

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

// setup of triangle t of mesh m in view v with S = 1 << LS samples per pixel and axis: false when its box holds no
// sample (zero area, off screen, bad index).  px0..py1 is the pixel range of the sample box.
template <int LS>
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
    T.flip = area < 0;
    if (area < 0) {                                              // orient to positive area
        int s = T.x1; T.x1 = T.x2; T.x2 = s;
        s = T.y1; T.y1 = T.y2; T.y2 = s;
        const unsigned z = T.z1; T.z1 = T.z2; T.z2 = z;
        area = -area;
    }
    T.area = area;
    const int xmin = min(T.x0, min(T.x1, T.x2)), xmax = max(T.x0, max(T.x1, T.x2));
    const int ymin = min(T.y0, min(T.y1, T.y2)), ymax = max(T.y0, max(T.y1, T.y2));
    // samples step * g + step / 2 inside [min, max], step = 256 >> LS (LS = 0: the pixel centres 256 i + 128)
    constexpr int LG = 8 - LS, HALF = 128 >> LS;
    const int gx0 = max((xmin + HALF - 1) >> LG, 0), gx1 = min((xmax - HALF) >> LG, (a.W << LS) - 1);
    const int gy0 = max((ymin + HALF - 1) >> LG, 0), gy1 = min((ymax - HALF) >> LG, (a.H << LS) - 1);
    T.px0 = gx0 >> LS;
    T.px1 = gx1 >> LS;
    T.py0 = gy0 >> LS;
    T.py1 = gy1 >> LS;
    return gx0 <= gx1 && gy0 <= gy1;
}

// face vector n = (w1 - w0) x (w2 - w0) of a triangle, unnormalised
__device__ __forceinline__ void face_vector(const MeshXf& x, const float* M, const float* p0, const float* p1,
                                            const float* p2, float n[3]) {
    float w0[3], w1[3], w2[3];
    world(x, M, p0, w0);
    world(x, M, p1, w1);
    world(x, M, p2, w2);
    const float a0 = add_rn(w1[0], -w0[0]), a1 = add_rn(w1[1], -w0[1]), a2 = add_rn(w1[2], -w0[2]);
    const float b0 = add_rn(w2[0], -w0[0]), b1 = add_rn(w2[1], -w0[1]), b2 = add_rn(w2[2], -w0[2]);
    n[0] = add_rn(mul_rn(a1, b2), -mul_rn(a2, b1));
    n[1] = add_rn(mul_rn(a2, b0), -mul_rn(a0, b2));
    n[2] = add_rn(mul_rn(a0, b1), -mul_rn(a1, b0));
}

// flat shading factor of a triangle (winding-defined world normal)
__device__ float shade_factor(const MeshXf& x, const float* M, const float* p0, const float* p1, const float* p2,
                              float3 light, float ambient, int two_sided) {
    float n[3];
    face_vector(x, M, p0, p1, p2, n);
    const float nl = add_rn(add_rn(mul_rn(n[0], light.x), mul_rn(n[1], light.y)), mul_rn(n[2], light.z));
    const float nn = add_rn(add_rn(mul_rn(n[0], n[0]), mul_rn(n[1], n[1])), mul_rn(n[2], n[2]));
    const float s = nn > 0.0f ? __fdiv_rn(nl, __builtin_sqrtf(nn)) : 0.0f;
    const float h = two_sided ? fabsf(s) : mul_rn(add_rn(s, 1.0f), 0.5f);
    return add_rn(ambient, mul_rn(add_rn(1.0f, -ambient), h));
}

// a mesh's triangles with S = 1 << LS samples per pixel and axis, as tile_bin_kernel sees them; the count pass of view 0
// also fills the flat shade table [sum T]
template <int LS>
struct MeshPrim : Args {
    float3 light;
    float ambient;
    int two_sided;
    typedef float CountOut;
    __device__ int status(int m) const { return xf[m].status; }
    __device__ int count(int m) const { return (int)(toff[m + 1] - toff[m]); }
    __device__ bool box(int m, int v, int t, int& px0, int& px1, int& py0, int& py1) const {
        Tri q;
        if (!tri_setup<LS>(*this, m, v, t, q)) return false;
        px0 = q.px0, px1 = q.px1, py0 = q.py0, py1 = q.py1;
        return true;
    }
    __device__ void counted(int m, int v, int t, float* shade) const {
        const float *p0, *p1, *p2;
        if (v == 0 && load_tri(*this, m, t, p0, p1, p2))
            shade[toff[m] - toff[0] + t] =
                shade_factor(xf[m], rots ? rots + (size_t)m * 9 : nullptr, p0, p1, p2, light, ambient, two_sided);
    }
};

// ---- smooth shading: vertex normals --------------------------------------------------------------------------------
// One thread per (table, vertex of the group): the face vectors of the vertex's corners (CSR: corner_off per vertex of
// the packed arrays, re-based by corner_off[0] as the mesh offsets are; corner_tri the local triangle ids, ascending)
// added in list order, then normalised.  Table v of a two-sided render turns every face vector towards view v's eye
// first; a one-sided render has one table.  No atomics: the result is a pure function of the inputs.
__global__ __launch_bounds__(RT) void vertex_normals_kernel(Args a, int n, long long total_verts,
                                                            const long long* __restrict__ corner_off,
                                                            const int* __restrict__ corner_tri, long long total_corners,
                                                            int two_sided, float* __restrict__ normals) {
    const long long gv = (long long)blockIdx.x * RT + threadIdx.x;
    const int tab = blockIdx.y;
    if (gv >= total_verts) return;
    int lo = 0, hi = n;                                          // the last mesh that starts at or before the vertex
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.voff[mid] - a.voff[0] <= gv) lo = mid;
        else hi = mid;
    }
    const int m = lo;
    float g[3] = {0.0f, 0.0f, 0.0f};
    const long long c0 = corner_off[gv] - corner_off[0], c1 = corner_off[gv + 1] - corner_off[0];
    // a mesh with status OK has its vertex and triangle ranges inside the arrays (normalise_kernel)
    if (a.xf[m].status == GV_RENDER_OK && gv >= a.voff[m] - a.voff[0] && gv < a.voff[m + 1] - a.voff[0] && c0 >= 0 &&
        c1 >= c0 && c1 <= total_corners) {
        const MeshXf x = a.xf[m];
        const float* M = a.rots ? a.rots + (size_t)m * 9 : nullptr;
        const float* fwd = a.cams + (size_t)tab * 9 + 6;
        bool first = true;
        for (long long c = c0; c < c1; ++c) {
            const float *p0, *p1, *p2;
            if (!load_tri(a, m, corner_tri[c], p0, p1, p2)) continue;
            float f[3];
            face_vector(x, M, p0, p1, p2, f);
            if (two_sided && dot3(fwd, f[0], f[1], f[2]) > 0.0f) {
                f[0] = -f[0];
                f[1] = -f[1];
                f[2] = -f[2];
            }
            for (int k = 0; k < 3; ++k) g[k] = first ? f[k] : add_rn(g[k], f[k]);
            first = false;
        }
        const float nn = add_rn(add_rn(mul_rn(g[0], g[0]), mul_rn(g[1], g[1])), mul_rn(g[2], g[2]));
        if (nn > 0.0f && nn < INFINITY) {
            const float r = __builtin_sqrtf(nn);
            for (int k = 0; k < 3; ++k) g[k] = __fdiv_rn(g[k], r);
        } else {
            g[0] = g[1] = g[2] = 0.0f;
        }
    }
    float* o = normals + ((long long)tab * total_verts + gv) * 3;
    o[0] = g[0];
    o[1] = g[1];
    o[2] = g[2];
}

// ---- raster + resolve ----------------------------------------------------------------------------------------------
struct LTri {                                                    // one setup in LDS (64 bytes)
    int x0, y0, x1, y1, x2, y2;
    unsigned z0, z1, z2;
    int bx, by;                                                  // px0 | px1 << 16, py0 | py1 << 16
    int id;                                                      // triangle id | owned-edge bits << 24
    long long area;
    double inv;                                                  // 1 / area, rounded once (S > 1 only)
};
static_assert(sizeof(LTri) == 64, "one setup is 64 bytes of LDS");

// the top-left rule.  Positive area in the y-down frame means clockwise on screen: a top edge runs left to right
// (dy == 0, dx > 0) and a left edge runs upwards (dy < 0); those edges own the pixel centres on them
__device__ __forceinline__ int owns(int ax, int ay, int bx, int by) {
    const int dx = bx - ax, dy = by - ay;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 1 : 0;
}
__device__ __forceinline__ long long edge(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// ---- smooth shading: per covered sample ------------------------------------------------------------------------------
struct Smooth : Reflect {                                        // the extra kernel argument of a smooth raster_kernel
    const float* normals;                                        // [tables, total_verts, 3], vertex_normals_kernel
    long long table_stride;                                      // vertices between two views' tables (0: one table)
};
struct SmoothTri {                                               // the recomputed setup of the last shaded triangle id
    int id, ok;
    Tri q;
    float area;
    float g[3][3];                                               // unit normals of vertices 0, 1, 2 after the swap
};

struct NoSmooth {};                                              // ... and of a flat one (its resolve keeps no state either)
template <bool SM> struct SmoothParam { typedef NoSmooth type; typedef NoSmooth state; };
template <> struct SmoothParam<true> { typedef Smooth type; typedef SmoothTri state; };

// colour cs of a covered sample at (SX, SY) whose winning triangle is id: the setup is recomputed (a pure function of
// the id) and kept while consecutive samples hold the same id; the three edge functions are the integers the raster
// loop had.  A sample whose interpolated normal has no finite positive length takes the triangle's flat factor.
template <int LS>
__device__ __forceinline__ void smooth_colour(const Args& a, const Smooth& sm, const float* __restrict__ shade, int m,
                                              int v, int id, int SX, int SY, float3 color, SmoothTri& st, float cs[3]) {
    const long long tb = a.toff[m] - a.toff[0];
    if (id != st.id) {
        st.id = id;
        st.ok = tri_setup<LS>(a, m, v, id, st.q) ? 1 : 0;
        if (st.ok) {                                             // (load_tri has checked the three indices)
            const int* ix = a.tris + (tb + id) * 3;
            const int i[3] = {ix[0], st.q.flip ? ix[2] : ix[1], st.q.flip ? ix[1] : ix[2]};
            const float* N = sm.normals + ((long long)v * sm.table_stride + (a.voff[m] - a.voff[0])) * 3;
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c) st.g[k][c] = N[(long long)i[k] * 3 + c];
            st.area = (float)st.q.area;
        }
    }
    if (st.ok) {
        const Tri& q = st.q;
        const float b0 = __fdiv_rn((float)edge(q.x1, q.y1, q.x2, q.y2, SX, SY), st.area);
        const float b1 = __fdiv_rn((float)edge(q.x2, q.y2, q.x0, q.y0, SX, SY), st.area);
        const float b2 = __fdiv_rn((float)edge(q.x0, q.y0, q.x1, q.y1, SX, SY), st.area);
        float n[3];
        for (int c = 0; c < 3; ++c)
            n[c] = add_rn(add_rn(mul_rn(b0, st.g[0][c]), mul_rn(b1, st.g[1][c])), mul_rn(b2, st.g[2][c]));
        if (reflect(sm, v, n, color, cs)) return;
    }
    scale_colour(color, shade[tb + id], cs);
}

// S = 1 << LS samples per pixel and axis.  The thread of pixel (px, py) holds the S * S keys of its samples (b rows,
// a columns, key b * S + a) in registers: every index into best[] below is a compile-time constant of a fully unrolled
// loop.  The edge functions are affine, so they are evaluated once per triangle at sample (0, 0) and stepped by the
// exact 64-bit increments d/dx = -(by - ay) * step, d/dy = (bx - ax) * step.
// SM: smooth shading; the resolve then shades every covered sample at its own position (smooth_colour) where the flat
// one reads its triangle's factor.
template <int OUT, int LS, bool SM>
__global__ __launch_bounds__(RT) void raster_kernel(Args a, const float* __restrict__ shade,
                                                    const int* __restrict__ tile_count,
                                                    const long long* __restrict__ tile_start,
                                                    const int* __restrict__ bins, long long cap, float3 color,
                                                    float3 background, void* __restrict__ out, int* __restrict__ face_id,
                                                    unsigned* __restrict__ depth, typename SmoothParam<SM>::type sm) {
    constexpr int S = 1 << LS, NS = S * S, STEP = 256 >> LS;
    __shared__ LTri s_tri[RT];
    const int T = a.tiles_x * a.tiles_y;
    const int tile = blockIdx.x, v = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    const long long img = (long long)m * a.V + v;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int px = tx * TS + (tid & (TS - 1)), py = ty * TS + (tid >> 4);
    const int PX = px * 256 + STEP / 2, PY = py * 256 + STEP / 2;   // sample (0, 0)
    u64 best[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) best[s] = BG_KEY;
    if (a.xf[m].status == GV_RENDER_OK) {
        const long long start = tile_start[img * T + tile];
        const long long end = min(start + (long long)tile_count[img * T + tile], cap);
        for (long long c0 = start; c0 < end; c0 += RT) {
            const int n = (int)min((long long)RT, end - c0);
            if (tid < n) {
                const int t = bins[c0 + tid];
                Tri q;
                LTri& L = s_tri[tid];
                if (tri_setup<LS>(a, m, v, t, q)) {
                    L.x0 = q.x0; L.y0 = q.y0; L.x1 = q.x1; L.y1 = q.y1; L.x2 = q.x2; L.y2 = q.y2;
                    L.z0 = q.z0; L.z1 = q.z1; L.z2 = q.z2;
                    L.bx = q.px0 | (q.px1 << 16);
                    L.by = q.py0 | (q.py1 << 16);
                    L.id = t | (owns(q.x1, q.y1, q.x2, q.y2) << 24) | (owns(q.x2, q.y2, q.x0, q.y0) << 25) |
                           (owns(q.x0, q.y0, q.x1, q.y1) << 26);
                    L.area = q.area;
                    if constexpr (LS > 0) L.inv = 1.0 / (double)q.area;      // area < 2^38: exact in a double
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
                if constexpr (LS == 0) {
                    const bool in = (e0 > 0 || (e0 == 0 && (L.id >> 24 & 1))) && (e1 > 0 || (e1 == 0 && (L.id >> 25 & 1))) &&
                                    (e2 > 0 || (e2 == 0 && (L.id >> 26 & 1)));
                    if (!in) continue;
                    const u64 num = (u64)e0 * L.z0 + (u64)e1 * L.z1 + (u64)e2 * L.z2;
                    // exact early-out: Z = num div area >= bestZ + 1 exactly when num >= (bestZ + 1) * area (< 2^62)
                    if (best[0] != BG_KEY && num >= ((best[0] >> 32) + 1) * (u64)L.area) continue;
                    const u64 Z = num / (u64)L.area;
                    const u64 key = (Z << 32) | (unsigned)(L.id & 0xffffff);
                    best[0] = key < best[0] ? key : best[0];
                } else {
                    const long long dx0 = -(long long)(L.y2 - L.y1) * STEP, dy0 = (long long)(L.x2 - L.x1) * STEP;
                    const long long dx1 = -(long long)(L.y0 - L.y2) * STEP, dy1 = (long long)(L.x0 - L.x2) * STEP;
                    const long long dx2 = -(long long)(L.y1 - L.y0) * STEP, dy2 = (long long)(L.x1 - L.x0) * STEP;
                    // an affine function has its maximum over the pixel's samples at a corner: below zero there, the
                    // edge excludes every sample
                    if (e0 + (S - 1) * (max(dx0, 0ll) + max(dy0, 0ll)) < 0 || e1 + (S - 1) * (max(dx1, 0ll) + max(dy1, 0ll)) < 0 ||
                        e2 + (S - 1) * (max(dx2, 0ll) + max(dy2, 0ll)) < 0)
                        continue;
                    const int o0 = L.id >> 24 & 1, o1 = L.id >> 25 & 1, o2 = L.id >> 26 & 1;
                    const unsigned z0 = L.z0, z1 = L.z1, z2 = L.z2, id = (unsigned)(L.id & 0xffffff);
                    const u64 area = (u64)L.area;
                    const double inv = L.inv;
#pragma unroll
                    for (int b = 0; b < S; ++b)
#pragma unroll
                        for (int c = 0; c < S; ++c) {
                            const long long f0 = e0 + b * dy0 + c * dx0, f1 = e1 + b * dy1 + c * dx1;
                            const long long f2 = e2 + b * dy2 + c * dx2;
                            const bool in = (f0 > 0 || (f0 == 0 && o0)) && (f1 > 0 || (f1 == 0 && o1)) &&
                                            (f2 > 0 || (f2 == 0 && o2));
                            if (!in) continue;
                            const u64 num = (u64)f0 * z0 + (u64)f1 * z1 + (u64)f2 * z2;
                            const u64 old = best[b * S + c];
                            // the same exact early-out, per sample
                            if (old != BG_KEY && num >= ((old >> 32) + 1) * area) continue;
                            // Z = num div area without the 64-bit division: num < 2^62 and 1 / area carry a relative
                            // error of 2^-53 each, their product one more, and Z < 2^24, so the estimate is within
                            // 2^-27 of num / area and its floor within 1 of Z; the exact remainder settles it
                            u64 Z = (u64)(unsigned)((double)num * inv);
                            const long long rem = (long long)(num - Z * area);
                            if (rem < 0) --Z;
                            else if ((u64)rem >= area) ++Z;
                            const u64 key = (Z << 32) | id;
                            best[b * S + c] = key < old ? key : old;
                        }
                }
            }
            __syncthreads();
        }
    }
    if (px >= a.W || py >= a.H) return;
    const size_t p = ((size_t)img * a.H + py) * a.W + px;
    // resolve: u8 per sample and channel, summed exactly; fp32 colours added in row-major sample order
    float acc[3] = {0.0f, 0.0f, 0.0f};
    unsigned sum[3] = {0u, 0u, 0u};
    [[maybe_unused]] typename SmoothParam<SM>::state st;
    if constexpr (SM) st.id = -1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float cs[3] = {background.x, background.y, background.z};
        if (best[s] != BG_KEY) {
            const int id = (int)(best[s] & 0xffffffffu);
            if constexpr (SM) {
                smooth_colour<LS>(a, sm, shade, m, v, id, PX + (s % S) * STEP, PY + (s / S) * STEP, color, st, cs);
            } else {
                scale_colour(color, shade[a.toff[m] - a.toff[0] + id], cs);
            }
        }
        if (face_id || depth) {
            const size_t q = ((size_t)img * (a.H << LS) + (py << LS) + s / S) * (a.W << LS) + (px << LS) + s % S;
            if (face_id) face_id[q] = best[s] == BG_KEY ? -1 : (int)(best[s] & 0xffffffffu);
            if (depth) depth[q] = best[s] == BG_KEY ? 0xFFFFFFFFu : (unsigned)(best[s] >> 32);
        }
        for (int c = 0; c < 3; ++c) {
            if (OUT == GV_RENDER_OUT_F32)
                acc[c] = s == 0 ? cs[c] : add_rn(acc[c], cs[c]);
            else
                sum[c] += to_u8(cs[c]);
        }
    }
    store_pixel<OUT, LS>(out, p, acc, sum);
}

// ---- host side -----------------------------------------------------------------------------------------------------
int64_t shade_bytes(int64_t total_tris) { return (total_tris > 0 ? total_tris : 1) * 4; }   // the flat shade table

TileWs ws_layout(int32_t n, int32_t v, int32_t h, int32_t w, int64_t total_tris) {
    return tile_ws_layout(n, v, h, w, shade_bytes(total_tris));
}

// the checks every entry point shares
int check_common(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
                 int32_t n, int64_t total_verts, int64_t total_tris, int32_t max_tris, const gv_render_desc* d,
                 const float* cameras, const void* workspace, int64_t workspace_bytes) {
    return check_tile_common(verts && vert_offsets && tris && tri_offsets, total_verts >= 0 && total_tris >= 0, n,
                             max_tris, d, cameras, workspace, workspace_bytes, shade_bytes(total_tris));
}

Args make_args(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
               const gv_render_desc* d, const float* cameras, const float* rotations, void* workspace, const TileWs& L) {
    Args a;
    static_cast<View&>(a) = make_view(d);
    a.verts = verts;
    a.voff = (const long long*)vert_offsets;
    a.tris = tris;
    a.toff = (const long long*)tri_offsets;
    a.cams = cameras;
    a.rots = rotations;
    a.xf = ws_at<const MeshXf>(workspace, L.xf);
    return a;
}

template <int LS>
MeshPrim<LS> make_prim(const Args& a, const gv_render_desc* d) {
    MeshPrim<LS> p;
    static_cast<Args&>(p) = a;
    p.light = make_float3(d->light[0], d->light[1], d->light[2]);
    p.ambient = d->ambient;
    p.two_sided = (d->flags & GV_RENDER_TWO_SIDED) ? 1 : 0;
    return p;
}

// samples per pixel and axis -> log2 (0, 1, 2); -1 for a power of two above 4 (GV_E_UNSUPPORTED once the shared checks
// have passed); false for anything else (GV_E_BADARG)
bool sample_shift(int32_t samples, int* ls) {
    if (samples <= 0 || (samples & (samples - 1))) return false;
    *ls = samples == 1 ? 0 : samples == 2 ? 1 : samples == 4 ? 2 : -1;
    return true;
}

int render_prepare(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
                   int32_t n, int64_t total_verts, int64_t total_tris, int32_t max_tris, const gv_render_desc* desc,
                   const float* cameras, const float* rotations, void* workspace, int64_t workspace_bytes,
                   int64_t* pair_total, int32_t* status, int ls, void* stream) {
    if (!pair_total || !status) return GV_E_BADARG;
    int rc = check_common(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc, cameras,
                          workspace, workspace_bytes);
    if (rc != GV_OK) return rc;
    if (ls < 0) return GV_E_UNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    const TileWs L = ws_layout(n, desc->num_views, desc->height, desc->width, total_tris);
    const Args a = make_args(verts, vert_offsets, tris, tri_offsets, desc, cameras, rotations, workspace, L);
    rc = start_prepare(st, a, n, workspace, L, verts, vert_offsets, tri_offsets, total_verts, total_tris, desc->fit, status);
    if (rc != GV_OK) return rc;
    rc = dispatch3<0, 1, 2>(ls, [&](auto LS) {
        return launch_bin<false>(st, make_prim<decltype(LS)::value>(a, desc), max_tris, n, workspace, L, nullptr, 0ll,
                                 ws_at<float>(workspace, L.extra));
    });
    return rc != GV_OK ? rc : finish_prepare(st, a, n, workspace, L, pair_total);
}

int64_t normal_tables(const gv_render_desc* d) { return (d->flags & GV_RENDER_TWO_SIDED) ? d->num_views : 1; }

int64_t normals_bytes(int64_t tables, int64_t total_verts) {
    return round_up((total_verts > 0 ? tables * total_verts : 1) * 12, 256);
}

struct SmoothCall {                                              // what gv_render_draw_smooth adds to a draw call
    const gv_render_shading* shading;
    const float *lights, *halfs, *normals;
    int64_t normals_size;
};

int render_draw(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
                int32_t n, int64_t total_verts, int64_t total_tris, int32_t max_tris, const gv_render_desc* desc,
                const float* cameras, const float* rotations, void* workspace, int64_t workspace_bytes, void* bins,
                int64_t bins_bytes, int64_t total, int32_t output, void* out, int32_t* face_id, uint32_t* depth, int ls,
                void* stream, const SmoothCall* sc = nullptr) {
    int squarings = 0;
    int rc = check_draw_args(bins, out, total, output);
    if (rc == GV_OK && sc) rc = sc->normals ? check_shading(sc->shading, sc->lights, sc->halfs, &squarings) : GV_E_BADARG;
    if (rc == GV_OK)
        rc = check_common(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc, cameras,
                          workspace, workspace_bytes);
    if (rc != GV_OK) return rc;
    if (ls < 0 || squarings < 0) return GV_E_UNSUPPORTED;
    if (sc && sc->normals_size < normals_bytes(normal_tables(desc), total_verts)) return GV_E_BADARG;
    rc = check_draw_buffers(bins, bins_bytes, total, output, out, face_id, depth);
    if (rc != GV_OK) return rc;
    if (sc && !gv_aligned16(sc->normals)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const TileWs L = ws_layout(n, desc->num_views, desc->height, desc->width, total_tris);
    const Args a = make_args(verts, vert_offsets, tris, tri_offsets, desc, cameras, rotations, workspace, L);
    const long long cap = bins_bytes / 4;
    const dim3 grid((unsigned)(a.tiles_x * a.tiles_y), (unsigned)desc->num_views, (unsigned)n);
    const float3 color = make_float3(desc->color[0], desc->color[1], desc->color[2]);
    const float3 bg = make_float3(desc->background[0], desc->background[1], desc->background[2]);
    Smooth smooth = {};
    if (sc) {
        static_cast<Reflect&>(smooth) = make_reflect(desc, sc->shading, squarings, sc->lights, sc->halfs);
        smooth.normals = sc->normals;
        smooth.table_stride = (desc->flags & GV_RENDER_TWO_SIDED) ? (long long)total_verts : 0ll;
    }
    // the one place that names the raster_kernel instantiations: S x shading x output
    auto raster = [&](auto LS, auto SM, auto sm) {
        dispatch_output(output, [&](auto OUT) {
            hipLaunchKernelGGL((raster_kernel<decltype(OUT)::value, decltype(LS)::value, decltype(SM)::value>), grid,
                               dim3(RT), 0, st, a, ws_at<const float>(workspace, L.extra),
                               ws_at<const int>(workspace, L.tile_count), ws_at<const long long>(workspace, L.tile_start),
                               static_cast<const int*>(bins), cap, color, bg, out, face_id, depth, sm);
        });
    };
    return dispatch3<0, 1, 2>(ls, [&](auto LS) {
        const int rc = launch_bin<true>(st, make_prim<decltype(LS)::value>(a, desc), max_tris, n, workspace, L,
                                        static_cast<int*>(bins), cap);
        if (rc != GV_OK) return rc;
        if (sc) raster(LS, std::true_type{}, smooth);
        else raster(LS, std::false_type{}, NoSmooth{});
        GV_LAUNCH_CHECK();
        return (int)GV_OK;
    });
}

int render_vertex_normals(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                          const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                          int32_t max_tris, const gv_render_desc* desc, const float* cameras, const float* rotations,
                          void* workspace, int64_t workspace_bytes, const int64_t* corner_offsets,
                          const int32_t* corner_tris, int64_t total_corners, float* normals, int64_t normals_size,
                          void* stream) {
    if (!corner_offsets || !corner_tris || !normals || total_corners < 0) return GV_E_BADARG;
    const int rc = check_common(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc,
                                cameras, workspace, workspace_bytes);
    if (rc != GV_OK) return rc;
    if (normals_size < normals_bytes(normal_tables(desc), total_verts)) return GV_E_BADARG;
    if (!gv_aligned16(normals)) return GV_E_ALIGN;
    if (total_verts == 0) return GV_OK;
    const TileWs L = ws_layout(n, desc->num_views, desc->height, desc->width, total_tris);
    const Args a = make_args(verts, vert_offsets, tris, tri_offsets, desc, cameras, rotations, workspace, L);
    const int64_t blocks = (total_verts + RT - 1) / RT;
    if (blocks > 0x7fffffffll) return GV_E_UNSUPPORTED;
    hipLaunchKernelGGL(vertex_normals_kernel, dim3((unsigned)blocks, (unsigned)normal_tables(desc)), dim3(RT), 0,
                       (hipStream_t)stream, a, n, (long long)total_verts, (const long long*)corner_offsets, corner_tris,
                       (long long)total_corners, (desc->flags & GV_RENDER_TWO_SIDED) ? 1 : 0, normals);
    GV_LAUNCH_CHECK();
    return GV_OK;
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
    return render_prepare(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc, cameras,
                          rotations, workspace, workspace_bytes, pair_total, status, 0, stream);
}

extern "C" int gv_render_draw(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                              const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                              int32_t max_tris, const gv_render_desc* desc, const float* cameras, const float* rotations,
                              void* workspace, int64_t workspace_bytes, void* bins, int64_t bins_bytes, int64_t total,
                              int32_t output, void* out, int32_t* face_id, uint32_t* depth, void* stream) {
    return render_draw(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc, cameras,
                       rotations, workspace, workspace_bytes, bins, bins_bytes, total, output, out, face_id, depth, 0,
                       stream);
}

// the same pair with S x S samples per pixel (S = samples: 1, 2 or 4)
extern "C" int gv_render_prepare_ss(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                                    const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                                    int32_t max_tris, const gv_render_desc* desc, const float* cameras,
                                    const float* rotations, void* workspace, int64_t workspace_bytes,
                                    int64_t* pair_total, int32_t* status, int32_t samples, void* stream) {
    int ls = 0;
    if (!sample_shift(samples, &ls)) return GV_E_BADARG;
    return render_prepare(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc, cameras,
                          rotations, workspace, workspace_bytes, pair_total, status, ls, stream);
}

extern "C" int gv_render_draw_ss(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                                 const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                                 int32_t max_tris, const gv_render_desc* desc, const float* cameras,
                                 const float* rotations, void* workspace, int64_t workspace_bytes, void* bins,
                                 int64_t bins_bytes, int64_t total, int32_t output, void* out, int32_t* face_id,
                                 uint32_t* depth, int32_t samples, void* stream) {
    int ls = 0;
    if (!sample_shift(samples, &ls)) return GV_E_BADARG;
    return render_draw(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc, cameras,
                       rotations, workspace, workspace_bytes, bins, bins_bytes, total, output, out, face_id, depth, ls,
                       stream);
}

// ---- smooth shading (contract: include/gvcnn_hip.h, "smooth shading") -------------------------------------------------
extern "C" int64_t gv_render_normals_bytes(int32_t num_views, int32_t flags, int64_t total_verts) {
    if (num_views <= 0 || total_verts < 0 || (flags & ~(GV_RENDER_PERSPECTIVE | GV_RENDER_TWO_SIDED))) return GV_E_BADARG;
    if (num_views > 64) return GV_E_UNSUPPORTED;
    return normals_bytes((flags & GV_RENDER_TWO_SIDED) ? num_views : 1, total_verts);
}

extern "C" int gv_render_vertex_normals(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                                        const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                                        int32_t max_tris, const gv_render_desc* desc, const float* cameras,
                                        const float* rotations, void* workspace, int64_t workspace_bytes,
                                        const int64_t* corner_offsets, const int32_t* corner_tris, int64_t total_corners,
                                        float* normals, int64_t normals_bytes, void* stream) {
    return render_vertex_normals(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc,
                                 cameras, rotations, workspace, workspace_bytes, corner_offsets, corner_tris,
                                 total_corners, normals, normals_bytes, stream);
}

extern "C" int gv_render_draw_smooth(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                                     const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                                     int32_t max_tris, const gv_render_desc* desc, const float* cameras,
                                     const float* rotations, void* workspace, int64_t workspace_bytes, void* bins,
                                     int64_t bins_bytes, int64_t total, int32_t output, void* out, int32_t* face_id,
                                     uint32_t* depth, int32_t samples, const gv_render_shading* shading,
                                     const float* lights, const float* halfs, const float* normals,
                                     int64_t normals_size, void* stream) {
    int ls = 0;
    if (!sample_shift(samples, &ls)) return GV_E_BADARG;
    const SmoothCall sc = {shading, lights, halfs, normals, normals_size};
    return render_draw(verts, vert_offsets, tris, tri_offsets, n, total_verts, total_tris, max_tris, desc, cameras,
                       rotations, workspace, workspace_bytes, bins, bins_bytes, total, output, out, face_id, depth, ls,
                       stream, &sc);
}
