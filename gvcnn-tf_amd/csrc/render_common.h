// What the two renderers share (render.hip: meshes in; render_points.hip: points in): the fp32 discipline, the per-shape
// normalisation, the camera transform / projection / snap, the reflection model, the pixel store, and the scans that turn
// tile counts into tile list starts (the tile binning built on them is in render_tiles.h).
// Everything sits in the including file's unnamed namespace: each translation unit has its own copy of the kernels.
#pragma once
#include <math.h>

#include "gv_common.h"

// Every fp32 step rounds on its own, so numpy float32 reproduces it.  hipcc contracts a * b + c into one FMA by default,
// the header's __fmul_rn / __fadd_rn included (they are plain operators there): the renderers turn contraction off and
// spell each step with the helpers below.  The one fused step, the quantised output, is an explicit fmaf.  Division is
// IEEE (HIP's default); the square root is __builtin_sqrtf, correctly rounded (__fsqrt_rn is the native approximation).
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

typedef unsigned long long u64;

constexpr int TS = 16;                                           // tile edge in pixels
constexpr int RT = 256;                                          // threads of every kernel but the scans
constexpr int SCAN_T = 1024;                                     // threads of the scan kernels
constexpr int CHUNK = 1024;                                      // triangles (points) per binning workgroup and pass
constexpr int MAX_SIDE = 512;
constexpr int MAX_TILES = (MAX_SIDE / TS) * (MAX_SIDE / TS);     // 1024
constexpr int MAX_TRIS = 1 << 24;                                // ... and points of a cloud: the id's 24 bits
// snapped coordinates are clamped to +-2^18 (+-1024 pixels; a vertex of the unit sphere lands inside the image): a
// triangle then spans at most 2^19 per axis, twice its area is below 2^38 and e0*Z0 + e1*Z1 + e2*Z2 <= area * (2^24-1)
// stays below 2^62, whatever the input
constexpr float SNAP_LIM = 262144.0f;
constexpr u64 BG_KEY = ~0ull;

struct MeshXf {                                                  // per mesh, written by normalise_kernel
    float cx, cy, cz, scale;
    int status, pad0, pad1, pad2;
};

struct View {                                                    // what project needs: the head of both renderers' Args
    int V, H, W, tiles_x, tiles_y, persp;
    float k, D, da, db, cxs, cys;                                // projection constants, image centre
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
__device__ __forceinline__ void project(const View& a, const float* C, const float w[3], int& X, int& Y, unsigned& Z) {
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

// the projection half of a descriptor
inline View make_view(const gv_render_desc* d) {
    View a;
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

// ---- reflection model (contract: include/gvcnn_hip.h, "smooth shading") ---------------------------------------------
struct Reflect {                                                 // the head of both renderers' shading arguments
    const float* lights;                                         // [V, 3] unit light of every view
    const float* halfs;                                          // [V, 3] unit half-vector of every view
    float specular, ambient;
    int squarings, lambert, two_sided;                           // squarings = log2(shininess)
};

// colour cs of a surface with (unnormalised) normal n in view v.  False, cs untouched, when n has no finite positive
// length: the caller then shades by its own fallback.
__device__ __forceinline__ bool reflect(const Reflect& r, int v, const float n[3], float3 color, float cs[3]) {
    const float nn = add_rn(add_rn(mul_rn(n[0], n[0]), mul_rn(n[1], n[1])), mul_rn(n[2], n[2]));
    if (!(nn > 0.0f && nn < INFINITY)) return false;
    const float len = __builtin_sqrtf(nn);
    const float s = __fdiv_rn(dot3(r.lights + v * 3, n[0], n[1], n[2]), len);
    const float h = r.two_sided ? fabsf(s) : r.lambert ? fmaxf(s, 0.0f) : mul_rn(add_rn(s, 1.0f), 0.5f);
    const float f = add_rn(r.ambient, mul_rn(add_rn(1.0f, -r.ambient), h));
    float sp = 0.0f;
    if (r.specular > 0.0f) {                                     // (uniform; specular = 0 adds exactly nothing)
        const float t = __fdiv_rn(dot3(r.halfs + v * 3, n[0], n[1], n[2]), len);
        float p = r.two_sided ? fabsf(t) : fmaxf(t, 0.0f);
        for (int k = 0; k < r.squarings; ++k) p = mul_rn(p, p);
        sp = mul_rn(r.specular, p);
    }
    cs[0] = fminf(add_rn(mul_rn(color.x, f), sp), 1.0f);
    cs[1] = fminf(add_rn(mul_rn(color.y, f), sp), 1.0f);
    cs[2] = fminf(add_rn(mul_rn(color.z, f), sp), 1.0f);
    return true;
}

// the unlit colour: one factor for the three channels (the flat table's entry, the splatter's depth factor)
__device__ __forceinline__ void scale_colour(float3 color, float f, float cs[3]) {
    cs[0] = mul_rn(color.x, f);
    cs[1] = mul_rn(color.y, f);
    cs[2] = mul_rn(color.z, f);
}

// ---- pixel store ---------------------------------------------------------------------------------------------------
// the byte a PNG of the render holds for a colour channel in [0, 1]
__device__ __forceinline__ unsigned to_u8(float c) {
    return (unsigned)(unsigned char)fminf(fmaxf(floorf(add_rn(mul_rn(c, 255.0f), 0.5f)), 0.0f), 255.0f);
}

// pixel p of `out` from its NS = 1 << 2 * LS samples: acc holds their fp32 colours added in row-major sample order
// (read by OUT_F32 alone), sum the exact sum of their to_u8 bytes (read by the other two modes)
template <int OUT, int LS>
__device__ __forceinline__ void store_pixel(void* out, size_t p, const float acc[3], const unsigned sum[3]) {
    constexpr int NS = 1 << (2 * LS);
    if (OUT == GV_RENDER_OUT_F32) {
        float* o = static_cast<float*>(out) + p * 3;
        for (int c = 0; c < 3; ++c) o[c] = add_rn(LS ? mul_rn(acc[c], 1.0f / NS) : acc[c], -0.5f);
    } else {
        unsigned char u[3];
        for (int c = 0; c < 3; ++c) u[c] = (unsigned char)((sum[c] + NS / 2) >> (2 * LS));
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

// ---- normalisation -------------------------------------------------------------------------------------------------
// (a point cloud passes its point offsets as both offset arrays: a shape without elements is EMPTY either way)
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

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

inline bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the descriptor checks every entry point of both renderers shares
inline int check_desc(const gv_render_desc* d) {
    if (d->height <= 0 || d->width <= 0 || d->num_views <= 0 || (d->flags & ~(GV_RENDER_PERSPECTIVE | GV_RENDER_TWO_SIDED)))
        return GV_E_BADARG;
    if (!(d->fit > 0.0f && d->fit <= 1.0f) || !(d->ambient >= 0.0f && d->ambient <= 1.0f)) return GV_E_BADARG;
    if (!(d->proj_scale > 0.0f) || !isfinite(d->proj_scale)) return GV_E_BADARG;
    if ((d->flags & GV_RENDER_PERSPECTIVE) &&
        !(d->persp_dist > 1.0f && isfinite(d->persp_dist) && isfinite(d->depth_a) && isfinite(d->depth_b)))
        return GV_E_BADARG;
    if (!finite3(d->light) || !finite3(d->color) || !finite3(d->background)) return GV_E_BADARG;
    return GV_OK;
}

// shininess -> the number of squarings; -1 for a power of two above 128 (GV_E_UNSUPPORTED once the shared checks have
// passed); false for anything else (GV_E_BADARG)
inline bool shininess_shift(int32_t shininess, int* k) {
    if (shininess <= 0 || (shininess & (shininess - 1))) return false;
    *k = -1;
    for (int i = 0; i <= 7; ++i)
        if (shininess == 1 << i) *k = i;
    return true;
}

// the reflection arguments of a shaded draw: GV_E_BADARG or GV_OK, with *squarings as shininess_shift leaves it
inline int check_shading(const gv_render_shading* s, const float* lights, const float* halfs, int* squarings) {
    if (!s || !lights || !halfs) return GV_E_BADARG;
    if ((s->flags & ~GV_RENDER_LAMBERT) || !(s->specular >= 0.0f && s->specular <= 1.0f)) return GV_E_BADARG;
    return shininess_shift(s->shininess, squarings) ? GV_OK : GV_E_BADARG;
}

// s: null for a draw that reflects nothing (the splatter's "depth" shading reads ambient alone)
inline Reflect make_reflect(const gv_render_desc* d, const gv_render_shading* s, int squarings, const float* lights,
                            const float* halfs) {
    return {lights, halfs, s ? s->specular : 0.0f, d->ambient, squarings, (s && (s->flags & GV_RENDER_LAMBERT)) ? 1 : 0,
            (d->flags & GV_RENDER_TWO_SIDED) ? 1 : 0};
}

}  // namespace
