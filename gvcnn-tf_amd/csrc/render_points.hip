// render_points.hip — multi-view point splatter: a batch of point clouds -> the backbone's input views [N, V, H, W, 3]
// on the device (the contract is in include/gvcnn_hip.h, "points in").  The launches mirror render.hip's:
//
//   gv_points_prepare   normalise_kernel    (render_common.h) one workgroup per cloud: c, r, scale = fit / r, status.
//                       pbin_kernel<false>  grid (point chunks, view, cloud): every thread sets up its points for the view
//                                           (world position, project, snap, radius, pixel-centre box of the disc) and
//                                           counts them into the image's 16x16-pixel tiles with LDS atomics; the workgroup
//                                           then adds its nonzero tile counts to the global counters (one atomic per
//                                           workgroup and tile, never per fragment).
//                       scan_images_kernel, scan_tiles_kernel  (render_common.h) tile list starts.
//   gv_points_draw      pbin_kernel<true>   the same setup and LDS counts; each workgroup reserves a run of every tile
//                                           list it feeds and places its point ids there through LDS cursors.  List order
//                                           is scheduling dependent; nothing downstream depends on it.
//                       splat_kernel        one workgroup per tile (256 threads = 16 x 16 pixels): the tile's list is
//                                           streamed through LDS 256 setups at a time; each pixel tests its centre against
//                                           the disc in int64, keeps the smallest key (Z << 32 | point id) in a register,
//                                           shades the winner and writes its outputs once.
//
// The splat setup is a pure function of (cloud, view, point), recomputed where needed (count, scatter, raster), so the
// bins hold 4-byte ids only.  A disc reaches at most R_MAX = 32 pixels from its centre: at most 6 x 6 tiles.
#include <math.h>

#include "render_common.h"

#pragma clang fp contract(off)

namespace {

constexpr float R_MIN = 1.0f;                                    // radius bounds in 1/256 pixel
constexpr float R_MAX = 8192.0f;                                 // 32 pixels

struct PArgs : View {                                            // everything a splat setup needs
    const float* pts;
    const long long* poff;
    const float* cams;                                           // [V, 3, 3]
    const float* rots;                                           // [N, 3, 3] or null
    const MeshXf* xf;
    const float* radius;                                         // [N], normalised units (the workspace's copy)
};

struct Splat {
    int X, Y;                                                    // snapped centre
    unsigned Z;
    int R;                                                       // radius in 1/256 pixel, 1 .. 8192
    int px0, px1, py0, py1;                                      // pixels whose centres lie in the disc's box
};

// setup of point i of cloud m in view v: false when the id is out of range (a tile-list slot a matching prepare never
// wrote), the world position is not finite, or the disc's box holds no pixel centre of the image
__device__ bool splat_setup(const PArgs& a, int m, int v, int i, Splat& s) {
    if (i < 0 || i >= a.poff[m + 1] - a.poff[m]) return false;
    const float* p = a.pts + (a.poff[m] - a.poff[0] + i) * 3;
    const MeshXf x = a.xf[m];
    const float* M = a.rots ? a.rots + (size_t)m * 9 : nullptr;
    const float* C = a.cams + (size_t)v * 9;
    float w[3];
    world(x, M, p, w);
    if (!(isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]))) return false;
    project(a, C, w, s.X, s.Y, s.Z);
    float r = mul_rn(a.radius[m], a.k);
    if (a.persp) r = __fdiv_rn(r, add_rn(dot3(C + 6, w[0], w[1], w[2]), a.D));   // project's z, the same steps
    s.R = (int)rintf(fminf(fmaxf(mul_rn(r, 256.0f), R_MIN), R_MAX));
    // centres 256 i + 128 inside [X - R, X + R]
    s.px0 = max((s.X - s.R + 127) >> 8, 0);
    s.px1 = min((s.X + s.R - 128) >> 8, a.W - 1);
    s.py0 = max((s.Y - s.R + 127) >> 8, 0);
    s.py1 = min((s.Y + s.R - 128) >> 8, a.H - 1);
    return s.px0 <= s.px1 && s.py0 <= s.py1;
}

// ---- binning: count (SCATTER = false) and scatter (SCATTER = true) --------------------------------------------------
// gridDim.x is a hint: the loop strides over every chunk of the cloud whatever the grid holds.
template <bool SCATTER>
__global__ __launch_bounds__(RT) void pbin_kernel(PArgs a, int* __restrict__ tile_count, long long* __restrict__ image_total,
                                                  const long long* __restrict__ tile_start, int* __restrict__ tile_fill,
                                                  int* __restrict__ bins, long long cap) {
    __shared__ int s_cnt[MAX_TILES];
    __shared__ long long s_base[SCATTER ? MAX_TILES : 1];
    __shared__ long long s_sum[RT / 64];
    const int m = blockIdx.z, v = blockIdx.y, tid = threadIdx.x;
    if (a.xf[m].status != GV_RENDER_OK) return;                  // (uniform)
    const int np = (int)(a.poff[m + 1] - a.poff[m]);             // <= 2^24 (status OK)
    const int T = a.tiles_x * a.tiles_y;
    const long long img = (long long)m * a.V + v;
    const long long stride = (long long)gridDim.x * CHUNK;
    for (long long c0 = (long long)blockIdx.x * CHUNK; c0 < np; c0 += stride) {
        const int lo = (int)c0, hi = min(lo + CHUNK, np);
        for (int i = tid; i < T; i += RT) s_cnt[i] = 0;
        __syncthreads();
        for (int t = lo + tid; t < hi; t += RT) {
            Splat q;
            if (!splat_setup(a, m, v, t, q)) continue;
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
            for (int t = lo + tid; t < hi; t += RT) {
                Splat q;
                if (!splat_setup(a, m, v, t, q)) continue;
                for (int ty = q.py0 >> 4; ty <= q.py1 >> 4; ++ty)
                    for (int tx = q.px0 >> 4; tx <= q.px1 >> 4; ++tx) {
                        const int i = ty * a.tiles_x + tx;
                        const long long pos = s_base[i] + atomicAdd(&s_cnt[i], 1);
                        if (pos >= 0 && pos < cap) bins[pos] = t;
                    }
            }
        }
        __syncthreads();                                         // s_cnt / s_sum are reused by the next chunk
    }
}

// ---- raster + shade ------------------------------------------------------------------------------------------------
struct LSplat {                                                  // one setup in LDS (20 bytes)
    int X, Y;
    unsigned Z;
    int R;                                                       // -1: a rejected slot (no |dx| is <= -1)
    int id;
};

struct PShade {
    const float* normals;                                        // [sum P, 3] per point, or null: "depth" shading
    const float* lights;                                         // [V, 3] unit light of every view
    const float* halfs;                                          // [V, 3] unit half-vector of every view
    float specular, ambient;
    int squarings, lambert, two_sided;                           // squarings = log2(shininess)
};

// colour of the pixel whose winning splat is point id at depth Z
__device__ __forceinline__ void splat_colour(const PArgs& a, const PShade& sh, int m, int v, int id, unsigned Z,
                                             float3 color, float cs[3]) {
    if (sh.normals) {                                            // (uniform)
        const float* g = sh.normals + (a.poff[m] - a.poff[0] + id) * 3;
        float n[3] = {g[0], g[1], g[2]};
        if (a.rots) {
            const float* M = a.rots + (size_t)m * 9;
            const float n0 = dot3(M, g[0], g[1], g[2]), n1 = dot3(M + 3, g[0], g[1], g[2]);
            const float n2 = dot3(M + 6, g[0], g[1], g[2]);
            n[0] = n0;
            n[1] = n1;
            n[2] = n2;
        }
        const float nn = add_rn(add_rn(mul_rn(n[0], n[0]), mul_rn(n[1], n[1])), mul_rn(n[2], n[2]));
        if (nn > 0.0f && nn < INFINITY) {
            const float len = __builtin_sqrtf(nn);
            const float s = __fdiv_rn(dot3(sh.lights + v * 3, n[0], n[1], n[2]), len);
            const float h = sh.two_sided ? fabsf(s) : sh.lambert ? fmaxf(s, 0.0f) : mul_rn(add_rn(s, 1.0f), 0.5f);
            const float f = add_rn(sh.ambient, mul_rn(add_rn(1.0f, -sh.ambient), h));
            float sp = 0.0f;
            if (sh.specular > 0.0f) {                            // (uniform; specular = 0 adds exactly nothing)
                const float t = __fdiv_rn(dot3(sh.halfs + v * 3, n[0], n[1], n[2]), len);
                float p = sh.two_sided ? fabsf(t) : fmaxf(t, 0.0f);
                for (int k = 0; k < sh.squarings; ++k) p = mul_rn(p, p);
                sp = mul_rn(sh.specular, p);
            }
            cs[0] = fminf(add_rn(mul_rn(color.x, f), sp), 1.0f);
            cs[1] = fminf(add_rn(mul_rn(color.y, f), sp), 1.0f);
            cs[2] = fminf(add_rn(mul_rn(color.z, f), sp), 1.0f);
            return;
        }
    }
    const float t = __fdiv_rn((float)Z, 16777215.0f);            // Z < 2^24: exact in fp32
    const float f = add_rn(sh.ambient, mul_rn(add_rn(1.0f, -sh.ambient), add_rn(1.0f, -t)));
    cs[0] = mul_rn(color.x, f);
    cs[1] = mul_rn(color.y, f);
    cs[2] = mul_rn(color.z, f);
}

template <int OUT>
__global__ __launch_bounds__(RT) void splat_kernel(PArgs a, PShade sh, const int* __restrict__ tile_count,
                                                   const long long* __restrict__ tile_start,
                                                   const int* __restrict__ bins, long long cap, float3 color,
                                                   float3 background, void* __restrict__ out, int* __restrict__ point_id,
                                                   unsigned* __restrict__ depth) {
    __shared__ LSplat s_sp[RT];
    const int T = a.tiles_x * a.tiles_y;
    const int tile = blockIdx.x, v = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    const long long img = (long long)m * a.V + v;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int px = tx * TS + (tid & (TS - 1)), py = ty * TS + (tid >> 4);
    const int PX = px * 256 + 128, PY = py * 256 + 128;
    u64 best = BG_KEY;
    if (a.xf[m].status == GV_RENDER_OK) {
        const long long start = max(tile_start[img * T + tile], 0ll);
        const long long end = min(start + (long long)tile_count[img * T + tile], cap);
        for (long long c0 = start; c0 < end; c0 += RT) {
            const int n = (int)min((long long)RT, end - c0);
            if (tid < n) {
                const int t = bins[c0 + tid];
                Splat q;
                LSplat& L = s_sp[tid];
                if (splat_setup(a, m, v, t, q)) {
                    L.X = q.X;
                    L.Y = q.Y;
                    L.Z = q.Z;
                    L.R = q.R;
                    L.id = t;
                } else {
                    L.X = L.Y = 0;
                    L.Z = 0u;
                    L.R = -1;
                    L.id = 0;
                }
            }
            __syncthreads();
            for (int i = 0; i < n; ++i) {
                const LSplat& L = s_sp[i];
                const int dx = PX - L.X, dy = PY - L.Y;          // |.| < 2^18 + 2^17
                if (abs(dx) > L.R || abs(dy) > L.R) continue;
                if ((long long)dx * dx + (long long)dy * dy > (long long)L.R * L.R) continue;
                const u64 key = ((u64)L.Z << 32) | (unsigned)L.id;
                best = key < best ? key : best;
            }
            __syncthreads();
        }
    }
    if (px >= a.W || py >= a.H) return;
    const size_t p = ((size_t)img * a.H + py) * a.W + px;
    float cs[3] = {background.x, background.y, background.z};
    if (best != BG_KEY) splat_colour(a, sh, m, v, (int)(best & 0xffffffffu), (unsigned)(best >> 32), color, cs);
    if (point_id) point_id[p] = best == BG_KEY ? -1 : (int)(best & 0xffffffffu);
    if (depth) depth[p] = best == BG_KEY ? 0xFFFFFFFFu : (unsigned)(best >> 32);
    if (OUT == GV_RENDER_OUT_F32) {
        float* o = static_cast<float*>(out) + p * 3;
        for (int c = 0; c < 3; ++c) o[c] = add_rn(cs[c], -0.5f);
    } else {
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
struct PWsLayout {
    int64_t xf, radius, tile_count, tile_fill, tile_start, image_total, image_base, bytes;
};

PWsLayout pws_layout(int32_t n, int32_t v, int32_t h, int32_t w) {
    const int64_t T = (int64_t)((h + TS - 1) / TS) * ((w + TS - 1) / TS);
    const int64_t nimg = (int64_t)n * v;
    PWsLayout L;
    int64_t o = 0;
    L.xf = o;          o += round_up((int64_t)n * sizeof(MeshXf), 256);
    L.radius = o;      o += round_up((int64_t)n * 4, 256);
    L.tile_count = o;  o += round_up(nimg * T * 4, 256);
    L.tile_fill = o;   o += round_up(nimg * T * 4, 256);
    L.tile_start = o;  o += round_up(nimg * T * 8, 256);
    L.image_total = o; o += round_up(nimg * 8, 256);
    L.image_base = o;  o += round_up(nimg * 8, 256);
    L.bytes = o;
    return L;
}

// the checks both entry points share
int pcheck_common(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points, int32_t max_points,
                  const gv_render_desc* d, const float* cameras, const void* workspace, int64_t workspace_bytes) {
    if (!points || !point_offsets || !d || !cameras || !workspace) return GV_E_BADARG;
    if (n <= 0 || total_points < 0 || max_points < 0) return GV_E_BADARG;
    if (check_desc(d) != GV_OK) return GV_E_BADARG;
    if (d->height > MAX_SIDE || d->width > MAX_SIDE || d->num_views > 64 || n > 65535 || max_points > MAX_TRIS)
        return GV_E_UNSUPPORTED;
    if (workspace_bytes < pws_layout(n, d->num_views, d->height, d->width).bytes) return GV_E_BADARG;
    if (!gv_aligned16(workspace)) return GV_E_ALIGN;
    return GV_OK;
}

PArgs make_pargs(const float* points, const int64_t* point_offsets, const gv_render_desc* d, const float* cameras,
                 const float* rotations, const MeshXf* xf, const float* radius) {
    PArgs a;
    static_cast<View&>(a) = make_view(d);
    a.pts = points;
    a.poff = (const long long*)point_offsets;
    a.cams = cameras;
    a.rots = rotations;
    a.xf = xf;
    a.radius = radius;
    return a;
}

dim3 pbin_grid(int32_t max_points, int32_t v, int32_t n) {
    const int chunks = max_points > 0 ? (max_points + CHUNK - 1) / CHUNK : 1;
    return dim3((unsigned)chunks, (unsigned)v, (unsigned)n);
}

}  // namespace

extern "C" int64_t gv_points_workspace_bytes(int32_t n, int32_t num_views, int32_t height, int32_t width) {
    if (n <= 0 || num_views <= 0 || height <= 0 || width <= 0) return GV_E_BADARG;
    if (height > MAX_SIDE || width > MAX_SIDE || num_views > 64 || n > 65535) return GV_E_UNSUPPORTED;
    return pws_layout(n, num_views, height, width).bytes;
}

extern "C" int gv_points_prepare(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                                 int32_t max_points, const float* radius, const gv_render_desc* desc,
                                 const float* cameras, const float* rotations, void* workspace, int64_t workspace_bytes,
                                 int64_t* pair_total, int32_t* status, void* stream) {
    if (!pair_total || !status || !radius) return GV_E_BADARG;
    const int rc = pcheck_common(points, point_offsets, n, total_points, max_points, desc, cameras, workspace,
                                 workspace_bytes);
    if (rc != GV_OK) return rc;
    for (int32_t i = 0; i < n; ++i)                              // radius is host memory
        if (!(radius[i] > 0.0f) || !isfinite(radius[i])) return GV_E_BADARG;
    const hipStream_t st = (hipStream_t)stream;
    const PWsLayout L = pws_layout(n, desc->num_views, desc->height, desc->width);
    char* ws = static_cast<char*>(workspace);
    MeshXf* xf = reinterpret_cast<MeshXf*>(ws + L.xf);
    const PArgs a = make_pargs(points, point_offsets, desc, cameras, rotations, xf,
                               reinterpret_cast<const float*>(ws + L.radius));
    const int T = a.tiles_x * a.tiles_y;
    const long long nimg = (long long)n * desc->num_views;
    GV_HIP_CHECK(hipMemcpyAsync(ws + L.radius, radius, (size_t)n * 4, hipMemcpyHostToDevice, st));
    GV_HIP_CHECK(hipMemsetAsync(ws + L.tile_count, 0, (size_t)nimg * T * 4, st));
    GV_HIP_CHECK(hipMemsetAsync(ws + L.image_total, 0, (size_t)nimg * 8, st));
    hipLaunchKernelGGL(normalise_kernel, dim3(n), dim3(RT), 0, st, points, (const long long*)point_offsets,
                       (const long long*)point_offsets, (long long)total_points, (long long)total_points, desc->fit, xf,
                       status);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(pbin_kernel<false>, pbin_grid(max_points, desc->num_views, n), dim3(RT), 0, st, a,
                       reinterpret_cast<int*>(ws + L.tile_count), reinterpret_cast<long long*>(ws + L.image_total),
                       nullptr, nullptr, nullptr, 0ll);
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

extern "C" int gv_points_draw(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                              int32_t max_points, const gv_render_desc* desc, const float* cameras,
                              const float* rotations, void* workspace, int64_t workspace_bytes, void* bins,
                              int64_t bins_bytes, int64_t total, int32_t output, void* out, int32_t* point_id,
                              uint32_t* depth, const float* normals, const gv_render_shading* shading,
                              const float* lights, const float* halfs, void* stream) {
    if (!bins || !out || total < 0) return GV_E_BADARG;
    if (output != GV_RENDER_OUT_F32_QUANTIZED && output != GV_RENDER_OUT_F32 && output != GV_RENDER_OUT_U8)
        return GV_E_BADARG;
    int squarings = 0;
    if (normals) {                                               // "normal" shading
        if (!shading || !lights || !halfs) return GV_E_BADARG;
        if ((shading->flags & ~GV_RENDER_LAMBERT) || !(shading->specular >= 0.0f && shading->specular <= 1.0f))
            return GV_E_BADARG;
        if (!shininess_shift(shading->shininess, &squarings)) return GV_E_BADARG;
    }
    const int rc = pcheck_common(points, point_offsets, n, total_points, max_points, desc, cameras, workspace,
                                 workspace_bytes);
    if (rc != GV_OK) return rc;
    if (squarings < 0) return GV_E_UNSUPPORTED;
    if (bins_bytes < gv_render_bins_bytes(total)) return GV_E_BADARG;
    if (!gv_aligned16(bins) || (output != GV_RENDER_OUT_U8 && ((uintptr_t)out & 3u))) return GV_E_ALIGN;
    if (((uintptr_t)point_id & 3u) || ((uintptr_t)depth & 3u) || ((uintptr_t)normals & 3u)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const PWsLayout L = pws_layout(n, desc->num_views, desc->height, desc->width);
    char* ws = static_cast<char*>(workspace);
    const PArgs a = make_pargs(points, point_offsets, desc, cameras, rotations, reinterpret_cast<const MeshXf*>(ws + L.xf),
                               reinterpret_cast<const float*>(ws + L.radius));
    const int T = a.tiles_x * a.tiles_y;
    const long long nimg = (long long)n * desc->num_views;
    const long long cap = bins_bytes / 4;
    const int* tc = reinterpret_cast<const int*>(ws + L.tile_count);
    const long long* ts = reinterpret_cast<const long long*>(ws + L.tile_start);
    int* b = static_cast<int*>(bins);
    GV_HIP_CHECK(hipMemsetAsync(ws + L.tile_fill, 0, (size_t)nimg * T * 4, st));
    hipLaunchKernelGGL(pbin_kernel<true>, pbin_grid(max_points, desc->num_views, n), dim3(RT), 0, st, a, nullptr, nullptr,
                       ts, reinterpret_cast<int*>(ws + L.tile_fill), b, cap);
    GV_LAUNCH_CHECK();
    const bool two = (desc->flags & GV_RENDER_TWO_SIDED) != 0;
    const PShade sh = {normals, lights, halfs, normals ? shading->specular : 0.0f, desc->ambient, squarings,
                       (normals && (shading->flags & GV_RENDER_LAMBERT)) ? 1 : 0, two ? 1 : 0};
    const float3 color = make_float3(desc->color[0], desc->color[1], desc->color[2]);
    const float3 bg = make_float3(desc->background[0], desc->background[1], desc->background[2]);
    const dim3 grid((unsigned)T, (unsigned)desc->num_views, (unsigned)n);
    const int* cb = b;
    if (output == GV_RENDER_OUT_F32_QUANTIZED)
        hipLaunchKernelGGL(splat_kernel<GV_RENDER_OUT_F32_QUANTIZED>, grid, dim3(RT), 0, st, a, sh, tc, ts, cb, cap, color,
                           bg, out, point_id, depth);
    else if (output == GV_RENDER_OUT_F32)
        hipLaunchKernelGGL(splat_kernel<GV_RENDER_OUT_F32>, grid, dim3(RT), 0, st, a, sh, tc, ts, cb, cap, color, bg, out,
                           point_id, depth);
    else
        hipLaunchKernelGGL(splat_kernel<GV_RENDER_OUT_U8>, grid, dim3(RT), 0, st, a, sh, tc, ts, cb, cap, color, bg, out,
                           point_id, depth);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
