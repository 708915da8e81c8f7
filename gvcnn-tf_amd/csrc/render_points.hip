// render_points.hip — multi-view point splatter: a batch of point clouds -> the backbone's input views [N, V, H, W, 3]
// on the device (the contract is in include/gvcnn_hip.h, "points in").  The launches are render.hip's with a splat for
// a triangle:
//
//   gv_points_prepare   normalise_kernel        (render_common.h) one workgroup per cloud: c, r, scale = fit / r, status.
//                       tile_bin_kernel<false>  (render_tiles.h, over PointPrim) counts every point's disc (world position,
//                                               project, snap, radius, pixel-centre box) into the image's tiles.
//                       scan_images_kernel, scan_tiles_kernel  (render_common.h) tile list starts.
//   gv_points_draw      tile_bin_kernel<true>   the same setup; places the point ids in the tile lists.
//                       splat_kernel            one workgroup per tile (256 threads = 16 x 16 pixels): the tile's list is
//                                               streamed through LDS 256 setups at a time; each pixel tests its centre
//                                               against the disc in int64, keeps the smallest key (Z << 32 | point id) in
//                                               a register, shades the winner and writes its outputs once.
//
// The splat setup is a pure function of (cloud, view, point), recomputed where needed (count, scatter, raster), so the
// bins hold 4-byte ids only.  A disc reaches at most R_MAX = 32 pixels from its centre: at most 6 x 6 tiles.
#include <math.h>

#include "render_tiles.h"

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

struct PointPrim : PArgs {                                       // a cloud's points, as tile_bin_kernel sees them
    __device__ int status(int m) const { return xf[m].status; }
    __device__ int count(int m) const { return (int)(poff[m + 1] - poff[m]); }
    __device__ bool box(int m, int v, int i, int& px0, int& px1, int& py0, int& py1) const {
        Splat s;
        if (!splat_setup(*this, m, v, i, s)) return false;
        px0 = s.px0, px1 = s.px1, py0 = s.py0, py1 = s.py1;
        return true;
    }
    typedef void CountOut;                                       // the count pass has nothing else to do
    __device__ void counted(int, int, int, void*) const {}
};

// ---- raster + shade ------------------------------------------------------------------------------------------------
struct LSplat {                                                  // one setup in LDS (20 bytes)
    int X, Y;
    unsigned Z;
    int R;                                                       // -1: a rejected slot (no |dx| is <= -1)
    int id;
};

struct PShade : Reflect {
    const float* normals;                                        // [sum P, 3] per point, or null: "depth" shading
};

// colour of the pixel whose winning splat is point id at depth Z
__device__ __forceinline__ void splat_colour(const PArgs& a, const PShade& sh, int m, int v, int id, unsigned Z,
                                             float3 color, float cs[3]) {
    if (sh.normals) {                                            // (uniform)
        const float* g = sh.normals + (a.poff[m] - a.poff[0] + id) * 3;
        float n[3] = {g[0], g[1], g[2]};
        if (a.rots) {
            const float* M = a.rots + (size_t)m * 9;
            n[0] = dot3(M, g[0], g[1], g[2]);
            n[1] = dot3(M + 3, g[0], g[1], g[2]);
            n[2] = dot3(M + 6, g[0], g[1], g[2]);
        }
        if (reflect(sh, v, n, color, cs)) return;
    }
    const float t = __fdiv_rn((float)Z, 16777215.0f);            // Z < 2^24: exact in fp32
    scale_colour(color, add_rn(sh.ambient, mul_rn(add_rn(1.0f, -sh.ambient), add_rn(1.0f, -t))), cs);
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
    const unsigned u[3] = {to_u8(cs[0]), to_u8(cs[1]), to_u8(cs[2])};
    store_pixel<OUT, 0>(out, p, cs, u);                          // one sample per pixel
}

// ---- host side -----------------------------------------------------------------------------------------------------
TileWs pws_layout(int32_t n, int32_t v, int32_t h, int32_t w) {  // extra: the clouds' radii
    return tile_ws_layout(n, v, h, w, (int64_t)n * 4);
}

// the checks both entry points share
int pcheck_common(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points, int32_t max_points,
                  const gv_render_desc* d, const float* cameras, const void* workspace, int64_t workspace_bytes) {
    return check_tile_common(points && point_offsets, total_points >= 0, n, max_points, d, cameras, workspace,
                             workspace_bytes, (int64_t)n * 4);
}

PointPrim make_prim(const float* points, const int64_t* point_offsets, const gv_render_desc* d, const float* cameras,
                     const float* rotations, void* workspace, const TileWs& L) {
    PointPrim a;
    static_cast<View&>(a) = make_view(d);
    a.pts = points;
    a.poff = (const long long*)point_offsets;
    a.cams = cameras;
    a.rots = rotations;
    a.xf = ws_at<const MeshXf>(workspace, L.xf);
    a.radius = ws_at<const float>(workspace, L.extra);
    return a;
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
    int rc = pcheck_common(points, point_offsets, n, total_points, max_points, desc, cameras, workspace, workspace_bytes);
    if (rc != GV_OK) return rc;
    for (int32_t i = 0; i < n; ++i)                              // radius is host memory
        if (!(radius[i] > 0.0f) || !isfinite(radius[i])) return GV_E_BADARG;
    const hipStream_t st = (hipStream_t)stream;
    const TileWs L = pws_layout(n, desc->num_views, desc->height, desc->width);
    const PointPrim a = make_prim(points, point_offsets, desc, cameras, rotations, workspace, L);
    GV_HIP_CHECK(hipMemcpyAsync(ws_at<char>(workspace, L.extra), radius, (size_t)n * 4, hipMemcpyHostToDevice, st));
    rc = start_prepare(st, a, n, workspace, L, points, point_offsets, point_offsets, total_points, total_points,
                       desc->fit, status);
    if (rc == GV_OK) rc = launch_bin<false>(st, a, max_points, n, workspace, L, nullptr, 0ll);
    return rc != GV_OK ? rc : finish_prepare(st, a, n, workspace, L, pair_total);
}

extern "C" int gv_points_draw(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                              int32_t max_points, const gv_render_desc* desc, const float* cameras,
                              const float* rotations, void* workspace, int64_t workspace_bytes, void* bins,
                              int64_t bins_bytes, int64_t total, int32_t output, void* out, int32_t* point_id,
                              uint32_t* depth, const float* normals, const gv_render_shading* shading,
                              const float* lights, const float* halfs, void* stream) {
    int squarings = 0;
    int rc = check_draw_args(bins, out, total, output);
    if (rc == GV_OK && normals) rc = check_shading(shading, lights, halfs, &squarings);      // "normal" shading
    if (rc == GV_OK)
        rc = pcheck_common(points, point_offsets, n, total_points, max_points, desc, cameras, workspace, workspace_bytes);
    if (rc != GV_OK) return rc;
    if (squarings < 0) return GV_E_UNSUPPORTED;
    rc = check_draw_buffers(bins, bins_bytes, total, output, out, point_id, depth);
    if (rc != GV_OK) return rc;
    if ((uintptr_t)normals & 3u) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const TileWs L = pws_layout(n, desc->num_views, desc->height, desc->width);
    const PointPrim a = make_prim(points, point_offsets, desc, cameras, rotations, workspace, L);
    const long long cap = bins_bytes / 4;
    int* b = static_cast<int*>(bins);
    rc = launch_bin<true>(st, a, max_points, n, workspace, L, b, cap);
    if (rc != GV_OK) return rc;
    PShade sh;
    static_cast<Reflect&>(sh) = make_reflect(desc, normals ? shading : nullptr, squarings, lights, halfs);
    sh.normals = normals;
    const float3 color = make_float3(desc->color[0], desc->color[1], desc->color[2]);
    const float3 bg = make_float3(desc->background[0], desc->background[1], desc->background[2]);
    const dim3 grid((unsigned)(a.tiles_x * a.tiles_y), (unsigned)desc->num_views, (unsigned)n);
    dispatch_output(output, [&](auto OUT) {
        hipLaunchKernelGGL(splat_kernel<decltype(OUT)::value>, grid, dim3(RT), 0, st, static_cast<const PArgs&>(a), sh,
                           ws_at<const int>(workspace, L.tile_count), ws_at<const long long>(workspace, L.tile_start),
                           static_cast<const int*>(b), cap, color, bg, out, point_id, depth);
    });
    GV_LAUNCH_CHECK();
    return GV_OK;
}
