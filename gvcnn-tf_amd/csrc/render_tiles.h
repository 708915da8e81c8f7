// The tile lists of the two renderers (render.hip: triangles; render_points.hip: splats): the binning kernel that counts
// and scatters a shape's elements into the image's 16x16-pixel tiles, the workspace that holds the lists, and the host
// steps and argument checks around them.  Like render_common.h, everything sits in the including file's unnamed namespace.
#pragma once
#include <type_traits>

#include "render_common.h"

namespace {

// ---- binning: count (SCATTER = false) and scatter (SCATTER = true) --------------------------------------------------
// Prim is a renderer's setup arguments (a View) by value, with
//   int  status(m)                              the shape's status,
//   int  count(m)                               its elements (<= 2^24 when the status is OK),
//   bool box(m, v, t, px0, px1, py0, py1)       the pixel range of element t in view v; false: it covers no sample,
//   void counted(m, v, t, Prim::CountOut*)      what the count pass does once per element besides counting, and where it
//                                               writes (a kernel argument of its own, so that it can be __restrict__:
//                                               a setup that follows the write then keeps what the hook has loaded).
// Grid (element chunks, view, shape); gridDim.x is a hint: the loop strides over every chunk whatever the grid holds.
// Count: every thread sets up its elements and counts them into the tiles with LDS atomics; the workgroup then adds its
// nonzero tile counts to the global counters (one atomic per workgroup and tile, never per fragment).  Scatter: the same
// setup and LDS counts; each workgroup reserves a run of every tile list it feeds and places its element ids there
// through LDS cursors.  List order is scheduling dependent; nothing downstream depends on it.
template <bool SCATTER, class Prim>
__global__ __launch_bounds__(RT) void tile_bin_kernel(Prim prim, int* __restrict__ tile_count,
                                                      long long* __restrict__ image_total,
                                                      const long long* __restrict__ tile_start,
                                                      int* __restrict__ tile_fill, int* __restrict__ bins, long long cap,
                                                      typename Prim::CountOut* __restrict__ count_out) {
    __shared__ int s_cnt[MAX_TILES];
    __shared__ long long s_base[SCATTER ? MAX_TILES : 1];
    __shared__ long long s_sum[RT / 64];
    const int m = blockIdx.z, v = blockIdx.y, tid = threadIdx.x;
    if (prim.status(m) != GV_RENDER_OK) return;                  // (uniform)
    const int ne = prim.count(m);
    const int T = prim.tiles_x * prim.tiles_y;
    const long long img = (long long)m * prim.V + v;
    const long long stride = (long long)gridDim.x * CHUNK;
    for (long long c0 = (long long)blockIdx.x * CHUNK; c0 < ne; c0 += stride) {
        const int lo = (int)c0, hi = min(lo + CHUNK, ne);
        for (int i = tid; i < T; i += RT) s_cnt[i] = 0;
        __syncthreads();
        for (int t = lo + tid; t < hi; t += RT) {
            if (!SCATTER) prim.counted(m, v, t, count_out);
            int px0, px1, py0, py1;
            if (!prim.box(m, v, t, px0, px1, py0, py1)) continue;
            for (int ty = py0 >> 4; ty <= py1 >> 4; ++ty)
                for (int tx = px0 >> 4; tx <= px1 >> 4; ++tx) atomicAdd(&s_cnt[ty * prim.tiles_x + tx], 1);
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
                int px0, px1, py0, py1;
                if (!prim.box(m, v, t, px0, px1, py0, py1)) continue;
                for (int ty = py0 >> 4; ty <= py1 >> 4; ++ty)
                    for (int tx = px0 >> 4; tx <= px1 >> 4; ++tx) {
                        const int i = ty * prim.tiles_x + tx;
                        const long long pos = s_base[i] + atomicAdd(&s_cnt[i], 1);
                        if (pos >= 0 && pos < cap) bins[pos] = t;
                    }
            }
        }
        __syncthreads();                                         // s_cnt / s_sum are reused by the next chunk
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The workspace of a prepare / draw pair, as byte offsets; `extra` is the renderer's own region (the flat shade table, the
// clouds' radii).
struct TileWs {
    int64_t xf, extra, tile_count, tile_fill, tile_start, image_total, image_base, bytes;
};

inline TileWs tile_ws_layout(int32_t n, int32_t v, int32_t h, int32_t w, int64_t extra_bytes) {
    const int64_t T = (int64_t)((h + TS - 1) / TS) * ((w + TS - 1) / TS);
    const int64_t nimg = (int64_t)n * v;
    TileWs L;
    int64_t o = 0;
    L.xf = o;          o += round_up((int64_t)n * sizeof(MeshXf), 256);
    L.extra = o;       o += round_up(extra_bytes, 256);
    L.tile_count = o;  o += round_up(nimg * T * 4, 256);
    L.tile_fill = o;   o += round_up(nimg * T * 4, 256);
    L.tile_start = o;  o += round_up(nimg * T * 8, 256);
    L.image_total = o; o += round_up(nimg * 8, 256);
    L.image_base = o;  o += round_up(nimg * 8, 256);
    L.bytes = o;
    return L;
}

template <class T>
inline T* ws_at(void* workspace, int64_t offset) {
    return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset);
}

// f(std::integral_constant<int, x>) for x one of A, B, C (the caller has checked that it is): a run-time code becomes a
// template argument in one place per kernel family
template <int A, int B, int C, class F>
decltype(auto) dispatch3(int x, F f) {
    return x == A   ? f(std::integral_constant<int, A>{})
           : x == B ? f(std::integral_constant<int, B>{})
                    : f(std::integral_constant<int, C>{});
}
template <class F>
decltype(auto) dispatch_output(int32_t output, F f) {
    return dispatch3<GV_RENDER_OUT_F32_QUANTIZED, GV_RENDER_OUT_F32, GV_RENDER_OUT_U8>(output, f);
}

// one binning pass over n shapes of at most max_elems elements each (the grid size is a hint)
inline dim3 bin_grid(int32_t max_elems, int32_t v, int32_t n) {
    const int chunks = max_elems > 0 ? (max_elems + CHUNK - 1) / CHUNK : 1;
    return dim3((unsigned)chunks, (unsigned)v, (unsigned)n);
}
template <bool SCATTER, class Prim>
int launch_bin(hipStream_t st, const Prim& prim, int32_t max_elems, int32_t n, void* ws, const TileWs& L, int* bins,
               long long cap, typename Prim::CountOut* count_out = nullptr) {
    const size_t tiles = (size_t)n * prim.V * prim.tiles_x * prim.tiles_y;
    if (SCATTER) GV_HIP_CHECK(hipMemsetAsync(ws_at<char>(ws, L.tile_fill), 0, tiles * 4, st));   // the lists' cursors
    hipLaunchKernelGGL((tile_bin_kernel<SCATTER, Prim>), bin_grid(max_elems, prim.V, n), dim3(RT), 0, st, prim,
                       ws_at<int>(ws, L.tile_count), ws_at<long long>(ws, L.image_total),
                       ws_at<const long long>(ws, L.tile_start), ws_at<int>(ws, L.tile_fill), bins, cap, count_out);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

// prepare, before the count pass: clear the counters, normalise the n shapes (a cloud passes its point offsets twice)
inline int start_prepare(hipStream_t st, const View& a, int32_t n, void* ws, const TileWs& L, const float* verts,
                         const int64_t* vert_offsets, const int64_t* elem_offsets, int64_t total_verts,
                         int64_t total_elems, float fit, int32_t* status) {
    const size_t tiles = (size_t)n * a.V * a.tiles_x * a.tiles_y;
    GV_HIP_CHECK(hipMemsetAsync(ws_at<char>(ws, L.tile_count), 0, tiles * 4, st));
    GV_HIP_CHECK(hipMemsetAsync(ws_at<char>(ws, L.image_total), 0, (size_t)n * a.V * 8, st));
    hipLaunchKernelGGL(normalise_kernel, dim3(n), dim3(RT), 0, st, verts, (const long long*)vert_offsets,
                       (const long long*)elem_offsets, (long long)total_verts, (long long)total_elems, fit,
                       ws_at<MeshXf>(ws, L.xf), status);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

// ... and after it: the counts become the tile list starts and *pair_total
inline int finish_prepare(hipStream_t st, const View& a, int32_t n, void* ws, const TileWs& L, int64_t* pair_total) {
    const long long nimg = (long long)n * a.V;
    hipLaunchKernelGGL(scan_images_kernel, dim3(1), dim3(SCAN_T), 0, st, ws_at<const long long>(ws, L.image_total), nimg,
                       ws_at<long long>(ws, L.image_base), (long long*)pair_total);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)nimg), dim3(SCAN_T), 0, st, ws_at<const int>(ws, L.tile_count),
                       ws_at<const long long>(ws, L.image_base), a.tiles_x * a.tiles_y, ws_at<long long>(ws, L.tile_start));
    GV_LAUNCH_CHECK();
    return GV_OK;
}

// what every entry point of both renderers checks first.  arrays: the shape arrays are all there; totals: none of the
// element totals is negative
inline int check_tile_common(bool arrays, bool totals, int32_t n, int32_t max_elems, const gv_render_desc* d,
                             const float* cameras, const void* workspace, int64_t workspace_bytes, int64_t extra_bytes) {
    if (!arrays || !d || !cameras || !workspace) return GV_E_BADARG;
    if (n <= 0 || !totals || max_elems < 0) return GV_E_BADARG;
    if (check_desc(d) != GV_OK) return GV_E_BADARG;
    if (d->height > MAX_SIDE || d->width > MAX_SIDE || d->num_views > 64 || n > 65535 || max_elems > MAX_TRIS)
        return GV_E_UNSUPPORTED;
    if (workspace_bytes < tile_ws_layout(n, d->num_views, d->height, d->width, extra_bytes).bytes) return GV_E_BADARG;
    if (!gv_aligned16(workspace)) return GV_E_ALIGN;
    return GV_OK;
}

// The checks every draw call shares beyond those come in two parts, because the return-code precedence puts each
// renderer's own checks (shading, shapes, workspace) between them: what a draw call refuses first ...
inline int check_draw_args(const void* bins, const void* out, int64_t total, int32_t output) {
    if (!bins || !out || total < 0) return GV_E_BADARG;
    if (output != GV_RENDER_OUT_F32_QUANTIZED && output != GV_RENDER_OUT_F32 && output != GV_RENDER_OUT_U8)
        return GV_E_BADARG;
    return GV_OK;
}
// ... and last: the tile lists' size, then the alignment of the lists, the output and the two optional buffers
inline int check_draw_buffers(const void* bins, int64_t bins_bytes, int64_t total, int32_t output, const void* out,
                              const void* ids, const void* depth) {
    if (bins_bytes < gv_render_bins_bytes(total)) return GV_E_BADARG;
    if (!gv_aligned16(bins) || (output != GV_RENDER_OUT_U8 && ((uintptr_t)out & 3u))) return GV_E_ALIGN;
    if (((uintptr_t)ids & 3u) || ((uintptr_t)depth & 3u)) return GV_E_ALIGN;
    return GV_OK;
}

}  // namespace
