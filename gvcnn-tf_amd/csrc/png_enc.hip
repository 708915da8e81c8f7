// PNG encode on the device (gv_png_encode_batch) and its host twin (gv_png_encode_host): png_enc_core.h holds the
// encoder, this file the four kernels, the argument checks and the workspace layout.
//
//   png_enc_color_kernel    one workgroup per image: is every pixel gray?  -> color_type[i]
//   png_enc_filter_kernel   one wave per row: the five filter costs (a wave reduction each), the choice, the filtered row
//                           into the workspace.  Rows are filtered from their unfiltered neighbours: no order among them.
//   png_enc_segment_kernel  one workgroup of 256 per (image, segment): the segment and its working arrays in 47 KB of
//                           LDS (GvPngEncSeg), one 32-byte chunk per lane; histogram and output words through LDS
//                           integer atomics (sums and ors: the result does not depend on their order); lane 0 builds the
//                           code lengths.  Output, byte length and Adler sums go to the segment's slot of the workspace.
//   png_enc_gather_kernel   one workgroup per (image, segment): sums the lengths of the segments before its own, copies
//                           its bytes there; the first writes 78 01, the last the Adler-32 and length[i].
// Workspace: [n] filtered rows (raw stride, 16-byte aligned) | [n, segs] output slots of GV_PNG_ENC_SEGOUT bytes |
// [n, segs] GV_PNG_ENC_META int32, segs = the segments of an RGB image of this size.
#include <new>

#include "gv_common.h"
#include "png_enc_core.h"

namespace {

inline int64_t enc_align16(int64_t v) { return (v + 15) / 16 * 16; }

struct EncLayout {
    int64_t raw_stride, segs, rows_bytes, slots_bytes, meta_bytes;
};
inline EncLayout enc_layout(int32_t n, int32_t h0, int32_t w0) {
    EncLayout L;
    L.raw_stride = enc_align16(gv_png_enc_raw_bytes(h0, w0, 3));
    L.segs = gv_png_enc_segments(gv_png_enc_raw_bytes(h0, w0, 3));
    L.rows_bytes = (int64_t)n * L.raw_stride;
    L.slots_bytes = (int64_t)n * L.segs * GV_PNG_ENC_SEGOUT;
    L.meta_bytes = enc_align16((int64_t)n * L.segs * GV_PNG_ENC_META * (int64_t)sizeof(int32_t));
    return L;
}

// the lanes of one wave (the filter kernel: no LDS, no barrier)
struct EncWaveCtx {
    int lane, nlanes;
    __device__ void sync() const {}
    __device__ uint32_t sum(uint32_t v) const {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
        return v;
    }
    __device__ void add(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
    __device__ void orr(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
};

// the lanes of one workgroup; add / orr go to LDS
struct EncGroupCtx {
    int lane, nlanes;
    __device__ void sync() const { __syncthreads(); }
    __device__ uint32_t sum(uint32_t v) const { return v; }      // (not used by the segment encoder)
    __device__ void add(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
    __device__ void orr(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
};

__global__ __launch_bounds__(256) void png_enc_color_kernel(const uint8_t* __restrict__ src, int h0, int w0, int color,
                                                            int32_t* __restrict__ color_type) {
    __shared__ int32_t flag;
    const int i = blockIdx.x;
    if (color == GV_PNG_COLOR_RGB) {
        if (threadIdx.x == 0) color_type[i] = 2;
        return;
    }
    if (threadIdx.x == 0) flag = 0;
    __syncthreads();
    const EncGroupCtx ctx = {(int)threadIdx.x, 256};
    gv_png_enc_scan_gray(src + (int64_t)i * h0 * w0 * 3, (uint32_t)h0 * (uint32_t)w0, &flag, ctx);
    __syncthreads();
    if (threadIdx.x == 0) color_type[i] = flag ? 2 : 0;
}

__global__ __launch_bounds__(256) void png_enc_filter_kernel(const uint8_t* __restrict__ src, int h0, int w0, int filter,
                                                             const int32_t* __restrict__ color_type, uint8_t* rows,
                                                             int64_t raw_stride, int row_groups) {
    const int i = blockIdx.x / row_groups, y = (blockIdx.x % row_groups) * 4 + (int)(threadIdx.x >> 6);
    if (y >= h0) return;                                         // (a whole wave)
    const int ch = color_type[i] == 0 ? 1 : 3;
    const EncWaveCtx ctx = {(int)(threadIdx.x & 63), 64};
    gv_png_enc_filter_row(src + (int64_t)i * h0 * w0 * 3, w0, ch, y, filter,
                          rows + (int64_t)i * raw_stride + (int64_t)y * (1 + (int64_t)w0 * ch), ctx);
}

__global__ __launch_bounds__(256) void png_enc_segment_kernel(int h0, int w0, const int32_t* __restrict__ color_type,
                                                              const uint8_t* __restrict__ rows, int64_t raw_stride, int segs,
                                                              uint8_t* slots, int32_t* meta) {
    __shared__ __attribute__((aligned(16))) GvPngEncSeg seg;
    const int i = blockIdx.x / segs, s = blockIdx.x % segs;
    const int ch = color_type[i] == 0 ? 1 : 3;
    const int64_t raw = gv_png_enc_raw_bytes(h0, w0, ch), mine = gv_png_enc_segments(raw);
    if (s >= mine) return;                                       // (a gray image has fewer segments than an RGB one)
    const int64_t off = (int64_t)s * GV_PNG_ENC_SEG;
    const uint32_t n = (uint32_t)(raw - off < GV_PNG_ENC_SEG ? raw - off : GV_PNG_ENC_SEG);
    const EncGroupCtx ctx = {(int)threadIdx.x, 256};
    const int64_t slot = (int64_t)i * segs + s;
    gv_png_enc_segment(rows + (int64_t)i * raw_stride + off, n, ch, s == mine - 1, &seg, slots + slot * GV_PNG_ENC_SEGOUT,
                       meta + slot * GV_PNG_ENC_META, ctx);
}

__global__ __launch_bounds__(256) void png_enc_gather_kernel(int h0, int w0, const int32_t* __restrict__ color_type, int segs,
                                                             const uint8_t* __restrict__ slots,
                                                             const int32_t* __restrict__ meta, uint8_t* out,
                                                             int64_t out_stride, int32_t* length) {
    __shared__ uint32_t red[256];
    const int i = blockIdx.x / segs, s = blockIdx.x % segs, lane = threadIdx.x;
    const int ch = color_type[i] == 0 ? 1 : 3;
    const int64_t raw = gv_png_enc_raw_bytes(h0, w0, ch), mine = gv_png_enc_segments(raw);
    if (s >= mine) return;
    const int32_t* m = meta + (int64_t)i * segs * GV_PNG_ENC_META;
    uint32_t part = 0;
    for (int k = lane; k < s; k += 256) part += (uint32_t)m[k * GV_PNG_ENC_META];
    red[lane] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (lane < o) red[lane] += red[lane + o];
        __syncthreads();
    }
    const uint32_t off = 2u + red[0], len = (uint32_t)m[s * GV_PNG_ENC_META];
    uint8_t* dst = out + (int64_t)i * out_stride;
    const uint8_t* from = slots + ((int64_t)i * segs + s) * GV_PNG_ENC_SEGOUT;
    if ((int64_t)off + len + 4 > out_stride) return;             // (cannot happen: out_stride >= the bound)
    for (uint32_t k = (uint32_t)lane; k < len; k += 256u) dst[off + k] = from[k];
    if (s == 0 && lane == 0) {
        dst[0] = 0x78;
        dst[1] = 0x01;
    }
    if (s == mine - 1 && lane == 0) {
        uint32_t a = 1, b = 0;
        int bad = 0;
        for (int k = 0; k < (int)mine; ++k) {
            const int64_t left = raw - (int64_t)k * GV_PNG_ENC_SEG;
            gv_png_enc_adler_append(a, b, (uint32_t)(left < GV_PNG_ENC_SEG ? left : GV_PNG_ENC_SEG),
                                    (uint32_t)m[k * GV_PNG_ENC_META + 1], (uint32_t)m[k * GV_PNG_ENC_META + 2]);
            bad |= m[k * GV_PNG_ENC_META + 3];
        }
        const uint32_t end = off + len;
        dst[end] = (uint8_t)(b >> 8);
        dst[end + 1] = (uint8_t)b;
        dst[end + 2] = (uint8_t)(a >> 8);
        dst[end + 3] = (uint8_t)a;
        length[i] = bad ? -1 : (int32_t)(end + 4);
    }
}

// the checks both entry points share
int enc_check_args(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t filter, int32_t color, const uint8_t* out,
                   int64_t out_stride, const int32_t* length, const int32_t* color_type) {
    if (!src || !out || !length || !color_type || n <= 0 || h0 <= 0 || w0 <= 0) return GV_E_BADARG;
    if (filter < 0 || filter > GV_PNG_FILTER_ADAPTIVE) return GV_E_BADARG;
    if (color != GV_PNG_COLOR_AUTO && color != GV_PNG_COLOR_RGB) return GV_E_BADARG;
    if (gv_png_enc_raw_bytes(h0, w0, 3) > 0x7fffffff) return GV_E_UNSUPPORTED;
    if (out_stride < gv_png_enc_bound(h0, w0) || (out_stride & 15)) return GV_E_BADARG;
    if ((int64_t)n * gv_png_enc_segments(gv_png_enc_raw_bytes(h0, w0, 3)) > 0x7fffffff ||
        (int64_t)n * ((h0 + 3) / 4) > 0x7fffffff)
        return GV_E_UNSUPPORTED;
    return GV_OK;
}

}  // namespace

extern "C" int64_t gv_png_encode_segment_bytes(void) { return GV_PNG_ENC_SEG; }

extern "C" int64_t gv_png_encode_bound(int32_t h0, int32_t w0) {
    if (h0 <= 0 || w0 <= 0) return GV_E_BADARG;
    if (gv_png_enc_raw_bytes(h0, w0, 3) > 0x7fffffff) return GV_E_UNSUPPORTED;
    return gv_png_enc_bound(h0, w0);
}

extern "C" int64_t gv_png_encode_workspace_bytes(int32_t n, int32_t h0, int32_t w0) {
    if (n <= 0 || h0 <= 0 || w0 <= 0) return GV_E_BADARG;
    if (gv_png_enc_raw_bytes(h0, w0, 3) > 0x7fffffff) return GV_E_UNSUPPORTED;
    const EncLayout L = enc_layout(n, h0, w0);
    return L.rows_bytes + L.slots_bytes + L.meta_bytes;
}

extern "C" int gv_png_encode_batch(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t filter, int32_t color,
                                   uint8_t* out, int64_t out_stride, int32_t* length, int32_t* color_type, void* ws,
                                   int64_t ws_bytes, void* stream) {
    const int rc = enc_check_args(src, n, h0, w0, filter, color, out, out_stride, length, color_type);
    if (rc != GV_OK) return rc;
    if (!ws || !gv_aligned16(ws)) return ws ? GV_E_ALIGN : GV_E_BADARG;
    if (ws_bytes < gv_png_encode_workspace_bytes(n, h0, w0)) return GV_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const EncLayout L = enc_layout(n, h0, w0);
    uint8_t* rows = (uint8_t*)ws;
    uint8_t* slots = rows + L.rows_bytes;
    int32_t* meta = (int32_t*)(slots + L.slots_bytes);
    const int row_groups = (h0 + 3) / 4, segs = (int)L.segs;
    hipLaunchKernelGGL(png_enc_color_kernel, dim3((unsigned)n), dim3(256), 0, st, src, h0, w0, color, color_type);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_enc_filter_kernel, dim3((unsigned)((int64_t)n * row_groups)), dim3(256), 0, st, src, h0, w0, filter,
                       (const int32_t*)color_type, rows, L.raw_stride, row_groups);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_enc_segment_kernel, dim3((unsigned)((int64_t)n * segs)), dim3(256), 0, st, h0, w0,
                       (const int32_t*)color_type, (const uint8_t*)rows, L.raw_stride, segs, slots, meta);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_enc_gather_kernel, dim3((unsigned)((int64_t)n * segs)), dim3(256), 0, st, h0, w0,
                       (const int32_t*)color_type, segs, (const uint8_t*)slots, (const int32_t*)meta, out, out_stride, length);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_png_encode_host(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t filter, int32_t color,
                                  uint8_t* out, int64_t out_stride, int32_t* length, int32_t* color_type) {
    const int rc = enc_check_args(src, n, h0, w0, filter, color, out, out_stride, length, color_type);
    if (rc != GV_OK) return rc;
    const int64_t raw3 = gv_png_enc_raw_bytes(h0, w0, 3);
    uint32_t* rows = new (std::nothrow) uint32_t[(size_t)(raw3 + 3) / 4];       // (4-byte aligned for the segment loads)
    uint32_t* slot = new (std::nothrow) uint32_t[GV_PNG_ENC_OUTWORDS];
    GvPngEncSeg* seg = new (std::nothrow) GvPngEncSeg;
    int bad = rows && slot && seg ? GV_OK : GV_E_UNSUPPORTED;
    for (int i = 0; i < n && bad == GV_OK; ++i) {
        const int st = gv_png_enc_image_serial(src + (size_t)i * h0 * w0 * 3, h0, w0, filter, color, (uint8_t*)rows, (uint8_t*)slot,
                                               seg, out + (size_t)i * out_stride, out_stride, &length[i], &color_type[i]);
        if (st != GV_PNG_OK) bad = GV_E_UNSUPPORTED;
    }
    delete[] rows;
    delete[] slot;
    delete seg;
    return bad;
}
