// PNG decode on the device (gv_png_decode_batch) and its host twin (gv_png_decode_host): png_core.h holds the decoder,
// this file the two kernels and the argument checks.
//
//   png_inflate_kernel      one wave per image.  All 64 lanes run the decoder of png_core.h on the same stream (same
//                           bit-reader state, same branches — scalar code —, tables in LDS built by lane 0); lane 0
//                           stores literals, the wave shares the bytes of a match / stored block and the Adler-32.
//                           The newest 64 KB of output (the window and more) are an LDS ring, flushed to the
//                           workspace row in pieces of 8 KB.
//   png_unfilter_kernel     one wave per image, 64 rows at a time: lane r un-filters row y0 + r in chunks of four pixels,
//                           one chunk behind the lane above it, so left / up / upper-left are registers and a lane
//                           shift; the pixels go to `out` expanded to RGB.
#include <new>

#include "gv_common.h"
#include "png_core.h"

namespace {

#define GV_PNG_RING 65536                                        // LDS ring of the newest output: window (32 KB) and more
#define GV_PNG_FLUSH 8192                                        // a piece of that size goes to global memory when complete

struct GvPngWaveCtx {
    int lane, nlanes;
    uint8_t* ring;
    __device__ void sync() const { __syncthreads(); }            // (one wave per workgroup: a fence, not a wait)
    __device__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ void put(uint8_t*, uint32_t pos, uint8_t v) const { ring[pos & (GV_PNG_RING - 1)] = v; }
    __device__ uint8_t get(const uint8_t*, uint32_t pos) const { return ring[pos & (GV_PNG_RING - 1)]; }
    __device__ uint32_t max_run() const { return GV_PNG_FLUSH; }
    // [from, to) was just written, to - from <= GV_PNG_FLUSH: at most ONE piece became complete — store it (16 bytes a
    // lane: `out` is 16-byte aligned, pieces start at multiples of GV_PNG_FLUSH).  It stays in the ring for another
    // GV_PNG_RING - 2 * GV_PNG_FLUSH bytes of output at least.
    __device__ void wrote(uint8_t* out, uint32_t from, uint32_t to) const {
        if ((from ^ to) < GV_PNG_FLUSH) return;                  // (same piece: the bits above the piece size agree)
        const uint32_t base = from & ~(uint32_t)(GV_PNG_FLUSH - 1);
        __syncthreads();
        for (uint32_t i = (uint32_t)lane * 16u; i < GV_PNG_FLUSH; i += (uint32_t)nlanes * 16u)
            *(uint4*)(out + base + i) = *(const uint4*)(ring + ((base + i) & (GV_PNG_RING - 1)));
    }
    __device__ void finish(uint8_t* out, uint32_t op) const {
        __syncthreads();
        for (uint32_t i = (op & ~(uint32_t)(GV_PNG_FLUSH - 1)) + (uint32_t)lane; i < op; i += (uint32_t)nlanes)
            out[i] = ring[i & (GV_PNG_RING - 1)];
    }
};

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ streams,
                                                         const gv_png_image* __restrict__ images, int h0, int w0,
                                                         uint8_t* ws, int64_t ws_stride, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];     // the ring, then the tables
    GvPngTables& tables = *(GvPngTables*)(png_lds + GV_PNG_RING);
    const int i = blockIdx.x;
    const gv_png_image im = images[i];
    const GvPngWaveCtx ctx = {(int)threadIdx.x, 64, png_lds};
    const uint32_t raw = (uint32_t)h0 * (1u + (uint32_t)w0 * (uint32_t)gv_png_channels(im.color_type));
    const int st = gv_png_inflate(streams + im.offset, (uint32_t)im.length, ws + (int64_t)i * ws_stride, raw, &tables, ctx);
    if (threadIdx.x == 0) status[i] = st;
}

// four pixels of BPP bytes each from p, one pixel per word (byte c of the pixel in bits 8c..8c+7); pixels at or past
// `valid` (a row's ragged last chunk) read as 0 and are not loaded
template <int BPP>
__device__ __forceinline__ void png_load_chunk(const uint8_t* p, int valid, uint32_t (&px)[4]) {
    if (valid >= 4) {
        uint32_t w[BPP];
        __builtin_memcpy(w, p, 4 * BPP);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < BPP; ++c) {
                const int i = k * BPP + c;
                v |= ((w[i >> 2] >> ((i & 3) * 8)) & 255u) << (8 * c);
            }
            px[k] = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t v = 0;
            if (k < valid) {
#pragma unroll
                for (int c = 0; c < BPP; ++c) v |= (uint32_t)p[k * BPP + c] << (8 * c);
            }
            px[k] = v;
        }
    }
}

// Un-filter + expand one image with one wave: 64 ROWS at a time, lane r on row y0 + r, in chunks of four pixels, each
// lane one chunk behind the lane above it — what a pixel needs (left: the lane's own last result; up and upper-left: what
// the lane above produced one step earlier) is then in registers, and comes down by a lane shift.  Lane 0 reads its "up"
// from the workspace, where lane 63 of the previous 64 rows left its un-filtered row.  Returns a GV_PNG_* status.
template <int BPP>
__device__ int png_unfilter_image(int ctype, int plen, const uint8_t* __restrict__ pal, int h0, int w0, uint8_t* raw,
                                  uint8_t* __restrict__ dst, int lane) {
    const int rb = w0 * BPP, nch = (w0 + 3) >> 2;
    int bad = 0;
    for (int y0 = 0; y0 < h0; y0 += 64) {
        const int y = y0 + lane;
        const bool act = y < h0, more = y0 + 64 < h0;
        uint8_t* row = raw + (int64_t)(act ? y : y0) * (rb + 1) + 1;
        const int ft = act ? row[-1] : 0;
        if (__any(ft > 4)) return GV_PNG_BAD_FILTER;
        const bool up_mem = lane == 0 && y > 0;                  // the row above was un-filtered by the previous pass
        uint32_t a = 0, c = 0, mine[4] = {0, 0, 0, 0}, nxt[4] = {0, 0, 0, 0}, upn[4] = {0, 0, 0, 0};
        if (lane == 0) {                                         // (chunk 0 of lane 0; the others start later)
            png_load_chunk<BPP>(row, w0, nxt);
            if (up_mem) png_load_chunk<BPP>(row - (rb + 1), w0, upn);
        }
        for (int s = 0; s < nch + 63; ++s) {
            const int j = s - lane;
            const bool ok = act && j >= 0 && j < nch;
            uint32_t x[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[k] = nxt[k];
                b[k] = __shfl_up(mine[k], 1);                    // (every lane takes part; lane 0 gets its own back)
                if (lane == 0) b[k] = upn[k];
            }
            if (act && j + 1 >= 0 && j + 1 < nch) {              // the next step's bytes, a step ahead of their use
                png_load_chunk<BPP>(row + (int64_t)(j + 1) * 4 * BPP, w0 - 4 * (j + 1), nxt);
                if (up_mem) png_load_chunk<BPP>(row - (rb + 1) + (int64_t)(j + 1) * 4 * BPP, w0 - 4 * (j + 1), upn);
            }
            if (ok) {
                const int valid = w0 - 4 * j;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t o = 0;
#pragma unroll
                    for (int ch = 0; ch < BPP; ++ch) {
                        const int xa = (a >> (8 * ch)) & 255, xb = (b[k] >> (8 * ch)) & 255, xc = (c >> (8 * ch)) & 255;
                        const int p = ft == 0 ? 0 : ft == 1 ? xa : ft == 2 ? xb : ft == 3 ? (xa + xb) >> 1 : gv_png_paeth(xa, xb, xc);
                        o |= (uint32_t)((((x[k] >> (8 * ch)) & 255) + p) & 255) << (8 * ch);
                    }
                    a = o;
                    c = b[k];
                    mine[k] = o;
                }
                uint32_t rgb[4];                                 // tf.image.decode_png(channels=3) of the four pixels
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t o = mine[k];
                    if (ctype == 3) {
                        const int idx = o & 255;
                        if (idx < plen) rgb[k] = pal[3 * idx] | (uint32_t)pal[3 * idx + 1] << 8 | (uint32_t)pal[3 * idx + 2] << 16;
                        else { rgb[k] = 0; if (k < valid) bad = 1; }
                    } else if (ctype == 2 || ctype == 6) {
                        rgb[k] = o & 0xffffffu;
                    } else {
                        rgb[k] = (o & 255u) * 0x010101u;
                    }
                }
                uint8_t* o = dst + ((int64_t)y * w0 + 4 * j) * 3;
                if (valid >= 4) {
                    const uint32_t w[3] = {rgb[0] | rgb[1] << 24, rgb[1] >> 8 | rgb[2] << 16, rgb[2] >> 16 | rgb[3] << 8};
                    __builtin_memcpy(o, w, 12);
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (k < valid) {
                            o[3 * k] = (uint8_t)rgb[k];
                            o[3 * k + 1] = (uint8_t)(rgb[k] >> 8);
                            o[3 * k + 2] = (uint8_t)(rgb[k] >> 16);
                        }
                }
                if (more && lane == 63) {                        // the next 64 rows' lane 0 reads this row as its "up"
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < valid) {
#pragma unroll
                            for (int ch = 0; ch < BPP; ++ch) row[(4 * j + k) * BPP + ch] = (uint8_t)(mine[k] >> (8 * ch));
                        }
                }
            }
        }
        __syncthreads();                                         // lane 63's row is visible to the next pass
    }
    return __any(bad) ? GV_PNG_BAD_PALETTE_INDEX : GV_PNG_OK;
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(const gv_png_image* __restrict__ images, int h0, int w0,
                                                          const uint8_t* __restrict__ palettes, uint8_t* ws,
                                                          int64_t ws_stride, uint8_t* __restrict__ out, int32_t* status) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (status[i] != GV_PNG_OK) return;                          // (uniform: the inflate kernel's verdict)
    const gv_png_image im = images[i];
    const uint8_t* pal = im.color_type == 3 ? palettes + im.palette_offset : nullptr;
    uint8_t* raw = ws + (int64_t)i * ws_stride;
    uint8_t* dst = out + (int64_t)i * h0 * w0 * 3;
    int st;
    switch (gv_png_channels(im.color_type)) {
        case 1: st = png_unfilter_image<1>(im.color_type, im.palette_len, pal, h0, w0, raw, dst, lane); break;
        case 2: st = png_unfilter_image<2>(im.color_type, im.palette_len, pal, h0, w0, raw, dst, lane); break;
        case 3: st = png_unfilter_image<3>(im.color_type, im.palette_len, pal, h0, w0, raw, dst, lane); break;
        default: st = png_unfilter_image<4>(im.color_type, im.palette_len, pal, h0, w0, raw, dst, lane); break;
    }
    if (lane == 0 && st != GV_PNG_OK) status[i] = st;
}

inline int64_t png_align16(int64_t v) { return (v + 15) / 16 * 16; }

// the checks both entry points share
int png_check_args(const uint8_t* streams, int64_t stream_bytes, const gv_png_image* images, int32_t n, int32_t h0,
                   int32_t w0, const uint8_t* palettes, const uint8_t* out, const int32_t* status) {
    if (!streams || !images || !out || !status || n <= 0 || h0 <= 0 || w0 <= 0 || stream_bytes < 16) return GV_E_BADARG;
    if ((int64_t)h0 * (1 + 4 * (int64_t)w0) > 0x7fffffff) return GV_E_UNSUPPORTED;
    for (int i = 0; i < n; ++i) {
        const gv_png_image& im = images[i];
        if (gv_png_channels(im.color_type) == 0) return GV_E_BADARG;
        if (im.offset < 0 || (im.offset & 15) || im.length < 0 || im.offset + im.length > stream_bytes - 16)
            return GV_E_BADARG;
        if (im.color_type == 3 && (!palettes || im.palette_offset < 0 || im.palette_len < 1 || im.palette_len > 256))
            return GV_E_BADARG;
    }
    return GV_OK;
}

}  // namespace

extern "C" int64_t gv_png_decode_workspace_bytes(int32_t n, int64_t max_raw_bytes) {
    if (n <= 0 || max_raw_bytes <= 0) return GV_E_BADARG;
    return png_align16((int64_t)n * (int64_t)sizeof(gv_png_image)) + (int64_t)n * png_align16(max_raw_bytes);
}

extern "C" int gv_png_decode_batch(const uint8_t* streams, int64_t stream_bytes, const gv_png_image* images, int32_t n,
                                   int32_t h0, int32_t w0, const uint8_t* palettes, uint8_t* out, int32_t* status,
                                   void* ws, int64_t ws_bytes, void* stream) {
    const int rc = png_check_args(streams, stream_bytes, images, n, h0, w0, palettes, out, status);
    if (rc != GV_OK) return rc;
    if (!ws || !gv_aligned16(ws)) return ws ? GV_E_ALIGN : GV_E_BADARG;
    if (ws_bytes < gv_png_decode_workspace_bytes(n, (int64_t)h0 * (1 + 4 * (int64_t)w0))) return GV_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t table = png_align16((int64_t)n * (int64_t)sizeof(gv_png_image));
    const int64_t stride = png_align16((int64_t)h0 * (1 + 4 * (int64_t)w0));
    gv_png_image* images_dev = (gv_png_image*)ws;
    uint8_t* rows = (uint8_t*)ws + table;
    GV_HIP_CHECK(hipMemcpyAsync(images_dev, images, (size_t)n * sizeof(gv_png_image), hipMemcpyHostToDevice, st));
    const int rl = gv_launch<png_inflate_kernel>(dim3((unsigned)n), dim3(64), GV_PNG_RING + sizeof(GvPngTables), st, streams,
                                                 (const gv_png_image*)images_dev, h0, w0, rows, stride, status);
    if (rl != GV_OK) return rl;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(64), 0, st, images_dev, h0, w0, palettes, rows, stride,
                       out, status);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_png_decode_host(const uint8_t* streams, int64_t stream_bytes, const gv_png_image* images, int32_t n,
                                  int32_t h0, int32_t w0, const uint8_t* palettes, uint8_t* out, int32_t* status) {
    const int rc = png_check_args(streams, stream_bytes, images, n, h0, w0, palettes, out, status);
    if (rc != GV_OK) return rc;
    uint8_t* raw = new (std::nothrow) uint8_t[(size_t)h0 * (1 + 4 * (size_t)w0)];
    GvPngTables* tables = new (std::nothrow) GvPngTables;
    if (!raw || !tables) {
        delete[] raw;
        delete tables;
        return GV_E_UNSUPPORTED;
    }
    for (int i = 0; i < n; ++i) {
        const gv_png_image& im = images[i];
        const uint32_t size = (uint32_t)h0 * (1u + (uint32_t)w0 * (uint32_t)gv_png_channels(im.color_type));
        int st = gv_png_inflate(streams + im.offset, (uint32_t)im.length, raw, size, tables, GvPngHostCtx());
        if (st == GV_PNG_OK)
            st = gv_png_unfilter_expand_serial(raw, h0, w0, im.color_type, im.color_type == 3 ? palettes + im.palette_offset : nullptr,
                                               im.palette_len, out + (size_t)i * h0 * w0 * 3);
        status[i] = st;
    }
    delete[] raw;
    delete tables;
    return GV_OK;
}

// ---- PNG row un-filtering (host code: tf.image.decode_png of train_data.py:55 after zlib inflate) -------------------
// raw: h rows of (1 filter byte + rowbytes data bytes); out: h x rowbytes.  Filters 0-4 of the PNG specification
// (None, Sub, Up, Average, Paeth); bpp = bytes per pixel.  Sequential by definition (each byte depends on its left
// neighbour), which is why it lives here and not in a Python loop.
extern "C" int gv_png_unfilter(const uint8_t* raw, int32_t h, int32_t rowbytes, int32_t bpp, uint8_t* out) {
    if (!raw || !out || h <= 0 || rowbytes <= 0 || bpp <= 0) return GV_E_BADARG;
    const uint8_t* prev = nullptr;
    for (int y = 0; y < h; ++y) {
        const uint8_t* line = raw + (size_t)y * (rowbytes + 1);
        uint8_t* cur = out + (size_t)y * rowbytes;
        const int ft = line[0];
        ++line;
        if (ft > 4) return GV_E_BADARG;
        for (int x = 0; x < rowbytes; ++x) {
            const int a = x >= bpp ? cur[x - bpp] : 0;
            const int b = prev ? prev[x] : 0;
            const int c = (prev && x >= bpp) ? prev[x - bpp] : 0;
            int p = 0;
            if (ft == 1) p = a;
            else if (ft == 2) p = b;
            else if (ft == 3) p = (a + b) >> 1;
            else if (ft == 4) {
                const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
                p = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            }
            cur[x] = (uint8_t)(line[x] + p);
        }
        prev = cur;
    }
    return GV_OK;
}
