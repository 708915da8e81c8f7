// pool.hip — HBM-bound NHWC window ops of the per-view backbone, one kernel template per op for every storage:
//   * max / average pooling (slim.max_pool2d / slim.avg_pool2d: nets/inception_v3.py:112,127,152,
//     219,355; nets/resnet_v2.py:181; `subsample`, nets/resnet_utils.py:64-67)
//   * per-channel scale/shift(+ReLU)  (stand-alone slim.batch_norm, nets/resnet_v2.py:75)
//   * global average pool              (tf.keras GlobalAveragePooling2D, nets/model.py:144,163)
// A kernel reads and writes pixels through accessors (Px: fp32 and 16-bit storage, lp_elem.h; P3Px: the three-plane layout,
// conv_x3_epi.h), its input's and its output's chosen independently.  One thread per (output pixel, N-channel group) with
// 16-byte accesses (N = 4 fp32 or 8 16-bit channels), consecutive lanes on consecutive channels, so every wave instruction
// moves whole 128-byte lines; N = 1 where the operands do not allow it.  Arithmetic is fp32 and an output is rounded to
// its storage type exactly once (max pooling is rounding-free).  Input and output carry an explicit pixel stride so a
// pool can read/write a channel slice of a concat buffer (Mixed_6a / Mixed_7a max-pool branches write straight into the
// block's output).
#include <math.h>

#include "gv_common.h"
#include "conv_x3_epi.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

template <class XA, class YA>
__global__ __launch_bounds__(256) void pool2d(const typename XA::elem* __restrict__ x, typename YA::elem* __restrict__ y,
                                              int nb, int ih, int iw, int c, int x_ld, int kh, int kw, int stride,
                                              int pad_t, int pad_l, int oh, int ow, int y_ld, int mode) {
    constexpr int N = XA::N;
    const int cg = c / N;
    const int64_t total = (int64_t)nb * oh * ow * cg;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(idx % cg);
        const int64_t pix = idx / cg;
        const int ox = (int)(pix % ow);
        const int64_t t = pix / ow;
        const int oy = (int)(t % oh);
        const int n = (int)(t / oh);
        float acc[N];
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = mode == GV_POOL_MAX ? -INFINITY : 0.f;
        int cnt = 0;
        for (int r = 0; r < kh; ++r) {
            const int iy = oy * stride + r - pad_t;
            if ((unsigned)iy >= (unsigned)ih) continue;
            for (int s = 0; s < kw; ++s) {
                const int ix = ox * stride + s - pad_l;
                if ((unsigned)ix >= (unsigned)iw) continue;
                float v[N];
                XA::load(x, (size_t)(n * ih + iy) * iw + ix, x_ld, g * N, v);
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e] = mode == GV_POOL_MAX ? fmaxf(acc[e], v[e]) : acc[e] + v[e];
                ++cnt;
            }
        }
        if (mode != GV_POOL_MAX) {
            const float inv = (float)cnt;             // divisor = number of valid taps (TF SAME semantics)
#pragma unroll
            for (int e = 0; e < N; ++e) {
                acc[e] = acc[e] / inv;
                if (mode == GV_POOL_AVG_RELU) acc[e] = fmaxf(acc[e], 0.f);
            }
        }
        YA::store(y, (size_t)pix, y_ld, g * N, acc);
    }
}

// 3x3 / stride 2 / VALID max pool (MaxPool_3a / 5a and the pooled branches of Mixed_6a / 7a, nets/inception_v3.py:112,127,
// 214,347), RH vertically adjacent outputs of an N-channel group per thread: the window rows 2*oy .. 2*oy + 2 of
// consecutive outputs share a row, so a thread that walks down RH outputs reads 2*RH + 1 input rows instead of 3*RH — and,
// what matters more, the shared rows are not re-fetched by ANOTHER workgroup on another XCD (pool2d: one output per
// thread, L2 hit 0.32, 1.5x the algorithmic bytes from the fabric; r3_pmc / r4_pmc).
// Giving every workgroup one contiguous span of pool2d's index instead was measured and dropped (round 4: the pools
// of a step 1.10 -> 1.25 ms — 4096 spans in flight at once walk 4096 far-apart regions).
template <class A, int RH>
__global__ __launch_bounds__(256) void maxpool3x3s2_rows(const typename A::elem* __restrict__ x,
                                                         typename A::elem* __restrict__ y, int nb, int ih, int iw, int c,
                                                         int x_ld, int oh, int ow, int y_ld) {
    constexpr int N = A::N;
    const int cg = c / N;
    const int nob = (oh + RH - 1) / RH;
    const int64_t total = (int64_t)nb * nob * ow * cg;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(idx % cg);
        int64_t t = idx / cg;
        const int ox = (int)(t % ow);
        t /= ow;
        const int ob = (int)(t % nob);
        const int n = (int)(t / nob);
        const int oy0 = ob * RH;
        const int nr = min(RH, oh - oy0);                          // output rows of this thread
        const auto* xp = A::at(x, (size_t)(n * ih + 2 * oy0) * iw + 2 * ox, x_ld);
        auto* yp = A::at(y, (size_t)(n * oh + oy0) * ow + ox, y_ld);
        float acc[N];
#pragma unroll
        for (int r = 0; r <= 2 * RH; ++r) {
            if (r > 2 * nr) break;                                 // (VALID: input row 2*oy + 2 exists for every oy < oh)
            const auto* rp = A::at(xp, (size_t)r * iw, x_ld);
            float a[N], b[N], d_[N], hm[N];
            A::load(rp, 0, x_ld, g * N, a);
            A::load(rp, 1, x_ld, g * N, b);
            A::load(rp, 2, x_ld, g * N, d_);
#pragma unroll
            for (int e = 0; e < N; ++e) hm[e] = fmaxf(fmaxf(a[e], b[e]), d_[e]);
            if (r == 0) {
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e] = hm[e];
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e] = fmaxf(acc[e], hm[e]);
                if ((r & 1) == 0) {                                // the third row of output r/2 - 1 = the first of output r/2
                    A::store(yp, (size_t)(r / 2 - 1) * ow, y_ld, g * N, acc);
#pragma unroll
                    for (int e = 0; e < N; ++e) acc[e] = hm[e];
                }
            }
        }
    }
}

// (A 4 x 4 block of outputs per thread for the 3x3 / stride-1 AVERAGE pool — 36 loads for 16 outputs instead of the row
// form's 18 for 4 — was measured and dropped in round 4: 0.027 -> 0.038 ms on a Mixed_5 branch, 0.018 -> 0.024 ms on a
// Mixed_6 one: a quarter of the threads and 96 live partial sums each.)

// sum / inv with rcp = 1 / inv, the correctly rounded reciprocal, taken once for several sums: a product and one
// exact-remainder correction (Markstein) — the correctly rounded quotient, i.e. the bits of the division, at 3 instead of
// ~10 instructions per value — for a FINITE sum; a non-finite one keeps sum * rcp (inf stays inf, NaN stays NaN, as the
// division gives; the correction would turn inf into NaN)
__device__ __forceinline__ float div_by_rcp(float sum, float inv, float rcp) {
    const float q0 = sum * rcp;
    const float qc = __builtin_fmaf(__builtin_fmaf(-inv, q0, sum), rcp, q0);
    return __builtin_fabsf(q0) < __builtin_inff() ? qc : q0;
}

// ROWS x 4 outputs (rows oy0 .., columns ox0 ..) of one N-channel group from a (ROWS + 2) x 6 input patch: the column sums
// are shared by the outputs of a row, and an input row by the output rows it serves.  Per output the same additions in the
// same order for every ROWS: per column the valid rows ascending, then (col[j] + col[j+1]) + col[j+2].
template <class XA, class YA, int ROWS>
__device__ __forceinline__ void avgpool3x3s1_tile(const typename XA::elem* __restrict__ x, typename YA::elem* __restrict__ y,
                                                  int n, int oy0, int ox0, int ch, int ih, int iw, int x_ld, int y_ld,
                                                  int relu) {
    constexpr int N = XA::N;
    float col[ROWS][6][N];
#pragma unroll
    for (int q = 0; q < ROWS; ++q)
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int e = 0; e < N; ++e) col[q][j][e] = 0.f;
#pragma unroll
    for (int r = -1; r <= ROWS; ++r) {
        const int iy = oy0 + r;
        if ((unsigned)iy >= (unsigned)ih) continue;
        const auto* xr = XA::at(x, (size_t)(n * ih + iy) * iw, x_ld);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int ix = ox0 - 1 + j;
            if ((unsigned)ix >= (unsigned)iw) continue;
            float v[N];
            XA::load(xr, ix, x_ld, ch, v);
#pragma unroll
            for (int q = 0; q < ROWS; ++q)
                if (r >= q - 1 && r <= q + 1) {
#pragma unroll
                    for (int e = 0; e < N; ++e) col[q][j][e] += v[e];
                }
        }
    }
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
        const int oy = oy0 + q;
        if (oy >= ih) break;
        const int rows = 1 + (oy > 0 ? 1 : 0) + (oy + 1 < ih ? 1 : 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = ox0 + j;
            if (ox >= iw) break;
            const int cols = 1 + (ox > 0 ? 1 : 0) + (ox + 1 < iw ? 1 : 0);
            const float inv = (float)(rows * cols);           // valid taps only (TF SAME semantics)
            const float rcp = 1.0f / inv;
            float v[N];
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const float sum = col[q][j][e] + col[q][j + 1][e] + col[q][j + 2][e];
                // (the divisions were most of the two-row form's vector instructions; the one-row form keeps them)
                v[e] = ROWS == 2 ? div_by_rcp(sum, inv, rcp) : sum / inv;
                if (relu) v[e] = fmaxf(v[e], 0.f);
            }
            YA::store(y, (size_t)(n * ih + oy) * iw + ox, y_ld, ch, v);
        }
    }
}

// 3x3 / stride 1 / SAME average pool (slim.avg_pool2d under the Inception arg-scope, nets/inception_v3.py:152,...): 18
// 16-byte loads for 4 outputs instead of 36 — the generic kernel is L2-request bound on this op (2.4 TB/s).
// ROWS = 1: a grid-stride loop.  ROWS = 2: rows oy and oy + 1 of a pair are loaded once, and workgroups are mapped so that
// an XCD owns a contiguous range of them — the rows two outputs share are then in ITS L2 (under round-robin dispatch
// vertical neighbours sat on different XCDs: c5's nine pooled branches fetched 3.9 x their input from beyond L2, the pooled
// branches of c2 3.5 x at an L2 hit rate of 0.28); launched with exactly ceil(total / 256) workgroups.
template <class XA, class YA, int ROWS>
__global__ __launch_bounds__(256) void avgpool3x3s1_rows(const typename XA::elem* __restrict__ x,
                                                         typename YA::elem* __restrict__ y, int nb, int ih, int iw, int c,
                                                         int x_ld, int y_ld, int relu) {
    constexpr int N = XA::N;
    const int cg = c / N, wg = (iw + 3) >> 2, hg = (ih + ROWS - 1) / ROWS;
    const int64_t total = (int64_t)nb * hg * wg * cg;
    const auto tile = [&](int64_t idx) {
        const int g = (int)(idx % cg);
        int64_t t = idx / cg;
        const int xg = (int)(t % wg);
        t /= wg;
        const int yg = (int)(t % hg);
        const int n = (int)(t / hg);
        avgpool3x3s1_tile<XA, YA, ROWS>(x, y, n, yg * ROWS, xg * 4, g * N, ih, iw, x_ld, y_ld, relu);
    };
    if constexpr (ROWS == 2) {
        const int64_t idx = (int64_t)gv_xcd_remap((int)blockIdx.x, (int)gridDim.x) * 256 + threadIdx.x;
        if (idx < total) tile(idx);
    } else {
        for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
             idx += (int64_t)gridDim.x * blockDim.x)
            tile(idx);
    }
}

template <class A>
__global__ __launch_bounds__(256) void scale_shift_act(const typename A::elem* __restrict__ x, int64_t npix, int c, int x_ld,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       int relu, typename A::elem* __restrict__ y, int y_ld) {
    constexpr int N = A::N;
    const int cg = c / N;
    const int64_t total = npix * cg;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(idx % cg);
        const int64_t pix = idx / cg;
        float v[N];
        A::load(x, (size_t)pix, x_ld, g * N, v);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            v[e] = v[e] * scale[g * N + e] + shift[g * N + e];
            if (relu) v[e] = fmaxf(v[e], 0.f);
        }
        A::store(y, (size_t)pix, y_ld, g * N, v);
    }
}

// y[b][c] = mean_p x[b][p][c]; thread per (b, c): lanes walk consecutive channels.
template <typename E, typename T>
__global__ __launch_bounds__(256) void global_avg_pool(const E* __restrict__ x, int nb, int hw, int c, int x_ld,
                                                       float* __restrict__ y) {
    const int64_t total = (int64_t)nb * c;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c);
    const int b = (int)(idx / c);
    const E* p = x + (size_t)b * hw * x_ld + ch;
    float s = 0.f;
    for (int i = 0; i < hw; ++i) s += up<T>(p[(size_t)i * x_ld]);
    y[idx] = s / (float)hw;
}

}  // namespace

// train_data.py:63,81-84,101: legacy bilinear resize + flips + brightness + x/255 - 0.5; thread per output pixel
__global__ __launch_bounds__(256) void preprocess_views_kernel(const unsigned char* __restrict__ src, int nimg, int h0,
                                                               int w0, int H, int W, const int* __restrict__ flip,
                                                               const float* __restrict__ delta,
                                                               float* __restrict__ dst) {
    const int64_t total = (int64_t)nimg * H * W;
    const float sy = (float)h0 / (float)H, sx = (float)w0 / (float)W;        // resize_images: scale = in / out
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const int64_t t = idx / W;
        const int y = (int)(t % H);
        const int img = (int)(t / H);
        const int f = flip ? flip[img] : 0;
        const int xr = (f & 1) ? W - 1 - x : x;                               // a flip of the resized image
        const int yr = (f & 2) ? H - 1 - y : y;
        const float fy = __fmul_rn((float)yr, sy), fx = __fmul_rn((float)xr, sx);
        const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
        const int y1 = min(y0 + 1, h0 - 1), x1 = min(x0 + 1, w0 - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const unsigned char* p = src + (size_t)img * h0 * w0 * 3;
        const float d = delta ? delta[img] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float tl = p[((size_t)y0 * w0 + x0) * 3 + c], tr = p[((size_t)y0 * w0 + x1) * 3 + c];
            const float bl = p[((size_t)y1 * w0 + x0) * 3 + c], br = p[((size_t)y1 * w0 + x1) * 3 + c];
            const float top = __fadd_rn(tl, __fmul_rn(tr - tl, lx));
            const float bot = __fadd_rn(bl, __fmul_rn(br - bl, lx));
            float v = __fadd_rn(top, __fmul_rn(bot - top, ly));
            v = __fadd_rn(v, d);
            dst[idx * 3 + c] = __fadd_rn(__fmul_rn(v, 1.0f / 255.0f), -0.5f);
        }
    }
}

extern "C" int gv_preprocess_views(const uint8_t* src, int32_t nimg, int32_t h0, int32_t w0, int32_t height,
                                   int32_t width, const int32_t* flip, const float* delta, float* dst,
                                   void* stream) {
    if (!src || !dst || nimg <= 0 || h0 <= 0 || w0 <= 0 || height <= 0 || width <= 0) return GV_E_BADARG;
    const int64_t total = (int64_t)nimg * height * width;
    hipLaunchKernelGGL(preprocess_views_kernel, dim3(gv_grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, nimg, h0,
                       w0, height, width, flip, delta, dst);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

namespace {

int g_pool_rows = 1;      // multi-row form of the 3x3 / stride-2 max pool (gv_pool2d_set_rows: 0 = one output per thread; A/B)

// The kernel form that serves a pool, and the channels a thread owns in it.
enum PoolKind { POOL_GENERIC, POOL_AVG_ROWS1, POOL_AVG_ROWS2, POOL_MAX_ROWS };
struct PoolForm {
    PoolKind kind;
    int n;                // 1: the scalar walk; 4 (fp32 values) / 8 (16-bit storage; the two-row form on three planes): 16-byte accesses
};
// mode without the three-plane bits; vec: c, both pixel strides and both bases allow the 16-byte walk of the storage
// (always so for a three-plane operand: the entry point rejects the others); max_rows: gv_pool2d_set_rows
PoolForm pool_form(const gv_pool_desc* d, int mode, bool xp3, bool yp3, bool vec, bool max_rows) {
    const int n = !vec ? 1 : d->dtype == GV_F32 ? 4 : 8;
    const bool k3 = d->kh == 3 && d->kw == 3;
    if (vec && mode != GV_POOL_MAX && k3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->oh == d->ih &&
        d->ow == d->iw) {
        // two rows per thread, XCD-contiguous workgroups: 16-bit storage, and three-plane input in whole 8-channel chunks
        const int64_t blk2 = ((int64_t)d->nb * ((d->ih + 1) / 2) * ((d->iw + 3) / 4) * (d->c / 8) + 255) / 256;
        if ((d->dtype != GV_F32 || (xp3 && d->c % 8 == 0)) && blk2 < 0x7fffffff) return {POOL_AVG_ROWS2, 8};
        return {POOL_AVG_ROWS1, n};
    }
    if (vec && max_rows && !xp3 && !yp3 && mode == GV_POOL_MAX && k3 && d->stride == 2 && d->pad_t == 0 && d->pad_l == 0 &&
        d->oh == (d->ih - 3) / 2 + 1 && d->ow == (d->iw - 3) / 2 + 1)
        return {POOL_MAX_ROWS, n};
    return {POOL_GENERIC, n};
}

template <class XA, class YA>
int launch_pool2d(const gv_pool_desc* d, int mode, const void* x, void* y, hipStream_t st) {
    const int64_t total = (int64_t)d->nb * d->oh * d->ow * (d->c / XA::N);
    return gv_launch<pool2d<XA, YA>>(dim3(gv_grid_for(total)), dim3(256), 0, st, (const typename XA::elem*)x,
                                     (typename YA::elem*)y, d->nb, d->ih, d->iw, d->c, d->x_ld, d->kh, d->kw, d->stride,
                                     d->pad_t, d->pad_l, d->oh, d->ow, d->y_ld, mode);
}

template <class XA, class YA, int ROWS>
int launch_avg_rows(const gv_pool_desc* d, int mode, const void* x, void* y, hipStream_t st) {
    const int64_t total = (int64_t)d->nb * ((d->ih + ROWS - 1) / ROWS) * ((d->iw + 3) / 4) * (d->c / XA::N);
    const dim3 grid(ROWS == 2 ? (unsigned)((total + 255) / 256) : gv_grid_for(total));
    return gv_launch<avgpool3x3s1_rows<XA, YA, ROWS>>(grid, dim3(256), 0, st, (const typename XA::elem*)x,
                                                      (typename YA::elem*)y, d->nb, d->ih, d->iw, d->c, d->x_ld, d->y_ld,
                                                      mode == GV_POOL_AVG_RELU ? 1 : 0);
}

template <class A>
int launch_max_rows(const gv_pool_desc* d, const void* x, void* y, hipStream_t st) {
    constexpr int RH = 4;
    const int64_t total = (int64_t)d->nb * ((d->oh + RH - 1) / RH) * d->ow * (d->c / A::N);
    return gv_launch<maxpool3x3s2_rows<A, RH>>(dim3(gv_grid_for(total)), dim3(256), 0, st, (const typename A::elem*)x,
                                               (typename A::elem*)y, d->nb, d->ih, d->iw, d->c, d->x_ld, d->oh, d->ow,
                                               d->y_ld);
}

template <class A>
int launch_ssa(const void* x, int64_t npix, int c, int x_ld, const float* scale, const float* shift, int relu, void* y,
               int y_ld, void* stream) {
    return gv_launch<scale_shift_act<A>>(dim3(gv_grid_for(npix * (c / A::N))), dim3(256), 0, (hipStream_t)stream,
                                         (const typename A::elem*)x, npix, c, x_ld, scale, shift, relu,
                                         (typename A::elem*)y, y_ld);
}

// fp32 values with three-plane input and / or output, 4 channels per thread: XA / YA the accessors of the two sides
#define GV_P3_DISPATCH(xp3, yp3, CALL)                                              \
    do {                                                                            \
        using P = P3Px<4>;                                                          \
        using Q = Px<float, float, 4>;                                              \
        if ((xp3) && (yp3)) { using XA = P; using YA = P; CALL; }                   \
        if (xp3) { using XA = P; using YA = Q; CALL; }                              \
        { using XA = Q; using YA = P; CALL; }                                       \
    } while (0)

}  // namespace

extern "C" void gv_pool2d_set_rows(int on) { g_pool_rows = on; }

extern "C" int gv_pool2d_fwd(const gv_pool_desc* d, const void* x, void* y, void* stream) {
    if (!d || !x || !y) return GV_E_BADARG;
    if (d->nb <= 0 || d->ih <= 0 || d->iw <= 0 || d->c <= 0 || d->kh <= 0 || d->kw <= 0 ||
        d->stride <= 0 || d->oh <= 0 || d->ow <= 0 || d->pad_t < 0 || d->pad_l < 0)
        return GV_E_BADARG;
    if (d->x_ld < d->c || d->y_ld < d->c) return GV_E_BADARG;
    if (!gv_pool_geometry_ok(d)) return GV_E_BADARG;             // (every dtype and storage form: checked before any branch)
    const bool xp3 = (d->mode & GV_POOL_X_P3) != 0, yp3 = (d->mode & GV_POOL_Y_P3) != 0, p3 = xp3 || yp3;
    const int mode = d->mode & ~(GV_POOL_X_P3 | GV_POOL_Y_P3);
    if (mode != GV_POOL_MAX && mode != GV_POOL_AVG && mode != GV_POOL_AVG_RELU) return GV_E_BADARG;
    // three-plane input and / or output (fp32 values, GV_MATH_BF16X3 plans): nothing but the 4-channel walk
    if (p3 && (d->dtype != GV_F32 || d->c % 4 != 0 || !gv_aligned16(x) || !gv_aligned16(y) ||
               (xp3 ? d->x_ld % 16 != 0 : d->x_ld % 4 != 0) || (yp3 ? d->y_ld % 16 != 0 : d->y_ld % 4 != 0)))
        return GV_E_UNSUPPORTED;
    const int quad = d->dtype == GV_F32 ? 4 : 8;
    const bool vec = p3 || (d->c % quad == 0 && gv_vec_ok(x, d->x_ld, quad) && gv_vec_ok(y, d->y_ld, quad));
    const PoolForm f = pool_form(d, mode, xp3, yp3, vec, g_pool_rows != 0);
    hipStream_t st = (hipStream_t)stream;
    switch (f.kind) {
    case POOL_AVG_ROWS2:
        if (xp3 && yp3) return launch_avg_rows<P3Px<8>, P3Px<8>, 2>(d, mode, x, y, st);
        if (xp3) return launch_avg_rows<P3Px<8>, Px<float, float, 8>, 2>(d, mode, x, y, st);
        GV_LP_DISPATCH(d->dtype, return (launch_avg_rows<Px<unsigned short, T, 8>, Px<unsigned short, T, 8>, 2>(d, mode, x, y, st)));
    case POOL_AVG_ROWS1:
        if (p3) GV_P3_DISPATCH(xp3, yp3, return (launch_avg_rows<XA, YA, 1>(d, mode, x, y, st)));
        GV_ST_DISPATCH(d->dtype, return (launch_avg_rows<Px<E, T, 16 / sizeof(E)>, Px<E, T, 16 / sizeof(E)>, 1>(d, mode, x, y, st)));
    case POOL_MAX_ROWS:
        GV_ST_DISPATCH(d->dtype, return (launch_max_rows<Px<E, T, 16 / sizeof(E)>>(d, x, y, st)));
    case POOL_GENERIC:
        break;
    }
    if (p3) GV_P3_DISPATCH(xp3, yp3, return (launch_pool2d<XA, YA>(d, mode, x, y, st)));
    if (f.n == 1) GV_ST_DISPATCH(d->dtype, return (launch_pool2d<Px<E, T, 1>, Px<E, T, 1>>(d, mode, x, y, st)));
    GV_ST_DISPATCH(d->dtype, return (launch_pool2d<Px<E, T, 16 / sizeof(E)>, Px<E, T, 16 / sizeof(E)>>(d, mode, x, y, st)));
}

extern "C" int gv_scale_shift_act(const void* x, int64_t npix, int32_t c, int32_t x_ld,
                                  const float* scale, const float* shift, int32_t relu, void* y,
                                  int32_t y_ld, int32_t dtype, void* stream) {
    if (!x || !y || !scale || !shift || npix <= 0 || c <= 0 || x_ld < c || y_ld < c) return GV_E_BADARG;
    const int quad = dtype == GV_F32 ? 4 : 8;
    // (fp32 storage takes the 16-byte walk only with 16-byte aligned coefficient rows as well)
    const bool vec = c % quad == 0 && gv_vec_ok(x, x_ld, quad) && gv_vec_ok(y, y_ld, quad) &&
                     (dtype != GV_F32 || (gv_aligned16(scale) && gv_aligned16(shift)));
    if (vec)
        GV_ST_DISPATCH(dtype, return (launch_ssa<Px<E, T, 16 / sizeof(E)>>(x, npix, c, x_ld, scale, shift, relu, y, y_ld, stream)));
    GV_ST_DISPATCH(dtype, return (launch_ssa<Px<E, T, 1>>(x, npix, c, x_ld, scale, shift, relu, y, y_ld, stream)));
}

extern "C" int gv_global_avg_pool(const void* x, int32_t nb, int32_t hw, int32_t c, int32_t x_ld,
                                  float* y, int32_t dtype, void* stream) {
    if (!x || !y || nb <= 0 || hw <= 0 || c <= 0 || x_ld < c) return GV_E_BADARG;
    const dim3 grid((unsigned)(((int64_t)nb * c + 255) / 256));
    GV_ST_DISPATCH(dtype, return (gv_launch<global_avg_pool<E, T>>(grid, dim3(256), 0, (hipStream_t)stream, (const E*)x, nb, hw,
                                                                   c, x_ld, y)));
}
