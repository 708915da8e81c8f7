// pool_train.hip — the pooling ops of the training step for every storage type: the backward pass of max / average
// pooling, and the forward max pool that records its winners.  Pixels are read and written through Px (lp_elem.h): one
// thread per N-channel group with 16-byte accesses (N = 4 fp32 or 8 16-bit channels) where the operands allow, else N = 1.
// The backward pass is a GATHER over the input pixels (no atomics: 16-bit storage has none worth using, and the result is
// deterministic): an input pixel folds, from +0 and in window order (oy ascending, then ox), the gradients of the windows
// that elected it, and the sum is rounded to the storage type once.  Which pixel a window elects is the kernels' Win:
//   Recomputed   the window's first maximum in row-major tap order, found again from x (tf MaxPoolGrad / torch)
//   Recorded     the tap byte r * kw + s the forward pass wrote ([nb, oh, ow, c] dense): no input re-read, no compare chain
//   Average      every pixel of the window, with dy / #valid taps
// train.hip holds the extern "C" entry points.
#include <math.h>

#include <type_traits>

#include "lowp.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

enum Win { Recomputed, Recorded, Average };

// The tap bytes of N consecutive channels <-> registers: one 4- or 8-byte word where a thread owns a quad of channels.
template <int N>
struct ArgBytes {
    static constexpr int W = N < 4 ? 1 : N / 4;
    static __device__ __forceinline__ void load(const unsigned char* p, int (&a)[N]) {
        if constexpr (N == 1) {
            a[0] = p[0];
        } else {
            unsigned w[W];
            if constexpr (N == 8) {
                const uint2 v = *reinterpret_cast<const uint2*>(p);
                w[0] = v.x; w[1] = v.y;
            } else {
                w[0] = *reinterpret_cast<const unsigned*>(p);
            }
#pragma unroll
            for (int e = 0; e < N; ++e) a[e] = (w[e / 4] >> (8 * (e % 4))) & 0xff;
        }
    }
    static __device__ __forceinline__ void store(unsigned char* p, const int (&a)[N]) {
        if constexpr (N == 1) {
            p[0] = (unsigned char)a[0];
        } else {
            unsigned w[W];
#pragma unroll
            for (int q = 0; q < W; ++q)
                w[q] = (unsigned)a[4 * q] | ((unsigned)a[4 * q + 1] << 8) | ((unsigned)a[4 * q + 2] << 16) |
                       ((unsigned)a[4 * q + 3] << 24);
            if constexpr (N == 8) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
            else *reinterpret_cast<unsigned*>(p) = w[0];
        }
    }
};

// Forward: y = max over the window AND, per output element, the row-major tap index of the FIRST maximum (one byte).
// (Not pool2d of pool.hip: that one's fmaxf skips a NaN tap, `v > best` here keeps a leading one.)
template <class A>
__global__ __launch_bounds__(256) void maxpool_argmax_fwd(const typename A::elem* __restrict__ x, int x_ld, int nb, int ih,
                                                          int iw, int c, int kh, int kw, int stride, int pad_t, int pad_l,
                                                          int oh, int ow, typename A::elem* __restrict__ y, int y_ld,
                                                          unsigned char* __restrict__ arg) {
    constexpr int N = A::N;
    const int cg = c / N;
    const int64_t total = (int64_t)nb * oh * ow * cg;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(idx % cg);
        const int64_t opix = idx / cg;
        const int ox = (int)(opix % ow);
        const int64_t t = opix / ow;
        const int oy = (int)(t % oh);
        const int n = (int)(t / oh);
        float best[N];
        int a[N];
#pragma unroll
        for (int e = 0; e < N; ++e) { best[e] = -INFINITY; a[e] = -1; }
        for (int r = 0; r < kh; ++r) {
            const int yy = oy * stride - pad_t + r;
            if ((unsigned)yy >= (unsigned)ih) continue;
            for (int s = 0; s < kw; ++s) {
                const int xx = ox * stride - pad_l + s;
                if ((unsigned)xx >= (unsigned)iw) continue;
                float v[N];
                A::load(x, (size_t)(n * ih + yy) * iw + xx, x_ld, q * N, v);
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (v[e] > best[e] || a[e] < 0) { best[e] = v[e]; a[e] = r * kw + s; }
            }
        }
        A::store(y, (size_t)opix, y_ld, q * N, best);
        ArgBytes<N>::store(arg + opix * c + q * N, a);
    }
}

// The tail of both backward kernels: dx = +0 + sum (store) or dx += sum, rounded once.
template <class A>
__device__ __forceinline__ void put_grad(typename A::elem* dx, size_t pix, int dx_ld, int ch, int store,
                                         const float (&sum)[A::N]) {
    float d[A::N];
    if (store) {
#pragma unroll
        for (int e = 0; e < A::N; ++e) d[e] = 0.f;
    } else {
        A::load(dx, pix, dx_ld, ch, d);
    }
#pragma unroll
    for (int e = 0; e < A::N; ++e) d[e] += sum[e];
    A::store(dx, pix, dx_ld, ch, d);
}

// Any window: one input pixel x N channels per thread, the windows that contain it.  A pixel no window covers is zero in
// the store form and left alone in the accumulate form.
template <class A, Win W>
__global__ __launch_bounds__(256) void pool_bwd_gather(const typename A::elem* __restrict__ x, int x_ld,
                                                       const unsigned char* __restrict__ arg,
                                                       const typename A::elem* __restrict__ dy, int dy_ld, int nb, int ih,
                                                       int iw, int c, int kh, int kw, int stride, int pad_t, int pad_l,
                                                       int oh, int ow, int store, typename A::elem* __restrict__ dx,
                                                       int dx_ld) {
    constexpr int N = A::N;
    const int cg = c / N;
    const int64_t total = (int64_t)nb * ih * iw * cg;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(idx % cg);
        const int64_t pix = idx / cg;
        const int ix = (int)(pix % iw);
        const int64_t t = pix / iw;
        const int iy = (int)(t % ih);
        const int n = (int)(t / ih);
        // windows (oy, ox) with oy*stride <= py <= oy*stride + kh - 1: from ceil((py - kh + 1) / stride) to py / stride
        const int py = iy + pad_t, px = ix + pad_l;
        const int oy_hi = min(oh - 1, py / stride), ox_hi = min(ow - 1, px / stride);
        const int oy_lo = py - kh + 1 <= 0 ? 0 : (py - kh + stride) / stride;
        const int ox_lo = px - kw + 1 <= 0 ? 0 : (px - kw + stride) / stride;
        float sum[N];
#pragma unroll
        for (int e = 0; e < N; ++e) sum[e] = 0.f;
        if (oy_lo > oy_hi || ox_lo > ox_hi) {
            if (store) A::store(dx, (size_t)pix, dx_ld, q * N, sum);
            continue;
        }
        float mine[N];
        if constexpr (W == Recomputed) A::load(x, (size_t)pix, x_ld, q * N, mine);
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const size_t opix = (size_t)(n * oh + oy) * ow + ox;
                float g[N];
                A::load(dy, opix, dy_ld, q * N, g);
                if constexpr (W == Average) {
                    int cnt = 0;
                    for (int r = 0; r < kh; ++r) {
                        if ((unsigned)(oy * stride + r - pad_t) >= (unsigned)ih) continue;
                        for (int s = 0; s < kw; ++s) cnt += (unsigned)(ox * stride + s - pad_l) < (unsigned)iw;
                    }
                    // (spelled as the FMA `sum += g * rc` contracts to: which lanes the compiler contracts is then not its choice)
                    const float rc = 1.f / (float)cnt;
#pragma unroll
                    for (int e = 0; e < N; ++e) sum[e] = fmaf(g[e], rc, sum[e]);
                } else {
                    bool win[N];
                    if constexpr (W == Recorded) {
                        const int tap = (py - oy * stride) * kw + (px - ox * stride);
                        int a[N];
                        ArgBytes<N>::load(arg + opix * c + q * N, a);
#pragma unroll
                        for (int e = 0; e < N; ++e) win[e] = a[e] == tap;
                    } else {
                        // this pixel wins when no earlier tap is >= it and no later tap is > it
#pragma unroll
                        for (int e = 0; e < N; ++e) win[e] = true;
                        bool before = true;
                        for (int r = 0; r < kh; ++r) {
                            const int yy = oy * stride + r - pad_t;
                            if ((unsigned)yy >= (unsigned)ih) continue;
                            for (int s = 0; s < kw; ++s) {
                                const int xx = ox * stride + s - pad_l;
                                if ((unsigned)xx >= (unsigned)iw) continue;
                                if (yy == iy && xx == ix) { before = false; continue; }
                                float v[N];
                                A::load(x, (size_t)(n * ih + yy) * iw + xx, x_ld, q * N, v);
#pragma unroll
                                for (int e = 0; e < N; ++e)
                                    win[e] = win[e] && (before ? !(v[e] >= mine[e]) : !(v[e] > mine[e]));
                            }
                        }
                    }
#pragma unroll
                    for (int e = 0; e < N; ++e) sum[e] += win[e] ? g[e] : 0.f;
                }
            }
        }
        put_grad<A>(dx, (size_t)pix, dx_ld, q * N, store, sum);
    }
}

// BnTail (z != nullptr, recorded winners only): the max pool follows relu(BN_train(z)) and pools z itself (BN + ReLU with
// a positive scale are monotone: max(relu(bn(z))) = relu(bn(max z)), same winner) — the gradient the kernel below gathers
// is then the gradient of the BatchNorm's OUTPUT at that pixel, and instead of storing it the kernel finishes the
// BatchNorm backward pass: dz = A*g + B*z + C with g = dy*[z*scale + shift > 0] and the per-(group, channel) coefficients
// of gv_bn_bwd_coeffs_t.  The activation y and its gradient are never materialised at the un-pooled size.
struct BnTail {
    const void* z;
    int z_ld, G;
    const float *A, *B, *C, *scale, *shift;                          // [G][c]
};

// 3x3 / stride 2 windows that start at even pixels (every max pool of Inception-v3; ResNet-v2's pool1): a thread owns the
// 2x2 input pixels (2a..2a+1, 2b..2b+1) x N channels and visits the four windows (a-1..a, b-1..b) that touch them ONCE
// each; the gradient goes to whichever of the thread's pixels is the window's winner.  Recomputed: the argmax of the
// window's nine taps, all of which must exist (VALID) — 11 loads per input pixel instead of the gather's 23.  Recorded: 2
// loads per input pixel, and the kernel only asks which windows exist, so a clipped last window (TF's SAME on an even
// map) is served too.  One image's work fits 32 bits: checked by the launcher.  BN: with the BatchNorm tail — a kernel of
// its own, because as a run-time branch it cost the plain kernel its registers (16-bit quads: 122 VGPRs against 72).
template <class A, Win W, bool BN>
__global__ __launch_bounds__(256) void maxpool3s2_bwd(const typename A::elem* __restrict__ x, int x_ld,
                                                      const unsigned char* __restrict__ arg,
                                                      const typename A::elem* __restrict__ dy, int dy_ld, int nb, int ih,
                                                      int iw, int c, int oh, int ow, int store,
                                                      typename A::elem* __restrict__ dx, int dx_ld, BnTail bn) {
    using E = typename A::elem;
    constexpr int N = A::N;
    const int cg = c / N, ah = (ih + 1) / 2, aw = (iw + 1) / 2;
    const int64_t total = (int64_t)nb * ah * aw * cg;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const unsigned per_img = (unsigned)(ah * aw * cg);
        const int n = (int)(idx / per_img);
        unsigned t = (unsigned)(idx - (int64_t)n * per_img);
        const int q = (int)(t % (unsigned)cg);
        t /= (unsigned)cg;
        const int b = (int)(t % (unsigned)aw);
        const int a = (int)(t / (unsigned)aw);
        float sum[4][N];                                         // [2*py + px of the 2x2 block]
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < N; ++e) sum[k][e] = 0.f;
#pragma unroll
        for (int wy = 0; wy < 2; ++wy) {
#pragma unroll
            for (int wx = 0; wx < 2; ++wx) {
                const int oy = a - 1 + wy, ox = b - 1 + wx;
                if ((unsigned)oy >= (unsigned)oh || (unsigned)ox >= (unsigned)ow) continue;
                const size_t opix = (size_t)(n * oh + oy) * ow + ox;
                int am[N];
                if constexpr (W == Recorded) {
                    ArgBytes<N>::load(arg + opix * c + q * N, am);
                } else {
                    float best[N];
#pragma unroll
                    for (int e = 0; e < N; ++e) { best[e] = -INFINITY; am[e] = -1; }
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        const int yy = 2 * oy + tap / 3, xx = 2 * ox + tap % 3;
                        float v[N];
                        A::load(x, (size_t)(n * ih + yy) * iw + xx, x_ld, q * N, v);
#pragma unroll
                        for (int e = 0; e < N; ++e)
                            if (v[e] > best[e] || am[e] < 0) { best[e] = v[e]; am[e] = tap; }
                    }
                }
                float g[N];
                A::load(dy, opix, dy_ld, q * N, g);
                // the thread's pixel (2a+py, 2b+px) is tap (2a+py-2oy, 2b+px-2ox) = (py + 2*(1-wy), px + 2*(1-wx))
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        const int tr = py + 2 * (1 - wy), tc = px + 2 * (1 - wx);
                        if (tr > 2 || tc > 2) continue;
                        const int tap = tr * 3 + tc;
#pragma unroll
                        for (int e = 0; e < N; ++e) sum[2 * py + px][e] += am[e] == tap ? g[e] : 0.f;
                    }
            }
        }
        [[maybe_unused]] float cA[N], cB[N], cC[N], cs[N], ch_[N];
        if constexpr (BN) {
            const int gi = (n % bn.G) * c + q * N;
            auto ld = [&](const float* p, float* o) {                // (c % N == 0 and 16-byte aligned tables: vector loads)
                if constexpr (N % 4 == 0) {
#pragma unroll
                    for (int e = 0; e < N; e += 4) {
                        const float4 v = *reinterpret_cast<const float4*>(p + gi + e);
                        o[e] = v.x; o[e + 1] = v.y; o[e + 2] = v.z; o[e + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < N; ++e) o[e] = p[gi + e];
                }
            };
            ld(bn.A, cA); ld(bn.B, cB); ld(bn.C, cC);
            if (bn.scale) { ld(bn.scale, cs); ld(bn.shift, ch_); }
            else {
#pragma unroll
                for (int e = 0; e < N; ++e) { cs[e] = 0.f; ch_[e] = 1.f; }
            }
        }
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const int iy = 2 * a + py, ix = 2 * b + px;
                if (iy >= ih || ix >= iw) continue;
                const size_t pix = (size_t)(n * ih + iy) * iw + ix;
                if constexpr (BN) {                              // dz = A*g + B*z + C, stored
                    float zv[N], d[N];
                    A::load(reinterpret_cast<const E*>(bn.z), pix, bn.z_ld, q * N, zv);
#pragma unroll
                    for (int e = 0; e < N; ++e) {
                        const float g = fmaf(zv[e], cs[e], ch_[e]) > 0.f ? sum[2 * py + px][e] : 0.f;
                        d[e] = fmaf(cA[e], g, fmaf(cB[e], zv[e], cC[e]));
                    }
                    A::store(dx, pix, dx_ld, q * N, d);
                } else {
                    put_grad<A>(dx, pix, dx_ld, q * N, store, sum[2 * py + px]);
                }
            }
    }
}

// c and every operand (nullptr: not used) can be walked in 16-byte quads, and so can the tap bytes (one per channel)
bool pool_quads(const gv_pool_desc* d, const void* p0, int ld0, const void* p1, int ld1, const void* p2, int ld2,
                const unsigned char* arg) {
    const int quad = d->dtype == GV_F32 ? 4 : 8;
    return d->c % quad == 0 && gv_vec_ok(p0, ld0, quad) && gv_vec_ok(p1, ld1, quad) && gv_vec_ok(p2, ld2, quad) &&
           (((uintptr_t)arg) & (uintptr_t)(quad - 1)) == 0;
}

// The kernel that serves a backward pool, and the channels a thread owns in it.
enum PoolBwdKind { POOL_BWD_GATHER, POOL_BWD_BLOCK, POOL_BWD_NONE };
struct PoolBwdForm {
    PoolBwdKind kind;
    int n;                // 1: the scalar walk; 4 (fp32) / 8 (16-bit storage): 16-byte accesses
};
// recorded: the winners are tap bytes; vec: pool_quads.  The 2x2-block kernel serves 3x3 / 2 windows that start at even
// pixels.  Recomputed winners: VALID only (all nine taps exist) and only with quads, anything else is the gather's.
// Recorded winners: also TF's SAME on an even map (pads (0, 1): the last window is clipped), at any width; an image
// beyond the kernel's 32-bit index is then served by nothing.
PoolBwdForm pool_bwd_form(const gv_pool_desc* d, bool recorded, bool vec) {
    const int n = !vec ? 1 : d->dtype == GV_F32 ? 4 : 8;
    const bool max3s2 = (d->mode & ~GV_POOL_BWD_STORE) == GV_POOL_MAX && d->kh == 3 && d->kw == 3 && d->stride == 2 &&
                        d->pad_t == 0 && d->pad_l == 0;
    const bool valid_h = d->oh == (d->ih - 3) / 2 + 1, valid_w = d->ow == (d->iw - 3) / 2 + 1;
    const bool same_h = d->ih % 2 == 0 && d->oh == d->ih / 2, same_w = d->iw % 2 == 0 && d->ow == d->iw / 2;
    const bool fits = (int64_t)((d->ih + 1) / 2) * ((d->iw + 1) / 2) * d->c <= 0x7fffffff;
    if (recorded) {
        if (!(max3s2 && (valid_h || same_h) && (valid_w || same_w))) return {POOL_BWD_GATHER, n};
        return {fits ? POOL_BWD_BLOCK : POOL_BWD_NONE, n};
    }
    return {max3s2 && valid_h && valid_w && vec && fits ? POOL_BWD_BLOCK : POOL_BWD_GATHER, n};
}

struct PoolBwdArgs {
    const gv_pool_desc* d;
    const void* x;                                                   // Recomputed
    const unsigned char* arg;                                        // Recorded
    const void* dy;
    int dy_ld;
    void* dx;
    int dx_ld;
    BnTail bn;
};

template <class A, Win W>
int launch_pool_bwd(PoolBwdKind kind, const PoolBwdArgs& a, hipStream_t st) {
    using E = typename A::elem;
    const gv_pool_desc* d = a.d;
    const int store = (d->mode & GV_POOL_BWD_STORE) ? 1 : 0;
    if constexpr (W != Average) {
        if (kind == POOL_BWD_BLOCK) {
            const int64_t total = (int64_t)d->nb * ((d->ih + 1) / 2) * ((d->iw + 1) / 2) * (d->c / A::N);
            const auto go = [&](auto tail) {
                return gv_launch<maxpool3s2_bwd<A, W, decltype(tail)::value>>(
                    dim3(gv_grid_for(total)), dim3(256), 0, st, (const E*)a.x, d->x_ld, a.arg, (const E*)a.dy, a.dy_ld, d->nb,
                    d->ih, d->iw, d->c, d->oh, d->ow, store, (E*)a.dx, a.dx_ld, a.bn);
            };
            if (!a.bn.z) return go(std::false_type{});
            // the BatchNorm tail: recorded winners on 16-bit storage (gv_pool2d_bwd_argmax_bn refuses the rest)
            if constexpr (W == Recorded && sizeof(E) == 2) return go(std::true_type{});
            return GV_E_UNSUPPORTED;
        }
    }
    const int64_t total = (int64_t)d->nb * d->ih * d->iw * (d->c / A::N);
    return gv_launch<pool_bwd_gather<A, W>>(dim3(gv_grid_for(total)), dim3(256), 0, st, (const E*)a.x, d->x_ld, a.arg,
                                            (const E*)a.dy, a.dy_ld, d->nb, d->ih, d->iw, d->c, d->kh, d->kw, d->stride,
                                            d->pad_t, d->pad_l, d->oh, d->ow, store, (E*)a.dx, a.dx_ld);
}

template <Win W>
int pool_bwd(PoolBwdForm f, const PoolBwdArgs& a, hipStream_t st) {
    if (f.n == 1) GV_ST_DISPATCH(a.d->dtype, return (launch_pool_bwd<Px<E, T, 1>, W>(f.kind, a, st)));
    GV_ST_DISPATCH(a.d->dtype, return (launch_pool_bwd<Px<E, T, 16 / sizeof(E)>, W>(f.kind, a, st)));
}

template <class A>
int launch_argmax_fwd(const gv_pool_desc* d, const void* x, void* y, unsigned char* arg, hipStream_t st) {
    using E = typename A::elem;
    const int64_t total = (int64_t)d->nb * d->oh * d->ow * (d->c / A::N);
    return gv_launch<maxpool_argmax_fwd<A>>(dim3(gv_grid_for(total)), dim3(256), 0, st, (const E*)x, d->x_ld, d->nb, d->ih,
                                            d->iw, d->c, d->kh, d->kw, d->stride, d->pad_t, d->pad_l, d->oh, d->ow, (E*)y,
                                            d->y_ld, arg);
}

}  // namespace

namespace gvlp {

int pool2d_bwd(const gv_pool_desc* d, const void* x, const void* dy, int dy_ld, void* dx, int dx_ld, hipStream_t st) {
    const PoolBwdArgs a{d, x, nullptr, dy, dy_ld, dx, dx_ld, BnTail{}};
    const PoolBwdForm f = pool_bwd_form(d, false, pool_quads(d, x, d->x_ld, dy, dy_ld, dx, dx_ld, nullptr));
    if ((d->mode & ~GV_POOL_BWD_STORE) == GV_POOL_MAX) return pool_bwd<Recomputed>(f, a, st);
    return pool_bwd<Average>(f, a, st);
}

// forward max pool + tap bytes ([nb, oh, ow, c] dense)
int pool2d_fwd_argmax(const gv_pool_desc* d, const void* x, void* y, unsigned char* arg, hipStream_t st) {
    if (pool_quads(d, x, d->x_ld, y, d->y_ld, nullptr, 0, arg))
        GV_ST_DISPATCH(d->dtype, return (launch_argmax_fwd<Px<E, T, 16 / sizeof(E)>>(d, x, y, arg, st)));
    GV_ST_DISPATCH(d->dtype, return (launch_argmax_fwd<Px<E, T, 1>>(d, x, y, arg, st)));
}

int pool2d_bwd_argmax(const gv_pool_desc* d, const unsigned char* arg, const void* dy, int dy_ld, void* dx, int dx_ld,
                      hipStream_t st, const void* bn_z, int bn_z_ld, int bn_G, const float* bn_A, const float* bn_B,
                      const float* bn_C, const float* bn_scale, const float* bn_shift) {
    const PoolBwdArgs a{d, nullptr, arg, dy, dy_ld, dx, dx_ld, BnTail{bn_z, bn_z_ld, bn_G, bn_A, bn_B, bn_C, bn_scale, bn_shift}};
    const PoolBwdForm f = pool_bwd_form(d, true, pool_quads(d, nullptr, 0, dy, dy_ld, dx, dx_ld, arg));
    if (bn_z && f.kind == POOL_BWD_GATHER) return GV_E_UNSUPPORTED;  // the BatchNorm tail exists in the 3x3 / 2 kernel only
    if (bn_z && !(gv_aligned16(bn_A) && gv_aligned16(bn_B) && gv_aligned16(bn_C) && gv_aligned16(bn_scale) &&
                  gv_aligned16(bn_shift)))
        return GV_E_BADARG;                                          // (the coefficient tables are read as float4)
    if (f.kind == POOL_BWD_NONE) return GV_E_UNSUPPORTED;
    return pool_bwd<Recorded>(f, a, st);
}

}  // namespace gvlp
