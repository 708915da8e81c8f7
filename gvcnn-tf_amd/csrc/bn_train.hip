// bn_train.hip — the train-mode BatchNorm of the training step for every storage type: the reference builds
// one graph copy per view, so every BatchNorm normalises over the N*h*w values of ONE view (nets/model.py:129-141 +
// slim.batch_norm with is_training=True); group of image b = b % G.  Three HBM-bound passes per direction that the
// convolutions have not folded into their epilogues (conv_stats.h): the per-(group, channel) sums, the forward apply
// y = act(z*scale + shift) and the backward apply dz += A*g + B*z + C; plus the bias gradient, which is a sums pass.
// Each piece of arithmetic is written once: per (group, channel) as __device__ functions that a small stand-alone kernel
// and the prologue of the apply kernel both call, per element as functions of the sums and apply bodies, one sums kernel
// and one apply kernel templated on E, the element in HBM (float, or unsigned short for the 16-bit types), T, the type it
// stands for, and VEC, the consecutive channels a thread owns: one 16-byte quad (4 fp32, 8 16-bit) wherever the channel
// count and the operands allow, else 1.  Statistics accumulate in fp64, dbeta / dgamma / dbias stay fp32, every
// elementwise result is computed in fp32 and rounded to the storage type once.  The extern "C" entry points are at the
// end: each checks its arguments and launches here.
#include <math.h>

#include <type_traits>

#include "conv_stats.h"
#include "gv_common.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

// ---- per (group, channel) ------------------------------------------------------------------------------------------------
// mean / var (biased) / inv and the folded scale / shift from the fp64 sums (sum z, sum z^2) of channel ch of group g,
// gi = g * c + ch
struct BnStats { float mean, var, inv, scale, shift; };
__device__ __forceinline__ BnStats bn_finalize_ch(const double* __restrict__ acc, const int* __restrict__ counts,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float eps, int g, int ch, int gi) {
    const double m = (double)counts[g];
    const double mu = acc[(size_t)gi * 2] / m;
    double v = acc[(size_t)gi * 2 + 1] / m - mu * mu;
    if (v < 0.0) v = 0.0;
    const float iv = (float)(1.0 / sqrt(v + (double)eps));
    const float ga = gamma ? gamma[ch] : 1.f;
    return {(float)mu, (float)v, iv, iv * ga, beta[ch] - (float)mu * iv * ga};
}

// sum g*zhat from the backward accumulator pair (a0, a1): a1 as it is, or converted from sum g*z (raw_z: GV_ACCUM_RAW_Z,
// what a data-gradient epilogue adds: conv_stats.h)
__device__ __forceinline__ double bn_sum_gzh(double a0, double a1, const float* __restrict__ mean,
                                             const float* __restrict__ inv, int gi, int raw_z) {
    return raw_z ? (double)inv[gi] * (a1 - (double)mean[gi] * a0) : a1;
}

// A, B, C of dz = A*g + B*z + C:  A = gamma*inv, B = -A*inv*s2/m, C = A*(mean*inv*s2 - s1)/m
// (= gamma*inv*(g - s1/m - zhat*s2/m) with s1 = sum g, s2 = sum g*zhat)
struct BnCoef { float A, B, C; };
__device__ __forceinline__ BnCoef bn_bwd_coef_ch(const double* __restrict__ acc, const int* __restrict__ counts,
                                                 const float* __restrict__ mean, const float* __restrict__ inv,
                                                 const float* __restrict__ gamma, int raw_z, int g, int ch, int gi) {
    const float iv = inv[gi], mu = mean[gi];
    const float rm = 1.f / (float)counts[g];
    const double a0 = acc[(size_t)gi * 2], a1 = acc[(size_t)gi * 2 + 1];
    const float s1 = (float)a0, s2 = (float)bn_sum_gzh(a0, a1, mean, inv, gi, raw_z);
    const float A_ = (gamma ? gamma[ch] : 1.f) * iv;
    return {A_, -A_ * iv * s2 * rm, A_ * (mu * iv * s2 - s1) * rm};
}

// dbeta[ch] += sum_g sum g,  dgamma[ch] += sum_g sum g*zhat  (mean / inv are read for raw_z only)
__device__ __forceinline__ void bn_param_grads_ch(const double* __restrict__ acc, const float* __restrict__ mean,
                                                  const float* __restrict__ inv, int G, int c, int ch, int raw_z,
                                                  float* __restrict__ dbeta, float* __restrict__ dgamma) {
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int g = 0; g < G; ++g) {
        const double a0 = acc[((size_t)g * c + ch) * 2], a1 = acc[((size_t)g * c + ch) * 2 + 1];
        a += a0;
        b += bn_sum_gzh(a0, a1, mean, inv, g * c + ch, raw_z);
    }
    if (dbeta) dbeta[ch] += (float)a;
    if (dgamma) dgamma[ch] += (float)b;
}

__global__ void bn_finalize_grouped(const double* __restrict__ acc, int G, int c, const int* __restrict__ counts,
                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                    float* __restrict__ mean, float* __restrict__ var, float* __restrict__ inv,
                                    float* __restrict__ scale, float* __restrict__ shift) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G * c) return;
    const int g = i / c, ch = i - g * c;
    const BnStats s = bn_finalize_ch(acc, counts, gamma, beta, eps, g, ch, i);
    mean[i] = s.mean;
    var[i] = s.var;
    inv[i] = s.inv;
    scale[i] = s.scale;
    shift[i] = s.shift;
}

// the parameter gradient of a sums pass on its own: the bias gradient (G = 1, no dgamma)
__global__ void bn_param_grads(const double* __restrict__ acc, int G, int c, float* __restrict__ dbeta,
                               float* __restrict__ dgamma) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    bn_param_grads_ch(acc, nullptr, nullptr, G, c, ch, 0, dbeta, dgamma);
}

// A, B, C per (group, channel) and dbeta / dgamma: what a kernel other than bn_stream (the pool backward with a
// BatchNorm tail, pool_train.hip) needs to finish a BatchNorm backward
__global__ __launch_bounds__(256) void bn_bwd_coeffs(const double* __restrict__ acc, const int* __restrict__ counts,
                                                     const float* __restrict__ mean, const float* __restrict__ inv,
                                                     const float* __restrict__ gamma, int c, int G, int raw_z,
                                                     float* __restrict__ A, float* __restrict__ B, float* __restrict__ Cc,
                                                     float* __restrict__ dbeta, float* __restrict__ dgamma) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    for (int g = 0; g < G; ++g) {
        const int gi = g * c + ch;
        const BnCoef k = bn_bwd_coef_ch(acc, counts, mean, inv, gamma, raw_z, g, ch, gi);
        A[gi] = k.A;
        B[gi] = k.B;
        Cc[gi] = k.C;
    }
    bn_param_grads_ch(acc, mean, inv, G, c, ch, raw_z, dbeta, dgamma);
}

// ---- per element ---------------------------------------------------------------------------------------------------------
// g = dy where the ReLU let the activation through: the kept y > 0, or (rmask: y was not kept) z*scale + shift > 0.
// Element e of the unpacked registers; y is read only where it was kept.
__device__ __forceinline__ float relu_masked(const float (&dy)[8], bool kept, const float (&y)[8], bool rmask,
                                             const float (&z)[8], const float (&sc)[8], const float (&sh)[8], int e) {
    float g = dy[e];
    if (kept && !(y[e] > 0.f)) g = 0.f;
    if (rmask && !(fmaf(z[e], sc[e], sh[e]) > 0.f)) g = 0.f;
    return g;
}

// the term (u, w) element e adds to (sum u, sum u*w):
//   MODE 0 (BN forward stats):  u = z,            w = z                       -> sum z, sum z^2
//   MODE 1 (BN backward):       u = dy*[y>0],     w = (z-mean)*inv            -> sum g, sum g*zhat
//   MODE 2 (bias gradient):     u = dz,           w unused
template <int MODE>
__device__ __forceinline__ void sums_term(const float (&z)[8], const float (&dy)[8], bool kept, const float (&y)[8],
                                          bool rmask, const float (&mu)[8], const float (&iv)[8], const float (&sc)[8],
                                          const float (&sh)[8], int e, float& u, float& w) {
    if constexpr (MODE == 0) {
        u = w = z[e];
    } else if constexpr (MODE == 1) {
        u = relu_masked(dy, kept, y, rmask, z, sc, sh, e);
        w = (z[e] - mu[e]) * iv[e];
    } else {
        u = dy[e];
        w = 0.f;
    }
}

// fp32 storage: every term straight into fp64 (fp32 runs would cost 1e-7 of the statistics); 16-bit storage: fp32 runs
// (exact enough for 16-bit inputs) that sums_fold empties into fp64 every 16 terms
template <typename E, int MODE>
__device__ __forceinline__ void sums_add(float u, float w, double& s0, double& s1, float& f0, float& f1) {
    if constexpr (sizeof(E) == 4) {
        s0 += u;
        if (MODE != 2) s1 += (double)u * w;
    } else {
        f0 += u;
        if (MODE != 2) f1 = fmaf(u, w, f1);
    }
}
__device__ __forceinline__ void sums_fold(double& s0, double& s1, float& f0, float& f1) {
    s0 += f0;
    s1 += f1;
    f0 = f1 = 0.f;
}

// what a thread moves per pixel and operand: a 16-byte quad of VEC = 16 / sizeof(E) elements, or one element
template <typename E, int VEC>
using Raw = std::conditional_t<VEC == 1, E, u32x4>;
template <typename E, int VEC>
__device__ __forceinline__ Raw<E, VEC> load_raw(const E* p) {
    if constexpr (VEC == 1) return *p;
    else return *reinterpret_cast<const u32x4*>(p);
}
template <typename E, typename T, int VEC>
__device__ __forceinline__ void unpack_raw(Raw<E, VEC> v, float (&f)[8]) {
    if constexpr (VEC == 1) f[0] = up<T>(v);
    else unpackq<E, T>(v, f);
}
template <typename E, typename T, int VEC>
__device__ __forceinline__ void store_raw(E* p, const float (&f)[8]) {
    if constexpr (VEC == 1) *p = down<T>(f[0]);
    else *reinterpret_cast<u32x4*>(p) = packq<E, T>(f);
}

// ---- the passes -----------------------------------------------------------------------------------------------------------
// Block = 64 / VEC channel threads (64 channels; a quad walk reads 128 or 256 contiguous bytes per pixel) x 256 * VEC / 64
// pixel lanes; grid (channel blocks, pixel splits, G).  A thread keeps its channels for the whole pixel range, so
// everything per (group, channel) — mean, inv, the folded backward coefficients — is computed once, and the walk over the
// group's pixels (images g, g+G, g+2G, ... of the batch) is incremental: no division in the loop, four loads in flight per
// stream.  A quad walk counts the group's pixels in int (the launcher checks that they fit), the one-element walk in
// int64_t, so that every shape has a kernel.
template <int VEC>
using PixIndex = std::conditional_t<VEC == 1, int64_t, int>;

template <typename I>
struct GroupWalk {
    int r, hw;
    I step_img;
    int64_t pix;
    __device__ __forceinline__ void init(I p, int hw_, int G, int g) {
        hw = hw_;
        const I k = p / hw_;
        r = (int)(p - k * hw_);
        pix = (int64_t)(k * G + g) * hw_ + r;
        step_img = (I)(G - 1) * hw_;
    }
    __device__ __forceinline__ void advance(int n) {
        pix += n;
        if (step_img) {                                          // (one group: the pixels are contiguous)
            r += n;
            while (r >= hw) { r -= hw; pix += step_img; }
        }
    }
};

// acc[g][c][0] += sum u,  acc[g][c][1] += sum u*w  (sums_term) over the pixels of images b with b % G == g
template <typename E, typename T, int MODE, int VEC>
__global__ __launch_bounds__(256) void bn_grouped_sums(const E* __restrict__ z, int z_ld,
                                                       const E* __restrict__ dy, int dy_ld,
                                                       const E* __restrict__ y, int y_ld,
                                                       const float* __restrict__ mean, const float* __restrict__ inv,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int nb, int hw, int c, int G,
                                                       double* __restrict__ acc) {
    using I = PixIndex<VEC>;
    using R = Raw<E, VEC>;
    constexpr int TPC = 64 / VEC, PL = 256 / TPC, U = 4;         // channel threads, pixel lanes, loads in flight
    const int cl = threadIdx.x % TPC, pl = threadIdx.x / TPC;
    const int ch = blockIdx.x * 64 + cl * VEC;
    const int g = blockIdx.z;
    const int nimg = (nb - g + G - 1) / G;
    const I npix = (I)nimg * hw;
    const I per = (npix + gridDim.y - 1) / gridDim.y;
    const I p0 = blockIdx.y * per;
    const I p1 = p0 + per < npix ? p0 + per : npix;
    double s0[8], s1[8];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s0[e] = s1[e] = 0.0;
    if (ch < c && p0 + pl < p1) {
        float mu[8], iv[8], sc[8], sh[8];
        const bool rmask = MODE == 1 && !y && scale;          // ReLU mask recomputed from z: y = z*scale + shift > 0
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            mu[e] = MODE == 1 ? mean[g * c + ch + e] : 0.f;
            iv[e] = MODE == 1 ? inv[g * c + ch + e] : 0.f;
            sc[e] = rmask ? scale[g * c + ch + e] : 0.f;
            sh[e] = rmask ? shift[g * c + ch + e] : 0.f;
        }
        GroupWalk<I> w;
        w.init(p0 + pl, hw, G, g);
        const I n_it = (p1 - p0 - pl + PL - 1) / PL;
        float f0[8], f1[8];
        auto fold = [&]() {
#pragma unroll
            for (int e = 0; e < VEC; ++e) sums_fold(s0[e], s1[e], f0[e], f1[e]);
        };
        auto add = [&](const R zq, const R gq, const R yq) {
            float zv[8], gv[8], yv[8];
            if (MODE != 2) unpack_raw<E, T, VEC>(zq, zv);
            if (MODE != 0) unpack_raw<E, T, VEC>(gq, gv);
            if (MODE == 1 && y) unpack_raw<E, T, VEC>(yq, yv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float u, v;
                sums_term<MODE>(zv, gv, y != nullptr, yv, rmask, mu, iv, sc, sh, e, u, v);
                sums_add<E, MODE>(u, v, s0[e], s1[e], f0[e], f1[e]);
            }
        };
#pragma unroll
        for (int e = 0; e < VEC; ++e) f0[e] = f1[e] = 0.f;
        I it = 0;
        for (; it + U <= n_it; it += U) {
            R zq[U], gq[U], yq[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (MODE != 2) zq[u] = load_raw<E, VEC>(z + w.pix * z_ld + ch);
                if (MODE != 0) gq[u] = load_raw<E, VEC>(dy + w.pix * dy_ld + ch);
                if (MODE == 1 && y) yq[u] = load_raw<E, VEC>(y + w.pix * y_ld + ch);
                w.advance(PL);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) add(zq[u], gq[u], yq[u]);
            if ((it & 12) == 12) fold();                         // fp32 runs of 16 values, then fp64
        }
        for (; it < n_it; ++it) {
            R zq = R{}, gq = zq, yq = zq;
            if (MODE != 2) zq = load_raw<E, VEC>(z + w.pix * z_ld + ch);
            if (MODE != 0) gq = load_raw<E, VEC>(dy + w.pix * dy_ld + ch);
            if (MODE == 1 && y) yq = load_raw<E, VEC>(y + w.pix * y_ld + ch);
            w.advance(PL);
            add(zq, gq, yq);
        }
        fold();
    }
    __shared__ double red[2][PL][64];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        red[0][pl][cl * VEC + e] = s0[e];
        red[1][pl][cl * VEC + e] = s1[e];
    }
    __syncthreads();
    if (threadIdx.x < 64 && blockIdx.x * 64 + threadIdx.x < c) {
        double a = 0.0, b = 0.0;
        for (int q = 0; q < PL; ++q) { a += red[0][q][threadIdx.x]; b += red[1][q][threadIdx.x]; }
        const size_t o = ((size_t)g * c + blockIdx.x * 64 + threadIdx.x) * 2;
        // the block's partial on the fixed grid of conv_stats.h: the fp64 additions are then exact, so the sums do not
        // depend on the order the blocks arrive in (bitwise reproducible run to run)
        // (fp32 storage: grids 2^-40 / 2^-36 forward, 2^-52 backward — far below fp32 resolution, and they have to be:
        // with the 16-bit grids, 2^-30 / 2^-24 / 2^-40, a layer whose activations are ~1e-2 gets its variance to a relative
        // 1e-7 only and a randomly initialised ResNet's gradient sums of ~1e-8 to 5e-5, which 50 train-mode BatchNorm layers
        // amplify past the 2e-4 the sharded-engine tests of test_gpu_train.py hold.  The price is the exactness range:
        // totals below 2^13 / 2^17 / 2 add exactly (order-independent, bitwise reproducible); beyond them the additions
        // are ordinary fp64 additions, reproducible to 1e-16 relative.  Round 3's backward grid, 2^-60, was exact only
        // below 2^-7.)
        const double q0 = gvconv::stat_grid(sizeof(E), MODE == 0, 0), q1 = gvconv::stat_grid(sizeof(E), MODE == 0, 1);
        atomicAdd(&acc[o], rint(a * q0) / q0);
        if (MODE != 2) atomicAdd(&acc[o + 1], rint(b * q1) / q1);
    }
}

// FWD: y = act(x*scale + shift).  BWD: dz (+)= A*g + B*z + C with g = relu_masked(dy) and bn_bwd_coef_ch's A, B, C.
// Folded into the launch (two tiny launches less per BatchNorm):
//   forward : with ex.fin_acc, the finalize step (bn_finalize_ch) — computed by one thread per channel of the block,
//             stored by the first pixel split;
//   backward: dbeta / dgamma (bn_param_grads_ch), by one thread per channel of the launch.
struct BnExtra {
    const double* fin_acc;
    const float* beta;
    float eps;
    float *mean, *var, *inv, *scale_out, *shift_out;
    float *dbeta, *dgamma;
};

// p0f, p1f: scale, shift (forward) or mean, inv (backward);  flag: relu (forward) or raw_z (backward)
template <typename E, typename T, bool BWD, int VEC>
__global__ __launch_bounds__(256) void bn_stream(const E* __restrict__ x, int x_ld,
                                                 const E* __restrict__ dy, int dy_ld,
                                                 const E* __restrict__ yact, int y_ld,
                                                 const float* __restrict__ p0f, const float* __restrict__ p1f,
                                                 const float* __restrict__ gamma, const double* __restrict__ acc,
                                                 const int* __restrict__ counts, const float* __restrict__ scale,
                                                 const float* __restrict__ shift, int accumulate, int nb, int hw,
                                                 int c, int G, int flag, E* __restrict__ out,
                                                 int out_ld, BnExtra ex) {
    using I = PixIndex<VEC>;
    using R = Raw<E, VEC>;
    constexpr int TPC = 64 / VEC, PL = 256 / TPC, U = 4;         // channel threads, pixel lanes, loads in flight
    const int cl = threadIdx.x % TPC, pl = threadIdx.x / TPC;
    const int ch = blockIdx.x * 64 + cl * VEC;
    const int g = blockIdx.z;
    const int nimg = (nb - g + G - 1) / G;
    const I npix = (I)nimg * hw;
    const I per = (npix + gridDim.y - 1) / gridDim.y;
    const I p0 = blockIdx.y * per;
    const I p1 = p0 + per < npix ? p0 + per : npix;
    // forward with finalize: ONE thread per channel of the block does the fp64 arithmetic (64 instead of 2048 fp64
    // rsqrt per block), the others pick the result up from LDS
    __shared__ float sA[64], sB[64];
    if constexpr (!BWD) {
        if (ex.fin_acc) {
            const int cht = blockIdx.x * 64 + threadIdx.x;
            if (threadIdx.x < 64 && cht < c) {
                const int gi = g * c + cht;
                const BnStats s = bn_finalize_ch(ex.fin_acc, counts, gamma, ex.beta, ex.eps, g, cht, gi);
                sA[threadIdx.x] = s.scale;
                sB[threadIdx.x] = s.shift;
                if (blockIdx.y == 0) {
                    ex.mean[gi] = s.mean;
                    ex.var[gi] = s.var;
                    ex.inv[gi] = s.inv;
                    ex.scale_out[gi] = s.scale;
                    ex.shift_out[gi] = s.shift;
                }
            }
            __syncthreads();
        }
    }
    if constexpr (BWD) {                                         // dbeta / dgamma: one thread per channel, once per launch
        const int cht = blockIdx.x * 64 + threadIdx.x;
        if ((ex.dbeta || ex.dgamma) && blockIdx.y == 0 && g == 0 && threadIdx.x < 64 && cht < c)
            bn_param_grads_ch(acc, p0f, p1f, G, c, cht, flag, ex.dbeta, ex.dgamma);
    }
    const bool rmask = BWD && !yact && scale;                    // ReLU mask recomputed from z (x here)
    // backward: the folded coefficients of the block's 64 channels — ONE thread per channel reads mean / inv / the sums /
    // gamma and does the fp64 conversion, everybody else picks A, B, C (and the mask constants) up from LDS: the small
    // late layers are latency-bound, and 256 threads each fetching 7 values for each of their 8 channels before the first
    // activation load was most of their prologue
    __shared__ float sBw[5][64];
    if constexpr (BWD) {
        const int cht = blockIdx.x * 64 + threadIdx.x;
        if (threadIdx.x < 64 && cht < c) {
            const int gi = g * c + cht;
            const BnCoef k = bn_bwd_coef_ch(acc, counts, p0f, p1f, gamma, flag, g, cht, gi);
            sBw[0][threadIdx.x] = k.A;
            sBw[1][threadIdx.x] = k.B;
            sBw[2][threadIdx.x] = k.C;
            sBw[3][threadIdx.x] = rmask ? scale[gi] : 0.f;
            sBw[4][threadIdx.x] = rmask ? shift[gi] : 0.f;
        }
        __syncthreads();
    }
    if (ch >= c || p0 + pl >= p1) return;
    float A[8], B[8], Cc[8], sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int gi = g * c + ch + e;
        if constexpr (BWD) {
            A[e] = sBw[0][cl * VEC + e];
            B[e] = sBw[1][cl * VEC + e];
            Cc[e] = sBw[2][cl * VEC + e];
            sc[e] = sBw[3][cl * VEC + e];
            sh[e] = sBw[4][cl * VEC + e];
        } else if (ex.fin_acc) {                                 // finalized above
            sc[e] = sh[e] = Cc[e] = 0.f;
            A[e] = sA[cl * VEC + e];
            B[e] = sB[cl * VEC + e];
        } else {                                                 // p0f = scale, p1f = shift
            sc[e] = sh[e] = Cc[e] = 0.f;
            A[e] = p0f[gi];
            B[e] = p1f[gi];
        }
    }
    GroupWalk<I> w;
    w.init(p0 + pl, hw, G, g);
    const I n_it = (p1 - p0 - pl + PL - 1) / PL;
    auto one = [&](int64_t pix, const R xq, const R gq, const R yq, const R oq) {
        float xv[8], o[8];
        unpack_raw<E, T, VEC>(xq, xv);
        if constexpr (BWD) {
            float gv[8], yv[8];
            unpack_raw<E, T, VEC>(gq, gv);
            if (accumulate) unpack_raw<E, T, VEC>(oq, o);
            else
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = 0.f;
            if (yact) unpack_raw<E, T, VEC>(yq, yv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float gg = relu_masked(gv, yact != nullptr, yv, rmask, xv, sc, sh, e);
                o[e] += fmaf(A[e], gg, fmaf(B[e], xv[e], Cc[e]));
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                o[e] = fmaf(xv[e], A[e], B[e]);
                if (flag) o[e] = fmaxf(o[e], 0.f);
            }
        }
        store_raw<E, T, VEC>(out + pix * out_ld + ch, o);
    };
    I it = 0;
    for (; it + U <= n_it; it += U) {
        R xq[U], gq[U], yq[U], oq[U];
        int64_t px[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            px[u] = w.pix;
            xq[u] = load_raw<E, VEC>(x + w.pix * x_ld + ch);
            if constexpr (BWD) {
                gq[u] = load_raw<E, VEC>(dy + w.pix * dy_ld + ch);
                if (yact) yq[u] = load_raw<E, VEC>(yact + w.pix * y_ld + ch);
                if (accumulate) oq[u] = load_raw<E, VEC>(out + w.pix * out_ld + ch);
            }
            w.advance(PL);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(px[u], xq[u], gq[u], yq[u], oq[u]);
    }
    for (; it < n_it; ++it) {
        R xq, gq = R{}, yq = gq, oq = gq;
        xq = load_raw<E, VEC>(x + w.pix * x_ld + ch);
        if constexpr (BWD) {
            gq = load_raw<E, VEC>(dy + w.pix * dy_ld + ch);
            if (yact) yq = load_raw<E, VEC>(yact + w.pix * y_ld + ch);
            if (accumulate) oq = load_raw<E, VEC>(out + w.pix * out_ld + ch);
        }
        one(w.pix, xq, gq, yq, oq);
        w.advance(PL);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// every operand (nullptr: not used) can be walked in 16-byte quads (4 fp32 or 8 16-bit channels) ...
inline bool quads_ok(size_t elem_bytes, int c, const void* p0, int ld0, const void* p1 = nullptr, int ld1 = 0,
                     const void* p2 = nullptr, int ld2 = 0, const void* p3 = nullptr, int ld3 = 0) {
    const int ne = (int)(16 / elem_bytes);
    return c % ne == 0 && gv_vec_ok(p0, ld0, ne) && gv_vec_ok(p1, ld1, ne) && gv_vec_ok(p2, ld2, ne) && gv_vec_ok(p3, ld3, ne);
}
// ... and a group's pixel index fits the int the quad walk counts in
inline bool pix_fit_int(int nb, int hw, int G) { return (int64_t)((nb + G - 1) / G) * hw < 0x7fffffffll; }

// Pixel splits (grid y) of a pass over npix pixels per group: per_wg pixels per workgroup on the big layers, but at least
// ~1024 workgroups in total while a workgroup still gets 128 pixels — the small late layers are latency-bound, a longer
// per-thread loop only adds to their time.  The split count decides the last bits of a sum.
inline int pixel_splits(int64_t npix, int per_wg, int cap, int c = 64, int G = 1) {
    int64_t s = (npix + per_wg - 1) / per_wg;
    const int64_t want = 1024 / ((int64_t)((c + 63) / 64) * G) + 1, most = (npix + 127) / 128;
    if (s < want) s = want < most ? want : most;
    return (int)(s < 1 ? 1 : (s > cap ? cap : s));
}

template <typename E, typename T, int MODE>
int sums_t(const void* z, int z_ld, const void* dy, int dy_ld, const void* y, int y_ld, const float* mean, const float* inv,
           const float* scale, const float* shift, int nb, int hw, int c, int G, int splits, double* acc, hipStream_t st) {
    const bool quads = quads_ok(sizeof(E), c, z, z_ld, dy, dy_ld, y, y_ld) && pix_fit_int(nb, hw, G);
    const auto kernel = quads ? bn_grouped_sums<E, T, MODE, 16 / sizeof(E)> : bn_grouped_sums<E, T, MODE, 1>;
    hipLaunchKernelGGL(kernel, dim3((c + 63) / 64, splits, G), dim3(256), 0, st, (const E*)z, z_ld, (const E*)dy, dy_ld,
                       (const E*)y, y_ld, mean, inv, scale, shift, nb, hw, c, G, acc);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

// MODE as sums_term has it; the accumulator is the caller's to clear
template <int MODE>
int launch_sums(int dtype, const void* z, int z_ld, const void* dy, int dy_ld, const void* y, int y_ld, const float* mean,
                const float* inv, const float* scale, const float* shift, int nb, int hw, int c, int G, int splits,
                double* acc, hipStream_t st) {
    GV_ST_DISPATCH(dtype, return (sums_t<E, T, MODE>(z, z_ld, dy, dy_ld, y, y_ld, mean, inv, scale, shift, nb, hw, c, G,
                                                     splits, acc, st)));
}

// The arguments of a BatchNorm apply by name; what a launch does not use stays null.
struct ApplyArgs {
    const void *x = nullptr, *dy = nullptr, *yact = nullptr;     // forward: x;  backward: z, dy and the kept activation
    int x_ld = 0, dy_ld = 0, y_ld = 0;                           // (nullptr: the ReLU mask is recomputed from scale / shift)
    const float *p0 = nullptr, *p1 = nullptr;                    // forward: scale, shift;  backward: mean, inv
    const float* gamma = nullptr;
    const double* acc = nullptr;
    const int* counts = nullptr;
    const float *scale = nullptr, *shift = nullptr;
    int accumulate = 0, nb = 0, hw = 0, c = 0, G = 0;
    int flag = 0;                                                // forward: relu;  backward: raw_z
    void* out = nullptr;
    int out_ld = 0;
    BnExtra ex{};
};

template <typename E, typename T, bool BWD>
int apply_t(const ApplyArgs& a, hipStream_t st) {
    const bool quads = quads_ok(sizeof(E), a.c, a.x, a.x_ld, a.dy, a.dy_ld, a.yact, a.y_ld, a.out, a.out_ld) &&
                       pix_fit_int(a.nb, a.hw, a.G);
    const auto kernel = quads ? bn_stream<E, T, BWD, 16 / sizeof(E)> : bn_stream<E, T, BWD, 1>;
    const int splits = pixel_splits((int64_t)((a.nb + a.G - 1) / a.G) * a.hw, 1024, 65535, a.c, a.G);
    hipLaunchKernelGGL(kernel, dim3((a.c + 63) / 64, splits, a.G), dim3(256), 0, st, (const E*)a.x, a.x_ld, (const E*)a.dy,
                       a.dy_ld, (const E*)a.yact, a.y_ld, a.p0, a.p1, a.gamma, a.acc, a.counts, a.scale, a.shift,
                       a.accumulate, a.nb, a.hw, a.c, a.G, a.flag, (E*)a.out, a.out_ld, a.ex);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

template <bool BWD>
int launch_apply(int dtype, const ApplyArgs& a, hipStream_t st) {
    GV_ST_DISPATCH(dtype, return (apply_t<E, T, BWD>(a, st)));
}

// fp32 storage has always asked for float4 operands in its forward apply; 16-bit storage takes any shape
inline bool f32_apply_misaligned(int dtype, const void* x, int x_ld, const void* y, int y_ld, int c) {
    return dtype == GV_F32 && !quads_ok(4, c, x, x_ld, y, y_ld);
}

}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------
// The storage-typed `_t` entry point (dtype GV_F32 | GV_BF16 | GV_F16, for some ops with GV_ACCUM_* bits OR-ed in) is the
// implementation; the fp32 entry point passes GV_F32.
extern "C" int gv_bn_sums_grouped_t(const void* z, int32_t nb, int32_t hw, int32_t c, int32_t z_ld,
                                    int32_t num_groups, double* accum, int32_t dtype, void* stream) {
    const bool zeroed = (dtype & GV_ACCUM_ZEROED) != 0;          // the caller keeps a pre-zeroed accumulator per layer
    dtype &= ~GV_ACCUM_ZEROED;
    if (!gv_storage_type(dtype)) return GV_E_UNSUPPORTED;
    if (!z || !accum) return GV_E_BADARG;
    if (nb <= 0 || hw <= 0 || c <= 0 || z_ld < c || num_groups <= 0 || nb % num_groups != 0) return GV_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (!zeroed || dtype == GV_F32)                              // (fp32 clears it whatever the bit says)
        GV_HIP_CHECK(hipMemsetAsync(accum, 0, sizeof(double) * 2 * (size_t)num_groups * c, st));
    const int splits = pixel_splits((int64_t)(nb / num_groups) * hw, 2048, 256, c, num_groups);
    return launch_sums<0>(dtype, z, z_ld, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nb, hw, c, num_groups,
                          splits, accum, st);
}

extern "C" int gv_bn_sums_grouped(const float* z, int32_t nb, int32_t hw, int32_t c, int32_t z_ld,
                                  int32_t num_groups, double* accum, void* stream) {
    return gv_bn_sums_grouped_t(z, nb, hw, c, z_ld, num_groups, accum, GV_F32, stream);
}

extern "C" int gv_bn_finalize_grouped(const double* accum, int32_t c, int32_t num_groups, const int32_t* counts,
                                      const float* gamma, const float* beta, float eps, float* mean, float* var,
                                      float* inv, float* scale, float* shift, void* stream) {
    if (!accum || !counts || !beta || !mean || !var || !inv || !scale || !shift || c <= 0 || num_groups <= 0)
        return GV_E_BADARG;
    hipLaunchKernelGGL(bn_finalize_grouped, dim3((num_groups * c + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       accum, num_groups, c, counts, gamma, beta, eps, mean, var, inv, scale, shift);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_bn_stats_grouped(const float* z, int32_t nb, int32_t hw, int32_t c, int32_t z_ld,
                                   int32_t num_groups, const int32_t* counts, const float* gamma,
                                   const float* beta, float eps, double* accum, float* mean, float* var,
                                   float* inv, float* scale, float* shift, void* stream) {
    const int rc = gv_bn_sums_grouped(z, nb, hw, c, z_ld, num_groups, accum, stream);
    if (rc != GV_OK) return rc;
    return gv_bn_finalize_grouped(accum, c, num_groups, counts, gamma, beta, eps, mean, var, inv, scale, shift, stream);
}

extern "C" int gv_scale_shift_act_grouped_t(const void* x, int32_t nb, int32_t hw, int32_t c, int32_t x_ld,
                                            const float* scale, const float* shift, int32_t num_groups,
                                            int32_t relu, void* y, int32_t y_ld, int32_t dtype, void* stream) {
    if (!gv_storage_type(dtype)) return GV_E_UNSUPPORTED;
    if (!x || !y || !scale || !shift || nb <= 0 || hw <= 0 || c <= 0 || x_ld < c || y_ld < c || num_groups <= 0)
        return GV_E_BADARG;
    if (f32_apply_misaligned(dtype, x, x_ld, y, y_ld, c) || (dtype == GV_F32 && !(gv_aligned16(scale) && gv_aligned16(shift))))
        return GV_E_ALIGN;
    ApplyArgs a;
    a.x = x; a.x_ld = x_ld; a.p0 = scale; a.p1 = shift;
    a.nb = nb; a.hw = hw; a.c = c; a.G = num_groups; a.flag = relu; a.out = y; a.out_ld = y_ld;
    return launch_apply<false>(dtype, a, (hipStream_t)stream);
}

extern "C" int gv_scale_shift_act_grouped(const float* x, int32_t nb, int32_t hw, int32_t c, int32_t x_ld,
                                          const float* scale, const float* shift, int32_t num_groups,
                                          int32_t relu, float* y, int32_t y_ld, void* stream) {
    return gv_scale_shift_act_grouped_t(x, nb, hw, c, x_ld, scale, shift, num_groups, relu, y, y_ld, GV_F32, stream);
}

// finalize + apply in one launch
extern "C" int gv_bn_finalize_apply_grouped_t(const double* accum, const int32_t* counts, const float* gamma,
                                              const float* beta, float eps, const void* x, int32_t nb, int32_t hw,
                                              int32_t c, int32_t x_ld, int32_t num_groups, int32_t relu, void* y,
                                              int32_t y_ld, float* mean, float* var, float* inv, float* scale,
                                              float* shift, int32_t dtype, void* stream) {
    if (!accum || !counts || !beta || !x || !y || !mean || !var || !inv || !scale || !shift) return GV_E_BADARG;
    if (nb <= 0 || hw <= 0 || c <= 0 || x_ld < c || y_ld < c || num_groups <= 0) return GV_E_BADARG;
    if (!gv_storage_type(dtype)) return GV_E_UNSUPPORTED;
    if (f32_apply_misaligned(dtype, x, x_ld, y, y_ld, c)) {
        // fp32 storage refuses the apply of such a shape as gv_scale_shift_act_grouped_t does.  NOTE: the call fails with
        // GV_E_ALIGN and y is untouched, but mean / var / inv / scale / shift ARE written first (no shape is refused its
        // statistics): this call has always behaved so, and the kernel sweep of test_gpu_train_lp.py relies on it
        const int rc = gv_bn_finalize_grouped(accum, c, num_groups, counts, gamma, beta, eps, mean, var, inv, scale, shift,
                                              stream);
        return rc != GV_OK ? rc : GV_E_ALIGN;
    }
    ApplyArgs a;
    a.x = x; a.x_ld = x_ld; a.gamma = gamma; a.counts = counts;
    a.nb = nb; a.hw = hw; a.c = c; a.G = num_groups; a.flag = relu; a.out = y; a.out_ld = y_ld;
    a.ex.fin_acc = accum; a.ex.beta = beta; a.ex.eps = eps;
    a.ex.mean = mean; a.ex.var = var; a.ex.inv = inv; a.ex.scale_out = scale; a.ex.shift_out = shift;
    return launch_apply<false>(dtype, a, (hipStream_t)stream);
}

// scale / shift (both or neither): the ReLU mask is recomputed from z when y was not kept
extern "C" int gv_bn_relu_bwd_sums_grouped_t(const void* dy, int32_t dy_ld, const void* y, int32_t y_ld,
                                             const void* z, int32_t z_ld, const float* mean, const float* inv,
                                             int32_t nb, int32_t hw, int32_t c, int32_t num_groups, double* accum,
                                             const float* scale, const float* shift, int32_t dtype, void* stream) {
    const bool zeroed = (dtype & GV_ACCUM_ZEROED) != 0;
    dtype &= ~GV_ACCUM_ZEROED;
    if ((scale == nullptr) != (shift == nullptr)) return GV_E_BADARG;
    if (!gv_storage_type(dtype)) return GV_E_UNSUPPORTED;
    if (!dy || !z || !mean || !inv || !accum) return GV_E_BADARG;
    if (nb <= 0 || hw <= 0 || c <= 0 || num_groups <= 0 || nb % num_groups != 0) return GV_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (!zeroed || dtype == GV_F32)                              // (fp32 clears it whatever the bit says)
        GV_HIP_CHECK(hipMemsetAsync(accum, 0, sizeof(double) * 2 * (size_t)num_groups * c, st));
    const int splits = pixel_splits((int64_t)(nb / num_groups) * hw, 2048, 256, c, num_groups);
    return launch_sums<1>(dtype, z, z_ld, dy, dy_ld, y, y_ld, mean, inv, scale, shift, nb, hw, c, num_groups, splits, accum,
                          st);
}

extern "C" int gv_bn_relu_bwd_sums_grouped(const float* dy, int32_t dy_ld, const float* y, int32_t y_ld,
                                           const float* z, int32_t z_ld, const float* mean, const float* inv,
                                           int32_t nb, int32_t hw, int32_t c, int32_t num_groups, double* accum,
                                           void* stream) {
    return gv_bn_relu_bwd_sums_grouped_t(dy, dy_ld, y, y_ld, z, z_ld, mean, inv, nb, hw, c, num_groups, accum, nullptr,
                                         nullptr, GV_F32, stream);
}

extern "C" int gv_bn_relu_bwd_apply_grouped_t(const void* dy, int32_t dy_ld, const void* y, int32_t y_ld,
                                              const void* z, int32_t z_ld, const float* mean, const float* inv,
                                              const float* gamma, const int32_t* counts, int32_t nb, int32_t hw,
                                              int32_t c, int32_t num_groups, const double* accum, void* dz,
                                              int32_t dz_ld, float* dbeta, float* dgamma, const float* scale,
                                              const float* shift, int32_t accumulate, int32_t dtype, void* stream) {
    const int raw_z = (dtype & GV_ACCUM_RAW_Z) ? 1 : 0;          // (sum g*z accumulators: 16-bit storage only)
    dtype &= ~GV_ACCUM_RAW_Z;
    if ((scale == nullptr) != (shift == nullptr)) return GV_E_BADARG;
    if (!gv_storage_type(dtype) || (raw_z && dtype == GV_F32)) return GV_E_UNSUPPORTED;
    if (!dy || !z || !mean || !inv || !counts || !accum || !dz) return GV_E_BADARG;
    if (nb <= 0 || hw <= 0 || c <= 0 || num_groups <= 0 || nb % num_groups != 0) return GV_E_BADARG;
    ApplyArgs a;
    a.x = z; a.x_ld = z_ld; a.dy = dy; a.dy_ld = dy_ld; a.yact = y; a.y_ld = y_ld; a.p0 = mean; a.p1 = inv;
    a.gamma = gamma; a.acc = accum; a.counts = counts; a.scale = scale; a.shift = shift; a.accumulate = accumulate;
    a.nb = nb; a.hw = hw; a.c = c; a.G = num_groups; a.flag = raw_z; a.out = dz; a.out_ld = dz_ld;
    a.ex.dbeta = dbeta; a.ex.dgamma = dgamma;
    return launch_apply<true>(dtype, a, (hipStream_t)stream);
}

extern "C" int gv_bn_relu_bwd_apply_grouped(const float* dy, int32_t dy_ld, const float* y, int32_t y_ld,
                                            const float* z, int32_t z_ld, const float* mean, const float* inv,
                                            const float* gamma, const int32_t* counts, int32_t nb, int32_t hw,
                                            int32_t c, int32_t num_groups, const double* accum, float* dz,
                                            int32_t dz_ld, float* dbeta, float* dgamma, void* stream) {
    return gv_bn_relu_bwd_apply_grouped_t(dy, dy_ld, y, y_ld, z, z_ld, mean, inv, gamma, counts, nb, hw, c, num_groups,
                                          accum, dz, dz_ld, dbeta, dgamma, nullptr, nullptr, 1, GV_F32, stream);
}

extern "C" int gv_bn_relu_bwd_grouped(const float* dy, int32_t dy_ld, const float* y, int32_t y_ld,
                                      const float* z, int32_t z_ld, const float* mean, const float* inv,
                                      const float* gamma, const int32_t* counts, int32_t nb, int32_t hw,
                                      int32_t c, int32_t num_groups, double* accum, float* dz, int32_t dz_ld,
                                      float* dbeta, float* dgamma, void* stream) {
    const int rc = gv_bn_relu_bwd_sums_grouped(dy, dy_ld, y, y_ld, z, z_ld, mean, inv, nb, hw, c, num_groups, accum,
                                               stream);
    if (rc != GV_OK) return rc;
    return gv_bn_relu_bwd_apply_grouped(dy, dy_ld, y, y_ld, z, z_ld, mean, inv, gamma, counts, nb, hw, c, num_groups,
                                        accum, dz, dz_ld, dbeta, dgamma, stream);
}

extern "C" int gv_bn_bwd_coeffs_t(const double* accum, const int32_t* counts, const float* mean, const float* inv,
                                  const float* gamma, int32_t c, int32_t num_groups, int32_t raw_z, float* coef_a,
                                  float* coef_b, float* coef_c, float* dbeta, float* dgamma, void* stream) {
    if (!accum || !counts || !mean || !inv || !coef_a || !coef_b || !coef_c || c <= 0 || num_groups <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(bn_bwd_coeffs, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, (hipStream_t)stream, accum, counts,
                       mean, inv, gamma, c, num_groups, raw_z ? 1 : 0, coef_a, coef_b, coef_c, dbeta, dgamma);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_bias_grad_t(const void* dz, int32_t dz_ld, int64_t npix, int32_t c, double* accum, float* dbias,
                              int32_t dtype, void* stream) {
    if (!gv_storage_type(dtype)) return GV_E_UNSUPPORTED;
    if (!dz || !accum || !dbias || npix <= 0 || c <= 0 || dz_ld < c || npix > 0x7fffffff) return GV_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    GV_HIP_CHECK(hipMemsetAsync(accum, 0, sizeof(double) * 2 * (size_t)c, st));
    // the split count decides the last bits of the sums, so fp32 keeps the rule it has always had: 2048 pixels per
    // workgroup, without the "at least ~1024 workgroups" term of pixel_splits
    const int most = gv_ceil_div(npix, 2048);
    const int splits = dtype == GV_F32 ? (most < 1024 ? most : 1024) : pixel_splits(npix, 2048, 1024);
    const int rc = launch_sums<2>(dtype, nullptr, 0, dz, dz_ld, nullptr, 0, nullptr, nullptr, nullptr, nullptr, (int)npix, 1,
                                  c, 1, splits, accum, st);
    if (rc != GV_OK) return rc;
    hipLaunchKernelGGL(bn_param_grads, dim3((c + 255) / 256), dim3(256), 0, st, accum, 1, c, dbias, (float*)nullptr);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_bias_grad(const float* dz, int32_t dz_ld, int64_t npix, int32_t c, double* accum,
                            float* dbias, void* stream) {
    return gv_bias_grad_t(dz, dz_ld, npix, c, accum, dbias, GV_F32, stream);
}
