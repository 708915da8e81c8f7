// train.hip — kernels that exist only for the training step of the hot path: the backward of the
// forward ops, the loss (train.py:145) and the Momentum update (train.py:171).  This file holds the extern "C" entry
// points of the step other than the train-mode BatchNorm's (bn_train.hip) and the view pool's (grouping.hip, next to its
// forward), the kernels of the small ops (accumulate for every storage type; BatchNorm moving averages, loss, dense
// backward, optimizer in fp32) and the fp32-MFMA filter gradient.  The training pools and the 16-bit filter gradient are
// checked here and launched by gvlp:: in pool_train.hip, wgrad_lp.hip and wgrad_dma.hip.
#include <math.h>

#include "gv_common.h"
#include "lowp.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

// One body for every storage type: E is the element type in HBM (float, or unsigned short for the 16-bit types), T the type
// it stands for (float, __bf16, _Float16): GV_ST_DISPATCH (gv_common.h).
// dst[p][c] += src[p][c]  (gradient fan-in of the residual add, nets/resnet_v2.py:91); VEC = 16 / sizeof(E) channels per thread (one
// 16-byte access) where the operands can be walked in quads, else 1
template <typename E, typename T, int VEC>
__global__ __launch_bounds__(256) void accumulate_t(const E* __restrict__ src, int src_ld, E* __restrict__ dst, int dst_ld,
                                                    int64_t npix, int c) {
    const int cg = c / VEC;
    const int64_t total = npix * cg;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(idx % cg);
        const int64_t pix = idx / cg;
        float a[8], b[8];
        load_v<T, VEC>(src + pix * src_ld + q * VEC, a);
        load_v<T, VEC>(dst + pix * dst_ld + q * VEC, b);
#pragma unroll
        for (int e = 0; e < VEC; ++e) b[e] += a[e];
        store_v<T, VEC>(dst + pix * dst_ld + q * VEC, b);
    }
}

// dx[b][p][c] += dgap[b][c] / hw
__global__ __launch_bounds__(256) void global_avg_pool_bwd_f32(const float* __restrict__ dgap, int nb, int hw,
                                                               int c, float* __restrict__ dx, int dx_ld) {
    const int64_t total = (int64_t)nb * hw * c;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % c);
        const int64_t pix = idx / c;
        dx[pix * dx_ld + ch] += dgap[(pix / hw) * c + ch] / (float)hw;
    }
}

// mean sparse-softmax cross-entropy (train.py:145): loss, dlogits = (softmax - onehot)/N; one block
__global__ __launch_bounds__(256) void softmax_ce_f32(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      int n, int c, float* __restrict__ loss,
                                                      float* __restrict__ dlogits) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float* l = logits + (size_t)i * c;
        float mx = -INFINITY;
        for (int j = 0; j < c; ++j) mx = fmaxf(mx, l[j]);
        float se = 0.f;
        for (int j = 0; j < c; ++j) se += expf(l[j] - mx);
        const float lse = logf(se) + mx;
        // a label outside [0, c) (or an int64 that does not fit an int) never indexes the logits: like TensorFlow's
        // GPU kernel the row's loss and gradient become NaN, which the trainer's check_numerics (train.py:175) raises on
        const int64_t lab64 = labels[i];
        const bool ok = lab64 >= 0 && lab64 < (int64_t)c;
        const int lab = ok ? (int)lab64 : 0;
        acc += ok ? lse - l[lab] : NAN;
        for (int j = 0; j < c; ++j)
            dlogits[(size_t)i * c + j] = ok ? (expf(l[j] - lse) - (j == lab ? 1.f : 0.f)) / (float)n : NAN;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = part[0] / (float)n;
}

// Dense backward: dx[n][f] = sum_c dy[n][c] W[f][c];  dW[f][c] += sum_n x[n][f] dy[n][c];  db[c] += sum_n dy[n][c]
__global__ __launch_bounds__(256) void dense_bwd_f32(const float* __restrict__ x, const float* __restrict__ dy,
                                                     const float* __restrict__ W, int n, int f, int c,
                                                     float* __restrict__ dx, float* __restrict__ dW,
                                                     float* __restrict__ db) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)n * f) {
        const int row = (int)(i / f), col = (int)(i % f);
        float s = 0.f;
        for (int j = 0; j < c; ++j) s += dy[(size_t)row * c + j] * W[(size_t)col * c + j];
        dx[i] = s;
    }
    if (i < (int64_t)f * c) {
        const int ff = (int)(i / c), cc = (int)(i % c);
        float s = 0.f;
        for (int r = 0; r < n; ++r) s += x[(size_t)r * f + ff] * dy[(size_t)r * c + cc];
        dW[i] += s;
    }
    if (i < c) {
        float s = 0.f;
        for (int r = 0; r < n; ++r) s += dy[(size_t)r * c + i];
        db[i] += s;
    }
}

// MomentumOptimizer(lr, 0.9), non-Nesterov, with the slim L2 term wd*w added to the gradient
// (train.py:171, train_utils.py:121-161):  m = mu*m + (g + wd*w);  w -= lr*m
__global__ void sgd_momentum_f32(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                 int64_t n, float lr, float mu, float wd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float mm = mu * m[i] + (g[i] + wd * w[i]);
    m[i] = mm;
    w[i] -= lr * mm;
}

// ---- filter gradient: dW[r][s][ci][co] += sum_m X[shift_{r,s}(m)][ci] * dZ[m][co] -------------------
// One TN GEMM per filter tap between two pixel-major matrices (the shifted input and dZ), reduction over the output
// pixels, on the exact fp32 MFMA (32x32x2).
// Storage-typed loads of the filter-gradient kernels: S = float, __bf16 or _Float16 in HBM, fp32 in registers.
template <typename S>
__device__ __forceinline__ f32x4 ld4(const S* p) {
    if constexpr (sizeof(S) == 4) {
        return *reinterpret_cast<const f32x4*>(p);
    } else {
        const uint2 raw = *reinterpret_cast<const uint2*>(p);
        f32x4 v;
        v[0] = (float)__builtin_bit_cast(S, (unsigned short)(raw.x & 0xffffu));
        v[1] = (float)__builtin_bit_cast(S, (unsigned short)(raw.x >> 16));
        v[2] = (float)__builtin_bit_cast(S, (unsigned short)(raw.y & 0xffffu));
        v[3] = (float)__builtin_bit_cast(S, (unsigned short)(raw.y >> 16));
        return v;
    }
}
template <typename S>
__device__ __forceinline__ bool ld4_ok(const S* p, int ld) {
    return (ld & 3) == 0 && ((((uintptr_t)p) & (4 * sizeof(S) - 1)) == 0);
}

// The tap-per-workgroup kernel: workgroup tile (64*TI) input channels x (64*TO) output channels for one
// filter tap, 2x2 waves of TI x TO MFMA tiles (v_mfma_f32_32x32x2_f32: exact fp32; the k axis of this GEMM is
// the PIXEL axis, and pixel-major LDS rows are exactly the k-major operand image this instruction wants:
// lane (i, h) reads element [pixel k + h][channel i], 32 consecutive dwords per half-wave).  16 pixels per
// step, LDS double buffered, the next step's global loads are issued before this step's MFMAs, one barrier
// per step.  Pixel slices (blockIdx.y) are combined with fp32 atomics.
template <typename S, int TI, int TO>
__global__ __launch_bounds__(256) void conv_wgrad2_f32(const S* __restrict__ x, int x_ld,
                                                       const S* __restrict__ dz, int dz_ld, int nb, int ih,
                                                       int iw, int cin, int kh, int kw, int stride, int pad_t,
                                                       int pad_l, int oh, int ow, int cout, int64_t M,
                                                       int64_t m_per_block, const GvDw dw) {
    constexpr int PT = (TI * TO == 1) ? 32 : 16, BI = 64 * TI, BO = 64 * TO;   // pixels per step
    constexpr int XV = PT * BI / 4 / 256, ZV = PT * BO / 4 / 256;      // float4 loads per thread and step
    __shared__ __attribute__((aligned(16))) float sX[2][PT][BI];
    __shared__ __attribute__((aligned(16))) float sZ[2][PT][BO];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int ntile_co = (cout + BO - 1) / BO, ntile_ci = (cin + BI - 1) / BI;
    // 1-D grid, XCD-aware: the tiles of one pixel slice re-read the same rows, so they share an XCD's L2
    const int tiles = ntile_co * ntile_ci * kh * kw;
    const int logical = gv_xcd_remap((int)blockIdx.x, (int)gridDim.x);
    int b = logical % tiles;
    const int tco = b % ntile_co; b /= ntile_co;
    const int tci = b % ntile_ci; b /= ntile_ci;
    const int tap = b;
    const int fr = tap / kw, fs = tap - fr * kw;
    const int ci0 = tci * BI, co0 = tco * BO;
    const int64_t m0 = (int64_t)(logical / tiles) * m_per_block;
    const int64_t m1 = m0 + m_per_block < M ? m0 + m_per_block : M;
    f32x16 acc[TI][TO];
#pragma unroll
    for (int t = 0; t < TI; ++t)
#pragma unroll
        for (int u = 0; u < TO; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    const int ohow = oh * ow;
    const bool xvec = (cin & 3) == 0 && ld4_ok(x, x_ld);
    const bool zvec = (cout & 3) == 0 && ld4_ok(dz, dz_ld);
    f32x4 xr[XV], zr[ZV];
    auto load = [&](int64_t mt) {
#pragma unroll
        for (int j = 0; j < XV; ++j) {
            const int idx = tid + j * 256;
            const int p = idx / (BI / 4), c = ci0 + (idx % (BI / 4)) * 4;
            const int64_t m = mt + p;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < m1 && c < cin) {
                const int n = (int)(m / ohow);
                const int rem = (int)(m - (int64_t)n * ohow);
                const int oy = rem / ow, ox = rem - oy * ow;
                const int iy = oy * stride + fr - pad_t, ix = ox * stride + fs - pad_l;
                if ((unsigned)iy < (unsigned)ih && (unsigned)ix < (unsigned)iw) {
                    const S* xp = x + (((size_t)n * ih + iy) * iw + ix) * x_ld + c;
                    if (xvec) {
                        v = ld4(xp);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (c + e < cin) v[e] = (float)xp[e];
                    }
                }
            }
            xr[j] = v;
        }
#pragma unroll
        for (int j = 0; j < ZV; ++j) {
            const int idx = tid + j * 256;
            const int p = idx / (BO / 4), c = co0 + (idx % (BO / 4)) * 4;
            const int64_t m = mt + p;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < m1 && c < cout) {
                const S* zp = dz + (size_t)m * dz_ld + c;
                if (zvec) {
                    v = ld4(zp);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (c + e < cout) v[e] = (float)zp[e];
                }
            }
            zr[j] = v;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < XV; ++j) {
            const int idx = tid + j * 256;
            *reinterpret_cast<f32x4*>(&sX[buf][idx / (BI / 4)][(idx % (BI / 4)) * 4]) = xr[j];
        }
#pragma unroll
        for (int j = 0; j < ZV; ++j) {
            const int idx = tid + j * 256;
            *reinterpret_cast<f32x4*>(&sZ[buf][idx / (BO / 4)][(idx % (BO / 4)) * 4]) = zr[j];
        }
    };
    load(m0);
    store(0);
    __syncthreads();
    int buf = 0;
    const int li = lane & 31, lh = lane >> 5;
    for (int64_t mt = m0; mt < m1; mt += PT) {
        const bool more = mt + PT < m1;
        if (more) load(mt + PT);
#pragma unroll
        for (int k = 0; k < PT; k += 2) {
            float av[TI], bv[TO];
#pragma unroll
            for (int t = 0; t < TI; ++t) av[t] = sX[buf][k + lh][(wi * TI + t) * 32 + li];
#pragma unroll
            for (int u = 0; u < TO; ++u) bv[u] = sZ[buf][k + lh][(wj * TO + u) * 32 + li];
#pragma unroll
            for (int t = 0; t < TI; ++t)
#pragma unroll
                for (int u = 0; u < TO; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[u], acc[t][u], 0, 0, 0);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int u = 0; u < TO; ++u) {
        const int col = co0 + (wj * TO + u) * 32 + li;
        if (col >= cout) continue;
#pragma unroll
        for (int t = 0; t < TI; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + (wi * TI + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (ci < cin) gv_dw_put(dw, logical / tiles, ((size_t)tap * cin + ci) * cout + col, acc[t][u][r]);
            }
    }
}


// Filter gradient of the few-channel layers (the stems: kh*kw*cin <= 288 im2col rows).  The tap-per-workgroup
// kernels above re-read x and dz once per filter tap and waste most of a 64-row tile on 3 or 32 input channels
// (Conv2d_1a/2a/2b: 12 of the 41 ms of filter gradients per step).  Here one WAVE owns a contiguous pixel range and
// ALL im2col rows rho = tap*cin + ci (NRT tiles of 32 rows) x one 32-column tile of cout; the MFMA operands are
// fetched straight from global memory — the k axis of this GEMM is the pixel axis, so lane (i, h) needs
// x[pixel k+h shifted by tap(i)][ci(i)] and dz[pixel k+h][co i]: 128-byte coalesced rows, no LDS, no barrier.
// Loads run U pixel pairs ahead of the MFMAs that consume them.  Waves are combined with fp32 atomics.
template <typename S, int NRT, int U>
__global__ __launch_bounds__(256) void conv_wgrad_direct_f32(const S* __restrict__ x, int x_ld,
                                                             const S* __restrict__ dz, int dz_ld, int ih, int iw,
                                                             int cin, int kh, int kw, int stride, int pad_t,
                                                             int pad_l, int oh, int ow, int cout, int64_t M,
                                                             int64_t m_per_wave, const GvDw dw) {
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    // column tile fastest: the workgroups that share a pixel range (and re-read the same x) run side by side
    const int nct = (cout + 31) / 32;
    const int64_t w = (int64_t)(blockIdx.x / nct) * 4 + (threadIdx.x >> 6);
    const int co = (blockIdx.x % nct) * 32 + li;
    const int64_t m0 = w * m_per_wave;
    const int64_t m1 = m0 + m_per_wave < M ? m0 + m_per_wave : M;
    if (m0 >= M) return;
    const int R = kh * kw * cin;
    int fr[NRT], fs[NRT], delta[NRT];
    bool rv[NRT];
#pragma unroll
    for (int t = 0; t < NRT; ++t) {
        const int rho = t * 32 + li;
        rv[t] = rho < R;
        const int tap = rv[t] ? rho / cin : 0;
        const int ci = rv[t] ? rho - tap * cin : 0;
        fr[t] = tap / kw;
        fs[t] = tap - fr[t] * kw;
        delta[t] = (fr[t] * iw + fs[t]) * x_ld + ci;
    }
    f32x16 acc[NRT];
#pragma unroll
    for (int t = 0; t < NRT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // this lane's pixel of the current pair: m = m0 + 2*pair + lh
    int64_t m = m0 + lh;
    int n = (int)(m / ((int64_t)oh * ow));
    int rem = (int)(m - (int64_t)n * oh * ow);
    int oy = rem / ow, ox = rem - oy * ow;
    S av[2][U][NRT], bv[2][U];             // RAW storage values: converting at the load site would wait for each load
                                          // (16-bit loads) and serialise the prefetch; the conversion happens at the MFMA
    auto fetch = [&](int s) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool pok = m < m1;
            const int iy0 = oy * stride - pad_t, ix0 = ox * stride - pad_l;
            const int base = ((n * ih + iy0) * iw + ix0) * x_ld;          // < 2^31 elements (checked by the launcher)
            // (no branch around the loads: a join would force vmcnt(0) and serialise the prefetch)
#pragma unroll
            for (int t = 0; t < NRT; ++t) {
                const bool ok = pok && rv[t] && (unsigned)(iy0 + fr[t]) < (unsigned)ih &&
                                (unsigned)(ix0 + fs[t]) < (unsigned)iw;
                av[s][u][t] = ok ? x[base + delta[t]] : (S)0.f;
            }
            bv[s][u] = (pok && co < cout) ? dz[m * dz_ld + co] : (S)0.f;
            m += 2;
            ox += 2;
            while (ox >= ow) {
                ox -= ow;
                if (++oy == oh) { oy = 0; ++n; }
            }
        }
    };
    auto consume = [&](int s) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < NRT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32((float)av[s][u][t], (float)bv[s][u], acc[t], 0, 0, 0);
    };
    const int64_t pairs = (m1 - m0 + 1) / 2;
    const int64_t stages = (pairs + U - 1) / U;
    fetch(0);
    for (int64_t st = 0; st + 1 < stages; st += 2) {     // two stages per trip: static register sets
        fetch(1);
        consume(0);
        if (st + 2 < stages) fetch(0);
        consume(1);
    }
    if (stages & 1) consume(0);
    if (co < cout) {
#pragma unroll
        for (int t = 0; t < NRT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rho = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (rho < R) gv_dw_put(dw, w, (size_t)rho * cout + co, acc[t][r]);
            }
    }
}


__global__ void bn_update_moving(const float* __restrict__ mean, const float* __restrict__ var,
                                 const int* __restrict__ counts, int G, int c, float decay,
                                 float* __restrict__ mm, float* __restrict__ mv) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    float m = mm[ch], v = mv[ch];
    for (int g = 0; g < G; ++g) {                         // one update per view graph copy, in view order
        const float n = (float)counts[g];
        const float unb = n > 1.f ? n / (n - 1.f) : 1.f;
        m = __fadd_rn(__fmul_rn(m, decay), __fmul_rn(mean[(size_t)g * c + ch], 1.f - decay));
        v = __fadd_rn(__fmul_rn(v, decay), __fmul_rn(__fmul_rn(var[(size_t)g * c + ch], unb), 1.f - decay));
    }
    mm[ch] = m;
    mv[ch] = v;
}

// every BatchNorm layer's moving-average update in ONE launch (block -> job through a table)
__global__ void bn_update_moving_batched(const gv_bn_moving_job* __restrict__ jobs, const int* __restrict__ block_job,
                                         int G, float decay) {
    const gv_bn_moving_job j = jobs[block_job[blockIdx.x]];
    const int ch = (blockIdx.x - j.first_block) * blockDim.x + threadIdx.x;
    if (ch >= j.c) return;
    float m = j.moving_mean[ch], v = j.moving_var[ch];
    const size_t ld = j.ld > 0 ? (size_t)j.ld : (size_t)j.c;
    for (int g = 0; g < G; ++g) {
        const float n = (float)j.counts[g];
        const float unb = n > 1.f ? n / (n - 1.f) : 1.f;
        m = __fadd_rn(__fmul_rn(m, decay), __fmul_rn(j.mean[g * ld + ch], 1.f - decay));
        v = __fadd_rn(__fmul_rn(v, decay), __fmul_rn(__fmul_rn(j.var[g * ld + ch], unb), 1.f - decay));
    }
    j.moving_mean[ch] = m;
    j.moving_var[ch] = v;
}

}  // namespace

extern "C" int gv_bn_update_moving_batched(const gv_bn_moving_job* jobs_dev, int32_t num_jobs,
                                           const int32_t* block_job_dev, int32_t num_blocks, int32_t num_groups,
                                           float decay, void* stream) {
    if (!jobs_dev || !block_job_dev || num_jobs <= 0 || num_blocks <= 0 || num_groups <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(bn_update_moving_batched, dim3((unsigned)num_blocks), dim3(256), 0, (hipStream_t)stream, jobs_dev,
                       block_job_dev, num_groups, decay);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

__global__ void scale_inplace_f32(float* __restrict__ x, int64_t n, float s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= s;
}

extern "C" int gv_scale(float* x, int64_t n, float s, void* stream) {
    if (!x || n <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(scale_inplace_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, s);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_accumulate_t(const void* src, int32_t src_ld, void* dst, int32_t dst_ld, int64_t npix, int32_t c,
                               int32_t dtype, void* stream) {
    if (!gv_storage_type(dtype)) return GV_E_UNSUPPORTED;
    if (!src || !dst || npix <= 0 || c <= 0 || src_ld < c || dst_ld < c) return GV_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    GV_ST_DISPATCH(dtype, {
        constexpr int NE = 16 / sizeof(E);
        if (c % NE == 0 && gv_vec_ok(src, src_ld, NE) && gv_vec_ok(dst, dst_ld, NE))
            hipLaunchKernelGGL((accumulate_t<E, T, NE>), dim3(gv_grid_for(npix * (c / NE))), dim3(256), 0, st, (const E*)src,
                               src_ld, (E*)dst, dst_ld, npix, c);
        else
            hipLaunchKernelGGL((accumulate_t<E, T, 1>), dim3(gv_grid_for(npix * c)), dim3(256), 0, st, (const E*)src, src_ld,
                               (E*)dst, dst_ld, npix, c);
        GV_LAUNCH_CHECK();
        return GV_OK;
    });
}

extern "C" int gv_accumulate(const float* src, int32_t src_ld, float* dst, int32_t dst_ld, int64_t npix,
                             int32_t c, void* stream) {
    return gv_accumulate_t(src, src_ld, dst, dst_ld, npix, c, GV_F32, stream);
}

// The descriptor checks of the training pools (pool_train.hip), after an entry point's null pointers: dimensions, the pixel
// strides of its two activation operands, the mode (without GV_POOL_BWD_STORE; an average only where avg_ok), a valid tap
// in every window, the storage type.
static int pool_train_check(const gv_pool_desc* d, int mode, int ld0, int ld1, bool avg_ok) {
    if (d->nb <= 0 || d->ih <= 0 || d->iw <= 0 || d->c <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->oh <= 0 ||
        d->ow <= 0 || d->pad_t < 0 || d->pad_l < 0 || ld0 < d->c || ld1 < d->c ||
        (mode != GV_POOL_MAX && !(avg_ok && mode == GV_POOL_AVG)))
        return GV_E_BADARG;
    if (!gv_pool_geometry_ok(d)) return GV_E_BADARG;
    if (!gv_storage_type(d->dtype)) return GV_E_UNSUPPORTED;
    return GV_OK;
}

extern "C" int gv_pool2d_bwd(const gv_pool_desc* d, const void* x, const void* dy, int32_t dy_ld, void* dx,
                             int32_t dx_ld, void* stream) {
    if (!d || !dy || !dx) return GV_E_BADARG;
    const int mode = d->mode & ~GV_POOL_BWD_STORE;
    if (mode == GV_POOL_MAX && !x) return GV_E_BADARG;
    if (const int rc = pool_train_check(d, mode, dy_ld, dx_ld, true)) return rc;
    return gvlp::pool2d_bwd(d, x, dy, dy_ld, dx, dx_ld, (hipStream_t)stream);
}

extern "C" int gv_pool2d_fwd_argmax(const gv_pool_desc* d, const void* x, void* y, uint8_t* argmax, void* stream) {
    if (!d || !x || !y || !argmax) return GV_E_BADARG;
    if (const int rc = pool_train_check(d, d->mode, d->x_ld, d->y_ld, false)) return rc;
    if (d->kh * d->kw > 255) return GV_E_UNSUPPORTED;               // the tap index is one byte
    return gvlp::pool2d_fwd_argmax(d, x, y, argmax, (hipStream_t)stream);
}

extern "C" int gv_pool2d_bwd_argmax_bn(const gv_pool_desc* d, const uint8_t* argmax, const void* dy, int32_t dy_ld,
                                       const void* z, int32_t z_ld, int32_t num_groups, const float* coef_a,
                                       const float* coef_b, const float* coef_c, const float* scale, const float* shift,
                                       void* dz, int32_t dz_ld, void* stream) {
    if (!d || !argmax || !dy || !z || !dz || !coef_a || !coef_b || !coef_c || num_groups <= 0) return GV_E_BADARG;
    if ((scale == nullptr) != (shift == nullptr) || z_ld < d->c) return GV_E_BADARG;
    if (const int rc = pool_train_check(d, d->mode & ~GV_POOL_BWD_STORE, dy_ld, dz_ld, false)) return rc;
    if (d->dtype == GV_F32) return GV_E_UNSUPPORTED;
    if (d->c % 8 != 0 || z_ld % 8 != 0 || !gv_aligned16(z)) return GV_E_UNSUPPORTED;
    return gvlp::pool2d_bwd_argmax(d, argmax, dy, dy_ld, dz, dz_ld, (hipStream_t)stream, z, z_ld, num_groups, coef_a, coef_b,
                                   coef_c, scale, shift);
}

extern "C" int gv_pool2d_bwd_argmax(const gv_pool_desc* d, const uint8_t* argmax, const void* dy, int32_t dy_ld, void* dx,
                                    int32_t dx_ld, void* stream) {
    if (!d || !argmax || !dy || !dx) return GV_E_BADARG;
    if (const int rc = pool_train_check(d, d->mode & ~GV_POOL_BWD_STORE, dy_ld, dx_ld, false)) return rc;
    return gvlp::pool2d_bwd_argmax(d, argmax, dy, dy_ld, dx, dx_ld, (hipStream_t)stream);
}

extern "C" int gv_global_avg_pool_bwd(const float* dgap, int32_t nb, int32_t hw, int32_t c, float* dx,
                                      int32_t dx_ld, void* stream) {
    if (!dgap || !dx || nb <= 0 || hw <= 0 || c <= 0 || dx_ld < c) return GV_E_BADARG;
    hipLaunchKernelGGL(global_avg_pool_bwd_f32, dim3(gv_grid_for((int64_t)nb * hw * c)), dim3(256), 0,
                       (hipStream_t)stream, dgap, nb, hw, c, dx, dx_ld);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_softmax_ce(const float* logits, const int64_t* labels, int32_t n, int32_t c, float* loss,
                             float* dlogits, void* stream) {
    if (!logits || !labels || !loss || !dlogits || n <= 0 || c <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(softmax_ce_f32, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, n, c, loss,
                       dlogits);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_dense_bwd(const float* x, const float* dy, const float* kernel, int32_t n, int32_t f,
                            int32_t c, float* dx, float* dkernel, float* dbias, void* stream) {
    if (!x || !dy || !kernel || !dx || !dkernel || !dbias || n <= 0 || f <= 0 || c <= 0) return GV_E_BADARG;
    int64_t total = (int64_t)n * f;
    if ((int64_t)f * c > total) total = (int64_t)f * c;
    hipLaunchKernelGGL(dense_bwd_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                       dy, kernel, n, f, c, dx, dkernel, dbias);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_sgd_momentum(float* w, const float* g, float* m, int64_t n, float lr, float mu, float wd,
                               void* stream) {
    if (!w || !g || !m || n <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(sgd_momentum_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, g,
                       m, n, lr, mu, wd);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int gv_bn_update_moving(const float* mean, const float* var, const int32_t* counts, int32_t num_groups,
                                   int32_t c, float decay, float* moving_mean, float* moving_var, void* stream) {
    if (!mean || !var || !counts || !moving_mean || !moving_var || num_groups <= 0 || c <= 0) return GV_E_BADARG;
    hipLaunchKernelGGL(bn_update_moving, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mean, var,
                       counts, num_groups, c, decay, moving_mean, moving_var);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

// The filter gradient's tuning hooks (tests and tools compare forms with them; nothing else sets them):
static int g_wgrad_lp_f32 = 0;         // 16-bit storage on the fp32 MFMA (typed loads), not the 16-bit MFMA kernels
static int g_wgrad_strip_taps = 5;     // taps per workgroup of the general strip variant: 5 keeps two waves per SIMD (9: one)
extern "C" void gv_conv2d_wgrad_set_lp_f32(int on) { g_wgrad_lp_f32 = on; }
extern "C" void gv_conv2d_wgrad_set_strip_taps(int n) { g_wgrad_strip_taps = n; }
int gvlp::wgrad_strip_taps() { return g_wgrad_strip_taps; }

// few-channel stem layers: all taps in one wave, operands straight from global memory
static bool wgrad_direct_ok(const gv_conv_desc* d) {
    const int64_t M = (int64_t)d->nb * d->oh * d->ow;
    return d->kh * d->kw * d->cin <= 288 && d->cin <= 32 && M >= 200000 &&
           (int64_t)d->nb * d->ih * d->iw * d->x_ld < 0x7fffffffll;
}

template <auto Kernel, typename S>
static int wgrad_direct_launch(dim3 grid, const gv_conv_desc* d, const S* x, const S* dz, int dz_ld, int64_t per,
                               const GvDw& sink, hipStream_t st) {
    return gv_launch<Kernel>(grid, dim3(256), 0, st, x, d->x_ld, dz, dz_ld, d->ih, d->iw, d->cin, d->kh, d->kw, d->stride,
                             d->pad_t, d->pad_l, d->oh, d->ow, d->cout, (int64_t)d->nb * d->oh * d->ow, per, sink);
}

// the fp32-MFMA filter gradient for storage type S (float; 16-bit: stems and shapes the 16-bit MFMA kernel
// does not take)
template <typename S>
static int wgrad_f32mfma(const gv_conv_desc* d, const S* x, const S* dz, int32_t dz_ld, const GvDw& dw, hipStream_t st) {
    const int64_t M = (int64_t)d->nb * d->oh * d->ow;
    const int R = d->kh * d->kw * d->cin;
    const size_t elems = (size_t)R * d->cout;
    if (wgrad_direct_ok(d)) {
        const int nrt = (R + 31) / 32;
        // a wave is a slice of pixel pairs (M >= 200000: the one-pixel minimum never binds)
        const GvSlices p = gv_dw_plan(dw, elems, M, 1, 256 * 4 * (nrt == 1 ? 6 : (nrt <= 5 ? 2 : 1)), 1, 2, 0);
        const dim3 grid((unsigned)(((p.splits + 3) / 4) * ((d->cout + 31) / 32)));
        const auto launch = nrt == 1   ? wgrad_direct_launch<conv_wgrad_direct_f32<S, 1, 8>, S>
                            : nrt <= 5 ? wgrad_direct_launch<conv_wgrad_direct_f32<S, 5, 4>, S>
                                       : wgrad_direct_launch<conv_wgrad_direct_f32<S, 9, 8>, S>;
        const int rc = launch(grid, d, x, dz, dz_ld, p.per, gv_dw_sink(dw, elems, p.splits), st);
        return rc != GV_OK ? rc : gv_dw_finish(dw, elems, p.splits, st);
    }
    // 128 channels on a side only where that wastes no more rows than 64-wide tiles would
    const int ti = (d->cin + 127) / 128 * 128 == (d->cin + 63) / 64 * 64 ? 2 : 1;
    const int to = (d->cout + 127) / 128 * 128 == (d->cout + 63) / 64 * 64 ? 2 : 1;
    const int tiles = d->kh * d->kw * ((d->cin + 64 * ti - 1) / (64 * ti)) * ((d->cout + 64 * to - 1) / (64 * to));
    // ~2k workgroups (256 CUs x 2-4 resident, 2+ rounds) of at least 512 pixels, in steps of 32
    const GvSlices p = gv_dw_plan(dw, elems, M, tiles, 2048, 512, 32, 65535);
    const auto launch = ti == 2 && to == 2 ? gv_wgrad_launch<conv_wgrad2_f32<S, 2, 2>, S>
                        : ti == 2          ? gv_wgrad_launch<conv_wgrad2_f32<S, 2, 1>, S>
                        : to == 2          ? gv_wgrad_launch<conv_wgrad2_f32<S, 1, 2>, S>
                                           : gv_wgrad_launch<conv_wgrad2_f32<S, 1, 1>, S>;
    const int rc = launch(dim3((unsigned)(tiles * p.splits)), d, x, dz, dz_ld, p.per, gv_dw_sink(dw, elems, p.splits), st);
    return rc != GV_OK ? rc : gv_dw_finish(dw, elems, p.splits, st);
}

/* tuning hook: number of launch configurations gv_conv2d_wgrad accepts in gv_conv_desc.tile_cfg for `dtype` */
extern "C" int gv_conv2d_wgrad_num_cfgs(int dtype) { return dtype == GV_BF16 || dtype == GV_F16 ? gvlp::wgrad_num_cfgs() : 0; }

// ---- the slices of a filter gradient, added in slice order (the deterministic form: gv_common.h, GvDw) ----------------
// dw[i] += part[0][i] + part[1][i] + ... : a workgroup owns 64 (float4) or 256 (scalar) consecutive elements and splits the
// slices over its four waves (wave w: slices w, w + 4, ...), whose sums are added in wave order — a fixed tree, whatever
// the dispatch order.  Reads are 1 KiB per wave-instruction, 4 in flight per lane.
template <typename V>
__global__ __launch_bounds__(256) void dw_reduce_slices(const V* __restrict__ part, size_t stride, int splits,
                                                        V* __restrict__ dw, size_t n) {
    const int cl = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + cl;
    V s0 = {}, s1 = {};
    if (i < n) {
        int k = sg;
        for (; k + 4 < splits; k += 8) {
            const V a = part[(size_t)k * stride + i], b = part[(size_t)(k + 4) * stride + i];
            s0 += a;
            s1 += b;
        }
        if (k < splits) s0 += part[(size_t)k * stride + i];
    }
    __shared__ V red[4][64];
    red[sg][cl] = s0 + s1;
    __syncthreads();
    if (sg == 0 && i < n) dw[i] += (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

int gv_dw_finish(const GvDw& o, size_t elems, int64_t splits, hipStream_t st) {
    if (!o.part || splits <= 1) return GV_OK;
    const size_t stride = (elems + 3) / 4 * 4;
    if (splits > 0x7fffffff) return GV_E_UNSUPPORTED;
    if (elems % 4 == 0 && gv_aligned16(o.dw) && gv_aligned16(o.part)) {
        const size_t n = elems / 4;
        hipLaunchKernelGGL(dw_reduce_slices<f32x4>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st,
                           (const f32x4*)o.part, stride / 4, (int)splits, (f32x4*)o.dw, n);
    } else {
        hipLaunchKernelGGL(dw_reduce_slices<float>, dim3((unsigned)((elems + 63) / 64)), dim3(256), 0, st,
                           (const float*)o.part, stride, (int)splits, o.dw, elems);
    }
    GV_LAUNCH_CHECK();
    return GV_OK;
}

static int wgrad_dispatch(const gv_conv_desc* d, const void* x, const void* dz, int32_t dz_ld, const GvDw& dw,
                          hipStream_t st) {
    if (!d || !x || !dz || !dw.dw) return GV_E_BADARG;
    if (d->nb <= 0 || d->cin <= 0 || d->cout <= 0 || dz_ld < d->cout || d->x_ld < d->cin) return GV_E_BADARG;
    if (d->dtype == GV_BF16 || d->dtype == GV_F16) {
        // (the 16-bit MFMA kernel also takes the 32-channel stem layers: the direct kernel's scalar 16-bit loads
        // lose the prefetch, 7-13 ms against ~1 ms)
        if (!g_wgrad_lp_f32 && gvlp::wgrad_mfma_ok(d, x, dz, dz_ld))
            return gvlp::conv_wgrad(d, x, dz, dz_ld, dw, st);
        if (!g_wgrad_lp_f32 && d->cin <= 4) {             // the 3-channel stems: row strips on the 16-bit MFMA
            const int rc = gvlp::conv_wgrad_stem(d, x, dz, dz_ld, dw, st);
            if (rc != GV_E_UNSUPPORTED) return rc;
        }
        if (d->dtype == GV_BF16) return wgrad_f32mfma<__bf16>(d, (const __bf16*)x, (const __bf16*)dz, dz_ld, dw, st);
        return wgrad_f32mfma<_Float16>(d, (const _Float16*)x, (const _Float16*)dz, dz_ld, dw, st);
    }
    if (d->dtype != GV_F32) return GV_E_UNSUPPORTED;
    return wgrad_f32mfma<float>(d, (const float*)x, (const float*)dz, dz_ld, dw, st);
}

extern "C" int gv_conv2d_wgrad(const gv_conv_desc* d, const void* x, const void* dz, int32_t dz_ld,
                               float* dw_hwio, void* stream) {
    return wgrad_dispatch(d, x, dz, dz_ld, gv_dw_plain(dw_hwio), (hipStream_t)stream);
}

/* The deterministic form: pixel slices store their partial tiles into `workspace` and are added in slice order. */
extern "C" int gv_conv2d_wgrad_ws(const gv_conv_desc* d, const void* x, const void* dz, int32_t dz_ld,
                                  float* dw_hwio, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!workspace || workspace_bytes < 0 || !gv_aligned16(workspace)) return GV_E_BADARG;
    return wgrad_dispatch(d, x, dz, dz_ld, GvDw{dw_hwio, (float*)workspace, 0, (size_t)workspace_bytes},
                          (hipStream_t)stream);
}
