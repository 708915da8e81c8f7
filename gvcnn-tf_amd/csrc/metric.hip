// metric.hip — the learned retrieval metric: a low-rank Mahalanobis projection W [r, d] trained on shape descriptors
// with a pairwise hinge loss over ALL pairs of a batch (the objective is written out in include/gvcnn_hip.h).
//
//   gv_metric_project     Z = X W^T, an "NT" GEMM on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32) with both operands read
//                         straight from their rows as 16-byte loads (the k order of retrieval.hip's fp32 path: a lane
//                         loads k = k0+8t+4h+e and feeds element e to MFMA e).  64 x 128 per workgroup, a 32 x 64 wave
//                         tile.  W rows r..rl-1 read as zero, so the pad columns of Z are stored as zero.  |z_i|^2 is a
//                         second small launch (one wave per row: a strided fmaf chain per lane, a fixed shuffle tree).
//   gv_metric_pair_grad   the hot path, the shape of an attention kernel.  A workgroup owns 128 rows i (32 per wave, held
//                         in registers as the B operand) and walks tiles of 32 rows j staged in LDS.  The score tile is
//                         computed TRANSPOSED, S'[j, i] = Z_j Z_i^T: the 32x32 accumulator then has i on the lane and j in
//                         its 16 registers (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), which is exactly the B
//                         operand layout of a product that sums over j.  So after distance / hinge / a_ij in registers,
//                         register e of the tile IS the B operand of MFMA e of G^T[c, i] += Z_j^T[c, j] a'[j, i], whose
//                         A operand is one LDS word per lane (row j = that register's row, column c on the lane): no
//                         transposition, no second LDS buffer.  A tile without an active pair skips the second product.
//                         The j tiles are cut into `slices` contiguous ranges over gridDim.y so that a batch of a few
//                         thousand rows still fills the device; slice s STORES its G and s_i = sum_j a_ij into its own
//                         image of the workspace and a second launch adds the slices in index order and writes
//                         dZ = 2 (s_i z_i - G_i).  Statistics: per-thread chains (fp64 sums of the per-pair fp32 values,
//                         integer counts) over the pairs i < j, a fixed LDS tree per workgroup, per-workgroup partials
//                         added by one ordered pass.
//   gv_metric_wgrad       dW = dZ^T X, both operands read with the lane on their contiguous axis (one word per lane per
//                         MFMA, 128-byte segments); 64 x 128 per workgroup, the batch axis cut into slices whose images
//                         an ordered finish adds, divides by P (read from stats on the device) and extends by dL/db.
//
// No floating-point atomics anywhere: the same inputs give the same bits every run.  Integer-valued inputs (see
// tests/test_gpu_metric.py) stay integers through every step, so Z, dZ and the statistics can be compared bit for bit.
#include "gv_common.h"

namespace {

constexpr int MT = 256;                                          // threads of every kernel here
constexpr int PAIR_ROWS = 128;                                   // rows i per workgroup of the pair kernel (32 per wave)
constexpr int PAIR_JT = 32;                                      // rows j per LDS tile
constexpr int PAIR_MAX_SLICES = 8;
constexpr int PAIR_WG_TARGET = 512;                              // slices are added until the grid has this many workgroups
constexpr int WG_MAX_SLICES = 32;                                // batch slices of the filter gradient
constexpr int WG_MIN_CHUNK = 256;

struct PairStats {                                               // one workgroup's share of the statistics
    double h_pos, h_neg, d_sum;
    long long pairs, act_pos, act_neg;
};

// row of register e in the 32x32 accumulator of lane half h
__device__ __forceinline__ int acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* s_red) {          // fixed tree; the result in every thread
    const int tid = threadIdx.x;
    __syncthreads();
    s_red[tid] = v;
    __syncthreads();
    for (int s = MT / 2; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    return s_red[0];
}

// 4 floats of a row at column k (k % 4 == 0), zero from column d on
__device__ __forceinline__ f32x4 load4(const float* row, int k, int d) {
    if (k + 4 <= d) return *reinterpret_cast<const f32x4*>(row + k);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k + e < d) v[e] = row[k + e];
    return v;
}

// ---- projection ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT) void project_kernel(const float* __restrict__ x, int n, int d, long long x_ld,
                                                     const float* __restrict__ w, int r, long long w_ld,
                                                     float* __restrict__ z, int rl) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.y * 64 + (wv >> 1) * 32, c0 = blockIdx.x * 128 + (wv & 1) * 64;
    if (c0 >= rl) return;                                        // rl = 64 or 192: the last half tile is empty
    const float* xr = x + (size_t)min(i0 + lr, n - 1) * x_ld;
    const float* wr[2];
    bool won[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = c0 + 32 * j + lr;
        won[j] = row < r;
        wr[j] = w + (size_t)min(row, r - 1) * w_ld;
    }
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < d; k0 += 16) {
        f32x4 a[2], b[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k = k0 + 8 * t + 4 * h;
            a[t] = load4(xr, k, d);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j][t] = won[j] ? load4(wr[j], k, d) : zero;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][e], b[j][t][e], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = c0 + 32 * j + lr;                        // < rl: rl is a multiple of 64
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = i0 + acc_row(e, h);
            if (row < n) z[(size_t)row * rl + col] = acc[j][e];
        }
    }
}

// one wave per row
__global__ __launch_bounds__(MT) void row_sqnorm_kernel(const float* __restrict__ z, int n, int rl,
                                                        float* __restrict__ sqnorm) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (MT / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* zr = z + (size_t)row * rl;
    float s = 0.f;
    for (int c = lane; c < rl; c += 64) s = __fmaf_rn(zr[c], zr[c], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);  // both partners add the same two values
    if (lane == 0) sqnorm[row] = s;
}

// ---- all pairs: hinge, a_ij, G = a Z ---------------------------------------------------------------------------------
template <int RL>
__global__ __launch_bounds__(MT) void pair_kernel(const float* __restrict__ z, const float* __restrict__ sqnorm,
                                                  const long long* __restrict__ labels, int n,
                                                  const float* __restrict__ b_ptr, float pos_weight, int slices,
                                                  float* __restrict__ g_part, float* __restrict__ s_part,
                                                  PairStats* __restrict__ wg_stats) {
    constexpr int LDZ = RL + 4;                                  // 16-byte rows; b128 row reads spread over all banks
    __shared__ __attribute__((aligned(16))) float s_z[PAIR_JT * LDZ];
    __shared__ float s_sq[PAIR_JT];
    __shared__ long long s_lab[PAIR_JT];
    __shared__ double s_red[MT];
    __shared__ long long s_redi[MT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lr = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * PAIR_ROWS + 32 * wv;
    const int i = i0 + lr;
    const bool wave_on = i0 < n;                                 // (wave-uniform)
    const float b = *b_ptr;
    const long long lab_i = i < n ? labels[i] : -1;
    const float sq_i = i < n ? sqnorm[i] : 0.f;

    f32x4 zi[RL / 8];                                            // the wave's rows as the B operand of S' = Z_j Z_i^T
    {
        const float* zr = z + (size_t)min(i, n - 1) * RL + 4 * h;
#pragma unroll
        for (int kb = 0; kb < RL / 8; ++kb) zi[kb] = *reinterpret_cast<const f32x4*>(zr + 8 * kb);
    }
    f32x16 G[RL / 32];                                           // G^T[c, i]: column c in the registers, row i on the lane
#pragma unroll
    for (int cb = 0; cb < RL / 32; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) G[cb][e] = 0.f;
    float s_i = 0.f;
    double h_pos = 0.0, h_neg = 0.0, d_sum = 0.0;
    int pairs = 0, act_pos = 0, act_neg = 0;

    const int ntiles = (n + PAIR_JT - 1) / PAIR_JT;
    const int t_begin = (int)((long long)ntiles * blockIdx.y / slices);
    const int t_end = (int)((long long)ntiles * (blockIdx.y + 1) / slices);
    for (int t = t_begin; t < t_end; ++t) {
        const int j0 = t * PAIR_JT;
        __syncthreads();                                         // the previous tile has been read
        for (int v = tid; v < PAIR_JT * (RL / 4); v += MT) {
            const int row = v / (RL / 4), c4 = v % (RL / 4);
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (j0 + row < n) val = *reinterpret_cast<const f32x4*>(z + (size_t)(j0 + row) * RL + 4 * c4);
            *reinterpret_cast<f32x4*>(&s_z[row * LDZ + 4 * c4]) = val;
        }
        if (tid < PAIR_JT) {
            const int j = j0 + tid;
            s_sq[tid] = j < n ? sqnorm[j] : 0.f;
            s_lab[tid] = j < n ? labels[j] : -1;
        }
        __syncthreads();
        if (!wave_on) continue;

        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int kb = 0; kb < RL / 8; ++kb) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(&s_z[lr * LDZ + 8 * kb + 4 * h]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], zi[kb][e], acc, 0, 0, 0);
        }

        // acc[e] = z_j . z_i with j = j0 + acc_row(e, h), i on the lane
        const bool upper = j0 + PAIR_JT - 1 > i0;               // the tile holds pairs with i < j (wave-uniform)
        float a[16];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int jl = acc_row(e, h), j = j0 + jl;
            const long long lab_j = s_lab[jl];
            const bool valid = lab_i >= 0 && lab_j >= 0 && j != i;
            const bool pos = lab_i == lab_j;
            const float dist = fmaxf(0.f, __fmaf_rn(-2.f, acc[e], sq_i + s_sq[jl]));
            const float m = b - dist;
            const float arg = pos ? 1.f - m : 1.f + m;          // 1 - y (b - d)
            const bool active = valid && arg > 0.f;
            a[e] = active ? (pos ? pos_weight : -1.f) : 0.f;
            s_i += a[e];
            any |= active;
            if (upper && valid && i < j) {
                ++pairs;
                d_sum += (double)dist;
                if (active) {
                    if (pos) { ++act_pos; h_pos += (double)arg; }
                    else { ++act_neg; h_neg += (double)arg; }
                }
            }
        }
        if (!__any(any)) continue;                               // nothing to add to G from this tile
#pragma unroll
        for (int cb = 0; cb < RL / 32; ++cb)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                G[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_z[acc_row(e, h) * LDZ + 32 * cb + lr], a[e], G[cb], 0, 0, 0);
    }

    // this slice's image: G[i, c] and s_i (the two lane halves hold different j: h = 0 first)
    const float s_other = __shfl_xor(s_i, 32, 64);
    const float s_row = h == 0 ? s_i + s_other : s_other + s_i;
    if (i < n) {
        float* gp = g_part + ((size_t)blockIdx.y * n + i) * RL;
#pragma unroll
        for (int cb = 0; cb < RL / 32; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = {G[cb][4 * q], G[cb][4 * q + 1], G[cb][4 * q + 2], G[cb][4 * q + 3]};
                *reinterpret_cast<f32x4*>(gp + 32 * cb + 8 * q + 4 * h) = v;
            }
        if (h == 0) s_part[(size_t)blockIdx.y * n + i] = s_row;
    }
    PairStats st;
    st.h_pos = block_sum(h_pos, s_red);
    st.h_neg = block_sum(h_neg, s_red);
    st.d_sum = block_sum(d_sum, s_red);
    st.pairs = block_sum((long long)pairs, s_redi);
    st.act_pos = block_sum((long long)act_pos, s_redi);
    st.act_neg = block_sum((long long)act_neg, s_redi);
    if (tid == 0) wg_stats[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = st;
}

// dz[i, c..c+3] = 2 (s_i z_i - G_i), the slices added in index order
__global__ __launch_bounds__(MT) void pair_finish_kernel(const float* __restrict__ z, const float* __restrict__ g_part,
                                                         const float* __restrict__ s_part, int n, int rl, int slices,
                                                         float* __restrict__ dz) {
    const size_t v = (size_t)blockIdx.x * MT + threadIdx.x, per_row = rl / 4;
    if (v >= (size_t)n * per_row) return;
    const size_t i = v / per_row;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    float s = 0.f;
    for (int sl = 0; sl < slices; ++sl) {
        g += *reinterpret_cast<const f32x4*>(g_part + (size_t)sl * n * rl + 4 * v);
        s += s_part[(size_t)sl * n + i];
    }
    const f32x4 zi = *reinterpret_cast<const f32x4*>(z + 4 * v);
    f32x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = 2.f * (s * zi[e] - g[e]);
    *reinterpret_cast<f32x4*>(dz + 4 * v) = out;
}

// one workgroup: the per-workgroup statistics in index order (strided chains, a fixed tree)
__global__ __launch_bounds__(MT) void pair_stats_kernel(const PairStats* __restrict__ wg_stats, int nwg,
                                                        float pos_weight, double* __restrict__ stats) {
    __shared__ double s_red[MT];
    __shared__ long long s_redi[MT];
    double h_pos = 0.0, h_neg = 0.0, d_sum = 0.0;
    long long pairs = 0, act_pos = 0, act_neg = 0;
    for (int g = threadIdx.x; g < nwg; g += MT) {
        const PairStats st = wg_stats[g];
        h_pos += st.h_pos; h_neg += st.h_neg; d_sum += st.d_sum;
        pairs += st.pairs; act_pos += st.act_pos; act_neg += st.act_neg;
    }
    h_pos = block_sum(h_pos, s_red);
    h_neg = block_sum(h_neg, s_red);
    d_sum = block_sum(d_sum, s_red);
    pairs = block_sum(pairs, s_redi);
    act_pos = block_sum(act_pos, s_redi);
    act_neg = block_sum(act_neg, s_redi);
    if (threadIdx.x == 0) {
        const double pw = (double)pos_weight;
        stats[0] = pw * h_pos + h_neg;
        stats[1] = (double)pairs;
        stats[2] = (double)(act_pos + act_neg);
        stats[3] = pw * (double)act_pos - (double)act_neg;
        stats[4] = d_sum;
    }
}

// ---- filter gradient --------------------------------------------------------------------------------------------------
// part[slice][rr, c] = sum over the slice's rows i of dz[i, rr] x[i, c]
__global__ __launch_bounds__(MT) void wgrad_kernel(const float* __restrict__ dz, int n, int r, int rl,
                                                   const float* __restrict__ x, int d, long long x_ld, int ld, int chunk,
                                                   float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 31, h = lane >> 5;
    const int rr0 = blockIdx.y * 64 + (wv >> 1) * 32, c0 = blockIdx.x * 128 + (wv & 1) * 64;
    const int i_begin = blockIdx.z * chunk, i_end = min(n, i_begin + chunk);
    const float* ap = dz + rr0 + lr;                             // rr0 + lr < rl
    const float* bp[2];
    bool bon[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + 32 * j + lr;
        bon[j] = c < d;
        bp[j] = x + min(c, d - 1);
    }
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    for (int i = i_begin + h; i < i_end + h; i += 2) {           // (both lane halves run the same trip count)
        const bool on = i < i_end;
        const size_t row = on ? i : i_begin;
        const float a = on ? ap[row * rl] : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float bv = on && bon[j] ? bp[j][row * x_ld] : 0.f;
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[j], 0, 0, 0);
        }
    }
    float* out = part + (size_t)blockIdx.z * r * ld;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + 32 * j + lr;
        if (c >= ld) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rr = rr0 + acc_row(e, h);
            if (rr < r) out[(size_t)rr * ld + c] = acc[j][e];
        }
    }
}

// grad = (sum of the slices in index order) / P, then dL/db; P and sum a come from stats on the device
__global__ __launch_bounds__(MT) void wgrad_finish_kernel(const float* __restrict__ part, int slices, long long elems,
                                                          const double* __restrict__ stats, float* __restrict__ grad,
                                                          float* __restrict__ loss) {
    const long long v = (long long)blockIdx.x * MT + threadIdx.x;
    if (v > elems) return;
    const double P = stats[1];
    if (v == elems) {
        grad[elems] = P > 0.0 ? (float)(-stats[3] / P) : 0.f;
        if (loss) *loss = P > 0.0 ? (float)(stats[0] / P) : 0.f;
        return;
    }
    float s = 0.f;
    for (int sl = 0; sl < slices; ++sl) s += part[(size_t)sl * elems + v];
    grad[v] = P > 0.0 ? (float)((double)s / P) : 0.f;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int rank_ld(int r) { return (r + 63) / 64 * 64; }

struct PairPlan {
    int blocks, slices;
    int64_t g_bytes, s_bytes, st_bytes;
};
inline PairPlan pair_plan(int n, int rl) {
    PairPlan p;
    p.blocks = gv_ceil_div(n, PAIR_ROWS);
    const int ntiles = gv_ceil_div(n, PAIR_JT);
    p.slices = PAIR_WG_TARGET / p.blocks;
    if (p.slices > PAIR_MAX_SLICES) p.slices = PAIR_MAX_SLICES;
    if (p.slices > ntiles) p.slices = ntiles;
    if (p.slices < 1) p.slices = 1;
    p.g_bytes = round_up((int64_t)p.slices * n * rl * 4, 256);
    p.s_bytes = round_up((int64_t)p.slices * n * 4, 256);
    p.st_bytes = round_up((int64_t)p.slices * p.blocks * (int64_t)sizeof(PairStats), 256);
    return p;
}

struct WgradPlan {
    int chunk, slices;
};
inline WgradPlan wgrad_plan(int n) {
    WgradPlan p;
    p.chunk = (int)round_up(gv_ceil_div(n, WG_MAX_SLICES), 2);
    if (p.chunk < WG_MIN_CHUNK) p.chunk = WG_MIN_CHUNK;
    p.slices = gv_ceil_div(n, p.chunk);
    return p;
}
inline int wgrad_ld(int d) { return (d + 3) / 4 * 4; }

}  // namespace

extern "C" int gv_metric_project(const float* x, int32_t n, int32_t d, int32_t x_ld, const float* w, int32_t r,
                                 int32_t w_ld, float* z, int32_t rl, float* sqnorm, void* stream) {
    if (!x || !w || !z || !sqnorm || n <= 0 || d <= 0 || r <= 0 || x_ld < d || w_ld < d) return GV_E_BADARG;
    if (r > GV_METRIC_MAX_RANK) return GV_E_UNSUPPORTED;
    if (rl != rank_ld(r)) return GV_E_BADARG;
    if (x_ld % 4 != 0 || w_ld % 4 != 0 || !gv_aligned16(x) || !gv_aligned16(w) || !gv_aligned16(z)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(project_kernel, dim3(gv_ceil_div(rl, 128), gv_ceil_div(n, 64)), dim3(MT), 0, st, x, n, d,
                       (long long)x_ld, w, r, (long long)w_ld, z, rl);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(gv_ceil_div(n, MT / 64)), dim3(MT), 0, st, z, n, rl, sqnorm);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int64_t gv_metric_pair_workspace_bytes(int32_t n, int32_t r) {
    if (n <= 0 || r <= 0) return GV_E_BADARG;
    if (r > GV_METRIC_MAX_RANK || n > GV_METRIC_MAX_BATCH) return GV_E_UNSUPPORTED;
    const PairPlan p = pair_plan(n, rank_ld(r));
    return p.g_bytes + p.s_bytes + p.st_bytes;
}

extern "C" int gv_metric_pair_grad(const float* z, const float* sqnorm, const int64_t* labels, int32_t n, int32_t r,
                                   int32_t rl, const float* b, float pos_weight, float* dz_unnorm, double* stats,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    if (!z || !sqnorm || !labels || !b || !dz_unnorm || !stats || !workspace || n <= 0 || r <= 0) return GV_E_BADARG;
    if (r > GV_METRIC_MAX_RANK || n > GV_METRIC_MAX_BATCH) return GV_E_UNSUPPORTED;
    if (rl != rank_ld(r) || workspace_bytes < gv_metric_pair_workspace_bytes(n, r)) return GV_E_BADARG;
    if (!gv_aligned16(z) || !gv_aligned16(dz_unnorm) || !gv_aligned16(workspace)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const PairPlan p = pair_plan(n, rl);
    float* g_part = static_cast<float*>(workspace);
    float* s_part = reinterpret_cast<float*>(static_cast<char*>(workspace) + p.g_bytes);
    PairStats* wg_stats = reinterpret_cast<PairStats*>(static_cast<char*>(workspace) + p.g_bytes + p.s_bytes);
    const dim3 grid(p.blocks, p.slices);
    const long long* lab = reinterpret_cast<const long long*>(labels);
#define GV_PAIR_LAUNCH(RL)                                                                                       \
    hipLaunchKernelGGL(pair_kernel<RL>, grid, dim3(MT), 0, st, z, sqnorm, lab, n, b, pos_weight, p.slices, g_part, \
                       s_part, wg_stats)
    if (rl == 64) GV_PAIR_LAUNCH(64);
    else if (rl == 128) GV_PAIR_LAUNCH(128);
    else if (rl == 192) GV_PAIR_LAUNCH(192);
    else GV_PAIR_LAUNCH(256);
#undef GV_PAIR_LAUNCH
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_finish_kernel, dim3(gv_ceil_div((int64_t)n * (rl / 4), MT)), dim3(MT), 0, st, z, g_part,
                       s_part, n, rl, p.slices, dz_unnorm);
    GV_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_stats_kernel, dim3(1), dim3(MT), 0, st, wg_stats, p.blocks * p.slices, pos_weight, stats);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int64_t gv_metric_wgrad_workspace_bytes(int32_t n, int32_t d, int32_t r) {
    if (n <= 0 || d <= 0 || r <= 0) return GV_E_BADARG;
    if (r > GV_METRIC_MAX_RANK || n > GV_METRIC_MAX_BATCH) return GV_E_UNSUPPORTED;
    return round_up((int64_t)wgrad_plan(n).slices * r * wgrad_ld(d) * 4, 256);
}

extern "C" int gv_metric_wgrad(const float* dz_unnorm, int32_t n, int32_t r, int32_t rl, const float* x, int32_t d,
                               int32_t x_ld, const double* stats, float* grad, int32_t ld, float* loss,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    if (!dz_unnorm || !x || !stats || !grad || !workspace || n <= 0 || d <= 0 || r <= 0 || x_ld < d) return GV_E_BADARG;
    if (r > GV_METRIC_MAX_RANK || n > GV_METRIC_MAX_BATCH) return GV_E_UNSUPPORTED;
    if (rl != rank_ld(r) || ld != wgrad_ld(d) || workspace_bytes < gv_metric_wgrad_workspace_bytes(n, d, r))
        return GV_E_BADARG;
    if (!gv_aligned16(dz_unnorm) || !gv_aligned16(workspace)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const WgradPlan p = wgrad_plan(n);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(wgrad_kernel, dim3(gv_ceil_div(ld, 128), rl / 64, p.slices), dim3(MT), 0, st, dz_unnorm, n, r, rl,
                       x, d, (long long)x_ld, ld, p.chunk, part);
    GV_LAUNCH_CHECK();
    const long long elems = (long long)r * ld;
    hipLaunchKernelGGL(wgrad_finish_kernel, dim3(gv_ceil_div(elems + 1, MT)), dim3(MT), 0, st, part, p.slices, elems,
                       stats, grad, loss);
    GV_LAUNCH_CHECK();
    return GV_OK;
}
