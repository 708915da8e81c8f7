// retrieval.hip — 3D shape retrieval on GVCNN shape descriptors (the fp32 `gap` vector [N, C] that the classifier's
// Dense layer reads, nets/model.py:163-164): index preparation, k-nearest-neighbour search and average precision.
//
//   gv_retr_prepare            one workgroup per row: (cosine: scale to unit L2 norm) -> round to the storage type ->
//                              zero-pad to ld; |row|^2 is summed from the values AS STORED (after the 16-bit rounding),
//                              per-thread strided fmaf chains + a fixed LDS tree: the same bits every run.
//   distance GEMM              Q x DB "NT" GEMM, both operands row-major with K contiguous, so every MFMA fragment is a
//                              16-byte load straight from a row (no LDS staging).  256 threads = 4 waves as 2 x 2, a
//                              64 x 64 wave tile of 2 x 2 32x32 blocks, 128 x 128 per workgroup.  16-bit storage:
//                              v_mfma_f32_32x32x16_{bf16,f16}, lane (r = l&31, h = l>>5) holds row r, k = k0+16s+8h+0..7.
//                              fp32 storage: the exact fp32 MFMA v_mfma_f32_32x32x2_f32; a lane loads 4 floats
//                              (k = k0+8t+4h+e) and feeds element e to MFMA e — any k permutation shared by both
//                              operands is a valid k order.  The K loop is the same for every pair wherever it sits in
//                              a tile, a chunk or a query block, so the distance of a pair never depends on chunking.
//                              ld is a multiple of 64 and the pad columns are zero: no K mask.  Out-of-range rows are
//                              clamped on load and masked on store.  Epilogue: l2 max(0, fma(-2, q.x, |q|^2 + |x|^2)),
//                              cosine 1 - q.x.
//   top-k (gv_knn_search)      the database runs in chunks of db_chunk rows: GEMM into a [nq, db_chunk] fp32 tile of the
//                              workspace, then one workgroup per query merges the chunk (in pieces of 4096 columns held
//                              in LDS) with its running k best.  Candidates are 64-bit keys (order-preserving bits of the
//                              distance << 32 | row id): ascending distance, ties by the lower id, and no two keys equal,
//                              so "the k smallest" is one set.  Radix select, 8 bits a pass from the top (early exit as
//                              soon as the bin holding the k-th key is taken whole), finds the k-th key T; every key <= T
//                              is gathered.  The running list is kept unsorted between chunks and bitonic-sorted once at
//                              the end.  Empty slots are the keys 0xFFFFFFFF'80000000 + slot (above every real key,
//                              unique), written out as id -1 / +inf; the excluded row gets ~0, which is never selected
//                              because the running list always holds k smaller keys.
//   average precision          queries in blocks of 1024: GEMM into a [block, ndb] tile, then one workgroup per query
//                              bitonic-sorts the query's whole row of keys in LDS (ndb <= 16384: 128 KB of the 160 KB),
//                              counts the relevant rows of each thread's contiguous run of ranks, scans the counts, and
//                              sums j / rank_j in fp64 over a fixed tree.  The excluded row sorts to the end as ~0.
//
// Integer-valued descriptors (|v| <= 3, d <= 2048) give integer dot products, norms and distances below 2^24: every
// storage type is then exact and the tests compare ids and distances with a float64 oracle bit for bit.
#include <math.h>

#include "gv_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int RT = 256;                                          // threads of every retrieval kernel
constexpr int TILE = 128;                                        // GEMM workgroup tile (both sides)
constexpr int SEL_PIECE = 4096;                                  // top-k columns held in LDS at a time
constexpr int AP_QB = 1024;                                      // queries per AP block (workspace rows)
constexpr u64 PAD_KEY = 0xFFFFFFFF80000000ull;                   // + slot: an empty slot of the running list
constexpr u64 DROP_KEY = ~0ull;                                  // the excluded row / padding of a sort

__device__ __forceinline__ u64 make_key(float d, unsigned id) {
    unsigned u = __float_as_uint(d);
    if ((u << 1) == 0) u = 0;                                    // -0 ranks as +0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);              // IEEE order -> unsigned order
    return ((u64)u << 32) | id;
}
__device__ __forceinline__ float key_dist(u64 key) {
    const unsigned o = (unsigned)(key >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// the sum of one value per thread over the workgroup: a fixed tree, the result in every thread
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* s_red) {
    const int tid = threadIdx.x;
    __syncthreads();                                             // s_red may still be read by a previous call
    s_red[tid] = v;
    __syncthreads();
    for (int s = RT / 2; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    return s_red[0];
}

// exclusive prefix sum of one int per thread (256 threads), *total = the sum of all
__device__ __forceinline__ int block_excl_scan(int v, int* s_wsum, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < RT / 64; ++i) {
        if (i < w) off += s_wsum[i];
        tot += s_wsum[i];
    }
    *total = tot;
    return off + incl - v;
}

// ascending bitonic sort of a[0..n), n a power of two; the caller has synchronised after writing a
__device__ void bitonic_sort(u64* a, int n) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < n / 2; i += RT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const u64 x = a[lo], y = a[hi];
                if ((x > y) == ((lo & size) == 0)) { a[lo] = y; a[hi] = x; }
            }
            __syncthreads();
        }
}

// ---- index preparation --------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ float store_elem(void* y, size_t i, float v) {
    if constexpr (DT == GV_F32) {
        static_cast<float*>(y)[i] = v;
        return v;
    } else if constexpr (DT == GV_BF16) {
        const __bf16 s = (__bf16)v;                              // round to nearest even
        static_cast<__bf16*>(y)[i] = s;
        return (float)s;
    } else {
        const _Float16 s = (_Float16)v;
        static_cast<_Float16*>(y)[i] = s;
        return (float)s;
    }
}

template <int DT>
__global__ __launch_bounds__(RT) void retr_prepare_kernel(const float* __restrict__ x, int d, long long x_ld,
                                                          int metric, void* __restrict__ y, int ld,
                                                          float* __restrict__ sqnorm) {
    __shared__ float s_red[RT];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float* xr = x + row * (size_t)x_ld;
    float scale = 1.f;
    if (metric == GV_METRIC_COSINE) {
        float s = 0.f;
        for (int c = tid; c < d; c += RT) s = __fmaf_rn(xr[c], xr[c], s);
        s = block_sum(s, s_red);
        scale = s > 0.f ? 1.f / sqrtf(s) : 0.f;                 // a zero row stays zero
    }
    float sq = 0.f;
    for (int c = tid; c < ld; c += RT) {
        const float v = c < d ? xr[c] * scale : 0.f;
        const float st = store_elem<DT>(y, row * (size_t)ld + c, v);
        sq = __fmaf_rn(st, st, sq);
    }
    sq = block_sum(sq, s_red);
    if (tid == 0) sqnorm[row] = sq;
}

// ---- distance GEMM --------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
    if constexpr (DT == GV_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                       0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                      0, 0);
}

// D[i, j] = dist(A row i, B row j) for i < na, j < nb (row stride of D: d_ld)
template <int DT>
__global__ __launch_bounds__(RT) void dist_gemm_kernel(const void* __restrict__ Av, const float* __restrict__ an,
                                                       int na, const void* __restrict__ Bv,
                                                       const float* __restrict__ bn, int nb, int ld, int metric,
                                                       float* __restrict__ D, long long d_ld) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int a0 = blockIdx.y * TILE + (w >> 1) * 64, b0 = blockIdx.x * TILE + (w & 1) * 64;
    size_t ar[2], br[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        ar[i] = (size_t)min(a0 + 32 * i + r, na - 1) * ld;
        br[i] = (size_t)min(b0 + 32 * i + r, nb - 1) * ld;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if constexpr (DT == GV_F32) {
        const float* A = static_cast<const float*>(Av);
        const float* B = static_cast<const float*>(Bv);
        for (int k0 = 0; k0 < ld; k0 += 16) {
            f32x4 a[2][2], b[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[i][t] = *reinterpret_cast<const f32x4*>(A + ar[i] + k0 + 8 * t + 4 * h);
                    b[i][t] = *reinterpret_cast<const f32x4*>(B + br[i] + k0 + 8 * t + 4 * h);
                }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][t][e], b[j][t][e], acc[i][j], 0, 0, 0);
        }
    } else {
        const unsigned short* A = static_cast<const unsigned short*>(Av);
        const unsigned short* B = static_cast<const unsigned short*>(Bv);
        for (int k0 = 0; k0 < ld; k0 += 64) {
            u32x4 a[2][4], b[2][4];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    a[i][s] = *reinterpret_cast<const u32x4*>(A + ar[i] + k0 + 16 * s + 8 * h);
                    b[i][s] = *reinterpret_cast<const u32x4*>(B + br[i] + k0 + 16 * s + 8 * h);
                }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma16<DT>(a[i][s], b[j][s], acc[i][j]);
        }
    }

    // C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = b0 + 32 * j + r;
        if (col >= nb) continue;
        const float xn = bn[col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = a0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (row >= na) continue;
                const float dot = acc[i][j][e];
                const float dist = metric == GV_METRIC_L2 ? fmaxf(0.f, __fmaf_rn(-2.f, dot, an[row] + xn)) : 1.f - dot;
                D[(size_t)row * d_ld + col] = dist;
            }
    }
}

// ---- top-k ---------------------------------------------------------------------------------------------------
// The k-th smallest of the keys cand[0..m) and top[0..k) (all keys up to it are unique, see the file header).
// Uniform across the workgroup; hist [256], s_res [3].
__device__ u64 radix_kth(const u64* cand, int m, const u64* top, int k, unsigned* hist, int* s_res) {
    const int tid = threadIdx.x, lane = tid & 63;
    u64 prefix = 0, mask = 0;
    int need = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int t = tid; t < m + k; t += RT) {
            const u64 key = t < m ? cand[t] : top[t - m];
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid < 64) {                                          // wave 0: lane l scans bins 4l .. 4l+3
            unsigned c[4], s = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) { c[i] = hist[4 * lane + i]; s += c[i]; }
            unsigned incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            unsigned cum = incl - s;
            if (cum < (unsigned)need && (unsigned)need <= incl) {
                for (int i = 0; i < 4; ++i) {
                    if (cum + c[i] >= (unsigned)need) {
                        s_res[0] = 4 * lane + i;
                        s_res[1] = (int)cum;
                        s_res[2] = (int)c[i];
                        break;
                    }
                    cum += c[i];
                }
            }
        }
        __syncthreads();
        const int digit = s_res[0], below = s_res[1], cnt = s_res[2];
        prefix |= (u64)digit << shift;
        mask |= 0xFFull << shift;
        need -= below;
        if (cnt == need) return prefix | ~mask;                  // the whole bin is among the k smallest
    }
    return prefix;
}

// One workgroup per query: merge columns [0, ncols) of its distance row (database ids c0 + column) into the running
// k best (run [nq, k], unsorted); `last`: sort and write dist / idx instead.
__global__ __launch_bounds__(RT) void knn_select_kernel(const float* __restrict__ dist, long long dist_ld, int c0,
                                                        int ncols, const long long* __restrict__ exclude, int ndb,
                                                        int k, int kp, u64* __restrict__ run, int first, int last,
                                                        float* __restrict__ out_d, long long* __restrict__ out_i) {
    __shared__ u64 s_cand[SEL_PIECE];
    __shared__ u64 s_top[GV_KNN_MAX_K];
    __shared__ u64 s_sel[GV_KNN_MAX_K];
    __shared__ unsigned s_hist[RT];
    __shared__ int s_res[4];
    const int tid = threadIdx.x;
    const size_t q = blockIdx.x;
    long long ex = exclude ? exclude[q] : -1;
    if (ex < 0 || ex >= ndb) ex = -1;
    for (int t = tid; t < k; t += RT) s_top[t] = first ? PAD_KEY + t : run[q * k + t];
    const float* row = dist + q * (size_t)dist_ld;
    for (int p0 = 0; p0 < ncols; p0 += SEL_PIECE) {
        const int m = min(SEL_PIECE, ncols - p0);
        for (int t = tid; t < m; t += RT) {
            const int id = c0 + p0 + t;
            s_cand[t] = id == ex ? DROP_KEY : make_key(row[p0 + t], (unsigned)id);
        }
        __syncthreads();
        const u64 T = radix_kth(s_cand, m, s_top, k, s_hist, s_res);
        if (tid == 0) s_res[3] = 0;
        __syncthreads();
        for (int t = tid; t < m + k; t += RT) {
            const u64 key = t < m ? s_cand[t] : s_top[t - m];
            if (key <= T) s_sel[atomicAdd(&s_res[3], 1)] = key;   // exactly k keys; the order is fixed later
        }
        __syncthreads();
        for (int t = tid; t < k; t += RT) s_top[t] = s_sel[t];
        __syncthreads();
    }
    if (!last) {
        for (int t = tid; t < k; t += RT) run[q * k + t] = s_top[t];
        return;
    }
    for (int t = tid; t < kp; t += RT) s_sel[t] = t < k ? s_top[t] : DROP_KEY;
    __syncthreads();
    bitonic_sort(s_sel, kp);
    for (int t = tid; t < k; t += RT) {
        const u64 key = s_sel[t];
        const bool empty = (unsigned)key >= 0x80000000u;
        out_d[q * k + t] = empty ? __builtin_huge_valf() : key_dist(key);
        out_i[q * k + t] = empty ? -1ll : (long long)(unsigned)key;
    }
}

// ---- average precision ----------------------------------------------------------------------------------------
// One workgroup per query of the block (global query q0 + blockIdx.x); np = the sort size (power of two >= ndb, >= RT).
__global__ __launch_bounds__(RT) void retr_ap_kernel(const float* __restrict__ dist, long long dist_ld, int q0,
                                                     const long long* __restrict__ q_labels,
                                                     const long long* __restrict__ db_labels, int ndb, int np,
                                                     const long long* __restrict__ exclude, float* __restrict__ ap) {
    extern __shared__ u64 s_keys[];
    __shared__ double s_red[RT];
    __shared__ int s_wsum[RT / 64];
    const int tid = threadIdx.x;
    const size_t q = (size_t)q0 + blockIdx.x;
    const long long qlab = q_labels[q];
    if (qlab < 0) {
        if (tid == 0) ap[q] = __builtin_nanf("");
        return;
    }
    long long ex = exclude ? exclude[q] : -1;
    if (ex < 0 || ex >= ndb) ex = -1;
    const float* row = dist + blockIdx.x * (size_t)dist_ld;
    for (int t = tid; t < np; t += RT) s_keys[t] = (t < ndb && t != ex) ? make_key(row[t], (unsigned)t) : DROP_KEY;
    __syncthreads();
    bitonic_sort(s_keys, np);
    const int seg = np / RT, p0 = tid * seg;                    // ranks p0+1 .. p0+seg
    int cnt = 0;
    for (int p = p0; p < p0 + seg; ++p) {
        const u64 key = s_keys[p];
        cnt += key != DROP_KEY && db_labels[(unsigned)key] == qlab;
    }
    int R = 0;
    int j = block_excl_scan(cnt, s_wsum, &R);
    double sum = 0.0;
    for (int p = p0; p < p0 + seg && cnt > 0; ++p) {
        const u64 key = s_keys[p];
        if (key != DROP_KEY && db_labels[(unsigned)key] == qlab) {
            ++j;
            sum += (double)j / (double)(p + 1);
        }
    }
    sum = block_sum(sum, s_red);
    if (tid == 0) ap[q] = R > 0 ? (float)(sum / R) : __builtin_nanf("");
}

// ---- host side ------------------------------------------------------------------------------------------------
inline bool metric_ok(int m) { return m == GV_METRIC_L2 || m == GV_METRIC_COSINE; }
inline bool dtype_ok(int t) { return t == GV_F32 || t == GV_BF16 || t == GV_F16; }
inline int esize(int t) { return t == GV_F32 ? 4 : 2; }
inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

int launch_gemm(const void* A, const float* an, int na, const void* B, const float* bn, int nb, int ld, int metric,
                int dtype, float* D, int64_t d_ld, hipStream_t st) {
    const dim3 grid(gv_ceil_div(nb, TILE), gv_ceil_div(na, TILE));
    if (dtype == GV_F32)
        hipLaunchKernelGGL(dist_gemm_kernel<GV_F32>, grid, dim3(RT), 0, st, A, an, na, B, bn, nb, ld, metric, D,
                           (long long)d_ld);
    else if (dtype == GV_BF16)
        hipLaunchKernelGGL(dist_gemm_kernel<GV_BF16>, grid, dim3(RT), 0, st, A, an, na, B, bn, nb, ld, metric, D,
                           (long long)d_ld);
    else
        hipLaunchKernelGGL(dist_gemm_kernel<GV_F16>, grid, dim3(RT), 0, st, A, an, na, B, bn, nb, ld, metric, D,
                           (long long)d_ld);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

int64_t knn_dist_bytes(int32_t nq, int32_t db_chunk) { return round_up((int64_t)nq * db_chunk * 4, 256); }
int64_t ap_dist_ld(int32_t ndb) { return round_up(ndb, 64); }

}  // namespace

extern "C" int gv_retr_prepare(const float* x, int32_t n, int32_t d, int32_t x_ld, int32_t metric, int32_t dtype,
                               void* y, int32_t ld, float* sqnorm, void* stream) {
    if (!x || !y || !sqnorm || n <= 0 || d <= 0 || x_ld < d || ld < d || !metric_ok(metric)) return GV_E_BADARG;
    if (!dtype_ok(dtype)) return GV_E_UNSUPPORTED;
    if (ld % 64 != 0 || !gv_aligned16(y)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == GV_F32)
        hipLaunchKernelGGL(retr_prepare_kernel<GV_F32>, dim3(n), dim3(RT), 0, st, x, d, (long long)x_ld, metric, y, ld,
                           sqnorm);
    else if (dtype == GV_BF16)
        hipLaunchKernelGGL(retr_prepare_kernel<GV_BF16>, dim3(n), dim3(RT), 0, st, x, d, (long long)x_ld, metric, y, ld,
                           sqnorm);
    else
        hipLaunchKernelGGL(retr_prepare_kernel<GV_F16>, dim3(n), dim3(RT), 0, st, x, d, (long long)x_ld, metric, y, ld,
                           sqnorm);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

extern "C" int64_t gv_knn_workspace_bytes(int32_t nq, int32_t db_chunk, int32_t k) {
    if (nq <= 0 || db_chunk <= 0 || db_chunk % 256 != 0 || k < 1 || k > GV_KNN_MAX_K) return GV_E_BADARG;
    return knn_dist_bytes(nq, db_chunk) + round_up((int64_t)nq * k * 8, 256);
}

extern "C" int gv_knn_search(const void* q, const float* q_sqnorm, int32_t nq, const void* db, const float* db_sqnorm,
                             int32_t ndb, int32_t d, int32_t ld, int32_t metric, int32_t dtype, int32_t k,
                             const int64_t* exclude, int32_t db_chunk, float* dist, int64_t* idx, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    if (!q || !q_sqnorm || !db || !db_sqnorm || !dist || !idx || !workspace) return GV_E_BADARG;
    if (nq <= 0 || ndb <= 0 || d <= 0 || ld < d || !metric_ok(metric)) return GV_E_BADARG;
    if (k < 1 || k > GV_KNN_MAX_K || db_chunk <= 0 || db_chunk % 256 != 0) return GV_E_BADARG;
    if (workspace_bytes < gv_knn_workspace_bytes(nq, db_chunk, k)) return GV_E_BADARG;
    if (!dtype_ok(dtype)) return GV_E_UNSUPPORTED;
    if (ld % 64 != 0 || !gv_aligned16(q) || !gv_aligned16(db) || !gv_aligned16(workspace)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    float* wdist = static_cast<float*>(workspace);
    u64* run = reinterpret_cast<u64*>(static_cast<char*>(workspace) + knn_dist_bytes(nq, db_chunk));
    const int kp = pow2_at_least(k);
    for (int c0 = 0; c0 < ndb; c0 += db_chunk) {
        const int nc = min(db_chunk, ndb - c0);
        const void* dbc = static_cast<const char*>(db) + (size_t)c0 * ld * esize(dtype);
        const int rc = launch_gemm(q, q_sqnorm, nq, dbc, db_sqnorm + c0, nc, ld, metric, dtype, wdist, db_chunk, st);
        if (rc != GV_OK) return rc;
        hipLaunchKernelGGL(knn_select_kernel, dim3(nq), dim3(RT), 0, st, wdist, (long long)db_chunk, c0, nc,
                           (const long long*)exclude, ndb, k, kp, run, c0 == 0 ? 1 : 0,
                           (int64_t)c0 + db_chunk >= ndb ? 1 : 0, dist, (long long*)idx);
        GV_LAUNCH_CHECK();
    }
    return GV_OK;
}

extern "C" int64_t gv_retr_ap_workspace_bytes(int32_t nq, int32_t ndb) {
    if (nq <= 0 || ndb <= 0) return GV_E_BADARG;
    if (ndb > GV_RETR_AP_MAX_NDB) return GV_E_UNSUPPORTED;
    return round_up((int64_t)min(nq, AP_QB) * ap_dist_ld(ndb) * 4, 256);
}

extern "C" int gv_retr_average_precision(const void* q, const float* q_sqnorm, const int64_t* q_labels, int32_t nq,
                                         const void* db, const float* db_sqnorm, const int64_t* db_labels,
                                         int32_t ndb, int32_t d, int32_t ld, int32_t metric, int32_t dtype,
                                         const int64_t* exclude, float* ap, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
    if (!q || !q_sqnorm || !q_labels || !db || !db_sqnorm || !db_labels || !ap || !workspace) return GV_E_BADARG;
    if (nq <= 0 || ndb <= 0 || d <= 0 || ld < d || !metric_ok(metric)) return GV_E_BADARG;
    if (!dtype_ok(dtype) || ndb > GV_RETR_AP_MAX_NDB) return GV_E_UNSUPPORTED;
    if (workspace_bytes < gv_retr_ap_workspace_bytes(nq, ndb)) return GV_E_BADARG;
    if (ld % 64 != 0 || !gv_aligned16(q) || !gv_aligned16(db) || !gv_aligned16(workspace)) return GV_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    const int np = pow2_at_least(ndb < RT ? RT : ndb);
    const size_t lds = (size_t)np * sizeof(u64);
    if (!GV_BIG_LDS_OK(retr_ap_kernel, lds)) return GV_E_UNSUPPORTED;
    float* wdist = static_cast<float*>(workspace);
    const int64_t dld = ap_dist_ld(ndb);
    for (int q0 = 0; q0 < nq; q0 += AP_QB) {
        const int nb = min(AP_QB, nq - q0);
        const void* qb = static_cast<const char*>(q) + (size_t)q0 * ld * esize(dtype);
        const int rc = launch_gemm(qb, q_sqnorm + q0, nb, db, db_sqnorm, ndb, ld, metric, dtype, wdist, dld, st);
        if (rc != GV_OK) return rc;
        hipLaunchKernelGGL(retr_ap_kernel, dim3(nb), dim3(RT), lds, st, wdist, (long long)dld, q0,
                           (const long long*)q_labels, (const long long*)db_labels, ndb, np,
                           (const long long*)exclude, ap);
        GV_LAUNCH_CHECK();
    }
    return GV_OK;
}
