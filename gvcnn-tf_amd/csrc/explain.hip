// Why a shape got its class: per-view, per-pixel attribution of one logit through the head above the final tap
// (view pooling -> group fusion -> global average pool -> Dense), with the grouping held constant as in the backward
// pass (view_pool_fuse_bwd_t in grouping.hip: the tie rule and the order of the coefficient's operations are its; the
// group table is the one both read, group_table.h).
//
//   dlogit_k/dF[n,v,p,c] = sum_{g contains v} ((w_g/W) * (K[c,k]/hw)) / ties_g(p,c)   where F[v] attains the maximum of g
//                                                                     / |g|            mean pooling
//   exact:    maps[n,v,p] = sum_c F * dlogit/dF                (gradient x input: complete for this piecewise-linear head)
//   gradcam:  alpha[n,v,c] = (1/hw) sum_p dlogit/dF,  maps[n,v,p] = max(0, sum_c alpha * F)
//
// One source for fp32 / bf16 / f16 storage (lp_elem.h loaders): F becomes fp32 on load, all arithmetic and every output
// is fp32.  No atomics anywhere: every sum has one owner and a fixed order, so two calls give the same bits.
//
// Work split.  A thread owns one CHANNEL of a chunk of CH channels (CH = blockDim.x: 64, 128 or 256).  A [V][CH] slab of
// one pixel is staged in LDS as fp32 (16-byte global loads when the layout allows, the next slab's loads in flight while
// this one is worked on); thread t then reads column t only, so the LDS traffic is conflict-free and the running sums
// per view — further [V][CH] arrays of LDS columns — need no barrier.  A column is walked group by group (ex_column):
// the groups' member masks are scalars, so the loops over members are uniform and run on the scalar unit; nothing is
// indexed by a runtime view or group number in registers.
//   explain_maps   (exact)            workgroup per (pixel, shape), all chunks: the terms add up in a second [V][CH]
//                                     array of LDS columns; at the end one wave per view sums a row in a fixed order and
//                                     maps[n,v,p] is stored once.
//   explain_alpha  (gradcam, sweep 1) workgroup per (chunk, shape), all pixels: per-(view, channel) sums over the pixels
//                                     live in LDS columns; alpha[n,v,c] is stored once, and the chunk's share of
//                                     view_contrib goes to part[n,v,chunk].
//   explain_cam    (gradcam, sweep 2) wave per (shape, view, pixel): relu(alpha . F).
//   explain_finish                    view_contrib (pixels of maps, or chunks of part, in index order) and baseline.
// exact reads F once; gradcam twice.
#include <type_traits>

#include "group_table.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

struct ExArgs {
    const void* F;
    int V, N, hw, C;
    int64_t vs, ss;                      // view / shape stride of F, in elements
    const int* scheme;
    int G;
    const float* weight;
    int64_t scheme_stride, weight_stride;    // per shape (0: one scheme for all)
    int mode;
    float fill;
    const float* K;
    const float* bias;
    int num_classes;
    const long long* target;             // resolved class per shape, -1: out of range
    float* maps;                         // [N, V, hw]
    float* contrib;                      // [N, V]
    float* baseline;                     // [N]
    float* alpha;                        // [N, V, C]            (gradcam)
    float* part;                         // [N, V, nchunks]      (gradcam)
    int nchunks;
};

// the group table in front of the dynamic LDS of explain_maps / explain_alpha: masks, weights, W in a 16-byte slot
constexpr size_t EX_TABLE_BYTES = 64 * (8 + 4) + 16;

// fixed-order sum over the 64 lanes (butterfly: every lane ends with the same bits)
__device__ __forceinline__ float ex_wave_sum(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// sum of row[0 .. ch) by one wave: lane l adds row[l], row[l + 64], ... then the butterfly
__device__ __forceinline__ float ex_row_sum(const float* row, int ch) {
    float s = 0.f;
    for (int i = threadIdx.x & 63; i < ch; i += 64) s += row[i];
    return ex_wave_sum(s);
}

// class per shape: the given one, else the first maximum of the logits (strict >, as eval_metrics_kernel)
__global__ void explain_targets(const float* __restrict__ logits, const long long* __restrict__ targets, int n, int c,
                                long long* __restrict__ target_out, int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long k;
    if (targets) {
        k = targets[i];
        if (k < 0 || k >= c) { k = -1; *status = 1; }      // every writer stores the same word: no atomic needed
    } else {
        const float* row = logits + (size_t)i * c;
        int best = 0;
        float bv = row[0];
        for (int j = 1; j < c; ++j)
            if (row[j] > bv) { bv = row[j]; best = j; }
        k = best;
    }
    target_out[i] = k;
}

// The group table of shape n with its weights normalised: t.w[g] = w_g / W.  False when W == 0 (the forward gives that
// shape S = 0; the weights stay as loaded).  Every thread of the workgroup calls it.
__device__ __forceinline__ bool ex_groups(const ExArgs& a, int n, const GroupTable& t) {
    group_table_load(t, a.scheme + (size_t)n * a.scheme_stride, a.weight + (size_t)n * a.weight_stride, a.G, a.V, false);
    const float ws = *t.W;
    if (ws != 0.f)
        for (int g = threadIdx.x; g < a.G; g += blockDim.x) t.w[g] = t.w[g] / ws;
    __syncthreads();
    return ws != 0.f;
}

// A 64-bit mask every lane holds the same value of (read from LDS), as a scalar: the loops over its bits then run on the
// scalar unit and only the data they select costs vector instructions.
__device__ __forceinline__ unsigned long long ex_uniform(unsigned long long m) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// The [V][ch] slab of one pixel: channels c0 .. c0 + ch of every view as fp32 in LDS, zeros past C.  16-byte path: a
// thread's first EX_PF quads are FETCHED into registers one step ahead (the loads fly while the previous slab is worked
// on) and STAGED into LDS between two barriers; what a thread holds beyond them (V / VEC > EX_PF), and the scalar path,
// is loaded when it is staged.
constexpr int EX_PF = 4;
template <typename E, typename T, int VEC>
struct ExSlab {
    u32x4 r[EX_PF];
    __device__ __forceinline__ void fetch(const E* __restrict__ px, int V, int64_t vs, int cw, int per_shift) {
        if constexpr (VEC > 1) {
            const int total = V << per_shift;                    // V * (ch / VEC) quads
#pragma unroll
            for (int j = 0; j < EX_PF; ++j) {
                const int idx = threadIdx.x + j * blockDim.x;
                r[j] = u32x4{0u, 0u, 0u, 0u};
                if (idx < total) {
                    const int v = idx >> per_shift;
                    const int c = (idx - (v << per_shift)) * VEC;
                    if (c < cw) r[j] = *reinterpret_cast<const u32x4*>(px + (size_t)v * vs + c);   // C % VEC == 0: c + VEC <= cw
                }
            }
        }
    }
    __device__ __forceinline__ void stage(const E* __restrict__ px, int V, int64_t vs, int cw, int ch, int per_shift,
                                          float* __restrict__ slab) const {
        const int total = V << per_shift;
        int first = threadIdx.x;
        if constexpr (VEC > 1) {
#pragma unroll
            for (int j = 0; j < EX_PF; ++j) {
                const int idx = threadIdx.x + j * blockDim.x;
                if (idx < total) {
                    const int v = idx >> per_shift;
                    const int c = (idx - (v << per_shift)) * VEC;
                    float f[8];
                    unpackq<E, T>(r[j], f);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) slab[v * ch + c + i] = f[i];
                }
            }
            first += EX_PF * blockDim.x;
        }
        for (int idx = first; idx < total; idx += blockDim.x) {
            const int v = idx >> per_shift;
            const int c = (idx - (v << per_shift)) * VEC;
            float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (c < cw) load_v<T, VEC>(px + (size_t)v * vs + c, f);
#pragma unroll
            for (int i = 0; i < VEC; ++i) slab[v * ch + c + i] = f[i];
        }
    }
};

// NB members taken off a group's (scalar) mask: their view numbers stay in scalar registers and address LDS rows.
constexpr int EX_B = 4;
template <int NB>
struct ExPick {
    int i[NB];
};
template <int NB>
__device__ __forceinline__ ExPick<NB> ex_pop(unsigned long long& m) {
    ExPick<NB> b;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        b.i[j] = __ffsll((long long)m) - 1;
        m &= m - 1;
    }
    return b;
}
// fn(members, count) over a mask in batches of EX_B and one exact remainder (no padded slots: a slot costs what a member
// costs).  The count is a compile-time constant inside fn, so its register arrays are indexed by unrolled constants.
template <typename Fn>
__device__ __forceinline__ void ex_batches(unsigned long long m, Fn fn) {
    int left = __popcll(m);
    for (; left >= EX_B; left -= EX_B) fn(ex_pop<EX_B>(m), std::integral_constant<int, EX_B>{});
    if (left == 3) fn(ex_pop<3>(m), std::integral_constant<int, 3>{});
    else if (left == 2) fn(ex_pop<2>(m), std::integral_constant<int, 2>{});
    else if (left == 1) fn(ex_pop<1>(m), std::integral_constant<int, 1>{});
}

// One column (channel) of a slab, group by group: every member v of group g receives
//   d = (w_g/W * K/hw) / ties  where it attains the group's maximum, else 0      (max pooling)
//   d = (w_g/W * K/hw) / |g|                                                     (mean pooling)
// and acc(members, count, f, d) adds it up — a view in several groups is simply visited once per group, which is the
// literal sum over its groups.  The values of up to EX_B members are read from LDS together (independent reads in
// flight, not one latency per member); a group that small never leaves the registers, a larger one is walked three
// times (maximum, ties, shares); a group of one needs no maximum and no division.
template <typename Acc>
__device__ __forceinline__ void ex_column(const ExArgs& a, const unsigned long long* gmask, const float* cg, float kc,
                                          const float* col, int ch, Acc acc) {
    const bool mean = a.mode == GV_VIEWPOOL_MEAN;
    for (int g = 0; g < a.G; ++g) {
        const unsigned long long m0 = ex_uniform(gmask[g]);
        if (m0 == 0) continue;
        const float coef = cg[g] * kc;
        const int cnt = __popcll(m0);
        if (cnt == 1 || mean) {
            const float q = cnt == 1 ? coef : coef / (float)cnt;
            ex_batches(m0, [&](auto b, auto nb) {
                constexpr int NB = decltype(nb)::value;
                float f[NB], d[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) { f[j] = col[b.i[j] * ch]; d[j] = q; }
                acc(b, nb, f, d);
            });
        } else if (cnt <= EX_B) {
            ex_batches(m0, [&](auto b, auto nb) {                // one call: the whole group
                constexpr int NB = decltype(nb)::value;
                float f[NB], d[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) f[j] = col[b.i[j] * ch];
                float best = f[0];
#pragma unroll
                for (int j = 1; j < NB; ++j) best = fmaxf(best, f[j]);
                int ties = 0;
#pragma unroll
                for (int j = 0; j < NB; ++j) ties += f[j] == best ? 1 : 0;
                const float q = coef / (float)ties;
#pragma unroll
                for (int j = 0; j < NB; ++j) d[j] = f[j] == best ? q : 0.f;
                acc(b, nb, f, d);
            });
        } else {
            float best = -INFINITY;
            ex_batches(m0, [&](auto b, auto nb) {
#pragma unroll
                for (int j = 0; j < decltype(nb)::value; ++j) best = fmaxf(best, col[b.i[j] * ch]);
            });
            int ties = 0;
            ex_batches(m0, [&](auto b, auto nb) {
#pragma unroll
                for (int j = 0; j < decltype(nb)::value; ++j) ties += col[b.i[j] * ch] == best ? 1 : 0;
            });
            const float q = coef / (float)ties;
            ex_batches(m0, [&](auto b, auto nb) {
                constexpr int NB = decltype(nb)::value;
                float f[NB], d[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    f[j] = col[b.i[j] * ch];
                    d[j] = f[j] == best ? q : 0.f;
                }
                acc(b, nb, f, d);
            });
        }
    }
}

template <typename E, typename T, int VEC>
__global__ __launch_bounds__(256) void explain_maps(ExArgs a, int per_shift) {
    extern __shared__ unsigned long long lds64[];                // no static LDS: the dynamic limit may be the CU's whole 160 KB
    float* lds = reinterpret_cast<float*>(lds64 + 64);
    const GroupTable tab = {lds64, lds, lds + 64};
    lds += 64 + 4;                                               // (the table: EX_TABLE_BYTES)
    const int p = blockIdx.x, n = blockIdx.y, t = threadIdx.x, ch = blockDim.x;
    float* out = a.maps + ((size_t)n * a.V) * a.hw + p;
    const long long k = a.target[n];
    const bool live = ex_groups(a, n, tab);
    if (k < 0 || !live) {
        for (int v = t; v < a.V; v += ch) out[(size_t)v * a.hw] = 0.f;
        return;
    }
    float* slab = lds;                                           // [V][ch]
    float* tsum = slab + a.V * ch + t;                           // [V][ch] sum over the chunks of F * dlogit/dF
    for (int v = 0; v < a.V; ++v) tsum[v * ch] = 0.f;            // column t is this thread's alone
    const E* px = (const E*)a.F + (size_t)n * a.ss + (size_t)p * a.C;
    ExSlab<E, T, VEC> ld;
    ld.fetch(px, a.V, a.vs, a.C, per_shift);
    float knext = t < a.C ? a.K[(size_t)t * a.num_classes + k] : 0.f;    // the classifier column, one chunk ahead as well
    for (int c0 = 0; c0 < a.C; c0 += ch) {
        ld.stage(px + c0, a.V, a.vs, a.C - c0, ch, per_shift, slab);
        __syncthreads();
        const float kc = knext / (float)a.hw;
        if (c0 + ch < a.C) {
            ld.fetch(px + c0 + ch, a.V, a.vs, a.C - c0 - ch, per_shift);
            knext = c0 + ch + t < a.C ? a.K[(size_t)(c0 + ch + t) * a.num_classes + k] : 0.f;
        }
        ex_column(a, tab.mask, tab.w, kc, slab + t, ch,
                  [&](auto b, auto nb, const auto& f, const auto& d) {
                      constexpr int NB = decltype(nb)::value;
                      float o[NB];
#pragma unroll
                      for (int j = 0; j < NB; ++j) o[j] = tsum[b.i[j] * ch];
#pragma unroll
                      for (int j = 0; j < NB; ++j) tsum[b.i[j] * ch] = o[j] + f[j] * d[j];    // distinct views: no overlap
                  });
        __syncthreads();                                         // the slab is free for the next chunk; tsum is complete
    }
    const int wave = t >> 6, nwave = ch >> 6;
    for (int v = wave; v < a.V; v += nwave) {
        const float r = ex_row_sum(tsum - t + v * ch, ch);
        if ((t & 63) == 0) out[(size_t)v * a.hw] = r;
    }
}

template <typename E, typename T, int VEC>
__global__ __launch_bounds__(256) void explain_alpha(ExArgs a, int per_shift) {
    extern __shared__ unsigned long long lds64[];
    float* lds = reinterpret_cast<float*>(lds64 + 64);
    const GroupTable tab = {lds64, lds, lds + 64};
    lds += 64 + 4;                                               // (the table: EX_TABLE_BYTES)
    const int chunk = blockIdx.x, n = blockIdx.y, t = threadIdx.x, ch = blockDim.x;
    const int c0 = chunk * ch;
    const bool mine = c0 + t < a.C;
    float* alpha = a.alpha + ((size_t)n * a.V) * a.C + c0 + t;
    float* part = a.part + ((size_t)n * a.V) * a.nchunks + chunk;
    const long long k = a.target[n];
    const bool live = ex_groups(a, n, tab);
    if (k < 0 || !live) {
        if (mine)
            for (int v = 0; v < a.V; ++v) alpha[(size_t)v * a.C] = 0.f;
        for (int v = t; v < a.V; v += ch) part[(size_t)v * a.nchunks] = 0.f;
        return;
    }
    float* slab = lds;                                           // [V][ch]
    float* asum = slab + a.V * ch;                               // [V][ch] sum over pixels of dlogit/dF
    float* csum = asum + a.V * ch;                               // [V][ch] sum over pixels of F * dlogit/dF
    for (int v = 0; v < a.V; ++v) { asum[v * ch + t] = 0.f; csum[v * ch + t] = 0.f; }
    const float kc = mine ? a.K[(size_t)(c0 + t) * a.num_classes + k] / (float)a.hw : 0.f;
    const E* base = (const E*)a.F + (size_t)n * a.ss + c0;
    const int cw = a.C - c0;
    ExSlab<E, T, VEC> ld;
    ld.fetch(base, a.V, a.vs, cw, per_shift);
    for (int p = 0; p < a.hw; ++p) {
        ld.stage(base + (size_t)p * a.C, a.V, a.vs, cw, ch, per_shift, slab);
        __syncthreads();
        if (p + 1 < a.hw) ld.fetch(base + (size_t)(p + 1) * a.C, a.V, a.vs, cw, per_shift);
        ex_column(a, tab.mask, tab.w, kc, slab + t, ch,
                  [&](auto b, auto nb, const auto& f, const auto& d) {
                      constexpr int NB = decltype(nb)::value;
                      float oa[NB], oc[NB];
#pragma unroll
                      for (int j = 0; j < NB; ++j) { oa[j] = asum[b.i[j] * ch + t]; oc[j] = csum[b.i[j] * ch + t]; }
#pragma unroll
                      for (int j = 0; j < NB; ++j) {
                          asum[b.i[j] * ch + t] = oa[j] + d[j];
                          csum[b.i[j] * ch + t] = oc[j] + f[j] * d[j];
                      }
                  });
        __syncthreads();
    }
    if (mine)
        for (int v = 0; v < a.V; ++v) alpha[(size_t)v * a.C] = asum[v * ch + t] / (float)a.hw;
    const int wave = t >> 6, nwave = ch >> 6;
    for (int v = wave; v < a.V; v += nwave) {
        const float r = ex_row_sum(csum + v * ch, ch);
        if ((t & 63) == 0) part[(size_t)v * a.nchunks] = r;
    }
}

// maps[n,v,p] = max(0, alpha[n,v,:] . F[n,v,p,:]); one wave per row
template <typename E, typename T, int VEC>
__global__ __launch_bounds__(256) void explain_cam(ExArgs a) {
    const int64_t rows = (int64_t)a.N * a.V * a.hw;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int p = (int)(row % a.hw);
    const int64_t nv = row / a.hw;
    const int v = (int)(nv % a.V), n = (int)(nv / a.V);
    const E* f = (const E*)a.F + (size_t)n * a.ss + (size_t)v * a.vs + (size_t)p * a.C;
    const float* al = a.alpha + (size_t)nv * a.C;
    float s = 0.f;
    for (int c = lane * VEC; c < a.C; c += 64 * VEC) {
        float x[8];
        load_v<T, VEC>(f + c, x);
        if constexpr (VEC > 1) {                                 // (the vector path asks for a 16-byte aligned workspace)
#pragma unroll
            for (int q = 0; q < VEC / 4; ++q) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(al + c + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) s += w[j] * x[4 * q + j];
            }
        } else {
            s += al[c] * x[0];
        }
    }
    s = ex_wave_sum(s);
    if (lane == 0) a.maps[(size_t)nv * a.hw + p] = a.target[n] < 0 ? 0.f : fmaxf(s, 0.f);
}

// One workgroup per (shape, row).  Rows v < V give view_contrib[n,v]: the pixels of the exact maps, or the chunks' shares,
// summed by the first wave — each lane every 64th in index order, then the butterfly (a shape that is switched off has
// zeros there already).  Row V gives baseline[n] = b[k] + sum_{g empty} (w_g/W) * fill * sum_c K[c,k]: every thread sums
// every 256th entry of the classifier column, the four waves' sums are added in wave order.
__global__ __launch_bounds__(256) void explain_finish(ExArgs a, int from_part) {
    GROUP_TABLE_SHARED(tab);
    __shared__ float s_part[4];
    const int n = blockIdx.x, v = blockIdx.y, t = threadIdx.x;
    if (v < a.V) {
        if (t >= 64) return;
        const float* src = from_part ? a.part + ((size_t)n * a.V + v) * a.nchunks : a.maps + ((size_t)n * a.V + v) * a.hw;
        const int cnt = from_part ? a.nchunks : a.hw;
        float s = 0.f;
        for (int i = t; i < cnt; i += 64) s += src[i];
        s = ex_wave_sum(s);
        if (t == 0) a.contrib[(size_t)n * a.V + v] = s;
        return;
    }
    const long long k = a.target[n];
    float ksum = 0.f;
    if (k >= 0) {
#pragma unroll 4
        for (int c = t; c < a.C; c += 256) ksum += a.K[(size_t)c * a.num_classes + k];
    }
    ksum = ex_wave_sum(ksum);
    if ((t & 63) == 0) s_part[t >> 6] = ksum;
    const bool live = ex_groups(a, n, tab);                     // (its barriers publish s_part too)
    if (t == 0) {
        float b = 0.f;
        if (k >= 0) {
            b = a.bias[k];
            ksum = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
            if (live)
                for (int g = 0; g < a.G; ++g)
                    if (tab.mask[g] == 0) b += tab.w[g] * a.fill * ksum;
        }
        a.baseline[n] = b;
    }
}

// (explain_alpha has one workgroup per chunk and shape and walks the pixels serially: it takes narrower chunks until
// `min_wgs` workgroups exist)
int ex_chunk(int C, int rows, int64_t shapes, int64_t min_wgs) {
    int ch = 256;
    while (ch > 64 && (EX_TABLE_BYTES + (size_t)rows * ch * sizeof(float) > 64 * 1024 || ch / 2 >= C ||
                       shapes * ((C + ch - 1) / ch) < min_wgs))
        ch >>= 1;
    return ch;
}
int ex_rows(int V, int kind) { return kind == GV_EXPLAIN_GRADCAM ? 3 * V : 2 * V; }

template <typename E, typename T>
int ex_run(ExArgs a, int kind, bool vec, hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(E);
    const int rows = ex_rows(a.V, kind);
    const int ch = ex_chunk(a.C, rows, a.N, kind == GV_EXPLAIN_GRADCAM ? 2048 : 0);
    const size_t lds = EX_TABLE_BYTES + (size_t)rows * ch * sizeof(float);
    int per_shift = 0;
    while ((1 << per_shift) < ch / (vec ? VEC : 1)) ++per_shift;
    int rc;
    if (kind == GV_EXPLAIN_EXACT) {
        const dim3 grid((unsigned)a.hw, (unsigned)a.N);
        rc = vec ? gv_launch<explain_maps<E, T, VEC>>(grid, dim3(ch), lds, st, a, per_shift)
                 : gv_launch<explain_maps<E, T, 1>>(grid, dim3(ch), lds, st, a, per_shift);
        if (rc != GV_OK) return rc;
        hipLaunchKernelGGL(explain_finish, dim3(a.N, a.V + 1), dim3(256), 0, st, a, 0);
        GV_LAUNCH_CHECK();
        return GV_OK;
    }
    a.nchunks = (a.C + ch - 1) / ch;
    const dim3 grid((unsigned)a.nchunks, (unsigned)a.N);
    rc = vec ? gv_launch<explain_alpha<E, T, VEC>>(grid, dim3(ch), lds, st, a, per_shift)
             : gv_launch<explain_alpha<E, T, 1>>(grid, dim3(ch), lds, st, a, per_shift);
    if (rc != GV_OK) return rc;
    hipLaunchKernelGGL(explain_finish, dim3(a.N, a.V + 1), dim3(256), 0, st, a, 1);
    GV_LAUNCH_CHECK();
    const dim3 cgrid((unsigned)(((int64_t)a.N * a.V * a.hw + 3) / 4));
    if (vec) hipLaunchKernelGGL((explain_cam<E, T, VEC>), cgrid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((explain_cam<E, T, 1>), cgrid, dim3(256), 0, st, a);
    GV_LAUNCH_CHECK();
    return GV_OK;
}

}  // namespace

extern "C" int64_t gv_explain_workspace_bytes(int32_t num_views, int32_t num_shapes, int32_t C, int32_t kind) {
    if (num_views <= 0 || num_shapes <= 0 || C <= 0) return GV_E_BADARG;
    if (kind != GV_EXPLAIN_EXACT && kind != GV_EXPLAIN_GRADCAM) return GV_E_BADARG;
    if (kind == GV_EXPLAIN_EXACT) return 0;
    // alpha [N, V, C], then the chunks' shares of view_contrib [N, V, ceil(C / 64)] (64: the narrowest chunk)
    return (int64_t)num_shapes * num_views * ((int64_t)C + (C + 63) / 64) * (int64_t)sizeof(float);
}

extern "C" int gv_explain_views(const void* F, int32_t num_views, int32_t num_shapes, int32_t hw, int32_t C,
                                int64_t view_stride, int64_t shape_stride, const int32_t* scheme, int32_t num_groups,
                                const float* weight, int32_t per_shape, int32_t pool_mode, float empty_fill,
                                const float* cls_kernel, const float* cls_bias, int32_t num_classes,
                                const float* logits, const int64_t* targets, int32_t kind, float* maps,
                                float* view_contrib, float* baseline, int64_t* target_out, int32_t* status,
                                void* workspace, int32_t dtype, void* stream) {
    if (!F || !scheme || !weight || !cls_kernel || !cls_bias || !maps || !view_contrib || !baseline || !target_out ||
        !status || (!logits && !targets))
        return GV_E_BADARG;
    if (num_views <= 0 || num_shapes <= 0 || hw <= 0 || C <= 0 || num_groups <= 0 || num_classes <= 0 ||
        view_stride < 0 || shape_stride < 0)
        return GV_E_BADARG;
    if (pool_mode != GV_VIEWPOOL_MAX && pool_mode != GV_VIEWPOOL_MEAN) return GV_E_BADARG;
    if (kind != GV_EXPLAIN_EXACT && kind != GV_EXPLAIN_GRADCAM) return GV_E_BADARG;
    if (kind == GV_EXPLAIN_GRADCAM && !workspace) return GV_E_BADARG;
    if (dtype != GV_F32 && dtype != GV_BF16 && dtype != GV_F16) return GV_E_UNSUPPORTED;
    if (num_views > 64 || num_groups > 64 || num_shapes > 65535) return GV_E_UNSUPPORTED;
    if ((int64_t)num_shapes * num_views * hw > 0x7fffffffll * 4) return GV_E_UNSUPPORTED;      // explain_cam's grid
    hipStream_t st = (hipStream_t)stream;
    ExArgs a;
    a.F = F; a.V = num_views; a.N = num_shapes; a.hw = hw; a.C = C; a.vs = view_stride; a.ss = shape_stride;
    a.scheme = scheme; a.G = num_groups; a.weight = weight;
    a.scheme_stride = per_shape ? (int64_t)num_groups * num_views : 0;
    a.weight_stride = per_shape ? num_groups : 0;
    a.mode = pool_mode; a.fill = empty_fill; a.K = cls_kernel; a.bias = cls_bias; a.num_classes = num_classes;
    a.target = (const long long*)target_out; a.maps = maps; a.contrib = view_contrib; a.baseline = baseline;
    a.alpha = (float*)workspace;
    a.part = a.alpha ? a.alpha + (size_t)num_shapes * num_views * C : nullptr;
    a.nchunks = 0;
    GV_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(explain_targets, dim3((num_shapes + 127) / 128), dim3(128), 0, st, logits,
                       (const long long*)targets, num_shapes, num_classes, (long long*)target_out, status);
    GV_LAUNCH_CHECK();
    const int vecn = dtype == GV_F32 ? 4 : 8;
    const bool vec = C % vecn == 0 && view_stride % vecn == 0 && shape_stride % vecn == 0 && gv_aligned16(F) &&
                     (!workspace || gv_aligned16(workspace));
    if (dtype == GV_F32) return ex_run<float, float>(a, kind, vec, st);
    if (dtype == GV_BF16) return ex_run<unsigned short, __bf16>(a, kind, vec, st);
    return ex_run<unsigned short, _Float16>(a, kind, vec, st);
}
