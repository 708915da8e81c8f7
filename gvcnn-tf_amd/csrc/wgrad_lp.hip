// wgrad_lp.hip — the filter gradient of 16-bit storage (configs[2]: bf16 forward + backward) on
// v_mfma_f32_32x32x16_{bf16,f16}: tap-per-workgroup tiles (conv_wgrad_lp), 32-pixel and 8 x 32 pixel strips
// (conv_wgrad_strip_lp) and the row strips of the 3-channel stems (conv_wgrad_stem_rows_lp), each with its launcher;
// gvlp::conv_wgrad / conv_wgrad_stem at the end choose among them by gv_conv_desc::tile_cfg (lowp.h: the table of
// configurations).  train.hip holds the extern "C" entry points, wgrad_dma.hip the LDS-DMA family.  dW stays fp32.
//
// The reduction axis is the PIXEL axis while both operands (the shifted input and dZ) are channel-contiguous in HBM,
// i.e. k-strided for the MFMA: the tiles are written to LDS as they arrive ([pixel][channel], ds_write_b128) and read
// back with gfx950's transposing ds_read_b64_tr_b16, which hands lane (channel i) four consecutive pixels of its column.
#include <math.h>

#include "lowp.h"
#include "lp_elem.h"

namespace {

using namespace gvlp_elem;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ---- filter gradient on the 16-bit MFMA ----------------------------------------------------------------------------
// dW[tap][ci][co] += sum_m X[shift_tap(m)][ci] * dZ[m][co].  One TN GEMM per filter tap; a workgroup owns a
// (64*TI) x (64*TO) tile of one tap and a slice of the pixels (slices are combined with fp32 atomics), 2x2 waves of
// TI x TO accumulators.  32 pixels per stage, LDS double buffered, the next stage's global loads are issued before
// this stage's MFMAs, one barrier per stage.
//   LDS rows = pixels, 2*B + 64 bytes apart: the four rows a transposed read touches per 16-lane group then start 16
//   dwords apart (conflict-free), and the 16-byte writes of 8 consecutive lanes fill one row's 128 bytes.
//   Operand of a 32-channel tile and 16 pixels k0..k0+15: lane l (channel c0 + l%32) needs pixels k0 + 8*(l/32) + 0..7 =
//   two ds_read_b64_tr_b16; in each, lane 4q+p of a 16-lane group supplies row q, channels 4p..4p+3 of the group's
//   16 channels.  Both operands use the same pixel order, so any consistent order is a valid k order.
template <typename T>
__device__ __forceinline__ f32x16 mfma16(s16x8 a, s16x8 b, f32x16 c) {
    if constexpr (__is_same(T, __bf16))
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ s16x4 lds_read_tr(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p));
}

template <typename T, int TI, int TO>
__global__ __launch_bounds__(256) void conv_wgrad_lp(const unsigned short* __restrict__ x, int x_ld,
                                                     const unsigned short* __restrict__ dz, int dz_ld, int nb, int ih,
                                                     int iw, int cin, int kh, int kw, int stride, int pad_t,
                                                     int pad_l, int oh, int ow, int cout, int64_t M,
                                                     int64_t m_per_block, const GvDw dw) {
    constexpr int PT = 32, BI = 64 * TI, BO = 64 * TO;
    constexpr int SX = 2 * BI + 64, SZ = 2 * BO + 64;                  // row strides in bytes
    constexpr int XV = PT * BI / 8 / 256, ZV = PT * BO / 8 / 256;      // 16-byte loads per thread and stage
    __shared__ __attribute__((aligned(16))) unsigned char sX[2][PT * SX];
    __shared__ __attribute__((aligned(16))) unsigned char sZ[2][PT * SZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int ntile_co = (cout + BO - 1) / BO, ntile_ci = (cin + BI - 1) / BI;
    // 1-D grid, XCD-aware: all tiles (taps x ci x co) of one PIXEL SLICE re-read the same X and dZ rows, so they get
    // consecutive logical ids = one XCD's L2 (round-robin dispatch would spread them over all eight)
    const int tiles = ntile_co * ntile_ci * kh * kw;
    const int logical = gv_xcd_remap((int)blockIdx.x, (int)gridDim.x);
    int b = logical % tiles;
    const int slice = logical / tiles;
    const int tco = b % ntile_co; b /= ntile_co;
    const int tci = b % ntile_ci; b /= ntile_ci;
    const int tap = b;
    const int fr = tap / kw, fs = tap - fr * kw;
    const int ci0 = tci * BI, co0 = tco * BO;
    const int64_t m0 = (int64_t)slice * m_per_block;
    const int64_t m1 = m0 + m_per_block < M ? m0 + m_per_block : M;
    f32x16 acc[TI][TO];
#pragma unroll
    for (int t = 0; t < TI; ++t)
#pragma unroll
        for (int u = 0; u < TO; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    const int ohow = oh * ow;
    u32x4 xr[XV], zr[ZV];
    auto load = [&](int64_t mt) {
#pragma unroll
        for (int j = 0; j < XV; ++j) {
            const int idx = tid + j * 256;
            const int p = idx / (BI / 8), c = ci0 + (idx % (BI / 8)) * 8;
            const int64_t m = mt + p;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m < m1 && c < cin) {
                const int n = (int)(m / ohow);
                const int rem = (int)(m - (int64_t)n * ohow);
                const int oy = rem / ow, ox = rem - oy * ow;
                const int iy = oy * stride + fr - pad_t, ix = ox * stride + fs - pad_l;
                if ((unsigned)iy < (unsigned)ih && (unsigned)ix < (unsigned)iw)
                    v = *reinterpret_cast<const u32x4*>(x + (((size_t)n * ih + iy) * iw + ix) * x_ld + c);
            }
            xr[j] = v;
        }
#pragma unroll
        for (int j = 0; j < ZV; ++j) {
            const int idx = tid + j * 256;
            const int p = idx / (BO / 8), c = co0 + (idx % (BO / 8)) * 8;
            const int64_t m = mt + p;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (m < m1 && c < cout) v = *reinterpret_cast<const u32x4*>(dz + (size_t)m * dz_ld + c);
            zr[j] = v;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < XV; ++j) {
            const int idx = tid + j * 256;
            *reinterpret_cast<u32x4*>(&sX[buf][(idx / (BI / 8)) * SX + (idx % (BI / 8)) * 16]) = xr[j];
        }
#pragma unroll
        for (int j = 0; j < ZV; ++j) {
            const int idx = tid + j * 256;
            *reinterpret_cast<u32x4*>(&sZ[buf][(idx / (BO / 8)) * SZ + (idx % (BO / 8)) * 16]) = zr[j];
        }
    };
    // transposed-read address of this lane inside a (16-pixel, 32-channel) operand block
    const int g16 = lane >> 4, q = (lane & 15) >> 2, p4 = lane & 3;
    const int row_l = 8 * (g16 >> 1) + q;                              // + 4*j for the second read
    const int col_l = 16 * (g16 & 1) + 4 * p4;                         // channel within the 32-channel tile
    const int xo = row_l * SX + 2 * ((wi * TI) * 32 + col_l);
    const int zo = row_l * SZ + 2 * ((wj * TO) * 32 + col_l);
    load(m0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int64_t mt = m0; mt < m1; mt += PT) {
        const bool more = mt + PT < m1;
        if (more) load(mt + PT);
#pragma unroll
        for (int k = 0; k < PT; k += 16) {
            s16x8 av[TI], bv[TO];
#pragma unroll
            for (int t = 0; t < TI; ++t) {
                const unsigned char* pa = &sX[buf][xo + k * SX + t * 64];
                const s16x4 lo = lds_read_tr(pa), hi = lds_read_tr(pa + 4 * SX);
                av[t] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int u = 0; u < TO; ++u) {
                const unsigned char* pb = &sZ[buf][zo + k * SZ + u * 64];
                const s16x4 lo = lds_read_tr(pb), hi = lds_read_tr(pb + 4 * SZ);
                bv[u] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int t = 0; t < TI; ++t)
#pragma unroll
                for (int u = 0; u < TO; ++u) acc[t][u] = mfma16<T>(av[t], bv[u], acc[t][u]);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    const int li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int u = 0; u < TO; ++u) {
        const int col = co0 + (wj * TO + u) * 32 + li;
        if (col >= cout) continue;
#pragma unroll
        for (int t = 0; t < TI; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + (wi * TI + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (ci < cin) gv_dw_put(dw, slice, ((size_t)tap * cin + ci) * cout + col, acc[t][u][r]);
            }
    }
}

// ---- filter gradient, strip form (stride-1 filters with more than one tap) ----------------------------------------
// The tap-per-workgroup kernel above re-reads dZ and X once per filter tap and is bound by L2->LDS traffic at
// 32-64 flop/byte.  Here a workgroup owns a tile (ci x co) for a GROUP OF TAPS (up to 9) and walks over "strips":
// up to 32 output pixels = R consecutive rows x L columns of one image.  Per strip it loads dZ ONCE ([32 slots][co])
// and the input patch with its halo ONCE ([(R+kh-1) x (L+kw-1) pixels][ci]); tap (r,s) of output slot (rho, ox) is
// LDS row (rho+r)*(L+kw-1) + ox+s, and because every lane of ds_read_b64_tr_b16 supplies its own row address the
// k-slot -> LDS-row map is free: the same patch serves every tap at a wave-uniform byte offset.  Accumulators: one
// 32x32 tile per (wave, tap).  Waves = WI x WJ x WT: WI x WJ sub-tiles of 32 channels, WT-way split of the taps
// (few-channel stem layers have only one 32x32 tile per tap).  One LDS buffer; the next strip's global loads are in
// flight (registers) while this strip's MFMAs run.
struct StripGeom {
    int nb, ih, iw, cin, kh, kw, pad_t, pad_l, oh, ow, cout;
    int R, L, Wx, Hx;             // strip rows/cols, patch width/height
    int nrs, ncs;                 // strips per image along y / x
    int tap0, ntaps;              // tap group of this launch slice: taps tap0 .. tap0+ntaps-1 (set per blockIdx.z)
    int stages, stages_per_block;
    int xrows;                    // Hx*Wx
    int x_ld, dz_ld;
};

// KS: 16-pixel k-steps per strip.  2: the strip of up to 32 pixels described above.  16 (the DEEP form, 32-channel inputs:
// Conv2d_2a / 2b): a strip is 8 rows x 32 columns of one image — the tile of the forward halo kernel — so that one fill of
// LDS (16 KB of dZ per 32 columns of co, 22 KB of input patch) and one barrier pair feed 16 x (taps per wave) MFMAs per
// wave instead of 2 x: the 32-pixel strips of a 109-wide map spend their time at barriers (6 MFMAs per wave between two).
template <typename T, int WI, int WJ, int WT, int NTW, int KS = 2>
__global__ __launch_bounds__(256) void conv_wgrad_strip_lp(const unsigned short* __restrict__ x,
                                                           const unsigned short* __restrict__ dz, StripGeom gm,
                                                           int taps_per_group, const GvDw dw) {
    static_assert(WI * WJ * WT == 4, "four waves");
    static_assert(KS == 2 || WI == 1, "the deep form: 32 input channels");
    constexpr int SLOTS = 16 * KS;
    constexpr int BI = 32 * WI, BO = 32 * WJ;
    // row strides: the four rows a transposed read touches per 16-lane group must start 16 dwords apart; a 32-channel
    // row IS 16 dwords (no padding: 2*B + 64 = 128 bytes would put rows q and q+2 on the same banks — measured 43 %
    // bank conflicts on the stem layers before this)
    constexpr int SX = BI == 32 ? 64 : 2 * BI + 64, SZ = BO == 32 ? 64 : 2 * BO + 64;
    constexpr int XC = BI / 8, ZC = BO / 8;                      // 16-byte chunks per LDS row
    constexpr int XVMAX = 6, ZV = (SLOTS * ZC + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* sZ = lds;
    unsigned char* sX = lds + SLOTS * SZ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wt = wave % WT, wj = (wave / WT) % WJ, wi = wave / (WT * WJ);
    const int ntile_co = (gm.cout + BO - 1) / BO, ntile_ci = (gm.cin + BI - 1) / BI;
    const int groups = (gm.kh * gm.kw + taps_per_group - 1) / taps_per_group;
    const int tiles = ntile_co * ntile_ci * groups;
    const int logical = gv_xcd_remap((int)blockIdx.x, (int)gridDim.x);   // tiles of one strip range share an XCD's L2
    int b = logical % tiles;
    const int tco = b % ntile_co; b /= ntile_co;
    const int tci = b % ntile_ci; b /= ntile_ci;
    const int tap0 = b * taps_per_group;
    const int ntaps = min(taps_per_group, gm.kh * gm.kw - tap0);
    const int ci0 = tci * BI, co0 = tco * BO;
    const int s0 = (logical / tiles) * gm.stages_per_block;
    const int s1 = min(s0 + gm.stages_per_block, gm.stages);
    if (s0 >= s1) return;
    f32x16 acc[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    // loader roles (strip-invariant): X chunk j of this thread -> patch pixel (py, px) and channel chunk
    const int xchunks = gm.xrows * XC;
    int xpy[XVMAX], xpx[XVMAX], xoff[XVMAX], xch[XVMAX];
#pragma unroll
    for (int j = 0; j < XVMAX; ++j) {
        const int idx = tid + j * 256;
        const int row = idx / XC;
        xch[j] = ci0 + (idx % XC) * 8;
        xpy[j] = row / gm.Wx;
        xpx[j] = row - xpy[j] * gm.Wx;
        xoff[j] = idx < xchunks ? row * SX + (idx % XC) * 16 : -1;
    }
    int zr[ZV], zc[ZV], zch[ZV], zoff[ZV];
#pragma unroll
    for (int j = 0; j < ZV; ++j) {
        const int idx = tid + j * 256;
        const int p = idx / ZC;                                  // k slot
        zr[j] = p / gm.L;
        zc[j] = p - zr[j] * gm.L;
        zch[j] = co0 + (idx % ZC) * 8;
        zoff[j] = idx < SLOTS * ZC ? p * SZ + (idx % ZC) * 16 : -1;
        if (zr[j] >= gm.R) zr[j] = -1;                           // padding slot: always zero
    }
    u32x4 xq[XVMAX], zq[ZV];
    auto load = [&](int stage) {
        const int cs = stage % gm.ncs;
        const int t = stage / gm.ncs;
        const int rs = t % gm.nrs;
        const int n = t / gm.nrs;
        const int oy0 = rs * gm.R, ox0 = cs * gm.L;
        const int lv = min(gm.L, gm.ow - ox0);                   // valid columns of this strip
#pragma unroll
        for (int j = 0; j < XVMAX; ++j) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (xoff[j] >= 0) {
                const int iy = oy0 - gm.pad_t + xpy[j], ix = ox0 - gm.pad_l + xpx[j];
                if ((unsigned)iy < (unsigned)gm.ih && (unsigned)ix < (unsigned)gm.iw && xch[j] < gm.cin)
                    v = *reinterpret_cast<const u32x4*>(x + (((size_t)n * gm.ih + iy) * gm.iw + ix) * gm.x_ld + xch[j]);
            }
            xq[j] = v;
        }
#pragma unroll
        for (int j = 0; j < ZV; ++j) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (zoff[j] >= 0 && zr[j] >= 0) {
                const int oy = oy0 + zr[j];
                if (oy < gm.oh && zc[j] < lv && zch[j] < gm.cout)
                    v = *reinterpret_cast<const u32x4*>(dz + (((size_t)n * gm.oh + oy) * gm.ow + ox0 + zc[j]) * gm.dz_ld + zch[j]);
            }
            zq[j] = v;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < XVMAX; ++j)
            if (xoff[j] >= 0) *reinterpret_cast<u32x4*>(sX + xoff[j]) = xq[j];
#pragma unroll
        for (int j = 0; j < ZV; ++j)
            if (zoff[j] >= 0) *reinterpret_cast<u32x4*>(sZ + zoff[j]) = zq[j];
    };
    // transposed-read addresses: k slot p = 16*ks + 8*(lane/32) + 4*j + q  ->  dZ row p, X row (p/L)*Wx + p%L (+ tap)
    const int g16 = lane >> 4, q = (lane & 15) >> 2, p4 = lane & 3;
    const int col_l = 16 * (g16 & 1) + 4 * p4;
    // (deep form: L = 32, so slot p = 16 ks + c is row ks / 2, column 16 (ks & 1) + c of the strip: one base per j, a
    // compile-time-unrolled offset per k-step)
    int xb[2][2], zb[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = 16 * ks + 8 * (g16 >> 1) + 4 * j + q;
            int rr = p / gm.L, cc = p - rr * gm.L;
            if (rr >= gm.R) { rr = 0; cc = 0; }                  // padding slot: dZ is zero there, any row will do
            xb[ks][j] = (rr * gm.Wx + cc) * SX + 2 * (wi * 32 + col_l);
            zb[ks][j] = p * SZ + 2 * (wj * 32 + col_l);
        }
    const int xstep = gm.Wx * SX;                                // deep form: one strip row further down the patch
    int tapoff[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int tap = tap0 + wt + WT * i;
        const int fr = tap / gm.kw, fs = tap - fr * gm.kw;
        tapoff[i] = (fr * gm.Wx + fs) * SX;
    }
    load(s0);
    for (int stage = s0; stage < s1; ++stage) {
        store();
        __syncthreads();
        if (stage + 1 < s1) load(stage + 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            // (KS = 2: the tables; deep: k-step ks = row ks / 2 of the strip, half ks & 1 of its 32 columns)
            const int zo = KS == 2 ? 0 : (ks >> 1) * 32 * SZ, xo = KS == 2 ? 0 : (ks >> 1) * xstep;
            const s16x4 blo = lds_read_tr(sZ + zb[ks & 1][0] + zo), bhi = lds_read_tr(sZ + zb[ks & 1][1] + zo);
            const s16x8 bv = __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                if (wt + WT * i < ntaps) {                       // wave-uniform
                    const s16x4 alo = lds_read_tr(sX + xb[ks & 1][0] + tapoff[i] + xo);
                    const s16x4 ahi = lds_read_tr(sX + xb[ks & 1][1] + tapoff[i] + xo);
                    const s16x8 av = __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[i] = mfma16<T>(av, bv, acc[i]);
                }
            }
        }
        __syncthreads();
    }
    const int li = lane & 31, lh = lane >> 5;
    const int col = co0 + wj * 32 + li;
    if (col < gm.cout) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            if (wt + WT * i >= ntaps) continue;
            const int tap = tap0 + wt + WT * i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (ci < gm.cin) gv_dw_put(dw, logical / tiles, ((size_t)tap * gm.cin + ci) * gm.cout + col, acc[i][r]);
            }
        }
    }
}

// Launch geometry: d->tile_cfg = 0 picks the side widths by divisibility and ~2048 workgroups; tile_cfg = 1 + tile +
// 9*split selects tile (TI,TO) in {1,2,3}^2 (64/128/192 channels per side) and a target of 1024 / 2048 / 4096
// workgroups; 28..30 the strip form (TrainGVCNN.autotune measures them per layer).
// strip form: geometry and eligibility
inline bool strip_geom(const gv_conv_desc* d, int dz_ld, int bi, StripGeom* gm, bool deep = false) {
    if (d->stride != 1 || d->kh * d->kw < 2) return false;
    StripGeom& g = *gm;
    g.nb = d->nb; g.ih = d->ih; g.iw = d->iw; g.cin = d->cin; g.kh = d->kh; g.kw = d->kw;
    g.pad_t = d->pad_t; g.pad_l = d->pad_l; g.oh = d->oh; g.ow = d->ow; g.cout = d->cout;
    g.x_ld = d->x_ld; g.dz_ld = dz_ld;
    if (deep) {                                                  // 8 rows x 32 columns per strip (KS = 16)
        if (bi != 32 || d->ow < 24 || d->oh < 8) return false;
        g.ncs = (d->ow + 31) / 32;
        g.L = 32;
        g.R = 8;
    } else if (d->ow >= 32) {
        g.ncs = (d->ow + 31) / 32;
        g.L = (d->ow + g.ncs - 1) / g.ncs;
        g.R = 1;
    } else {
        g.ncs = 1;
        g.L = d->ow;
        g.R = 32 / d->ow;
        if (g.R > d->oh) g.R = d->oh;
    }
    g.nrs = (d->oh + g.R - 1) / g.R;
    g.Wx = g.L + d->kw - 1;
    g.Hx = g.R + d->kh - 1;
    g.xrows = g.Hx * g.Wx;
    const int64_t stages = (int64_t)d->nb * g.nrs * g.ncs;
    if (stages > 0x7fffffff) return false;
    g.stages = (int)stages;
    if (g.xrows * (bi / 8) > 6 * 256) return false;              // XVMAX chunks per thread
    if (!deep && (int64_t)g.xrows * (2 * bi + 64) + 32 * (2 * 128 + 64) > 64 * 1024) return false;
    return true;
}

template <typename T, int WI, int WJ, int WT, int NTW, int KS = 2>
int strip_launch(const gv_conv_desc* d, const unsigned short* x, const unsigned short* dz, int dz_ld, const GvDw& dw,
                 int target_wgs, hipStream_t st) {
    constexpr int BI = 32 * WI, BO = 32 * WJ;
    StripGeom gm;
    if (!strip_geom(d, dz_ld, BI, &gm, KS != 2)) return GV_E_UNSUPPORTED;
    const int taps = d->kh * d->kw, tpg = NTW * WT;              // taps per workgroup
    const int groups = (taps + tpg - 1) / tpg;
    const int tiles = ((d->cin + BI - 1) / BI) * ((d->cout + BO - 1) / BO) * groups;
    const size_t elems = (size_t)taps * d->cin * d->cout;
    // at least 8 strips per workgroup (deep: 3 of 256 pixels)
    const GvSlices p = gv_dw_plan(dw, elems, gm.stages, tiles, target_wgs, KS == 2 ? 8 : 3, 1, 65535);
    const int64_t splits = p.splits;
    gm.stages_per_block = (int)p.per;
    const size_t lds = (size_t)(16 * KS) * (BO == 32 ? 64 : 2 * BO + 64) + (size_t)gm.xrows * (BI == 32 ? 64 : 2 * BI + 64);
    auto kern = conv_wgrad_strip_lp<T, WI, WJ, WT, NTW, KS>;
    // the deep form needs the raised LDS limit; the 32-pixel strips fit 64 KB (strip_geom) and only ask
    const bool attr = GV_BIG_LDS_OK(kern, KS == 2 ? 64 * 1024 : 96 * 1024);
    if (KS != 2 && !attr) return GV_E_UNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * splits)), dim3(256), lds, st, x, dz, gm, tpg,
                       gv_dw_sink(dw, elems, splits));
    GV_LAUNCH_CHECK();
    return gv_dw_finish(dw, elems, splits, st);
}

template <typename T>
int strip_t(const gv_conv_desc* d, const unsigned short* x, const unsigned short* dz, int dz_ld, const GvDw& dw,
            int target_wgs, hipStream_t st) {
    if (d->cin <= 32 && d->cout <= 32) return strip_launch<T, 1, 1, 4, 3>(d, x, dz, dz_ld, dw, target_wgs, st);
    if (d->cin <= 32) return strip_launch<T, 1, 2, 2, 5>(d, x, dz, dz_ld, dw, target_wgs, st);
    if (d->cout <= 32) return strip_launch<T, 2, 1, 2, 5>(d, x, dz, dz_ld, dw, target_wgs, st);
    const int ntw = gvlp::wgrad_strip_taps();                     // (5 unless a tool asked for 4 or 9)
    if (ntw == 5) return strip_launch<T, 2, 2, 1, 5>(d, x, dz, dz_ld, dw, target_wgs, st);
    if (ntw == 4) return strip_launch<T, 2, 2, 1, 4>(d, x, dz, dz_ld, dw, target_wgs, st);
    return strip_launch<T, 2, 2, 1, 9>(d, x, dz, dz_ld, dw, target_wgs, st);
}

// the deep form (8 x 32 pixel strips): 32 input channels, 32 or 64 output channels
template <typename T>
int strip_deep_t(const gv_conv_desc* d, const unsigned short* x, const unsigned short* dz, int dz_ld, const GvDw& dw,
                 int target_wgs, hipStream_t st) {
    // (measured on wider layers too — Conv2d_4a 80 -> 192: equal to the LDS-DMA form at best; Mixed_5's 3x3 / 5x5 on 25 x 25
    // maps: 20-40 % slower — so the form stays with the layers it wins on)
    if (d->cin > 32 || d->cout > 64) return GV_E_UNSUPPORTED;
    if (d->cout <= 32) return strip_launch<T, 1, 1, 4, 3, 16>(d, x, dz, dz_ld, dw, target_wgs, st);
    return strip_launch<T, 1, 2, 2, 5, 16>(d, x, dz, dz_ld, dw, target_wgs, st);
}

// the tap-per-workgroup tiles: sides of 64 * ti and 64 * to channels, ~target workgroups of at least 512 pixels
template <typename T>
int tiles_launch(const gv_conv_desc* d, const unsigned short* x, const unsigned short* dz, int dz_ld, const GvDw& dw,
                 int ti, int to, int target, hipStream_t st) {
    const int tiles = d->kh * d->kw * ((d->cin + 64 * ti - 1) / (64 * ti)) * ((d->cout + 64 * to - 1) / (64 * to));
    const size_t elems = (size_t)d->kh * d->kw * d->cin * d->cout;
    const GvSlices p = gv_dw_plan(dw, elems, (int64_t)d->nb * d->oh * d->ow, tiles, target, 512, 32, 65535);
    const dim3 grid((unsigned)(tiles * p.splits));
    const GvDw sink = gv_dw_sink(dw, elems, p.splits);
    int rc = GV_E_BADARG;
#define GV_WGRAD_LP(TI, TO) \
    case TI * 10 + TO: rc = gv_wgrad_launch<conv_wgrad_lp<T, TI, TO>>(grid, d, x, dz, dz_ld, p.per, sink, st); break
    switch (ti * 10 + to) {
        GV_WGRAD_LP(1, 1); GV_WGRAD_LP(1, 2); GV_WGRAD_LP(1, 3);
        GV_WGRAD_LP(2, 1); GV_WGRAD_LP(2, 2); GV_WGRAD_LP(2, 3);
        GV_WGRAD_LP(3, 1); GV_WGRAD_LP(3, 2); GV_WGRAD_LP(3, 3);
    }
#undef GV_WGRAD_LP
    return rc != GV_OK ? rc : gv_dw_finish(dw, elems, p.splits, st);
}

// workgroup targets of the families' configurations, by local index
constexpr int kTileTargets[] = {1024, 2048, 4096};               // x 9 sides: local = 9 * (index here) + 3 * (to - 1) + (ti - 1)
constexpr int kStripTargets[] = {1024, 2048, 4096};
constexpr int kDeepTargets[] = {512, 768, 1024, 2048, 4096};
static_assert(9 * sizeof(kTileTargets) / sizeof(int) == gvlp::wgrad_family_count(gvlp::WGRAD_TILES) &&
                  sizeof(kStripTargets) / sizeof(int) == gvlp::wgrad_family_count(gvlp::WGRAD_STRIPS) &&
                  sizeof(kDeepTargets) / sizeof(int) == gvlp::wgrad_family_count(gvlp::WGRAD_DEEP),
              "lowp.h: the families' counts");

template <typename T>
int wgrad_t(const gv_conv_desc* d, const unsigned short* x, const unsigned short* dz, int dz_ld, const GvDw& dw,
            hipStream_t st) {
    if (d->tile_cfg > gvlp::wgrad_num_cfgs()) return GV_E_BADARG;
    const gvlp::WgradRef c = gvlp::wgrad_lookup(d->tile_cfg);
    switch (c.fam) {
        case gvlp::WGRAD_TILES:
            return tiles_launch<T>(d, x, dz, dz_ld, dw, 1 + c.local % 3, 1 + c.local % 9 / 3, kTileTargets[c.local / 9], st);
        case gvlp::WGRAD_STRIPS: return strip_t<T>(d, x, dz, dz_ld, dw, kStripTargets[c.local], st);
        case gvlp::WGRAD_DMA: return gvlp::conv_wgrad_dma_launch(d, x, dz, dz_ld, dw, c.local, st);
        case gvlp::WGRAD_DEEP: {                                 // layers the deep form declines: the 32-pixel strips
            const int rc = strip_deep_t<T>(d, x, dz, dz_ld, dw, kDeepTargets[c.local], st);
            return rc != GV_E_UNSUPPORTED ? rc : strip_t<T>(d, x, dz, dz_ld, dw, kDeepTargets[c.local], st);
        }
        case gvlp::WGRAD_NONE: break;
    }
    // tile_cfg 0 (and below): the first of these that takes the layer
    // 1. the strip form for the few-channel stem layers (2.5-3.5x there); its general 64x64x9-tap variant runs at one wave per
    //    SIMD and loses to the tap-per-workgroup tiles — autotune may still pick it
    if (d->tile_cfg == 0 && d->cin <= 32) {
        const int rc = strip_t<T>(d, x, dz, dz_ld, dw, 2048, st);
        if (rc != GV_E_UNSUPPORTED) return rc;
    }
    // 2. the two-stage LDS-DMA form (fastest on 64 of Inception-v3's 67 layers), 128-channel sides where the layer has them,
    //    ~2048 workgroups
    if (d->tile_cfg == 0) {
        const int k = gvlp::wgrad_dma_find(d->cin >= 128 ? 2 : 1, d->cout >= 128 ? 2 : 1, 2, 32, 2048);
        const int rc = k < 0 ? GV_E_UNSUPPORTED : gvlp::conv_wgrad_dma_launch(d, x, dz, dz_ld, dw, k, st);   // (no such row: the tiles)
        if (rc != GV_E_UNSUPPORTED) return rc;
    }
    // 3. the tiles, sides 64 / 128 / 192 channels wide: the widest that pads no more channels than 64-wide tiles would (a
    //    192-wide side triples the flop/byte of this L2->LDS bound kernel on the many 192-channel layers)
    auto side = [](int c) {
        const int base = (c + 63) / 64 * 64;
        if ((c + 191) / 192 * 192 == base) return 3;
        if ((c + 127) / 128 * 128 == base) return 2;
        return 1;
    };
    return tiles_launch<T>(d, x, dz, dz_ld, dw, side(d->cin), side(d->cout), 2048, st);
}


// ---- filter gradient of the 3-channel stems (Conv2d_1a 3x3/2, ResNet conv1 7x7/2) on the 16-bit MFMA -----------------------
// dW[rho][co] = sum over pixels of X[pixel shifted by tap(rho)][ci(rho)] * dZ[pixel][co], rho = tap*cin + ci: 27 (147)
// rows of 32 (64) columns over millions of pixels — a reduction, HBM-bound by construction (Conv2d_1a: 116 MB of
// images + 303 MB of dZ per step).  The direct kernel (train.hip: conv_wgrad_direct_f32) gathers both operands with
// 2-byte loads, one per lane and pixel, and multiplies on the fp32 MFMA (2 pixels per instruction): 0.48 ms at 17 TFLOP/s.
// Here a WAVE owns a run of (image, output row) units.  Per unit it copies the kh input rows and the one dZ row into its
// private LDS area with 16-byte loads (both are contiguous in memory), one unit ahead in registers, and multiplies
// 16 pixels per v_mfma_f32_32x32x16: the dZ operand comes back through the transposing ds_read_b64_tr_b16 (lane =
// channel, 4 consecutive pixels per read), the image operand as 8 two-byte LDS reads per lane at a 2*stride*cin-byte
// pitch (row rho of the operand is one (filter row, column, channel) = one fixed offset into the staged rows).  No
// barrier inside the loop (a wave reads only what it wrote); the four waves' accumulators are summed in LDS and
// leave as one fp32 atomic per (rho, co) and workgroup.
// ZL: 16-byte loads per lane that hold the unit's dZ row (10: rows up to 640 chunks — Conv2d_1a's 111 x 32; 14: ResNet conv1's
// 112 pixels x 64 channels = 896 chunks, 96 KB of LDS per workgroup — one workgroup per CU, whose four waves keep 24 loads per
// lane in flight each: the layer was 2.75 ms on the fp32-MFMA fallback, 9 % of the ResNet training step).
template <typename T, int NRT, int NCT, int ZL = 10>
__global__ __launch_bounds__(256) void conv_wgrad_stem_rows_lp(const unsigned short* __restrict__ x,
                                                               const unsigned short* __restrict__ dz, int dz_ld, int nb,
                                                               int ih, int iw, int cin, int kh, int kw, int stride,
                                                               int pad_t, int pad_l, int oh, int ow, int cout, int xrow_b,
                                                               int zrows, int units_per_wave, const GvDw dw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_w[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int ZB = NCT * 64;                                       // bytes of one dZ pixel row in LDS
    const int wave_b = kh * xrow_b + zrows * ZB;                   // this wave's area: kh image rows, then the dZ row
    unsigned char* sXw = smem_w + wave * wave_b;
    unsigned char* sZw = sXw + kh * xrow_b;
    for (int i = lane * 16; i < wave_b; i += 1024) *reinterpret_cast<u32x4*>(sXw + i) = u32x4{0u, 0u, 0u, 0u};
    const int R = kh * kw * cin;
    // image rows sit pad_l pixels (+ xoff bytes, so that their 4-byte pieces stay aligned: ResNet conv1 pads 3 pixels of 6 bytes)
    // into their LDS rows; what is in front stays zero
    const int xoff = (4 - ((pad_l * cin * 2) & 3)) & 3;
    int abase[NRT];                                                // byte offset of operand row rho at output column 0
#pragma unroll
    for (int t = 0; t < NRT; ++t) {
        const int rho = min(t * 32 + li, R - 1);                   // (rows past R: any finite data; never stored)
        const int tap = rho / cin, ci = rho - tap * cin;
        const int r = tap / kw, sx = tap - r * kw;
        abase[t] = r * xrow_b + xoff + (sx * cin + ci) * 2;
    }
    const int apitch = stride * cin * 2;                           // bytes between consecutive output columns
    // transposed-read address of this lane inside a (16-pixel, 32-channel) block of the dZ row (see conv_wgrad_lp)
    const int g16 = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int zoff = (8 * (g16 >> 1) + q4) * ZB + 2 * (16 * (g16 & 1) + 4 * p4);
    const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
    const int64_t units = (int64_t)nb * oh;
    const int64_t u0 = wid * units_per_wave;
    const int64_t u1 = u0 + units_per_wave < units ? u0 + units_per_wave : units;
    f32x16 acc[NRT][NCT];
#pragma unroll
    for (int t = 0; t < NRT; ++t)
#pragma unroll
        for (int u = 0; u < NCT; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    constexpr int XL = NRT == 1 ? 6 : 10;                          // 16-byte loads per lane: image rows (capacity; ZL: the dZ row)
    const int xbytes = iw * cin * 2;                               // one image row (contiguous: x_ld == cin)
    const int xchunks = (kh * xbytes + 15) / 16, zchunks = ow * (NCT * 4);
    u32x4 xr[XL], zr[ZL];
    auto fetch = [&](int64_t u) {
        const int n = (int)(u / oh), oy = (int)(u - (int64_t)n * oh);
        const int iy0 = oy * stride - pad_t;
#pragma unroll
        for (int k = 0; k < XL; ++k) {
            const int c = lane + 64 * k;                           // chunk c covers bytes [16c, 16c + 16) of the kh rows
            u32x4 v = {0u, 0u, 0u, 0u};
            if (c < xchunks) {
                const int row = (c * 16) / xbytes;                 // (a chunk may straddle two rows: both must be inside)
                const int row2 = (c * 16 + 15) / xbytes;
                const int iyA = iy0 + row, iyB = iy0 + (row2 < kh ? row2 : kh - 1);
                if (iyA >= 0 && iyB < ih)
                    v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(x) +
                                                        ((size_t)n * ih + iy0) * xbytes + (size_t)c * 16);
            }
            xr[k] = v;
        }
#pragma unroll
        for (int k = 0; k < ZL; ++k) {
            const int c = lane + 64 * k;                           // (pixel, 8-channel chunk)
            u32x4 v = {0u, 0u, 0u, 0u};
            if (c < zchunks) {
                const int px = c / (NCT * 4), ch = (c - px * (NCT * 4)) * 8;
                if (ch < cout) v = *reinterpret_cast<const u32x4*>(dz + ((size_t)u * ow + px) * dz_ld + ch);
            }
            zr[k] = v;
        }
    };
    auto stage = [&]() {                                           // registers -> this wave's LDS area
#pragma unroll
        for (int k = 0; k < XL; ++k) {
            const int c = lane + 64 * k;
            if (c < xchunks) {
                const int b0 = c * 16;                             // (rows xrow_b apart)
#pragma unroll
                for (int w4 = 0; w4 < 4; ++w4) {                   // 4-byte pieces: a chunk may straddle two rows
                    const int b = b0 + 4 * w4, row = b / xbytes, off = b - row * xbytes;
                    if (row < kh) *reinterpret_cast<unsigned*>(sXw + row * xrow_b + xoff + pad_l * cin * 2 + off) = xr[k][w4];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < ZL; ++k) {
            const int c = lane + 64 * k;
            if (c < zchunks) *reinterpret_cast<u32x4*>(sZw + (c / (NCT * 4)) * ZB + (c % (NCT * 4)) * 16) = zr[k];
        }
    };
    if (u0 < u1) fetch(u0);
    for (int64_t u = u0; u < u1; ++u) {
        __builtin_amdgcn_wave_barrier();
        stage();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        if (u + 1 < u1) fetch(u + 1);                              // in flight under this unit's reads and MFMAs
        for (int k0 = 0; k0 < ow; k0 += 16) {
            s16x8 bv[NCT];
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const unsigned char* pb = sZw + zoff + k0 * ZB + c * 64;
                const s16x4 lo = lds_read_tr(pb), hi = lds_read_tr(pb + 4 * ZB);
                bv[c] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int t = 0; t < NRT; ++t) {
                s16x8 av;
                const unsigned char* pa = sXw + abase[t] + (k0 + 8 * lh) * apitch;
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] = *reinterpret_cast<const short*>(pa + j * apitch);
#pragma unroll
                for (int c = 0; c < NCT; ++c) acc[t][c] = mfma16<T>(av, bv[c], acc[t][c]);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // every read of this unit done before it is overwritten
    }
    // the four waves' tiles -> LDS -> one atomic per element
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem_w);                 // [4][NRT*NCT][32 x 32]
#pragma unroll
    for (int t = 0; t < NRT; ++t)
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                red[((wave * NRT + t) * NCT + c) * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = acc[t][c][r];
    __syncthreads();
    for (int i = threadIdx.x; i < NRT * NCT * 1024; i += 256) {
        const int tc = i >> 10, e = i & 1023;
        const int t = tc / NCT, c = tc - t * NCT;
        const int rho = t * 32 + (e >> 5), co = c * 32 + (e & 31);
        if (rho < R && co < cout) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) v += red[(w * NRT * NCT + tc) * 1024 + e];
            gv_dw_put(dw, blockIdx.x, (size_t)rho * cout + co, v);
        }
    }
}

// (above 64 KB of LDS — the wide form's dZ rows — gv_launch raises the kernel's limit first)
template <auto Kernel>
int stem_launch(int64_t nwg, size_t lds, const gv_conv_desc* d, const unsigned short* x, const unsigned short* dz, int dz_ld,
                int xrow_b, int zrows, int64_t per, const GvDw& sink, hipStream_t st) {
    return gv_launch<Kernel>(dim3((unsigned)nwg), dim3(256), lds, st, x, dz, dz_ld, d->nb, d->ih, d->iw, d->cin, d->kh, d->kw,
                             d->stride, d->pad_t, d->pad_l, d->oh, d->ow, d->cout, xrow_b, zrows, (int)per, sink);
}

// the stems this kernel takes: 3 input channels stored densely (x_ld == cin), stride 2, <= 64 output channels, rows that
// fit the per-lane staging registers; 0 on success, GV_E_UNSUPPORTED otherwise
template <typename T>
int wgrad_stem_rows(const gv_conv_desc* d, const unsigned short* x, const unsigned short* dz, int dz_ld, const GvDw& dw,
                    hipStream_t st) {
    const int R = d->kh * d->kw * d->cin;
    const int nrt = (R + 31) / 32, nct = (d->cout + 31) / 32;
    if (d->cin > 4 || d->x_ld != d->cin || d->stride != 2 || (nrt != 1 && nrt != 5) || nct > 2 || d->cout % 8 != 0 ||
        dz_ld % 8 != 0 || !gv_aligned16(x) || !gv_aligned16(dz) || (d->iw * d->cin * 2) % 16 != 0)
        return GV_E_UNSUPPORTED;
    const int xbytes = d->iw * d->cin * 2;
    // what a lane's staging registers hold (XL / ZL of the kernel), and 4-byte aligned rows behind the left padding
    const bool wide = d->ow * nct * 4 > 10 * 64;                   // the dZ row needs the 14-load form (nrt == 5, nct == 2 only)
    if ((d->kh * xbytes + 15) / 16 > (nrt == 1 ? 6 : 10) * 64 || d->ow * nct * 4 > (nrt == 5 && nct == 2 ? 14 : 10) * 64 ||
        xbytes % 4 != 0)
        return GV_E_UNSUPPORTED;
    // LDS row of the image: left padding + iw pixels + the columns the last (padded to 16) output pixels reach
    const int owp = (d->ow + 15) / 16 * 16;
    const int need_px = (owp - 1) * d->stride + d->kw;
    const int row_px = need_px > d->iw + d->pad_l ? need_px : d->iw + d->pad_l;
    const int xrow_b = (row_px * d->cin * 2 + 15) / 16 * 16 + 16;
    const int zrows = owp;
    const size_t wave_b = (size_t)d->kh * xrow_b + (size_t)zrows * nct * 64;
    size_t lds = 4 * wave_b;
    const size_t red_b = (size_t)4 * nrt * nct * 1024 * 4;
    if (red_b > lds) lds = red_b;
    if (lds > (wide ? 160 : 64) * 1024) return GV_E_UNSUPPORTED;
    const int64_t units = (int64_t)d->nb * d->oh;
    int64_t waves = 256 * (wide ? 1 : 3) * 4;                      // three workgroups per CU (the wide form: one)
    int64_t per = (units + waves - 1) / waves;
    if (per < 4) per = 4;
    int64_t nwg = ((units + per - 1) / per + 3) / 4;
    const size_t elems = (size_t)R * d->cout;
    if (gv_dw_clamp(dw, elems, nwg) < nwg) {                      // fewer workgroups (slices) than wanted: what the workspace holds
        nwg = gv_dw_clamp(dw, elems, nwg);
        per = (units + 4 * nwg - 1) / (4 * nwg);
        nwg = ((units + per - 1) / per + 3) / 4;
    }
    const GvDw sink = gv_dw_sink(dw, elems, nwg);
    const auto launch = wide                   ? stem_launch<conv_wgrad_stem_rows_lp<T, 5, 2, 14>>
                        : nrt == 1 && nct == 1 ? stem_launch<conv_wgrad_stem_rows_lp<T, 1, 1>>
                        : nrt == 1             ? stem_launch<conv_wgrad_stem_rows_lp<T, 1, 2>>
                        : nct == 1             ? stem_launch<conv_wgrad_stem_rows_lp<T, 5, 1>>
                                               : stem_launch<conv_wgrad_stem_rows_lp<T, 5, 2>>;
    const int rc = launch(nwg, lds, d, x, dz, dz_ld, xrow_b, zrows, per, sink, st);
    return rc != GV_OK ? rc : gv_dw_finish(dw, elems, nwg, st);
}

}  // namespace

namespace gvlp {

bool wgrad_mfma_ok(const gv_conv_desc* d, const void* x, const void* dz, int dz_ld) {
    return d->cin % 8 == 0 && d->cout % 8 == 0 && d->x_ld % 8 == 0 && dz_ld % 8 == 0 && gv_aligned16(x) &&
           gv_aligned16(dz);
}

int conv_wgrad(const gv_conv_desc* d, const void* x, const void* dz, int dz_ld, const GvDw& dw, hipStream_t st) {
    GV_LP_DISPATCH(d->dtype, return wgrad_t<T>(d, (const unsigned short*)x, (const unsigned short*)dz, dz_ld, dw, st));
}

// the 3-channel stems on the 16-bit MFMA (conv_wgrad_stem_rows_lp); GV_E_UNSUPPORTED: not such a layer
int conv_wgrad_stem(const gv_conv_desc* d, const void* x, const void* dz, int dz_ld, const GvDw& dw, hipStream_t st) {
    GV_LP_DISPATCH(d->dtype, return wgrad_stem_rows<T>(d, (const unsigned short*)x, (const unsigned short*)dz, dz_ld, dw, st));
}

}  // namespace gvlp
