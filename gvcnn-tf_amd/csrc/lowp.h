// Internal entry points of the training kernels: the extern "C" functions of train.hip validate their arguments and
// dispatch here on dtype.
#pragma once
#include "gv_common.h"

namespace gvlp {

// train_lp.hip: the HBM-bound ops of the training step for every storage type (dtype GV_F32 | GV_BF16 | GV_F16), and the
// filter gradient of 16-bit storage
int accumulate(int dtype, const void* src, int src_ld, void* dst, int dst_ld, int64_t npix, int c, hipStream_t st);
int grouped_sums(int dtype, int mode, const void* z, int z_ld, const void* dy, int dy_ld, const void* y, int y_ld,
                 const float* mean, const float* inv, const float* scale, const float* shift, int nb, int hw, int c,
                 int G, int splits, double* acc, hipStream_t st);
int scale_shift_act_grouped(int dtype, const void* x, int nb, int hw, int c, int x_ld, const float* scale,
                            const float* shift, int G, int relu, void* y, int y_ld, hipStream_t st);
int bn_bwd_apply_grouped(int dtype, const void* dy, int dy_ld, const void* y, int y_ld, const void* z, int z_ld,
                         const float* mean, const float* inv, const float* gamma, const double* acc, const int* counts,
                         const float* scale, const float* shift, int accumulate, int nb, int hw, int c, int G, void* dz,
                         int dz_ld, float* dbeta, float* dgamma, bool* param_grads_done, hipStream_t st, int raw_z = 0);
int bn_finalize_apply_grouped(int dtype, const double* acc, const int* counts, const float* gamma, const float* beta,
                              float eps, const void* x, int nb, int hw, int c, int x_ld, int G, int relu, void* y,
                              int y_ld, float* mean, float* var, float* inv, float* scale, float* shift, hipStream_t st);
// pool_train.hip: the pooling ops of the training step (d->dtype: every storage type)
int pool2d_bwd(const gv_pool_desc* d, const void* x, const void* dy, int dy_ld, void* dx, int dx_ld, hipStream_t st);
int pool2d_fwd_argmax(const gv_pool_desc* d, const void* x, void* y, unsigned char* arg, hipStream_t st);
int pool2d_bwd_argmax(const gv_pool_desc* d, const unsigned char* arg, const void* dy, int dy_ld, void* dx, int dx_ld,
                      hipStream_t st, const void* bn_z = nullptr, int bn_z_ld = 0, int bn_G = 1, const float* bn_A = nullptr,
                      const float* bn_B = nullptr, const float* bn_C = nullptr, const float* bn_scale = nullptr,
                      const float* bn_shift = nullptr);
// train_lp.hip
int bn_bwd_coeffs_launch(const double* acc, const int* counts, const float* mean, const float* inv, const float* gamma,
                         int c, int G, int raw_z, float* A, float* B, float* Cc, float* dbeta, float* dgamma, hipStream_t st);
int view_pool_fuse_bwd(int dtype, const void* F, const float* dS, int V, int N, int64_t E, int64_t vs, int64_t ss,
                       const int* scheme, int G, const float* weight, int mode, void* dF, hipStream_t st,
                       int64_t scheme_stride, int64_t weight_stride);
bool wgrad_mfma_ok(const gv_conv_desc* d, const void* x, const void* dz, int dz_ld);
int conv_wgrad(const gv_conv_desc* d, const void* x, const void* dz, int dz_ld, const GvDw& dw, hipStream_t st);
int conv_wgrad_stem(const gv_conv_desc* d, const void* x, const void* dz, int dz_ld, const GvDw& dw, hipStream_t st);

// ---- the configurations of the 16-bit filter gradient -------------------------------------------------------------------
// gv_conv_desc::tile_cfg (1-based; 0: the heuristic) names one launch configuration.  The table is the kernel families IN
// ORDER, each with as many indices as it has configurations: the one place that says which index is whose.  The autotuner,
// tools, documents and tests hold indices as numbers: append to the last family or add a family, never reorder.
enum WgradFamily {
    WGRAD_TILES,       // tap-per-workgroup tiles (conv_wgrad_lp): sides (TI, TO) in {1,2,3}^2 x 1024 / 2048 / 4096 workgroups
    WGRAD_STRIPS,      // 32-pixel strips (conv_wgrad_strip_lp): 1024 / 2048 / 4096 workgroups
    WGRAD_DMA,         // LDS-DMA staging (wgrad_dma.hip: its table of tiles, ring depths and targets)
    WGRAD_DEEP,        // 8 x 32 pixel strips: 512 / 768 / 1024 / 2048 / 4096 workgroups
    WGRAD_NONE
};
struct WgradRange { WgradFamily fam; int count; };
struct WgradRef { WgradFamily fam; int local; };             // configuration `local` of family `fam`
constexpr WgradRange kWgradTable[] = {{WGRAD_TILES, 27}, {WGRAD_STRIPS, 3}, {WGRAD_DMA, 61}, {WGRAD_DEEP, 5}};

constexpr int wgrad_family_count(WgradFamily fam) {
    for (const WgradRange& r : kWgradTable)
        if (r.fam == fam) return r.count;
    return 0;
}
constexpr int wgrad_num_cfgs() {
    int n = 0;
    for (const WgradRange& r : kWgradTable) n += r.count;
    return n;
}
// tile_cfg -> (family, local index); WGRAD_NONE for 0 and outside the table
inline WgradRef wgrad_lookup(int tile_cfg) {
    int k = tile_cfg - 1;
    for (const WgradRange& r : kWgradTable) {
        if (k < 0) break;
        if (k < r.count) return {r.fam, k};
        k -= r.count;
    }
    return {WGRAD_NONE, 0};
}
int wgrad_strip_taps();                                       // train.hip: gv_conv2d_wgrad_set_strip_taps
// wgrad_dma.hip: configuration k of the LDS-DMA family; the first one with these properties, -1 if there is none
int conv_wgrad_dma_launch(const gv_conv_desc* d, const void* x, const void* dz, int dz_ld, const GvDw& dw, int k, hipStream_t st);
int wgrad_dma_find(int ti, int to, int stages, int stage_pixels, int target_wgs);

}  // namespace gvlp
