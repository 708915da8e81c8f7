// Internal entry points of the training kernels that live in a file of their own: the extern "C" functions of train.hip
// validate their arguments and dispatch here.
#pragma once
#include "gv_common.h"

namespace gvlp {

// pool_train.hip: the pooling ops of the training step (d->dtype: every storage type)
int pool2d_bwd(const gv_pool_desc* d, const void* x, const void* dy, int dy_ld, void* dx, int dx_ld, hipStream_t st);
int pool2d_fwd_argmax(const gv_pool_desc* d, const void* x, void* y, unsigned char* arg, hipStream_t st);
int pool2d_bwd_argmax(const gv_pool_desc* d, const unsigned char* arg, const void* dy, int dy_ld, void* dx, int dx_ld,
                      hipStream_t st, const void* bn_z = nullptr, int bn_z_ld = 0, int bn_G = 1, const float* bn_A = nullptr,
                      const float* bn_B = nullptr, const float* bn_C = nullptr, const float* bn_scale = nullptr,
                      const float* bn_shift = nullptr);
// wgrad_lp.hip: the filter gradient of 16-bit storage on the 16-bit MFMA
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
