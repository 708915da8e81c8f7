/* gvcnn_hip.h — C ABI of the MI355X-native GVCNN hot path (libgvcnn_hip.so).
 *
 * Drop-in boundary for the path BASELINE.json:north_star names: the per-view
 * backbone + grouping module of ace19-dev/gvcnn-tf.  The reference has no
 * FFI/plugin layer (it is Python on TensorFlow 1.x), so each entry point cites
 * the reference CALL SITE whose arithmetic it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes binding a maintainer would
 * add on the reference side.
 *
 * Conventions
 *  - every function returns 0 on success, a positive hipError_t value on a HIP
 *    failure, or a negative GV_E_* code; nothing throws;
 *  - every pointer is CALLER-OWNED DEVICE memory unless the name ends in
 *    `_host`; no hidden allocation, no hidden synchronisation;
 *  - `stream` is a hipStream_t passed as void*; launches are asynchronous and
 *    re-entrant across streams (safe to capture into a hipGraph);
 *  - activations are NHWC with an explicit pixel stride `ld` (in elements), so
 *    a tensor can be a channel slice of a wider (concat) buffer;
 *  - written for gfx950 only.
 */
#ifndef GVCNN_HIP_H
#define GVCNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GV_ABI_VERSION 1

/* error codes */
#define GV_OK 0
#define GV_E_BADARG (-1)      /* null pointer / non-positive size / inconsistent descriptor */
#define GV_E_UNSUPPORTED (-2) /* valid request the library does not implement (dtype, size cap) */
#define GV_E_ALIGN (-3)       /* pointer / stride not aligned as the vector path requires */
#define GV_E_PLAN (-4)        /* plan misuse (bad slot index, destroyed plan) */

/* element types (arithmetic type of the path; accumulation is always fp32) */
#define GV_F32 0
#define GV_BF16 1
#define GV_F16 2

/* gv_conv_desc.flags */
#define GV_CONV_RELU 1        /* ReLU after scale/shift(/residual)   */
#define GV_CONV_RELU2 2       /* ReLU on the second output           */
#define GV_CONV_SPLIT 4       /* y2 is not a second activation but the destination of output
                                 columns >= split_col (sibling convs fused into one GEMM) */
#define GV_CONV_X_F32 8       /* 16-bit dtype only: x is fp32 (the network input, nets/model.py:121) and is
                                 rounded to `dtype` by the loader — no separate cast pass over the images */
#define GV_CONV_X_P3 16       /* GV_F32 + GV_MATH_BF16X3 only: x holds every fp32 value as its three bf16 planes
                                 a = a0 + a1 + a2, laid out [pixel][channel/16][plane][16] (6 bytes per value; x_ld and
                                 the channel offset of a slice are multiples of 16 channels).  The producer split the
                                 value once; the LDS-DMA loader (csrc/conv_dma.hip) then only moves bytes */
#define GV_CONV_Y_P3 32       /* same dtype / math mode: y is written in that three-plane layout (y_ld, the slice offset
                                 and cout — with GV_CONV_SPLIT split_col — multiples of 16 channels); residual stays fp32 */
#define GV_CONV_Y2_P3 64      /* GV_CONV_SPLIT only: the second destination (columns >= split_col) is three-plane */
#define GV_CONV_MAXPOOL3S2 128 /* the convolution is followed by the reference's max_pool2d 3x3 / stride 2 / VALID
                                 (nets/inception_v3.py:113, Conv2d_2b_3x3 -> MaxPool_3a_3x3) and only the POOLED tensor is
                                 written: y is [nb, (oh-3)/2+1, (ow-3)/2+1, cout] with pixel stride y_ld; oh / ow stay the
                                 convolution's own output size.  Bit-identical to gv_conv2d_fwd + gv_pool2d.  Served for
                                 the halo-kernel class only (16-bit storage, 3x3 / stride 1, cin 32, cout 64, GV_CONV_RELU
                                 on every column, no residual / second output / BatchNorm sums, oh, ow >= 3):
                                 GV_E_UNSUPPORTED otherwise, and the caller issues the two launches.  Also served for the
                                 strip kernel of the 3-channel stems (GV_CONV_X_F32, 3x3 or 7x7 / stride 2, cout 64, any
                                 activation), and on GV_F32 storage under GV_MATH_BF16X3 for the same halo class (fp32
                                 input and output) on the maps where the kernel's 30-pixel strip form wastes fewer columns
                                 than its 16-pixel one: ceil(ow/16)*80 > ceil(ow/30)*128 — ow 17..30, 49..60, 65..90,
                                 97..120, and every ow >= 129 (csrc/conv_bf16s.hip, bf16s_halo_pool_ok) */
#define GV_CONV_MAXPOOL3S2_SAME 256 /* the same with TF's SAME padding on an even map (pads (0, 1): the last window is
                                 clipped; resnet_v2.py:181, conv1 -> pool1): y is [nb, oh/2, ow/2, cout].  Stem strip
                                 kernel only; odd oh / ow: GV_E_UNSUPPORTED */

#define GV_CONV_POOL_ACT2 512  /* with GV_CONV_MAXPOOL3S2[_SAME], y2 == NULL: the POOLED tensor is stored as
                                 act2(pool * scale2[c] + shift2[c]) (GV_CONV_RELU2: ReLU), computed from the pooled value as it
                                 would have been stored — ResNet-v2's first `preact` batch_norm + ReLU (nets/resnet_v2.py:75),
                                 whose only input is pool1 (:181): bit-identical to the fused launch + gv_scale_shift_act.  16-bit
                                 storage, the 3-channel stem kernel's class; anything else GV_E_UNSUPPORTED */

/* gv_conv_desc.math_mode: how an fp32 convolution is evaluated on the matrix cores */
#define GV_MATH_F32 0         /* v_mfma_f32_32x32x2_f32: exact fp32 fmaf chain                         */
#define GV_MATH_BF16X3 1      /* operands split into 3 bf16 planes, 6 bf16 MFMAs per product block:
                                 fp32-level accuracy (dropped terms <= 2^-24 relative), ~2.7x the rate */
#define GV_MATH_BF16X2 2      /* 2 planes, 3 MFMAs: ~2^-16 relative                                     */
#define GV_MATH_BF16X1 3      /* plain bf16 products, fp32 accumulate                                   */

/* pooling modes */
#define GV_POOL_MAX 0         /* padding value -inf (slim.max_pool2d) */
#define GV_POOL_AVG 1         /* divisor = number of VALID taps (slim.avg_pool2d, SAME) */
#define GV_POOL_BWD_STORE 0x100 /* gv_pool2d_bwd and gv_pool2d_bwd_argmax, OR-ed into mode, every dtype: dx = ... instead of
                                   dx += ... */
#define GV_POOL_X_P3 0x200    /* OR-ed into mode, GV_F32 only: x is in the three-plane layout of GV_CONV_Y_P3 (x_ld and the
                                 slice offset multiples of 16 channels, c a multiple of 4) */
#define GV_POOL_Y_P3 0x400    /* OR-ed into mode, GV_F32 only: y is written in that layout */
#define GV_POOL_AVG_RELU 2    /* GV_POOL_AVG followed by ReLU.  avg_pool -> 1x1 conv -> BN -> ReLU
                                 (nets/inception_v3.py:152-154,...) is evaluated as relu(avgpool(BN(conv1x1(x)))):
                                 the 1x1 conv and the BN affine commute with the average (its weights sum to 1),
                                 so the pool runs on cout instead of cin channels and the 1x1 joins the block's
                                 other 1x1 convs in one GEMM */

/* view-pooling modes */
#define GV_VIEWPOOL_MAX 0     /* tf.reduce_max  — nets/model.py:72   */
#define GV_VIEWPOOL_MEAN 1    /* tf.reduce_mean — unit_test.py:30    */

/* image order of a flattened view batch */
#define GV_ORDER_SHAPE_MAJOR 0 /* image b = n*V + v  (the [N,V,H,W,3] input as stored, model.py:121) */
#define GV_ORDER_VIEW_MAJOR 1  /* image b = v*N + n  (after the transpose of model.py:128)            */

/* ------------------------------------------------------------------------
 * Convolution descriptor (implicit GEMM: M = nb*oh*ow, N = cout, K = kh*kw*cin)
 * ---------------------------------------------------------------------- */
typedef struct gv_conv_desc {
    int32_t nb, ih, iw, cin;   /* input  [nb, ih, iw, cin], pixel stride x_ld */
    int32_t x_ld;
    int32_t kh, kw;            /* filter window */
    int32_t stride;            /* same in h and w (all call sites) */
    int32_t pad_t, pad_l;      /* zero padding before; after-padding is implied by oh/ow */
    int32_t oh, ow, cout;      /* output [nb, oh, ow, cout], pixel stride y_ld */
    int32_t y_ld;
    int32_t res_ld;            /* pixel stride of the residual input (ignored when residual == NULL) */
    int32_t y2_ld;             /* pixel stride of the optional second output */
    int32_t flags;             /* GV_CONV_* */
    int32_t dtype;             /* GV_F32 | GV_BF16 | GV_F16: type of x, w_packed, residual, y, y2 (16-bit types:
                                  fp32 accumulation and epilogue, one rounding on store; math_mode ignored) */
    int32_t split_col;         /* GV_CONV_SPLIT: columns [0,split_col) -> y, [split_col,cout) -> y2 at
                                  column (c - split_col), pixel stride y2_ld; same scale/shift/act */
    int32_t tile_cfg;          /* 0 = library heuristic; k >= 1 = tile configuration k-1 (a speed choice only: the same
                                  products, summed in the same order within a kernel family — bitwise the same result —
                                  and in another k order across families (register-staged, LDS-DMA chunk-major, the
                                  wave-specialised kernels): fp32-rounding-level differences, <= 6e-6 of the tensor's
                                  largest value in the tests) */
    int32_t math_mode;         /* GV_MATH_*; w_packed must have been packed for the same mode */
    int32_t in_dilation;       /* 0/1: plain convolution.  2: the input tensor is read as if zero-dilated by 2
                                  (only even tap positions exist, at index/2) — the data gradient of a stride-2
                                  convolution is a stride-1 convolution of the dilated dZ (GV_MATH_BF16X* only) */
    int32_t relu_cols;         /* 0: GV_CONV_RELU applies to every output column.  n > 0: only to columns < n — the
                                  trailing columns leave the GEMM as BN(conv) without ReLU (an Inception pooled branch
                                  computed as relu(avgpool(BN(conv1x1(x)))), see GV_POOL_AVG_RELU) */
    int32_t y_step;            /* 0: output pixel (n, oy, ox) is pixel (n*oh + oy)*ow + ox of y.  2: it is pixel
                                  (2*oy + y_py, 2*ox + y_px) of an image of y_ih x y_iw pixels — ONE PARITY CLASS of the
                                  data gradient of a stride-2 convolution (16-bit storage): dX at rows of parity y_py
                                  and columns of parity y_px only receives the taps r = (y_py + pad_t) mod 2, +2, ...
                                  (likewise s), so each class is a small stride-1 convolution over the UN-dilated dZ
                                  with those taps; four launches cover dX with 1/4 of the multiply-adds the zero-dilated
                                  form (in_dilation = 2) spends.  The residual, if any, is read at the same pixels. */
    int32_t y_py, y_px, y_ih, y_iw;
} gv_conv_desc;

typedef struct gv_pool_desc {
    int32_t nb, ih, iw, c;
    int32_t x_ld;
    int32_t kh, kw, stride;
    int32_t pad_t, pad_l;
    int32_t oh, ow;
    int32_t y_ld;
    int32_t mode;              /* GV_POOL_* */
    int32_t dtype;
} gv_pool_desc;

int gv_abi_version(void);
/* Human-readable text for a code returned by any function below. */
const char* gv_error_string(int code);

/* ---- filters ------------------------------------------------------------
 * Packed filter layout consumed by gv_conv2d_fwd, GV_MATH_F32: [cout][Kpad], k = (r*kw+s)*cin + c,
 * Kpad = K rounded up to 32, zero filled; GV_MATH_BF16X*: [cout][K/16][plane][16 bf16] (the filter is
 * split into its bf16 planes once, here); dtype GV_BF16 / GV_F16: [cout][Kpad] 16-bit.  Source is TensorFlow's HWIO
 * [kh,kw,cin,cout] fp32 variable (slim `.../weights`). */
int64_t gv_packed_filter_bytes(int32_t kh, int32_t kw, int32_t cin, int32_t cout, int32_t dtype,
                               int32_t math_mode);
int gv_pack_filter_hwio(const float* w_hwio, int32_t kh, int32_t kw, int32_t cin, int32_t cout,
                        void* w_packed, int32_t dtype, int32_t math_mode, void* stream);
/* Many filters in ONE launch (16-bit dtypes; the training step re-packs every filter after each update).
 * jobs (device array): source HWIO variable, destination, geometry; flipped = 1 packs the DATA-GRADIENT filter
 * W'[r',s',co,ci] = W[kh-1-r', kw-1-s', ci, co] (gv_packed_filter_bytes(kh,kw,cout,cin) bytes) straight from the
 * forward variable (the forward image of a fused filter needs no extra field: member rows are contiguous, `out`
 * points at the member's first row).  Job j owns blocks [first_block, first_block + ceil(rows*Kpad/256)); block_job (device int32
 * [num_blocks]) maps a block to its job. */
typedef struct gv_pack_job {
    const float* w;
    void* out;
    int32_t kh, kw, cin, cout;
    int32_t flipped;
    int32_t first_block;
    int32_t k_off, k_total;     /* flipped only, k_total > 0: this filter is columns [k_off, k_off + cout) of a FUSED
                                   filter of k_total output channels (several 1x1 convolutions of one input run as one
                                   GEMM; its data-gradient image has rows of kh*kw*k_total, padding zeroed by the caller) */
    int32_t w_ld;               /* row stride of `w` in elements (0 = cout): a member filter stored as a column slice of
                                   the fused [kh,kw,cin,k_total] variable block */
    int32_t sub_step;           /* flipped only; 0 / 1: every tap.  2: ONE PARITY CLASS of a stride-2 data gradient
                                   (gv_conv_desc.y_step): kh x kw are the class's tap counts and tap (u, v) of the packed
                                   image is W[sub_r0 + 2*(kh-1-u), sub_s0 + 2*(kw-1-v)] of the src_kw-wide variable */
    int32_t sub_r0, sub_s0, src_kw, reserved2;
} gv_pack_job;
int gv_pack_filters_batched(const gv_pack_job* jobs_dev, int32_t num_jobs, const int32_t* block_job_dev,
                            int32_t num_blocks, int32_t dtype, void* stream);

/* ---- convolution ---------------------------------------------------------
 * y  = act( conv(x, w) * scale[c] + shift[c] (+ residual) )
 * y2 = act2( (that pre-activation value) * scale2[c] + shift2[c] )       (optional)
 * or, with GV_CONV_SPLIT, y receives columns [0, split_col) and y2 columns [split_col, cout): the
 * 1x1 convs of one Inception block that read the same input (nets/inception_v3.py:140-146,...)
 * run as one GEMM over their concatenated filters and the input is read once.
 *
 * Replaces slim.conv2d (+ slim.batch_norm + ReLU, folded into scale/shift) at
 * nets/inception_v3.py:97-405 (94 call sites), nets/resnet_v2.py:79-89,
 * nets/resnet_utils.py:94-105 (explicit pad + VALID), and `shortcut + residual`
 * at nets/resnet_v2.py:91 (residual), and the next unit's `preact`
 * slim.batch_norm at nets/resnet_v2.py:75 (second output).
 * scale/shift: fp32 [cout] (BN fold: scale = gamma*rsqrt(var+eps), shift = beta - mean*scale;
 * bias-only conv: scale = 1, shift = bias).  residual/y2/scale2/shift2 may be NULL. */
int gv_conv2d_fwd(const gv_conv_desc* d, const void* x, const void* w_packed,
                  const float* scale, const float* shift, const void* residual,
                  void* y, void* y2, const float* scale2, const float* shift2, void* stream);
/* The same convolution over x' = relu(x * xscale[ci] + xshift[ci]) (xscale/xshift: fp32 [cin], BN fold as above),
 * x' computed by the kernel's loader in fp32 and rounded once to the storage type: the `preact` slim.batch_norm of a
 * ResNet-v2 unit (nets/resnet_v2.py:75) applied by the convolution that consumes it (conv1, nets/resnet_v2.py:83), so
 * that the unit before it writes `shortcut + residual` (nets/resnet_v2.py:91) once and no pre-activation tensor exists.
 * 16-bit storage (GV_BF16 / GV_F16), 1x1 window, no padding, cin a multiple of 8 and <= 2048, 16-byte aligned pixels;
 * tile_cfg 0 or one of the register-staged tiles {1, 2, 7, 8, 9}; or gv_conv2d_special_tile_cfg(-1) + 1: the streaming form
 * (csrc/conv_chain.hip, TAIL) for cin = 4 * cout, cout 64 / 128 / 256, BatchNorm + ReLU on every column, one destination, no
 * residual — the conv1 of a bottleneck identity unit — bit for bit the register-staged result; anything else:
 * GV_E_UNSUPPORTED. */
int gv_conv2d_fwd_xpre(const gv_conv_desc* d, const void* x, const float* xscale, const float* xshift,
                       const void* w_packed, const float* scale, const float* shift, const void* residual,
                       void* y, void* y2, const float* scale2, const float* shift2, void* stream);

/* ---- bottleneck chain ----------------------------------------------------
 * The TAIL of one ResNet-v2 bottleneck unit and the HEAD of the next as ONE launch (csrc/conv_chain.hip):
 *   y = conv1x1(x, w3) * scale3[c] + shift3[c] + shortcut          nets/resnet_v2.py:87-91 of unit u (d -> 4d channels,
 *                                                                  normalizer_fn=None: scale3 = 1, shift3 = biases)
 *   z = relu( conv1x1( relu(y * pre_scale + pre_shift), w1 ) * scale1 + shift1 )
 *                                                                  nets/resnet_v2.py:75 (`preact`) and :83-84 (conv1 +
 *                                                                  BatchNorm + ReLU) of unit u+1 (4d -> d channels)
 * for two consecutive units of one block, where the next unit's shortcut is the identity (resnet_v2.py:76-77) and conv1 is
 * the pre-activation's only reader.  y is written once and never read back by conv1; the pre-activation is applied to the
 * ROUNDED y, as gv_conv2d_fwd_xpre's loader does — the results are those of gv_conv2d_fwd (y) followed by
 * gv_conv2d_fwd_xpre (z), bit for bit.  x [m, d], shortcut / y [m, 4d], z [m, d] with pixel strides *_ld (multiples of 8
 * elements, 16-byte aligned bases); w3_packed [4d][d], w1_packed [d][4d] as gv_pack_filter_hwio writes them for the dtype.
 * 16-bit storage, d = 64 or 128 (the HBM-bound blocks 1 and 2 of ResNet-v2-50): anything else GV_E_UNSUPPORTED and the
 * caller issues the two launches.
 * GV_CHAIN_PROJ (flags; d = 64): the unit's depth CHANGES and its shortcut is the 1x1 projection of its pre-activation
 * (nets/resnet_v2.py:79-81) — x is [m, 2d] = [the unit's conv2 output | the unit's pre-activation], w3_packed the
 * K-concatenated [4d][2d] filter [conv3 ; shortcut] (gv_pack_filter_hwio of the two HWIO filters concatenated along cin),
 * shift3 = conv3's biases + the shortcut's, `shortcut` NULL:  y = (conv3(x2) + shortcut(x0)) * scale3 + shift3  is ONE fp32
 * accumulation with one rounding, and no shortcut tensor is written or read.  Against the separate launches (which round
 * the shortcut to the storage type first) y differs by at most that one rounding. */
#define GV_CHAIN_PROJ 4096
typedef struct gv_chain_desc {
    int32_t m;                 /* rows = nb * oh * ow (all three tensors share the pixel grid) */
    int32_t d;                 /* bottleneck depth */
    int32_t x_ld, res_ld, y_ld, z_ld;
    int32_t dtype;             /* GV_BF16 | GV_F16 */
    int32_t flags;             /* GV_CONV_RELU2: ReLU on z; GV_CHAIN_PROJ */
    int32_t tile_cfg;          /* 0 (reserved) */
} gv_chain_desc;
int gv_bottleneck_chain_fwd(const gv_chain_desc* d, const void* x, const void* w3_packed, const float* scale3,
                            const float* shift3, const void* shortcut, void* y, const float* pre_scale,
                            const float* pre_shift, const void* w1_packed, const float* scale1, const float* shift1,
                            void* z, void* stream);

/* The same launch with the unit's conv2 in front (csrc/conv_chain.hip, FRONT): x is the unit's conv1 output [nb, ih, iw, d] and
 *   c2 = relu( conv3x3(x, w2, stride 1, SAME) * scale2 + shift2 )        nets/resnet_v2.py:85-86 (conv2 + BatchNorm + ReLU)
 * feeds gv_bottleneck_chain_fwd's y / z without ever being stored: one launch per bottleneck unit (from its conv2 to the
 * next unit's conv1), reading [m, d] + [m, 4d] and writing [m, 4d] + [m, d].  w2_packed [d][9*d] as gv_pack_filter_hwio
 * writes a 3x3 filter for the dtype.  conv2's k order here is tap-major; against the separate launches the results agree to
 * fp32 summation order (the other kernel families of gv_conv2d_fwd sum k chunk-major), everything behind c2's rounding is
 * the chain's arithmetic.  Same classes: 16-bit storage, d = 64 or 128, stride 1; else GV_E_UNSUPPORTED. */
typedef struct gv_unit_desc {
    int32_t nb, ih, iw;        /* the pixel grid of all four tensors */
    int32_t d;                 /* bottleneck depth */
    int32_t x_ld, res_ld, y_ld, z_ld;
    int32_t dtype;             /* GV_BF16 | GV_F16 */
    int32_t flags;             /* GV_CONV_RELU2: ReLU on z */
    int32_t tile_cfg;          /* 0 (reserved) */
} gv_unit_desc;
int gv_bottleneck_unit_fwd(const gv_unit_desc* d, const void* x, const void* w2_packed, const float* scale2,
                           const float* shift2, const void* w3_packed, const float* scale3, const float* shift3,
                           const void* shortcut, void* y, const float* pre_scale, const float* pre_shift,
                           const void* w1_packed, const float* scale1, const float* shift1, void* z, void* stream);

/* ---- pooling -------------------------------------------------------------
 * slim.max_pool2d / slim.avg_pool2d: nets/inception_v3.py:112,127,152,219,355,...;
 * nets/resnet_v2.py:181 (3x3/2 SAME, pad (0,1)); nets/resnet_utils.py:64-67
 * (`subsample` = 1x1 max-pool with stride). */
int gv_pool2d_fwd(const gv_pool_desc* d, const void* x, void* y, void* stream);

/* y[p,c] = act(x[p,c]*scale[c] + shift[c]) over npix pixels — slim.batch_norm (+ReLU)
 * used stand-alone: the `preact` of the first unit, nets/resnet_v2.py:75. */
int gv_scale_shift_act(const void* x, int64_t npix, int32_t c, int32_t x_ld, const float* scale,
                       const float* shift, int32_t relu, void* y, int32_t y_ld, int32_t dtype,
                       void* stream);

/* Global average pool over h*w: x [nb, hw, c] (pixel stride x_ld) -> y fp32 [nb, c].
 * tf.keras.layers.GlobalAveragePooling2D at nets/model.py:144,163. */
int gv_global_avg_pool(const void* x, int32_t nb, int32_t hw, int32_t c, int32_t x_ld, float* y,
                       int32_t dtype, void* stream);

/* ---- grouping module ------------------------------------------------------
 * Scorer, nets/model.py:144-145: r_img[b] = GAP(raw[b]) . kernel[v(b)] + bias[v(b)],
 * one Dense(1) per view.  raw [nb, hw, cr] (pixel stride raw_ld), kernel fp32 [V, cr],
 * bias fp32 [V]; v(b) from `order` (GV_ORDER_*), nb = N*V.  r_img fp32 [nb]. */
int gv_view_score_partial(const void* raw, int32_t nb, int32_t hw, int32_t cr, int32_t raw_ld,
                          const float* kernel, const float* bias, int32_t num_views,
                          int32_t order, float* r_img, int32_t dtype, void* stream);

/* nets/model.py:146-147: score[v] = sigmoid(log(|mean_n r_img[b(n,v)]|)), fixed summation
 * order (n ascending) so every rank of a multi-GPU job gets identical scores. */
int gv_view_score_finalize(const float* r_img, int32_t num_shapes, int32_t num_views,
                           int32_t order, float* scores, void* stream);

/* nets/model.py:16-41 (`group_scheme` + `group_weight`) on device:
 * gidx[v] = (int)(scores[v] * (float)num_bins)  — fp32 product, truncation (model.py:23 uses 10);
 * scheme [G,V] one-hot int32; weight[g] = 1 + #views in g (fp32).
 * status (device int32): 0 ok; 1 some gidx >= G or < 0 (the reference raises IndexError
 * there); 2 a score is NaN.  Outputs for in-range views are still written. */
int gv_group_assign(const float* scores, int32_t num_views, int32_t num_groups, int32_t num_bins,
                    int32_t* gidx, int32_t* scheme, float* weight, int32_t* status, void* stream);

/* nets/model.py:28-41 (`group_weight`) alone, for an arbitrary 0/1 scheme fed by the caller:
 * weight[g] = 1 + #{v : scheme[g,v] == 1}. */
int gv_group_weight(const int32_t* scheme, int32_t num_groups, int32_t num_views, float* weight,
                    void* stream);

/* nets/model.py:44-102 (`view_pooling` + `group_fusion`) fused, one pass over the views:
 *   D[g] = pool_{v: scheme[g,v] != 0} F[v]      (empty group -> `empty_fill`: 1 in model.py:63)
 *   S    = sum_g weight[g]*D[g] / sum_g weight[g]
 * F element (v, n, e) at F + v*view_stride + n*shape_stride + e, e < E = h*w*C.
 * D (nullable) [G, N, E], S (nullable) [N, E].  scheme int32 [G,V] and weight fp32 [G] are
 * device arrays (they never visit the host on the fused path). V <= 64, G <= 64. */
int gv_view_pool_fuse_fwd(const void* F, int32_t num_views, int32_t num_shapes, int64_t E,
                          int64_t view_stride, int64_t shape_stride, const int32_t* scheme,
                          int32_t num_groups, const float* weight, int32_t mode, float empty_fill,
                          void* D, void* S, int32_t dtype, void* stream);

/* ---- per-shape grouping (the paper's grouping module; NOT what nets/model.py computes) -------
 * nets/model.py:146 averages the scorer response over the batch, so one scheme serves all N shapes.  The
 * per-shape form scores, bins and fuses every shape on its own: nothing couples the shapes of a batch, hence a
 * shape-sharded multi-GPU job needs no exchange at all. */
#define GV_WEIGHT_COUNT 0       /* weight[g] = 1 + #members                      (nets/model.py:28-41)          */
#define GV_WEIGHT_MEAN_SCORE 1  /* weight[g] = mean score of the members, 0 for an empty group (score-derived,
                                   as in the paper's figure assets/grouping module.png)                          */
/* scores[b] = sigmoid(log(|r_img[b]|)) for every image b (no batch mean). */
int gv_view_score_per_shape(const float* r_img, int32_t nb, float* scores, void* stream);
/* scores [N,V] (image b = n*V + v) -> gidx [N,V], scheme [N,G,V] one-hot int32, weight [N,G]; binning exactly as
 * gv_group_assign; status is OR-ed over the shapes. */
int gv_group_assign_per_shape(const float* scores, int32_t num_shapes, int32_t num_views, int32_t num_groups,
                              int32_t num_bins, int32_t weight_mode, int32_t* gidx, int32_t* scheme,
                              float* weight, int32_t* status, void* stream);
/* gv_view_pool_fuse_fwd with one scheme [G,V] and one weight [G] PER SHAPE (scheme [N,G,V], weight [N,G]).
 * A shape whose weights sum to 0 gets S = 0. */
int gv_view_pool_fuse_fwd_per_shape(const void* F, int32_t num_views, int32_t num_shapes, int64_t E,
                                    int64_t view_stride, int64_t shape_stride, const int32_t* scheme,
                                    int32_t num_groups, const float* weight, int32_t mode, float empty_fill,
                                    void* D, void* S, int32_t dtype, void* stream);

/* tf.keras.layers.Dense at nets/model.py:164: y[n,:] = x[n,:] @ kernel[F,C] + bias (fp32). */
int gv_dense_fwd(const float* x, int32_t n, int32_t f, const float* kernel, const float* bias,
                 int32_t c, float* y, void* stream);

/* ---- explain a prediction: per-view, per-pixel attribution of one logit ------------------------------------------
 * The head above the final tap (view pooling, group fusion, global average pool, Dense) is piecewise linear in the view
 * descriptors F.  With the grouping held constant (as in gv_view_pool_fuse_bwd) the logit of class k = target[n] is
 *   logit[n,k] = baseline[n] + sum_{v,p} maps[n,v,p]                                         (kind GV_EXPLAIN_EXACT)
 *   dlogit/dF[n,v,p,c] = K[c,k]/hw * sum_{g contains v} w_g/W * share_g(v,p,c)
 *   share_g = [F[v] attains the maximum of g] / #members attaining it (max pooling), 1/|g| (mean pooling)
 *   maps[n,v,p]     = sum_c F * dlogit/dF            view_contrib[n,v] = sum_p maps[n,v,p]
 *   baseline[n]     = b[k] + sum_{g empty} w_g/W * empty_fill * sum_c K[c,k]
 * GV_EXPLAIN_GRADCAM: alpha[n,v,c] = 1/hw sum_p dlogit/dF, maps[n,v,p] = max(0, sum_c alpha * F); view_contrib and
 * baseline as above.  A shape whose weights sum to 0 has maps = view_contrib = 0 and baseline = b[k].
 * F element (n, v, p, c) at F + n*shape_stride + v*view_stride + p*C + c, in `dtype`; everything else is fp32.
 * scheme [G,V] / weight [G], or [N,G,V] / [N,G] with per_shape != 0.  cls_kernel [C, num_classes] row-major, cls_bias
 * [num_classes].  targets int64 [N], or NULL: the first maximum of logits [N, num_classes] (one of the two must be given).
 * Outputs: maps [N,V,hw], view_contrib [N,V], baseline [N], target_out int64 [N] (the class used; -1 for a target
 * outside [0, num_classes): bit 0 of *status is set and that shape's outputs are 0).  No atomics: two calls give the same
 * bits.  exact reads F once, gradcam twice.  V, G <= 64, N <= 65535 (else GV_E_UNSUPPORTED).
 * workspace (GV_EXPLAIN_GRADCAM only, gv_explain_workspace_bytes): alpha [N,V,C] fp32 first, then the per-chunk shares
 * of view_contrib that the first sweep leaves for its fixed-order finish. */
#define GV_EXPLAIN_EXACT 0
#define GV_EXPLAIN_GRADCAM 1
int64_t gv_explain_workspace_bytes(int32_t num_views, int32_t num_shapes, int32_t C, int32_t kind);
int gv_explain_views(const void* F, int32_t num_views, int32_t num_shapes, int32_t hw, int32_t C, int64_t view_stride,
                     int64_t shape_stride, const int32_t* scheme, int32_t num_groups, const float* weight,
                     int32_t per_shape, int32_t pool_mode, float empty_fill, const float* cls_kernel,
                     const float* cls_bias, int32_t num_classes, const float* logits, const int64_t* targets,
                     int32_t kind, float* maps, float* view_contrib, float* baseline, int64_t* target_out,
                     int32_t* status, void* workspace, int32_t dtype, void* stream);

/* ---- input preprocessing (train_data.py:63,81-84,101; eval_data.py:72,109) -----------------------
 * One launch turns a batch of decoded 8-bit RGB views [nimg, h0, w0, 3] into the network input [nimg, H, W, 3] fp32:
 *   tf.image.resize (TF1 resize_images: bilinear, align_corners=False, src = dst * in/out — no half-pixel shift),
 *   random_flip_left_right / random_flip_up_down (bit 0 / bit 1 of flip[img]; NULL = none),
 *   random_brightness (delta[img] added on the 0..255 scale; NULL = none),
 *   x * (1/255) - 0.5.
 * The random decisions are made by the caller (host RNG), the arithmetic happens here. */
int gv_preprocess_views(const uint8_t* src, int32_t nimg, int32_t h0, int32_t w0, int32_t height, int32_t width,
                        const int32_t* flip, const float* delta, float* dst, void* stream);

/* PNG row un-filtering on the HOST (the sequential half of tf.image.decode_png, train_data.py:55 / eval_data.py:64,
 * after zlib inflate): raw = h rows of (filter byte + rowbytes bytes), out = h x rowbytes; filter types 0-4 of the PNG
 * specification, bpp bytes per pixel.  Both pointers are host memory; no stream. */
int gv_png_unfilter(const uint8_t* raw, int32_t h, int32_t rowbytes, int32_t bpp, uint8_t* out);

/* ---- PNG decode of a whole batch (the other half of tf.image.decode_png(channels=3): zlib inflate, un-filter, expand) --
 * Input: the zlib stream of every image (its IDAT bodies concatenated by the caller, who walks the chunks) in ONE byte
 * buffer, plus one gv_png_image per image.  8-bit, non-interlaced images that all share one size h0 x w0.
 * Output: out [n, h0, w0, 3] uint8 (gray replicated to three channels, alpha dropped, palette indices looked up) and
 * status [n] int32, one GV_PNG_* value per image.  An image whose status is not GV_PNG_OK leaves its own slot of `out`
 * unspecified and touches nothing else; the other images of the batch are decoded.  Every byte is exact (there is no
 * tolerance): the stream is checked like zlib checks it (block types, stored lengths, over-subscribed and incomplete
 * code sets, distances, the Adler-32 trailer; FDICT is rejected, any window size CINFO <= 7 accepted).
 *
 * Layout rules (GV_E_BADARG otherwise, checked before any launch): every stream starts at a multiple of 16 bytes,
 * ends at or before stream_bytes - 16 (the buffer closes with 16 bytes of padding so that wide loads stay inside it);
 * colour type 0, 2, 3, 4 or 6; a palette image has 1..256 entries; n > 0, h0, w0 > 0, no NULL pointer (palettes may
 * be NULL when no image has colour type 3).  GV_E_UNSUPPORTED: h0 * (1 + 4 * w0) does not fit 31 bits.
 *
 * gv_png_decode_batch: streams, palettes, out, status and ws are DEVICE memory; `images` is HOST memory, checked
 * during the call and copied into the workspace by an asynchronous copy on `stream` (keep it unchanged until the stream
 * has passed the call).  ws: gv_png_decode_workspace_bytes(n, h0 * (1 + 4 * w0)) bytes, 16-byte aligned — the
 * inflated rows of every image, whose already written part is also the DEFLATE window.
 * gv_png_decode_host: the same decoder run serially on the host, every pointer host memory, no workspace. */
#define GV_PNG_OK 0
#define GV_PNG_TRUNCATED 1          /* the stream ends inside a block or inside the trailer */
#define GV_PNG_BAD_HEADER 2         /* zlib header: method, window size, check bits, or a preset dictionary (FDICT) */
#define GV_PNG_BAD_BLOCK 3          /* block type 3, or a stored block whose LEN and NLEN do not match */
#define GV_PNG_BAD_CODES 4          /* over-subscribed / incomplete code set, bad repeat, unused or reserved symbol */
#define GV_PNG_BAD_DISTANCE 5       /* a match reaches back past the first byte of the output */
#define GV_PNG_TOO_LONG 6           /* the stream holds more than h0 * (1 + w0 * channels) bytes */
#define GV_PNG_TOO_SHORT 7          /* ... fewer */
#define GV_PNG_BAD_CHECKSUM 8       /* Adler-32 trailer */
#define GV_PNG_BAD_FILTER 9         /* a row's filter byte is above 4 */
#define GV_PNG_BAD_PALETTE_INDEX 10 /* a pixel's index is past the end of the image's palette */
typedef struct gv_png_image {
    int64_t offset;          /* of the zlib stream in `streams`, bytes, a multiple of 16 */
    int32_t length;          /* of the zlib stream, bytes */
    int32_t color_type;      /* IHDR colour type: 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA */
    int32_t palette_offset;  /* colour type 3: of the image's PLTE body (RGB triples) in `palettes`, bytes */
    int32_t palette_len;     /* colour type 3: entries of that palette, 1..256 */
} gv_png_image;
/* negative: an error code (n <= 0, max_raw_bytes <= 0: GV_E_BADARG) */
int64_t gv_png_decode_workspace_bytes(int32_t n, int64_t max_raw_bytes);
int gv_png_decode_batch(const uint8_t* streams, int64_t stream_bytes, const gv_png_image* images, int32_t n,
                        int32_t h0, int32_t w0, const uint8_t* palettes, uint8_t* out, int32_t* status, void* ws,
                        int64_t ws_bytes, void* stream);
int gv_png_decode_host(const uint8_t* streams, int64_t stream_bytes, const gv_png_image* images, int32_t n,
                       int32_t h0, int32_t w0, const uint8_t* palettes, uint8_t* out, int32_t* status);

/* ---- PNG encode of a whole batch (the mirror of the decoder: colour type, line filter, DEFLATE) ------------------------
 * Input: src [n, h0, w0, 3] uint8.  Output: the zlib stream (what one IDAT chunk holds) of image i in
 * out[i * out_stride, i * out_stride + length[i]), and color_type[i]: 0 (gray, one byte per pixel) or 2 (RGB).  The
 * caller frames the chunks (signature, IHDR, IDAT, IEND, CRC-32).  Bytes of a slot past length[i] are not written.
 *  - color: GV_PNG_COLOR_AUTO stores an image whose every pixel has R = G = B as colour type 0, GV_PNG_COLOR_RGB never.
 *  - filter: 0-4 forces that PNG filter type on every row; GV_PNG_FILTER_ADAPTIVE takes per row the type with the smallest
 *    sum of |signed residual| (a residual byte v counts v below 128, 256 - v otherwise), the lowest type on a tie; the
 *    candidates are computed from the unfiltered neighbours.
 *  - stream: 78 01, then the raw stream (h0 rows of filter byte + w0 * channels bytes) in SEGMENTS of
 *    gv_png_encode_segment_bytes() bytes, each encoded on its own — run matches at distance 1 and at the pixel stride,
 *    lengths 3-258; stored, fixed or dynamic Huffman block, whichever is shortest (ties: stored, fixed, dynamic) — and
 *    every segment but the last followed by an empty non-final stored block; then the Adler-32.  The bytes are the same
 *    on every run and the same from both entry points.
 * gv_png_encode_bound: the most bytes the stream of an h0 x w0 image can take, a multiple of 16.  out_stride must be at
 * least that and a multiple of 16.
 * GV_E_BADARG: NULL pointer, n / h0 / w0 <= 0, unknown filter or colour constant, out_stride too small or not a multiple
 * of 16, workspace too small.  GV_E_ALIGN: ws not 16-byte aligned.  GV_E_UNSUPPORTED: h0 * (1 + 3 * w0) does not fit 31
 * bits (or the batch has more than 2^31 - 1 segments).  Arguments are checked before any HIP call.
 * gv_png_encode_batch: src, out, length, color_type and ws are DEVICE memory; ws: gv_png_encode_workspace_bytes(n, h0,
 * w0) bytes, 16-byte aligned (the filtered rows, the segments' outputs and their lengths / Adler sums).  No global
 * atomics.  gv_png_encode_host: the same encoder run serially on host memory, no workspace. */
#define GV_PNG_FILTER_ADAPTIVE 5
#define GV_PNG_COLOR_AUTO 0
#define GV_PNG_COLOR_RGB 1
int64_t gv_png_encode_segment_bytes(void);
/* negative: an error code (h0, w0 <= 0: GV_E_BADARG; 31 bits exceeded: GV_E_UNSUPPORTED) */
int64_t gv_png_encode_bound(int32_t h0, int32_t w0);
int64_t gv_png_encode_workspace_bytes(int32_t n, int32_t h0, int32_t w0);
int gv_png_encode_batch(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t filter, int32_t color,
                        uint8_t* out, int64_t out_stride, int32_t* length, int32_t* color_type, void* ws,
                        int64_t ws_bytes, void* stream);
int gv_png_encode_host(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t filter, int32_t color,
                       uint8_t* out, int64_t out_stride, int32_t* length, int32_t* color_type);

/* ---- evaluation metrics (eval.py:94-99) ---------------------------------------------------------
 * prediction[n] = argmax_c logits[n,c] (first maximum, like tf.argmax); confusion[label, prediction] += 1
 * (tf.math.confusion_matrix, int32 [C,C], ACCUMULATED so a whole evaluation run needs one buffer);
 * *correct += #{n : prediction[n] == labels[n]}.  labels int64 [N]; a label outside [0,C) is counted in neither. */
int gv_eval_metrics(const float* logits, const int64_t* labels, int32_t n, int32_t c, int64_t* prediction,
                    int32_t* confusion, int32_t* correct, void* stream);

/* ---- shape retrieval on the shape descriptor (the fp32 GAP vector [N, C] of nets/model.py:163) ---------------------
 * An index is n descriptors prepared by gv_retr_prepare into `dtype` storage [n, ld] plus their squared norms.
 * Ranking order of every function: the 64-bit key (distance, row id) — ascending distance, equal distances by the lower
 * id.  The distance of a pair does not depend on where it sits in a tile or a chunk: db_chunk changes speed only, and
 * the results are bitwise identical for every valid chunk size.
 * Argument errors: GV_E_BADARG for a NULL required pointer, a size <= 0, ld < d, k outside [1, GV_KNN_MAX_K], an
 * unknown metric, a workspace smaller than the *_workspace_bytes answer, a db_chunk that is not a positive multiple of
 * 256; GV_E_UNSUPPORTED for an unknown dtype or an AP database above GV_RETR_AP_MAX_NDB rows; GV_E_ALIGN for
 * ld % 64 != 0 or a storage / workspace pointer that is not 16-byte aligned.  All checked before any HIP call. */
#define GV_METRIC_L2 0        /* squared Euclidean distance, clamped at 0 */
#define GV_METRIC_COSINE 1    /* 1 - cosine similarity (rows normalised by gv_retr_prepare) */
#define GV_KNN_MAX_K 256
#define GV_RETR_AP_MAX_NDB 16384
/* x [n, d] fp32 (row stride x_ld) -> y [n, ld] in `dtype` (columns d..ld-1 zero; GV_METRIC_COSINE: each row scaled to
 * unit L2 norm first, a zero row stays zero) and sqnorm [n] = |y row|^2 of the values as stored (after rounding). */
int gv_retr_prepare(const float* x, int32_t n, int32_t d, int32_t x_ld, int32_t metric, int32_t dtype,
                    void* y, int32_t ld, float* sqnorm, void* stream);
/* Workspace of gv_knn_search: a [nq, db_chunk] fp32 distance tile and the running k best of every query. */
int64_t gv_knn_workspace_bytes(int32_t nq, int32_t db_chunk, int32_t k);
/* k nearest database rows of every query (both prepared with the same metric / dtype / ld): dist [nq, k] fp32 and
 * idx [nq, k] int64, ascending by (distance, id); a query with fewer than k candidates is padded with id -1 / +inf.
 * exclude [nq] (NULL: none): a value in [0, ndb) drops that row from the query's ranking (leave-self-out). */
int gv_knn_search(const void* q, const float* q_sqnorm, int32_t nq, const void* db, const float* db_sqnorm,
                  int32_t ndb, int32_t d, int32_t ld, int32_t metric, int32_t dtype, int32_t k,
                  const int64_t* exclude, int32_t db_chunk, float* dist, int64_t* idx,
                  void* workspace, int64_t workspace_bytes, void* stream);
/* Workspace of gv_retr_average_precision (GV_E_UNSUPPORTED above GV_RETR_AP_MAX_NDB). */
int64_t gv_retr_ap_workspace_bytes(int32_t nq, int32_t ndb);
/* ap [nq] fp32: average precision of each query over the FULL ranking of the database (same order, same exclusion),
 * AP = (1/R) sum_{j=1..R} j / rank_j with R relevant rows (db_labels == q_labels), accumulated in fp64.  A query with a
 * label < 0, or with no relevant row left after exclusion, gets NaN; a database row with a label < 0 is ranked but never
 * relevant.  ndb <= GV_RETR_AP_MAX_NDB (a whole-row sort in LDS). */
int gv_retr_average_precision(const void* q, const float* q_sqnorm, const int64_t* q_labels, int32_t nq,
                              const void* db, const float* db_sqnorm, const int64_t* db_labels, int32_t ndb,
                              int32_t d, int32_t ld, int32_t metric, int32_t dtype, const int64_t* exclude,
                              float* ap, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- learned retrieval metric: low-rank Mahalanobis projection (the paper's second retrieval number) ---------------
 * W [r, d] fp32 and a scalar threshold b, z_i = W x_i.  Over the pairs i < j of a batch whose labels are both >= 0 (P
 * pairs), y = +1 for equal labels and -1 otherwise, c = pos_weight for y = +1 and 1 otherwise,
 * d_ij = max(0, |z_i|^2 + |z_j|^2 - 2 z_i.z_j):
 *     L = (1/P) sum c_ij max(0, 1 - y_ij (b - d_ij));   a pair is ACTIVE when 1 - y_ij (b - d_ij) > 0 (strictly);
 *     a_ij = c_ij y_ij [active];   dL/dz_i = (2/P) ((sum_j a_ij) z_i - sum_j a_ij z_j);   dL/db = -(1/P) sum_{i<j} a_ij.
 * All storage is fp32 and every product runs on the exact fp32 MFMA; every reduction has a fixed order (no
 * floating-point atomics): the same inputs give the same bits every run.  rl = r rounded up to 64.
 * Argument errors: GV_E_BADARG for a NULL required pointer, a size <= 0, a row stride below its row length, an rl
 * that is not r rounded up to 64, a workspace smaller than the *_workspace_bytes answer; GV_E_UNSUPPORTED for
 * r > GV_METRIC_MAX_RANK or n > GV_METRIC_MAX_BATCH (pair / wgrad); GV_E_ALIGN for a row stride that is not a multiple
 * of 4 or a pointer that is not 16-byte aligned.  All checked before any HIP call. */
#define GV_METRIC_MAX_RANK 256
#define GV_METRIC_MAX_BATCH 16384
/* z [n, rl] = x [n, d] (row stride x_ld) W^T (w [r, d], row stride w_ld), columns r..rl-1 written as zero, and
 * sqnorm [n] = |z row|^2 summed from the stored values.  Any n > 0. */
int gv_metric_project(const float* x, int32_t n, int32_t d, int32_t x_ld, const float* w, int32_t r, int32_t w_ld,
                      float* z, int32_t rl, float* sqnorm, void* stream);
/* Workspace of gv_metric_pair_grad: per-slice partial row sums and per-workgroup statistics, linear in n. */
int64_t gv_metric_pair_workspace_bytes(int32_t n, int32_t r);
/* One pass over all pairs of the batch, nothing n x n leaves the compute unit.  z / sqnorm as gv_metric_project wrote
 * them, labels int64 [n] (a label < 0 takes part in no pair), b a DEVICE scalar.  Writes
 * dz_unnorm [n, rl] = 2 ((sum_j a_ij) z_i - sum_j a_ij z_j)  (not divided by P; pad columns zero) and
 * stats fp64 [5] = {sum_{i<j} c h, P, active pairs, sum_{i<j} a_ij, sum_{i<j} d_ij}: the per-pair fp32 values are
 * summed in fp64, the counts in integers. */
int gv_metric_pair_grad(const float* z, const float* sqnorm, const int64_t* labels, int32_t n, int32_t r, int32_t rl,
                        const float* b, float pos_weight, float* dz_unnorm, double* stats, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* Workspace of gv_metric_wgrad: one image of the gradient per slice of the batch axis. */
int64_t gv_metric_wgrad_workspace_bytes(int32_t n, int32_t d, int32_t r);
/* grad [r * ld + 1]: dL/dW [r, ld] = (dz_unnorm^T x) / P (columns d..ld-1 zero), then dL/db = -(sum a) / P as the last
 * element; P and sum a are read from stats ON THE DEVICE (P = 0: all zeros).  The batch axis is split over workgroups
 * and the slices are added in index order.  loss (NULL: not wanted): a device scalar that receives stats[0] / P
 * (P = 0: 0). */
int gv_metric_wgrad(const float* dz_unnorm, int32_t n, int32_t r, int32_t rl, const float* x, int32_t d, int32_t x_ld,
                    const double* stats, float* grad, int32_t ld, float* loss, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ---- meshes in: multi-view rasteriser (replaces the reference's offline off2obj -> obj2png -> TFRecord chain) -------
 * Turns N triangle meshes into the backbone's input views [N, V, H, W, 3].  Results are defined bit for bit (every
 * fp32 step below is rounded on its own; the kernels are compiled with FMA contraction off):
 *  - meshes: fp32 vertices [sum nv, 3] and int32 triangles [sum nt, 3] of LOCAL vertex indices, concatenated; int64
 *    vert_offsets / tri_offsets [N+1] (offsets[0] need not be 0: mesh m is rows offsets[m]-offsets[0] ..
 *    offsets[m+1]-offsets[0] of the arrays passed, so a group of meshes is a pointer into the offsets).  The triangle
 *    index within its mesh is its id.  A triangle with an index outside [0, nv) is dropped.
 *  - normalisation, per mesh, fp32, every step rounded (no FMA): c = (min + max) * 0.5 per axis,
 *    r = sqrt(max_i ((dx*dx + dy*dy) + dz*dz)) with d = v - c, u = (v - c) * (fit / r).  Status GV_RENDER_*.
 *  - rotation (rotations [N,3,3] row-major, NULL = identity): w = M u, w_i = (M_i0*u0 + M_i1*u1) + M_i2*u2.  M must
 *    be a rotation (orthonormal, det +1; the Python layer checks this); any other M gives unspecified pictures (memory
 *    stays in bounds).
 *  - cameras [V,3,3] (rows: right, up, forward = from the eye to the origin), computed on the host in float64 from
 *    matplotlib's view_init(elev, azim) with +z up and rounded to fp32: q = C_v w (same sum order).
 *  - projection: orthographic: sx = W/2 + q0*k, sy = H/2 - q1*k, t = (q2 + 1) * 0.5 with k = proj_scale (min(H,W)/2);
 *    GV_RENDER_PERSPECTIVE: z = q2 + D, sx = W/2 + (q0*k)/z, sy = H/2 - (q1*k)/z, t = a - b/z with D = persp_dist
 *    = 1/sin(fov/2), k = min(H,W)/2 / tan(fov/2), a = depth_a = (D+1)/2, b = depth_b = (D*D-1)/2 (all computed on the
 *    host in float64, rounded to fp32).  X = rint(clamp(sx*256, +-2^18)) (round to nearest even), Y likewise; pixel
 *    (i, j) has its centre at (256 i + 128, 256 j + 128); row 0 is the top row.  Z = rint(clamp(t, 0, 1) * (2^24-1)).
 *  - coverage, int64 on the snapped coordinates: a zero-area triangle is dropped, a negative one is re-oriented
 *    (vertices 1 and 2 swapped).  E_ab(P) = (Xb-Xa)*(Py-Ya) - (Yb-Ya)*(Px-Xa); weights e0 = E_12, e1 = E_20, e2 = E_01.
 *    Covered: every e > 0, or e == 0 on an edge a -> b that owns its centres.  Top-left rule: positive area in this
 *    y-down frame is clockwise on screen, so top edges (dy == 0, dx > 0) and left edges (dy < 0) own: a square with
 *    corners on centres covers its top row and left column, not its bottom row and right column, and two triangles on
 *    either side of a shared edge never both cover a centre.  Depth Z = (e0*Z0 + e1*Z1 + e2*Z2) div (e0 + e1 + e2),
 *    unsigned 64-bit; the clamp keeps the numerator below 2^62.  The pixel keeps the smallest key (Z << 32) | id: equal depths go to the lower id.
 *  - shading, per triangle from its winding: n = (w1-w0) x (w2-w0), s = (n.l) / sqrt(n.n) (0 when n.n == 0),
 *    f = ambient + (1-ambient) * h with h = (s+1)*0.5, or |s| with GV_RENDER_TWO_SIDED; colour = color * f, and
 *    background where nothing covers the pixel.
 *  - output: GV_RENDER_OUT_U8 u8 = clamp(floor(c*255 + 0.5), 0, 255); GV_RENDER_OUT_F32_QUANTIZED fma(u8, 1/255, -0.5)
 *    rounded once (what gv_preprocess_views computes from 8-bit views: a render equals its own PNG round trip);
 *    GV_RENDER_OUT_F32 c - 0.5.
 *    face_id int32 [N,V,H,W] (-1 background) and depth uint32 [N,V,H,W] (Z, 0xFFFFFFFF background) are optional.
 * Sequence: ws = workspace_bytes(...); prepare(...) writes *pair_total and status[N] (device memory); the host reads the
 * total; bins = bins_bytes(total) bytes; draw(...) writes the views.  Bitwise deterministic for any batch split or
 * mesh order.  Limits: H, W <= 512, V <= 64, N <= 65535, max_tris (the largest nt of the batch: it sizes the grid)
 * <= 2^24 (GV_E_UNSUPPORTED beyond).  Argument errors (GV_E_BADARG before any HIP call): a NULL required pointer, a
 * size <= 0, fit outside (0, 1], ambient outside [0, 1], a non-finite colour / light / projection constant, D <= 1,
 * unknown flags or output, a workspace / bins buffer smaller than the size query's answer; GV_E_ALIGN for a
 * workspace / bins pointer that is not 16-byte aligned or a 4-byte output that is not 4-byte aligned. */
#define GV_RENDER_PERSPECTIVE 1       /* gv_render_desc.flags */
#define GV_RENDER_TWO_SIDED 2
#define GV_RENDER_OUT_F32_QUANTIZED 0 /* output selectors */
#define GV_RENDER_OUT_F32 1
#define GV_RENDER_OUT_U8 2
#define GV_RENDER_OK 0                /* per-mesh status: rendered */
#define GV_RENDER_EMPTY 1             /* no triangles or no vertices: background */
#define GV_RENDER_ZERO_RADIUS 2       /* every vertex at one point: background */
#define GV_RENDER_NONFINITE 3         /* radius or scale not finite: background */
#define GV_RENDER_TOO_LARGE 4         /* more than 2^24 triangles: background */
#define GV_RENDER_BAD_OFFSETS 5       /* offsets decreasing or beyond total_verts / total_tris: background */
typedef struct gv_render_desc {
    int32_t height, width, num_views, flags;
    float fit;                        /* (0, 1] */
    float proj_scale;                 /* k */
    float persp_dist, depth_a, depth_b; /* D, a, b (perspective only) */
    float ambient;
    float light[3];
    float color[3];
    float background[3];
} gv_render_desc;
/* Bytes of the size-determined workspace (16-byte aligned; total_tris = tri_offsets[N] - tri_offsets[0]). */
int64_t gv_render_workspace_bytes(int32_t n, int32_t num_views, int32_t height, int32_t width, int64_t total_tris);
/* Normalise, set up and count the (triangle, view, tile) pairs: *pair_total (int64, device) and status [N] (device). */
int gv_render_prepare(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
                      int32_t n, int64_t total_verts, int64_t total_tris, int32_t max_tris, const gv_render_desc* desc,
                      const float* cameras, const float* rotations, void* workspace, int64_t workspace_bytes,
                      int64_t* pair_total, int32_t* status, void* stream);
/* Bytes of the tile lists for `total` pairs. */
int64_t gv_render_bins_bytes(int64_t total);
/* Scatter, raster and resolve with the workspace of the prepare call on the same arguments; out [N,V,H,W,3] as
 * `output` selects; face_id / depth nullable. */
int gv_render_draw(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
                   int32_t n, int64_t total_verts, int64_t total_tris, int32_t max_tris, const gv_render_desc* desc,
                   const float* cameras, const float* rotations, void* workspace, int64_t workspace_bytes, void* bins,
                   int64_t bins_bytes, int64_t total, int32_t output, void* out, int32_t* face_id, uint32_t* depth,
                   void* stream);
/* Anti-aliased renders: the same pair with S x S coverage and depth samples per pixel, S = samples in {1, 2, 4}, kept
 * in registers and resolved to one pixel in the same launch.  Everything up to the snapped vertices and the shading
 * factor is unchanged.
 *  - sample positions: step = 256 / S; sample (a, b) of pixel (i, j), a, b in [0, S), sits at x = 256 i + step*a + step/2,
 *    y = 256 j + step*b + step/2: integers on the vertices' grid (S = 2: offsets 64, 192; S = 4: 32, 96, 160, 224; S = 1:
 *    the pixel centre).
 *  - coverage and depth: every sample is treated exactly as a pixel centre above (integer edge functions at the sample,
 *    top-left rule, Z = (e0*Z0 + e1*Z1 + e2*Z2) div area, smallest key (Z << 32) | id).  Coordinates are not rescaled:
 *    the 2^62 bound holds as it stands.
 *  - binning: with g = S*i + a the sample index along an axis, a triangle's sample box is
 *    g0 = max((min + step/2 - 1) >> log2(step), 0) .. g1 = min((max - step/2) >> log2(step), S*W - 1) (rows likewise, with
 *    H); it is dropped when g0 > g1 and belongs to the tiles of pixels g0 / S .. g1 / S (S = 1: (min + 127) >> 8 ..
 *    (max - 128) >> 8).  The tile lists therefore depend on S: draw_ss must be given the samples of the prepare_ss that
 *    filled the workspace.
 *  - resolve: sample colour c_s = background, or color * f of its triangle.  GV_RENDER_OUT_U8: u8_s = clamp(floor(c_s*255
 *    + 0.5), 0, 255) per sample and channel, pixel = (sum_s u8_s + S*S/2) div (S*S), exact integers;
 *    GV_RENDER_OUT_F32_QUANTIZED: fma(pixel u8, 1/255, -0.5) (still its own PNG round trip); GV_RENDER_OUT_F32: per
 *    channel the c_s added in row-major sample order (b outer, a inner), one rounding per add, times 1/(S*S) (exact), plus
 *    -0.5 (S = 1: c - 0.5).
 *  - face_id / depth, when requested, are on the sample grid: [N, V, S*H, S*W], sample (a, b) of pixel (i, j) at row
 *    S*j + b, column S*i + a; background -1 / 0xFFFFFFFF.
 * Status codes, gv_render_workspace_bytes and gv_render_bins_bytes (with the pair total of prepare_ss) are unchanged.
 * samples <= 0 or not a power of two: GV_E_BADARG; a power of two above 4: GV_E_UNSUPPORTED; every other rejection as in
 * the pair above.  samples = 1 gives bitwise the results of the pair above. */
int gv_render_prepare_ss(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                         const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                         int32_t max_tris, const gv_render_desc* desc, const float* cameras, const float* rotations,
                         void* workspace, int64_t workspace_bytes, int64_t* pair_total, int32_t* status, int32_t samples,
                         void* stream);
int gv_render_draw_ss(const float* verts, const int64_t* vert_offsets, const int32_t* tris, const int64_t* tri_offsets,
                      int32_t n, int64_t total_verts, int64_t total_tris, int32_t max_tris, const gv_render_desc* desc,
                      const float* cameras, const float* rotations, void* workspace, int64_t workspace_bytes, void* bins,
                      int64_t bins_bytes, int64_t total, int32_t output, void* out, int32_t* face_id, uint32_t* depth,
                      int32_t samples, void* stream);
/* Smooth shading: per-vertex normals computed on the device for each render and interpolated per coverage sample in the
 * raster kernel's resolve (Phong reflection: a diffuse and an optional specular term, a light per view).  Coverage,
 * depth, face_id, binning and the resolve from the sample colours on are exactly those above; only the colour of a
 * covered sample changes.  Every fp32 step rounds on its own (no FMA), so the pictures stay defined bit for bit.
 *  - face vector of triangle t: n_t = (w1-w0) x (w2-w0) from world positions, the steps of the flat shading, left
 *    unnormalised (the sum below is area-weighted; a triangle that names a vertex twice gives exactly zero).
 *  - GV_RENDER_TWO_SIDED: before it is summed, n_t is turned to face the viewer of view v: d = (F0*n0 + F1*n1) + F2*n2
 *    with F the forward row of C_v (orthographic and perspective alike); n_t is negated when d > 0.  The normal table
 *    is then [V, total_verts, 3], otherwise [1, total_verts, 3].
 *  - vertex normal: the corners of vertex i are the (triangle, corner) pairs that name it, of triangles whose three
 *    indices are all inside [0, nv); corner_offsets int64 [total_verts + 1] (per vertex of the packed arrays; as with
 *    the mesh offsets, corner_offsets[0] need not be 0: vertex i owns corner_tris[corner_offsets[i]-corner_offsets[0]
 *    .. corner_offsets[i+1]-corner_offsets[0]) of the array passed) and corner_tris int32 [total_corners], the LOCAL
 *    triangle ids in ascending order (a stable sort of the flattened index array).  g_i = the face vectors of the list
 *    added per component in list order, starting from the first; nn = (g0*g0 + g1*g1) + g2*g2; the unit normal is
 *    g_i / sqrt(nn) per component when nn is finite and > 0, else (0, 0, 0).  One thread per (table, vertex), no
 *    atomics: a pure function of the inputs.  Vertices of a mesh whose status is not GV_RENDER_OK get (0, 0, 0).
 *  - per covered sample: the winning key holds depth and id only; the triangle's setup is recomputed from the id and,
 *    with it, the three integer edge functions e0 = E_12, e1 = E_20, e2 = E_01 at the sample.  Where the setup swapped
 *    vertices 1 and 2 (negative screen area) the normals follow: (a, b, c) = (i0, i2, i1).  b_k = (float)e_k /
 *    (float)area (int64 -> fp32 round to nearest even), n = ((b0*ga + b1*gb) + b2*gc) per component: affine in SCREEN
 *    space like the depth, NOT perspective-correct.  nn = (n0*n0 + n1*n1) + n2*n2; when nn is not finite and > 0 the
 *    sample takes colour = color * f of its triangle from the flat table of the prepare call (desc->light, h =
 *    (s+1)*0.5 or |s|) and no specular term.
 *  - shading: s = ((l0*n0 + l1*n1) + l2*n2) / sqrt(nn) with l = lights[v]; h = (s+1)*0.5, or max(s, 0) with
 *    GV_RENDER_LAMBERT, or |s| with GV_RENDER_TWO_SIDED; f = ambient + (1-ambient) * h.  t = (m.n) / sqrt(nn) with m =
 *    halfs[v], clamped max(t, 0) (|t| with GV_RENDER_TWO_SIDED); p = t squared log2(shininess) times, one rounding per
 *    squaring; channel c = min(color_c * f + specular * p, 1).  lights / halfs [V, 3] are unit vectors built by the
 *    host (float64, rounded to fp32): a world light repeated, or the headlight -F_v; m_v = normalize(l_v + eye_v) with
 *    eye_v = -F_v, a directional viewer for both projections.
 *  - samples > 1: each of the S x S samples is shaded at its own position, then resolved as above.
 * Sequence: prepare[_ss] (binning does not depend on shading; its flat table is the fallback above), then
 * gv_render_vertex_normals into a table of gv_render_normals_bytes(num_views, desc->flags, total_verts) bytes, then
 * gv_render_draw_smooth with the arguments of gv_render_draw_ss, the shading descriptor, lights, halfs and the table.
 * Rejections before any launch: those of the pair above; GV_E_BADARG for a NULL shading / lights / halfs / normals /
 * corner array, unknown shading flags, specular outside [0, 1], a shininess that is no power of two, a normal table
 * smaller than the size query's answer; GV_E_UNSUPPORTED for a power-of-two shininess above 128; GV_E_ALIGN for a normal
 * table that is not 16-byte aligned. */
#define GV_RENDER_LAMBERT 1           /* gv_render_shading.flags: h = max(s, 0) */
typedef struct gv_render_shading {
    int32_t flags;
    int32_t shininess;                /* 1, 2, 4, ..., 128 */
    float specular;                   /* [0, 1] */
    int32_t reserved;
} gv_render_shading;
int64_t gv_render_normals_bytes(int32_t num_views, int32_t flags, int64_t total_verts);
int gv_render_vertex_normals(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                             const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                             int32_t max_tris, const gv_render_desc* desc, const float* cameras, const float* rotations,
                             void* workspace, int64_t workspace_bytes, const int64_t* corner_offsets,
                             const int32_t* corner_tris, int64_t total_corners, float* normals, int64_t normals_bytes,
                             void* stream);
int gv_render_draw_smooth(const float* verts, const int64_t* vert_offsets, const int32_t* tris,
                          const int64_t* tri_offsets, int32_t n, int64_t total_verts, int64_t total_tris,
                          int32_t max_tris, const gv_render_desc* desc, const float* cameras, const float* rotations,
                          void* workspace, int64_t workspace_bytes, void* bins, int64_t bins_bytes, int64_t total,
                          int32_t output, void* out, int32_t* face_id, uint32_t* depth, int32_t samples,
                          const gv_render_shading* shading, const float* lights, const float* halfs,
                          const float* normals, int64_t normals_bytes, void* stream);

/* ---- points in: multi-view point splatter (scans, LiDAR crops, sampled meshes: shapes that are not triangulated) -----
 * Turns N point clouds into the same views [N, V, H, W, 3] as "meshes in", under the same discipline: fp32 with every
 * step rounded on its own (no FMA), integer coverage, results defined bit for bit and independent of scheduling.
 *  - clouds: fp32 points [sum P, 3] concatenated, int64 point_offsets [N+1] (offsets[0] need not be 0, as for meshes).
 *    The index of a point within its cloud is its id.  Optional unit-free normals [sum P, 3], one per point, laid out
 *    like the points.
 *  - normalisation, rotation, cameras, projection, snap and depth: exactly those of "meshes in", applied to the cloud's
 *    points (c = bbox midpoint, r = max |p - c|, u = (p - c) * (fit / r), w = M u, q = C_v w, X, Y in 1/256 pixel, Z in
 *    24 bits).  Status GV_RENDER_* per cloud: GV_RENDER_EMPTY for a cloud without points, GV_RENDER_ZERO_RADIUS when
 *    all its points coincide (a single point included), GV_RENDER_TOO_LARGE above 2^24 points.
 *  - splat: point i of cloud m is a disc around (X, Y), parallel to the screen, at depth Z over its whole area.  Its
 *    radius in 1/256 pixel, every step rounded: orthographic R = rint(min(max((radius_m * k) * 256, 1), 8192));
 *    GV_RENDER_PERSPECTIVE R = rint(min(max(((radius_m * k) / z) * 256, 1), 8192)) with z = q2 + D of the projection
 *    (min / max as fminf / fmaxf: a NaN gives 1).  radius [N] is per cloud, in normalised units (the unit sphere has
 *    radius 1), HOST memory: gv_points_prepare checks it, copies it into the workspace on the stream (keep it alive
 *    until the stream has passed that copy) and gv_points_draw reads it there.  R <= 8192 (32 pixels) bounds the tiles
 *    a splat touches; R >= 1 only: a disc under about 0.71 pixel (R < 182) can miss every pixel centre and then leaves
 *    no trace.  A point whose world position w is not finite has no snapped position or depth and is skipped.
 *  - coverage, int64: pixel centre P = (256 i + 128, 256 j + 128) is covered when dx*dx + dy*dy <= R*R with
 *    d = P - (X, Y): the boundary is inclusive.  The pixel keeps the smallest key (Z << 32) | id: the nearest splat,
 *    the lower id at equal depth.
 *  - binning: a splat belongs to the 16x16-pixel tiles of the pixels i0 = max((X - R + 127) >> 8, 0) .. i1 =
 *    min((X + R - 128) >> 8, W - 1) (rows likewise); it is dropped when that box is empty.
 *  - shading of the winning splat.  normals == NULL ("depth"): t = float(Z) / 16777215, f = ambient + (1 - ambient) *
 *    (1 - t), channel = color * f: nearer is brighter.  normals != NULL ("normal"): n = M g (g the point's normal; the
 *    rotation's sum order; n = g without rotations), nn = (n0*n0 + n1*n1) + n2*n2, and the reflection model of "smooth
 *    shading" evaluated on n: s = ((l0*n0 + l1*n1) + l2*n2) / sqrt(nn) with l = lights[v]; h = (s+1)*0.5, or
 *    max(s, 0) with GV_RENDER_LAMBERT, or |s| with GV_RENDER_TWO_SIDED; f = ambient + (1-ambient) * h; t = (m.n) /
 *    sqrt(nn) with m = halfs[v], max(t, 0) (|t| with GV_RENDER_TWO_SIDED); p = t squared log2(shininess) times;
 *    channel = min(color * f + specular * p, 1).  A normal whose nn is not finite and > 0 takes the depth factor.
 *    desc->light is not used.
 *  - output, point_id int32 [N,V,H,W] (-1 background) and depth uint32 [N,V,H,W] (0xFFFFFFFF background): as "meshes
 *    in" (one sample per pixel only).
 * Sequence: ws = gv_points_workspace_bytes(...); gv_points_prepare(...) writes *pair_total and status[N] (device
 * memory); the host reads the total; bins = gv_render_bins_bytes(total) bytes; gv_points_draw(...) writes the views.
 * max_points (the largest P of the batch) only sizes the binning grid: any value >= 0 gives the same results.
 * Limits: H, W <= 512, V <= 64, N <= 65535, max_points <= 2^24 (GV_E_UNSUPPORTED beyond).  GV_E_BADARG before any HIP
 * call: a NULL required pointer (shading / lights / halfs are required with normals), a size <= 0, the descriptor
 * errors of "meshes in", a radius that is not finite or not > 0, unknown shading flags, specular outside [0, 1], a
 * shininess that is no power of two (GV_E_UNSUPPORTED above 128), an unknown output, a workspace / bins buffer smaller
 * than the size query's answer; GV_E_ALIGN for a workspace / bins pointer that is not 16-byte aligned or a 4-byte
 * buffer that is not 4-byte aligned. */
int64_t gv_points_workspace_bytes(int32_t n, int32_t num_views, int32_t height, int32_t width);
int gv_points_prepare(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                      int32_t max_points, const float* radius, const gv_render_desc* desc, const float* cameras,
                      const float* rotations, void* workspace, int64_t workspace_bytes, int64_t* pair_total,
                      int32_t* status, void* stream);
int gv_points_draw(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                   int32_t max_points, const gv_render_desc* desc, const float* cameras, const float* rotations,
                   void* workspace, int64_t workspace_bytes, void* bins, int64_t bins_bytes, int64_t total,
                   int32_t output, void* out, int32_t* point_id, uint32_t* depth, const float* normals,
                   const gv_render_shading* shading, const float* lights, const float* halfs, void* stream);
/* Normal estimation: the normals "normal" shading needs, for clouds that come without (raw scans): per point the exact
 * k nearest neighbours within its own cloud, the covariance of that neighbourhood, the eigenvector of its smallest
 * eigenvalue, a sign convention.  Defined bit for bit: independent of scheduling, of how a batch is split, of the grid
 * size and of the order of the points in memory (up to the ids that order gives); no floating-point atomics.
 *  - inputs: points / point_offsets as above (a point's id is its index within its cloud); k in [3, 32]; orient, one of
 *    GV_NORMALS_ORIENT_*; viewpoint[3], HOST memory, read before the call returns (GV_NORMALS_ORIENT_VIEWPOINT only,
 *    otherwise it may be NULL); grid_cells: 0 = auto, else 1..128, a hint that only sizes the search grid; max_points
 *    (the largest P of the batch) only sizes the launches.  Any value of either gives the same results.
 *  - neighbours of point i of a cloud of P points: k_eff = min(k, P).  fp32, every step rounded on its own (no FMA):
 *    dx = xj - xi, dy = yj - yi, dz = zj - zi, d2 = (dx*dx + dy*dy) + dz*dz for every j of the cloud, i included
 *    (d2 = 0).  key = ((uint64)bits(d2) << 32) | j.  The neighbourhood is the k_eff smallest keys in ascending order
 *    (rank 0 .. k_eff-1): among equal distances the lower id wins.  This is the brute-force answer; the search grid
 *    only finds it faster.
 *  - covariance, fp64, every operation rounded on its own, in rank order: d_r = (double)p_r - (double)p_i per
 *    component; s = d_0 + d_1 + ... (from 0.0, left to right); m = s / (double)k_eff; C starts as 0.0 and for r = 0 ..
 *    k_eff-1, with e = d_r - m: C00 += e0*e0, C01 += e0*e1, C02 += e0*e2, C11 += e1*e1, C12 += e1*e2, C22 += e2*e2.
 *  - eigenvectors: cyclic Jacobi on A = C with V = I, fp64, only + - * / and a correctly rounded sqrt.  6 sweeps, each
 *    the pairs (p, q) = (0,1), (0,2), (1,2) in that order, r the third index.  A pair whose A_pq is exactly 0 is skipped.
 *    Otherwise theta = (A_qq - A_pp) / (2 * A_pq); t = sgn / (|theta| + sqrt(theta*theta + 1)) with sgn = -1 when
 *    theta < 0, else 1; c = 1 / sqrt(t*t + 1); s = t * c; h = t * A_pq; A_pp = A_pp - h; A_qq = A_qq + h; A_pq = 0;
 *    (A_rp, A_rq) = (c*A_rp - s*A_rq, s*A_rp + c*A_rq) from the old pair; and for each row i = 0, 1, 2 of V:
 *    (V_ip, V_iq) = (c*V_ip - s*V_iq, s*V_ip + c*V_iq).  The eigenvalues are the diagonal of A, ordered l0 <= l1 <= l2
 *    with ties by column index; the normal is column c0 of V, the column of l0, as it stands (unit up to the rounding
 *    of the rotations: it is not normalised again).
 *  - degenerate: k_eff < 3, l2 == 0, or l1 <= 1e-12 * l2 (coincident or collinear neighbourhoods).  Normal (0, 0, 0),
 *    variation 0, and GV_POINTS_DEGENERATE_NORMAL is set in the cloud's status.  The splatter gives a zero normal the
 *    depth factor.
 *  - sign, fp64.  "none" rule: the component of largest magnitude becomes positive (the first of x, y, z on a tie).
 *    GV_NORMALS_ORIENT_NONE: that rule.  GV_NORMALS_ORIENT_OUTWARD: w = p_i - c with c = 0.5 * ((double)min +
 *    (double)max) of the cloud's bounding box per component; GV_NORMALS_ORIENT_VIEWPOINT: w = (double)viewpoint - p_i.
 *    d = (n0*w0 + n1*w1) + n2*w2; the normal is negated when d < 0; d == 0 falls back to the "none" rule.
 *  - outputs: normals fp32 [sum P, 3], each fp64 component rounded once; neighbours int32 [sum P, k] or NULL: the ids
 *    in rank order, -1 from k_eff on; variation fp32 [sum P] or NULL: l0 / ((l0 + l1) + l2) in fp64, rounded once;
 *    status int32 [N], device memory: GV_RENDER_OK, GV_RENDER_EMPTY (no points), GV_RENDER_NONFINITE (a point that is
 *    not finite, or a bounding box whose extent is not: zero normals, -1 neighbours, variation 0), GV_RENDER_TOO_LARGE
 *    / GV_RENDER_BAD_OFFSETS (nothing is written for the cloud), with GV_POINTS_DEGENERATE_NORMAL or-ed in.
 * workspace: gv_points_normals_workspace_bytes(n, total_points, grid_cells) bytes, 16-byte aligned; nothing else is
 * allocated, and two calls on two streams with two workspaces do not interfere.  GV_E_BADARG before any HIP call: a
 * NULL points / point_offsets / normals / workspace / status, n <= 0, total_points or max_points < 0, k outside [3, 32],
 * an unknown orient, GV_NORMALS_ORIENT_VIEWPOINT without a viewpoint or with one that is not finite, grid_cells outside
 * [0, 128], a workspace smaller than the size query's answer; GV_E_UNSUPPORTED for n > 65535 or max_points > 2^24;
 * GV_E_ALIGN for a workspace that is not 16-byte aligned, point_offsets not 8-byte aligned or a 4-byte buffer that is
 * not 4-byte aligned.
 * Known limit: a cloud with a far outlier has nearly all its points in one cell of the grid; its queries then cost
 * O(P) each.  The results are the same. */
#define GV_NORMALS_ORIENT_NONE 0
#define GV_NORMALS_ORIENT_OUTWARD 1
#define GV_NORMALS_ORIENT_VIEWPOINT 2
#define GV_POINTS_DEGENERATE_NORMAL 0x100  /* or-ed into status[m]: some point of cloud m has a degenerate neighbourhood */
int64_t gv_points_normals_workspace_bytes(int32_t n, int64_t total_points, int32_t grid_cells);
int gv_points_estimate_normals(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                               int32_t max_points, int32_t k, int32_t orient, const float* viewpoint, int32_t grid_cells,
                               float* normals, int32_t* neighbours, float* variation, void* workspace,
                               int64_t workspace_bytes, int32_t* status, void* stream);
/* Cleaning: what a raw scan needs before its normals are estimated and before the normalisation above may trust every
 * point: statistical outlier selection, voxel selection, and the one compaction that turns either selection into a new
 * batch.  Defined bit for bit, under the discipline of the normals call: independent of scheduling, of how a batch is
 * split, of grid_cells / max_points and of the order of the points in memory (up to the ids that order gives); no
 * floating-point atomics; every step rounded on its own (no FMA).
 *  - inputs: points / point_offsets / max_points / grid_cells as for the normals call.  The per-cloud status [N] (device
 *    memory) comes from the same bounding-box pass.  GV_RENDER_EMPTY, GV_RENDER_TOO_LARGE and GV_RENDER_BAD_OFFSETS:
 *    nothing is written for the cloud and its output count is 0.  GV_RENDER_NONFINITE: the cloud passes through unchanged
 *    (every keep flag 1, centroid = the point, index = its id, mean_dist 0, stats 0) with GV_POINTS_CLEAN_PASSTHROUGH
 *    or-ed into its status.
 *  - gv_points_outlier_select: k in [1, 32], std_ratio finite and >= 0.  Neighbours of point i of a cloud of P points: the
 *    fp32 d2 and the keys (bits(d2) << 32) | j of the normals contract over every j != i; the neighbourhood is the k_eff =
 *    min(k, P - 1) smallest keys in ascending order.  Mean distance, fp64, every step rounded: m_i = (sqrt((double)d2_0)
 *    + ... + sqrt((double)d2_{k_eff-1})) / (double)k_eff, summed from 0.0 left to right in rank order, sqrt correctly
 *    rounded.  Sums over a cloud are the tree sum T(a): a_0 .. a_{P-1} padded with +0.0 to the next power of two, then
 *    level by level b_t = a_{2t} + a_{2t+1} until one value is left (a fixed tree over ids).  mu = T(m) / (double)P; e_i =
 *    m_i - mu; sigma = sqrt(T(e*e) / (double)(P - 1)); T = mu + (double)std_ratio * sigma; keep_i = (m_i <= T).  P < 2:
 *    every point is kept, m_i = 0 and the stats are 0.  Outputs: keep int32 [sum P] (1 / 0); mean_dist fp32 [sum P] or
 *    NULL: m_i rounded once; stats fp64 [N, 3] or NULL: (mu, sigma, T), zeros for a cloud without a selection.
 *  - gv_points_voxel_select: voxel fp32 [N], HOST memory (copied into the workspace on the stream: keep it alive until
 *    the stream has passed that copy); relative 0 / 1.  Per cloud, with mn / ext the bounding box's minimum and fp32
 *    extent per axis: h = voxel_m, or fl(voxel_m * max(ext_x, ext_y, ext_z)) when relative.  An h that is not finite or
 *    not > 0, or fl(ext_a / h) >= 2097152 on some axis: the cloud passes through unchanged with
 *    GV_POINTS_CLEAN_PASSTHROUGH.  Cell of a point per axis: t = x - mn, q = t / h (a correctly rounded fp32 division),
 *    c = (int)q; the voxel key is (c2 << 42) | (c1 << 21) | c0.  Centroid through integers, so that no order enters:
 *    frexpf(max ext) = f * 2^E and s = 2^(29 - E) as a double (s = 1 when the largest extent is 0); F = llrint((double)t
 *    * s) per axis (the product is exact; ties to even); S = the int64 sum of F over the voxel's n_v members (at most
 *    2^53); centroid = (float)((double)mn + ((double)S / (double)n_v) / s), each fp64 step rounded, one rounding to
 *    fp32.  Representative member: the smallest key (bits(d2) << 32) | id over the members, d = p - centroid per
 *    component in fp32 and d2 = (dx*dx + dy*dy) + dz*dz.  Outputs at the voxel's LOWEST member id: keep 1, centroids
 *    [sum P, 3] the centroid, index int32 [sum P] the representative's id; at every other member: keep 0, centroid
 *    (0, 0, 0), index -1.  GV_POINTS_CLEAN_TABLE_FULL in a status says the voxel table overflowed: a defect, never a
 *    property of the input (the table holds more slots than the cloud has points).
 *  - gv_points_compact: per cloud the exclusive scan of keep in id order; counts int32 [N] and the new point_offsets
 *    int64 [N + 1] (from 0), both device memory; out_points [new sum P, 3] = selected (the centroids) or, with selected
 *    NULL, the points themselves; out_index int32 [new sum P] = index or, with index NULL, the point's own id: ids within
 *    the ORIGINAL cloud; out_normals = normals[out_index], with normals NULL none (both or neither).  The kept points of
 *    a cloud stay in ascending id order, so voxels come in the order of their lowest member.  status: the selection's,
 *    read on the device.  Output buffers are caller-allocated at the old sum P.
 * workspace: gv_points_clean_workspace_bytes(n, total_points, grid_cells) bytes, 16-byte aligned, serves all three calls
 * (the compaction with any grid_cells).  The argument errors are those of the normals call, before any HIP call:
 * GV_E_BADARG for a NULL required pointer, n <= 0, total_points or max_points < 0, k outside [1, 32], a std_ratio that is
 * not finite or < 0, relative outside {0, 1}, grid_cells outside [0, 128], normals without out_normals or the reverse, a
 * workspace smaller than the size query's answer; GV_E_UNSUPPORTED for n > 65535 or max_points > 2^24; GV_E_ALIGN for a
 * workspace that is not 16-byte aligned, an 8-byte buffer (point_offsets, stats, out_offsets) that is not 8-byte aligned
 * or a 4-byte buffer that is not 4-byte aligned.
 * Not here: radius-count outlier removal, normals averaged over a voxel, voxel sizes below 2^-21 of the extent. */
#define GV_POINTS_CLEAN_PASSTHROUGH 0x200  /* or-ed into status[m]: cloud m went through unchanged */
#define GV_POINTS_CLEAN_TABLE_FULL 0x400   /* or-ed into status[m]: the voxel table of cloud m overflowed (a defect) */
int64_t gv_points_clean_workspace_bytes(int32_t n, int64_t total_points, int32_t grid_cells);
int gv_points_outlier_select(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                             int32_t max_points, int32_t k, float std_ratio, int32_t grid_cells, int32_t* keep,
                             float* mean_dist, double* stats, void* workspace, int64_t workspace_bytes, int32_t* status,
                             void* stream);
int gv_points_voxel_select(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                           int32_t max_points, const float* voxel, int32_t relative, int32_t grid_cells, int32_t* keep,
                           float* centroids, int32_t* index, void* workspace, int64_t workspace_bytes, int32_t* status,
                           void* stream);
int gv_points_compact(const float* points, const int64_t* point_offsets, int32_t n, int64_t total_points,
                      int32_t max_points, const int32_t* keep, const float* selected, const int32_t* index,
                      const float* normals, const int32_t* status, float* out_points, float* out_normals,
                      int32_t* out_index, int64_t* out_offsets, int32_t* counts, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* Registration: rigid point-to-point ICP (iterative closest point) for a batch of N pairs (source cloud m, target cloud
 * m): the rotation R and translation t that carry the source onto the target, found by repeating "nearest target point
 * of every moved source point, then the best rigid motion for those matches".  Everything runs on the stream with no
 * read-back between rounds.  Defined bit for bit, under the discipline of the calls above: independent of scheduling, of
 * how a batch is split, of grid_cells / max_source / max_target; no floating-point atomics; every step rounded on its own
 * (no FMA); fp64 uses only + - * / and a correctly rounded sqrt.  (The order of the SOURCE points fixes the order of the
 * sums; the order of the target points enters through ties alone.)
 *  - inputs: source / source_offsets and target / target_offsets, two batches of N clouds laid out as above; a point's id
 *    is its index within its cloud.  source_normals fp32 [sum Ps, 3] or NULL.  init fp64 [N, 4, 4] row-major, HOST memory
 *    (copied into the workspace on the stream: keep it alive until the stream has passed that copy), or NULL for the
 *    identity: T = (R | t) is its upper three rows, whatever they hold (no check that R is a rotation); its last row is
 *    not read.  iterations >= 1; max_distance fp32 >= 0, +inf for none; tolerance fp64 >= 0; grid_cells as above.
 *  - status byte of pair m: the source cloud's GV_RENDER_* from the bounding-box pass (EMPTY, NONFINITE, TOO_LARGE,
 *    BAD_OFFSETS); where that is GV_RENDER_OK, the target cloud's.  A pair whose byte is not GV_RENDER_OK runs no round:
 *    T stays the initial transform, used = 0, inliers = 0, rmse = 0.
 *  - move, the one formula for a point p under T (here and in the final apply): per component c, in fp64,
 *    q_c = ((R_c0 * (double)p_0 + R_c1 * (double)p_1) + R_c2 * (double)p_2) + t_c, rounded once to fp32.
 *  - round k = 1 .. iterations of a pair that has not stopped, T the pair's current transform:
 *    1. every source point p_i is moved to q_i.  If some component of some q_i is not finite: GV_POINTS_ICP_NONFINITE
 *       is set, the pair stops with used = k, inliers = 0, rmse = 0 and every correspondence -1; T is kept.
 *    2. match: over every target point y_j of the pair, fp32, dx = y_j0 - q_i0, dy, dz likewise, d2 = (dx*dx + dy*dy) +
 *       dz*dz, key = ((uint64)bits(d2) << 32) | j; the match of i is the smallest key: the nearest target point, the
 *       lower id among equal distances.  This is the brute-force answer; the grid over the target only finds it faster.
 *    3. i is an inlier when d2_i <= max_d2 with max_d2 = max_distance * max_distance in fp32 (the boundary included;
 *       +inf stays +inf).  Sums over the source ids are the tree sum T(a) of the cleaning contract, over a_0 .. a_{Ps-1}
 *       with a_i = +0.0 at every i that is no inlier.  First pass: c = T(1.0), Sp = T((double)p_i) (the ORIGINAL source
 *       points), Sy = T((double)y_match(i)) per component, Sd = T((double)d2_i).  used = k, inliers = c.
 *    4. c < 3: GV_POINTS_ICP_FEW_PAIRS is set, rmse = sqrt(Sd / c) (0 when c = 0), T is kept and the pair stops.
 *    5. rmse = sqrt(Sd / c).  From round 2 on: |rmse_prev - rmse| <= tolerance (false for a NaN) sets
 *       GV_POINTS_ICP_CONVERGED; T is kept (it is the transform the matches of this round were found under) and the pair
 *       stops.  Otherwise rmse_prev = rmse.
 *    6. cp = Sp / c, cy = Sy / c per component.  Second pass: H_ab = T(((double)p_ia - cp_a) * ((double)y_ib - cy_b)) for
 *       a, b in 0..2, y_i the match of i.
 *    7. Horn's closed form.  The symmetric 4x4 matrix A: A00 = (H00 + H11) + H22; A11 = (H00 - H11) - H22; A22 = (H11 -
 *       H00) - H22; A33 = (H22 - H00) - H11; A01 = H12 - H21; A02 = H20 - H02; A03 = H01 - H10; A12 = H01 + H10; A13 = H20
 *       + H02; A23 = H12 + H21.  Cyclic Jacobi on A with V = I: 8 sweeps, each the pairs (p, q) = (0,1), (0,2), (0,3),
 *       (1,2), (1,3), (2,3) in that order, with the rotation formulas of the normals contract (a pair whose A_pq is
 *       exactly 0 is skipped; theta, t, c, s, h; A_pp, A_qq, A_pq; then (A_rp, A_rq) = (c*A_rp - s*A_rq, s*A_rp + c*A_rq)
 *       for the two other indices r in ascending order, kept symmetric; then rows i = 0..3 of V).  The eigenvalues are
 *       the diagonal; e = column of V of the largest, the lower column on a tie.  e is negated when its first non-zero
 *       component is negative; nn = ((e0*e0 + e1*e1) + e2*e2) + e3*e3; (w, x, y, z) = e / sqrt(nn) per component.
 *    8. R00 = ((w*w + x*x) - y*y) - z*z; R01 = 2 * (x*y - w*z); R02 = 2 * (x*z + w*y); R10 = 2 * (x*y + w*z); R11 = ((w*w
 *       - x*x) + y*y) - z*z; R12 = 2 * (y*z - w*x); R20 = 2 * (x*z - w*y); R21 = 2 * (y*z + w*x); R22 = ((w*w - x*x) -
 *       y*y) + z*z; t_c = cy_c - ((R_c0 * cp_0 + R_c1 * cp_1) + R_c2 * cp_2).  This (R, t) replaces T whole: it maps the
 *       original source points onto their matches, nothing is composed from round to round.  A unit quaternion always
 *       gives a proper rotation: there is no reflection case.
 *  - outputs, device memory: transforms fp64 [N, 4, 4] (T over the row 0 0 0 1); rmse fp64 [N], inliers int32 [N] and
 *    used int32 [N] (each or NULL): those of the last round the pair ran, so rmse describes the transform that ENTERED
 *    that round; correspondence int32 [sum Ps] or NULL: the match of the last round run, -1 where i was no inlier or
 *    no round ran; moved fp32 [sum Ps, 3]: the source points under the final T; moved_normals fp32 [sum Ps, 3] (with
 *    source_normals, both or neither): ((R_c0 * (double)g_0 + R_c1 * (double)g_1) + R_c2 * (double)g_2), rounded once;
 *    status int32 [N]: the pair's byte with GV_POINTS_ICP_* or-ed in.  Nothing is written to correspondence, moved or
 *    moved_normals for a pair whose SOURCE is EMPTY, TOO_LARGE or BAD_OFFSETS.
 * workspace: gv_points_register_workspace_bytes(n, total_source, total_target, grid_cells) bytes, 16-byte aligned.
 * GV_E_BADARG before any HIP call: a NULL source / source_offsets / target / target_offsets / transforms / moved /
 * workspace / status, source_normals without moved_normals or the reverse, n <= 0, a total or max below 0, iterations
 * < 1, a max_distance or tolerance that is negative or NaN, grid_cells outside [0, 128], a workspace smaller than the size
 * query's answer; GV_E_UNSUPPORTED for n > 65535 or a max above 2^24; GV_E_ALIGN as for the cleaning calls.
 * Not here: point-to-plane ICP, a trimmed fraction of the pairs, a global (initial-pose-free) alignment, more than two
 * clouds in one solve.  Known limit: a source point far outside the target's box walks most of the grid. */
#define GV_POINTS_ICP_CONVERGED 0x800   /* or-ed into status[m]: pair m stopped on the tolerance */
#define GV_POINTS_ICP_FEW_PAIRS 0x1000  /* or-ed into status[m]: a round of pair m had fewer than 3 inliers */
#define GV_POINTS_ICP_NONFINITE 0x2000  /* or-ed into status[m]: a moved source point of pair m was not finite */
int64_t gv_points_register_workspace_bytes(int32_t n, int64_t total_source, int64_t total_target, int32_t grid_cells);
int gv_points_register(const float* source, const int64_t* source_offsets, const float* target,
                       const int64_t* target_offsets, int32_t n, int64_t total_source, int64_t total_target,
                       int32_t max_source, int32_t max_target, const float* source_normals, const double* init,
                       int32_t iterations, float max_distance, double tolerance, int32_t grid_cells, double* transforms,
                       double* rmse, int32_t* inliers, int32_t* used, int32_t* correspondence, float* moved,
                       float* moved_normals, void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);

/* ---- training step (train.py:145,166-187, utils/train_utils.py:217-259) -----------
 * fp32.  Gradient outputs ACCUMULATE (+=) into caller-zeroed buffers, because a tensor that feeds several
 * consumers (an Inception block input, a ResNet shortcut) sums their gradients.
 *
 * Data gradient of a convolution = gv_conv2d_fwd on dZ with the filter flipped and transposed
 * (W'[r',s',co,ci] = W[kh-1-r',kw-1-s',ci,co]), pad' = k-1-pad, stride 1, in_dilation = forward stride,
 * residual = dX (accumulate).  Filter gradient: gv_conv2d_wgrad. */

/* Batch statistics per (group, channel), group of image b = b % num_groups (one group per view: the
 * reference normalises each view's graph copy over its own N*h*w values).  counts[g] = pixels of group g.
 * Writes mean/var(biased)/inv = rsqrt(var+eps) and the folded scale = inv*gamma, shift = beta - mean*scale,
 * all [num_groups, c].  accum: workspace double [num_groups, c, 2].  gamma may be NULL (Inception). */
int gv_bn_stats_grouped(const float* z, int32_t nb, int32_t hw, int32_t c, int32_t z_ld, int32_t num_groups,
                        const int32_t* counts, const float* gamma, const float* beta, float eps,
                        double* accum, float* mean, float* var, float* inv, float* scale, float* shift,
                        void* stream);
/* The two halves of gv_bn_stats_grouped, for data-parallel jobs that cut the batch on SHAPE boundaries: a view's
 * images then live on several ranks, so the per-(view, channel) sums (accum: double [num_groups, c, 2] = sum, sum of
 * squares) are all-reduced between the halves and `counts` holds the GLOBAL pixel counts. */
int gv_bn_sums_grouped(const float* z, int32_t nb, int32_t hw, int32_t c, int32_t z_ld, int32_t num_groups,
                       double* accum, void* stream);
int gv_bn_finalize_grouped(const double* accum, int32_t c, int32_t num_groups, const int32_t* counts,
                           const float* gamma, const float* beta, float eps, float* mean, float* var, float* inv,
                           float* scale, float* shift, void* stream);
/* Moving-average update of slim.batch_norm in training (the UPDATE_OPS train.py:178-186 groups with the
 * optimizer step), one update per view graph copy, applied in view order:
 *   moving_mean = moving_mean*decay + mean[g]*(1-decay)
 *   moving_var  = moving_var *decay + var[g]*n/(n-1)*(1-decay)      (fused batch norm: unbiased estimate)
 * for g = 0..num_groups-1, n = counts[g].  decay: inception_utils.py:32 (0.9997), resnet_utils.py:199 (0.997). */
int gv_bn_update_moving(const float* mean, const float* var, const int32_t* counts, int32_t num_groups,
                        int32_t c, float decay, float* moving_mean, float* moving_var, void* stream);
/* gv_bn_update_moving for every BatchNorm layer of a plan in ONE launch: job j = one layer (device pointers as in
 * gv_bn_update_moving), owning blocks [first_block, first_block + ceil(c / 256)); block_job (device int32) maps a
 * block to its job. */
typedef struct gv_bn_moving_job {
    const float* mean;
    const float* var;
    const int32_t* counts;
    float* moving_mean;
    float* moving_var;
    int32_t c;
    int32_t first_block;
    int32_t ld;                 /* row stride of mean / var in elements (0 = c): statistics gathered from all ranks sit
                                   side by side in one [views, sum of 2c] message */
    int32_t reserved;
} gv_bn_moving_job;
int gv_bn_update_moving_batched(const gv_bn_moving_job* jobs_dev, int32_t num_jobs, const int32_t* block_job_dev,
                                int32_t num_blocks, int32_t num_groups, float decay, void* stream);
/* y = act(x*scale[g][c] + shift[g][c]), g = image % num_groups. */
int gv_scale_shift_act_grouped(const float* x, int32_t nb, int32_t hw, int32_t c, int32_t x_ld,
                               const float* scale, const float* shift, int32_t num_groups, int32_t relu,
                               float* y, int32_t y_ld, void* stream);
/* Backward of y = relu(BN_train(z)) (y == NULL: no ReLU): dz += gamma*inv*(g - mean_g(g) - zhat*mean_g(g*zhat)),
 * g = dy*[y>0]; dbeta[c] += sum g, dgamma[c] += sum g*zhat (either may be NULL). */
int gv_bn_relu_bwd_grouped(const float* dy, int32_t dy_ld, const float* y, int32_t y_ld, const float* z,
                           int32_t z_ld, const float* mean, const float* inv, const float* gamma,
                           const int32_t* counts, int32_t nb, int32_t hw, int32_t c, int32_t num_groups,
                           double* accum, float* dz, int32_t dz_ld, float* dbeta, float* dgamma, void* stream);
/* The two halves of gv_bn_relu_bwd_grouped (sums of g and g*zhat -> all-reduce over the ranks -> apply with the
 * global counts).  After the all-reduce dbeta / dgamma are already the GLOBAL gradients on every rank. */
int gv_bn_relu_bwd_sums_grouped(const float* dy, int32_t dy_ld, const float* y, int32_t y_ld, const float* z,
                                int32_t z_ld, const float* mean, const float* inv, int32_t nb, int32_t hw, int32_t c,
                                int32_t num_groups, double* accum, void* stream);
int gv_bn_relu_bwd_apply_grouped(const float* dy, int32_t dy_ld, const float* y, int32_t y_ld, const float* z,
                                 int32_t z_ld, const float* mean, const float* inv, const float* gamma,
                                 const int32_t* counts, int32_t nb, int32_t hw, int32_t c, int32_t num_groups,
                                 const double* accum, float* dz, int32_t dz_ld, float* dbeta, float* dgamma,
                                 void* stream);
/* x *= s (the 1/world factor of a loss averaged over a sharded batch). */
int gv_scale(float* x, int64_t n, float s, void* stream);
/* dst[p][c] += src[p][c]: gradient fan-in of `shortcut + residual` (nets/resnet_v2.py:91). */
int gv_accumulate(const float* src, int32_t src_ld, float* dst, int32_t dst_ld, int64_t npix, int32_t c,
                  void* stream);
/* dbias[c] += sum over pixels of dz (bias-only convolutions, nets/resnet_v2.py:79-89,178-180). */
int gv_bias_grad(const float* dz, int32_t dz_ld, int64_t npix, int32_t c, double* accum, float* dbias,
                 void* stream);
/* dW_hwio[r,s,ci,co] += sum_pixels x[shifted pixel, ci] * dz[pixel, co]  (descriptor of the FORWARD conv).
 * x and dz in d->dtype (GV_F32: exact fp32 MFMA; GV_BF16 / GV_F16: 16-bit MFMA, fp32 accumulation); dW is fp32. */
int gv_conv2d_wgrad(const gv_conv_desc* d, const void* x, const void* dz, int32_t dz_ld, float* dw_hwio,
                    void* stream);
/* The same gradient, bitwise reproducible (the reference's CPU gradients are: utils/train_utils.py:217-259; the plain
 * form combines its pixel slices with fp32 atomics, whose arrival order decides the last bits).  Every pixel slice
 * STORES its partial image of dW into `workspace` (caller-owned device memory, 16-byte aligned, workspace_bytes long;
 * contents are scratch) and one more launch adds the slices into dw_hwio in slice order.  The number of slices is
 * limited to the images the workspace holds (workspace_bytes / (4 * kh*kw*cin*cout)); with room for fewer than two the
 * launch runs un-split.  Same descriptor, same tile_cfg values, same result up to fp32 summation order. */
int gv_conv2d_wgrad_ws(const gv_conv_desc* d, const void* x, const void* dz, int32_t dz_ld, float* dw_hwio,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* Pool backward (descriptor of the forward pool): max -> first maximum of each window (tf MaxPoolGrad),
 * avg -> dy / #valid taps.  x is the forward input (max only).  x, dy, dx in d->dtype.  GV_E_BADARG: a non-positive
 * dimension, dy_ld or dx_ld below c, a window without a valid tap. */
int gv_pool2d_bwd(const gv_pool_desc* d, const void* x, const void* dy, int32_t dy_ld, void* dx,
                  int32_t dx_ld, void* stream);
/* Max pool for the training step (slim.max_pool2d, nets/inception_v3.py:112,127 / nets/resnet_v2.py:181, under a
 * gradient tape): the forward also records, per output element, the row-major window tap of its FIRST maximum
 * (argmax: uint8 [nb, oh, ow, c], dense), and the backward routes dy by that record — same result as gv_pool2d_bwd
 * (tf MaxPoolGrad: first maximum) without re-reading the forward input.  d: the forward descriptor, mode GV_POOL_MAX
 * (| GV_POOL_BWD_STORE in the backward: dx = instead of dx +=), kh*kw <= 255; x, y, dy, dx in d->dtype. */
int gv_pool2d_fwd_argmax(const gv_pool_desc* d, const void* x, void* y, uint8_t* argmax, void* stream);
int gv_pool2d_bwd_argmax(const gv_pool_desc* d, const uint8_t* argmax, const void* dy, int32_t dy_ld, void* dx,
                         int32_t dx_ld, void* stream);
/* A max pool that directly follows relu(BatchNorm_train(z)) with a positive BatchNorm scale (slim's Inception arg scope:
 * no gamma — nets/inception_utils.py:36; Conv2d_2b -> MaxPool_3a, Conv2d_4a -> MaxPool_5a: nets/inception_v3.py:107-128)
 * may pool z ITSELF: BN + ReLU are monotone there, so max(relu(bn(z))) = relu(bn(max z)) with the same winner, bit for
 * bit.  Forward: gv_pool2d_fwd_argmax on z, then gv_bn_finalize_apply_grouped_t on the POOLED tensor with the sums and
 * counts of the whole z (a quarter of the elements to normalise, and the activation at the un-pooled size never exists).
 * Backward: the BatchNorm sums are sums over the pooled elements (gv_bn_relu_bwd_sums_grouped_t on (d pooled, pooled z):
 * only a window's winner carries a gradient), gv_bn_bwd_coeffs_t turns them into the per-(group, channel) coefficients of
 * dz = A*g + B*z + C (and adds dbeta / dgamma), and gv_pool2d_bwd_argmax_bn gathers every input pixel's gradient g from
 * the windows that elected it (as gv_pool2d_bwd_argmax), masks it with [z*scale + shift > 0] and stores dz — the gradient
 * of the activation is never materialised either.  3x3 / stride 2 / VALID windows, 16-bit storage. */
int gv_bn_bwd_coeffs_t(const double* accum, const int32_t* counts, const float* mean, const float* inv, const float* gamma,
                       int32_t c, int32_t num_groups, int32_t raw_z, float* coef_a, float* coef_b, float* coef_c,
                       float* dbeta, float* dgamma, void* stream);
int gv_pool2d_bwd_argmax_bn(const gv_pool_desc* d, const uint8_t* argmax, const void* dy, int32_t dy_ld, const void* z,
                            int32_t z_ld, int32_t num_groups, const float* coef_a, const float* coef_b, const float* coef_c,
                            const float* scale, const float* shift, void* dz, int32_t dz_ld, void* stream);
/* Backward of gv_view_pool_fuse_fwd: dF += ... (tf.reduce_max splits equally among ties). */
int gv_view_pool_fuse_bwd(const float* F, const float* dS, int32_t num_views, int32_t num_shapes, int64_t E,
                          int64_t view_stride, int64_t shape_stride, const int32_t* scheme,
                          int32_t num_groups, const float* weight, int32_t mode, float* dF, void* stream);
/* The same with one scheme [G,V] / weight [G] per shape (gv_view_pool_fuse_fwd_per_shape); the scores that produced
 * scheme and weight receive no gradient FROM THIS CALL (scheme and weight are its constants, as in the batch form).
 * With mean_score weights the weight is a function of the scores: gv_group_weight_bwd_per_shape + gv_view_score_bwd
 * below compute that gradient, down to the scorer and the raw tap. */
int gv_view_pool_fuse_bwd_per_shape(const float* F, const float* dS, int32_t num_views, int32_t num_shapes,
                                    int64_t E, int64_t view_stride, int64_t shape_stride, const int32_t* scheme,
                                    int32_t num_groups, const float* weight, int32_t mode, float* dF, void* stream);
/* ---- the scorer's gradient (per-shape grouping, GV_WEIGHT_MEAN_SCORE) ----------------------------------------------
 * S = sum_g w_g D_g / W with w_g = mean of the member scores is differentiable in the scores; the binning that decides
 * the members is piecewise constant and stays a constant of the backward pass (no straight-through term).
 *   dw[n,g] = (1/W) sum_e dS[n,e] (D_g[n,e] - S[n,e])     0 for an empty group and for W = 0
 * D_g and S are recomputed from F, scheme and weight with the forward kernel's arithmetic (no stored S is read); an
 * empty group counts with weight 0, which is what GV_WEIGHT_MEAN_SCORE gives it.  F in `dtype`, dS fp32 [N,E], dw fp32
 * [N,G].  Workgroups store their partial sums into ws ([N][chunks][G] fp32, at least
 * gv_group_weight_bwd_workspace_bytes, 4-byte aligned), a second launch adds them in chunk order: no atomics, the same
 * bits every run.  V, G <= 64, N <= 65535.  Argument errors (before any HIP call): GV_E_UNSUPPORTED for an unknown
 * dtype or a size above its cap, GV_E_BADARG for a NULL pointer, a size <= 0, an unknown mode, a short workspace. */
int64_t gv_group_weight_bwd_workspace_bytes(int32_t num_shapes, int64_t E, int32_t num_groups);
int gv_group_weight_bwd_per_shape(const void* F, const float* dS, int32_t num_views, int32_t num_shapes, int64_t E,
                                  int64_t view_stride, int64_t shape_stride, const int32_t* scheme, int32_t num_groups,
                                  const float* weight, int32_t mode, float* dw, void* ws, int64_t ws_bytes,
                                  int32_t dtype, void* stream);
/* From dw to the scorer (image b = n*num_views + v, shape-major; gidx [N,V] as gv_group_assign_per_shape wrote it):
 *   dr_b       = dw[n, gidx_b] / #{u: gidx[n,u] = gidx_b} * sign(r_b) / (1 + |r_b|)^2     (= dL/ds * sign(r) (1 - s)^2;
 *                0 for r_b = 0 and for a view in no group, gidx_b outside [0, G))
 *   dbias[v]   = sum_n dr_{n,v}                                    (n ascending; stored)
 *   dkernel[v] = sum_n dr_{n,v} * mean_p raw[n,v,p,:]              (fp32 [V,cr]; stored)
 *   draw[b,p,c] = (accumulate ? draw[b,p,c] : 0) + dr_b * kernel[v,c] / hw     (nullable; one rounding into `dtype`)
 * raw and draw are `dtype` tensors [nb, hw, cr] with pixel strides raw_ld / draw_ld >= cr (a channel slice of a wider
 * tensor; the columns past cr are not touched).  Three launches, fixed reduction order.  nb <= 65535, V, G <= 64. */
int gv_view_score_bwd(const void* raw, int32_t nb, int32_t hw, int32_t cr, int32_t raw_ld, const float* kernel,
                      const float* r_img, const int32_t* gidx, const float* dw, int32_t num_groups, int32_t num_views,
                      float* dkernel, float* dbias, void* draw, int32_t draw_ld, int32_t accumulate, int32_t dtype,
                      void* stream);
int gv_global_avg_pool_bwd(const float* dgap, int32_t nb, int32_t hw, int32_t c, float* dx, int32_t dx_ld,
                           void* stream);
/* Mean sparse-softmax cross-entropy (train.py:145): loss (device scalar) and dlogits = (softmax-onehot)/n. */
int gv_softmax_ce(const float* logits, const int64_t* labels, int32_t n, int32_t c, float* loss,
                  float* dlogits, void* stream);
/* Dense backward: dx = dy W^T (overwritten); dkernel += x^T dy; dbias += sum dy. */
int gv_dense_bwd(const float* x, const float* dy, const float* kernel, int32_t n, int32_t f, int32_t c,
                 float* dx, float* dkernel, float* dbias, void* stream);
/* tf.train.MomentumOptimizer(lr, mu) with the slim L2 term: m = mu*m + (g + wd*w); w -= lr*m. */
int gv_sgd_momentum(float* w, const float* g, float* m, int64_t n, float lr, float mu, float wd,
                    void* stream);

/* ---- the training step on any storage type (configs[2]: bf16 forward + backward) -----------------------
 * Storage-typed forms of the functions above: activations and activation gradients (z, y, dy, dz, F, dF, src, dst)
 * are `dtype` elements (GV_F32, GV_BF16 or GV_F16; the fp32 functions above forward here with GV_F32), arithmetic is
 * fp32 with one rounding per stored element, batch statistics accumulate in fp64, parameter gradients (dbeta, dgamma, dbias, dW),
 * dS and the optimizer state stay fp32.  gv_conv2d_fwd (forward and data gradient), gv_conv2d_wgrad,
 * gv_pool2d_fwd/_bwd, gv_global_avg_pool, gv_view_score_partial and gv_view_pool_fuse_fwd take the storage type
 * from their descriptor / dtype argument. */
/* OR-ed into the `dtype` of the two *_sums_grouped_t calls (16-bit dtypes): `accum` is already zero (a training engine
 * keeps one accumulator per layer and zeroes them all with one fill per step instead of one memset per call). */
#define GV_ACCUM_ZEROED 0x100
int gv_bn_sums_grouped_t(const void* z, int32_t nb, int32_t hw, int32_t c, int32_t z_ld, int32_t num_groups,
                         double* accum, int32_t dtype, void* stream);
int gv_scale_shift_act_grouped_t(const void* x, int32_t nb, int32_t hw, int32_t c, int32_t x_ld, const float* scale,
                                 const float* shift, int32_t num_groups, int32_t relu, void* y, int32_t y_ld,
                                 int32_t dtype, void* stream);
/* gv_bn_finalize_grouped + gv_scale_shift_act_grouped_t as one call (one launch on 16-bit storage: every thread
 * derives its channels' scale/shift from the fp64 sums with gv_bn_finalize_grouped's arithmetic, one thread per
 * (group, channel) stores mean/var/inv/scale/shift for the backward pass and the moving averages). */
int gv_bn_finalize_apply_grouped_t(const double* accum, const int32_t* counts, const float* gamma, const float* beta,
                                   float eps, const void* x, int32_t nb, int32_t hw, int32_t c, int32_t x_ld,
                                   int32_t num_groups, int32_t relu, void* y, int32_t y_ld, float* mean, float* var,
                                   float* inv, float* scale, float* shift, int32_t dtype, void* stream);
/* Backward of y = relu(BN_train(z)).  The ReLU mask [y > 0] is read from y, or — y == NULL with scale/shift given (the
 * folded forward coefficients of gv_bn_finalize_grouped) — recomputed as [z*scale + shift > 0], which is the same
 * mask (the forward pass rounded that very value) without reading y at all; y == NULL and scale == NULL: no ReLU.
 * accumulate = 0 stores dz instead of adding to it (z has one consumer: no zero-fill, no read of dz). */
int gv_bn_relu_bwd_sums_grouped_t(const void* dy, int32_t dy_ld, const void* y, int32_t y_ld, const void* z,
                                  int32_t z_ld, const float* mean, const float* inv, int32_t nb, int32_t hw,
                                  int32_t c, int32_t num_groups, double* accum, const float* scale,
                                  const float* shift, int32_t dtype, void* stream);
int gv_bn_relu_bwd_apply_grouped_t(const void* dy, int32_t dy_ld, const void* y, int32_t y_ld, const void* z,
                                   int32_t z_ld, const float* mean, const float* inv, const float* gamma,
                                   const int32_t* counts, int32_t nb, int32_t hw, int32_t c, int32_t num_groups,
                                   const double* accum, void* dz, int32_t dz_ld, float* dbeta, float* dgamma,
                                   const float* scale, const float* shift, int32_t accumulate, int32_t dtype,
                                   void* stream);
/* OR-ed into the `dtype` of gv_bn_relu_bwd_apply_grouped_t: accum[g][c][1] holds sum g*z (the raw BatchNorm input, as
 * gv_conv2d_fwd_bnstats / GV_BN_STATS_BWD produces it) instead of sum g*zhat; the call converts it first:
 * sum g*zhat = inv * (sum g*z - mean * sum g). */
#define GV_ACCUM_RAW_Z 0x200
/* ---- train-mode BatchNorm sums folded into the launch that produces the tensor -------------------------------------
 * slim.batch_norm(is_training=True) (nets/inception_utils.py:52-62, nets/resnet_utils.py:230) normalises every view's
 * graph copy over its own values (nets/model.py:129-141): statistics per (view, channel), view of image b = b % groups.
 * gv_conv2d_fwd_bnstats is gv_conv2d_fwd (16-bit storage, one destination, no activation) whose epilogue also adds the
 * sums of the values it stores, exactly as stored, into fp64 accumulators [groups][c1-c0][2]:
 *   GV_BN_STATS_FWD  a forward convolution writing z:           { sum z, sum z^2 }   = what gv_bn_sums_grouped_t adds
 *   GV_BN_STATS_BWD  a data-gradient launch writing the FINAL dy of a tensor (its last or only contributor):
 *                    { sum g, sum g*z }, g = dy * [z*scale + shift > 0]; z = the BatchNorm's input, scale / shift
 *                    [groups][c1-c0] = its folded forward coefficients (NULL: no ReLU) — what
 *                    gv_bn_relu_bwd_sums_grouped_t adds, with z in place of zhat (GV_ACCUM_RAW_Z).
 * The output's channels may belong to several BatchNorm layers (members of a fused sibling GEMM; the concat a block's
 * data gradient writes): one segment each; acc == NULL: no sums for those columns.  Accumulators must be zero on entry
 * of a pass.  The sums are bitwise reproducible run to run (fixed-point partials, exact fp64 additions).
 * GV_E_UNSUPPORTED: this tile configuration / geometry cannot fold them (the caller runs the plain convolution and the
 * separate sums pass instead); nothing has been written in that case. */
#define GV_BN_STATS_FWD 1
#define GV_BN_STATS_BWD 2
#define GV_BN_STATS_MAX_SEG 8
typedef struct gv_bn_stats_seg {
    int32_t c0, c1;            /* output columns [c0, c1), multiples of 8 */
    int32_t z_ld, reserved;    /* BWD: pixel stride of z */
    const void* z;             /* BWD: BatchNorm input (storage type), channel c0 of the segment at z[pixel * z_ld] */
    const float* scale;        /* BWD: [groups][c1-c0] */
    const float* shift;
    double* acc;               /* [groups][c1-c0][2] */
} gv_bn_stats_seg;
typedef struct gv_bn_stats {
    int32_t mode, groups, nseg, reserved;
    gv_bn_stats_seg seg[GV_BN_STATS_MAX_SEG];
} gv_bn_stats;
int gv_conv2d_fwd_bnstats(const gv_conv_desc* d, const void* x, const void* w_packed, const float* scale,
                          const float* shift, const void* residual, void* y, const gv_bn_stats* stats, void* stream);
int gv_accumulate_t(const void* src, int32_t src_ld, void* dst, int32_t dst_ld, int64_t npix, int32_t c,
                    int32_t dtype, void* stream);
int gv_bias_grad_t(const void* dz, int32_t dz_ld, int64_t npix, int32_t c, double* accum, float* dbias,
                   int32_t dtype, void* stream);
/* gv_view_pool_fuse_bwd (per_shape = 0) / gv_view_pool_fuse_bwd_per_shape (per_shape = 1) with F, dF in `dtype`. */
int gv_view_pool_fuse_bwd_t(const void* F, const float* dS, int32_t num_views, int32_t num_shapes, int64_t E,
                            int64_t view_stride, int64_t shape_stride, const int32_t* scheme, int32_t num_groups,
                            const float* weight, int32_t mode, void* dF, int32_t per_shape, int32_t dtype,
                            void* stream);

/* ---- plan: the per-view backbone as one native launch sequence -------------
 * A plan is an ordered list of the ops above whose operands are (slot, element offset)
 * pairs into a caller-supplied table of device base pointers, so that one plan runs
 * on any set of buffers of the right size.  Building is host-only work; gv_plan_run
 * only launches (capturable).  Replaces the V unrolled copies of the backbone graph
 * that nets/model.py:129-141 builds, folded to one batch of N*V images. */
typedef struct gv_plan gv_plan;
int gv_plan_create(gv_plan** out);
void gv_plan_destroy(gv_plan* p);
int gv_plan_num_ops(const gv_plan* p);
int gv_plan_add_conv(gv_plan* p, const gv_conv_desc* d,
                     int32_t x_slot, int64_t x_off, int32_t w_slot, int64_t w_off,
                     int32_t ss_slot, int64_t scale_off, int64_t shift_off,
                     int32_t res_slot, int64_t res_off, int32_t y_slot, int64_t y_off,
                     int32_t y2_slot, int64_t y2_off, int64_t scale2_off, int64_t shift2_off);
/* Set gv_conv_desc.tile_cfg of conv op `op_index` (plan-time autotuning; speed only). */
int gv_plan_set_conv_tile(gv_plan* p, int32_t op_index, int32_t tile_cfg);
/* Conv op `op_index` runs as gv_conv2d_fwd_xpre: xscale / xshift at these fp32 offsets of the op's scale/shift slot. */
int gv_plan_set_conv_xpre(gv_plan* p, int32_t op_index, int64_t xscale_off, int64_t xshift_off);
/* gv_bottleneck_chain_fwd as a plan op.  Offsets into the weight slot are in `dtype` elements, into the scale/shift slot in
 * fp32 elements: conv3's filter / scale / shift, the pre-activation's scale / shift, conv1's filter / scale / shift.
 * GV_CHAIN_PROJ: res_slot = -1 (no shortcut operand), anything else GV_E_BADARG. */
int gv_plan_add_chain(gv_plan* p, const gv_chain_desc* d, int32_t x_slot, int64_t x_off, int32_t w_slot, int64_t w3_off,
                      int64_t w1_off, int32_t ss_slot, int64_t scale3_off, int64_t shift3_off, int64_t pre_scale_off,
                      int64_t pre_shift_off, int64_t scale1_off, int64_t shift1_off, int32_t res_slot, int64_t res_off,
                      int32_t y_slot, int64_t y_off, int32_t z_slot, int64_t z_off);
/* gv_bottleneck_unit_fwd as a plan op: gv_plan_add_chain's operands plus conv2's filter / scale / shift. */
int gv_plan_add_unit(gv_plan* p, const gv_unit_desc* d, int32_t x_slot, int64_t x_off, int32_t w_slot, int64_t w2_off,
                     int64_t w3_off, int64_t w1_off, int32_t ss_slot, int64_t scale2_off, int64_t shift2_off,
                     int64_t scale3_off, int64_t shift3_off, int64_t pre_scale_off, int64_t pre_shift_off,
                     int64_t scale1_off, int64_t shift1_off, int32_t res_slot, int64_t res_off, int32_t y_slot, int64_t y_off,
                     int32_t z_slot, int64_t z_off);
/* Branch-level concurrency: put op `op_index` on launch lane `lane` (0 = the caller's stream, 1..7 =
 * plan-owned streams) and name the EARLIER ops it must wait for (producers of its inputs, and ops
 * still using a buffer it overwrites).  A whole-plan run then forks the lanes off `stream` and joins
 * them back, so the independent branches of an Inception block (nets/inception_v3.py:139-155) overlap
 * and one kernel's tail is filled by another's workgroups.  Partial runs stay single-lane.  A plan
 * with lanes owns its streams/events: do not run it from two host threads at once. */
int gv_plan_set_schedule(gv_plan* p, int32_t op_index, int32_t lane, const int32_t* deps,
                         int32_t num_deps);
int gv_plan_add_pool(gv_plan* p, const gv_pool_desc* d, int32_t x_slot, int64_t x_off,
                     int32_t y_slot, int64_t y_off);
int gv_plan_add_scale_shift_act(gv_plan* p, int64_t npix, int32_t c, int32_t x_ld, int32_t y_ld,
                                int32_t relu, int32_t dtype, int32_t x_slot, int64_t x_off,
                                int32_t ss_slot, int64_t scale_off, int64_t shift_off,
                                int32_t y_slot, int64_t y_off);
/* buffers_host: host array of `num_slots` device base pointers. */
int gv_plan_run(const gv_plan* p, void* const* buffers_host, int32_t num_slots, void* stream);
/* Run ops [first, first+count) only (per-layer timing / profiling). */
int gv_plan_run_range(const gv_plan* p, int32_t first, int32_t count, void* const* buffers_host,
                      int32_t num_slots, void* stream);

/* ---- hipGraph capture ------------------------------------------------------
 * Small view batches are launch-bound (~90 launches for ~2 ms of work at 12 views): record everything enqueued on
 * `stream` between begin and end — gv_plan_run with its lane fork/join included, the grouping kernels, anything else
 * the caller launches there — into one executable graph and replay it with one call.  `stream` must not be the
 * legacy default stream.  The recorded launches keep the POINTERS they were issued with: replay on the same buffers. */
typedef struct gv_graph gv_graph;
int gv_capture_begin(void* stream);
int gv_capture_end(void* stream, gv_graph** out);
int gv_graph_launch(const gv_graph* g, void* stream);
void gv_graph_destroy(gv_graph* g);

/* ---- timing helper ---------------------------------------------------------
 * Average duration (ms) of `iters` back-to-back gv_conv2d_fwd launches measured with
 * hipEvents on `stream` (the stream the kernel is launched on); used by bench.py for the
 * roofline line.  Synchronises the stream. */
int gv_conv2d_time(const gv_conv_desc* d, const void* x, const void* w_packed, const float* scale,
                   const float* shift, void* y, int32_t iters, float* ms_avg_host, void* stream);
/* Same for a whole plan (or a range of it). */
int gv_plan_time(const gv_plan* p, int32_t first, int32_t count, void* const* buffers_host,
                 int32_t num_slots, int32_t iters, float* ms_avg_host, void* stream);
/* Every op timed IN SEQUENCE (the number bench.py's `roofline` object is built from): `iters` whole passes of the plan
 * on `stream` in plan order (single launch lane), an event behind every op; ms_per_op_host [gv_plan_num_ops()] = average
 * duration of each op where it sits in the step, behind its real predecessor (a launch timed as a warm repeat of itself
 * finds its filters and part of its input in L2). */
int gv_plan_time_each(const gv_plan* p, void* const* buffers_host, int32_t num_slots, int32_t iters,
                      float* ms_per_op_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVCNN_HIP_H */
