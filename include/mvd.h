/*
 * mvd.h — C ABI of libmvd_hip.so: the MI355X (gfx950) plane-sweep cost-volume engine that sits
 * behind the reference's model protocol (rmvd.create_model("robust_mvd") / "mvsnet_train").
 *
 * Every entry point replaces a composition of stock torch ops in the reference (the reference has
 * no native code); the file:line each one replaces is cited per function, relative to
 * the reference repository root.
 *
 * Conventions
 *   - all tensors fp32, contiguous, resident in device (HBM) memory; `const float* const*` arguments
 *     are HOST arrays of V device pointers (one per source view), V <= MVD_MAX_VIEWS;
 *   - calibration (intrinsics, poses, projection matrices, depth samples) is passed as DEVICE
 *     pointers too: the kernels derive their per-view coefficients themselves, so a call never
 *     synchronises with the host and can be captured into a hipGraph;
 *   - the caller owns every buffer (inputs, outputs, workspace); the library allocates nothing and
 *     keeps no pointer after the call returns; kernels are enqueued on `stream` (a hipStream_t;
 *     NULL = the default stream) of the CURRENT device and the call returns without waiting;
 *   - re-entrant, no global mutable state except a thread-local error string;
 *   - return value: 0 = MVD_OK, otherwise an mvd_status; mvd_last_error() describes the failure.
 */
#ifndef MVD_H_
#define MVD_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVD_VERSION 100 /* 0.1.0 */
#define MVD_MAX_VIEWS 32

typedef void* mvd_stream_t; /* hipStream_t */

typedef enum {
    MVD_OK = 0,
    MVD_ERR_INVALID_ARG = 1, /* NULL pointer, non-positive dimension, unsupported channel count ... */
    MVD_ERR_WORKSPACE = 2,   /* workspace NULL or smaller than the *_workspace_bytes() answer */
    MVD_ERR_LAUNCH = 3,      /* HIP reported an error when enqueueing (message has hipGetErrorString) */
    MVD_ERR_NO_DEVICE = 4    /* no gfx950 device visible */
} mvd_status;

/* layouts of a 5-D cost volume */
#define MVD_LAYOUT_NCDHW 0 /* (B, C, D, h, w): what the reference's homo_warp / CostRegNet use */
#define MVD_LAYOUT_NDHWC 1 /* (B, D, h, w, C): channel-last, what the engine uses between its own kernels */
/* OR into `out_layout` of mvd_warp_variance_f32: compute the sampling positions with the reference's own
 * operation chain (IEEE divisions, normalise then un-normalise), rounding for rounding, instead of the default
 * folded form ix = X * rcp(Z) * W/(W-1) - 0.5.  The default is within 1e-4 px of the chain; exact costs ~5 % (C = 32,
 * channel-last: only the locate phase of the tile kernel changes). */
#define MVD_GRID_EXACT 0x100
/* OR into `out_layout` of mvd_warp_variance_f32: key_feat and every src_feat are not (B,C,h,w) maps but already the
 * zero-bordered channel-last copies (B,h+3,w+3,C) the kernel gathers from (map at rows/cols 1..h / 1..w, zeros around),
 * as mvd_conv2d_bn_relu_f32 writes them with MVD_LAYOUT_NHWC_BORDER: the re-packing launches are skipped and the
 * workspace only has to hold the composed transforms (MVD_MAX_VIEWS*B*12 floats, rounded up to 256 bytes). */
#define MVD_FEAT_NHWC_BORDER 0x200

/* layouts of a 4-D feature map */
#define MVD_LAYOUT_NCHW 0        /* (B, C, h, w): the reference's */
#define MVD_LAYOUT_NHWC 1        /* (B, h, w, C): channel-last, between the engine's own 2-D layers */
#define MVD_LAYOUT_NHWC_BORDER 2 /* (B, h+3, w+3, C): channel-last with the map at (1,1) and zeros around: what K3 gathers from */

int mvd_version(void);
/* thread-local; valid until the next failing call on this thread */
const char* mvd_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Path A (robust_mvd): inverse-depth plane sweep with dot-product correlation
 * ---------------------------------------------------------------------------------------------- */

/* K1 — replaces PlanesweepCorrelation.forward for ALL source views in one call:
 *   EpipolarCoeffs.from_calib            rmvd/models/blocks/planesweep_corr.py:228-300
 *   us_from_ds / vs_from_ds (+non-finite replacement)                         :333-349
 *   visibility mask of get_plane_sweep_sampling_points                        :489-512
 *   TorchCorr.forward (all-pairs matmul, /sqrt(C), grid_sample lookup, masks) :152-195 with warp() :49-104
 *   correlate() loop over views                                               :514-521
 *
 *   feat_key   (N,C,h,w)              key-view features
 *   feat_src   V x (N,C,hs,ws)        source-view features
 *   K_key      (N,3,3)                relative intrinsics of the key view (fx,fy,cx,cy in [0,1])
 *   K_src      V x (N,3,3)            relative intrinsics of each source view
 *   T_src2key  V x (N,4,4)            source_to_key_transform (p_src = T p_key)
 *   invdepths  (N,S) if invdepth_batched else (1,S)   sampling inverse depths
 *   corr_out   V x (N,S,h,w)          mask * (1/sqrt(C)) * sum_c f_key * bilinear(f_src)
 *   mask_out   V x (N,S,h,w)          1.0 where all bilinear taps are in bounds (weight sum >= 0.9999)
 *                                     and the plane is in front of both cameras, else 0.0
 * C must be a multiple of 64 (256 in robust_mvd). */
size_t mvd_sweep_corr_workspace_bytes(int N, int C, int h, int w, int hs, int ws, int V);
int mvd_sweep_corr_f32(const float* feat_key, const float* const* feat_src, const float* K_key,
                       const float* const* K_src, const float* const* T_src2key, const float* invdepths,
                       int invdepth_batched, int N, int C, int h, int w, int hs, int ws, int S, int V,
                       float* const* corr_out, float* const* mask_out, void* workspace, size_t workspace_bytes,
                       mvd_stream_t stream);

/* K1 with the block's other options (planesweep_corr.py:371-394, 465-487): sampling inverse depths shared (1,S), per batch
 * element (N,S) or PER KEY PIXEL (N,S,h,w); `corr_scale` multiplies the dot products: 1/sqrt(C) for normalize="dim" (what
 * mvd_sweep_corr_f32 uses), 1 for normalize=False / "before" (the caller normalises the features beforehand). */
#define MVD_INVDEPTH_SHARED 0
#define MVD_INVDEPTH_BATCHED 1
#define MVD_INVDEPTH_PER_PIXEL 2
int mvd_sweep_corr_ex_f32(const float* feat_key, const float* const* feat_src, const float* K_key,
                          const float* const* K_src, const float* const* T_src2key, const float* invdepths,
                          int invdepth_mode, float corr_scale, int N, int C, int h, int w, int hs, int ws, int S, int V,
                          float* const* corr_out, float* const* mask_out, void* workspace, size_t workspace_bytes,
                          mvd_stream_t stream);
/* K1 on the layouts the kernel works in, without the re-packing launches: feat_key (N,h,w,C) channel-last, feat_src[v] zero-bordered
 * channel-last (N,hs+3,ws+3,C) with the map at rows/columns 1.. (what mvd_conv2d_split_f32 writes with its row/image strides),
 * outputs pixel-major: corr_out[v][(n h w + pixel) * out_pixel_stride + s] (and mask_out alike), i.e. (N,h,w,S) maps that the
 * 2-D convolutions behind the sweep read as S channels.  No workspace.  corr_absmax: NULL, or a device float that receives
 * max |corr| over all views by atomic maximum (the caller zeroes it; C <= 256). */
int mvd_sweep_corr_nhwc_f32(const float* feat_key, const float* const* feat_src, const float* K_key, const float* const* K_src,
                            const float* const* T_src2key, const float* invdepths, int invdepth_mode, float corr_scale, int N, int C,
                            int h, int w, int hs, int ws, int S, int V, float* const* corr_out, float* const* mask_out,
                            int out_pixel_stride, float* corr_absmax, mvd_stream_t stream);

/* The sweep of PlanesweepCorrelation(warp_only=True) — replaces WarpOnlyCorr.forward + warp_multi
 *   rmvd/models/blocks/planesweep_corr.py:107-140, 13-45 (reached through correlate(), :514-521):
 * the source features sampled at the S sweep positions of every key pixel (same grids as K1, :228-349, 489-512), times the
 * SAMPLING mask ([sum of in-bounds tap weights >= 0.9999], :96-102; WarpOnlyCorr ignores the visibility mask it is handed).
 * feat_src[v] (N,C,hs,ws); warped_out[v] (N,S,C,h,w); mask_out[v] (N,S,h,w).  normalize_after != 0: the warped features are
 * L2-normalised along C, x / (|x| + 1e-9) (:8-10, 135-136), before the mask is applied.  invdepth_mode as in
 * mvd_sweep_corr_ex_f32.  No workspace. */
int mvd_sweep_warp_f32(const float* const* feat_src, const float* K_key, const float* const* K_src,
                       const float* const* T_src2key, const float* invdepths, int invdepth_mode, int normalize_after, int N,
                       int C, int h, int w, int hs, int ws, int S, int V, float* const* warped_out, float* const* mask_out,
                       mvd_stream_t stream);

/* K2 — replaces the view-weighting arithmetic of LearnedFusion.forward
 *   rmvd/models/blocks/learned_fusion.py:32-48 (softmax over views + 1e-9, mask-weighted mean, fused mask).
 * The per-view score maps (conv3x3+ReLU+conv1x1, :13-17,:28-30) are 2-D convolutions that stay on
 * MIOpen and are passed in.  V == 1 is the caller's pass-through (:50-52) and is rejected here.
 *   corr, mask  V x (N,S,h,w);  score  V x (N,1,h,w);  fused, fused_mask  (N,S,h,w) */
int mvd_fuse_views_f32(const float* const* corr, const float* const* mask, const float* const* score, int N, int S,
                       int h, int w, int V, float* fused, float* fused_mask, mvd_stream_t stream);
/* K2 on pixel-major volumes (N,h,w,S) with pixels in_pixel_stride floats apart (mvd_sweep_corr_nhwc_f32's outputs); score[v]
 * (N,1,h,w).  fused: channel slice of a channel-last buffer (pixels out_pixel_stride floats apart); fused_mask NULL or the same
 * layout; fused_absmax NULL or a device float receiving max |fused| by atomic maximum (the caller zeroes it). */
int mvd_fuse_views_nhwc_f32(const float* const* corr, const float* const* mask, const float* const* score, int N, int S, int h,
                            int w, int V, int in_pixel_stride, float* fused, float* fused_mask, int out_pixel_stride,
                            float* fused_absmax, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Path B (mvsnet): fronto-parallel homography warp, variance aggregation, 3-D regulariser, soft argmin
 * ---------------------------------------------------------------------------------------------- */

/* K3 — replaces the cost-volume construction of MVSNet.forward:
 *   homo_warp for every source view                rmvd/models/blocks/utils.py:222-268
 *   key volume repeat + sum / sum-of-squares loop  rmvd/models/mvsnet.py:124-133
 *   variance                                       rmvd/models/mvsnet.py:135
 *
 *   key_feat      (B,C,h,w)
 *   src_feat      V x (B,C,h,w)
 *   src_proj      V x (B,4,4)      source projection matrices (mvsnet.py:76-88)
 *   key_proj_inv  (B,4,4)          inverse key projection (mvsnet.py:85-86)
 *   depth_values  (B,D)
 *   var_out       (B,C,D,h,w) for MVD_LAYOUT_NCDHW or (B,D,h,w,C) for MVD_LAYOUT_NDHWC
 * C must be a multiple of 4 and <= 64 (32 in MVSNet).  Algorithmic HBM bytes: 4*((V+1)*C*h*w + C*D*h*w)*B. */
size_t mvd_warp_variance_workspace_bytes(int B, int C, int h, int w, int V);
int mvd_warp_variance_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                          const float* key_proj_inv, const float* depth_values, int B, int C, int D, int h, int w,
                          int V, float* var_out, int out_layout, void* workspace, size_t workspace_bytes,
                          mvd_stream_t stream);
/* The same, and max |var_out| over the whole volume into *absmax_out (device, one float): what
 * mvd_conv3d_bn_relu_f32_split scales its activations by.  A by-product of the kernel's store epilogue for C = 32 /
 * MVD_LAYOUT_NDHWC (no extra pass over the volume), a separate streaming read otherwise. */
int mvd_warp_variance_absmax_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                                 const float* key_proj_inv, const float* depth_values, int B, int C, int D, int h, int w,
                                 int V, float* var_out, float* absmax_out, int out_layout, void* workspace,
                                 size_t workspace_bytes, mvd_stream_t stream);

/* K3, fp16-feature variant (BASELINE.json configs[3]: "fp16 features"; SURVEY.md 8b names mvd_warp_variance_{f32,f16}).
 * Same operation as mvd_warp_variance_f32 with MVD_FEAT_NHWC_BORDER | MVD_LAYOUT_NDHWC, C = 32:
 *   key_feat, src_feat[v]   fp16 zero-bordered channel-last maps (B,h+3,w+3,32) (map at rows/cols 1..h / 1..w, zeros around)
 *   var_out                 fp16 channel-last volume (B,D,h,w,32)
 * Sampling positions, bilinear weights, the blend and the variance are computed in fp32 exactly as in the f32 entry point
 * (the fp16 taps enter the same fmaf chain): the result equals the f32 kernel's on the same fp16-representable feature
 * values, rounded once (to nearest even) to fp16 on the way out.  Calibration stays fp32.
 * Algorithmic HBM bytes: 2*((V+1)*C*h*w + C*D*h*w)*B — the volume is stored fp16 (1,137.5 MB at configs[3]).
 * Map size: h, w <= 65532 and h*w*64 < 2^31 (the range of the one kernel behind this entry point); larger maps return
 * MVD_ERR_INVALID_ARG (mvd_warp_variance_f32 runs longer maps on another kernel). */
size_t mvd_warp_variance_f16_workspace_bytes(int B);
int mvd_warp_variance_f16(const void* key_feat, const void* const* src_feat, const float* const* src_proj,
                          const float* key_proj_inv, const float* depth_values, int B, int D, int h, int w, int V,
                          void* var_out, void* workspace, size_t workspace_bytes, mvd_stream_t stream);
/* elementwise fp32 <-> fp16 (round to nearest even); n must be a multiple of 4.
 * Range of the fp16-feature variant (this converter, mvd_warp_variance_f16, mvd_conv3d_bn_relu_f16in): plain IEEE fp16, no
 * scaling — |x| > 65504 becomes +-inf, |x| < 6.1e-5 loses precision (subnormal), |x| < 3e-8 becomes 0; inf / NaN propagate.
 * FeatureNet's last convolution has no normalisation, so the magnitude of the features (and of their variance, which is
 * stored in fp16 too) depends on the checkpoint: the variant is for feature magnitudes of O(1), as with BASELINE.json
 * configs[3]'s weights; the fp32 path (range-scaled split first layer) has no such limit. */
int mvd_convert_f32_to_f16(const float* src, void* dst, long long n, mvd_stream_t stream);
int mvd_convert_f16_to_f32(const void* src, float* dst, long long n, mvd_stream_t stream);

/* homo_warp alone (one view, no aggregation): rmvd/models/blocks/utils.py:222-268 -> (B,C,D,h,w). */
int mvd_homo_warp_f32(const float* src_feat, const float* src_proj, const float* key_proj_inv,
                      const float* depth_values, int B, int C, int D, int h, int w, float* warped_out,
                      void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* K4 — one layer of CostRegNet (rmvd/models/blocks/mvsnet_components.py:69-123) as an implicit GEMM
 * on the fp32 matrix cores: 3x3x3 Conv3d (stride 1 or 2, padding 1; ConvBnReLU3D :25-41) or
 * ConvTranspose3d (stride 2, padding 1, output_padding 1; :84-109), followed by a per-channel affine
 * (eval-mode BatchNorm folded to scale/shift, or scale=1 / shift=bias for `prob`), optional ReLU and
 * optional skip addition AFTER the ReLU (the `conv4 + conv7(x)` form of :116-121).
 * Activations are channel-last (B,D,h,w,C).  Weights must first be packed with mvd_pack_conv3d_weights_f32. */
#define MVD_CONV3D_STRIDE1 0
#define MVD_CONV3D_STRIDE2 1
#define MVD_DECONV3D_STRIDE2 2
size_t mvd_conv3d_packed_weight_floats(int Cin, int Cout);
/* w: Conv3d layout (Cout,Cin,3,3,3), or ConvTranspose3d layout (Cin,Cout,3,3,3) when mode == MVD_DECONV3D_STRIDE2 */
int mvd_pack_conv3d_weights_f32(const float* w, int Cin, int Cout, int mode, float* packed, mvd_stream_t stream);
/* x (B,Di,hi,wi,Cin) -> y (B,Do,ho,wo,Cout); Do = Di (stride 1), Di/2 (stride 2; Di,hi,wi even), 2*Di (deconv).
 * scale, shift (Cout); skip NULL or (B,Do,ho,wo,Cout).  Cin in {8,16,32,64}; Cout in {1,8,16,32,64}.
 * Also Cin = 1 with MVD_CONV3D_STRIDE1 and Cout a multiple of 4 up to 64 (the adjoint of `prob` in training, below): a vector
 * kernel over the one-channel volume. */
int mvd_conv3d_bn_relu_f32(const float* x, const float* packed_w, const float* scale, const float* shift,
                           const float* skip, float* y, int B, int Di, int hi, int wi, int Cin, int Cout, int mode,
                           int relu, mvd_stream_t stream);
/* The same, and max |y| over the finite outputs into *absmax_out (device, one float): what mvd_conv3d_bn_relu_f32_split scales
 * the activations of a following layer by.  A by-product of the store epilogue of the stride-2 layers (the regulariser's conv1
 * and conv3, whose outputs its split-operand conv2 and conv4 consume); after any other mode a pass over y (mvd_absmax_f32). */
int mvd_conv3d_bn_relu_absmax_f32(const float* x, const float* packed_w, const float* scale, const float* shift,
                                  const float* skip, float* y, float* absmax_out, int B, int Di, int hi, int wi, int Cin,
                                  int Cout, int mode, int relu, mvd_stream_t stream);

/* K4 for training — the backward of one CostRegNet layer, i.e. what autograd runs for
 *   rmvd/models/blocks/mvsnet_components.py:25-41,69-123 when rmvd/train/multi_view_depth_training.py:231-246 calls backward().
 * Data gradient: no entry point of its own.  Each layer's adjoint is a layer mvd_conv3d_bn_relu_f32 runs (scale 1, shift 0, no
 * ReLU): stride-1 conv W -> stride-1 conv with W flipped along the taps and its channel axes swapped; stride-2 conv W ->
 * MVD_DECONV3D_STRIDE2 with W as it is (in = Cout, out = Cin); transposed conv W -> MVD_CONV3D_STRIDE2 with W as it is.
 * Weight gradient: mvd_conv3d_weight_grad_f32.  x (B,Di,hi,wi,Cin) the layer's input, gy (B,Do,ho,wo,Cout) the gradient of its
 * output (sizes as for mvd_conv3d_bn_relu_f32; Di,hi,wi even for MVD_CONV3D_STRIDE2), both channel-last;
 *   gw (Cout,Cin,3,3,3)[co,ci,k] = sum_{b,o} gy[b,o,co] * xpad[b, s*o + k, ci]          (conv, stride s, xpad = x padded by 1)
 *   gw (Cin,Cout,3,3,3)[ci,co,k] = sum_{b,i} x[b,i,ci] * gypad[b, 2*i + k, co]          (MVD_DECONV3D_STRIDE2)
 * i.e. the layer's own torch weight layout.  Cin, Cout in 1..64; any positive sizes.  fp32 MFMA: exact products, fp32 sums.
 * DETERMINISTIC: no atomics; every workgroup writes one partial gradient to the workspace and a second kernel adds the
 * partials in a fixed order, so two calls on the same inputs give bit-identical gw.  gw is written, not accumulated.
 * The measurement hook (mvd_arm_kernel_timing) brackets the two kernels. */
size_t mvd_conv3d_weight_grad_workspace_bytes(int B, int Di, int hi, int wi, int Cin, int Cout, int mode);
/* One field of the launch plan mvd_conv3d_weight_grad_f32 follows for these arguments, from the same planning code as the launch
 * (for tests and tools that must know which path a size takes; the values are a tuning matter and may change between versions).
 * A workgroup marches over DZ depth planes of the tiled tensor per work item; `items` work items are walked by PARTIALS
 * workgroups per channel block (items > PARTIALS: a workgroup takes several items and keeps summing); the kernel instantiation
 * is <COT, CIT, S> (16-channel tiles per 32-channel block on the tiled and on the haloed side, stride of the taps) and
 * CS_BLOCKS x CG_BLOCKS channel blocks.  0 for unsupported arguments (where the workspace size is 0) or an unknown field. */
#define MVD_WGRAD_PLAN_DZ 0
#define MVD_WGRAD_PLAN_ITEMS 1
#define MVD_WGRAD_PLAN_PARTIALS 2
#define MVD_WGRAD_PLAN_COT 3
#define MVD_WGRAD_PLAN_CIT 4
#define MVD_WGRAD_PLAN_S 5
#define MVD_WGRAD_PLAN_CS_BLOCKS 6
#define MVD_WGRAD_PLAN_CG_BLOCKS 7
size_t mvd_conv3d_weight_grad_plan_field(int B, int Di, int hi, int wi, int Cin, int Cout, int mode, int field);
int mvd_conv3d_weight_grad_f32(const float* x, const float* gy, float* gw, int B, int Di, int hi, int wi, int Cin, int Cout,
                               int mode, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* K4, fp16-input first layer (BASELINE.json configs[3]: "3D-conv regulariser on MFMA, fp16 features"): conv0 of
 * CostRegNet (mvsnet_components.py:78; ConvBnReLU3D 32 -> 8, 3x3x3, stride 1, padding 1, :25-41) on
 * v_mfma_f32_16x16x32_f16 — fp16 operands (the volume of mvd_warp_variance_f16 and the weights rounded to fp16),
 * fp32 accumulation, fp32 BN scale/shift + ReLU epilogue, fp32 output that feeds mvd_conv3d_bn_relu_f32 layers.
 *   x (B,D,h,w,32) fp16 channel-last -> y (B,D,h,w,8) fp32 channel-last.  Only Cin = 32, Cout = 8 is built. */
size_t mvd_conv3d_f16_packed_weight_bytes(int Cin, int Cout);
/* w: Conv3d layout (Cout,Cin,3,3,3) fp32; rounded to fp16 and laid out in MFMA fragment order */
int mvd_pack_conv3d_weights_f16(const float* w, int Cin, int Cout, void* packed, mvd_stream_t stream);
int mvd_conv3d_bn_relu_f16in(const void* x, const void* packed_w, const float* scale, const float* shift, float* y, int B,
                             int D, int h, int w, int Cin, int Cout, int relu, mvd_stream_t stream);

/* K4 first layer, split-operand form (what the model uses by default; mvd_conv3d_bn_relu_f32 on fp32 MFMA is the other
 * form): fp32 input and fp32 weights, each split exactly into two fp16 terms (a = a_hi + 2^-11 a_lo), products
 * a_hi w_hi + 2^-11 (a_hi w_lo + a_lo w_hi) on v_mfma_f32_16x16x32_f16 with fp32 accumulation; the dropped term is
 * 2^-22 a_lo w_lo, i.e. relative error per product <= ~3 * 2^-22 against fp32's own 2^-24, and one accumulator rounding per
 * 32 products instead of per product: the result is at least as close to the exact convolution as the fp32-MFMA kernel's
 * (tests/test_hip_f16.py measures both against a float64 oracle).
 * Range: both operands are scaled by exact powers of two before the split and the result is scaled back, so inputs of any
 * uniform magnitude (1e-30 .. 1e30, denormals included) keep that accuracy.  The activations' scale comes from
 * `x_absmax`, a DEVICE pointer to one float holding max |x| over the whole input (mvd_absmax_f32, or the by-product of
 * mvd_warp_variance_absmax_f32); any upper bound is safe, a tight one most precise: a value v is represented to
 * |error| <= max(2^-22 |v|, 2^-50 max|x|).  inf / NaN inputs give inf / NaN outputs where they reach, as on fp32.
 * x (B,D,h,w,Cin) fp32 -> y (B,D,h,w,Cout) fp32; Cin = 16 or 32, Cout = 8, 16, ... 64 (a workgroup computes 8 output channels
 * of its tile; the regulariser's conv0 (32 -> 8), conv2 (16 -> 16) and conv4 (32 -> 32) use it).  With 16 input channels a
 * 64-byte MFMA fragment spans two x-adjacent voxels: the kw taps go in pairs (0,1), (2, zero weights). */
size_t mvd_conv3d_split_packed_weight_bytes(int Cin, int Cout);
int mvd_pack_conv3d_weights_split(const float* w, int Cin, int Cout, void* packed, mvd_stream_t stream);
int mvd_conv3d_bn_relu_f32_split(const float* x, const float* x_absmax, const void* packed_w, const float* scale, const float* shift,
                                 float* y, int B, int D, int h, int w, int Cin, int Cout, int relu, mvd_stream_t stream);
/* The same, and max |y| over the finite outputs into *y_absmax (device, one float): a by-product of the store epilogue. */
int mvd_conv3d_bn_relu_absmax_f32_split(const float* x, const float* x_absmax, const void* packed_w, const float* scale, const float* shift,
                                        float* y, float* y_absmax, int B, int D, int h, int w, int Cin, int Cout, int relu,
                                        mvd_stream_t stream);
/* K4's stride-2 and transposed layers (and stride-1 layers with many channels) on the split-operand implicit-GEMM kernel of the
 * 2-D engine (csrc/conv2d_split.hip: the depth taps are extra chunks of the reduction; a transposed 3x3x3 stride-2 layer runs as a
 * 2x2x2 convolution with 8 Cout output channels = (parity class, channel)).  x (B,Di,Hi,Wi,Cin) channel-last fp32, Cin a multiple of 8
 * (16 for the transposed form), Cout a multiple of 4; mode MVD_CONV3D_STRIDE1 / _STRIDE2 / MVD_DECONV3D_STRIDE2 with the output
 * sizes of mvd_conv3d_bn_relu_f32; weights in Conv3d / ConvTranspose3d layout.  y = relu?(conv * scale + shift) (+ skip, laid out
 * like y, may be NULL).  x_absmax as for mvd_conv3d_bn_relu_f32_split; y_absmax NULL or a device float that is RAISED to max |y|
 * (atomic maximum: the caller zeroes it, as for mvd_conv2d_split_f32).  workspace NULL or mvd_conv3d_igemm_workspace_bytes bytes (few-voxel layers split the reduction). */
size_t mvd_conv3d_igemm_packed_weight_bytes(int Cin, int Cout, int mode);
int mvd_pack_conv3d_weights_igemm(const float* w, int Cin, int Cout, int mode, void* packed, mvd_stream_t stream);
size_t mvd_conv3d_igemm_workspace_bytes(int B, int Di, int Hi, int Wi, int Cin, int Cout, int mode);
int mvd_conv3d_bn_relu_igemm_f32(const float* x, const float* x_absmax, const void* packed_w, const float* scale, const float* shift,
                                 const float* skip, float* y, float* y_absmax, int B, int Di, int Hi, int Wi, int Cin, int Cout, int mode,
                                 int relu, void* workspace, size_t workspace_bytes, mvd_stream_t stream);
/* K4's transposed layers on a kernel of their own (csrc/deconv3d_split.hip): ConvTranspose3d 3x3x3, stride 2, padding 1,
 * output_padding 1 with split operands as above (each fp32 value two fp16 terms after an exact power-of-two scaling, products
 * w_hi a_hi + w_lo a_hi + w_hi a_lo on v_mfma_f32_16x16x32_f16 into one fp32 accumulator), in the decomposition of the fp32 kernel: a
 * workgroup stages 2 input planes x 5 rows once and writes all eight output parity classes, so no product is a structural zero.
 * w: ConvTranspose3d layout (Cin, Cout, 3, 3, 3).  Cin = 32 or 64 with Cout = 16, 32, 48 or 64, and 16 -> 8; the packed size is 0 for
 * any other pair.  x (B,Di,hi,wi,Cin) channel-last fp32 -> y (B,2Di,2hi,2wi,Cout); y = relu?(deconv * scale + shift) (+ skip, laid
 * out like y, may be NULL).  x_absmax: DEVICE pointer to one float with max |x| over the whole input (any upper bound is safe); a
 * value v is represented to |error| <= max(2^-22 |v|, 2^-39 max|x|).  y_absmax: NULL, or a device float that is RAISED to max |y|
 * over the finite outputs, after the skip addition (one atomic maximum per workgroup: the caller zeroes it); the output is bit-identical
 * either way.  inf / NaN inputs give inf / NaN outputs where they reach.  16 -> 8: the two w-parities of an output column pair share
 * one MFMA (as in the fp32 kernel of that layer), so a non-finite input column c + 1 also reaches output column 2c. */
size_t mvd_deconv3d_split_packed_weight_bytes(int Cin, int Cout);
int mvd_pack_deconv3d_weights_split(const float* w, int Cin, int Cout, void* packed, mvd_stream_t stream);
int mvd_deconv3d_bn_relu_f32_split(const float* x, const float* x_absmax, const void* packed_w, const float* scale, const float* shift,
                                   const float* skip, float* y, float* y_absmax, int B, int Di, int hi, int wi, int Cin, int Cout, int relu,
                                   mvd_stream_t stream);
/* ---- Path A's 2-D CNN: split-operand implicit-GEMM convolutions ------------------------------------------------------------
 * Replace torch.nn.functional.conv2d / conv_transpose2d + bias + LeakyReLU (+ torch.cat of the inputs) of the DispNet blocks of
 * robust_mvd (rmvd/models/blocks/dispnet_encoder.py:6-27, dispnet_context_encoder.py, learned_fusion.py:8-20,
 * dispnet_costvolume_encoder.py:7-50, dispnet_decoder.py:36-138).  fp32 in, fp32 out; inside, both operands are split into two
 * fp16 terms (block-scaled by exact powers of two) and multiplied on fp16 MFMA with fp32 accumulation: fp32-grade results
 * (csrc/conv2d_split.hip states the bound).
 * Activations are NHWC with a free pixel stride: x points at the first channel of a slice of Cin_pad channels (a multiple of 8;
 * channels Cin .. Cin_pad-1 must hold zeros) inside pixels `x_pixel_stride` floats apart, y likewise for Cout channels, so that
 * layers read and write slices of the decoder's concat buffers directly.  x, y 16-byte aligned, strides multiples of 4.
 * mode MVD_CONV2D: Conv2d, padding k/2: 1x1 (Cin_pad % 32 == 0), 3x3 stride 1, 3x3 stride 2, 5x5 stride 2; weights (Cout,Cin,k,k).
 * mode MVD_DECONV2D: ConvTranspose2d 4x4, stride 2, padding 1 (Cin_pad % 32 == 0); weights (Cin,Cout,4,4); output 2Hi x 2Wi.
 * mode MVD_CONV2D_IMAGE: Conv2d 7x7 stride 2 padding 3 on a PLANAR (B,3,Hi,Wi) image (Cin = 3, Cin_pad = 8, stride argument unused).
 * x_absmax: device float, max |x| over the input tensor (an upper bound is safe); y_absmax: NULL, or a device float that
 * receives max |y| by atomic maximum (the caller zeroes it; several layers may share one to cover a concat buffer).
 * act: 0 none, 1 LeakyReLU(slope), 2 ReLU; bias NULL or (Cout).  workspace: NULL, or mvd_conv2d_split_workspace_bytes bytes:
 * lets layers with few pixels and many weights split the reduction over workgroups (partial sums added in a fixed order).
 * Output strides (floats): y_pixel_stride between pixels; y_row_stride / y_image_stride between rows / images (0 = dense: a layer
 * may write the interior of a zero-bordered map, which is what mvd_sweep_corr_nhwc_f32 reads); y_channel_stride between channels
 * (0 or 1 = channel-last; with y_pixel_stride = 1 and y_channel_stride = Ho Wo the output is planar (B,Cout,Ho,Wo)). */
#define MVD_CONV2D 0
#define MVD_DECONV2D 1
#define MVD_CONV2D_IMAGE 2
size_t mvd_conv2d_split_packed_weight_bytes(int Cin_pad, int Cout, int KH, int KW, int stride, int mode);
int mvd_pack_conv2d_weights_split(const float* w, int Cin, int Cin_pad, int Cout, int KH, int KW, int stride, int mode, void* packed,
                                  mvd_stream_t stream);
size_t mvd_conv2d_split_workspace_bytes(int B, int Hi, int Wi, int Cin_pad, int Cout, int KH, int KW, int stride, int mode);
int mvd_conv2d_split_f32(const float* x, const float* x_absmax, const void* packed_w, const float* bias, float* y, float* y_absmax, int B,
                         int Hi, int Wi, int Cin_pad, int x_pixel_stride, int Cout, int y_pixel_stride, long long y_row_stride,
                         long long y_image_stride, long long y_channel_stride, int KH, int KW, int stride, int mode, int act, float slope,
                         void* workspace, size_t workspace_bytes, mvd_stream_t stream);
/* F.interpolate(x, size=(2h,2w), mode="bilinear", align_corners=False) of a planar (B,C,h,w) map (the decoder's up-sampled
 * prediction, dispnet_decoder.py:131), written as C channels of a channel-last slice y (pixels y_pixel_stride floats apart);
 * torch's formula and operation order.  y_absmax as above (NULL or atomic maximum). */
int mvd_upsample2x_nhwc_f32(const float* x, float* y, float* y_absmax, int B, int C, int h, int w, int y_pixel_stride, mvd_stream_t stream);
/* max |x[i]| over the FINITE values of n floats (inf and NaN left out, 0 if there is none) into *absmax (device, one
 * float); a streaming read */
int mvd_absmax_f32(const float* x, long long n, float* absmax, mvd_stream_t stream);

/* K6 — one layer of MVSNet's FeatureNet (rmvd/models/blocks/mvsnet_components.py:44-66; ConvBnReLU :8-22) as an
 * implicit GEMM on the fp32 matrix cores: Conv2d k x k with padding k/2 (k = 3 stride 1, or k = 5 stride 2), then a
 * per-channel affine (eval-mode BatchNorm2d folded to scale/shift; scale = 1, shift = bias for the final `feature`
 * conv) and optional ReLU, in one pass.  Weights must first be packed with mvd_pack_conv2d_weights_f32.
 *   x   in_layout MVD_LAYOUT_NCHW: (B,3,hi,wi) — the normalised image, Cin must be 3
 *       in_layout MVD_LAYOUT_NHWC: (B,hi,wi,Cin), Cin in {8,16,32}
 *   y   out_layout MVD_LAYOUT_NHWC: (B,ho,wo,Cout);  MVD_LAYOUT_NCHW: (B,Cout,ho,wo) (the reference's layout);
 *       MVD_LAYOUT_NHWC_BORDER: (B,ho+3,wo+3,Cout) with the map at rows/cols 1..ho/1..wo — the zero-bordered layout
 *       K3 gathers from (mvd_warp_variance_f32 with MVD_FEAT_NHWC_BORDER); the caller zeroes the buffer once, the
 *       kernel writes only the interior.
 *   ho = (hi-1)/stride + 1, wo likewise; Cout in {8,16,32}; scale, shift (Cout). */
size_t mvd_conv2d_packed_weight_floats(int Cin, int Cout, int ksize);
/* w: Conv2d layout (Cout,Cin,k,k) */
int mvd_pack_conv2d_weights_f32(const float* w, int Cin, int Cout, int ksize, float* packed, mvd_stream_t stream);
int mvd_conv2d_bn_relu_f32(const float* x, int in_layout, const float* packed_w, const float* scale, const float* shift,
                           float* y, int out_layout, int B, int hi, int wi, int Cin, int Cout, int ksize, int stride,
                           int relu, mvd_stream_t stream);
/* The same, and *y_absmax (device, one float; the caller zeroes it) RAISED to max |y| over the finite outputs: what a split-operand
 * layer behind this one (mvd_conv2d_split_f32) scales its activations by.  A by-product of the store epilogue. */
int mvd_conv2d_bn_relu_absmax_f32(const float* x, int in_layout, const float* packed_w, const float* scale, const float* shift,
                                  float* y, float* y_absmax, int out_layout, int B, int hi, int wi, int Cin, int Cout, int ksize,
                                  int stride, int relu, mvd_stream_t stream);

/* FeatureNet's two full-resolution layers in one pass — replaces conv0 -> conv1 of FeatureNet
 *   rmvd/models/blocks/mvsnet_components.py:47-48 (ConvBnReLU(3,8,3,1,1), ConvBnReLU(8,8,3,1,1)), BN folded as above.
 *   image (B,3,H,W); w0 (3,3,3,8) and w1 (3,3,8,8): the Conv2d weights permuted to [ky][kx][cin][cout]; scale*, shift* (8);
 *   y (B,H,W,8) channel-last.  The 8-channel intermediate stays in LDS (the two launches write and read it once each).
 *   All pointers except image 16-byte aligned.
 *   tile_absmax (optional, mvd_conv2d_head_tile_count(B,H,W) floats): max |y| over the finite outputs of each workgroup's tile,
 *   written with plain stores — mvd_absmax_f32 over that array is max |y| of the layer (what the split-operand layer behind it
 *   scales by) at the cost of a 35 KB pass instead of one over y. */
size_t mvd_conv2d_head_tile_count(int B, int H, int W);
int mvd_conv2d_head_f32(const float* image, const float* w0, const float* scale0, const float* shift0, const float* w1,
                        const float* scale1, const float* shift1, float* y, float* tile_absmax, int B, int H, int W,
                        mvd_stream_t stream);
/* The same pair with conv1 on the fp16 matrix instruction: conv0 as above (fp32, vector ALU), its outputs kept in LDS as two fp16
 *   terms under a per-tile power-of-two scale (max |conv0| over the finite values of the workgroup's patch), conv1's weights as two
 *   fp16 terms under a per-channel power of two, fp32 accumulation: fp32-grade for inputs of any uniform magnitude.
 *   w1 (8,8,3,3): conv1's Conv2d weight as it is; mvd_pack_conv2d_head_split_weights packs it once per model into
 *   mvd_conv2d_head_split_packed_bytes() bytes (16-byte aligned).  Everything else as mvd_conv2d_head_f32. */
size_t mvd_conv2d_head_split_packed_bytes(void);
int mvd_pack_conv2d_head_split_weights(const float* w1, void* packed, mvd_stream_t stream);
int mvd_conv2d_head_split_f32(const float* image, const float* w0, const float* scale0, const float* shift0, const void* w1_packed,
                              const float* scale1, const float* shift1, float* y, float* tile_absmax, int B, int H, int W,
                              mvd_stream_t stream);

/* K5 — replaces F.softmax + depth_regression + the 4-bin confidence of MVSNet.forward
 *   rmvd/models/mvsnet.py:139-160, rmvd/models/blocks/utils.py:271-274.
 *   cost (B,D,h,w) raw regulariser output; depth_values (B,D);
 *   depth_out (B,h,w) = sum_d softmax(cost)_d * depth_d
 *   conf_out  (B,h,w) = sum_{j=idx-1..idx+2, 0<=j<D} softmax(cost)_j, idx = trunc(sum_d p_d * d)
 * (the reference returns uncertainty = 1 - conf). conf_out may be NULL. */
int mvd_softmax_regress_f32(const float* cost, const float* depth_values, int B, int D, int h, int w,
                            float* depth_out, float* conf_out, mvd_stream_t stream);

/* K5 for training — the forward of MVSNet.forward's soft argmin with autograd recording (rmvd/models/mvsnet.py:139-141,
 * rmvd/models/blocks/utils.py:271-274).
 * mvd_softmax_regress_stats_f32: depth_out and conf_out bit-identical to mvd_softmax_regress_f32's (same kernel body); also
 *   stats_out (B,2,h,w): plane 0 = M = max_d cost, plane 1 = 1 / sum_d exp(cost_d - M).  conf_out may be NULL.
 * mvd_softmax_regress_backward_f32: VJP w.r.t. the cost volume, from the forward's depth (B,h,w) and stats:
 *   g_cost (B,D,h,w)[b,d,p] = exp(cost - M) * (1/se) * g_depth[b,p] * (depth_values[b,d] - depth[b,p]).
 *   g_depth (B,h,w) NULL = zero gradient (g_cost is written with zeros).  No gradient to depth_values (the reference's samples
 *   come from linspace of a range that carries none) and none through the confidence (computed under no_grad, mvsnet.py:143-160). */
int mvd_softmax_regress_stats_f32(const float* cost, const float* depth_values, int B, int D, int h, int w,
                                  float* depth_out, float* conf_out, float* stats_out, mvd_stream_t stream);
int mvd_softmax_regress_backward_f32(const float* cost, const float* depth_values, const float* depth, const float* stats,
                                     const float* g_depth, int B, int D, int h, int w, float* g_cost, mvd_stream_t stream);

/* Measurement aid (bench.py's `measured_stream_peak_gbs`): fills n floats (n % 4 == 0, dst 16-byte aligned) with a pure
 * streaming-store pass, the access pattern an HBM-write-bound kernel can reach at best on this device. */
int mvd_stream_fill_f32(float* dst, long long n, float value, mvd_stream_t stream);

/* Measurement hook (bench.py): arms a pair of hipEvent_t for THIS thread; the next mvd_warp_variance_f32,
 * mvd_homo_warp_f32, mvd_sweep_corr_f32 or mvd_conv3d_weight_grad_f32 call records `start` on its stream immediately before its main kernel
 * (after the small feature re-packing launches) and `stop` immediately after it, then disarms.  Pass NULLs to
 * disarm.  Nothing is synchronised; the caller reads the events after synchronising the stream. */
int mvd_arm_kernel_timing(void* start_event, void* stop_event);

/* Epilogue of the DispNet 2-D convolutions around the Path-A sweep (rmvd/models/blocks/dispnet_encoder.py,
 * dispnet_costvolume_encoder.py, dispnet_decoder.py: Conv2d / ConvTranspose2d with bias followed by LeakyReLU(0.2)):
 *   x[n][c][i] = leaky_relu(x[n][c][i] + bias[c], slope), in place, x (N,C,HW) contiguous.
 * The convolutions themselves stay on the vendor library; this replaces the two elementwise passes after each. */
int mvd_bias_leaky_relu_f32(float* x, const float* bias, int N, int C, long long HW, float slope, mvd_stream_t stream);

/* Other consumers of the sweep as reduction modes of one generic kernel: CVP-MVSNet's variance
 * with PER-PIXEL depth hypotheses (rmvd/models/cvp_mvsnet.py:125-168, blocks/cvp_mvsnet_components.py:375-456) and
 * Vis-MVSNet's group-wise correlation (blocks/utils.py:71-89, blocks/vis_mvsnet_singlestage.py:230-260).
 *   key_feat (B,C,h,w); src_feat[v] (B,C,h,w); M[v] (B,3,4) = [R | t] with (X,Y,Z) = R (x+o, y+o, 1)^T d + t;
 *   depth (B,D), or (B,D,h,w) when depth_per_pixel; sample index = (X/Z) * scale + bias, bilinear, zero padding
 *   (homo_warp / cvp homo_warping: o = 0, scale = W/(W-1), H/(H-1), bias = -0.5; vis homography_warping: o = 0.5, scale = 1,
 *   bias = -0.5);
 *   mode MVD_REDUCE_VARIANCE / MVD_REDUCE_VARIANCE_KEYSQ: out[0] (B,C,D,h,w) — KEYSQ reproduces the reference's aliasing
 *   of the running sum with the squared key volume (cvp_mvsnet.py:129-130);
 *   mode MVD_REDUCE_GROUPCORR: out[v] (B,groups,D,h,w) = sum over each group's channels of key * warped source v. */
#define MVD_REDUCE_VARIANCE 0
#define MVD_REDUCE_VARIANCE_KEYSQ 1
#define MVD_REDUCE_GROUPCORR 2
size_t mvd_sweep_reduce_workspace_bytes(int B, int C, int h, int w, int V);
int mvd_sweep_reduce_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                         int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, int mode, int groups,
                         int B, int C, int D, int h, int w, int V, float* const* out, void* workspace, size_t workspace_bytes,
                         mvd_stream_t stream);

/* The variance modes of mvd_sweep_reduce_f32 on the layouts the engine uses between its own kernels, for CVP-MVSNet as a model
 * (rmvd/models/cvp_mvsnet.py:125-160 coarse level, blocks/cvp_mvsnet_components.py:375-456 proj_cost):
 *   key_feat (B,h,w,C) channel-last; src_feat[v] (B,h+3,w+3,C) channel-last, zero-bordered with the map at (1,1) (what
 *   mvd_conv2d_split_f32 writes through its row / image strides); out (B,D,h,w,C) channel-last, what the 3-D convolutions read.
 *   depth, M, pix_offset, scale, bias: as in mvd_sweep_reduce_f32.  mode MVD_REDUCE_VARIANCE or MVD_REDUCE_VARIANCE_KEYSQ
 *   (MVD_REDUCE_GROUPCORR: MVD_ERR_INVALID_ARG).  C a multiple of 4 up to 64; all maps 16-byte aligned.
 * No workspace, no repacking launches.  The arithmetic per output element is mvd_sweep_reduce_f32's operation for operation: the
 * result is bit-identical to that entry's on the same values, permuted. */
int mvd_sweep_reduce_nhwc_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                              int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, int mode, int B, int C,
                              int D, int h, int w, int V, float* out, mvd_stream_t stream);

/* K5 with per-pixel hypotheses — replaces F.softmax + depth_regression_refine + the 4-bin confidence of CVPMVSNet.forward
 *   rmvd/models/cvp_mvsnet.py:210-236, rmvd/models/blocks/cvp_mvsnet_components.py:138-141.
 *   cost (B,D,h,w) raw regulariser output; depth_hypos (B,D,h,w);
 *   depth_out (B,h,w) = sum_d softmax(cost)_d * depth_hypos_d
 *   conf_out  (B,h,w) = sum_{j=idx-1..idx+2, 0<=j<D} softmax(cost)_j, idx = trunc(sum_d p_d * d)   (mvd_softmax_regress_f32's
 * conventions).  conf_out may be NULL.  Any D >= 1; D <= 8 keeps a pixel's planes in registers (one pass over both volumes). */
int mvd_softmax_regress_pp_f32(const float* cost, const float* depth_hypos, int B, int D, int h, int w, float* depth_out,
                               float* conf_out, mvd_stream_t stream);

/* Vis-MVSNet's group-wise correlation (MVD_REDUCE_GROUPCORR of mvd_sweep_reduce_f32) on the layouts the engine uses between its own
 * kernels, for Vis-MVSNet as a model — replaces SingleStage.build_cost_volume + groupwise_correlation,
 *   rmvd/models/blocks/vis_mvsnet_singlestage.py:86-122,242, rmvd/models/blocks/utils.py:71-89,95-186.
 *   key_feat (B,h,w,C) channel-last; src_feat[v] (B,h+3,w+3,C) channel-last, zero-bordered with the map at (1,1);
 *   out[v] (B,D,h,w,groups) channel-last, what the 3-D convolutions read (V pointers: they may be consecutive slices of one
 *   (V B,D,h,w,groups) buffer); depth, M, pix_offset, scale, bias: as in mvd_sweep_reduce_f32.
 *   grid_clamp > 0: the reference's interpolate clamps its NORMALISED sampling grid to +-grid_clamp (1.1, blocks/utils.py:168) before
 *   grid_sample, i.e. the sample index to [((1 - c) w - 1) / 2, ((1 + c) w - 1) / 2]: on maps narrower than 10 pixels a sample far
 *   outside the map then still takes a part of the rim pixel (at w = 8 the index stops at 7.9).  The kernel clamps the index to that
 *   interval (within its own [-1, w]); on wider maps it changes nothing.  grid_clamp <= 0: no such clamp (mvd_sweep_reduce_f32's values).
 *   C a multiple of 4 up to 64, C / groups a multiple of 4; key_feat, src_feat[v] and out[0] 16-byte aligned, out[v > 0] 4-byte (the
 *   slices that follow out[0] in one buffer are not 16-byte aligned when B D h w groups is no multiple of 4) (MVD_ERR_INVALID_ARG otherwise).
 * No workspace, no repacking launches; without grid_clamp bit-identical to mvd_sweep_reduce_f32's group correlation on the same
 * values, permuted. */
int mvd_sweep_groupcorr_nhwc_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                                 int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, float grid_clamp,
                                 int groups, int B, int C, int D, int h, int w, int V, float* const* out, mvd_stream_t stream);

/* Vis-MVSNet's soft argmin, entropy and windowed probability in one kernel — replaces soft_argmin and entropy,
 *   rmvd/models/blocks/utils.py:51-68, as called from rmvd/models/blocks/vis_mvsnet_singlestage.py:254-258,330-333.
 *   score (B,D,h,w); depth_start (B), or (B,h,w) when start_per_pixel; depth_interval (B); with p = softmax_D(score):
 *   depth_out    (B,h,w) = (sum_i i p_i) * depth_interval + depth_start
 *   entropy_out  (B,h,w) = sum_i -p_i log(clamp(p_i, 1e-9, 1))          (may be NULL)
 *   prob_map_out (B,h,w) = sum_i p_i [|i - sum_j j p_j| <= window]      (may be NULL; window is read only when it is given)
 * Any D >= 1. */
int mvd_soft_argmin_f32(const float* score, const float* depth_start, int start_per_pixel, const float* depth_interval, float window,
                        int B, int D, int h, int w, float* depth_out, float* entropy_out, float* prob_map_out, mvd_stream_t stream);

/* Vis-MVSNet's "soft" fusion of the pair-wise regularised volumes — replaces the weight / weight_sum / fused_interm chain of
 *   rmvd/models/blocks/vis_mvsnet_singlestage.py:263-266,302-303.
 *   x[v] (B,D,h,w,C) channel-last, C a multiple of 4, 16-byte aligned; u[v] (B,h,w);
 *   out (B,D,h,w,C) = (sum_v x_v exp(-u_v)) / (sum_v exp(-u_v)), both sums in view order starting from 0, then one division. */
int mvd_vis_fuse_f32(const float* const* x, const float* const* u, int B, int D, int h, int w, int C, int V, float* out,
                     mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the sweep operators w.r.t. the feature maps, for the training loop
 * (rmvd/train/multi_view_depth_training.py:231-246).  The sampling grids carry no gradient (planesweep_corr.py:436,464,489;
 * homo_warp's grid depends on calibration only).  Scatter-adds use float atomics: run-to-run summation order varies.
 * All feature / gradient maps are CHANNEL-LAST; source maps are zero-bordered (.., h+3, w+3, C) with the map at (1,1), as in
 * the forward kernels.  The callee zeroes the gradient outputs it accumulates into.
 * ---------------------------------------------------------------------------------------------- */

/* VJP of mvd_warp_variance_f32.  key_feat, src_feat[v], grad_key, grad_src[v]: (B,h+3,w+3,C) zero-bordered channel-last
 * (gradient border entries = the share of taps that fell on the zero padding; discard them); grad_var (B,D,h,w,C). */
size_t mvd_warp_variance_backward_workspace_bytes(int B);
int mvd_warp_variance_backward_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                                   const float* key_proj_inv, const float* depth_values, const float* grad_var, int B, int C,
                                   int D, int h, int w, int V, float* grad_key, float* const* grad_src, void* workspace,
                                   size_t workspace_bytes, mvd_stream_t stream);

/* The same VJP as a gather: no float atomics and a fixed summation order, so two calls on the same inputs return the same bits.
 * Arguments as mvd_warp_variance_backward_f32 (C in {4,8,16,32,64}; all maps 16-byte aligned), with these differences:
 *   - grad_src[v] receives its INTERIOR only (written once, not accumulated; no memset needed); its border entries are undefined.
 *     grad_key is bit-identical to mvd_warp_variance_backward_f32's.
 *   - every source pixel searches a window of (2 MVD_K3_GATHER_RADIUS + 1)^2 key pixels per plane.  Where a view's mapping minifies
 *     so much that a contribution falls outside that window, the kernels detect it on the device (exactly, per (b, view)) and that
 *     view's gradient is produced by the atomic scatter instead: always correct, bit-reproducible for the views that did not fall
 *     back.  fallback_count: device int, or NULL; the number of (b, view) that fell back is ADDED to it (zero it yourself).
 *   - the workspace also holds the per-voxel mean volume (B,D,h,w,C).  No host synchronisation. */
#define MVD_K3_GATHER_RADIUS 3
size_t mvd_warp_variance_backward_gather_workspace_bytes(int B, int C, int D, int h, int w, int V);
int mvd_warp_variance_backward_gather_f32(const float* key_feat, const float* const* src_feat, const float* const* src_proj,
                                          const float* key_proj_inv, const float* depth_values, const float* grad_var, int B, int C,
                                          int D, int h, int w, int V, float* grad_key, float* const* grad_src, int* fallback_count,
                                          void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* VJP of mvd_sweep_corr_f32 (masks are constants).  feat_key, grad_key (N,h,w,C) channel-last; feat_src[v], grad_src[v]
 * (N,hs+3,ws+3,C) zero-bordered channel-last; grad_corr[v] (N,S,h,w).  C in {64,128,192,256}.  invdepth_mode / corr_scale as
 * in mvd_sweep_corr_ex_f32. */
int mvd_sweep_corr_backward_f32(const float* feat_key, const float* const* feat_src, const float* K_key,
                                const float* const* K_src, const float* const* T_src2key, const float* invdepths,
                                int invdepth_mode, float corr_scale, const float* const* grad_corr, int N, int C, int h, int w,
                                int hs, int ws, int S, int V, float* grad_key, float* const* grad_src, mvd_stream_t stream);

/* VJP of mvd_sweep_warp_f32 (normalize_after = 0) w.r.t. the source features: what autograd computes through WarpOnlyCorr's
 * grid_sample (rmvd/models/blocks/planesweep_corr.py:107-140; grids under no_grad, :436,464,489).  The op is linear in the
 * features, so no feature map is passed: grad_warped[v] (N,S,C,h,w) is the cotangent of warped_out[v]; grad_src[v]
 * (N,hs+3,ws+3,C) zero-bordered channel-last (border = the zero padding's share; discard it).  The sampling mask is a constant
 * and a masked sample contributes nothing.  C in 1..256.  normalize_after has no kernel here: differentiate x / (|x|_2 + 1e-9)
 * outside (ops.sweep_warp_autograd does it in torch). */
int mvd_sweep_warp_backward_f32(const float* K_key, const float* const* K_src, const float* const* T_src2key, const float* invdepths,
                                int invdepth_mode, const float* const* grad_warped, int N, int C, int h, int w, int hs, int ws, int S,
                                int V, float* const* grad_src, mvd_stream_t stream);

/* VJP of mvd_sweep_reduce_f32 w.r.t. the feature maps: what autograd computes through grid_sample in CVP-MVSNet's proj_cost
 * (rmvd/models/blocks/cvp_mvsnet_components.py:375-456, grid detached :397) and in Vis-MVSNet's homography_warping +
 * groupwise_correlation (rmvd/models/blocks/utils.py:71-89,154-186, grids without gradient :97,164,181; the depths are detached,
 * rmvd/models/vis_mvsnet.py:124,150).  Forward arguments as in mvd_sweep_reduce_f32, in the reference's layouts:
 *   key_feat, src_feat[v], grad_key, grad_src[v] (B,C,h,w); grad_out: the cotangent of `out`, grad_out[0] (B,C,D,h,w) for the
 *   variance modes, grad_out[v] (B,groups,D,h,w) for MVD_REDUCE_GROUPCORR.
 * Depths and M are constants.  grad_key is a plain sum (bit-reproducible); grad_src is scatter-added with float atomics into
 * zero-bordered maps in the workspace and copied out without the border. */
size_t mvd_sweep_reduce_backward_workspace_bytes(int B, int C, int h, int w, int V);
int mvd_sweep_reduce_backward_f32(const float* key_feat, const float* const* src_feat, const float* const* M, const float* depth,
                                  int depth_per_pixel, float pix_offset, float scale_x, float scale_y, float bias, int mode,
                                  int groups, const float* const* grad_out, int B, int C, int D, int h, int w, int V, float* grad_key,
                                  float* const* grad_src, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* VJP of mvd_fuse_views_f32 w.r.t. corr[v] (N,S,h,w) and score[v] (N,1,h,w); masks and the fused mask are constants. */
int mvd_fuse_views_backward_f32(const float* const* corr, const float* const* mask, const float* const* score,
                                const float* grad_fused, int N, int S, int h, int w, int V, float* const* grad_corr,
                                float* const* grad_score, mvd_stream_t stream);

/* Input resize of the model adapters: replaces ResizeInputs / UpscaleInputsToNextMultipleOf
 * (rmvd/data/transforms.py:40-98, called from robust_mvd.py:104-113 and mvsnet.py:178), i.e.
 * skimage.transform.resize(order=1) for UPSCALING (ho >= hi, wo >= wi): no anti-aliasing, float32 kept, mirror boundary,
 * half-pixel centres, float64 interpolation — the arithmetic of scipy.ndimage.zoom(order=1, mode='mirror',
 * grid_mode=True), which skimage delegates to.  src (planes,hi,wi) -> dst (planes,ho,wo); planes = N*C <= 65535. */
int mvd_resize_order1_f32(const float* src, float* dst, long long planes, int hi, int wi, int ho, int wo,
                          mvd_stream_t stream);

/* Prediction head of the DispNet decoder in one pass (rmvd/models/blocks/dispnet_decoder.py:17-22,126-138; ReLUAndSigmoid,
 * blocks/utils.py:30-41 with min -10 / max 10): x (N,2,HW) = output of a pred_k convolution;
 * pred (N,2,HW): channel 0 = relu(x0), channel 1 = sigmoid(x1 * 0.2) * 20 - 10; ent (N,1,HW) = log(2 exp(pred1) + 1e-4) + 1. */
int mvd_dispnet_head_f32(const float* x, float* pred, float* ent, int N, long long HW, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Scoring of the multi-view depth evaluation on the device — replaces the numpy post-processing and metrics of
 *   rmvd/eval/multi_view_depth_evaluation.py:469-547,583-610 and rmvd/eval/metrics.py:32-220.
 * gt (H,W); pred and the optional uncertainty (h,w), any size relation.  The nearest resize to (H,W) is a gather through two
 * int32 tables: output row y reads input row row[y] in [0,h), output column x reads col[x] in [0,w); the rule of
 * skimage.transform.resize(order=0) is floor((o + 0.5) * (n_in / n_out)) in float64, clamped.  The tables are trusted.
 * mask = gt > 0, and pred != 0 when sparse_pred.  All cross-workgroup float reductions are partials summed in a fixed order (two
 * calls give the same bits); workspace: mvd_depth_eval_workspace_bytes(H, W), shared by the three entries that take one. */
#define MVD_ALIGN_NONE 0
#define MVD_ALIGN_MEDIAN 1 /* ratio = median(gt[mask]) / median(pred[mask]), np.median on float32, exact radix select */
#define MVD_ALIGN_LSQ 2    /* least-squares scale and shift on nan_to_num(1 / x), five float64 sums */
size_t mvd_depth_eval_workspace_bytes(int H, int W);

/* params (8 floats, device): [0] ratio (median; NaN = leave the prediction unscaled) or scale (least squares; NaN when the mask is
 *   empty or det <= 0), [1] shift, [2] median(gt[mask]), [3] median(pred[mask]), [4] 1 when the mask is not empty (median) or
 *   det > 0 (least squares), [5] min of the resized uncertainty over ALL (H,W) pixels (NaN without one, or when one is NaN).
 * sums (5 doubles, device, may be NULL; least squares only): sum p^2, sum p, n, sum g p, sum g. */
int mvd_depth_align_stats_f32(const float* gt, const float* pred, const float* uncertainty, const int* row, const int* col, int H,
                              int W, int h, int w, int mode, int sparse_pred, float* params, double* sums, void* workspace,
                              size_t workspace_bytes, mvd_stream_t stream);

/* One run's alignment (params[0..1] read from DEVICE memory: mvd_depth_align_stats_f32's or the caller's own; may be NULL for
 * MVD_ALIGN_NONE), clip to [clip_lo, clip_hi] times the prediction mask when clip, invdepth = nan_to_num(1 / pred), rel_ae =
 * nan_to_num(|pred - gt| / gt) * mask and the inlier test 0 < max(nan_to_num(gt / pred -> thresh_plus_one), nan_to_num(pred / gt))
 * < thresh.  result (40 bytes, device, 8-byte aligned): double sum of rel_ae; int64 count of the mask, of the inliers in it, of the
 * evaluated pixels (pred_aligned != 0 when sparse_pred, else all); float min of rel_ae over all pixels; 4 bytes of scratch.
 * The four (H,W) maps are written where their pointer is not NULL. */
int mvd_depth_score_f32(const float* gt, const float* pred, const float* uncertainty, const int* row, const int* col, int H, int W,
                        int h, int w, int mode, int sparse_pred, int clip, float clip_lo, float clip_hi, float thresh,
                        float thresh_plus_one, const float* params, void* result, float* pred_out, float* invdepth_out,
                        float* rel_ae_out, float* uncertainty_out, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* keys[p] = ((u[p] - u_min[0]) + 1) * mask[p] in float32 (metrics.py:169); u, gt, pred_aligned, keys: n floats; u_min on the device. */
int mvd_rank_keys_f32(const float* u, const float* u_min, const float* gt, const float* pred_aligned, int sparse_pred, long long n,
                      float* keys, mvd_stream_t stream);

/* ranked: n errors in ranked order (the valid pixels first); count[0] (device int64, clamped to n): the number of valid ones.
 * step_sums[i], i < 100 = float64 sum of ranked[int((count / 100) * i) .. count), the steps formed on the device in float64. */
int mvd_ranked_step_sums_f64(const float* ranked, long long n, const long long* count, double* step_sums, void* workspace,
                             size_t workspace_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-view depth fusion: geometric consistency of per-view depth maps and their point cloud.  The reference has NO counterpart
 * (it stops at the per-view depth map): the definition is robustmvd_amd/depth_fusion.py's fuse_numpy and DESIGN.md.
 * key_depth and every src_depth[s]: (H,W), H and W >= 2, no alignment requirement.  matrices (V,24) on the device, composed by the
 * host in float64: per source  A = Ks R Kk^-1 (9, row-major), b = Ks t (3) with [R|t] = Ts Tk^-1, then A' = Kk R' Ks^-1 (9) and
 * b' = Kk t' (3) with [R'|t'] = Tk Ts^-1.  For key pixel (x,y) with depth d:  Q = d A (x,y,1) + b, (u,v) = Q.xy / Q.z, valid when d
 * is finite and > 0, Q.z > 0 and 0 <= u <= W-1, 0 <= v <= H-1;  ds = the bilinear blend of src_depth[s] in the cell x0 = min(floor(u),
 * W-2), y0 = min(floor(v), H-2), invalid when one of its four taps is not finite or <= 0;  Q' = ds A' (u,v,1) + b', d' = Q'.z,
 * err = hypot(Q'.x / d' - x, Q'.y / d' - y), rel = |d' - d| / d;  consistent = valid and err < max_reproj_error and
 * rel < max_rel_depth_diff.  (The kernel forms (u,v) from Q / d = A (x,y,1) + b / d, which is (x,y) itself for A = I, b = 0.)
 * view_bits (H,W) uint32: bit s = source s is consistent;  fused (H,W) = (d + sum of the consistent d') / (count + 1), 0 where d is
 * invalid;  mask (H,W) uint8 = count >= min_consistent_views, and uncertainty <= max_uncertainty (false for a NaN) when uncertainty
 * is not NULL;  num_consistent (H,W) uint8, may be NULL = popcount(view_bits), for callers that would otherwise count the bits again.
 * No atomics and a fixed summation order: two calls give the same bits. */
int mvd_geo_consistency_f32(const float* key_depth, const float* const* src_depth, const float* matrices, const float* uncertainty,
                            int V, int H, int W, float max_reproj_error, float max_rel_depth_diff, int min_consistent_views,
                            float max_uncertainty, unsigned* view_bits, float* fused, unsigned char* mask,
                            unsigned char* num_consistent, mvd_stream_t stream);

/* The masked pixels in row-major order as 3-D points: a deterministic stream compaction (per-chunk counts from wave ballots, an exclusive scan
 * by one workgroup, a scatter to chunk offset + rank in the ballot; no atomic decides a position).
 * backproject (12 floats, device): B = Rk^T Kk^-1 (9, row-major) and c = -Rk^T tk (3) of the key's world-to-view pose [Rk|tk]:
 * xyz[m] = depth * B (x,y,1) + c.  image: NULL or planar (3,H,W), gathered into rgb (M,3).  xyz and rgb hold H*W points; count (device,
 * 8-byte aligned) receives M.  workspace: mvd_compact_points_workspace_bytes(H, W). */
size_t mvd_compact_points_workspace_bytes(int H, int W);
int mvd_compact_points_f32(const unsigned char* mask, const float* depth, const float* image, const float* backproject, int H, int W,
                           float* xyz, float* rgb, long long* count, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* mvd_compact_points_f32 with a second optional planar attribute: attr NULL or (3,H,W) (the normals), gathered into attr_out (M,3) in
 * the same order as rgb; attr and attr_out go together.  xyz, rgb and count are what mvd_compact_points_f32 gives. */
int mvd_compact_points_attr_f32(const unsigned char* mask, const float* depth, const float* image, const float* attr,
                                const float* backproject, int H, int W, float* xyz, float* rgb, float* attr_out, long long* count,
                                void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* World-frame normals of one depth map (H,W) -> normals (3,H,W) planar.  backproject: mvd_compact_points_f32's 12 floats, of which
 * only B is read: P(x,y) = depth(x,y) B (x,y,1), without the translation, which cancels in the differences;
 * n = (P(x+1,y) - P(x-1,y)) x (P(x,y+1) - P(x,y-1)), normalised, negated when n . B (x,y,1) > 0 so that it points towards the camera.
 * (0,0,0) = invalid: on the image border, where one of the five depths is not finite or <= 0, where |n| is zero or not finite.
 * There is no depth-discontinuity guard. */
int mvd_depth_normals_f32(const float* depth, const float* backproject, int H, int W, float* normals, mvd_stream_t stream);

/* mvd_geo_consistency_f32 for fusing a scene view by view into one point per surface sample (depth_fusion.py: merge_numpy).
 * view_bits, fused and num_consistent are mvd_geo_consistency_f32's, bit for bit.  key_claimed (H,W) bytes, read only: non-zero where
 * an earlier view has merged this pixel into one of its points; mask = mvd_geo_consistency_f32's mask and key_claimed == 0.  For a
 * pixel with mask set and every consistent source s the target is the source pixel (rint(u), rint(v)), half to even: the byte 1 is
 * stored at the target in src_claimed[s] (host array of V device pointers, (H,W) bytes each, none of them key_claimed: the entry
 * refuses a view among its own sources).  Several lanes may store the same byte, all store 1: two calls give the same bits.
 * key_image / src_image[V] (planar (3,H,W); all NULL or none) -> merged_rgb (3,H,W) = (the key pixel's colour + the targets' colours
 * in source order) / (count + 1);  key_normal / src_normal[V] (planar, mvd_depth_normals_f32's; all NULL or none) -> merged_normal
 * (3,H,W) = the normalised sum of the key pixel's and the targets' normals (an invalid one is zero and adds nothing), (0,0,0) when
 * the sum's length is zero or not finite.  Both are 0 where mask is 0.  float32 sums in source order, no atomics. */
int mvd_geo_merge_f32(const float* key_depth, const float* const* src_depth, const float* matrices, const float* uncertainty, int V,
                      int H, int W, float max_reproj_error, float max_rel_depth_diff, int min_consistent_views, float max_uncertainty,
                      const unsigned char* key_claimed, unsigned char* const* src_claimed, const float* key_image,
                      const float* const* src_image, const float* key_normal, const float* const* src_normal, unsigned* view_bits,
                      float* fused, unsigned char* mask, unsigned char* num_consistent, float* merged_rgb, float* merged_normal,
                      mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Point-cloud evaluation: the truncated nearest neighbour between two clouds, the scores of its distances, and voxel thinning.  The
 * reference has NO counterpart: the definition is robustmvd_amd/cloud_eval.py (nearest_numpy, cloud_scores_numpy,
 * voxel_downsample_numpy) and DESIGN.md.  A point with a non-finite coordinate is INVALID.  Every count is below 2^31.
 *
 * Cells.  i_a = floor((double(x_a) - origin_a) * inv) for a in x, y, z, two IEEE double operations and a floor, with inv formed by
 * the host (1.0 / cell edge, or 1.0 / voxel), so that numpy on the host and the device agree on membership bit for bit.
 * key = i_x << 42 | i_y << 21 | i_z with every index in [0, 2^21 - 1) (the caller checks the extent; the device clamps);
 * an invalid point gets INT64_MAX, which no valid point can have, and sorts last.  Between mvd_cloud_cell_keys_f32 and its
 * consumers the caller sorts the keys STABLY and keeps the permutation (perm[i] = the original index of sorted position i).
 *
 * Truncated nearest neighbour, queries Q (n), targets P (m), max_dist > 0:
 *   dist[i]  = min(max_dist, min over valid j of |Q_i - P_j|)   (max_dist when Q_i is invalid or there is no valid target)
 *   index[i] = the j of that minimum when it is < max_dist (strict), else -1
 * |q - p| = sqrt(dx^2 + dy^2 + dz^2) of the float32 coordinate DIFFERENCES, never |q|^2 + |p|^2 - 2 q.p, which at coordinates
 * around 10^3 and distances around 10^-2 has no correct digit.  Among targets with an equal sum of squares, as the device computed
 * it, the smallest original index wins.  No atomic decides a value: two calls give the same bits. */
#define MVD_CLOUD_MAX_THRESHOLDS 8
int mvd_cloud_cell_keys_f32(const float* points, long long n, double origin_x, double origin_y, double origin_z, double inv,
                            long long* keys, mvd_stream_t stream);

/* records (n,4), 16-byte aligned: sorted position i holds x, y, z of points[perm[i]] and perm[i] as the bits of the fourth float. */
int mvd_cloud_grid_build_f32(const float* points, const long long* perm, long long n, float* records, mvd_stream_t stream);

/* query_records (n,4) and target_records (m,4): mvd_cloud_grid_build_f32's, both clouds keyed with this origin and inv (the queries'
 * order only decides how well a wave's queries share cells; any order gives the same result); target_keys (m): the targets' sorted
 * keys.  The cell edge 1 / inv must be at least max_dist (1 + 2^-10): then the 3 x 3 x 3 cells around a query's hold every target
 * within max_dist (the argument is in csrc/cloud_eval.hip).  dist (n) and index (n) are written in the queries' ORIGINAL order.
 * n == 0 writes nothing; m == 0 truncates every query. */
int mvd_cloud_nearest_f32(const float* query_records, long long n, const float* target_records, const long long* target_keys,
                          long long m, double origin_x, double origin_y, double origin_z, double inv, float max_dist, float* dist,
                          int* index, mvd_stream_t stream);

/* Over the VALID queries of one direction (points (n,3): the queries in original order, looked at only where index < 0; NULL = every
 * query is valid): result (80 bytes, device, 8-byte aligned) = double sum of dist; int64 count of the valid queries; eight int64
 * counts of dist < thresholds[t] (strict), zero for t >= T.  thresholds: T <= MVD_CLOUD_MAX_THRESHOLDS floats on the device.
 * Workgroup partials summed in a fixed order; workspace: mvd_cloud_scores_workspace_bytes(n). */
size_t mvd_cloud_scores_workspace_bytes(long long n);
int mvd_cloud_scores_f32(const float* dist, const int* index, const float* points, long long n, const float* thresholds, int T,
                         void* result, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* Voxel thinning from the sorted voxel keys and their permutation: one output point per occupied voxel in ascending key order, the
 * float64 mean of the voxel's points in original order (a voxel of more than 64 points: 64 interleaved partial sums and a fixed
 * tree), rounded to float32; colors (n,3) -> rgb likewise, both or neither NULL; counts = the voxel's number of points; invalid
 * points are dropped.  xyz, rgb (n,3) and counts (n) hold n voxels; num_voxels (device, 8-byte aligned) receives their number.
 * A deterministic compaction of the segment heads (ballot counts, one workgroup's scan, rank in the ballot), as
 * mvd_compact_points_f32's.  workspace: mvd_voxel_reduce_workspace_bytes(n). */
size_t mvd_voxel_reduce_workspace_bytes(long long n);
int mvd_voxel_reduce_f32(const long long* keys, const long long* perm, const float* points, const float* colors, long long n,
                         float* xyz, float* rgb, int* counts, long long* num_voxels, void* workspace, size_t workspace_bytes,
                         mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Point-cloud registration (ICP): the per-iteration work around mvd_cloud_nearest_f32.  The reference has NO counterpart: the
 * definition is robustmvd_amd/cloud_register.py (transform_numpy, pair_sums_numpy) and DESIGN.md.
 *
 * transform: 12 doubles ON THE HOST, the rows of [M | t], all finite; it travels with the launch.  A point moves as
 *   q_a = float32(((M[a,0] x + M[a,1] y) + M[a,2] z) + t[a])   in float64 in exactly this order, rounded once;
 * a row with a non-finite coordinate before or after the move becomes (NaN, NaN, NaN) with the bits 0x7fc00000.  A normal goes
 * through M alone (the same order) and is divided by its float64 length; an invalid or vanishing one becomes (0, 0, 0).
 * normals / out_normals: both or neither NULL. */
int mvd_cloud_transform_f32(const float* points, const float* normals, long long n, const double* transform, float* out_points,
                            float* out_normals, mvd_stream_t stream);

/* mvd_cloud_grid_build_f32 of the MOVED points: sorted position i holds T(points[perm[i]]) and perm[i]'s bits; the moved cloud is
 * never stored in its own order. */
int mvd_cloud_transform_records_f32(const float* points, const long long* perm, long long n, const double* transform, float* records,
                                    mvd_stream_t stream);

/* The sums of one ICP iteration.  Source point i pairs with target j = index[i] (mvd_cloud_nearest_f32's, in the source's original
 * order) when 0 <= j < m, q_i = T(source_i) (recomputed: the records' bits) and target_j are valid and, with target_normals, that
 * normal is finite and not (0,0,0).  With c = pivot, a = double(q_i) - c, b = double(target_j) - c, d = a - b, all float64:
 *   target_normals == NULL: N; sum a (3); sum b (3); sum a_r b_c (9, row-major); sum (a_x a_x + a_y a_y) + a_z a_z; the same of b; of d
 *   else, u = double(normal_j), r = (d_x u_x + d_y u_y) + d_z u_z, J = (a_y u_z - a_z u_y, a_z u_x - a_x u_z, a_x u_y - a_y u_x, u):
 *                           N; sum J_i J_k for i <= k (21, row-major); sum J_k r (6); sum r r
 * result (256 bytes, device, 8-byte aligned): N as int64, then the doubles in this order, then zeros.  Every workgroup adds
 * MVD_CLOUD_PAIR_SUMS_PER_WORKGROUP consecutive points in a fixed order and one workgroup adds the partials: no atomics, two calls give
 * the same bits; n == 0 or no pair writes zeros.  workspace: mvd_cloud_pair_sums_workspace_bytes(n). */
#define MVD_CLOUD_PAIR_SUMS_PER_WORKGROUP 2048
size_t mvd_cloud_pair_sums_workspace_bytes(long long n);
int mvd_cloud_pair_sums_f32(const float* source, long long n, const double* transform, const int* index, const float* target,
                            const float* target_normals, long long m, double pivot_x, double pivot_y, double pivot_z, void* result,
                            void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Point-cloud clean-up: the neighbours within a radius, the k nearest, PCA normals and outlier removal.  The reference has NO
 * counterpart: the definition is robustmvd_amd/cloud_clean.py (neighbourhood_numpy, knn_numpy, list_moments_numpy,
 * normals_from_moments_numpy, remove_outliers_numpy) and DESIGN.md, restated here.  No entry uses an atomic.
 *
 * Pair distance of a query q and a target p, in float32 and in exactly this order, without contraction:
 *   dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z,  d2 = (dx dx + dy dy) + dz dz
 * which are float32 numpy's bits, so membership and order are exact integers.  (mvd_cloud_nearest_f32 contracts to FMAs: another d2.)
 * p is a NEIGHBOUR of q iff both are valid and d2 < r2 (strict), r2 = radius * radius in float32.  exclude_self != 0: the queries ARE
 * the targets (the same records), and a point is not its own neighbour, by index; its duplicates are, at distance 0.
 * Records, keys, origin and inv are mvd_cloud_grid_build_f32's and mvd_cloud_nearest_f32's; the cell edge 1 / inv must be at least
 * radius (1 + 2^-10) (the 27-cell argument for d2 < r2 is in csrc/cloud_clean.hip).  Outputs are in the queries' ORIGINAL order.
 * n == 0 writes nothing; m == 0 gives empty neighbourhoods.
 *
 * Radius moments.  count (n) int32; sum_dist (n) float64 = sum of double(sqrtf(d2)); moments (n,9) float64: with
 * v = (double(p.x) - double(q.x), double(p.y) - double(q.y), double(p.z) - double(q.z)), relative to the QUERY, sum v (3) then
 * sum v_a v_b for a <= b (6, row-major).  ORDER: every sum starts from +0.0 and adds the neighbours one after the other in ascending
 * position of the target grid's sorted order, that is by (cell key, original index).  An invalid query or one without neighbours
 * gives 0 and zeros. */
#define MVD_CLOUD_KNN_MAX 16
int mvd_cloud_radius_moments_f32(const float* query_records, long long n, const float* target_records, const long long* target_keys,
                                 long long m, double origin_x, double origin_y, double origin_z, double inv, float radius,
                                 int exclude_self, int* count, double* sum_dist, double* moments, mvd_stream_t stream);

/* The up-to-k neighbours within max_dist that are smallest in (bits of d2, original index), 1 <= k <= MVD_CLOUD_KNN_MAX, n k < 2^31:
 * index (n,k) int32 ascending in that order and -1 past the found ones; dist (n,k) float32 = sqrtf(d2), max_dist past them; count (n)
 * int32.  The list is kept in registers at a capacity of 4, 8 or 16: a k in between is served by the next capacity. */
int mvd_cloud_knn_f32(const float* query_records, long long n, const float* target_records, const long long* target_keys, long long m,
                      double origin_x, double origin_y, double origin_z, double inv, float max_dist, int k, int exclude_self,
                      int* index, float* dist, int* count, mvd_stream_t stream);

/* mvd_cloud_radius_moments_f32's outputs over each query's list instead: queries (n,3), targets (m,3), index and dist (n,k) of
 * mvd_cloud_knn_f32; the entries are added in LIST order up to the first index outside [0, m), sum_dist from double(dist). */
int mvd_cloud_list_moments_f32(const float* queries, long long n, const float* targets, long long m, const int* index, const float* dist,
                               int k, int* count, double* sum_dist, double* moments, mvd_stream_t stream);

/* Normals from moments, one lane per point, float64.  The PCA is over the neighbours AND the point itself, which adds zeros:
 * N = count + 1, mean = sum v / N, C = sum v v^T / N - mean mean^T (each entry: one division, one product, one difference).
 * l0 <= l1 <= l2: C's eigenvalues (cyclic Jacobi, a fixed number of sweeps); normal (n,3) float32 = the unit eigenvector of l0;
 * curvature (n) float32 = l0 / ((l0 + l1) + l2), the surface variation, 0 when the sum is 0.  The normal is (0,0,0) and the curvature NaN
 * where count < min_neighbours (at least 2), where l1 <= 1e-9 l2 (collinear or coincident neighbours) or where the point is invalid.
 * Orientation, on the float64 unit vector u before it is rounded: orient 1: w = (toward_x, toward_y, toward_z) - double(q);
 * 2: w = double(toward[i]) - double(q); 3: w = double(toward[i]) (reference normals); dot = (u.x w.x + u.y w.y) + u.z w.z; u is
 * flipped when dot < 0.  orient 0, or a dot that is 0 or NaN: flipped when its component of largest magnitude (the first among
 * equals) is negative.  toward (n,3) float32: orient 2 and 3 only, else NULL. */
int mvd_cloud_normals_f64(const float* points, long long n, const int* count, const double* moments, int min_neighbours, int orient,
                          double toward_x, double toward_y, double toward_z, const float* toward, float* normal, float* curvature,
                          mvd_stream_t stream);

/* The verdicts of outlier removal, keep (n) bytes 0 / 1; an invalid point is always dropped.
 * Density: keep iff the point is valid and count >= min_neighbours.
 * Statistical: mean (n) float64 = (sum over the list of double(dist), in list order from +0.0) / k where count == k (a FULL list), NaN
 * elsewhere; result (32 bytes, device, 8-byte aligned) = the float64 sum of those means, the float64 sum of their squares, their
 * number as int64 and a zero, added in the two-level order of mvd_cloud_scores_f32 (2048 consecutive points per workgroup).  The host
 * forms the threshold; keep iff mean <= threshold.  workspace: mvd_cloud_knn_mean_sums_workspace_bytes(n). */
int mvd_cloud_keep_density(const float* points, const int* count, long long n, int min_neighbours, unsigned char* keep,
                           mvd_stream_t stream);
size_t mvd_cloud_knn_mean_sums_workspace_bytes(long long n);
int mvd_cloud_knn_mean_sums_f32(const float* dist, const int* count, long long n, int k, double* mean, void* result, void* workspace,
                                size_t workspace_bytes, mvd_stream_t stream);
int mvd_cloud_keep_threshold(const double* mean, long long n, double threshold, unsigned char* keep, mvd_stream_t stream);

/* The kept points of a keep mask: kept (n) int32 receives their original indices in ascending order, remap (n) int32 the new index of
 * every point or -1, total (device, 8-byte aligned) their number.  A deterministic compaction (ballot counts, one workgroup's scan,
 * rank in the ballot), as mvd_voxel_reduce_f32's; rows then move through mvd_mesh_gather_rows_f32 with remap.
 * workspace: mvd_cloud_select_workspace_bytes(n). */
size_t mvd_cloud_select_workspace_bytes(long long n);
int mvd_cloud_select(const unsigned char* keep, long long n, int* kept, int* remap, long long* total, void* workspace,
                     size_t workspace_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * TSDF volume: the views' depth maps averaged into a truncated signed distance volume, and its surface as a triangle mesh.  The
 * reference has NO counterpart: the definition is robustmvd_amd/tsdf.py (its docstring, integrate_numpy, extract_numpy) and DESIGN.md.
 *
 * Volume (nx,ny,nz), nx ny nz < 2^31: voxel (i,j,k) sits at origin + voxel (i,j,k).  tsdf and weight (nz,ny,nx) float32, x fastest;
 * color NULL or (3,nz,ny,nx) planar; all three 16-byte aligned, dense (no padding of the rows), zero before the first view.
 *
 * mvd_tsdf_integrate_f32 applies V <= MVD_MAX_VIEWS views of one size (H,W >= 1) in order, in one launch.  depth: host array of V
 * device pointers to (H,W) maps; weight_maps: NULL (every pixel weighs 1) or V maps (H,W); images: NULL or V planar (3,H,W) maps,
 * read only when color is not NULL.  matrices (V,12) on the device, row-major 3x4, composed by the host in float64:
 * M = K T[:3] [[voxel I, origin], [0, 1]] with K the intrinsics and T the world-to-view pose, so that (Qx,Qy,Qz) = M (i,j,k,1).
 * Per voxel and view, skipping the view at the first condition that fails:  Qz > 0;  px = rint(Qx / Qz), py = rint(Qy / Qz), half to
 * even, with 0 <= px <= W-1 and 0 <= py <= H-1;  dm = depth[py,px] and wm = weight_maps[py,px] both finite and > 0;
 * sdf = dm - Qz >= -trunc.  Then f = min(1, sdf / trunc);  W' = W + wm;  F' = (F W + f wm) / W';  C' = (C W + c wm) / W' per channel;
 * W' = min(W', max_weight) when max_weight > 0 (<= 0: no cap).  (The kernel forms Qx / Qz and sdf / trunc with a reciprocal.)
 * A voxel that no view updates keeps its bits.  V views in one call give the bits of V calls of one view.  No atomics. */
int mvd_tsdf_integrate_f32(float* tsdf, float* weight, float* color, int nx, int ny, int nz, const float* const* depth,
                           const float* const* weight_maps, const float* const* images, const float* matrices, int V, int H, int W,
                           float trunc, float max_weight, mvd_stream_t stream);

/* Marching tetrahedra on the Kuhn subdivision.  A voxel is observed when weight >= min_weight and inside when tsdf < 0 (0 counts as
 * outside).  Edge kinds 0..6 run from the owner voxel p to p + (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1).  An edge
 * carries a vertex iff both ends are in the grid and observed and exactly one is inside: t = Fa / (Fa - Fb) with a the owner,
 * position = origin + voxel (p + t delta), colour = Ca + t (Cb - Ca); vertices are ordered by (owner's linear index (k ny + j) nx + i,
 * kind).  A cell whose 8 corners are observed is cut into 6 tetrahedra, v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = (1,1,1) for the
 * permutations (a,b,c) of (0,1,2) in lexicographic order; its triangles, their vertex order and orientation (normals point from
 * inside to outside) are tsdf.py's tri_table(), compiled in as csrc/tsdf_tables.h; triangles are ordered by (cell's linear index,
 * tetrahedron, slot).  Vertices that no triangle references (on edges none of whose cells is fully observed) stay.
 *
 * One entry, two uses.  With vertices == NULL (then triangles and colors are NULL too) it classifies and counts only.  With them it
 * also writes vertices (M,3), colors (M,3) (NULL, or with color) and triangles (T,3) int32: a slot at or past max_vertices /
 * max_triangles (both <= 2^31 - 1) is not written.  counts (device, 16-byte aligned) always receives the true M and T, two int64, exact
 * while each is below 2^32: the caller reads them (one 16-byte copy), refuses 2^31 and more, and allocates.  classified != 0: the
 * workspace still holds the classification of an earlier call on this volume with this min_weight, and it is not formed again.
 * workspace: mvd_tsdf_extract_workspace_bytes(nx, ny, nz), 256-byte aligned.  No atomic decides a position: two calls give the same
 * bits. */
size_t mvd_tsdf_extract_workspace_bytes(int nx, int ny, int nz);
int mvd_tsdf_extract_f32(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, float origin_x,
                         float origin_y, float origin_z, float voxel, float min_weight, int classified, float* vertices, float* colors,
                         int* triangles, long long max_vertices, long long max_triangles, long long* counts, void* workspace,
                         size_t workspace_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh rendering: a triangle mesh rasterised into V <= MVD_MAX_VIEWS pinhole views of one size (H,W).  The reference has NO
 * counterpart: the definition is robustmvd_amd/render.py (its docstring and render_numpy) and DESIGN.md, restated here.
 *
 * vertices (M,3) float32 world coordinates, triangles (T,3) int32 with 0 <= index < M (the caller checks the range; a triangle with an
 * index outside it is skipped), colors NULL or (M,3) float32.  matrices (V,12) on the device, row-major 3x4, composed by the host in
 * float64: P = K T[:3] with K the intrinsics and T the world-to-view pose.  Pixel (px,py) is sampled at the image point (px,py).
 *  1. Vertex: (qx,qy,qz) = P (X,1), each row summed left to right; valid iff qz > near and x = qx / qz, y = qy / qz are finite; z = qz.
 *  2. Triangle (i0,i1,i2): skipped if a vertex is invalid (no near-plane clipping); skipped unless the signed area
 *     A = (x1-x0)(y2-y0) - (y1-y0)(x2-x0) is < 0 or > 0; skipped if its pixel box [ceil(min x), floor(max x)] x [ceil(min y),
 *     floor(max y)], clamped to the image, is empty.  Front-facing iff A < 0 (x right, y down, z forward: a winding normal
 *     (p1-p0) x (p2-p0) that points at the camera).  cull: MVD_CULL_NONE, MVD_CULL_BACK skips A > 0, MVD_CULL_FRONT skips A < 0.
 *  3. Edge value: for the vertex pair a < b by index, e_ab(p) = (x_b-x_a)(p_y-y_a) - (y_b-y_a)(p_x-x_a), evaluated as written, one
 *     rounding per operation.  The oriented edge (i,j) is +e_ij where i < j and -e_ji otherwise.  w0, w1, w2 = the oriented edges
 *     (i1,i2), (i2,i0), (i0,i1) times sign(A).  Covered iff w0, w1, w2 >= 0 and s = (w0 + w1) + w2 > 0.  Two triangles that share an
 *     edge compute the same bits with opposite sign: no pixel between them is lost, a pixel exactly on the edge belongs to both.
 *  4. Depth: b_k = w_k / s, u_k = b_k / z_k, z = 1 / ((u0 + u1) + u2); a pixel whose z is not finite is not covered.
 *  5. Winner: the smallest 64-bit key (float bits of z) << 32 | triangle index: the nearest triangle, among equals the lowest index.
 *  6. Maps, dense, 16-byte aligned: depth (V,H,W) float32, the winner's z or 0; triangle (V,H,W) int32, its index or -1; NULL or
 *     (V,3,H,W) float32 each: bary (b0,b1,b2), out_colors z ((u0 c0 + u1 c1) + u2 c2) (needs colors), normals the winner's unit
 *     winding normal n / |n|, n = (p1-p0) x (p2-p0) in world coordinates, (0,0,0) where |n| is 0 or not finite; all 0 on empty pixels.
 * Left out: near-plane clipping, anti-aliasing, vertex normals.
 *
 * A triangle whose clamped box holds at most max_small pixels is rasterised by one lane, a larger one cooperatively by waves; every
 * max_small >= 0 gives the same bits.  The winner is kept with 64-bit integer min atomics: two calls give the same bits.  H W V and T
 * are at most 2^31 - 1, V T below 2^32.  workspace: mvd_mesh_render_workspace_bytes(M, T, V, H, W), 256-byte aligned.
 * flags, all for measurements: MVD_RENDER_LOAD_FIRST: a plain load of the key before the atomic, which is skipped when the key has lost
 * already (measured slower, profiles/mesh_render.txt; the bits are the same).  The stages can be run apart on one workspace: MVD_RENDER_KEEP_PROJECT (the workspace still holds the screen vertices of these arguments: not projected again),
 * MVD_RENDER_KEEP_KEYS (it still holds the keys: not rasterised again), MVD_RENDER_NO_RESOLVE (the maps are not written). */
#define MVD_CULL_NONE 0
#define MVD_CULL_BACK 1
#define MVD_CULL_FRONT 2
#define MVD_RENDER_LOAD_FIRST 1
#define MVD_RENDER_KEEP_PROJECT 16
#define MVD_RENDER_KEEP_KEYS 32
#define MVD_RENDER_NO_RESOLVE 64
size_t mvd_mesh_render_workspace_bytes(long long M, long long T, int V, int H, int W);
int mvd_mesh_render_f32(const float* vertices, long long M, const int* triangles, long long T, const float* colors,
                        const float* matrices, int V, int H, int W, float near_plane, int cull, int max_small, int flags, float* depth,
                        int* triangle, float* bary, float* out_colors, float* normals, void* workspace, size_t workspace_bytes,
                        mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh clean-up: the connected components of a triangle mesh, their table, the filter that drops components, and area-weighted
 * vertex normals.  The reference has NO counterpart: the definition is robustmvd_amd/mesh_clean.py (components_numpy,
 * component_table_numpy, clean_numpy, vertex_normals_numpy) and DESIGN.md.
 *
 * triangles (T,3) int32 with 0 <= index < M (the caller checks the range; a triangle with an index outside it is skipped by every
 * entry), vertices (M,3) float32; M, T <= 2^31 - 1.  Two vertices are connected when a triangle names both; degenerate and duplicate
 * triangles connect like any other.  Every kernel is one bounded pass: none waits for another thread, the rounds are the caller's
 * loop.  The only atomics are 32-bit integer min / add; every float64 sum has a fixed order: two calls give the same bits.
 *
 * mvd_mesh_hook_round: one round of min-label hooking with pointer jumping on label (M) int32.  flags: MVD_MESH_ROUND_FIRST starts a
 * labelling: label[v] = v and referenced[v] = 0, and the hook pass stores the byte 1 in referenced (M) for every vertex a triangle names.
 * Hook, per triangle (a,b,c): m = min over x of label[label[x]], lowered with atomicMin into label[label[x]] and label[x].  Shortcut,
 * per vertex: label[v] = label[label[v]].  Labels only decrease and every value is a vertex of the same component
 * (csrc/mesh_clean.hip).  changed (device, 4-byte aligned) is zeroed and receives 1 when a word changed.  The caller repeats the
 * round until changed stays 0, at most 2 ceil(log2(max(M,2))) + 4 times (mesh_clean.py: MAX_ROUNDS); then label[v] is the lowest
 * vertex index of v's component, a unique fixed point.  T == 0: one call, label[v] = v.  For measurements, the two launches apart:
 * MVD_MESH_ROUND_NO_SHORTCUT runs the hook alone (changed is zeroed first, as in a whole round), MVD_MESH_ROUND_NO_HOOK the shortcut
 * alone, which leaves changed as it is and only raises it: the two calls in this order are one round. */
#define MVD_MESH_ROUND_FIRST 1
#define MVD_MESH_ROUND_NO_HOOK 2
#define MVD_MESH_ROUND_NO_SHORTCUT 4
int mvd_mesh_hook_round(const int* triangles, long long T, long long M, int flags, int* label, unsigned char* referenced, int* changed,
                        mvd_stream_t stream);

/* From a converged labelling: the roots (referenced, label[v] == v) ranked in ascending vertex order give the component ids
 * 0 .. C-1; vertex_component (M) int32 = the id of label[v], -1 for an unreferenced vertex; num_components (device, 8-byte aligned)
 * receives C.  compact.h's ballot counts and two-level scan: no atomic decides an id.
 * workspace: mvd_mesh_component_rank_workspace_bytes(M), 256-byte aligned. */
size_t mvd_mesh_component_rank_workspace_bytes(long long M);
int mvd_mesh_component_rank(const int* label, const unsigned char* referenced, long long M, int* vertex_component,
                            long long* num_components, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* triangle_component (T) int32 = the component of the triangle's first vertex; num_vertices (C) int32 = the vertices of each
 * component (zeroed here; integer adds, one per wave and distinct component).  C: what mvd_mesh_component_rank gave. */
int mvd_mesh_component_table(const int* vertex_component, const int* triangles, long long T, long long M, long long C,
                             int* triangle_component, int* num_vertices, mvd_stream_t stream);

/* The fixed-order sums.  Between mvd_mesh_component_table and this entry the caller sorts triangle_component STABLY and keeps the
 * permutation: sorted_component (T) int32 ascending, perm (T) int64, perm[p] = the triangle at sorted position p.
 * num_triangles (C) int32 = the length of each component's segment.  area (C) float64, 8-byte aligned: the sum of the component's
 * triangle areas.  A triangle's area: e1 = p1 - p0, e2 = p2 - p0 in float64 from the float32 coordinates,
 * n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), area = 0.5 sqrt((nx nx + ny ny) + nz nz), one rounding per operation,
 * 0 where that is not finite.  A segment of at most 64 triangles is added in ascending triangle order by one lane.  A longer one by
 * a wave: the sorted positions are cut at multiples of 2048; a block of 2048 that lies inside the segment enters as its own sum
 * (256 interleaved partial sums, a xor tree per wave, the four waves in order); lane l adds items l, l + 64, ... of the segment's
 * head, its blocks and its tail, and the 64 sums meet in a xor tree.  The order depends on the segment's bounds alone.
 * workspace: mvd_mesh_component_sums_workspace_bytes(T, C), 256-byte aligned. */
size_t mvd_mesh_component_sums_workspace_bytes(long long T, long long C);
int mvd_mesh_component_sums_f64(const float* vertices, long long M, const int* triangles, long long T, const int* sorted_component,
                                const long long* perm, long long C, int* num_triangles, double* area, void* workspace,
                                size_t workspace_bytes, mvd_stream_t stream);

/* The filter.  A triangle stays when keep_component[triangle_component[t]] != 0 (keep_component (C) bytes; NULL: every triangle
 * stays, and triangle_component is not read).  A vertex stays when a kept triangle names it, or, with remove_unreferenced == 0,
 * always.  Kept triangles and kept vertices keep their order: two compact.h compactions with exact sizes, no atomic decides a
 * position.  One entry, two uses, as mvd_tsdf_extract_f32.  With out_triangles == NULL (then kept_triangles and vertex_remap too) it
 * counts only.  With them it also writes vertex_remap (M) int32: the new index of a vertex or -1;  kept_triangles: the old index of
 * each kept triangle;  out_triangles: its indices through the remap; a slot at or past max_triangles is not written.  counts
 * (device, 16-byte aligned) always receives two int64: the kept vertices and the kept triangles.  counted != 0: the workspace still
 * holds the counts of an earlier call with these arguments, and they are not formed again.
 * workspace: mvd_mesh_filter_workspace_bytes(M, T), 256-byte aligned. */
size_t mvd_mesh_filter_workspace_bytes(long long M, long long T);
int mvd_mesh_filter(const int* triangles, long long T, long long M, const int* triangle_component, const unsigned char* keep_component,
                    long long C, int remove_unreferenced, int counted, int* out_triangles, int* kept_triangles, int* vertex_remap,
                    long long max_triangles, long long* counts, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* A per-vertex array through the remap: dst[vertex_remap[v]] = src[v], rows of k float32 (1 <= k <= 65536), bit for bit, for every
 * v with 0 <= vertex_remap[v] < max_rows.  src (M,k), dst (max_rows,k).  One lane per value: M k <= 2^31 - 1. */
int mvd_mesh_gather_rows_f32(const float* src, const int* vertex_remap, long long M, int k, long long max_rows, float* dst,
                             mvd_stream_t stream);

/* Area-weighted vertex normals.  The caller sorts the 3 T corner keys triangles[t][k] STABLY: sorted_vertex (3T) int32 ascending,
 * perm (3T) int64, perm[p] = the corner 3 t + k at sorted position p.  normals (M,3) float32 = the sum over the vertex's corners, in
 * ascending (t, k) order, of the un-normalised cross product n of triangle t (mvd_mesh_component_sums_f64's), in float64, divided by
 * its length sqrt((sx sx + sy sy) + sz sz) and rounded to float32; (0,0,0) where the length is zero or not finite or no triangle
 * names the vertex.  A triangle that names a vertex twice adds twice.  One lane per vertex: a binary search for its run, then the
 * run in order.  No atomics.  3 T <= 2^31 - 1. */
int mvd_mesh_vertex_normals_f32(const float* vertices, long long M, const int* triangles, long long T, const int* sorted_vertex,
                                const long long* perm, float* normals, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh simplification: vertex clustering on a uniform grid with quadric-error placement (Lindstrom 2000).  The reference has NO
 * counterpart: the definition is robustmvd_amd/mesh_simplify.py (cluster_numpy, cluster_quadrics_numpy, place_numpy,
 * simplify_numpy) and DESIGN.md, restated here.  No entry uses an atomic.  Every float64 sum is a segment sum in ONE fixed order: a
 * segment of at most 64 items is added one item after the other from +0.0; a longer one by 64 lanes, lane l the items l, l + 64, ...
 * in that order from +0.0, and the 64 sums meet in the xor tree v += shuffle_xor(v, s), s = 32 .. 1.  The order depends on the
 * segment's length alone and the library is built without contraction: two runs give the same bits.
 * The callers' sorts are STABLE.  After these entries the kept triangles and the referenced clusters are compacted by
 * mvd_mesh_filter (every triangle its own component, the keep bytes as verdicts) and rows move through mvd_mesh_gather_rows_f32. */

/* Cluster ids.  No counterpart in the reference.  keys (M) int64 ascending: the vertices' cell keys of mvd_cloud_cell_keys_f32
 * sorted, the invalid vertices' INT64_MAX last;  perm (M) int64: perm[p] = the vertex at sorted position p.  The clusters are the
 * runs of equal valid keys, numbered in key order (a compact.h compaction of the runs' heads: no atomic decides a number).
 * vertex_cluster (M) int32: the cluster of every vertex, -1 for an invalid one;  cluster_start (M + 1 entries, K + 1 written): the
 * first sorted position of each cluster, cluster_start[K] = the number of valid vertices;  cluster_key (M entries, K written);
 * num_clusters (device, 8-byte aligned): K.  No float sum.
 * workspace: mvd_mesh_cluster_ids_workspace_bytes(M), 256-byte aligned. */
size_t mvd_mesh_cluster_ids_workspace_bytes(long long M);
int mvd_mesh_cluster_ids(const long long* keys, const long long* perm, long long M, int* vertex_cluster, int* cluster_start,
                         long long* cluster_key, long long* num_clusters, void* workspace, size_t workspace_bytes, mvd_stream_t stream);

/* Segment means.  No counterpart in the reference.  rows (M,k) float32, 1 <= k <= 65536, M k <= 2^31 - 1.  means (K,k) float64:
 * per column the sum of float64(rows[perm[p]]) over the cluster's sorted positions p in ascending order (= ascending vertex index)
 * in the segment order above, divided by the number of positions.  One lane per cluster, the wave for a cluster of more than 64. */
int mvd_mesh_cluster_means_f64(const float* rows, const long long* perm, const int* cluster_start, long long K, long long M, int k,
                               double* means, mvd_stream_t stream);

/* Triangle triples.  No counterpart in the reference; no sum.  Per triangle: triples (T,3) int32, the clusters of its vertices
 * rotated so that the smallest comes first, and alive (T) bytes = 1, when the three vertices are valid and the three clusters
 * pairwise different; otherwise (-1,-1,-1) and 0.  corner_key (T,3) int32: the cluster of each corner, or K for every corner of a
 * triangle with an invalid vertex (the sentinel sorts last).  3 T <= 2^31 - 1. */
int mvd_mesh_cluster_triples(const int* triangles, long long T, long long M, const int* vertex_cluster, long long K, int* triples,
                             unsigned char* alive, int* corner_key, mvd_stream_t stream);

/* Quadrics.  No counterpart in the reference.  The caller sorts the 3 T corner keys stably: sorted_cluster (3T) int32 ascending,
 * perm (3T) int64, perm[p] = the corner 3 t + j at sorted position p.  Per corner, float64 from the float32 coordinates, one
 * rounding per operation: e1 = p1 - p0, e2 = p2 - p0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
 * q = p0 - ctr with ctr = (idx + 0.5) * cell + origin per axis from the cluster's key, d = -((nx qx + ny qy) + nz qz), and the ten
 * terms nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d, d d.  quadrics (K,10) float64: the sums over each cluster's
 * corners in ascending sorted position (= ascending (t, j)) in the segment order above; zeros for a cluster without a corner.
 * The segments come from a binary search per cluster.  3 T <= 2^31 - 1.
 * workspace: mvd_mesh_cluster_quadrics_workspace_bytes(K), 4-byte aligned. */
size_t mvd_mesh_cluster_quadrics_workspace_bytes(long long K);
int mvd_mesh_cluster_quadrics_f64(const float* vertices, long long M, const int* triangles, long long T, const int* sorted_cluster,
                                  const long long* perm, const long long* cluster_key, long long K, double origin_x, double origin_y,
                                  double origin_z, double cell, double* quadrics, void* workspace, size_t workspace_bytes,
                                  mvd_stream_t stream);

/* Placement.  No counterpart in the reference; no sum.  One lane per cluster.  A cluster of one vertex: that vertex's bits,
 * placed = 2.  Otherwise, with quadrics != NULL: lam = regularisation ((a00 + a11) + a22), A' = A + lam I,
 * r = -b + lam (mean - ctr), x = adj(A') r / det(A') with the cofactors and the associations of mesh_simplify.py's step 5; the
 * vertex is float32(ctr + x), placed = 1, when lam > 0, det is finite and > 0, every x_i is finite and |x_i| <= 0.5 cell.
 * Otherwise, and always with quadrics == NULL: float32(mean), placed = 0.  out_vertices (K,3) float32, placed (K) bytes. */
int mvd_mesh_cluster_place_f32(const double* quadrics, const double* means, const int* cluster_start, const long long* cluster_key,
                               const long long* perm, const float* vertices, long long K, long long M, double origin_x, double origin_y,
                               double origin_z, double cell, double regularisation, float* out_vertices, unsigned char* placed,
                               mvd_stream_t stream);

/* Duplicates.  No counterpart in the reference; no sum.  perm (T) int64: the triangles ordered so that the alive triples ascend
 * lexicographically, equal triples in ascending triangle index (two stable sorts: by the third index, then by the 64-bit pair of
 * the first two).  keep (T) bytes: 1 for an alive triangle whose predecessor in that order is dead or has another triple, 0 for
 * every other triangle. */
int mvd_mesh_cluster_mark_first(const int* triples, const unsigned char* alive, const long long* perm, long long T, unsigned char* keep,
                                mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh evaluation: the truncated distance from points to a triangle mesh, and deterministic covering samples of its surface.  The
 * reference has NO counterpart: the definition is robustmvd_amd/mesh_eval.py (mesh_distance_numpy, mesh_grid_pairs_numpy,
 * sample_mesh_numpy) and DESIGN.md, restated here.
 *
 * vertices (M,3) float32, triangles (T,3) int32; M, T and every other count <= 2^31 - 1.  A triangle is INVALID if an index is
 * outside [0, M) or a vertex has a non-finite coordinate: it matches no query and gets no sample.  A degenerate finite triangle
 * (zero area) is valid and acts as its segment or point.
 *
 * Distance of a query q to a triangle A, B, C, everything relative to the query (the values must survive coordinates of 10^3):
 *   a = A - q, b = B - q, c = C - q;  E0 = B - A, E1 = C - B, E2 = A - C;  dot(u,v) = (u.x v.x + u.y v.y) + u.z v.z
 *   seg(p, E): ee = dot(E,E); t = clamp(-dot(p,E) / ee, 0, 1), t = 0 when ee == 0; r = p + t E; the result is dot(r,r)
 *   d2 = min(seg(a,E0), seg(b,E1), seg(c,E2));  n = E0 x E1, nn = dot(n,n)
 *   inside iff nn > 0 and dot(n, a x E0) >= 0 and dot(n, b x E1) >= 0 and dot(n, c x E2) >= 0;  inside: d2 = min(d2, dot(n,a)^2 / nn)
 *   dist(q, triangle) = sqrt(d2)
 * (The kernel forms the sums as FMAs and the two divisions with a 1-ulp reciprocal.)  Truncated nearest triangle, max_dist > 0:
 *   dist[i]  = min(max_dist, min over valid triangles)   (max_dist for an invalid query, T = 0 or no valid triangle)
 *   index[i] = the triangle of that minimum when it is < max_dist (strict), else -1
 * Among triangles with an equal d2, as the device computed it, the smallest triangle index wins.  No atomic decides a value: two
 * calls give the same bits.
 *
 * The triangle grid.  Cells, keys and inv are mvd_cloud_cell_keys_f32's.  A valid triangle is entered into every cell of its
 * axis-aligned box, per axis floor((double(min_a) - origin_a) * inv) .. floor((double(max_a) - origin_a) * inv), no dilation (the
 * caller checks that every index is in [0, 2^21 - 1); the device clamps).
 * mvd_mesh_cell_counts_f32: counts (T) int64 = the cells of each triangle's box, 0 for an invalid triangle (saturating at 2^31). */
int mvd_mesh_cell_counts_f32(const float* vertices, long long M, const int* triangles, long long T, double origin_x, double origin_y,
                             double origin_z, double inv, long long* counts, mvd_stream_t stream);

/* The pair list: ends (T) int64 = the INCLUSIVE prefix sums of the counts (the caller's), P = ends[T-1] <= 2^31 - 1.  keys (P) int64
 * and pair_triangle (P) int32: one pair per cell of every valid triangle's box, in triangle order, inside a triangle x-major, then
 * y, then z.  One lane per pair: the triangle by an upper-bound search in ends, the cell from the rank inside the box.  Between
 * this entry and mvd_mesh_records_f32 the caller sorts the keys STABLY and keeps the permutation. */
int mvd_mesh_pairs_f32(const float* vertices, long long M, const int* triangles, long long T, const long long* ends, long long P,
                       double origin_x, double origin_y, double origin_z, double inv, long long* keys, int* pair_triangle,
                       mvd_stream_t stream);

/* records (P,12) float32, 16-byte aligned, 48 bytes per sorted pair: sorted position i holds the vertices A, B, C (nine floats) of
 * triangle pair_triangle[perm[i]], that index as the bits of the tenth float, and two zeros. */
int mvd_mesh_records_f32(const float* vertices, long long M, const int* triangles, long long T, const int* pair_triangle,
                         const long long* perm, long long P, float* records, mvd_stream_t stream);

/* query_records (n,4): mvd_cloud_grid_build_f32's, keyed with this origin and inv (the queries' order only decides how well a wave's
 * queries share cells); triangle_records (P,12) and pair_keys (P): the sorted pair list.  The cell edge 1 / inv must be at least
 * max_dist (1 + 2^-10): then the 3 x 3 x 3 cells around a query's hold every triangle within max_dist (the argument is in
 * csrc/mesh_eval.hip).  dist (n) and index (n) are written in the queries' ORIGINAL order.  n == 0 writes nothing; P == 0 truncates
 * every query. */
int mvd_mesh_nearest_f32(const float* query_records, long long n, const float* triangle_records, const long long* pair_keys,
                         long long P, double origin_x, double origin_y, double origin_z, double inv, float max_dist, float* dist,
                         int* index, mvd_stream_t stream);

/* Surface samples at a spacing s > 0, inv_s2 = 1.0 / (double(s) * double(s)) formed by the host.  A valid triangle with longest
 * squared edge L2 (float64 differences of the float32 coordinates, (dx^2 + dy^2) + dz^2) gets k = the smallest integer >= 1 with
 * k k >= L2 * inv_s2, found with integer correction steps (independent of how sqrt rounds; capped at 2^26), and k^2 samples: the
 * centroids of its k^2 congruent sub-triangles.  Rows i = 0 .. k-1; row i holds 2 (k - i) - 1 samples; position t in the row gives
 * j = t >> 1, down = t & 1 and the weights, each ONE double division,
 *   on B (3 i + 1 + down) / (3 k),   on C (3 j + 1 + down) / (3 k),   on A (3 (k - i - j) - 2 - 2 down) / (3 k);
 * the point is (wA A + wB B) + wC C in double, rounded once to float32 (no contraction: numpy forms the same bits); attributes
 * (M,channels) float32, NULL or with out_attributes, go through the same expression.  Every surface point is within 2 s / 3 of a
 * sample.  mvd_mesh_sample_counts_f32: counts (T) int64 = k^2, 0 for an invalid triangle (saturating at 2^31).
 * mvd_mesh_sample_f32: ends (T) = the INCLUSIVE prefix sums of the counts (the caller's), S = ends[T-1]; points (S,3), sample_triangle
 * (S) int32, out_attributes (S,channels), in triangle order, then sample order.  One lane per sample: the triangle by an upper-bound
 * search in ends, the row by an integer square root. */
int mvd_mesh_sample_counts_f32(const float* vertices, long long M, const int* triangles, long long T, double inv_s2, long long* counts,
                               mvd_stream_t stream);
int mvd_mesh_sample_f32(const float* vertices, long long M, const int* triangles, long long T, const float* attributes, int channels,
                        const long long* ends, long long S, double inv_s2, float* points, int* sample_triangle, float* out_attributes,
                        mvd_stream_t stream);

/* layout helpers used at the operator-level boundary (reference tensors are NCHW / NCDHW) */
int mvd_nchw_to_nhwc_f32(const float* src, float* dst, int N, int C, long long HW, mvd_stream_t stream);
int mvd_nhwc_to_nchw_f32(const float* src, float* dst, int N, int C, long long HW, mvd_stream_t stream);

/* Zeroes the border of a zero-bordered channel-last map y (B, h + 3, w + 3, C), C a multiple of 4 (K3's staging layout,
 * MVD_FEAT_NHWC_BORDER): row 0, rows h + 1 and h + 2, column 0, columns w + 1 and w + 2.  The interior (rows 1 .. h, columns 1 .. w)
 * is not touched: its producer writes it. */
int mvd_zero_border_nhwc_f32(float* y, int B, int h, int w, int C, mvd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVD_H_ */
