/*
 * omnifusion.h — C ABI of libomnifusion_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the reference's `equi_pers` hot path.  Every entry point is
 * `extern "C"`, takes plain device pointers + sizes + a hipStream_t passed as void*,
 * allocates nothing the caller can see, never synchronises the host and returns an
 * int status (OMNI_OK == 0); omni_last_error() returns the thread-local message.
 * The reference has no FFI of its own (it is pure Python on stock PyTorch ops), so
 * each function cites the reference *Python* interface it replaces.
 *
 * Tensor layouts (all dense, row-major, last index fastest):
 *   ERP image          [B, C, H, W]
 *   patches, reference [B, C, ph, pw, N]   OMNI_LAYOUT_BCHWN  (N innermost,
 *                      equi2pers_v3.py:112-113; what the public Python API returns)
 *   patches, planar    [B, N, C, ph, pw]   OMNI_LAYOUT_BNCHW  (patch-major; what the
 *                      model uses internally so that no N-innermost tensor is ever
 *                      materialised between the sampler, the network and the blender)
 *   patches, NHWC      [B, N, ph, pw, C]   OMNI_LAYOUT_BNHWC  (network activations)
 */
#ifndef OMNIFUSION_H_
#define OMNIFUSION_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMNI_VERSION 200

enum omni_status {
    OMNI_OK = 0,
    OMNI_ERR_INVALID = 1,   /* bad nrows / shape / layout / null pointer  -> Python ValueError  */
    OMNI_ERR_HIP = 2,       /* a HIP runtime call failed                  -> Python RuntimeError */
    OMNI_ERR_UNSUPPORTED = 3
};

enum omni_layout { OMNI_LAYOUT_BCHWN = 0, OMNI_LAYOUT_BNCHW = 1, OMNI_LAYOUT_BNHWC = 2,
                   OMNI_LAYOUT_BCHNW = 3 /* [B, C, h, N*w]: views side by side along the width, free-view sampling only */ };
enum omni_dtype { OMNI_F32 = 0, OMNI_F16 = 1 };

typedef void* omni_stream_t;            /* hipStream_t */
typedef struct omni_geometry omni_geometry_t;

int omni_version(void);
const char* omni_last_error(void);

/* Tuning options (tile shapes, kernel selection, cache size — csrc/omni_internal.h `OmniOptions`; each also has an
 * OMNI_<NAME> environment variable that is read ONCE, when the library first needs it).  No option changes a result
 * bit except "splitk_max" (K summation order).  Unknown name -> OMNI_ERR_INVALID.  No reference counterpart (the
 * reference has no tunables below PyTorch); used by tests/ and tools/ to sweep kernel variants. */
int omni_set_option(const char* name, int value);
int omni_get_option(const char* name, int* value);

/* Number of patches for an nrows preset (3,4,5,6 -> 10,18,26,46), -1 otherwise.
 * equi2pers_v3.py:32-47 / pers2equi_v3.py:36-51 (the reference raises
 * UnboundLocalError for any other value). */
int omni_num_patches(int nrows);

/* Patch centres in [-1,1] (`center_p`, equi2pers_v3.py:81-82) written to HOST memory
 * center_p[N*2]; `which` = 0 equi2pers table, 1 pers2equi table (nrows=3 differs). */
int omni_patch_centers(int nrows, int which, float* center_p_host);

/*
 * Geometry handle: the constants of one (nrows, fov, patch size, ERP size) configuration
 * resident on the current device — patch-centre trig, per-row/column trig of the ERP
 * grid and the per-tile candidate-patch masks of pers2equi.  A few KB; replaces the
 * reference's per-call CPU grid build + H2D (equi2pers_v3.py:24-109) and its 0.5 GB
 * ./grid/<layer_name>.pth tables (pers2equi_v3.py:24-29,155-167).  The convenience
 * entry points below look handles up in an internal per-device, mutex-protected cache,
 * so callers that mirror the reference's free functions never see this type.
 */
int omni_geometry_create(omni_geometry_t** out, int nrows, float fov_h, float fov_w,
                         int ph, int pw, int H, int W, omni_stream_t stream);
void omni_geometry_destroy(omni_geometry_t* g);
/* The internal cache is an LRU capped at option "geom_cache_max" (default 16) handles; evicted / cleared handles are
 * destroyed only after their device has drained.  omni_geometry_cache_size: handles currently cached (all devices). */
void omni_geometry_cache_clear(void);
int omni_geometry_cache_size(void);

/*
 * equi2pers — replaces equi_pers/equi2pers_v3.py:20 `equi2pers(erp_img, fov, nrows, patch_size)`
 * (grid build :24-109, F.grid_sample bilinear/border/align_corners=True :111, unfold+reshape
 * :112-113).  erp [B,C,H,W] -> pers in `layout`.  dtype: OMNI_F32 or OMNI_F16 storage
 * (arithmetic is fp32 either way).
 */
int omni_equi2pers(const void* erp, void* pers, int dtype, int B, int C, int H, int W,
                   int ph, int pw, int nrows, float fov_h, float fov_w, int layout,
                   omni_stream_t stream);

/* The other three return values of equi2pers (equi2pers_v3.py:115-122): xyz [N,3,ph,pw]
 * unit rays from the UNWRAPPED lon/lat, uv [N,2,ph,pw] (the reference's scrambled strip
 * reshape), both fp32 device buffers; either may be NULL. */
int omni_equi2pers_aux(float* xyz, float* uv, int ph, int pw, int nrows, float fov_h, float fov_w,
                       omni_stream_t stream);

/*
 * pers2equi — replaces equi_pers/pers2equi_v3.py:16
 * `pers2equi(pers_img, fov, nrows, patch_size, erp_size, layer_name)` (tables :109-152,
 * gathers :174-177, mask/threshold/L1-normalise/blend :179-196).  pers in `layout` -> erp
 * [B,C,H,W].  `layer_name` was only the reference's cache-file key and has no counterpart.
 */
int omni_pers2equi(const void* pers, void* erp, int dtype, int B, int C, int ph, int pw,
                   int H, int W, int nrows, float fov_h, float fov_w, int layout,
                   omni_stream_t stream);

/* [B,C,ph,pw,N] (OMNI_LAYOUT_BCHWN, the reference's N-innermost patch tensor, equi2pers_v3.py:112-113) -> [B,N,C,ph,pw]
 * (OMNI_LAYOUT_BNCHW), one coalesced pass.  The blend on planar patches is 5x faster than on the N-innermost tensor (every cache
 * line of which is shared by all N patches): conversion + omni_pers2equi(..., OMNI_LAYOUT_BNCHW) is what the drop-in pers2equi()
 * runs for reference-layout inputs (same result bits as omni_pers2equi(..., OMNI_LAYOUT_BCHWN)). */
int omni_patches_to_planar(const void* src, void* dst, int dtype, int B, int C, int ph, int pw, int N, omni_stream_t stream);

/*
 * Fused confidence blend — replaces model/spherical_model.py:307-311 (two pers2equi calls +
 * zero-safe division):  out = P(pred_w) / (P(conf) + 1e-8*[P(conf) <= 1e-8]),
 * pred_w = relu(pred)*sigmoid(weight_pred), conf = sigmoid(weight_pred), both C=1 patch
 * tensors in `layout`; out [B,1,H,W] fp32.
 */
int omni_pers2equi_conf(const void* pred_w, const void* conf, float* out, int dtype, int B,
                        int ph, int pw, int H, int W, int nrows, float fov_h, float fov_w,
                        int layout, omni_stream_t stream);

/* Explicit-handle forms of the three operators (same semantics, no cache lookup). */
int omni_equi2pers_g(const omni_geometry_t* g, const void* erp, void* pers, int dtype, int B, int C,
                     int layout, omni_stream_t stream);
int omni_pers2equi_g(const omni_geometry_t* g, const void* pers, void* erp, int dtype, int B, int C,
                     int layout, omni_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Network operators (rows a3-a8 of SURVEY.md 8a).  Activations are NHWC fp32 over M = B*N patches
 * ([M,H,W,C]); eval-mode BatchNorm is folded into the weights by the caller at load time.  The
 * reference runs these as Conv3d(k,k,1)/BatchNorm3d/Linear modules over [B,C,P,P,N] tensors.
 * ---------------------------------------------------------------------------------------------- */
enum omni_act { OMNI_ACT_NONE = 0, OMNI_ACT_RELU = 1, OMNI_ACT_GELU = 2 };

/* Backward of the two operators: the vector-Jacobian products that autograd derives from
 * F.grid_sample (equi_pers/equi2pers_v3.py:111) and from the indexing gathers of equi_pers/pers2equi_v3.py:174-196 in the
 * reference's training scripts (train_erp_depth.py:255-300).  Both operators are linear in the image.  fp32 only; the output
 * gradient is overwritten; layouts as in the forward (grad_pers: OMNI_LAYOUT_BCHWN or _BNCHW).  No atomics: the result of a call is
 * a function of its inputs and the geometry handle only (fixed summation order).  The first backward of a geometry builds its tables
 * (synchronises the stream once); the first call of a (geometry, stream, B * C) allocates scratch the size of the incoming gradient
 * — OMNI_ERR_UNSUPPORTED if that first call happens while the stream is being captured (run the shape once before capturing). */
int omni_equi2pers_bwd(const void* grad_pers, void* grad_erp, int dtype, int B, int C, int H, int W,
                       int ph, int pw, int nrows, float fov_h, float fov_w, int layout, omni_stream_t stream);
int omni_pers2equi_bwd(const void* grad_erp, void* grad_pers, int dtype, int B, int C, int ph, int pw,
                       int H, int W, int nrows, float fov_h, float fov_w, int layout, omni_stream_t stream);
/* dst[M,Ho,Wo,Cout] = act(conv(src1 ++ src2 (channel concat), wt) + bias + res) on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32).  wt: [Cout][KH*KW*(C1+C2)], k ordered (ky,kx,c).  C1,C2,Cout multiples of 32.
 * Replaces: encoder BasicBlock convs model/spherical_model.py:122-167,257-261 (residual+ReLU fused), decoder
 * ConvBnReLU_v2 :29-37,274-302 incl. torch.cat :275,282,289,296, `down` :211,263, and every nn.Linear of
 * model/blocks.py:19-21,43-46 (H=W=KH=KW=1; GELU of :20 and the residual adds of :86-87 fused). */
int omni_conv2d_nhwc_f32(const float* src1, const float* src2, const float* wt, const float* bias,
                         const float* res, float* dst, int M, int H, int W, int C1, int C2, int Cout,
                         int KH, int KW, int stride, int pad, int act, omni_stream_t stream);
/* Same, split along K into `splitk` ranges (workspace ws: splitk*rows*Cout floats) and reduced by a deterministic
 * second pass: for problems too small to fill the 256 CUs (layer4, de_conv0_x, the transformer's nn.Linear layers at
 * B*N rows).  omni_conv2d_splitk_plan(rows, Cout, ksteps) returns the factor the library recommends for `rows` output
 * pixels (ksteps = KH*KW*(C1+C2)/32); plan with a nominal batch to keep results bit-identical across batch sizes. */
int omni_conv2d_splitk_plan(long long rows, int Cout, int ksteps);
int omni_conv2d_nhwc_f32_ws(const float* src1, const float* src2, const float* wt, const float* bias,
                            const float* res, float* dst, int M, int H, int W, int C1, int C2, int Cout,
                            int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                            omni_stream_t stream);
/* The same operator with the products on the fp16 matrix cores at fp32-class accuracy ("f16x3"): every operand is split
 * into a pair of halfs x = hi + lo*2^-11 and a product block is three v_mfma_f32_32x32x16_f16 (3/16 of the fp32-MFMA
 * time, max error ~3e-6).  Activations, bias, residual and output stay fp32 NHWC (the A tile is split on its way into
 * LDS); wt16 is the weight matrix split once at load time: halfs [Cout][KH*KW*(C1+C2)/32][hi32|lo32],
 * hi = fp16(w) (0 below 2^-14), lo = fp16((w - hi) * 2048). */
int omni_conv2d_nhwc_f16x3_ws(const float* src1, const float* src2, const void* wt16, const float* bias,
                              const float* res, float* dst, int M, int H, int W, int C1, int C2, int Cout,
                              int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                              omni_stream_t stream);
/* The single-product form ("f16x1"): an operand is hi alone, a product block ONE v_mfma_f32_32x32x16_f16 with fp32
 * accumulation — the arithmetic of mixed-precision training: fp16 operands, fp32 sums, about 2^-11 relative error per operand.  wt16 is the
 * hi-only image of omni_conv2d_split_weights_f16x1: halfs [Cout][KH*KW*(C1+C2)].  Same operator, shapes, split-K and rejections. */
int omni_conv2d_nhwc_f16x1_ws(const float* src1, const float* src2, const void* wt16, const float* bias,
                              const float* res, float* dst, int M, int H, int W, int C1, int C2, int Cout,
                              int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                              omni_stream_t stream);
/* The same operator with SPLIT-HALF ("SH") activations: per pixel and per group of 32 channels a tensor stores 32 hi
 * halfs then 32 lo halfs (x = hi + lo*2^-11; 128 bytes per group = the footprint of 32 floats).  The producer splits
 * once, consumers stream tiles straight into LDS by LDS-DMA.  src1 and src2 are SH tensors; fmt bit 0: dst is SH
 * (else fp32 NHWC), fmt bit 1: res is fp32 NHWC (else SH), fmt bit 2: latency form — the caller runs so few images (one panorama) that the
 * kernel choice for 16-pixel-wide images should stay with the im2col tiles (results equal up to the K summation order) and the epilogue with
 * the direct 8-byte stores (same bits); wt16 as above.
 * fmt bit 3 (value 8): "f16x1" — ONE v_mfma_f32_32x32x16_f16 per product block, src_hi . wt_hi with fp32 accumulation: the lo halves of
 * the activations and of wt16 stay in memory (same layouts, same sizes) but are not multiplied.  Every kernel form this operator dispatches
 * (whatever omni_set_option chose: tile sizes, ping-pong, loader waves, halo forms, split-K) has its f16x1 instantiation; bias, residual,
 * activation, split-K reduction and the SH split of the output are those of f16x3.  The mode is per call (no global state): calls of
 * both modes may be interleaved and may run on concurrent streams.  Accuracy: ~1e-3 relative per product (fp16 operands).
 * Entry points without an f16x1 form (omni_conv3x3_wino_sh_f16x3, omni_gemm_rows_sh_f16x3, omni_gemm_rows_ln_sh_f16x3,
 * omni_gemm_sh_f16x3_ln512_ws) return OMNI_ERR_UNSUPPORTED for fmt bit 3.
 * omni_sh_from_f32 / omni_sh_to_f32 convert n elements (n % 32 == 0). */
int omni_conv2d_sh_f16x3_ws(const void* src1, const void* src2, const void* wt16, const float* bias,
                            const void* res, void* dst, int fmt, int M, int H, int W, int C1, int C2, int Cout,
                            int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                            omni_stream_t stream);
/* Which kernel omni_conv2d_sh_f16x3_ws (has_post != 0: omni_conv2d_sh_f16x3_post_ws) would launch for these arguments under the options set at
 * the time of the call, without launching anything: host code only, no device needed.  Same argument checks and the same status codes as the
 * convolution itself (the pointer checks apart).  Writes 14 integers to out (n_out >= 14), in this order:
 *   family     0 conv_sh_kernel (im2col tiles) | 1 conv_pm_sh_kernel (position-major tiles) | 2 conv3x3_halo_sh_kernel | 3 halo2_sh_kernel
 *   bm, bn, wm, wn, nst, nl, pp    the tile kernel's template arguments: block tile, matrix waves, stages, loader waves, ping-pong
 *                                  (families 1 and 2: bn only, the output channels per block)
 *   th, iw     family 2: rows per block, image width of the whole-image forms or 0; family 3: iw
 *   grid_x, grid_y, threads        the launch
 *   splitk     the split-K factor in effect (the caller's, at most KH*KW*(C1+C2)/32, at least 1)
 * A template argument the family does not have is 0.  The arithmetic mode (fmt bit 3) does not enter the choice. */
int omni_conv2d_sh_plan(int fmt, int M, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, int splitk, int has_post,
                        int* out, int n_out);
/* The nn.Linear layers of ONE panorama's transformer (model/blocks.py:19-21,43-46 at 18 tokens): out[rows, N] =
 * act(x . W^T + bias + res) for rows <= 32.  x SH [rows, K], res fp32 [rows, N] or null, fmt bit 0: dst is SH
 * (else fp32).  K in {512, 2048}, N % 32 == 0.  Operands go straight into registers, K is split over the waves of a block and
 * summed in a fixed order: equal to omni_conv2d_sh_f16x3_ws (H = W = KH = KW = 1) up to fp32 rounding, not bit for bit.
 * wt16r is the weight matrix in FRAGMENT ORDER (a wave's load = one contiguous KiB): omni_gemm_rows_pack makes it, once at load
 * time, from wt16 [N][K/32][hi32|lo32] (same size). */
int omni_gemm_rows_sh_f16x3(const void* x, const void* wt16r, const float* bias, const float* res, void* dst, int fmt,
                            int rows, int K, int N, int act, omni_stream_t stream);
int omni_gemm_rows_pack(const void* wt16, void* wt16r, int N, int K, omni_stream_t stream);
/* LayerNorm (model/blocks.py:69,75: nn.LayerNorm(512), eps as given) + the following nn.Linear of one panorama's transformer in ONE launch:
 * x fp32 [rows <= 32, 512] is normalised by every block itself (the arithmetic of omni_layernorm512_sh), then multiplied as in
 * omni_gemm_rows_sh_f16x3 (K = 512).  Same bits as the two calls. */
int omni_gemm_rows_ln_sh_f16x3(const float* x, const float* ln_weight, const float* ln_bias, float eps, const void* wt16r, const float* bias,
                               const float* res, void* dst, int fmt, int rows, int N, int act, omni_stream_t stream);
/* F.interpolate(scale_factor 2, bilinear, align_corners=False) + ConvBnReLU (3x3, pad 1) of the decoder, model/spherical_model.py:
 * 279-301, in ONE kernel: the up-sampled tensor never exists.  src SH [M,Hl,Wl,C], dst [M,2Hl,2Wl,Cout] SH (fmt bit 0) or fp32;
 * 2Wl % 32 == 0 and 2Hl % 4 == 0 (else OMNI_ERR_UNSUPPORTED: omni_upsample_bilinear_sh + omni_conv2d_sh_f16x3_ws give the same bits).
 * fmt bit 3: f16x1 as for omni_conv2d_sh_f16x3_ws (the product takes the hi split of the up-sampled value). */
int omni_conv3x3_up2_sh_f16x3(const void* src, const void* wt16, const float* bias, void* dst, int fmt,
                              int M, int Hl, int Wl, int C, int Cout, int act, omni_stream_t stream);
/* de_conv4_0 AND the two heads in one pass over the widest tensor of the network (model/spherical_model.py:300-307: F.interpolate + ConvBnReLU 32 -> 32,
 * then pred (ReLU) / weight_pred (sigmoid), 3x3, 32 -> 1, and their product): a = relu(pred(y)) * (confidence ? sigmoid(weight_pred(y)) : 1),
 * c = sigmoid(weight_pred(y)); y = de_conv4_0's output never exists.  src SH [M,P/2,P/2,32]; heads_w16f from omni_heads_pack_f16x3; scratch of
 * omni_up2_heads_scratch_bytes(M, P) bytes; out_a / out_c planar [M,P,P] (out_c may be NULL).  Equal to omni_conv3x3_up2_sh_f16x3 + omni_heads_f32 up to
 * the fp32 summation order of the heads (whose products run f16x3 here).  Deterministic. */
size_t omni_up2_heads_scratch_bytes(int M, int P);
int omni_conv3x3_up2_heads_sh_f16x3(const void* src, const void* wt16, const float* bias, const void* heads_w16f, float bias_pred, float bias_weight,
                                    float* scratch, size_t scratch_bytes, float* out_a, float* out_c, int M, int P, int confidence, omni_stream_t stream);
/* The same operator with de_conv4_0 in f16x1 (see omni_conv2d_sh_f16x3_ws, fmt bit 3); the two heads' own products stay f16x3.  Same arguments. */
int omni_conv3x3_up2_heads_sh_f16x1(const void* src, const void* wt16, const float* bias, const void* heads_w16f, float bias_pred, float bias_weight,
                                    float* scratch, size_t scratch_bytes, float* out_a, float* out_c, int M, int P, int confidence, omni_stream_t stream);
/* w [2][9][32] fp32 (HOST memory) -> the 4 KB fragment-ordered f16x3 operand of omni_conv3x3_up2_heads_sh_f16x3 (HOST memory; copy it to the device). */
int omni_heads_pack_f16x3(const float* w_host, void* dst_host);
/* omni_conv2d_sh_f16x3_ws with `post` (fp32, post_elems = whole rows of Cout channels) added AFTER the activation, output row index
 * modulo its row count: `layer1 + point_feat` (model/spherical_model.py:258; point_feat [N,h,w,64] broadcast over the batch, or
 * full size) inside layer1's last convolution.  post = NULL: the plain operator.  Not combinable with split-K. */
int omni_conv2d_sh_f16x3_post_ws(const void* src1, const void* src2, const void* wt16, const float* bias,
                                 const void* res, void* dst, int fmt, int M, int H, int W, int C1, int C2, int Cout,
                                 int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                                 const float* post, size_t post_elems, omni_stream_t stream);
/* EXPERIMENTAL (round 6): Winograd F(2x2, 3x3) for the 3x3 stride-1 pad-1 convolutions of small images (model/spherical_model.py:122-143, layer3 / layer4 /
 * de_conv0: Conv3d (3,3,1) + BatchNorm3d + ReLU) — 16 matrix products per 2 x 2 output tile instead of 36.  omni_wino_input_sh: x SH [M,H,W,C] (H, W even) ->
 * V SH [16][M*H/2*W/2][C] = B^T d B per tile.  omni_conv3x3_wino_sh_f16x3: dst = act(conv3x3(x) + bias + res) from V and wt16 = the f16x3 split of
 * [Cout][16*C] (k = p*C + c) holding (G g G^T)[p]; multiply stage and output transform in one kernel (conv_sh_kernel<.., WINO>); splitk in {1,2,4} divides the
 * sixteen positions (ws: splitk * M*H*W * Cout floats).  Equal to omni_conv2d_sh_f16x3_ws up to rounding, not bit for bit. */
int omni_wino_input_sh(const void* src, void* V, int M, int H, int W, int C, omni_stream_t stream);
int omni_conv3x3_wino_sh_f16x3(const void* V, const void* wt16, const float* bias, const void* res, void* dst, int fmt,
                               int M, int H, int W, int C, int Cout, int act, int splitk, float* ws, size_t ws_bytes, omni_stream_t stream);
int omni_sh_from_f32(const float* src, void* dst, size_t n, omni_stream_t stream);
int omni_sh_to_f32(const void* src, float* dst, size_t n, omni_stream_t stream);
/* Range guard of the SH format: values with |x| > 65504 (the fp16 range) are SATURATED when an activation is split, and a
 * sticky per-device flag records it.  *flag = 1 if that happened on the current device since the flag was last cleared
 * (reset != 0 clears it).  Synchronises the device: diagnostic only.  The fp32 reference has no such limit
 * (model/spherical_model.py runs fp32 end to end): a checkpoint that trips the flag needs OMNI_NET_PRECISION=fp32. */
int omni_sh_overflow(int* flag, int reset);
/* The non-GEMM operators of the network, from here to omni_mlp_points_f32 (csrc/omni_net.hip).  All of them return OMNI_ERR_INVALID before any
 * launch for a null tensor (the two optional ones are named) or a dimension below 1; omni_maxpool3x3s2_f32 / omni_upsample_bilinear_f32 for C % 4 != 0
 * (four channels per thread); the SH forms for C % 32 != 0; omni_add_period_* for period == 0 (the SH form also unless total and period are multiples of 32). */
/* conv1 7x7 s2 p3 (3->64) + bn1 + ReLU, model/spherical_model.py:254.  src planar [M,3,P,P]
 * (OMNI_LAYOUT_BNCHW patches), wt [147][64] (k = (ky*7+kx)*3+c), dst NHWC [M,P/2,P/2,64]. */
int omni_stem_f32(const float* src, const float* wt, const float* bias, float* dst, int M, int P, omni_stream_t stream);
/* F.max_pool3d((3,3,1),(2,2,1),(1,1,0)), model/spherical_model.py:255 */
int omni_maxpool3x3s2_f32(const float* src, float* dst, int M, int H, int W, int C, omni_stream_t stream);
/* F.interpolate(bilinear, align_corners=False), model/spherical_model.py:271,279,286,293,300 */
int omni_upsample_bilinear_f32(const float* src, float* dst, int M, int H, int W, int C, int Ho, int Wo, omni_stream_t stream);
/* x[m,hw,c] += y[m,c]: the transformer token added as a channel bias, model/spherical_model.py:267-268 */
int omni_add_hw_f32(float* x, const float* y, int M, int HW, int C, omni_stream_t stream);
/* x[i] += y[i % period]: layer1 + point_feat, model/spherical_model.py:258 */
int omni_add_period_f32(float* x, const float* y, size_t total, size_t period, omni_stream_t stream);
/* The element-wise operators above on split-half (SH) activations (see omni_conv2d_sh_f16x3_ws): same arguments,
 * activation tensors in the SH layout (C % 32 == 0); the broadcast operand y and the stem's planar input stay fp32. */
int omni_stem_sh(const float* src, const float* wt, const float* bias, void* dst, int M, int P, omni_stream_t stream);
/* the stem as an implicit GEMM on the fp16 matrix cores (f16x3): wt16 = the folded filter bank [64][192], k = (c*7+ky)*8+kx
 * (kx = 7 and k >= 168 zero), split into [64][6][hi32|lo32]; P % 32 == 0 */
int omni_stem_sh_f16x3(const float* src, const void* wt16, const float* bias, void* dst, int M, int P, omni_stream_t stream);
/* the same stem in f16x1: one matrix instruction per product block, fp16(input) . wt_hi with fp32 accumulation.  Same arguments. */
int omni_stem_sh_f16x1(const float* src, const void* wt16, const float* bias, void* dst, int M, int P, omni_stream_t stream);
int omni_maxpool3x3s2_sh(const void* src, void* dst, int M, int H, int W, int C, omni_stream_t stream);
int omni_upsample_bilinear_sh(const void* src, void* dst, int M, int H, int W, int C, int Ho, int Wo, omni_stream_t stream);
/* conv3x3(F.interpolate(x, scale_factor 2, bilinear, align_corners=False), pad 1) from the nine 1x1 TAP PRODUCTS on the low-resolution map
 * (both operators are linear): y fp32 [M][Hl][Wl][9][Cout], y[..., t, co] = sum_ci W[co][t][ci] * x[..., ci] with t = ky*3 + kx — the result of
 * omni_conv2d_sh_f16x3_ws (1x1, 9*Cout outputs, no bias, fp32) on weights repacked tap-major, row t*Cout + co.  The kernel forms
 *   dst[q] = act(bias + sum_t [q + t - 1 inside the 2Hl x 2Wl map] * up2(y_t)[q + t - 1]),   dst SH [M][2Hl][2Wl][Cout],
 * reading y once (one image x 32 channels per block, staged in LDS), with the source index arithmetic of omni_upsample_bilinear_* and a fixed
 * summation order: deterministic, and an image's bits do not depend on M.  Values are saturated to the SH range (omni_sh_overflow reports it).
 * bias fp32 [Cout] or NULL; act OMNI_ACT_NONE or OMNI_ACT_RELU; tensors 16-byte aligned.
 * Cout % 32 != 0, Hl * Wl > 64 or another activation: OMNI_ERR_UNSUPPORTED (omni_upsample_bilinear_sh + omni_conv2d_sh_f16x3_ws compute the
 * same convolution); null tensors or an empty shape: OMNI_ERR_INVALID. */
int omni_up2_tapsum_sh(const float* y, const float* bias, void* dst, int M, int Hl, int Wl, int Cout, int act, omni_stream_t stream);
/* The same identity in ONE launch, for the 64 -> 64 decoder stages: the nine tap products are formed on the matrix cores (f16x3), parked in LDS as fp32 and
 * summed into register accumulators with omni_up2_tapsum_sh's arithmetic and fixed order — they never reach memory.  src SH [M][Hl][Wl][64]; wt16t: the
 * tap-major f16x3 weights [9*Cout][64], row t*Cout + co = W[co][t][:] (the operand of the two-launch form); bias fp32 [Cout] or NULL; dst SH [M][2Hl][2Wl][Cout];
 * fmt 1 (SH result; bit 2 accepted and ignored: one form for every batch).  Deterministic; an image's bits do not depend on M.  Values are saturated to the
 * SH range (omni_sh_overflow reports it).  Serves C == Cout == 64 with Wl == 32 and Hl % 8 == 0, or Hl == Wl == 16, no activation or ReLU; anything else
 * (f16x1, an fp32 result included): OMNI_ERR_UNSUPPORTED before any launch (omni_conv3x3_up2_sh_f16x3 computes the same convolution); null tensors, an empty
 * shape, channels that are no multiple of 32 or tensors not 16-byte aligned: OMNI_ERR_INVALID. */
int omni_conv3x3_up2_taps_sh_f16x3(const void* src, const void* wt16t, const float* bias, void* dst, int fmt,
                                   int M, int Hl, int Wl, int C, int Cout, int act, omni_stream_t stream);
int omni_add_hw_sh(void* x, const float* y, int M, int HW, int C, omni_stream_t stream);
int omni_add_period_sh(void* x, const float* y, size_t total, size_t period, omni_stream_t stream);
/* nn.LayerNorm(512) with an SH result, and the attention core on a fused q|k|v projection [B*N, 1536] (q at column 0,
 * k at 512, v at 1024; heads of 128) with an SH result: the f16x3 GEMMs of the transformer consume them directly. */
int omni_layernorm512_sh(const float* x, const float* g, const float* b, void* y, int rows, float eps, omni_stream_t stream);
/* A lone panorama's fc2 (K = 2048, <= 32 rows) in K slices: N / 32 x slices blocks stream the weights instead of N / 32; each slice's RAW partial sums go to
 * parts[slice][rows][N] (fp32).  The consumer adds them up: omni_gemm_rows_ln_parts_sh_f16x3 (x = sum parts + pbias + pres -> xout, then LayerNorm + the rows
 * GEMM of omni_gemm_rows_ln_sh_f16x3: the next Transformer_Block's norm1 + qkv, model/blocks.py:83-88) or omni_splitk_reduce_ln512 (encoder_norm,
 * model/spherical_model.py:186).  slices in {1, 2, 4}. */
int omni_gemm_rows_slices_sh_f16x3(const void* x, const void* wt16r, float* parts, int rows, int K, int N, int slices, omni_stream_t stream);
int omni_gemm_rows_ln_parts_sh_f16x3(const float* parts, int nparts, const float* pbias, const float* pres, float* xout,
                                     const float* ln_weight, const float* ln_bias, float eps, const void* wt16r, const float* bias,
                                     void* dst, int fmt, int rows, int N, int act, omni_stream_t stream);
int omni_splitk_reduce_ln512(const float* parts, int nparts, const float* bias, const float* res, float* tok, const float* ln_weight, const float* ln_bias,
                             float eps, void* y, int fmt, int rows, omni_stream_t stream);
/* x = x + mlp.fc2(h) FOLLOWED BY the next LayerNorm (model/blocks.py:83-88 into the next block's norm1, or into encoder_norm,
 * model/spherical_model.py:180-187) as a split-K GEMM whose second pass normalises: tok [rows,512] fp32 = x . wt16^T + bias + res (res fp32),
 * y = LayerNorm(tok) as SH (fmt bit 0) or fp32.  splitk >= 2; ws as for omni_conv2d_sh_f16x3_ws.  The bits of the separate calls, one launch fewer. */
int omni_gemm_sh_f16x3_ln512_ws(const void* x, const void* wt16, const float* bias, const float* res, float* tok, const float* ln_g, const float* ln_b,
                                float eps, void* y, int fmt, int rows, int K, int splitk, float* ws, size_t ws_bytes, omni_stream_t stream);
int omni_attention_qkv_sh(const float* qkv, void* out, int B, int N, omni_stream_t stream);
/* tokens: reshape(bs,-1,N).transpose(1,2) of the `down` output + pos_emb, model/spherical_model.py:264,181 */
int omni_token_pack_f32(const float* d, const float* pos, float* tok, int M, int N, int HW, int C, omni_stream_t stream);
/* nn.LayerNorm(512), model/blocks.py:74,81 (eps 1e-5) and model/spherical_model.py:173 (eps 1e-6) */
int omni_layernorm512_f32(const float* x, const float* g, const float* b, float* y, int rows, float eps, omni_stream_t stream);
/* softmax(q k^T * 128^-1/2) v, 4 heads x 128 over N <= 64 tokens, model/blocks.py:52-62.  q [B*N,512], kv [B*N,1024] */
int omni_attention_f32(const float* q, const float* kv, float* out, int B, int N, omni_stream_t stream);
/* pred (ReLU) and weight_pred (sigmoid) 3x3 heads, model/spherical_model.py:304-307.  x NHWC [M,P,P,32], w [2][9][32];
 * out_a = relu(pred) * (confidence ? sigmoid(weight) : 1), out_c = sigmoid(weight) (may be NULL); planar [M,P,P] */
int omni_heads_f32(const float* x, const float* w, float bias_pred, float bias_weight, float* out_a, float* out_c,
                   int M, int P, int confidence, omni_stream_t stream);
/* mlp_points1 / mlp_points2 (1x1 conv 3->16->64, BN folded, ReLU) of xyz[N,3,HW] (* depth[Mo,HW] if non-NULL),
 * model/spherical_model_iterative.py:290-305,319,387-393.  out NHWC [Mo,HW,64]. */
int omni_mlp_points_f32(const float* xyz, const float* depth, const float* w1, const float* b1, const float* w2,
                        const float* b2, float* out, int Mo, int N, int HW, omni_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics on the device (first "next" row): test.py:151-176 compute_eval_metrics and
 * metrics.py:7-26, without a device->host copy per batch.
 * ---------------------------------------------------------------------------------------------- */
/* x[mask > 0].median() (torch semantics: the lower middle element; NaN for an empty selection and for one that holds
 * a NaN of either sign).  ws: >= 260 unsigned; out: one device float. */
int omni_masked_median_f32(const float* x, const float* mask, size_t n, unsigned* ws, float* out, omni_stream_t stream);
/* pred *= *scale_num / *scale_den in place (test.py:161-162; device scalars, both NULL = no scaling), then
 * out[9] = abs_rel, sq_rel, rms_sq_lin, rms_sq_log, d1, d2, d3 (masked means, metrics.py:7-26), N = the count of mask > 0 (mask.sum()
 * for a 0/1 mask), N_log = the count with pred, gt > 1e-7 as well.
 * ws: >= 2048*9 doubles. */
int omni_depth_metrics_f32(float* pred, const float* gt, const float* mask, const float* scale_num, const float* scale_den,
                           size_t n, double* ws, float* out, omni_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Semantic segmentation (csrc/omni_semantic.hip): the supervision and scoring of train_erp_sem.py:203-210, 261-278 and
 * iou.py:21-24 in one pass over the logits.  logits: float32 [B, C, HW] (contiguous NCHW), 2 <= C <= 64; target: int64 [B, HW].
 * Pixel rules: target == ignore_index is outside the loss; a negative label is outside the matrix; a label
 * that is neither ignored nor a class index is dropped from both and counted in n_bad.  Nothing synchronises the host.
 * ---------------------------------------------------------------------------------------------- */
/* bytes of the workspace that carries the valid count, n_bad and the per-pixel log-sum-exp from the step to the gradient:
 * int64 count at offset 0, int64 n_bad at offset 8 (both written by every call) */
size_t omni_semantic_workspace_bytes(size_t npix);
/* *loss = mean over the valid pixels of lse(logits) - logits[target] (F.cross_entropy; NaN when no pixel is valid);
 * pred [B, HW] int64 = argmax over C (first index of the maximum, a NaN counts as the maximum), NULL = not written;
 * confusion [K, K] int64 += count of (pred, target) pairs (rows = predictions), NULL = not counted.  K = 0 means C; C <= K <= 64. */
int omni_semantic_step_f32(const float* logits, const int64_t* target, int B, int C, size_t HW, int64_t ignore_index, int K,
                           void* workspace, float* loss, int64_t* pred, int64_t* confusion, omni_stream_t stream);
/* grad_logits = (softmax - onehot) * (*grad_out) / count on the valid pixels, 0 elsewhere; `workspace` as the step left it. */
int omni_semantic_grad_f32(const float* logits, const int64_t* target, int B, int C, size_t HW, int64_t ignore_index,
                           const void* workspace, const float* grad_out, float* grad_logits, omni_stream_t stream);
/* confusion [K, K] int64 += count of (pred, gt) pairs of two int64 label maps of n pixels, 1 <= K <= 64 (iou.py:21-24); gt < 0 is
 * skipped, a pair with gt >= K or pred outside [0, K) is dropped and counted in *n_bad (device int64, accumulated; NULL = not counted). */
int omni_confusion_matrix_i64(const int64_t* pred, const int64_t* gt, size_t n, int K, int64_t* confusion, int64_t* n_bad,
                              omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Host-facing ends of the hot path, csrc/omni_io.hip.
 *
 * omni_preprocess_rgb_u8: decoded BGR uint8 frames [B,Hs,Ws,3] (device memory; the Python side stages them through pinned
 * buffers on a copy stream) -> cv2.INTER_AREA down-scale to HxW (identity when equal) -> /255 -> float32 [B,3,H,W].
 * Replaces dataset_loader_stanford.py:54,85,92-97 (`readRGBPano`, `rgb.astype(np.float32)/255`, transpose(2,0,1)).
 * omni_preprocess_depth_u16: 16-bit depth frames [B,Hs,Ws] -> float32 -> INTER_AREA -> /65535*128 -> mask (min, max] ->
 * depth [B,1,H,W] (* mask) and mask uint8.  Replaces dataset_loader_stanford.py:76-80,99-109. */
int omni_preprocess_rgb_u8(const unsigned char* src_hwc, float* dst_chw, int B, int Hs, int Ws, int H, int W, omni_stream_t stream);
int omni_preprocess_depth_u16(const unsigned short* src, float* depth, unsigned char* mask, int B, int Hs, int Ws, int H, int W,
                              float min_depth, float max_depth, omni_stream_t stream);
/* Training-time augmentation of the reference's loaders folded into the same pass (csrc/omni_augment.hip): random horizontal flip and
 * yaw roll (dataset_loader_stanford.py:57-67), gamma (dataset_loader_360d.py:67-71), colour permutation (dataset_loader_stanford.py:70-73).
 * Per item b the kernels read, from DEVICE memory, aug[b][5] = {flip, dx, perm0, perm1, perm2} (int32) and gamma[b] (float32; gamma may be
 * NULL = no gamma).  flip then roll is one column map, out[y][x] = in[y][s(x)] with r = (x - dx) mod W, s(x) = r without flip and
 * W-1-r with flip; colour is out[c] = in[perm[c]] ** gamma in the loader's channel order.  dx is reduced modulo W (negative values
 * included) and perm modulo 3 inside the kernels; nothing is read back on the host, the calls are capturable and a replayed graph reads
 * the table's current contents.  No atomics, no workspace: bitwise reproducible.
 * omni_augment_rgb_u8 / omni_augment_depth_u16: the arithmetic of omni_preprocess_rgb_u8 / omni_preprocess_depth_u16 (INTER_AREA and its
 * uint8 rounding happen BEFORE the map) sampled through s(x); gamma == 1 is bit-identical to no gamma.  Option "augment_lut" = 0 evaluates
 * powf per value instead of through the 256-entry table a block builds (same bits).
 * omni_augment_planes: the index map on planes [B,C,H,W] of elem_bytes (1, 2, 4, 8) bytes per element that already live on the device
 * (label maps, masks, float32 depth or images), copied as bytes.  color = 1 (C == 3) also applies perm and, with gamma != NULL (float32
 * elements only), powf.  inverse = 1 applies s^-1 instead — x' = x without flip, W-1-x with flip, t(x) = (x' + dx) mod W — and no colour:
 * it puts a prediction made on an augmented batch back onto the original panorama.  src == dst is OMNI_ERR_INVALID. */
int omni_augment_rgb_u8(const unsigned char* src_hwc, float* dst_chw, const int* aug, const float* gamma, int B, int Hs, int Ws, int H, int W,
                        omni_stream_t stream);
int omni_augment_depth_u16(const unsigned short* src, float* depth, unsigned char* mask, const int* aug, int B, int Hs, int Ws, int H, int W,
                           float min_depth, float max_depth, omni_stream_t stream);
int omni_augment_planes(const void* src, void* dst, int elem_bytes, const int* aug, const float* gamma, int B, int C, int H, int W,
                        int color, int inverse, omni_stream_t stream);
/* PNG decoding on the host (csrc/omni_png.hip; no GPU involved) — the two decode calls of dataset_loader_stanford.py:
 *   :85 cv2.imread(path)      -> kind 0: uint8 [H,W,3] in B,G,R order (alpha dropped, gray replicated, 16-bit samples >> 8)
 *   :96 cv2.imread(path, -1)  -> kind 1: the file's own samples, single-channel gray only: uint8 or uint16 (host byte order) [H,W]
 * `data` is the file's bytes; omni_png_info reads the header only.  Colour types 0/2/3/4/6 at 8 bits, 0/2/4/6 at 16 bits, not interlaced;
 * anything else returns OMNI_ERR_UNSUPPORTED, a damaged stream (signature, chunk CRC, zlib, size) OMNI_ERR_INVALID.
 * omni_png_decode_batch decodes n files of one size on the library's persistent decoder pool (one thread per core, at most 64, started on first use;
 * `threads`: at most that many of THIS call's images at a time, 0: no limit, 1: in the calling thread) — the loader's worker pool (test.py:90-97 uses 8
 * DataLoader workers); several calls may run side by side; dsts[i] may point into pinned memory so that the H2D copy needs no staging. */
int omni_png_info(const void* data, size_t nbytes, int* width, int* height, int* bit_depth, int* color_type);
int omni_png_decode(const void* data, size_t nbytes, void* dst, int H, int W, int kind);
int omni_png_decode_batch(const void* const* datas, const size_t* nbytes, void* const* dsts, int n, int H, int W, int kind, int threads);
/* The decoder's own inflate and checksums (csrc/omni_inflate.h), exposed so that they can be checked against an independent zlib (tests/test_png.py
 * decodes the same valid, truncated and damaged streams with Python's zlib module): what cv2.imread gets from libpng -> libz.
 * omni_zlib_inflate: one zlib stream (RFC 1950) -> at most cap bytes at dst; *produced = bytes written (also on failure: how far it got), *consumed =
 * bytes of the stream including its Adler-32.  OMNI_OK | OMNI_ERR_INVALID (damaged stream, or more than cap bytes) | OMNI_ERR_UNSUPPORTED (the input ends
 * inside the stream).  omni_png_checksums: CRC-32 (chunk check) and Adler-32 (zlib trailer) of a buffer, continuing from *crc32 / *adler32 (start: 0 / 1). */
int omni_zlib_inflate(const void* src, size_t nbytes, void* dst, size_t cap, size_t* produced, size_t* consumed);
int omni_png_checksums(const void* data, size_t nbytes, unsigned* crc32, unsigned* adler32);
/* Reverse-Huber loss of supervision/direct.py:3-18 (train_erp_depth.py:267): *loss = mean_b(sum(loss * mask * weights)_b / sum(mask)_b)
 * with c = max|gt - pred| / 5 evaluated on the device.  `workspace` (omni_berhu_workspace_bytes(B) bytes) carries c and the
 * per-item counts to omni_berhu_grad_f32, which writes dloss/dpred * (*grad_out). */
size_t omni_berhu_workspace_bytes(int B);
int omni_berhu_loss_f32(const float* pred, const float* gt, const float* mask, const float* weights, int B, size_t per_item,
                        void* workspace, float* loss, omni_stream_t stream);
int omni_berhu_grad_f32(const float* pred, const float* gt, const float* mask, const float* weights, int B, size_t per_item,
                        const void* workspace, const float* grad_out, float* grad_pred, omni_stream_t stream);
/* Point cloud of test.py:210-240: depth [B,1,H,W], rgb [B,3,H,W] -> B*H*W packed 15-byte PLY vertex records
 * (x, y, z float32 = uv2xyz(coords2uv(pixel)) * depth, util.py:159-174; three uint8 colours = uint8(rgb * 255)). */
int omni_pointcloud_ply_f32(const float* depth, const float* rgb, unsigned char* records, int B, int H, int W, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Depth-image-based rendering (csrc/omni_dibr.hip): a panorama as seen from a camera moved by a stereo baseline, by a forward
 * bilinear splat.  Layouts: img/recon [B,C,H,W], depth [B,1,H,W], coords [B,2,H,W] (u = column, v = row), mask [B,1,H,W] uint8
 * (NULL: not written).  The sums are 64-bit fixed-point integers: the result is bit-identical from run to run, under graph replay and
 * for a batch against its items one at a time.  `workspace` (omni_dibr_workspace_bytes(B, C, H, W) bytes, any content) is zeroed
 * inside the call; nothing is allocated and the host is never synchronised.  Non-finite img / depth values make the targets they
 * reach NaN. */
size_t omni_dibr_workspace_bytes(int B, int C, int H, int W);
/* supervision/splatting.py:73-80 */
int omni_splat_render_f32(const float* img, const float* depth, const float* coords, float max_depth,
                          float* recon, unsigned char* mask /* nullable */, int B, int C, int H, int W,
                          void* workspace, omni_stream_t stream);
/* util.py:384-413; mode 0 = vertical, 1 = horizontal; grid_batched: grids are [B,2,H,W] instead of [1,2,H,W] */
int omni_dibr_f32(const float* img, const float* depth, const float* uvgrid, const float* sgrid, int grid_batched,
                  float baseline, int mode, float* recon, unsigned char* mask /* nullable */,
                  int B, int C, int H, int W, void* workspace, omni_stream_t stream);
/* The same two forwards (same launches, same recon / mask bits), also writing the splatted weight sum wt [B,1,H,W] float32 — what the
 * backward needs (NaN where a non-finite weight reached the target). */
int omni_splat_render_wt_f32(const float* img, const float* depth, const float* coords, float max_depth,
                             float* recon, unsigned char* mask /* nullable */, float* wt, int B, int C, int H, int W,
                             void* workspace, omni_stream_t stream);
int omni_dibr_wt_f32(const float* img, const float* depth, const float* uvgrid, const float* sgrid, int grid_batched,
                     float baseline, int mode, float* recon, unsigned char* mask /* nullable */, float* wt,
                     int B, int C, int H, int W, void* workspace, omni_stream_t stream);
/* Backward of the splat: grad_recon = dL/drecon [B,C,H,W]; recon, wt: the forward's outputs.  A gather: every source
 * pixel re-derives its corners exactly as the forward does and reads its <= 4 targets; no atomics, nothing to zero, deterministic.
 * Each of grad_img [B,C,H,W], grad_depth [B,1,H,W], grad_coords [B,2,H,W] is written only if non-NULL (at least one must be).
 * The corner selection, floor and the clean-ups are constants of the backward, as in the reference's autograd; the DIBR modes chain
 * dL/du, dL/dv into the depth through the displacement.  Where depth == 0 or the displacement is not finite the depth gradient of
 * the DIBR modes is 0 (the reference: NaN).  `workspace`: omni_dibr_bwd_workspace_bytes(B, C, H, W) bytes, any content. */
size_t omni_dibr_bwd_workspace_bytes(int B, int C, int H, int W);
int omni_splat_render_bwd_f32(const float* grad_recon, const float* recon, const float* wt, const float* img, const float* depth,
                              const float* coords, float max_depth, float* grad_img, float* grad_depth, float* grad_coords,
                              int B, int C, int H, int W, void* workspace, omni_stream_t stream);
int omni_dibr_bwd_f32(const float* grad_recon, const float* recon, const float* wt, const float* img, const float* depth,
                      const float* uvgrid, const float* sgrid, int grid_batched, float baseline, int mode,
                      float* grad_img, float* grad_depth, int B, int C, int H, int W, void* workspace, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Photometric loss of view synthesis (csrc/omni_photometric.hip).  pred / gt [B,C,H,W] float32; `win`: HOST pointer to the `window`
 * 1-D window weights (odd window, 3 .. 11); mode 0 = 'gaussian' (zero-padded), 1 = 'box' (valid average, the map zero-padded).
 * omni_ssim_f32: the SSIM map of supervision/ssim.py `ssim_loss`.
 * omni_photometric_loss_f32: supervision/photometric.py:34-51; mask [B,mask_c,H,W], weights [B,weights_c,H,W] float32 with 1 or C
 * channels; *loss stays on the device.  `workspace` (omni_photometric_workspace_bytes bytes) carries the per-item counts to
 * omni_photometric_grad_f32, which writes dloss/dpred * (*grad_out); `scratch`: omni_photometric_grad_scratch_bytes bytes. */
int omni_ssim_f32(const float* pred, const float* gt, int B, int C, int H, int W, int window, const float* win, int mode,
                  float* ssim, omni_stream_t stream);
size_t omni_photometric_workspace_bytes(int B, int C, int H, int W);
size_t omni_photometric_grad_scratch_bytes(int B, int C, int H, int W);
int omni_photometric_loss_f32(const float* pred, const float* gt, const float* mask, int mask_c, const float* weights, int weights_c,
                              int B, int C, int H, int W, int window, const float* win, int mode, float alpha,
                              void* workspace, float* loss, omni_stream_t stream);
int omni_photometric_grad_f32(const float* pred, const float* gt, const float* mask, int mask_c, const float* weights, int weights_c,
                              int B, int C, int H, int W, int window, const float* win, int mode, float alpha,
                              const void* workspace, void* scratch, const float* grad_out, float* grad_pred, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Free-view sampling (csrc/omni_freeview.hip): N perspective views of h x w pixels at per-view yaw theta / pitch phi
 * (degrees) and one pair of fields of view (hfov: vertical extent, wfov: horizontal extent, each in (0, 180) degrees), and back.
 * Replaces equi_pers/equi2pers_torch.py:37 `equi2pers` and equi_pers/pers2equi_torch.py:37 `pers2equi` (grid build + F.grid_sample
 * bilinear / zeros / align_corners=True) with the reference's arithmetic order and quirks.  float32 only.
 *
 * omni_freeview_rotations: the rotations of `rotation_matrix` (equi2pers_torch.py:12-34), evaluated in double and rounded once, written
 * to HOST memory: rot_fwd[N*9] = R2.R1 per view, rot_inv[N*18] = R2^-1 then R1^-1 per view (either may be NULL).  The caller copies them to
 * the device once per set of angles; the three launches below read them there, allocate nothing, copy nothing and never synchronise
 * (capturable on one stream).
 * omni_freeview_equi2pers_f32: erp [B,C,H,W] -> pers [B,N,C,h,w] (OMNI_LAYOUT_BNCHW) or the reference's [B,C,h,N*w] (OMNI_LAYOUT_BCHNW,
 * equi2pers_torch.py:86-93).
 * omni_freeview_pers2equi_f32: pers [N,C,h,w] (one image per view) -> erp [N,C,H,W], zero outside the view, and mask [N,1,H,W] uint8.
 * omni_freeview_merge_f32 (no reference counterpart): pers [B,N,C,h,w] -> erp [B,C,H,W] = sum_v sample_v mask_v / max(sum_v mask_v, 1),
 * views summed in index order, and count [H,W] uint8 = sum_v mask_v (a function of the geometry only; N <= 255).  Every per-view sample
 * is the one omni_freeview_pers2equi_f32 computes; the N intermediate ERP images are never written.
 * pers / erp outputs must be 16-byte aligned, mask / count 4-byte aligned. */
int omni_freeview_rotations(const float* theta_deg, const float* phi_deg, int N, float* rot_fwd_host /*N*9*/, float* rot_inv_host /*N*18*/);
int omni_freeview_equi2pers_f32(const float* erp, float* pers, const float* rot_fwd_dev, int B, int C, int H, int W,
                                int N, int h, int w, float hfov_deg, float wfov_deg, int layout, omni_stream_t stream);
int omni_freeview_pers2equi_f32(const float* pers, float* erp, unsigned char* mask, const float* rot_inv_dev,
                                int N, int C, int h, int w, int H, int W, float hfov_deg, float wfov_deg, omni_stream_t stream);
int omni_freeview_merge_f32(const float* pers, float* erp, unsigned char* count, const float* rot_inv_dev,
                            int B, int N, int C, int h, int w, int H, int W, float hfov_deg, float wfov_deg, omni_stream_t stream);

/* The backwards of the three launches above (csrc/omni_freeview_bwd.hip, DESIGN.md §12 "Backward"): each sends w_k * g through the
 * forward's own tap set, summed as in §11 — every contribution rounded once to a 64-bit fixed-point integer (scale from the largest
 * finite |g| of the item: a batch item, or a view for pers2equi) and added with an integer atomic, so the bits do not depend on the
 * order of arrival, the batch split or the stream.  Four launches on the caller's stream, no allocation, no host synchronisation.
 * omni_freeview_equi2pers_bwd_f32: grad_pers (the layout of the forward's output) -> grad_erp [B,C,H,W], summed over the N views.
 * omni_freeview_pers2equi_bwd_f32: grad_erp [N,C,H,W] -> grad_pers [N,C,h,w]; an ERP pixel outside the view's mask contributes nothing.
 * omni_freeview_merge_bwd_f32: grad_erp [B,C,H,W] -> grad_pers [B,N,C,h,w], once per covering view, divided by max(count, 1).
 * A non-finite g makes NaN exactly the gradient elements it reaches through a corner that lies on the image.
 * `ws`: omni_freeview_bwd_workspace_bytes(op, items, C, Ht, Wt) bytes, 16-byte aligned, any content; op 0 / 1 / 2 = the three
 * functions in this order, items = the number of gradient images written (B | N | B * N), Ht x Wt their size; 0 for invalid arguments. */
size_t omni_freeview_bwd_workspace_bytes(int op, int items, int C, int Ht, int Wt);
int omni_freeview_equi2pers_bwd_f32(const float* grad_pers, float* grad_erp, const float* rot_fwd_dev, int B, int C, int H, int W,
                                    int N, int h, int w, float hfov_deg, float wfov_deg, int layout, void* ws, omni_stream_t stream);
int omni_freeview_pers2equi_bwd_f32(const float* grad_erp, float* grad_pers, const float* rot_inv_dev, int N, int C, int h, int w,
                                    int H, int W, float hfov_deg, float wfov_deg, void* ws, omni_stream_t stream);
int omni_freeview_merge_bwd_f32(const float* grad_erp, float* grad_pers, const float* rot_inv_dev, int B, int N, int C, int h, int w,
                                int H, int W, float hfov_deg, float wfov_deg, void* ws, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The geometry terms of depth training (csrc/omni_normals.hip; train_erp_depth.py:267-275).  float32, H, W >= 2
 * (smaller: OMNI_ERR_UNSUPPORTED).  `ray_tables`: a device array of 2 H + 2 W floats, [sin lat: H][cos lat: H][sin lon: W][cos lon: W]
 * of coords2uv / uv2xyz (util.py:159-174), built by the caller once per image size.  Nothing is allocated, nothing synchronises.
 * omni_depth_normals_f32: util.py:332-382 depth2normal_gpu, depth [B,1,H,W] -> normals [B,3,H,W]; the cross products always run over the
 * channel axis (the reference: over the batch axis when B == 3).
 * omni_sobel_f32: util.py:426-446 imgrad, img [B,C,H,W] -> the Sobel maps of its channel mean, grad_y and grad_x [B,1,H,W].
 * omni_l1_loss_f32 / omni_l1_grad_f32: supervision/direct.py:20-26 calculate_l1_loss over pred / gt [B,C,hw] and mask [B,mask_c,hw],
 * mask_c = 1 or C; count = the sum of the mask as stored.  `workspace` (omni_l1_workspace_bytes(B) bytes) carries the counts to the gradient,
 * which writes dloss/dpred * (*grad_out).
 * omni_geometry_terms_f32: losses[0] = normal_loss = 1 - mean_b(sum_b(normals(pred) normals(gt) mask) / sum(mask)) (terms & 1),
 * losses[1] = grad_loss = calculate_l1_loss(imgrad_yx(pred), imgrad_yx(gt), mask) (terms & 2) from one pass over pred, gt, mask [B,1,H,W];
 * a term that is not asked for is not computed and its slot is 0.  erode_mask: the mask is mask * [all eight neighbours non-zero]
 * (outside the image counts as non-zero).  `workspace`: omni_geometry_terms_workspace_bytes(B, H, W) bytes (0 for invalid arguments), any
 * content, 16-byte aligned; it carries the mask sums to omni_geometry_terms_grad_f32, which writes
 * (*grad_normal) d normal_loss / d pred + (*grad_grad) d grad_loss / d pred; a NULL upstream pointer leaves that term out (not both).
 * An item (grad_loss) or batch (normal_loss) whose mask sum is 0: NaN, as omni_berhu_loss_f32. */
int omni_depth_normals_f32(const float* depth, const float* ray_tables, int B, int H, int W, float* normals, omni_stream_t stream);
int omni_sobel_f32(const float* img, int B, int C, int H, int W, float* grad_y, float* grad_x, omni_stream_t stream);
size_t omni_l1_workspace_bytes(int B);
int omni_l1_loss_f32(const float* pred, const float* gt, const float* mask, int B, int C, size_t hw, int mask_c, void* workspace,
                     float* loss, omni_stream_t stream);
int omni_l1_grad_f32(const float* pred, const float* gt, const float* mask, int B, int C, size_t hw, int mask_c, const void* workspace,
                     const float* grad_out, float* grad_pred, omni_stream_t stream);
size_t omni_geometry_terms_workspace_bytes(int B, int H, int W);
int omni_geometry_terms_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W, int terms,
                            int erode_mask, void* workspace, float* losses, omni_stream_t stream);
int omni_geometry_terms_grad_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W,
                                 int erode_mask, const void* workspace, const float* grad_normal, const float* grad_grad, float* grad_pred,
                                 omni_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * The plane-fit normals of a depth map (csrc/omni_planefit.hip; equi_pers/depth2normal.py).  float32 in and out, any
 * H, W >= 1; `ray_tables` as above.  Over the 25 vertices p = ray * depth at offsets {-4,-2,0,2,4}^2 of a pixel (zero vectors outside the
 * image, no wrap across the seam): M = sum p p^T, s = sum p, n = M^-1 s where det M >= 1e-5 and n = s otherwise, normal = n / max(|n|,
 * 1e-12).  Moments, determinant and solve are float64 (the reference's float32 solve is off by 1e-2 at 512 x 1024); a NaN depth gives NaN
 * normals at exactly the centres whose windows hold it.  Nothing is allocated, nothing synchronises.
 * omni_planefit_normals_f32: depth [B,1,H,W] -> normals [B,3,H,W].
 * omni_planefit_normals_grad_f32: grad_depth [B,1,H,W] = d <grad_normals, normals> / d depth for an upstream [B,3,H,W].
 * omni_planefit_loss_f32: *loss = 1 - mean_b(sum_b(N(pred) . N(gt) mask) / sum(mask)) (train_erp_depth.py:271 with these normals; the
 * mask sum is the whole batch's, the mask is multiplied in by value; erode_mask as in omni_geometry_terms_f32) from pred, gt, mask
 * [B,1,H,W]; neither normal map is written.  A batch whose mask sum is 0: NaN.
 * omni_planefit_loss_grad_f32: grad_pred = (*grad_out) d loss / d pred; `workspace` is the one omni_planefit_loss_f32 filled for the same
 * arguments (it carries the mask sum).
 * `workspace`: omni_planefit_workspace_bytes(B, H, W) bytes (0 for invalid arguments), any content on entry, 16-byte aligned: the sums
 * of the loss and the [B,6,H,W] float64 map the two backward kernels hand over (the normals' backward uses that part alone). */
size_t omni_planefit_workspace_bytes(int B, int H, int W);
int omni_planefit_normals_f32(const float* depth, const float* ray_tables, int B, int H, int W, float* normals, omni_stream_t stream);
int omni_planefit_normals_grad_f32(const float* depth, const float* ray_tables, const float* grad_normals, int B, int H, int W, void* workspace,
                                   float* grad_depth, omni_stream_t stream);
int omni_planefit_loss_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W, int erode_mask,
                           void* workspace, float* loss, omni_stream_t stream);
int omni_planefit_loss_grad_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W,
                                int erode_mask, void* workspace, const float* grad_out, float* grad_pred, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The guided (edge-aware) smoothness term of the self-supervised objective (csrc/omni_smoothness.hip, DESIGN.md §15;
 * supervision/smoothness.py:3-8, spherical/derivatives.py:7-24,190-214, spherical/cartesian.py:14-50).  float32, B, C, H, W >= 1.
 * Nothing is allocated, nothing synchronises, nothing is read back.  Differences are t[i,j] - t[i,j+1] (du) and t[i,j] - t[i+1,j] (dv)
 * with replicate padding: the last column's du and the last row's dv are 0.  A mask element is valid where it is != 0.
 * omni_image_diff_f32: dI_du (axis 0) / dI_dv (axis 1), img [B,C,H,W] -> out [B,C,H,W].
 * omni_image_diff_norm_f32: dI_duv, the 2-norm over the 2 C difference channels, img [B,C,H,W] -> out [B,1,H,W].
 * omni_vertex_diff_norm_f32: dV_dxyz, pcloud [B,3,H,W] -> out [B,1,H,W] = sqrt(du^2 + dv^2), du = |du_x| + |du_y| + |du_z|, dv likewise.
 * omni_guided_smoothness_f32: *loss = sum(mask ? input_duv exp(-guide_duv) weights : 0) / sum(mask != 0) over n elements each (the mask
 * selects: nothing at a masked element, the weight included, reaches the sum); omni_guided_smoothness_grad_f32 writes
 * (*grad_out) dloss / dinput_duv.  `workspace`: omni_guided_smoothness_workspace_bytes(n) bytes.
 * omni_depth_smoothness_f32: the same loss for input_duv = dV_dxyz of the vertices x = depth cos(phi) (-1) cos(theta), y = depth sin(theta),
 * z = depth sin(phi) cos(theta) and guide_duv = dI_duv(image), from one pass over depth [B,1,H,W], image [B,C,H,W], mask and weights
 * [B,1,H,W] (weights may be NULL: 1); no intermediate map is written.  `factors`: a device array [4][H][W] = cos phi | sin phi |
 * cos theta | sin theta of the spherical grid, built by the caller once per grid.  omni_depth_smoothness_grad_f32 writes
 * (*grad_out) dloss / ddepth by a gather (no atomics); d|x|/dx = 0 at 0 and the gradient of a 2-norm is 0 where the norm is 0.
 * `workspace`: omni_depth_smoothness_workspace_bytes(B, H, W) bytes.  Workspaces: 0 for invalid arguments, any content, 16-byte aligned;
 * the forward leaves the mask sum there for the gradient.  sum(mask != 0) == 0: NaN (0 / 0), as the reference. */
int omni_image_diff_f32(const float* img, int B, int C, int H, int W, int axis, float* out, omni_stream_t stream);
int omni_image_diff_norm_f32(const float* img, int B, int C, int H, int W, float* out, omni_stream_t stream);
int omni_vertex_diff_norm_f32(const float* pcloud, int B, int H, int W, float* out, omni_stream_t stream);
size_t omni_guided_smoothness_workspace_bytes(size_t n);
int omni_guided_smoothness_f32(const float* input_duv, const float* guide_duv, const float* mask, const float* weights, size_t n,
                               void* workspace, float* loss, omni_stream_t stream);
int omni_guided_smoothness_grad_f32(const float* guide_duv, const float* mask, const float* weights, size_t n, const void* workspace,
                                    const float* grad_out, float* grad_input, omni_stream_t stream);
size_t omni_depth_smoothness_workspace_bytes(int B, int H, int W);
int omni_depth_smoothness_f32(const float* depth, const float* image, const float* mask, const float* weights, const float* factors, int B,
                              int C, int H, int W, void* workspace, float* loss, omni_stream_t stream);
int omni_depth_smoothness_grad_f32(const float* depth, const float* image, const float* mask, const float* weights, const float* factors,
                                   int B, int C, int H, int W, const void* workspace, const float* grad_out, float* grad_depth,
                                   omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The one-directional Chamfer term between two point clouds and its gradient (csrc/omni_chamfer.hip; util.py:201-257,
 * chamfer_distance_with_batch).  float32, contiguous p1 [B,N,D] and p2 [B,M,D], D = 2 or 3, B, N, M >= 1 (B <= 65535; N x M has no limit).
 * mask1 [B,N] / mask2 [B,M]: uint8, valid where != 0, either may be NULL (every point valid).  Nothing is allocated, nothing synchronises,
 * nothing is read back; no floating-point atomics: every output has the same bits on every run.
 * omni_chamfer_nn_f32: dist [B,N] = min over the valid j of |p1[i] - p2[j]| (squared distances from direct differences, sqrt of the winner),
 * 0 at a masked query; idx [B,N] int32 = the argmin, the LOWEST index among equal distances, -1 at a masked query and in an item without a
 * valid target (whose dist is +inf); *loss = sum(dist), added in double in a fixed order and rounded once.  A NaN coordinate of a valid
 * target makes every dist of its item NaN, one of a valid query its own dist (idx -1), and the loss NaN.
 * omni_chamfer_grad_f32: with g_i = *grad_loss (NULL: 0) + grad_dist[b,i] (NULL: 0), at least one of them given:
 * grad_p1 [B,N,D] = g_i (p1[i] - p2[idx_i]) / dist_i, 0 where dist_i == 0, at masked queries and where idx_i < 0; grad_p2 [B,M,D] = the
 * negated sum of the same vectors over the queries whose idx is j, in 64-bit fixed point (exact, order-independent).  Either gradient
 * pointer may be NULL (not computed), not both.  idx is the forward's output.
 * `workspace`: omni_chamfer_workspace_bytes(B, N, M, D) bytes (0 for invalid arguments), any content, 16-byte aligned; the two calls do
 * not share state through it.  Option "chamfer_split" = 0 keeps the search from cutting the targets into chunks (same bits). */
size_t omni_chamfer_workspace_bytes(int B, int N, int M, int D);
int omni_chamfer_nn_f32(const float* p1, const float* p2, const unsigned char* mask1, const unsigned char* mask2, int B, int N, int M, int D,
                        float* dist, int* idx, float* loss, void* workspace, omni_stream_t stream);
int omni_chamfer_grad_f32(const float* p1, const float* p2, const unsigned char* mask1, const int* idx, const float* grad_loss,
                          const float* grad_dist, int B, int N, int M, int D, float* grad_p1, float* grad_p2, void* workspace,
                          omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The backward of omni_conv2d_nhwc_f16x3_ws (csrc/omni_conv_bwd.hip): out = act(Z), Z = conv(src1 ++ src2, wt) + bias + res.
 * fp32 NHWC tensors, wt fp32 [Cout][(ky,kx,c)], C1, C2, Cout multiples of 32, KH = KW = 1 or 3, stride 1 or 2, any pad >= 0, act NONE or
 * RELU (GELU: OMNI_ERR_UNSUPPORTED — the forward does not keep the pre-activation).  rows = M * Ho * Wo.  Products are f16x3 as in the
 * forward.  Nothing is allocated, nothing synchronises, nothing is read back; no floating-point atomics: the same bits on every run.
 * omni_conv2d_bwd_epilogue_f32: dz[r][j] = grad_out[r][j] . [out[r][j] > 0] (act NONE: dz = grad_out; dz may then be NULL and the caller
 * passes grad_out on as dZ); grad_bias[j] = sum_r dZ[r][j] (two fixed-order stages); the residual's gradient is dZ itself.  scale: two
 * floats in device memory, 2^s and 2^-s, s = 8 - floor(log2 max|dZ|) clamped to [-126, 126]; s = 0 where dZ is all zero or its largest
 * magnitude is not finite.  The two calls below multiply dZ by 2^s before they split it into halfs and their result by 2^-s (both exact), so
 * gradients of any magnitude keep the precision of the format and grad_out . 2^n gives every gradient . 2^n bit for bit.
 * omni_conv2d_bwd_data_f16x3: dx[m,y,x,ci] = sum_{ky,kx,co} dz[m,(y+p-ky)/s,(x+p-kx)/s,co] . wt[co][(ky,kx,ci)] over the taps where both
 * divisions are exact and the source lies inside the Ho x Wo map; channels [0, C1) go to dx1 [M,H,W,C1], [C1, C1+C2) to dx2 [M,H,W,C2]; either
 * may be NULL (not computed), not both; every element of a given tensor is written.  A tap that does not apply is not read.
 * omni_conv2d_bwd_weight_f16x3: dw[co][(ky,kx,ci)] = sum_r dz[r][co] . A[r][(ky,kx,ci)], A the forward's implicit im2col of src1 ++ src2.
 * The rows are cut into chunks of option "conv_wgrad_rows" rows (a multiple of 32, least 32; 0 = the library's plan), summed in chunk
 * order: the result is a function of the inputs and the chunk length.
 * `workspace`: omni_conv2d_bwd_workspace_bytes(...) bytes serve any of the three calls (0 for shapes outside the scope above; it depends on
 * "conv_wgrad_rows"), any content, 16-byte aligned; the calls share no state through it — scale is the only hand-over.
 * omni_conv2d_split_weights_f16x3: wt fp32 [Cout][K] -> wt16, the halfs [Cout][K/32][hi32|lo32] the forward reads, on the device.
 * The _f16x1 entry points are the single-product forms of their _f16x3 siblings: the same arguments, workspace, rejections,
 * chunks, epilogue and scale; operands hi(dZ . 2^s), hi(wt), hi(A), one matrix instruction per product block.  An element of dZ below
 * 2^-22 max|dZ| contributes 0.  omni_conv2d_split_weights_f16x1 writes the hi-only image, halfs [Cout][K] (half the bytes). */
size_t omni_conv2d_bwd_workspace_bytes(int M, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad);
int omni_conv2d_bwd_epilogue_f32(const float* grad_out, const float* out, float* dz, float* grad_bias, float* scale, long long rows,
                                 int Cout, int act, void* workspace, size_t ws_bytes, omni_stream_t stream);
int omni_conv2d_bwd_data_f16x3(const float* dz, const float* wt, const float* scale, float* dx1, float* dx2, int M, int H, int W, int C1,
                               int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes,
                               omni_stream_t stream);
int omni_conv2d_bwd_weight_f16x3(const float* dz, const float* src1, const float* src2, const float* scale, float* dw, int M, int H, int W,
                                 int C1, int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes,
                                 omni_stream_t stream);
int omni_conv2d_split_weights_f16x3(const float* wt, void* wt16, int Cout, int K, omni_stream_t stream);
int omni_conv2d_bwd_data_f16x1(const float* dz, const float* wt, const float* scale, float* dx1, float* dx2, int M, int H, int W, int C1,
                               int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes,
                               omni_stream_t stream);
int omni_conv2d_bwd_weight_f16x1(const float* dz, const float* src1, const float* src2, const float* scale, float* dw, int M, int H, int W,
                                 int C1, int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes,
                                 omni_stream_t stream);
int omni_conv2d_split_weights_f16x1(const float* wt, void* wt16, int Cout, int K, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Batch normalisation with a fused residual and ReLU, and its backward (csrc/omni_batchnorm.hip):
 *     y = act(fmaf(x - mean, invstd . gamma, beta) + res),   fp32, contiguous NHWC: rows = M.H.W rows of C channels, C a multiple of 4,
 * act NONE or RELU (GELU: OMNI_ERR_UNSUPPORTED).  gamma / beta [C] may be NULL (no affine), res may be NULL.  Nothing is allocated, nothing
 * synchronises, nothing is read back; no atomics, every sum in a fixed order (partials and finish in double): the same bits on every run.
 * omni_batchnorm_fwd_f32, training != 0: mean and the biased variance of each channel over the rows (rows >= 2), saved[0][c] = mean,
 * saved[1][c] = invstd = 1 / sqrt(var + eps); with running buffers (both or neither) running_mean = (1 - momentum) running_mean + momentum mean
 * and running_var likewise with var . rows / (rows - 1), in place.  training == 0: mean = running_mean, invstd from running_var (both
 * required, unchanged); saved is written all the same, so the backward reads one pair.  eps > 0 and finite, momentum in [0, 1].
 * omni_batchnorm_bwd_f32: dZ = g . [y > 0] (a select; act NONE: dZ = g, y is not read).  dbeta[c] = sum_r dZ, dgamma[c] = sum_r dZ . xhat,
 * xhat = (x - mean) . invstd; dx = gamma . invstd . (dZ - dbeta / rows - xhat . dgamma / rows) in training mode, gamma . invstd . dZ in eval
 * mode; dres = dZ (act RELU only: with act NONE the residual's gradient is g itself and dres must be NULL).  Every output pointer may be
 * NULL (not computed), not all four; a pass nobody needs is not launched (no dx: no apply pass; eval mode without dgamma and dbeta: no
 * reduction pass).  x, y, gamma, saved are the forward's; `training` and `act` must be the forward's.
 * `workspace`: omni_batchnorm_workspace_bytes(rows, C) bytes (0 for arguments outside the scope), any content, 16-byte aligned; the eval-mode
 * forward does not touch it.  The two calls share no state through it. */
size_t omni_batchnorm_workspace_bytes(long long rows, int C);
int omni_batchnorm_fwd_f32(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean, float* running_var,
                           float* y, float* saved, long long rows, int C, int training, double momentum, double eps, int act,
                           void* workspace, size_t ws_bytes, omni_stream_t stream);
int omni_batchnorm_bwd_f32(const float* g, const float* x, const float* y, const float* gamma, const float* saved, float* dx, float* dres,
                           float* dgamma, float* dbeta, long long rows, int C, int training, int act, void* workspace, size_t ws_bytes,
                           omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The same operator in training mode with its statistics over the rows of ALL ranks of a group (csrc/omni_batchnorm.hip):
 * the two calls above, cut at their finishes into four.  The library moves no data between ranks: the caller gathers the records.  The
 * same rules: fp32 contiguous NHWC, C a multiple of 4, nothing allocated, nothing synchronised, nothing read back, no atomics, fixed
 * summation orders, every rejection before a launch.  `rows` is THIS rank's row count, >= 1 (only the group's total has to be >= 2; with
 * world == 1 a single row is rejected).  `workspace`: omni_batchnorm_workspace_bytes(rows, C) bytes.
 * A rank's exchange record `sums` is 2 C + 1 doubles, 8-byte aligned: [0][c] and [1][c] the two sums of channel c over the rank's rows (the
 * slab plan and summation order of the calls above, left in double), [2 C] = rows.  `all_sums` is [world][2 C + 1]: the records of the
 * ranks in rank order, 1 <= world <= 64 (else INVALID).  Totals over ranks are added in ascending rank order in double, so every rank
 * computes the same bits from the same table.
 * omni_syncbn_stats_f32: the record of (sum x, sum x^2).
 * omni_syncbn_fwd_apply_f32: n = sum_r rows_r, mean = sum x / n, var = max(sum x^2 / n - mean^2, 0) (a NaN stays a NaN), saved = (float)(mean,
 * 1 / sqrt(var + eps)), the running buffers (both or neither) move with var . n / (n - 1) as in omni_batchnorm_fwd_f32; then the apply pass.
 * omni_syncbn_bwd_reduce_f32: the record of (sum dZ, sum dZ . xhat), dZ = g . [y > 0] with act RELU (y required), g with act NONE.  dgamma /
 * dbeta (each may be NULL) get THIS rank's sums rounded to fp32: parameter gradients stay local, the gradient exchange adds them.  dz
 * non-NULL: dZ is written (act RELU only; with act NONE dZ is g itself and dz must be NULL).
 * omni_syncbn_bwd_apply_f32: per channel the total of each sum over the ranks, rounded once to fp32; k = (float)((double)total / n);
 * dx = gamma . invstd . ((dZ - k1) - xhat . k2).  y non-NULL with act RELU: the first argument is g and dZ is selected again; y NULL (or act
 * NONE): the first argument is dZ.  dres non-NULL (act RELU and y required): dZ is written there.  dx or dres may be NULL, not both; without
 * dx, x, saved and all_sums are not read.
 * With world == 1 and their own record the four calls write bit for bit the y, saved, running buffers, dx, dres, dgamma and dbeta of
 * omni_batchnorm_fwd_f32 / omni_batchnorm_bwd_f32 (training) on the same tensors. */
int omni_syncbn_stats_f32(const float* x, double* sums, long long rows, int C, void* workspace, size_t ws_bytes, omni_stream_t stream);
int omni_syncbn_fwd_apply_f32(const float* x, const float* res, const float* gamma, const float* beta, const double* all_sums, int world,
                              float* running_mean, float* running_var, float* y, float* saved, long long rows, int C, double momentum,
                              double eps, int act, omni_stream_t stream);
int omni_syncbn_bwd_reduce_f32(const float* g, const float* x, const float* y, const float* saved, float* dz, double* sums, float* dgamma,
                               float* dbeta, long long rows, int C, int act, void* workspace, size_t ws_bytes, omni_stream_t stream);
int omni_syncbn_bwd_apply_f32(const float* g_or_dz, const float* y, const float* x, const float* gamma, const float* saved,
                              const double* all_sums, int world, float* dx, float* dres, long long rows, int C, int act,
                              omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The transformer's training operators beyond its linear layers (csrc/omni_transformer_bwd.hip): layer normalisation over
 * the last axis with its backward, the backward of omni_attention_f32, the exact GELU with its backward.  fp32, contiguous.  Nothing is
 * allocated, nothing synchronises, nothing is read back; no atomics, every sum in a fixed order that depends on the shapes alone: the same
 * bits on every run.  Every rejection happens before a launch.  No backward reads anything a forward left behind except the operator's
 * own inputs.
 * omni_layernorm_fwd_f32: y[r] = (x[r] - mean_r) . rstd_r . gamma + beta over rows of C values, C a multiple of 4 in [4, 1024] (else
 * INVALID / past 1024 UNSUPPORTED), biased variance, rstd = 1 / sqrt(var + eps), eps > 0; gamma / beta [C] may be NULL.  One wave per row; at
 * C = 512 the bits of omni_layernorm512_f32.
 * omni_layernorm_bwd_f32: recomputes mean and rstd from x (the forward's code).  xhat = (x - mean) . rstd, a = grad_y . gamma,
 * dx = rstd . (a - mean_c(a) - xhat . mean_c(a . xhat)); dgamma[c] = sum_r grad_y . xhat, dbeta[c] = sum_r grad_y: per-slab partials in
 * double, rows ascending, then the slabs ascending, one rounding.  Each of dx, dgamma, dbeta may be NULL (not computed), not all three; no
 * dgamma and no dbeta: no reduction pass and no workspace.  gamma, eps: the forward's.
 * `workspace`: omni_layernorm_bwd_workspace_bytes(rows, C) = nslab . 2 . C . 8 + rows . 8 bytes, rounded up to 16 (0 outside the scope), with
 * slab = max(8, ceil(rows / 1024)) rows and nslab = ceil(rows / slab); any content, 16-byte aligned.
 * omni_attention_bwd_f32: the gradients of omni_attention_f32's out [B.N, 512] w.r.t. q [B.N, 512] and kv [B.N, 1024] (k | v), N <= 64
 * (else UNSUPPORTED).  P is recomputed from q and k with the forward's arithmetic.  dP_ij = dO_i . v_j, delta_i = sum_j P_ij dP_ij,
 * dS_ij = P_ij (dP_ij - delta_i), dq_i = scale . sum_j dS_ij k_j, dv_j = sum_i P_ij dO_i, dk_j = scale . sum_i dS_ij q_i, every sum over i
 * or j in ascending order.  dq or dkv may be NULL (not computed), not both; dkv is written whole.  `workspace` (needed for dkv only):
 * omni_attention_bwd_workspace_bytes(B, N) = 2 . B . 4 . N . N floats (0 outside the scope), any content, 16-byte aligned.
 * omni_gelu_fwd_f32: y = 0.5 x (1 + erf(x / sqrt 2)), the expression of the fused act = GELU epilogues; n a positive multiple of 4.
 * omni_gelu_bwd_f32: dx = grad_y . (0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi)); reads x, not y. */
size_t omni_layernorm_bwd_workspace_bytes(long long rows, int C);
int omni_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, long long rows, int C, float eps,
                           omni_stream_t stream);
int omni_layernorm_bwd_f32(const float* grad_y, const float* x, const float* gamma, float* dx, float* dgamma, float* dbeta, long long rows,
                           int C, float eps, void* workspace, size_t ws_bytes, omni_stream_t stream);
size_t omni_attention_bwd_workspace_bytes(int B, int N);
int omni_attention_bwd_f32(const float* q, const float* kv, const float* grad_out, float* dq, float* dkv, int B, int N, void* workspace,
                           size_t ws_bytes, omni_stream_t stream);
int omni_gelu_fwd_f32(const float* x, float* y, long long n, omni_stream_t stream);
int omni_gelu_bwd_f32(const float* grad_y, const float* x, float* dx, long long n, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The encoder's first operators and the decoder's up-sampling in training mode.  fp32; activations contiguous NHWC.
 * Nothing is allocated, nothing synchronises, nothing is read back; no atomics, every sum in a fixed order that depends on the shapes
 * alone: the same bits on every run.  Every rejection (null pointers, M, H, W <= 0, C % 4, a short workspace: OMNI_ERR_INVALID)
 * happens before a launch.
 * omni_stem_conv_fwd_f32 (csrc/omni_stem_conv.hip): conv1 of model/spherical_model.py:254 ALONE — 7x7, stride 2, padding 3, 3 -> 64
 * channels, y = conv(x, wt) + bias with no normalisation and no activation (omni_stem_f32 folds bn1 and the ReLU in).  x planar
 * [M,3,H,W] with ANY H, W >= 1, wt [147][64] with k = (ky*7+kx)*3+c (omni_stem_f32's layout), bias [64] or NULL, y [M,Ho,Wo,64],
 * Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1.
 * omni_stem_conv_bwd_weight_f32: the gradient of that convolution (:254) w.r.t. wt and bias: dw[k][o] = sum over (m, oy, ox) of
 * g[m,oy,ox,o] . x[m,c,2oy-3+ky,2ox-3+kx] (zero outside the image), dbias[o] = sum g[m,oy,ox,o], out of one pass.  g [M,Ho,Wo,64],
 * dw [147][64], dbias [64]; either may be NULL (not written), not both.  fp32 FMAs over chunks of 8x8-pixel output tiles, pixels
 * ascending within a chunk; the chunks' partial sums are added in double in a fixed order and rounded once.  There is no gradient
 * w.r.t. x (the image).
 * `workspace`: omni_stem_conv_bwd_workspace_bytes(M, H, W) = nchunk . 148 . 64 . 4 bytes (0 outside the scope), with
 * ntiles = M . ceil(Ho/8) . ceil(Wo/8), tpc = max(4, ceil(ntiles / 1024)) tiles per chunk and nchunk = ceil(ntiles / tpc); any content,
 * 16-byte aligned.
 * omni_maxpool3x3s2_bwd_f32 (csrc/omni_maxpool_bwd.hip): the backward of omni_maxpool3x3s2_f32 (:255) w.r.t. its input: x [M,H,W,C] the
 * forward's input, g [M,Ho,Wo,C], dx [M,H,W,C] written whole.  A gather: each input pixel recomputes the winner of the at most 2 x 2
 * windows that contain it — the FIRST greatest element in (ky, kx) order over the taps inside the map, torch's rule — and adds the g of
 * the windows it wins, windows in (oy, ox) order.  A NaN never wins against a number (the forward's fmaxf drops it too).
 * omni_upsample_bilinear2x_bwd_f32 (csrc/omni_upsample_bwd.hip): the backward of omni_upsample_bilinear_f32 at Ho = 2H, Wo = 2W
 * (:271,279,286,293,300) w.r.t. its input: g [M,2H,2W,C], dx [M,H,W,C] written whole.  A gather with the constant weights 0.25 / 0.75 / 1
 * per axis, the at most 4 x 4 taps added in (row, column) order. */
int omni_stem_conv_fwd_f32(const float* x, const float* wt, const float* bias, float* y, int M, int H, int W, omni_stream_t stream);
size_t omni_stem_conv_bwd_workspace_bytes(int M, int H, int W);
int omni_stem_conv_bwd_weight_f32(const float* g, const float* x, float* dw, float* dbias, int M, int H, int W, void* workspace,
                                  size_t ws_bytes, omni_stream_t stream);
int omni_maxpool3x3s2_bwd_f32(const float* g, const float* x, float* dx, int M, int H, int W, int C, omni_stream_t stream);
int omni_upsample_bilinear2x_bwd_f32(const float* g, float* dx, int M, int H, int W, int C, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The two depth heads in training mode (csrc/omni_heads_bwd.hip): pred and weight_pred of model/spherical_model.py:304-307,
 * 3x3 convolutions 32 -> 1 with bias, then ReLU, sigmoid and the product.  fp32 FMAs; x contiguous NHWC [M,H,W,32] with ANY H, W >= 1;
 * w [2][9][32] (pred, then weight_pred: omni_heads_f32's layout); bias [2] in DEVICE memory; every map planar [M,H,W], M.H.W < 2^31 (else
 * UNSUPPORTED).  Nothing is allocated, nothing synchronises, nothing is read back; no atomics, every sum in a fixed order that depends on
 * the shapes alone: the same bits on every run, and dx of an item is a function of that item.  Every rejection happens before a launch.
 * omni_depth_heads_fwd_f32: p = conv(x, w[0]) + bias[0], q = conv(x, w[1]) + bias[1] (taps in (ky, kx, c) order, one fp32 chain each);
 * out_a = relu(p) . (confidence ? sigmoid(q) : 1), out_c = sigmoid(q) (may be NULL); out_p / out_q receive the pre-activations (each may
 * be NULL: pass them when a gradient is pending — the backward reads them instead of reading x a second time).
 * omni_depth_heads_bwd_f32: s = sigmoid(q); gp = grad_a . s . [p > 0], gq = (grad_a . relu(p) + grad_c) . s (1 - s); with confidence = 0
 * gp = grad_a . [p > 0], gq = grad_c . s (1 - s).  grad_a or grad_c may be NULL (zero), not both; q may be NULL when confidence = 0 and
 * grad_c is NULL.  dx[m,y,x,c] = sum_tap gp[y-ky+1, x-kx+1] . w[0][tap][c] + gq[...] . w[1][tap][c], taps in (ky, kx) order, a tap
 * outside the map never read; dw[h][tap][c] = sum over the pixels of g_h[pixel] . x[pixel + tap - 1][c] and dbias[h] = sum g_h: fp32
 * FMAs over chunks of 16x16 tiles, the chunks' partials [578] added in double in a fixed order, one rounding.  Each of dx [M,H,W,32],
 * dw [2][9][32], dbias [2] may be NULL (not computed), not all three; x is read for dw / dbias only.
 * `workspace`: omni_depth_heads_bwd_workspace_bytes(M, H, W) = M.H.W . 8 (rounded up to 16) + nchunk . 578 . 4 bytes (0 outside the scope),
 * with ntiles = M . ceil(H/16) . ceil(W/16), tpc = max(4, ceil(ntiles / 1024)) and nchunk = ceil(ntiles / tpc); any content, 16-byte
 * aligned. */
int omni_depth_heads_fwd_f32(const float* x, const float* w, const float* bias, float* out_a, float* out_c, float* out_p, float* out_q,
                             int M, int H, int W, int confidence, omni_stream_t stream);
size_t omni_depth_heads_bwd_workspace_bytes(int M, int H, int W);
int omni_depth_heads_bwd_f32(const float* grad_a, const float* grad_c, const float* p, const float* q, const float* x, const float* w,
                             float* dx, float* dw, float* dbias, int M, int H, int W, int confidence, void* workspace, size_t ws_bytes,
                             omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * AdamW with the gradient norm and the clip of clip_grad_norm_ over one flat arena (csrc/omni_optim.hip).  Parameters,
 * exp_avg and exp_avg_sq are three fp32 arenas of one layout: a segment per tensor, each at a multiple of 64 floats, the padding zero and
 * never read or written.  A chunk is 4096 elements of one segment (the last chunk of a segment is short).  Two DEVICE tables describe the
 * work: `segments`, long long [nseg][4] = arena offset in floats, element count, address of the gradient (0: none; any 4-byte alignment,
 * contiguous in the parameter's storage order), parameter group; `chunks`, int [nchunk][2] = segment, offset of the chunk within it.  Both
 * 8-byte aligned; an entry that points outside [0, nseg) or past its segment's count is skipped, an arena shorter than the table says is
 * the caller's error.  Nothing is allocated, nothing synchronises, nothing is read back; no atomics, every sum in a fixed order: the same
 * bits on every run, whatever the gradients' alignment.  The three calls can be captured; what changes between steps is in device memory.
 * omni_adamw_grad_sqnorm_f32: partials[c] = the sum of g . g over chunk c in double, 0 for a segment without a gradient.
 * omni_adamw_prepare_f32 (one block): adds the partials in the order of omni_partials.h, rounds once to fp32 and takes the square root;
 * writes `record`, float [4 + 8 . ngroups]: [0] that norm, [1] clip = min(1, max_norm / (norm + 1e-6)) in fp32 (1 where max_norm < 0: no
 * clipping), [2] 1 where the norm is inf or NaN, [3] 1 where this step is skipped (skip_nonfinite and [2]); then per group, from
 * `groups` = double [ngroups][5] (lr, beta1, beta2, eps, weight_decay) in DEVICE memory: 1 - lr . wd, lr / (1 - beta1^t), sqrt(1 - beta2^t),
 * eps, beta2, 1 - beta1, 1 - beta2, 0, each computed in double and rounded once.  `counters`, long long [2]: a skipped step adds 1 to
 * counters[1]; any other adds 1 to the step count t = counters[0] first.  1 <= ngroups <= 256.
 * omni_adamw_apply_f32: per element of every segment that has a gradient, unless record[3] is set, in fp32:
 *     g' = g . clip;  p = p . (1 - lr . wd);  m = fma(g' - m, 1 - beta1, m);  v = fma((1 - beta2) . g', g', v . beta2);
 *     p = fma(-lr / bc1, m / (sqrt(v) / sqrt(bc2) + eps), p)
 * A skipped step or a segment without a gradient leaves p, m, v untouched; the gradient is never written.  Arenas 16-byte aligned. */
int omni_adamw_grad_sqnorm_f32(const void* segments, int nseg, const int* chunks, int nchunk, double* partials, omni_stream_t stream);
int omni_adamw_prepare_f32(const double* partials, int nchunk, const double* groups, int ngroups, double max_norm, int skip_nonfinite,
                           float* record, long long* counters, omni_stream_t stream);
int omni_adamw_apply_f32(float* params, float* exp_avg, float* exp_avg_sq, const void* segments, int nseg, const int* chunks, int nchunk,
                         const float* record, int ngroups, omni_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The 1x1 convolutions of the point-feature MLPs in training mode (csrc/omni_point_conv.hip): mlp_points1 / mlp_points2 of
 * model/spherical_model_iterative.py:290-305, 387-393 and mlp_points of model/spherical_model.py:228-235.  fp32 FMAs, no bias:
 *     y[m,hw,o] = sum_c w[o][c] . (x[m mod Mx, c, hw] . (scale ? scale[m,hw] : 1)),  c ascending, the product x . scale rounded first.
 * Exactly three forms (anything else UNSUPPORTED): Cin -> Cout = 3 -> 16 with x planar [Mx,3,HW], M a multiple of Mx (x is broadcast over
 * the M / Mx repeats) and an optional scale [M,HW]; 5 -> 16 with x planar [M,5,HW]; 16 -> 64 with x NHWC [M,HW,16]; the last two with
 * Mx = M and scale NULL.  w [Cout][Cin] (the parameter's storage); y and gy contiguous NHWC [M,HW,Cout]; M.HW < 2^31 (else UNSUPPORTED);
 * every pointer 16-byte aligned.  Nothing is allocated, nothing synchronises, no atomics, every sum in an order that depends on the
 * shapes alone: the same bits on every run, and dx / dscale of an item are functions of that item.  Every rejection happens before a launch.
 * omni_point_conv_bwd_f32: each of dx, dw, dscale may be NULL (not computed, its kernel not launched), not all three.
 *   dscale [M,HW] (3 -> 16 with a scale only) = sum_c x[m mod Mx,c,hw] . (sum_o w[o][c] . gy[m,hw,o]), o then c ascending;
 *   dx [M,HW,16] (16 -> 64 only; UNSUPPORTED for the planar forms) = sum_o w[o][c] . gy[m,hw,o], o ascending;
 *   dw [Cout][Cin] = sum over the rows of gy[row][o] . (x . scale)[row][c]: fp32 FMAs over chunks of `per` rows, the chunks' partials
 *   [Cout.Cin] added in double in a fixed order, one rounding.  x is read for dw and dscale only.
 * `workspace` (dw only): omni_point_conv_bwd_workspace_bytes(M, HW, Cin, Cout) = nchunk . Cout . Cin . 4 bytes (0 outside the scope), with
 * per = 64 . max(5, ceil(ceil(M.HW / 1024) / 64)) rows and nchunk = ceil(M.HW / per); any content, 16-byte aligned. */
int omni_point_conv_fwd_f32(const float* x, const float* w, const float* scale, float* y, int Mx, int M, int HW, int Cin, int Cout,
                            omni_stream_t stream);
size_t omni_point_conv_bwd_workspace_bytes(int M, int HW, int Cin, int Cout);
int omni_point_conv_bwd_f32(const float* gy, const float* x, const float* w, const float* scale, float* dx, float* dw, float* dscale,
                            int Mx, int M, int HW, int Cin, int Cout, void* workspace, size_t ws_bytes, omni_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OMNIFUSION_H_ */
