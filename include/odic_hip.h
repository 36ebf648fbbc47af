/*
 * odic_hip.h — C ABI of libodic_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * ExpansionNet v2 inference path (Swin-L/384 backbone → expansion encoder → beam-search decoder).
 *
 * The reference (nighting0le01/On_Device_Image_Captioning) has NO native code and NO FFI: its
 * boundary is a Python class contract.  This header is therefore the boundary
 * that the build's own Python host code (the on_device_image_captioning_amd package, ctypes) binds; each
 * entry point names the reference computation it replaces (file:line under /root/reference).
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless noted.
 *   - no allocation, no ownership transfer, no host synchronisation inside any entry point: the
 *     caller allocates outputs/workspaces and passes the HIP stream (hipStream_t as void*).
 *     All entry points are therefore legal inside a stream capture (hipGraph).
 *   - return 0 on success, a negative ODIC_E* code on a rejected argument, or the positive
 *     hipError_t of a failed launch.  Nothing is printed.
 *   - row-major everywhere; `ld*` are leading dimensions in ELEMENTS.
 *   - dtype codes: ODIC_F32 = 0 (float), ODIC_BF16 = 1 (bfloat16, raw uint16 storage), ODIC_FP8 = 2 (OCP e4m3,
 *     raw uint8), ODIC_F16 = 3 (IEEE half), ODIC_H2 = 4 (split fp16, see below).
 *   - ODIC_H2 ("split fp16": the operand format of the near-exact fast mode): a value x is carried as hi + lo with
 *     hi = fp16(x), lo = fp16(x - hi) — 22 significand bits — and a contraction runs as three fp16 MFMAs
 *     (hi·hi + hi·lo + lo·hi, fp32 accumulate).  Storage is 4 bytes per element, so shapes, leading dimensions and
 *     strides (in ELEMENTS) are those of the fp32 tensor it replaces; inside a row, every group of 8 consecutive
 *     elements is 32 bytes: [8 x hi | 8 x lo].  Rows start on 32-byte boundaries (base 32-byte aligned, ld % 8 == 0).
 *     All-zero bytes are the value 0, so zero-filled K padding is valid.  |x| saturates at 65504.
 *   - OUTPUT CASTS: wherever a kernel narrows an fp32 result to `out_dtype` (every odic_gemm epilogue and store path,
 *     odic_layernorm, odic_patch_merge_layernorm, the two casts), one rule per format, pinned bitwise at ties, subnormals,
 *     the range limit, ±inf and NaN by tests/test_output_casts_gpu.py:
 *       rounding   to nearest, ties to even, in every format (subnormal results included; nothing is flushed);
 *       ODIC_FP8   finite values past the range and ±inf SATURATE to ±448; NaN stays NaN (0x7F / 0xFF);
 *       ODIC_H2    finite values past the range and ±inf SATURATE to ±65504 (hi = ±65504, lo = 0); NaN stays NaN
 *                  (hi and lo both NaN);
 *       ODIC_BF16, ODIC_F16   as IEEE 754 and torch do: values that round past the largest finite one (bf16: from
 *                  0x7F7F8000; fp16: from 65520) and ±inf give ±inf; NaN stays NaN.  NO saturation: a caller that cannot
 *                  take an fp16 inf keeps its values in range (DESIGN.md "Output casts").
 *     A NaN in an input therefore always reaches the output as a NaN, never as a plausible finite value.
 */
#ifndef ODIC_HIP_H
#define ODIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ODIC_F32 0
#define ODIC_BF16 1
#define ODIC_FP8 2     /* OCP e4m3 (e4m3fn), one byte per element: the low-precision backbone mode's GEMM operands */
#define ODIC_F16 3     /* IEEE half: that mode's qkv / attention activations */
#define ODIC_H2 4      /* split fp16 (hi + lo pairs, 4 bytes per element): the near-exact fast mode's operands */

#define ODIC_ACT_NONE 0
#define ODIC_ACT_GELU 1    /* exact erf GELU (nn.GELU, swin_transformer_mod.py:87) */
#define ODIC_ACT_RELU 2
#define ODIC_ACT_SIGMOID 3

#define ODIC_EINVAL (-1)   /* bad shape / alignment / enum */
#define ODIC_ENULL (-2)    /* required pointer is NULL */
#define ODIC_EUNSUPPORTED (-3)

/* ABI version of this header; bumped on any signature change.
 *   19: the one-launch search step entry point removed (odic_logsoftmax_topk + odic_beam_step is the step).
 *   21: odic_jpeg_decode_scaled and odic_jpeg_decode_progressive_scaled added (decode at 1/2, 1/4, 1/8 scale).
 *   22: odic_resize_boxes_normalize added (batched box resize, PIL's resize(..., box=)).
 *   25: odic_group_beam_step added (diverse beam search: groups with a Hamming penalty).
 *   26: odic_topk_rows_constrained added (no-repeat n-grams, minimum length, banned words in the search).
 *       Pure additions since, the number unchanged (detect them by the symbol): odic_dynexp_fill_caches,
 *       odic_beam_reset_prefix, odic_require_beam_step, odic_cider_vectorize, odic_cider_pairs, odic_bleu_stats,
 *       odic_lcs_pairs, odic_orient_rgb8, odic_cmyk_to_rgb8, odic_jpeg_progressive_any_workspace_bytes,
 *       odic_jpeg_decode_progressive_any, odic_jpeg_decode_progressive_any_scaled.
 *   27: the two baseline per-component records and their six entry points (four components; three at any layout) removed:
 *       odic_jpeg_header_any with odic_jpeg_any_workspace_bytes, odic_jpeg_any_decode and odic_jpeg_any_decode_scaled
 *       decodes both kinds, in one call. */
#define ODIC_ABI_VERSION 27
int odic_abi_version(void);

/* Human-readable build string ("gfx950 hipcc ..."), static storage. */
const char* odic_build_info(void);

/* ---------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:   out = act(alpha * A·Wᵀ + bias) + residual
 *   A [M,K] (lda), W [N,K] (ldw) — the nn.Linear weight layout, so no transposes anywhere.
 *   bias: fp32, NULL or length N (bias_axis 0, per column) / length M (bias_axis 1, per row)
 *   residual: fp32 [M,N] (ldr) or NULL; out: `out_dtype` [M,N] (ldc)
 *   batch > 1: operands advance by the given element strides (0 = shared operand).
 *   Containment (every family, every tile configuration; pinned by tests/test_containment_gpu.py): `out` columns [N, ldc) of
 *   every row, rows >= M and the elements between batches (strideC > M·ldc) are LEFT UNTOUCHED — a caller may keep zeros
 *   there and read them as the K padding of a later product.  Nothing is read from A / a_ln / W columns [K, ld), rows
 *   >= M / >= N, residual columns [N, ldr), or past the N (M) entries of bias / col_scale / ln_colsum
 *   (test_gemm_f32_folded_layernorm_reads_exactly_n_column_sums): those bytes may hold anything, NaN included.  A refused
 *   launch writes nothing.
 *   Output cast (OUTPUT CASTS above; the same in the vector, whole-line, scalar-tail and A-resident stores of every family):
 *   nearest-even; an ODIC_FP8 out saturates at ±448 and an ODIC_H2 out at ±65504; an ODIC_BF16 / ODIC_F16 out overflows to
 *   ±inf; NaN stays NaN.  The residual is added in fp32 in front of the cast.
 * Replaces every nn.Linear on the path: swin_transformer_mod.py:190,212 (qkv/proj), :94-97
 * (Mlp fc1/fc2), :396 (PatchMerging.reduction), layers.py:49-51,99,154-161,274-276,293,306-307,
 * End_ExpansionNet_v2.py:82,97,134,137.
 * in_dtype ODIC_BF16: MFMA 16x16x32 bf16, fp32 accumulate; needs K % 64 == 0, lda/ldw % 8 == 0,
 *   16-byte aligned A/W.   in_dtype ODIC_F32: MFMA 16x16x4 f32 (exact fp32 FMA chain), any M,N,K.
 * in_dtype ODIC_FP8 / ODIC_F16 (low-precision backbone mode, BASELINE.json configs[4]): MFMA 16x16x32 fp8 / f16,
 *   fp32 accumulate, out = cast(act(alpha·col_scale[n]·(A·Wᵀ) + bias)·out_scale) + residual with out_dtype in
 *   {ODIC_F32, ODIC_F16, ODIC_FP8}; K a multiple of 64 (fp8) / 32 (f16); batch == 1.  The caller quantises: W per
 *   output channel at pack time, A per tensor with a static scale — col_scale[n] is their product.
 * in_dtype ODIC_H2 (near-exact fast mode): A and W are split-fp16 tensors, three MFMA 16x16x32 f16 per step into one
 *   fp32 accumulator; out_dtype ODIC_F32 or ODIC_H2; exact-erf GELU; K % 32 == 0, lda / ldw / strides % 8 == 0,
 *   32-byte aligned operands; any batch.  Weights may be pre-scaled by a power of two at pack time (undone in alpha).
 * ------------------------------------------------------------------------------------------- */
typedef struct odic_gemm_args {
  const void* A; const void* W; const float* bias; const float* residual; void* out;
  int32_t M, N, K;
  int64_t lda, ldw, ldr, ldc;
  int32_t batch;
  int64_t strideA, strideW, strideBias, strideR, strideC;
  float alpha;
  int32_t act;        /* ODIC_ACT_* */
  int32_t bias_axis;  /* 0: bias[n]   1: bias[m] */
  int32_t in_dtype;   /* dtype of A and W */
  int32_t out_dtype;  /* dtype of out */
  int32_t tile_cfg;   /* tile configuration, -1 = built-in choice.  bf16 (csrc/gemm_bf16.hip): 0, 1, 2, 7, 10 power-of-two tiles,
                       * 40..47 tiles of 48 x 96 wave patches (144 / 288 rows), 48 / 49 64 x 64, 50..53 the A-resident streaming
                       * kernels for K = 192 / 384 (whole tiles only; the only ones that take `a_ln`); every other value is refused.
                       * fp8 / fp16 (gemm_lowp.hip): 0..4, 5..9 = the same on the block-scaled fp8 MFMA.  split fp16 (gemm_x3.hip):
                       * 0..9, 20 / 21 the A-resident kernels for K = 192.  An unsupported (shape, configuration) pair is refused. */
  /* Optional LayerNorm of the A operand, folded (fp32 skinny-M path only: M <= 192, K % 16 == 0,
   * bias_axis 0).  The caller prepares  W' = W·diag(gamma),  ln_colsum[n] = Σ_k W'[n][k]  and
   * bias' = bias + W·beta, passes W' / bias' as W / bias, and the kernel computes
   *     out = act(rstd[m]·(alpha·A·W'ᵀ − mean[m]·ln_colsum) + bias') + residual
   *         = act(LayerNorm(A; gamma, beta, ln_eps)·Wᵀ + bias) + residual
   * with mean/rstd the moments of row m of the RAW fp32 A, accumulated from the operand fragments.
   * Neither Σa² − (Σa)²/K nor A·W'ᵀ − mean·ln_colsum is formed as written: every K-slice of a row is
   * centred on a mean of its own elements before the product, the slices' moments are merged
   * pairwise, and the column sums the centring needs are taken per slice from the W' fragments.
   * So ln_colsum is NOT the operand of a subtraction any more.  It is (1) the flag that selects the
   * fold (non-NULL) and (2) with alpha != 1 only, the factor of the term (alpha − 1)·mean[m]·ln_colsum[n]
   * that makes the result the formula above for any alpha; with alpha = 1 (every caller in this
   * project) its N values are not read.  Accuracy on offset rows (randn ± 30), constant,
   * zero, single-outlier and near-eps rows is pinned by tests/test_decoder_hard_rows_gpu.py: every
   * such row within 3e-5 of the output scale against fp64, at every tile_cfg.
   * Replaces the separate norm_1/2/3 + dec_reduce_norm launches of the decoder step
   * (layers.py:225,228,232; End_ExpansionNet_v2.py:135).  NULL = plain GEMM. */
  const float* ln_colsum; float ln_eps;
  /* Reserved (kept for the layout): pass NULL.  Ignored. */
  int32_t* workspace;
  /* fp8 / fp16 inputs only: per-output-column dequantisation factor (fp32 [N], NULL = 1) and the factor applied
   * before the output cast (0 = 1; 1/scale of the consumer's fp8 operand). */
  const float* col_scale; float out_scale;
  /* Reserved (kept for the layout): pass NULL / 0.  A non-NULL out16, stats_out or ln_stats is refused with
   * ODIC_EUNSUPPORTED before anything is launched. */
  void* out16; int64_t ld16; float* stats_out;
  const float* ln_stats;
  /* LayerNorm of the A operand computed while A is read (A-resident tile configurations only: bf16 50-53, split fp16 20 / 21 — the
   * K = 192 / 384 products of Swin stages 0-1; whole tiles, batch == 1): A = NULL and the operand is
   *     (x − mean(x)) / sqrt(var(x) + ln_eps)   of each fp32 row of a_ln [M,K] (ld_aln elements),
   * rounded to bf16 in registers; W and bias are folded by the caller as above (W' = W·diag(gamma), bias' = bias + W·beta), so
   *     out = act(alpha·LayerNorm(x; gamma, beta)·Wᵀ + bias) + residual.
   * Replaces norm1 → qkv and norm2 → fc1 (swin_transformer_mod.py:309-310, 338) by one launch each and removes the bf16
   * copy of the residual stream between them.  NULL = A is the operand. */
  const float* a_ln; int64_t ld_aln;
} odic_gemm_args;
int odic_gemm(const odic_gemm_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (eps inside sqrt, biased variance — torch.nn.LayerNorm).
 *   x fp32 [M,C] (ldx) → out `out_dtype` [M,C] contiguous (ODIC_F32 / ODIC_BF16 / ODIC_FP8 / ODIC_H2; an fp8 consumer's
 *   quantisation scale is folded into gamma / beta by the caller).   C % 4 == 0 (ODIC_H2: % 8), C <= 8192.
 *   `out` has no leading dimension: exactly M·C elements are written, nothing in front or behind; x columns [C, ldx) are
 *   not read (test_layernorm_reads_ldx_and_writes_compact_rows).
 *   Output cast (OUTPUT CASTS above; the same for odic_patch_merge_layernorm): nearest-even; ODIC_FP8 saturates at ±448,
 *   ODIC_H2 at ±65504, ODIC_BF16 overflows to ±inf; NaN stays NaN.
 * Replaces swin_transformer_mod.py:309,338 (norm1/norm2), :639 (final norm), layers.py:119,121,
 * 225,228,232 and the reduce norms End_ExpansionNet_v2.py:99,135.
 * ------------------------------------------------------------------------------------------- */
int odic_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, void* out,
                   int32_t M, int32_t C, float eps, int32_t out_dtype, void* stream);

/* Device-to-device copy of nbytes (a multiple of 16; both pointers 16-byte aligned) by a kernel of this library:
 * the pipeline's K/V hand-off from the encode stream's staging buffer to a decode lane.  Exactly nbytes of dst are written
 * (test_copy_exact_extent). */
int odic_copy(const void* src, void* dst, int64_t nbytes, void* stream);

/* Row-strided fp32 → bf16 conversion (feeds fp32 residual streams / caller tensors to the bf16 MFMA
 * GEMM).  x fp32 [M,C] (ldx) → out bf16 [M,C] (ldo); C, ldx, ldo multiples of 4.  out columns [C, ldo) are left untouched,
 * x columns [C, ldx) are not read (test_casts_respect_ldx_and_ldo; the same for the split-fp16 form below).
 * Nearest-even; values from 0x7F7F8000 up and ±inf give ±inf; NaN stays NaN (OUTPUT CASTS above). */
int odic_cast_f32_to_bf16(const float* x, int64_t ldx, void* out, int64_t ldo, int32_t M, int32_t C,
                          void* stream);
/* The same into split fp16 (ODIC_H2): C % 8 == 0, ldo % 8 == 0 (elements of 4 bytes), out 32-byte aligned.
 * hi = fp16(x), lo = fp16(x - hi), both nearest-even; |x| > 65504 and ±inf saturate to ±65504; NaN stays NaN. */
int odic_cast_f32_to_h2(const float* x, int64_t ldx, void* out, int64_t ldo, int32_t M, int32_t C, void* stream);

/* PatchMerging gather + LayerNorm(4C)  (swin_transformer_mod.py:386-395):
 *   x fp32 [B, res*res, C] → out `out_dtype` (ODIC_F32 / ODIC_BF16 / ODIC_H2) [B, (res/2)², 4C]; channel blocks in
 *   the order (0,0),(1,0),(0,1),(1,1) of the 2x2 neighbourhood (row offset, col offset).  `out` is compact: exactly
 *   B·(res/2)²·4C elements are written, nothing in front or behind (test_patch_merge_layernorm_compact_output). */
int odic_patch_merge_layernorm(const float* x, const float* gamma, const float* beta, void* out,
                               int32_t B, int32_t res, int32_t C, float eps, int32_t out_dtype,
                               void* stream);

/* PatchEmbed: Conv2d(in_chans→C, k=s=patch) + flatten + LayerNorm(C)
 * (swin_transformer_mod.py:511-519).  img fp32 [B,in_chans,H,W]; w fp32 [C,in_chans*patch*patch];
 * out fp32 [B,(H/patch)*(W/patch),C].  patch == 4, C in {64,96,128,192,256}, in_chans*16 <= 64; H and W any multiples of patch
 * (images of fewer than 64 tokens included: test_patch_embed_shapes); anything else is refused and nothing is written.  `out`
 * is compact: exactly that many elements are written (test_patch_embed_compact_output). */
int odic_patch_embed(const float* img, const float* w, const float* b, const float* gamma,
                     const float* beta, float* out, int32_t B, int32_t in_chans, int32_t H,
                     int32_t W, int32_t patch, int32_t C, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image preprocessing on the device (utils/image_utils.py:5-23: Resize((S,S)) → ToTensor → Normalize),
 * bit-exact with PIL.Image.resize(..., BILINEAR) followed by the fp32 /255, -mean, /std of torch.
 *   src_rgb  host-decoded RGB8 image in device memory, H rows of W pixels, row pitch src_stride_bytes
 *   bounds_* int32 [S, 2] (first tap, tap count), coef_* int32 [S, ksize_*] fixed-point (2^22) weights of
 *            PIL's antialiased triangle filter for that axis — computed on the host exactly as
 *            libImaging/Resample.c does (on_device_image_captioning_amd.image_utils.pil_bilinear_coeffs)
 *   tmp      uint8 workspace [H, S, 3] (the horizontally resampled image)
 *   dst      fp32 [3, S, S];  mean3 / std3 are HOST pointers to 3 floats.
 * ------------------------------------------------------------------------------------------- */
int odic_resize_bilinear_normalize(const uint8_t* src_rgb, int32_t H, int32_t W, int64_t src_stride_bytes,
                                   const int32_t* bounds_x, const int32_t* coef_x, int32_t ksize_x,
                                   const int32_t* bounds_y, const int32_t* coef_y, int32_t ksize_y,
                                   uint8_t* tmp, float* dst, int32_t out_size, const float* mean3,
                                   const float* std3, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same resize + normalise for N regions of any of several images in one call, bit-exact with
 * PIL.Image.resize((S, S), BILINEAR, box=(l, t, r, b)) (float boxes) followed by the same fp32 arithmetic.  One job per
 * region, packed by on_device_image_captioning_amd.image_utils.pack_resize_jobs, which also validates the geometry: the
 * records live in device memory and are not checked here.  The tap tables of an axis are those of
 * image_utils.pil_bilinear_coeffs_box(in_size, in0, in1, S): windows clipped to the IMAGE, not to the box, so the pixels
 * just outside a box contribute at its edges, as in Pillow.
 *   src_off             byte offset of the source image (its pixel (0, 0)) from src_base: images decoded by one
 *                       odic_jpeg_decode call share one RGB buffer, other sets are gathered into one first
 *   src_pitch           bytes from one source row to the next (>= 3 W)
 *   tmp_off             byte offset of the job's n_rows x S x 3 slice of tmp (the horizontally resampled rows)
 *   H, W                size of the source image
 *   row_first, n_rows   the source rows the vertical taps of the box touch, [row_first, row_first + n_rows): the first
 *                       tap of output row 0 to the last tap of output row S - 1; only these are resampled horizontally
 *   bounds_x, bounds_y  int32 index in bounds_pool of the axis's [S, 2] (first tap, tap count) table; the y table holds
 *                       source rows of the image (the kernel subtracts row_first), so a table can serve several jobs
 *   coef_x, coef_y      int32 index in coef_pool of the axis's [S, ksize] fixed-point (2^22) weights
 *   ksize_x, ksize_y    row length of those weight tables
 * ------------------------------------------------------------------------------------------- */
typedef struct odic_resize_job {
  int64_t src_off, src_pitch, tmp_off;
  int32_t H, W, row_first, n_rows;
  int32_t bounds_x, coef_x, bounds_y, coef_y;
  int32_t ksize_x, ksize_y;
} odic_resize_job;

/* jobs, src_base, bounds_pool, coef_pool, tmp, dst are DEVICE pointers; mean3 / std3 HOST pointers to 3 floats.  Job j
 * writes dst[j] = fp32 [3, S, S] (S = out_size).  Two launches for any n_jobs, on `stream`, no allocation, no host
 * synchronisation, capturable: the horizontal pass on a grid of (ceil(S / 256), max_rows, n_jobs) blocks (max_rows: the
 * largest n_rows of the jobs; rows at or beyond a job's n_rows exit) and the vertical pass + normalise on
 * (ceil(S / 256), S, n_jobs).  Exactly n_jobs·3·S·S floats of dst are written and at most tmp_bytes of tmp: a job whose
 * tmp slice would end behind tmp_bytes is skipped (test_resize_boxes_containment).  ODIC_ENULL for a null pointer;
 * ODIC_EINVAL for n_jobs outside 1..65535, out_size or max_rows outside 1..65535, or tmp_bytes below one row (3·S). */
int odic_resize_boxes_normalize(const odic_resize_job* jobs, int32_t n_jobs, const uint8_t* src_base,
                                const int32_t* bounds_pool, const int32_t* coef_pool, uint8_t* tmp, size_t tmp_bytes,
                                float* dst, int32_t out_size, int32_t max_rows, const float* mean3, const float* std3,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * EXIF orientation (tag 0x0112) applied to packed RGB8 images on the device: one job per image, a pure permutation of
 * its pixels, bit for bit Pillow's Image.transpose with the method ImageOps.exif_transpose picks:
 *     2 FLIP_LEFT_RIGHT   3 ROTATE_180   4 FLIP_TOP_BOTTOM   5 TRANSPOSE   6 ROTATE_270   7 TRANSVERSE   8 ROTATE_90
 *   src_off            byte offset of the source image (its pixel (0, 0)) from src_base; any value, odd ones included
 *   dst_off            byte offset of the output image from dst_base; any value
 *   src_stride_bytes   bytes from one source row to the next (>= 3 W); any value, odd ones included
 *   H, W               size of the SOURCE image
 *   orientation        2..8
 * The output rows are packed: H rows of 3·W bytes for orientations 2..4, W rows of 3·H bytes for 5..8; exactly those
 * 3·H·W bytes from dst_off on are written (test_orient_kernel_gpu.py).  Source and destination must NOT overlap, within a
 * job or between jobs: tiles are read and written in no particular order.
 * ------------------------------------------------------------------------------------------- */
typedef struct odic_orient_job {
  int64_t src_off, dst_off, src_stride_bytes;
  int32_t H, W, orientation;
} odic_orient_job;

/* jobs is a HOST pointer (the records are checked here and travel as kernel arguments); src_base and dst_base are DEVICE
 * pointers.  One launch per 64 jobs, on `stream`, no allocation, no host synchronisation, capturable: the grid walks
 * the 64 x 64 pixel tiles of all jobs of the launch.  n_jobs == 0 succeeds and launches nothing.  ODIC_EINVAL, before any
 * launch and with nothing written: n_jobs < 0; jobs, src_base or dst_base NULL while n_jobs > 0; a job with an orientation
 * outside 2..8, H <= 0, W <= 0, src_stride_bytes < 3·W, or more than 2^31 - 1 tiles. */
int odic_orient_rgb8(const odic_orient_job* jobs, int32_t n_jobs, const uint8_t* src_base, uint8_t* dst_base,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched JPEG decode on the device, baseline files here and progressive ones below (utils/image_utils.py:7, PIL_Image.open), bit-exact with
 * np.asarray(PIL.Image.open(f)) on Pillow's libjpeg-turbo default path (ISLOW IDCT, fancy upsampling,
 * fixed-point YCbCr→RGB).  The host parser (on_device_image_captioning_amd/jpeg.py) walks the markers up to
 * SOS and fills one odic_jpeg_header per image; only its `device` kind is passed here: 8-bit SOF0/SOF1
 * Huffman, one interleaved scan of 3 YCbCr components, luma sampling 1x1 / 2x1 / 2x2 with 1x1 chroma,
 * restart interval present or absent; or, when the caller asked for non_rgb="convert", one scan of ONE component
 * (sampling 3, grayscale): one 8x8 block per MCU in block-raster order, mcus_x = ceil(W / 8), mcus_y = ceil(H / 8), the
 * restart interval counted in blocks, qt[0], table 0 (DC) and table 3 (AC) filled and the other slots zero, one plane of
 * whole blocks, and R = G = B = Y in the output (Pillow's L → RGB).  A batch may mix the samplings.  All offsets are set
 * by that parser.
 *   data_off / data_end  byte range in `data` from the first entropy-coded byte to the end of the file,
 *                        at most 2^27 bytes (bit positions are int32)
 *   out_off              byte offset of the image's H×W×3 uint8 RGB output in `out`
 *   scan_off / coef_off / plane_off / int_off / unit_off   the image's slices of the workspace regions:
 *                        compacted scan bytes (4-aligned, round_up(data_end - data_off, 4) + 16 reserved),
 *                        coefficient blocks, component planes (bytes, 16-aligned), intervals (n_intervals
 *                        + 1 slots), units (n_units slots)
 *   restart              MCUs per restart interval (all MCUs without DRI); n_intervals = ceil(MCUs / restart)
 *   n_units              ceil(8 (data_end - data_off) / subseq_bits) + n_intervals
 *   qt                   quantisation table of each component, natural order
 *   lut/maxcode/valoff/huffval  tables 0-2: DC of components 0-2, 3-5: their AC.  lut[peek9] = (len << 8) |
 *                        symbol for codes of at most 9 bits, else 0; longer codes: the first length l with
 *                        code(l) <= maxcode[l] gives huffval[code + valoff[l]]
 * ------------------------------------------------------------------------------------------- */
typedef struct odic_jpeg_header {
  int64_t data_off, data_end, out_off, scan_off, coef_off, plane_off;
  int32_t int_off, unit_off, width, height;
  int32_t sampling;              /* 0: 4:4:4, 1: 4:2:2 (h2v1), 2: 4:2:0 (h2v2), 3: one component (gray) */
  int32_t mcus_x, mcus_y, restart, n_intervals, n_units;
  uint16_t qt[3][64];
  uint16_t lut[6][512];
  int32_t maxcode[6][18];
  int32_t valoff[6][18];
  uint8_t huffval[6][256];
} odic_jpeg_header;

/* One decode call.  headers, data, out, status are DEVICE pointers; status int32 [n_images] receives 0 for a
 * decoded image and 1 for one whose entropy data did not decode (invalid code, unexpected marker, restart
 * markers out of sequence, an interval whose MCUs need bits past its end, no EOI) or whose coefficients leave
 * the range where libjpeg-turbo's SIMD and C IDCTs agree (a dequantised coefficient or pass-1 value beyond
 * ±8191, a result beyond [-512, 511], a DC beyond int16): the caller decodes those again on the host.  subseq_bits (32..4096): bits per speculative unit; max_sync_passes (0..64): synchronisation
 * passes before the intervals that have not converged are decoded serially (0: all of them).  The max_* and
 * total_* fields are the maxima / sums of the headers' sizes (widths, heights, units, intervals + 1 per image,
 * blocks, reserved scan bytes, plane bytes) that size the grids and the workspace. */
typedef struct odic_jpeg_batch {
  const void* headers;           /* odic_jpeg_header [n_images] */
  const uint8_t* data;
  uint8_t* out;
  int32_t* status;
  int32_t n_images, subseq_bits, max_sync_passes, max_units, max_intervals, max_width, max_height, pad;
  int64_t max_blocks, max_scan_bytes, total_scan_bytes, total_intervals, total_units, total_blocks,
      total_plane_bytes;
} odic_jpeg_batch;

/* Workspace bytes odic_jpeg_decode needs for this batch (host-side query, reads no device memory); 0 for an
 * invalid descriptor. */
size_t odic_jpeg_workspace_bytes(const odic_jpeg_batch* batch);

/* Decode the batch on `stream` (one pass of launches, no host synchronisation, capturable).  At most ws_bytes =
 * odic_jpeg_workspace_bytes(batch) of `workspace` are touched, `data` is only read, and exactly the images' H·W·3 bytes of
 * `out` and n_images entries of `status` are written (test_jpeg_decode_stays_inside_its_workspace). */
int odic_jpeg_decode(const odic_jpeg_batch* batch, void* workspace, size_t ws_bytes, void* stream);

/* The same decode at 1/1, 1/2, 1/4 or 1/8 of each frame's size, bit-exact with Pillow's Image.draft (libjpeg's
 * scale_denom): scale_log2 is a DEVICE pointer to int32 [n_images], each 0..3 (jpeg.draft_scale picks it as Pillow
 * does).  Image i yields ceil(W / s) × ceil(H / s)
 * × 3 bytes at its out_off, s = 1 << scale_log2[i]; out_off, and the batch's max_width / max_height, are those of the
 * scaled sizes, while width, height, mcus_x and mcus_y stay the frame's own.  Everything up to the coefficients runs
 * as in odic_jpeg_decode; the inverse transforms are libjpeg's reduced ones (8 / s samples per luma block side;
 * 4:2:0 chroma takes twice that and needs no upsampling, 4:2:2 chroma is upsampled horizontally).  Workspace query,
 * workspace layout, status rule (the ±8191 / [-512, 511] limits apply to what the reduced transform reads and makes) and
 * containment are those of odic_jpeg_decode.  ODIC_ENULL for a null scale_log2. */
int odic_jpeg_decode_scaled(const odic_jpeg_batch* batch, const int32_t* scale_log2, void* workspace, size_t ws_bytes,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * Baseline files with per-component sampling, bit-exact with np.asarray(PIL.Image.open(f).convert("RGB")): four
 * components (CMYK and YCCK: print workflows, Photoshop; jpeg.parse(..., "convert", cmyk="device")) and three components
 * at every sampling layout libjpeg decodes that odic_jpeg_header cannot describe, stored as YCbCr or as RGB
 * (jpeg.parse(..., layouts="all")).  Both are 8-bit SOF0/SOF1 Huffman frames with one interleaved scan of all components
 * in frame order; one batch may mix them.  The record has odic_jpeg_header's offset and size fields with the same
 * meaning (mcus_x = ceil(W / (8 max h)), mcus_y = ceil(H / (8 max v)); restart in MCUs), and instead of `sampling`:
 *   color        three components: 1 the components are R, G, B as stored (Adobe transform 0, or ids 'R', 'G', 'B' with
 *                neither a JFIF nor an Adobe marker), 0 Y, Cb, Cr (libjpeg's ycc_rgb_convert); four components: 1 Adobe
 *                transform 2, components 0..2 are YCbCr of the complemented C, M, Y (libjpeg's ycck_cmyk_convert), 0 the
 *                components are C, M, Y, K as stored.  odic_jpeg_prog_header_any's `color`
 *   h / v        sampling factors of each component (entries from ncomp on are not read).  An MCU holds h[c]·v[c] blocks
 *                of component c, row by row, in component order; the planes follow each other in component order from
 *                plane_off, plane c being mcus_x·8·h[c] wide and mcus_y·8·v[c] high (64 bytes per block in all)
 *   ncomp        3 or 4
 *   qt           quantisation table of each component, natural order
 *   lut/maxcode/valoff/huffval  tables 0-3: DC of components 0-3, 4-7: their AC, in odic_jpeg_header's form; the slots
 *                of a component the frame lacks stay zero
 * Frame rules, checked on the device, those of odic_jpeg_prog_header_any: ncomp 3 or 4; factors in 1..4, every factor a
 * divisor of the largest in its direction, at most 10 blocks per MCU (libjpeg's limit); four components: component 0 at
 * 1x1, 2x1 or 2x2 and every other one at 1x1 or at component 0's sampling.  A record that breaks them is not decoded:
 * its status is 1 and none of its pixels are written.
 * Every component, component 0 and K included, is brought to the output grid by libjpeg's rule for its ratios (rh, rv) =
 * (max h / h[c], max v / v[c]): (1,1) as it is; (2,1) / (2,2) the fancy triangle filters, or replication where the
 * component is at most two samples wide; (1,2) h1v2_fancy_upsample at every width; any other ratio replication.  Three
 * components are then converted or copied by `color`; of four, every sample is complemented (Pillow reads all four-layer
 * JPEGs as "CMYK;I") after the YCCK step and the pixel goes through Pillow's CMYK → RGB.
 * ------------------------------------------------------------------------------------------- */
typedef struct odic_jpeg_header_any {
  int64_t data_off, data_end, out_off, scan_off, coef_off, plane_off;
  int32_t int_off, unit_off, width, height;
  int32_t color;
  int32_t mcus_x, mcus_y, restart, n_intervals, n_units;
  int32_t h[4], v[4];
  int32_t ncomp, pad;
  uint16_t qt[4][64];
  uint16_t lut[8][512];
  int32_t maxcode[8][18];
  int32_t valoff[8][18];
  uint8_t huffval[8][256];
} odic_jpeg_header_any;             /* 12032 bytes */

/* odic_jpeg_workspace_bytes / odic_jpeg_decode for a batch whose `headers` are odic_jpeg_header_any [n_images]: the same
 * descriptor, launches, workspace layout, status rule and contract (all launches on `stream`, no allocation, no host
 * synchronisation; at most the queried workspace bytes are touched, and exactly the images' H·W·3 bytes of `out` and
 * n_images entries of `status` are written — test_jpeg_any_decode_stays_inside_its_buffers).  An out_off that is a
 * multiple of 4 lets the colour kernel store whole words. */
size_t odic_jpeg_any_workspace_bytes(const odic_jpeg_batch* batch);
int odic_jpeg_any_decode(const odic_jpeg_batch* batch, void* workspace, size_t ws_bytes, void* stream);

/* odic_jpeg_decode_scaled for odic_jpeg_header_any records: scale_log2 (DEVICE int32 [n_images], each 0..3), out_off,
 * max_width / max_height and the output sizes as there; ODIC_ENULL for a null scale_log2; a value outside 0..3 leaves the
 * image undecoded with status 1 and nothing of it written.  Every component takes libjpeg's own transform size n at the
 * scale (jdmaster.c; jpeg.scaled_components): it starts at 8 / s and doubles while it is below 8 and 2 n·h[c] still
 * divides (8 / s)·max h, and the same down.  Plane c is mcus_x·n·h[c] wide and mcus_y·n·v[c] high; the planes follow each
 * other from plane_off, each rounded up to a multiple of 16 bytes (at full size that is the layout above).  The
 * upsampling that remains, by ((8 / s)·max h) / (n·h[c]) across and the same down, follows the rule above, with the
 * triangle filters only while 8 / s > 1 (at 1/8 every ratio is replication).  Workspace query, status rule and
 * containment are odic_jpeg_any_decode's (test_scaled_decodes_stay_inside_their_buffers). */
int odic_jpeg_any_decode_scaled(const odic_jpeg_batch* batch, const int32_t* scale_log2, void* workspace, size_t ws_bytes,
                                void* stream);

/* The last stage of the four-component decode on its own: n_pixels interleaved C, M, Y, K bytes (DEVICE pointers) →
 * interleaved RGB, as Pillow's convert("RGB") of a CMYK image: per channel x with nk = 255 - K, t = x·nk + 128,
 * out = clip(nk - (((t >> 8) + t) >> 8), 0, 255).  invert != 0: every input sample is first replaced by 255 - x (the
 * "CMYK;I" unpacking of a JPEG).  n_pixels == 0 launches nothing.  ODIC_ENULL for a null pointer, ODIC_EINVAL for a
 * negative n_pixels. */
int odic_cmyk_to_rgb8(const uint8_t* cmyk, uint8_t* rgb, int64_t n_pixels, int invert, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Progressive files (8-bit SOF2 Huffman, 3 YCbCr components, the samplings above — sampling 3 included: one component,
 * every scan non-interleaved over its block raster, comp_mask 1), bit-exact with Pillow as well.
 * The host parser (jpeg.parse_progressive) reads the whole scan script and accepts what libjpeg accepts without a
 * warning and what leaves every coefficient at full precision by EOI; it packs one odic_jpeg_prog_header per image,
 * one odic_jpeg_scan per scan and one odic_jpeg_table per distinct Huffman table of the batch.
 *   header   out_off / coef_off / plane_off as above; n_intervals = the sum of its scans' n_intervals
 *   scan     data_off / data_end: the scan's entropy-coded bytes in `data`, from the byte behind the SOS header to the
 *            marker that closes the scan (exclusive); scan_off: its compacted bytes in the workspace (4-aligned,
 *            round_up(data_end - data_off, 4) + 16 reserved); int_off: its n_intervals + 1 interval slots;
 *            n_units: what the scan walks — the frame's MCUs for an interleaved scan, else the blocks of the component's
 *            own raster, ceil(ceil(W·h/hmax)/8) (= blocks_w) by ceil(ceil(H·v/vmax)/8); restart: units per restart
 *            interval (n_units without DRI), n_intervals = ceil(n_units / restart); comp_mask: bit c = frame component c
 *            takes part; ss / se / ah / al: the SOS parameters; level: 1 + the highest level of an earlier scan of the
 *            image that shares a component and overlaps the band (an AC scan also follows its component's first DC scan);
 *            table: indices into `tables` — the DC table of each participating component in order (first DC pass) or the
 *            AC table in [0] (AC scans); -1 where none is needed
 *   scans are sorted by level: level l (0-based) is scans [level_first[l], level_first[l + 1]), at most 65535 of them, and
 *   level_intervals[l] is the largest n_intervals among them.  One launch per level decodes all its scans concurrently.
 * ------------------------------------------------------------------------------------------- */
#define ODIC_JPEG_MAX_SCANS 64   /* scans per image, and so levels per batch; files with more go to the host */

typedef struct odic_jpeg_table {
  uint16_t lut[512];
  int32_t maxcode[18];
  int32_t valoff[18];
  uint8_t huffval[256];
} odic_jpeg_table;

typedef struct odic_jpeg_prog_header {
  int64_t out_off, coef_off, plane_off;
  int32_t width, height, sampling, mcus_x, mcus_y, n_intervals;
  uint16_t qt[3][64];
} odic_jpeg_prog_header;

typedef struct odic_jpeg_scan {
  int64_t data_off, data_end, scan_off;
  int32_t image, int_off, n_intervals, restart, n_units, blocks_w, comp_mask, ss, se, ah, al, level;
  int32_t table[3];
  int32_t pad;                   /* odic_jpeg_decode_progressive_any: the fourth DC table index of an interleaved first DC
                                    scan of four components, else -1; the other entry points never read it */
} odic_jpeg_scan;

typedef struct odic_jpeg_prog_batch {
  const void* headers;           /* odic_jpeg_prog_header [n_images] */
  const void* scans;             /* odic_jpeg_scan [n_scans], sorted by level */
  const void* tables;            /* odic_jpeg_table [n_tables] */
  const uint8_t* data;
  uint8_t* out;
  int32_t* status;
  int32_t n_images, n_scans, n_tables, n_levels, max_width, max_height, pad0, pad1;
  int64_t max_blocks, total_scan_bytes, total_intervals, total_blocks, total_plane_bytes;
  int32_t level_first[ODIC_JPEG_MAX_SCANS + 1];
  int32_t level_intervals[ODIC_JPEG_MAX_SCANS];
  int32_t pad2;
} odic_jpeg_prog_batch;

/* Workspace bytes odic_jpeg_decode_progressive needs (host-side query); 0 for an invalid descriptor. */
size_t odic_jpeg_progressive_workspace_bytes(const odic_jpeg_prog_batch* batch);

/* Diagnostic: byte offset inside that workspace of the int16 coefficient blocks ([total_blocks][64], natural order,
 * image i at block coef_off, MCU by MCU), valid after a decode until the workspace is reused; 0 for an invalid descriptor. */
size_t odic_jpeg_progressive_coef_offset(const odic_jpeg_prog_batch* batch);

/* Decode the batch on `stream`: same contract as odic_jpeg_decode (all launches on the stream, no allocation, no host
 * synchronisation, capturable; only `workspace`, `out` and `status` are written —
 * test_jpeg_progressive_decode_stays_inside_its_workspace).  status 1: a marker other than RSTn inside a scan, too few or too
 * many intervals, an invalid code, an EOB run or coefficient index past the band, bits needed past an interval's end, or
 * coefficients outside the IDCT's range as above.  The parser vouches for the script and the closing EOI. */
int odic_jpeg_decode_progressive(const odic_jpeg_prog_batch* batch, void* workspace, size_t ws_bytes, void* stream);

/* odic_jpeg_decode_scaled for progressive files: scale_log2 as there, everything else as odic_jpeg_decode_progressive. */
int odic_jpeg_decode_progressive_scaled(const odic_jpeg_prog_batch* batch, const int32_t* scale_log2, void* workspace,
                                        size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Progressive files with per-component sampling: four components (CMYK / YCCK) and three components at the layouts of
 * odic_jpeg_header_any, YCbCr or RGB, bit-exact with np.asarray(PIL.Image.open(f).convert("RGB")).
 * jpeg.parse_progressive(..., cmyk="device") / (..., layouts="all") admits them.  The record starts with
 * odic_jpeg_prog_header's fields (`color` in the place of `sampling`) and goes on with the frame:
 *   color        three components: 1 the components are R, G, B as stored, 0 Y, Cb, Cr;
 *                four components: 1 YCCK, 0 CMYK as stored (odic_jpeg_header_any's `color`)
 *   ncomp        3 or 4
 *   h / v        sampling factors of each component (entries from ncomp on are not read).  mcus_x = ceil(W / (8 max h)),
 *                mcus_y = ceil(H / (8 max v)); coefficient blocks MCU by MCU and planes as odic_jpeg_header_any has them
 *   qt           quantisation table of each component, natural order
 * Frame rules, checked on the device: ncomp 3 or 4; factors in 1..4, every factor a divisor of the largest in its
 * direction, at most 10 blocks per MCU; four components: component 0 at 1x1, 2x1 or 2x2 and every other one at 1x1 or at
 * component 0's sampling.  Scans are odic_jpeg_scan records under the rules above with comp_mask four bits wide and, for
 * an interleaved first DC scan of four components, the fourth table index in `pad`; an interleaved scan walks the
 * frame's MCUs (largest factors) whichever components it names, a single-component scan the component's own raster.
 * A record that breaks the frame rules, or a scan of it whose mask names a component the frame lacks, is not decoded.
 * An image with status 1 — by these rules or by those of odic_jpeg_decode_progressive — has none of its pixels written.
 * Upsampling and colour are odic_jpeg_any_decode's; at a reduced scale (odic_jpeg_decode_progressive_any_scaled)
 * those of odic_jpeg_any_decode_scaled.
 * ------------------------------------------------------------------------------------------- */
typedef struct odic_jpeg_prog_header_any {
  int64_t out_off, coef_off, plane_off;
  int32_t width, height, color, mcus_x, mcus_y, n_intervals;
  int32_t ncomp, pad;
  int32_t h[4], v[4];
  uint16_t qt[4][64];
} odic_jpeg_prog_header_any;        /* 600 bytes */

/* odic_jpeg_progressive_workspace_bytes / odic_jpeg_decode_progressive for a batch whose `headers` are
 * odic_jpeg_prog_header_any [n_images]: the same descriptor, workspace layout, per-level launches and contract (all
 * launches on `stream`, no allocation, no host synchronisation; only `workspace`, `out` and `status` are written —
 * test_progressive_any_decode_stays_inside_its_workspace).  An out_off that is a multiple of 4 lets the colour kernels
 * store whole words. */
size_t odic_jpeg_progressive_any_workspace_bytes(const odic_jpeg_prog_batch* batch);
int odic_jpeg_decode_progressive_any(const odic_jpeg_prog_batch* batch, void* workspace, size_t ws_bytes, void* stream);

/* odic_jpeg_any_decode_scaled for odic_jpeg_prog_header_any records: the scans decode as at
 * full size, the inverse transforms, planes, upsampling and output follow scale_log2 as there. */
int odic_jpeg_decode_progressive_any_scaled(const odic_jpeg_prog_batch* batch, const int32_t* scale_log2,
                                            void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Swin (shifted-)window attention core  (WindowAttention.forward swin_transformer_mod.py:193-211
 * plus the roll / window_partition / window_reverse / roll index maps of :312-334, folded into the
 * kernel's loads and stores so no permuted copy is ever materialised):
 *   qkv  `dtype` [B*res*res, 3C]   token-major output of the qkv Linear, columns (3, heads, 32)
 *   bias_table fp32 [(2ws-1)², heads]   relative_position_bias_table; the index buffer (:163-173)
 *        and the SW-MSA mask (:281-297, values 0/-100) are recomputed from coordinates.
 *   bias_shifted_prescaled (optional, bf16 path, ws = 12) fp32 [heads, 4, 576]: per head four copies of the
 *        x-reversed bias table with rows padded to 24, R[r·24 + c'] = bias_table[r·23 + (22 - c')] / scale,
 *        copy s holding R shifted by s floats (copy_s[i] = R[i + s]) — the four keys of an accumulator quad
 *        are then ONE aligned 16-byte LDS read (the gather of :196-198 without a dense [ws², ws²] tensor).
 *        The fast kernel keeps the 9 KiB in LDS, loads the bias as the accumulator init of the q·kᵀ MFMA and
 *        applies scale·log2(e) afterwards (base-2 softmax).  NULL → the table is used (slower kernel).
 *   out  `dtype` [B*res*res, C]    softmax(q·kᵀ·scale + bias + mask)·v, heads concatenated,
 *        written back at the un-shifted token positions (ready for the proj Linear).  Compact: exactly B·res²·C elements
 *        are written and nothing outside qkv's B·res²·3C is read, for every dtype, B and shift
 *        (test_window_attention_front_and_back_guards).
 * head_dim is 32 (every Swin-L stage), ws*ws <= 144, res % ws == 0, 0 <= shift < ws.
 * dtype ODIC_H2 (near-exact fast mode; needs bias_shifted_prescaled, ws = 12): qkv and out are split-fp16 tensors,
 *        q·kᵀ and P·v run as three fp16 MFMAs each, the softmax between them in fp32.
 * ------------------------------------------------------------------------------------------- */
int odic_window_attention(const void* qkv, const float* bias_table, const float* bias_shifted_prescaled,
                          void* out, int32_t B, int32_t res, int32_t C, int32_t heads, int32_t ws,
                          int32_t shift, float scale, int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * norm1 → qkv Linear → window attention core of one Swin block in ONE launch (swin_transformer_mod.py:309-334 with
 * WindowAttention.forward :222-263 up to, not including, the proj Linear), for the stage of width C = 192 (ws = 12):
 *   x        fp32 [B*res*res, C] (ldx)   the residual stream (token-major, un-shifted, un-partitioned)
 *   w_qkv_folded bf16 [3C, C], b_qkv_folded fp32 [3C]:  W·diag(gamma) and bias + W·beta of norm1 → qkv (the caller folds the
 *            LayerNorm's affine part at pack time; the kernel computes (x − mean)/sqrt(var + ln_eps) in registers)
 *   bias_shifted_prescaled fp32 [heads, 4, 576]   as for odic_window_attention
 *   out      bf16 [B*res*res, C]   attention output at the un-shifted token positions (ready for the proj Linear); compact:
 *            exactly B·res²·C elements are written; x columns [C, ldx) are not read (test_swin_qkv_attention_ldx_and_guards)
 * One block per window keeps its 144 normalised rows as MFMA fragments in registers; q / k / v of a head never leave the
 * chip.  Results are bit-identical to odic_gemm(a_ln = x, …) followed by odic_window_attention (bf16).
 * ------------------------------------------------------------------------------------------- */
int odic_swin_qkv_attention(const float* x, int64_t ldx, const void* w_qkv_folded, const float* b_qkv_folded,
                            const float* bias_shifted_prescaled, void* out, int32_t B, int32_t res, int32_t C,
                            int32_t heads, int32_t ws, int32_t shift, float scale, float ln_eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * qkv Linear → window attention core of one Swin block in ONE launch for the wide stages (WindowAttention.forward
 * swin_transformer_mod.py:222-263 up to, not including, the proj Linear, with the shift / partition / reverse of :312-334):
 *   xn       bf16 [B*res*res, C] compact   the norm1 output (token-major, un-shifted, un-partitioned)
 *   w_qkv    bf16 [3C, C] compact, b_qkv fp32 [3C]   the qkv Linear, unpacked
 *   bias_shifted_prescaled fp32 [heads, 4, 576]   as for odic_window_attention (required)
 *   out      bf16 [B*res*res, C]   attention output at the un-shifted token positions (ready for the proj Linear); compact:
 *            exactly B·res²·C elements are written
 * One block is the tiled GEMM's 144 x 288 tile read as (window, three heads): q / k / v of a head never leave the chip.
 * Results are bit-identical to odic_gemm(tile_cfg = 41, bf16 out) followed by odic_window_attention (bf16, packed bias).
 * The tile is chosen by rule: the call is legal inside a stream capture at a shape never run before.
 * ws = 12, head dim 32 (heads·32 = C), heads % 3 == 0, C % 64 == 0: ODIC_EUNSUPPORTED otherwise.  res % ws == 0,
 * 0 <= shift < ws, xn / w_qkv / b_qkv / bias_shifted_prescaled 16-byte and out 8-byte aligned: ODIC_EINVAL otherwise.
 * ODIC_ENULL for a null operand.  All before any launch.
 * ------------------------------------------------------------------------------------------- */
int odic_swin_qkv_attention_tiled(const void* xn, const void* w_qkv, const float* b_qkv,
                                  const float* bias_shifted_prescaled, void* out, int32_t B, int32_t res, int32_t C,
                                  int32_t heads, int32_t ws, int32_t shift, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The MLP half of one Swin block in ONE launch (swin_transformer_mod.py:338: x + mlp(norm2(x))),
 * for the stage of width C = 192:
 *   x        fp32 [M, C] (ldx)           the residual stream after the attention half
 *   w1_folded bf16 [4C, C], b1_folded fp32 [4C]:  W·diag(gamma) and bias + W·beta of norm2 → fc1 (the caller folds the
 *            LayerNorm's affine part at pack time; the kernel computes (x − mean)/sqrt(var + ln_eps) in registers)
 *   w2       bf16 [C, 4C], b2 fp32 [C], alpha2:  fc2; the product is scaled by alpha2 before the bias is added
 *   out      fp32 [M, C] (ldo)           x + alpha2·GELU(LN0(x)·w1ᵀ + b1)·w2ᵀ + b2.  May be x itself (ldo = ldx): every row
 *            panel is read and written by one block only.  Any other overlap of out and x is not supported.
 * The bf16 hidden activations [M, 4C] never leave the registers: a wave's finished fc1 accumulators are, after GELU and
 * rounding, its fc2 operand fragments.  Results are bit-identical to odic_gemm(a_ln = x, GELU, bf16 out) followed by
 * odic_gemm(hidden, w2, residual = x, fp32 out).  Exactly M·C elements are written (columns [C, ldo) are untouched) and
 * x columns [C, ldx) are not read.
 * C = 192, M a positive multiple of 128, ldx and ldo multiples of 4 and >= C, x / out / w1_folded / w2 16-byte aligned:
 * ODIC_EINVAL otherwise, ODIC_ENULL for a null operand, both before any launch.
 * ------------------------------------------------------------------------------------------- */
int odic_swin_mlp(const float* x, int64_t ldx, const void* w1_folded, const float* b1_folded, const void* w2,
                  const float* b2, float alpha2, float* out, int64_t ldo, int32_t M, int32_t C, float ln_eps,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Static expansion (encoder) helpers — layers.py:45-102.  The contractions run through
 * odic_gemm; these kernels do the relu/mask/L1-normalise steps in between.
 *   z fp32 [B, nq, S]: Q·Kᵀ/sqrt(d).
 *   fw:  pos = relu(z)·valid, neg = relu(-z)·valid, each row divided by (rowsum + eps) over S
 *        (layers.py:56-61) → pos_fw, neg_fw `out_dtype` [B, nq, ld_fw].  enc_len[b] = #valid keys.
 *   bw:  relu(±zᵀ), each of the `ngroups` column groups L1-normalised separately (layers.py:67-79)
 *        and pre-divided by ngroups (:84-85) → pos_bw, neg_bw `out_dtype` [B, S, ld_bw].
 *   ld_fw >= S and ld_bw >= nq: the padding columns [S, ld_fw) / [nq, ld_bw) are ZERO-FILLED (the opposite of odic_gemm's
 *        outputs; nothing beyond the last row is written — test_stcexp_normalize_zero_fills_its_padding), so the outputs can be the
 *        K-padded operands of odic_gemm (bf16 needs K % 64 == 0, ODIC_H2 K % 32 == 0); out_dtype ODIC_F32 / ODIC_BF16 /
 *        ODIC_H2.
 *   group_meta: device int32 [ngroups+1+nq] = exclusive prefix sums of the group sizes (last = nq)
 *        followed by the group index of every query row.
 *   colsum_ws: fp32 scratch [B*ngroups*2*S].
 *   scale_fw / scale_bw: factors applied to the fw / bw tables on output (1 = as the reference; the split-fp16 mode
 *        writes them times a power of two so that the lo halves of these small weights stay fp16 normals, and
 *        undoes it in the consuming product's alpha).
 * ------------------------------------------------------------------------------------------- */
int odic_stcexp_normalize(const float* z, const int32_t* enc_len, const int32_t* group_meta,
                          int32_t ngroups, void* pos_fw, void* neg_fw, int64_t ld_fw, void* pos_bw,
                          void* neg_bw, int64_t ld_bw, float* colsum_ws, int32_t B, int32_t nq,
                          int32_t S, float eps, float scale_fw, float scale_bw, int32_t out_dtype, void* stream);

/* out = x + sigmoid(sel_pre)·a + (1-sigmoid(sel_pre))·b     (layers.py:99-100 + the residual add of
 * EncoderLayer :120); all fp32 [M, d] with row strides.  out columns [d, ldo) are left untouched and the inputs' columns
 * beyond d are not read, so out may be a column block of the buffer x lives in (test_selector_mix_leading_dimensions). */
int odic_selector_mix(const float* x, int64_t ldx, const float* sel_pre, int64_t lds,
                      const float* a, int64_t lda, const float* b, int64_t ldb, float* out,
                      int64_t ldo, int32_t M, int32_t d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Incremental decoder step (exact because the decoder is causal).
 * N = number of live sequences (images × beams), laid out image-major: seq = img*beams + beam.
 * `pos` (device int32 scalar) is the position being processed; kernels read it from memory so one
 * captured graph can be replayed for every step.
 * ------------------------------------------------------------------------------------------- */

/* y[n,:] = embed[tok[n]]·sqrt(d) + pos_table[pos]   (layers.py:16-17, End_ExpansionNet_v2.py:118-121).
 * pos_rows = rows of pos_table (pos_encoder = nn.Embedding(max_seq_len, d), End_ExpansionNet_v2.py:105): *pos is device
 * memory, so the bound is checked ON the device — a launch with *pos outside [0, pos_rows) writes nothing.  y columns
 * [d, ldy) are left untouched (test_dec_embed_ldy). */
int odic_dec_embed(const int64_t* tokens, const float* embed, const float* pos_table,
                   const int32_t* pos, float* y, int64_t ldy, int32_t N, int32_t d, int32_t pos_rows,
                   float scale, void* stream);

/* Dynamic expansion for the newest position (layers.py:152-204), with per-position caches.
 *   lin fp32 [N, >=5d] (ldlin): cond | key | class_a | class_b | selector-pre-activation of
 *        LN1(y) at `pos`
 *   qexp, bexp fp32 [E, d]: query_exp_vectors / bias_exp_vectors
 *   caches (fp32), indexed [pos][seq_slot]:  cond_c, key_c, va_c, vb_c  [T, N, d]
 *                                            wfa_c, wfb_c  [T, N, T, E] — the normalised FORWARD weights of that
 *                                               position's E expansion queries over its keys 0..pos (:165-176);
 *                                               the (t·E) x d class matrices of :177-180,199-200 are never formed:
 *                                               the backward sum of :183-200 is re-associated onto va / vb / cond
 *                                            qk_c [T, N, E]   (query_exp[e]·key of that position)
 *   anc int32 [N, T]: for sequence n and position j < pos, the slot (sequence index) whose cache
 *        entry at j belongs to n's history (beam re-ordering without copying caches); position
 *        `pos` itself is always slot n.  Entries at positions j >= pos are not read: they may hold anything.
 *   row_valid int32 [N]: 0 → padded row (finished beam): the block contributes 0 (masked rows of
 *        utils/masking.py:37-47), caches are still written.
 *   y_in fp32 [N,d] (ldy_in) → y fp32 [N,d] (ldy):  y = y_in + sel·A' + (1-sel)·B'  (may alias).
 *   T <= 128, E in {4, 8, 16, 32}, d a multiple of 64; one launch (one 1024-thread block per sequence).
 *   A launch with *pos outside [0, T) changes nothing (the caches hold T positions; checked on the device).
 *   y columns [d, ldy) are left untouched; lin columns beyond 5d and y_in columns beyond d are not read; the caches are
 *   compact, written only at position *pos, and no entry is read that an earlier position did not write — they need no
 *   clearing (test_dynexp_step_leading_dimensions_and_caches): cache rows at positions > *pos, rows of slots outside the
 *   history and forward weights [j][slot][i > j] may hold NaN (tests/test_dynexp_hard_rows_gpu.py).
 */
int odic_dynexp_step(const float* lin, int64_t ldlin, const float* qexp, const float* bexp,
                     float* cond_c, float* key_c, float* va_c, float* vb_c, float* wfa_c,
                     float* wfb_c, float* qk_c, const int32_t* anc, const int32_t* row_valid,
                     const int32_t* pos, const float* y_in, int64_t ldy_in, float* y, int64_t ldy,
                     int32_t N, int32_t T, int32_t d, int32_t E, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-sequence (teacher-forced) decoder pass: every token is known up front, so all T positions of all N sequences
 * are processed at once — rows are sequence-major, row = n·T + t, and the linear layers are odic_gemm with M = N·T.
 * (The reference's evaluation loss, test.py:84-138: model(enc_x, dec_x = y[:, :-1]) → LabelSmoothingLoss.)  Nothing is
 * cached in global memory and the launch count does not depend on T.  csrc/decoder_seq.hip.
 * ------------------------------------------------------------------------------------------- */

/* y[n·T + t, :] = embed[tokens[n][t]]·scale + pos_table[t]   (layers.py:16-17, End_ExpansionNet_v2.py:118-121).
 *   tokens int64 [N, T] compact; embed fp32 [vocab, d]; pos_table fp32 [pos_rows, d]; T <= pos_rows (ODIC_EINVAL otherwise,
 *   checked on the host).  A token outside [0, vocab) embeds as the zero vector: nothing is read out of bounds.
 *   row_valid (optional, with dec_len int32 [N]): int32 [N·T] receives 1 where t < dec_len[n], else 0 — the row mask
 *   odic_cross_attn_step takes.  y columns [d, ldy) are left untouched; row_valid is compact.
 *   Any int64 is a legal token: an id outside the table (vocab, -1, INT64_MIN, 2^40) is compared before an address is
 *   formed and gives exactly pos_table[t] (embed row 0 is read in its place and multiplied by 0); dec_len[n] <= 0 marks no row, >= T every row; without row_valid nothing is
 *   written but y.  ldy < d or N·T > 2^31 - 1: ODIC_EINVAL; row_valid without dec_len: ODIC_ENULL; nothing is written. */
int odic_dec_embed_seq(const int64_t* tokens, const float* embed, const float* pos_table, const int32_t* dec_len,
                       int32_t* row_valid, float* y, int64_t ldy, int32_t N, int32_t T, int32_t d, int32_t vocab,
                       int32_t pos_rows, float scale, void* stream);

/* Dynamic expansion (layers.py:152-204) for all positions of every sequence in one launch.
 *   lin fp32 [N·T, >=5d] (ldlin): cond | key | class_a | class_b | selector pre-activation of LN1(y), the layout
 *        odic_dynexp_step reads; qexp, bexp fp32 [E, d]; dec_len int32 [N] (clamped to [0, T]).
 *   y_in fp32 [N·T, d] (ldy_in) → y fp32 [N·T, d] (ldy):  y = y_in + sel·A' + (1-sel)·B'  (may alias).
 *   Masking as the reference: causal in position, rows and columns at t >= dec_len[n] masked.  A padded row gets
 *   y = y_in (its weights are 0/(0+eps)), exactly what the step kernel gives with row_valid = 0.  The masks are loop
 *   bounds: lin rows at positions t >= dec_len[n] are not read and may hold NaN (y_in rows there are read: they are copied).
 *   z[(i,e), j] = (qexp[e]·key_j + cond_i·key_j)/sqrt(d) splits into an E x T and a T x T product per sequence; both,
 *   the normalisers of the forward and backward weights and 16 rows at a time of the re-associated backward sum
 *   (odic_dynexp_step above) stay in LDS; fp32 accumulation throughout.  One 1024-thread block per sequence.
 *   T <= 128, E in {4, 8, 16, 32}, d a multiple of 64, ldlin a multiple of 4, lin / qexp 16-byte aligned: ODIC_EINVAL
 *   before any launch otherwise.
 *   y columns [d, ldy) are left untouched; lin columns beyond 5d and y_in columns beyond d are not read. */
int odic_dynexp_seq(const float* lin, int64_t ldlin, const float* qexp, const float* bexp, const int32_t* dec_len,
                    const float* y_in, int64_t ldy_in, float* y, int64_t ldy, int32_t N, int32_t T, int32_t d,
                    int32_t E, float eps, void* stream);

/* The scoring tail (log_softmax + gather of test.py:119-131 / losses/loss.py:15-39), one pass per logits row, no
 * [R, V] log-prob tensor:   logits fp32 [R, V] (ldl); target int64 [R] or NULL.
 *   logp_target fp32 [R]  logits[r][target[r]] − logsumexp(logits[r])       (written only with target)
 *   sum_logp    fp32 [R]  Σ_v logits[r][v] − V·logsumexp  (the label-smoothing term; summed in fp64)
 *   argmax     int32 [R]  (ties → lower index, as odic_logsoftmax_topk);  max_logp fp32 [R] its log-probability
 *   status     int32 scalar, required with target: bit 0 is OR-ed in when some target lies outside [0, V); that row's
 *              logp_target is 0 and nothing is read out of bounds.  The caller clears it.
 * All outputs are compact; logits columns [V, ldl) are not read.
 * Log-probs are formed as (x − max) − log Σ exp(x − max), as torch forms them: the error does not grow with |logsumexp|
 * (odic_logsoftmax_topk's does).  A masked word (logit -inf) has log-prob exactly -inf, as a target too; a row with one
 * has sum_logp exactly -inf; argmax / max_logp ignore it.  A row without a finite logit, or with a NaN, is outside the
 * contract.  What such a row gets today (tests/token_stats_model.py, pinned by tests/test_token_stats_gpu.py):
 *   ties       the lowest index of the maximum, wherever in the block the tied words sit (an all-equal row: 0);
 *   status     only ever OR-ed (4 on entry and a flagged row: 5; no flagged row: unchanged); the flagged row's three
 *              other outputs are those of an unflagged row;
 *   +inf, or no finite word (all -inf): logp_target, sum_logp and max_logp are NaN (inf - inf, as torch.log_softmax),
 *              argmax is the lowest index of the maximum (all -inf: 0);
 *   a NaN      logp_target, sum_logp and max_logp are NaN; argmax is the arg-max of the other words when the NaN sits at
 *              an index >= 256, 0 when it sits at index 0, and otherwise that of the words the NaN's lane does not hide
 *              (it is NOT the NaN's index, which is what torch.argmax would give).
 *   R <= 0, V <= 0 or ldl < V: ODIC_EINVAL; a NULL logits / sum_logp / argmax / max_logp, or target without logp_target
 *   and status: ODIC_ENULL; nothing is written either way. */
int odic_token_stats(const float* logits, int64_t ldl, const int64_t* target, float* logp_target, float* sum_logp,
                     int32_t* argmax, float* max_logp, int32_t* status, int32_t R, int32_t V, void* stream);

/* Cross attention of one query row per sequence against per-IMAGE cached K/V (layers.py:266-295;
 * the reference re-projects K/V of the 144 encoder tokens every step for every beam copy).
 *   q fp32 [N, d] (ldq; already Wq-projected, bias included);
 *   kv fp32 [n_img, S, ldkv]: projected keys at column koff, values at column voff;
 *   enc_len int32 [n_img]; beams = N / n_img; row_valid as above (0 → all scores masked to -1e4,
 *   i.e. a uniform average over all S positions, exactly what masked_fill + softmax gives).
 *   out fp32 [N, d] (ldo) = softmax(q·kᵀ/sqrt(d/heads))·v, heads concatenated.  d/heads in {16,32,64}.
 *   ldq, ldkv and koff are multiples of 4 and q / kv 16-byte aligned (ODIC_EINVAL otherwise, before any launch).  Every
 *   out row is written, row_valid = 0 rows included; out columns [d, ldo) are left untouched; q / kv columns beyond their
 *   widths are not read (test_cross_attn_step_leading_dimensions). */
int odic_cross_attn_step(const float* q, int64_t ldq, const float* kv, int64_t ldkv, int32_t koff,
                         int32_t voff, const int32_t* enc_len, const int32_t* row_valid, float* out,
                         int64_t ldo, int32_t N, int32_t n_img, int32_t S, int32_t d, int32_t heads,
                         void* stream);

/* The cross-attention probabilities themselves — where the model looked for each word — instead of the attention output:
 * what odic_cross_attn_step computes in LDS, uses for P·V and discards.  q, kv, koff, enc_len, row_valid and the row →
 * image map (row n belongs to image n / (N / n_img)) are those of odic_cross_attn_step; with the [N·T] rows of the
 * whole-sequence pass, one launch covers every position of every caption.
 *   p_h[n, s] = softmax_s(q_h[n]·k_h[s]/sqrt(d/heads)), a score set to exactly -1e4 where s >= enc_len[img] or
 *   row_valid[n] == 0 (layers.py:247-250): a masked key of a valid row gets exactly 0, a row_valid = 0 row and every row
 *   of an image with enc_len = 0 get exactly 1/S everywhere.  fp32 throughout, base e.
 *   per_head = 0: out fp32 [N, S] (ldo)        = scale·Σ_h p_h[n, s]  (heads summed in the block, in head order)
 *   per_head = 1: out fp32 [N, heads·S] (ldo)  = scale·p_h[n, s] at column h·S + s
 *   accumulate = 1 adds that to what out holds, 0 overwrites: the mean over L layers and the heads is L calls with
 *   scale = 1/(L·heads) into one [N, S] buffer.  scale·x and out + x are separate roundings (no FMA), so an accumulated
 *   call adds exactly what an overwriting call would have stored.
 *   One thread writes each element, there are no atomics and the result does not depend on the grid.
 *   d/heads in {16,32,64}, S >= 1, N >= 1 a multiple of n_img, ldq, ldkv and koff multiples of 4, q / kv 16-byte aligned,
 *   ldo >= S (per_head: heads·S), and an S whose score and sum rows fit the block's 64 KB of LDS (S <= 8159 at d/heads = 64;
 *   the shipped decoder has S = 144): ODIC_EINVAL otherwise, before any launch.
 *   Every out row is written, row_valid = 0 rows included; out columns [S, ldo) (per_head: [heads·S, ldo)) are left
 *   untouched; q / kv columns beyond their widths are not read (test_cross_attn_probs_containment). */
int odic_cross_attn_probs(const float* q, int64_t ldq, const float* kv, int64_t ldkv, int32_t koff,
                          const int32_t* enc_len, const int32_t* row_valid, float* out, int64_t ldo,
                          int32_t N, int32_t n_img, int32_t S, int32_t d, int32_t heads,
                          int32_t per_head, int32_t accumulate, float scale, void* stream);

/* log_softmax over V + top-k (captioning_model.py:126-127,162-170).  logits fp32 [N, V] (ldl);
 * writes logp_out fp32 [N, V] (ldp) if non-NULL, top_val fp32 [N,k] / top_idx int32 [N,k] sorted
 * descending (ties: lower index first).  k <= 16.  logp_out columns [V, ldp) are left untouched, top_val / top_idx are compact,
 * logits columns [V, ldl) are not read (test_logsoftmax_topk_leading_dimensions).
 * Log-probs are formed as x − (max + log Σ exp(x − max)): one rounding of the log-sum-exp is shared by the whole row, so
 * the error is bounded by 6e-6 + 2^-23·(|logsumexp| + |log-prob|) and grows with the offset of the logits
 * (odic_token_stats uses the other form; tests/vocab_rows_refs.py derives both bounds).
 * A masked word (logit -inf) has log-prob exactly -inf and ranks behind every finite word; a row with fewer than k finite
 * words fills the remaining slots with masked words by ascending index, top_val -inf.  A row without a finite logit, or
 * with a NaN, is outside the contract (every entry point below says the same of its rows). */
int odic_logsoftmax_topk(const float* logits, int64_t ldl, float* logp_out, int64_t ldp,
                         float* top_val, int32_t* top_idx, int32_t N, int32_t V, int32_t k,
                         void* stream);

/* The `sample` variants of the search (captioning_model.py:128-131,166-168: exp(log_probs).multinomial(k,
 * replacement=False); :59-109 ancestral sampling with k = 1): k words drawn WITHOUT replacement from
 * softmax(logits[n]) on the device (Gumbel-top-k), top_idx int32 [N,k] in draw order, top_val fp32 [N,k] =
 * their log-probabilities; logp_out as in odic_logsoftmax_topk.  Noise = Philox4x32-10(seed; row, word/4,
 * *pos): `pos` (device int32 scalar, may be NULL = 0) separates the steps of a captured graph.  Padding as for
 * odic_logsoftmax_topk: logp_out columns [V, ldp) left untouched, top_val / top_idx compact
 * (test_logsoftmax_sample_leading_dimensions).  Log-probs in odic_logsoftmax_topk's form, with its bound.
 * A masked word (logit -inf) has probability 0 and is never drawn while a word of non-zero probability is left.  A row
 * with m < k finite words gives those m words in draw order, then the masked words with the lowest indices in ascending
 * order, each with top_val -inf: every top_idx lies in [0, V) and nothing outside the row is read.  Rows with at least k
 * finite words are not affected by that rule.  A row without a finite logit, or with a NaN, is outside the contract. */
int odic_logsoftmax_sample(const float* logits, int64_t ldl, float* logp_out, int64_t ldp, float* top_val,
                           int32_t* top_idx, int32_t N, int32_t V, int32_t k, uint64_t seed,
                           const int32_t* pos, void* stream);

/* odic_logsoftmax_sample that also reports the PERTURBED scores its draws were ranked by — what stochastic beam search
 * (odic_stochastic_beam_step below) ranks whole captions by.  An addition to ABI 26.
 *   top_pert fp32 [N, k], compact: top_pert[n][r] = (x[v_r] + Gumbel(v_r)) − logsumexp(x), v_r = top_idx[n][r]: the fp32 sum
 *   the draw order was decided on, minus the row's one shared log-sum-exp.  Non-increasing along r.  Within
 *   2e-6 + 2^-23·(|x| + |logsumexp| + |Gumbel|) of the exact value for the same noise bits.
 *   top_idx, top_val and logp_out are bit for bit odic_logsoftmax_sample's for the same seed and *pos (one kernel serves
 *   both; odic_logsoftmax_sample is the call with top_pert not stored).
 *   A slot filled by the short-row rule (a masked word, top_val -inf) has top_pert -inf.
 * Refusals (before any launch, nothing written), padding and containment are odic_logsoftmax_sample's: ODIC_ENULL for a
 * NULL logits, top_val, top_idx or top_pert; ODIC_EINVAL for N, V or k < 1, k > 16 or k > V.  All stores stay inside
 * top_val, top_idx, top_pert and columns [0, V) of logp_out; logits columns [V, ldl) are not read. */
int odic_logsoftmax_sample_scored(const float* logits, int64_t ldl, float* logp_out, int64_t ldp, float* top_val,
                                  int32_t* top_idx, float* top_pert, int32_t N, int32_t V, int32_t k, uint64_t seed,
                                  const int32_t* pos, void* stream);

/* Sampling controls: odic_logsoftmax_sample's draws from a temperature-scaled top-k / nucleus (top-p) subset of the row. */
typedef struct odic_sample_filter {
  float   inv_temperature; /* 1/temperature, rounded once to fp32 by the caller; finite, > 0 */
  int32_t top_k;           /* 0 = off, else keep the top_k best-ranked words */
  float   top_p;           /* in (0, 1]; 1 = off */
} odic_sample_filter;

/* odic_logsoftmax_sample with a filter; logits, logp_out, top_val, top_idx, seed and pos are its arguments.  One block
 * handles one row.
 *   Scaled logits: z[v] = x[v]·inv_temperature, one fp32 multiply; ranking, filtering and drawing happen on z.  Rank:
 *     larger z first, ties to the lower index (-0 = +0); a masked word (x = -inf) has zero mass and ranks last.
 *   Top-k set K: the first top_k words in rank order; all V words when top_k == 0 or top_k >= V.
 *   Nucleus: q = softmax(z) renormalised over K, c(v) = the mass of the words of K ranked strictly before v; v is in the
 *     nucleus iff c(v) < top_p — the smallest rank-prefix whose mass reaches top_p, never empty; equal values at the
 *     boundary are split by index.  top_p == 1 is OFF: every word of K is in the nucleus, masked ones and those whose
 *     mass underflows included (their c(v) is 1, or rounds to it).
 *   kept int32 [N] (may be NULL): m = the number of words in top-k ∩ nucleus, before the extension below.
 *   Draw set S: the first max(m, k) words in rank order — the filter never leaves fewer candidates than are drawn (a
 *     min_tokens_to_keep of k), so a beam search with k = beam_size keeps beam_size finite candidates whenever the row
 *     has that many finite words.
 *   Draws: the k words of S with the largest z[v] + Gumbel(v), in draw order; the noise is odic_logsoftmax_sample's,
 *     Philox counter (row, v/4, *pos, 0) under the same key.
 *   Reported values: top_val and logp_out are the MODEL'S OWN log-probs x[v] − logsumexp(x), unscaled and unfiltered, in
 *     odic_logsoftmax_sample's form, summation order and bound: a sampled caption's log-probs are its teacher-forced ones.
 *   Short rows: a row with fewer than k finite words follows odic_logsoftmax_sample's rule.
 *   Filter off (inv_temperature == 1, top_k == 0, top_p == 1): top_idx, top_val and logp_out are bit for bit those of
 *     odic_logsoftmax_sample for the same seed and *pos.
 *   Boundary band: with c(v) in exact arithmetic from the fp32 z, a word with c(v) < top_p·(1 − 1e-5) is kept, one with
 *     c(v) > top_p·(1 + 1e-5) is dropped, in between either (expf is good to about 2^-22 per term; the masses are summed in
 *     double, so the summation order adds nothing visible).
 *   ODIC_EINVAL before any launch, nothing written: inv_temperature not finite or <= 0; top_k < 0; top_p outside (0, 1] or
 *     NaN; k outside [1, 16]; V < k, V < 1 or V > 262144; N < 1; ldl < V, or ldp < V with logp_out given; f, logits,
 *     top_val or top_idx NULL.
 *   All stores stay inside top_val, top_idx, kept and columns [0, V) of logp_out; logits columns [V, ldl) are not read.
 *   A row without a finite logit, or with a NaN, is outside the contract. */
int odic_logsoftmax_sample_filtered(const float* logits, int64_t ldl, float* logp_out, int64_t ldp, float* top_val,
                                    int32_t* top_idx, int32_t* kept /* [N] or NULL */, int32_t N, int32_t V, int32_t k,
                                    const odic_sample_filter* f, uint64_t seed, const int32_t* pos, void* stream);

/* Ensemble step distribution (ensemble_captioning_model.py:66-83): `logits` is a HOST array of M (<= 8)
 * device pointers to fp32 [N, V] logits (row pitch ldl); out[n][v] = log(mean_m softmax(logits_m[n])[v]).  out columns
 * [V, ldo) are left untouched, logits columns [V, ldl) are not read.
 * The probabilities are averaged in fp32: out is exactly -inf where every member masks the word (logit -inf) AND where
 * every member's probability underflows (below about 2^-150, i.e. a word some 104 below each member's maximum); between
 * 2^-126 and that the result carries the absolute spacing of fp32 denormals.  A word masked by some members only is
 * finite.  Within 6e-6 + 2^-23·(max_m |x_m − max_m| + |out|) while the mean probability is a normal number.  A member
 * row without a finite logit, or with a NaN, is outside the contract. */
int odic_ensemble_logprobs(const float* const* logits, int32_t M, int64_t ldl, float* out, int64_t ldo,
                           int32_t N, int32_t V, void* stream);
/* k largest entries of every row (ties → lower index), values taken as they are (rows already hold
 * log-probabilities, e.g. the output of odic_ensemble_logprobs): top_val fp32 [N,k], top_idx int32 [N,k], both compact;
 * logp columns [V, ldl) are not read (test_ensemble_logprobs_and_topk_rows_leading_dimensions, also for the one above).
 * Values are copied, never recomputed.  -inf entries rank behind every finite one; with fewer than k finite entries the
 * remaining slots hold -inf entries by ascending index.  NaN entries are outside the contract. */
int odic_topk_rows(const float* logp, int64_t ldl, float* top_val, int32_t* top_idx, int32_t N, int32_t V,
                   int32_t k, void* stream);

/* Constrained word selection, the sibling of odic_topk_rows for a search that may not choose every word: the k best
 * ADMISSIBLE entries of every row (value descending, ties → lower index), values taken as they are — the rows already hold
 * log-probabilities (logp_out of odic_logsoftmax_topk, or the output of odic_ensemble_logprobs), so the log-probs of a
 * constrained caption are bit for bit what the unconstrained kernels compute.  top_val fp32 [N,k], top_idx int32 [N,k],
 * both compact; logp columns [V, ldl) are not read.  It runs between the top-k launch of a step and odic_beam_step /
 * odic_group_beam_step, overwriting the candidates the former wrote.  Every pointer of the struct is a device pointer
 * and the step is read on the device, so a step stays capturable.
 *   Let p = tokens[n][0 .. *pos] (slot 0 = SOS; *pos is clamped to [0, T-1]).  For a growing row, word w is inadmissible if
 *     - w is in `banned`, or
 *     - w == eos_idx and *pos < min_words (the caption would end with *pos words), or
 *     - no_repeat_ngram = g > 0 and some j in [0, *pos - g + 1] has p[j .. j+g-2] == p[*pos-g+2 .. *pos] and p[j+g-1] == w:
 *       appending w would write a g-gram the prefix already holds (g = 1: every word of the prefix, SOS included; while
 *       the prefix is shorter than g - 1 words plus one the range of j is empty).
 *   Banned ids and prefix words outside [0, V) are ignored; nothing is stored out of range.  A finished row
 *   (row_valid[n] == 0) gets exactly what odic_topk_rows gives it: the step kernels use only its rank-0 slot.
 *   k admissible words always exist: a row loses at most n_banned + 1 + (T - 1) words, and a call with
 *   n_banned + T + k > V is refused.  With no active constraint the output is odic_topk_rows', bit for bit, -inf entries
 *   included: they rank behind every finite admissible word and fill the last slots by ascending index.
 *   ODIC_EINVAL, before any launch and with nothing written: n_banned + T + k > V, k outside [1, 16], no_repeat_ngram
 *   outside [0, T], min_words < 0, T outside odic_beam_step's [2, 128], n_banned outside [0, 1024], V above 262144 (the
 *   inadmissible set is a bitmap in 32 KB of LDS), N or V < 1, ldl < V, or a required pointer NULL (logp, c, top_val,
 *   top_idx, tokens, pos; banned with n_banned > 0) — one refusal code for this entry point.
 *   All stores stay inside top_val / top_idx (tests/test_search_constraints_gpu.py runs every operand in a guarded buffer). */
typedef struct odic_search_constraints {
  const int64_t* tokens;      /* [N, T] prefixes, row n = tokens + n*T (the beam state's `tokens`, viewed flat) */
  const int32_t* pos;         /* device scalar: the step; row n's prefix is tokens[n][0 .. *pos], slot 0 = SOS */
  const int32_t* row_valid;   /* [N] or NULL; a row with row_valid == 0 (finished beam) is selected UNCONSTRAINED */
  const int32_t* banned;      /* [n_banned] word ids, or NULL with n_banned == 0 */
  int32_t n_banned;
  int32_t no_repeat_ngram;    /* 0 = off, else n >= 1 */
  int32_t min_words;          /* eos is inadmissible while *pos < min_words (the caption would hold *pos words) */
  int64_t eos_idx;
  int32_t T;
} odic_search_constraints;
int odic_topk_rows_constrained(const float* logp, int64_t ldl, const odic_search_constraints* c,
                               float* top_val, int32_t* top_idx, int32_t N, int32_t V, int32_t k, void* stream);

/* The candidates of a CONTRASTIVE search step (the emitter–suppressor beam search of Vedantam et al., "Context-aware
 * captions from context-agnostic supervision", CVPR 2017, with the plausibility cut of contrastive decoding, Li et al.
 * 2022): a word is ranked by its log-prob under the target image minus a weighted log-prob under up to
 * seven distractor images, among the words the target itself finds plausible.  An addition to ABI 26.  One block per row. */
typedef struct odic_contrast_args {
  float   weight;     /* w >= 0, finite: how strongly the suppressor counts (Vedantam's 1 − λ); 0 = off */
  float   log_alpha;  /* <= 0 or -inf: a word is plausible iff x_t[v] − max(x_t) >= log_alpha (one fp32 subtract); -inf = off */
  float   floor;      /* finite, <= 0: the suppressor log-prob is clamped from below to this */
  int32_t min_keep;   /* >= k: the cut never leaves fewer than this many candidates */
} odic_contrast_args;
/*   logits: a HOST array of M = 1 + D (<= 8) device pointers to fp32 [N, V] rows of one pitch ldl, [0] the target's;
 *   count int32 [N] on the device: row n uses distractors 1 .. c, c = count[n] clamped to [0, D] (NULL only with M == 1).
 *   For row n:
 *   1. Log-probs lp_t, lp_1 .. lp_c as odic_logsoftmax_topk forms them, x − (max + log Σ exp(x − max)), in its summation
 *      order, with its bound.
 *   2. Suppressor: c == 1: s[v] = lp_1[v] exactly.  c > 1: s[v] = (m + logf(Σ_d expf(lp_d[v] − m))) − logf(c), m = max_d
 *      lp_d[v], the sum in ascending d: the log of the mean probability, formed in the log domain, so it does not
 *      underflow where odic_ensemble_logprobs does.  s'[v] = max(s[v], floor); a word every active distractor masks
 *      (-inf) has s' = floor.
 *   3. Score: out[v] = lp_t[v] − w·s'[v], a rounded product and a rounded difference (no FMA).  With c == 0 or w == 0,
 *      out[v] = lp_t[v] and no distractor row is read.  A word the target masks has out = -inf.  Scores may be POSITIVE.
 *   4. Plausibility: the words are ranked by x_t (larger first, ties to the lower index, -0 = +0); m = the number of
 *      plausible words; the admissible words are the first max(m, min_keep) in that order (the rule by which
 *      odic_logsoftmax_sample_filtered never leaves fewer candidates than are drawn); every other word has out = -inf.
 *      kept[n] = m (kept may be NULL).  log_alpha == -inf: every word is admissible, m = V.
 *   5. top_val / top_idx [N, k], compact: the k best out values, ties to the lower index; -inf entries come last by
 *      ascending index (odic_topk_rows' short-row rule).  top_val[n][r] is out[top_idx[n][r]] bit for bit.  score_out
 *      fp32 [N, V] (lds), when given, takes the whole row: what odic_topk_rows_constrained re-selects from.
 *   6. Off: with w == 0 or count[n] == 0, and log_alpha == -inf, top_val, top_idx and score_out are bit for bit
 *      odic_logsoftmax_topk's top_val, top_idx and logp_out.  (A row with w == 0 or count[n] == 0 is ranked by x_t under
 *      any log_alpha, as that kernel ranks: where two different logits round to one log-prob, the larger logit comes
 *      first, not the lower index.)
 *   ODIC_EINVAL / ODIC_ENULL before any launch, nothing written: M outside [1, 8]; k outside [1, 16], k > V, V > 262144,
 *     N < 1; ldl < V, or lds < V with score_out given; min_keep < k or > V; weight negative or not finite; log_alpha > 0 or
 *     NaN; floor not finite or > 0; logits, one of its M pointers, a, top_val or top_idx NULL; count NULL with M > 1.
 *   All stores stay inside top_val, top_idx, kept and columns [0, V) of score_out; logits columns [V, ldl) and the
 *   distractor rows beyond count[n] are never read (tests/test_contrast_rows_gpu.py runs every operand in a guarded
 *   buffer, the unused distractor rows filled with NaN).  A target row, or an active distractor row, without a finite
 *   logit or with a NaN is outside the contract.  Rows above 10240 words recompute a word's score in every one of the k
 *   selection rounds: exact, slower. */
int odic_contrast_topk(const float* const* logits, int32_t M, int64_t ldl, const int32_t* count,
                       const odic_contrast_args* a, float* score_out, int64_t lds, float* top_val, int32_t* top_idx,
                       int32_t* kept /* [N] or NULL */, int32_t N, int32_t V, int32_t k, void* stream);

/* Beam bookkeeping of one search step on device (captioning_model.py:172-223; the call with
 * *pos == 0 is the seeding of :126-140).  All arrays are device resident.
 *   cand_val/cand_idx [n_img*beams, beams]: per-sequence top-k log-probs / words
 *   tokens int64 [n_img, beams, T] prefixes (tokens[:, :, 0] = SOS before the first call),
 *   logprobs fp32 [n_img, beams, T] per-token log-probs (slot 0 = 0), anc int32 [N, T],
 *   cumul fp32 [N], n_elem int32 [N] (length incl. SOS/EOS), has_eos int32 [N],
 *   row_valid int32 [N] (output: 1 while the beam was still growing), next_tok int64 [N] (output:
 *   token to feed at the next step), pos int32 scalar (incremented at the end),
 *   done int32 scalar (set to 1 when every beam has stopped growing, :222).
 * All of these are compact arrays without leading dimensions.  The search-level test
 * test_pipeline_search_is_independent_of_the_previous_search pins that a search reads nothing a previous search left in them;
 * tests/test_group_beam_gpu.py runs odic_group_beam_step (which shares the update
 * half of odic_beam_step) with every array inside a guarded buffer.
 */
typedef struct odic_beam_state {
  int64_t* tokens; float* logprobs; int32_t* anc;
  float* cumul; int32_t* n_elem; int32_t* has_eos; int32_t* row_valid; int64_t* next_tok;
  int32_t* pos; int32_t* done;
  int32_t* ctr;      /* int32 scalar, zero before the first call: inter-block arrival counter */
} odic_beam_state;
/* Optional tail of the launch that chooses the next words: the decoder input of the next position,
 *   y[n] = embed[word_n]·scale + pos_table[pos + 1]   (EmbeddingLayer, layers.py:118-121 — what odic_dec_embed does in
 * a launch of its own), written while pos + 1 <= T - 2 (the last prefix position is never fed back);
 * embed fp32 [V, d], pos_table fp32 [pos_rows, d], y fp32 [n_img·beams, d] (ldy); nothing is written for a position
 * pos + 1 >= pos_rows (device-side bound, as odic_dec_embed). */
typedef struct odic_embed_args {
  const float* embed; const float* pos_table; float* y; int64_t ldy; int32_t d; float scale; int32_t pos_rows;
} odic_embed_args;
/*   Limits: beams <= 16, 2 <= T <= 128 (per-token log-probs are staged in LDS), n_img <= 32767 (the
 *   arrival counter packs {arrivals, still-growing images} into one int32): ODIC_EINVAL otherwise.
 *   A call with *pos == T - 1 (the prefix is full) changes nothing.  emb: NULL or the embedding tail above.
 *   Dead rows (one convention for the four step entry points).  At *pos >= 1 a total of -inf is never ranked: a row with
 *   cumul = -inf offers nothing, nor does a candidate of value -inf (the short-row rule of the top-k kernels); a finished
 *   row offers its rank-0 candidate at 0 and the others at -999.  The `beams` largest totals above -inf are taken, the
 *   lowest flat index row·beams + rank winning a tie.  With fewer than `beams` of them, every remaining slot becomes an
 *   EMPTY row: parent = the slot's own row, word = eos_idx (embedded like any other word: the caller keeps it inside the
 *   table), stored log-prob -inf — after the update it has cumul = -inf and has_eos = 1, offers nothing again, counts as
 *   finished for *done from the next step on, and odic_beam_finalize scores it -inf.  Every index the kernel forms from a
 *   selection lies inside the image's rows and candidates, whatever the candidate values are
 *   (tests/test_beam_dead_rows_gpu.py).  The seeding call (*pos == 0) takes the candidates of row 0 as they come.  Rows
 *   with a NaN stay outside the contract (a NaN total is never ranked either). */
int odic_beam_step(const float* cand_val, const int32_t* cand_idx, const odic_beam_state* st,
                   const odic_embed_args* emb, int32_t n_img, int32_t beams, int32_t T, int64_t eos_idx,
                   void* stream);

/* The step of diverse (group) beam search (Vijayakumar et al., "Diverse Beam Search"), the sibling of odic_beam_step
 * on the same state: the R = groups·group_beams rows of an image are `groups` groups of `group_beams` beams, rows
 * g·group_beams .. (g+1)·group_beams - 1 being group g, and a beam's parent is always a row of its own group.
 *   cand_val / cand_idx [n_img·R, ncand], compact, as odic_logsoftmax_topk writes them with k = R (value descending, then
 *   word ascending); ncand must equal R.
 * Within one step the groups choose one after the other.  count[w] = the number of beams of groups 0..g-1 that
 * appended word w at this step and had not finished before it.  A growing beam j of group g offers word w at
 *   v = logp_j(w) - penalty·count[w],   total = cumul_j + v
 * (three separately rounded fp32 operations); a finished beam offers its rank-0 candidate at 0 and the others at -999,
 * never penalised, as in odic_beam_step.  The group keeps its group_beams best candidates: total descending, then beam
 * in group ascending, then word ascending — among the -999 fillers of one finished beam, rank ascending (at groups = 1 the
 * rule of odic_beam_step; the call then leaves the state bitwise as odic_beam_step does, EMPTY rows included, at every
 * *pos >= 1, and at *pos == 0 while row 0 holds `beams` candidates above -inf).  Dead rows follow odic_beam_step's
 * convention, group by group: a total of -inf is never ranked, and a slot for which the group has no total above -inf left
 * becomes an EMPTY row (parent = the slot's own row, word = eos_idx, stored log-prob -inf) that no later group counts in
 * count[w] — a group never holds one live caption twice.  At *pos == 0 group g draws from its own first row (all rows hold the same
 * distribution) against the seeds of the groups before it.  The penalty only steers the choice: logprobs[.., pos+1] is
 * the word's own log-prob and cumul the re-summed unpenalised prefix, so odic_beam_finalize scores the captions by the
 * model alone.  R candidates per row suffice: the penalised top-group_beams of a row lies inside its unpenalised
 * top-(group_beams + P), P <= g·group_beams <= R - group_beams being the number of penalised words.
 * Everything else (permutation of prefixes / log-probs / ancestors, embedding tail, n_elem, has_eos, row_valid,
 * next_tok, *pos, *done, the arrival counter) is odic_beam_step's, with its limits on T and n_img.
 *   ODIC_EINVAL: groups < 1, group_beams < 1, R > 16, ncand != R, penalty negative or not finite, T / n_img outside
 *   odic_beam_step's limits.  A refused call writes nothing.  All stores stay inside the compact state arrays and
 *   columns [0, d) of the R·n_img rows of emb->y (tests/test_group_beam_gpu.py). */
int odic_group_beam_step(const float* cand_val, const int32_t* cand_idx, int32_t ncand,
                         const odic_beam_state* st, const odic_embed_args* emb,
                         int32_t n_img, int32_t groups, int32_t group_beams, int32_t T,
                         int64_t eos_idx, float penalty, void* stream);

/* The step of a beam search whose captions must CONTAIN given words (Anderson et al., "Guided Open Vocabulary Image
 * Captioning with Constrained Beam Search"), the sibling of odic_beam_step on the same state.  An addition
 * to ABI 26.
 *   required int64 [n_img, n_required], device resident: the word ids image b must mention, -1 in unused slots (an id
 *   outside [0, V) counts as -1; the ids of an image are distinct: the caller checks).  C = n_required <= 4.
 *   The R = 2^C·bank_beams rows of an image are 2^C banks of bank_beams rows, bank m (a bit mask over the C slots) being
 *   rows m·bank_beams .. (m+1)·bank_beams - 1.  A row lives in bank m when its caption holds exactly the required words
 *   whose bits are set in m; the accepting bank of an image is the mask of its used slots.
 *   cand_val / cand_idx [n_img·R, ncand] as for odic_group_beam_step (ncand must equal R); logp fp32 [n_img·R, V] (ldl):
 *   the log-prob rows the candidates were taken from (logp_out of odic_logsoftmax_topk); columns [V, ldl) are not read.
 * At *pos = t the live rows are those with cumul > -inf.  Target bank m keeps the bank_beams best of
 *   stay:  from every live row j of bank m — a finished row (has_eos) its rank-0 candidate at 0 and nothing else; a
 *          growing row each of its ncand candidates whose word is neither a required word of the image whose bit is
 *          clear in m, nor EOS unless m is the accepting bank;
 *   enter: for every slot c set in m with required[b][c] >= 0 and every live, growing row j of bank m ^ (1 << c): the
 *          word required[b][c] at v = logp[row j][required[b][c]] (it need not be among the row's candidates);
 * total = cumul_j + v (one rounded fp32 addition); at t = 0 only row 0 of the image offers anything, and total = v.
 * Order: total descending, then source row (within the image) ascending, then word ascending.  A (row, word) pair leads to
 * exactly one bank.  A bank with fewer than bank_beams finite totals fills its remaining slots as EMPTY rows: parent =
 * the slot's own row (row 0 at t = 0), word = EOS, stored log-prob -inf — after the update such a row has cumul = -inf and
 * has_eos = 1, never offers anything again, and odic_beam_finalize scores it -inf.  Banks that carry the bit of an unused
 * slot stay empty.  A caption cannot take EOS before it holds every required word.
 * Everything after the choice (permutation of prefixes / log-probs / ancestors, embedding tail, n_elem, has_eos,
 * row_valid, next_tok, *pos, *done, the arrival counter) is odic_beam_step's: logprobs[.., pos+1] is the word's own
 * log-prob and cumul the re-summed prefix.  With n_required = 0 (logp and required may be NULL) the call leaves the state
 * bitwise as odic_beam_step with beams = bank_beams does, as long as every image has bank_beams finite totals (where
 * odic_beam_step would take a finished row's -999 fillers, this step writes empty rows).
 * A row loses at most C + 1 of its R candidates (the unmet required words and EOS) and must still offer bank_beams.
 *   ODIC_EINVAL, before any launch and with nothing written: n_required outside [0, 4], bank_beams < 1, R > 16,
 *   ncand != R, R < bank_beams + n_required + 1 with n_required > 0 (only C = 1 with one beam), ldl < V, V < 1, eos_idx
 *   outside [0, V) (it is the word of an empty row), logp or required NULL with n_required > 0, T / n_img outside
 *   odic_beam_step's limits.  All stores stay inside the compact state arrays and columns [0, d) of the R·n_img rows of
 *   emb->y (tests/test_require_beam_step_gpu.py). */
int odic_require_beam_step(const float* cand_val, const int32_t* cand_idx, int32_t ncand,
                           const float* logp, int64_t ldl, const int64_t* required, int32_t n_required,
                           const odic_beam_state* st, const odic_embed_args* emb,
                           int32_t n_img, int32_t bank_beams, int32_t T, int64_t eos_idx, int32_t V, void* stream);

/* The step of STOCHASTIC beam search (Kool, van Hoof & Welling, "Stochastic Beams and Where to Find Them", ICML 2019;
 * DESIGN.md §4.21), the sibling of odic_beam_step on the same state: after the last step the `beams` rows of an image are
 * `beams` DISTINCT captions sampled from the model without replacement, row 0 an exact sample.  An addition to ABI 26; the
 * state struct is unchanged, the rows' perturbed scores travel in an argument of their own.
 *   cand_val / cand_idx / cand_pert [n_img·beams, beams], compact: as odic_logsoftmax_sample_scored writes them with
 *   k = beams (cand_pert[.][0] the row's largest).  gscore fp32 [n_img·beams], compact, in and out: the perturbed score
 *   G of every row; it need not be initialised before the call with *pos == 0.
 * Let row j of an image have phi_j = cumul[j] and G_j = gscore[j].
 *   Offers.  A live row is one with cumul > -inf.  A live growing row offers each of its candidates r with
 *   cand_val > -inf.  A live finished row (has_eos) offers exactly one candidate, itself: the word of its rank-0 slot at
 *   log-prob 0, as odic_beam_step keeps a finished row, with G~ = G_j.  At *pos == 0 only row 0 offers, with phi = G = 0.
 *   Perturbed score of candidate r of a growing row, G~_r = -log(e^-G_j − e^-Z + e^-g_r) (Z the row's largest g), in fp32 as
 *     d = cand_pert[r] − cand_pert[0]                         (<= 0; phi_j cancels)
 *     d == 0:  G~_r = G_j exactly                             (rank 0, and any exact tie with it)
 *     else     u = (G_j − phi_j) − cand_pert[r];  v = u + log1mexp(d);  G~_r = G_j − max(v, 0) − log1p(exp(−|v|))
 *     with log1mexp(d) = d > −ln 2 ? log(−expm1(d)) : log1p(−exp(d)): neither e^-G nor e^-Z is ever formed.
 *   Selection.  The `beams` best offers of the image: G~ descending, then source row ascending, then rank ascending.  New
 *   row i takes the parent, the word and the word's OWN log-prob cand_val (cumul is re-summed as in odic_beam_step), and
 *   gscore[i] = G~.  Rows leave every step sorted by G~; every child's G~ <= its parent's G, the best child of a row
 *   inherits it bit for bit, and the live rows of an image hold different prefixes.  With fewer offers than beams the
 *   remaining slots become EMPTY rows by odic_require_beam_step's convention (parent = the slot itself, row 0 at *pos == 0;
 *   word = EOS; stored log-prob -inf, so cumul = -inf and has_eos = 1) with gscore -inf.
 * Everything after the choice (permutation of prefixes / log-probs / ancestors, embedding tail, n_elem, has_eos,
 * row_valid, next_tok, *pos, *done, the arrival counter, the no-op at *pos == T − 1) is odic_beam_step's, with its limits.
 * The inclusion probability of a caption of log-prob phi in the sample, given the threshold kappa = the G of the first
 * caption NOT returned, is 1 − exp(−exp(phi − kappa)) (Kool et al., eq. 15 ff.); this library reports G and leaves that to
 * the caller.
 *   ODIC_EINVAL — one refusal code for this entry point — before any launch and with nothing written: beams outside
 *   [1, 16], T outside [2, 128], n_img outside [1, 32767], eos_idx < 0 (it is the word of an empty row, embedded like any
 *   other: the caller keeps it inside the embedding table), cand_val, cand_idx, cand_pert, gscore, st or one of its arrays
 *   NULL, an emb with a NULL table or d / pos_rows < 1.  All stores stay inside the compact state arrays, gscore and
 *   columns [0, d) of the beams·n_img rows of emb->y (tests/test_stochastic_beam_step_gpu.py). */
int odic_stochastic_beam_step(const float* cand_val, const int32_t* cand_idx, const float* cand_pert, float* gscore,
                              const odic_beam_state* st, const odic_embed_args* emb, int32_t n_img, int32_t beams,
                              int32_t T, int64_t eos_idx, void* stream);

/* POOLED beam search (csrc/pool_beam.hip), on the same beam state: a hypothesis that takes EOS leaves the
 * beam for a per-image pool of at most P = beams finished hypotheses scored by sum / len^alpha, the `beams` rows stay live,
 * and an image closes once its pool cannot be improved.  Additions to ABI 26.
 *   The pool, all device resident and compact: tokens int64 / logprobs fp32 [n_img, P, T]; len int32, sum fp32, score fp32,
 *   serial int32 [n_img, P]; count int32 [n_img] (entries [0, count) of an image are hypotheses); closed int32 [n_img]
 *   (0 = open; bit 0: closed by a step; bit 1: finalized).  odic_pool_reset zeroes count and closed — nothing else of the
 *   pool is read before it is written.  scale fp32 [T + 1]: scale[L] = (fp32)((double)L ** alpha), built by the host, so
 *   that the device never calls powf and score = __fdiv_rn(sum, scale[len]) can be reproduced bit for bit; len counts SOS
 *   and EOS like n_elem (alpha = 1: odic_beam_finalize's score of the same row).
 *   cand_val / cand_idx [n_img·beams, beams]: every row's `beams` best admissible words OTHER than eos_idx (the caller
 *   selects them with EOS inadmissible: odic_topk_rows_constrained with min_words >= T); logp fp32 [n_img·beams, V] (ldl):
 *   the log-prob rows they came from — the step reads logp[row][eos_idx] and nothing else of them.
 * One step at *pos = t for an open image:
 *   1. Every live row j (cumul > -inf; t = 0: row 0 alone, its cumul taken as 0) offers candidate c < beams at cand_val as
 *      slot c, and EOS at logp[j][eos_idx] as slot `beams` — the latter only when t >= min_words.
 *   2. The candidates are ranked by total = cumul_j + value (one rounded addition; t = 0: the value), descending, a tie
 *      to the lower key j·(beams + 1) + slot; a total of -inf or NaN is never ranked.
 *   3. The ranking is walked from the best, 2·beams extractions at most: a word becomes the next live row until `beams`
 *      are chosen; an EOS met while fewer than `beams` candidates were extracted before it is offered to the pool, a later
 *      one dropped.  A slot for which nothing is left becomes the EMPTY row of odic_beam_step (parent = the slot itself,
 *      row 0 at t = 0; word = eos_idx; stored log-prob -inf).
 *   4. A pool offer: sum = the parent's per-token log-probs re-summed in position order, + value (odic_beam_step's order
 *      for cumul); len = n_elem(parent) + 1; score as above (len clamped to [0, T] for the table).  While count < P it is
 *      appended; else it replaces the worst entry (lowest score, a tie to the highest serial) if its score is STRICTLY
 *      greater.  An accepted hypothesis takes serial = 1 + the largest serial in the pool (0 in an empty pool), the
 *      parent's tokens / log-probs [0..t] as they stand before this step permutes the rows, eos_idx / value at t + 1 and
 *      zeros behind.  The offers of one step are applied one after the other in walk order.
 *   5. The image closes if count == P and (early_stopping != 0 or worst score >= __fdiv_rn(best new cumul, scale[T])), best
 *      new cumul the largest cumul of the rows chosen in 3 (-inf when there is none).  Its rows are written as by any step
 *      but with row_valid = 0, they do not count as growing for *done, and closed = 1.
 *   Everything else (permutation, embedding tail, n_elem, has_eos, next_tok, *pos, *done, the counter, the no-op at
 *   *pos == T - 1) is odic_beam_step's.  For a closed image a step changes nothing (its block only arrives at the counter).
 * odic_pool_beam_finalize, once after the last step, one block per image: an image still open (closed == 0) offers its rows
 *   with cumul > -inf and has_eos == 0 in row order, sum = cumul, len = n_elem, tokens / log-probs [0, len) and zeros behind
 *   (no EOS), by the rule of 4.  Then order int32 [n_img, P]: the pool slots by score descending, a tie to the lower serial,
 *   -1 behind the count; score fp32 [n_img, P]: the scores in that order, -inf behind the count; closed |= 2.
 *   ODIC_EINVAL — one refusal code — before any launch and with nothing written: beams outside [1, 15] (beams·(beams + 1)
 *   candidates are ranked 256 at a time), T / n_img outside odic_beam_step's limits, V < 1, ldl < V, eos_idx outside
 *   [0, V), min_words < 0, a NULL pointer (cand_val, cand_idx, logp, order, score, pool or one of its arrays, st or one of
 *   its arrays), an emb with a NULL table.  All stores stay inside the compact state and pool arrays, order, score and
 *   columns [0, d) of emb->y (the pool and state arrays run in guarded buffers in
 *   tests/test_pool_beam_kernels_gpu.py; the embedding tail is odic_beam_step's). */
typedef struct odic_pool_args {
  int64_t* tokens; float* logprobs;
  int32_t* len; float* sum; float* score; int32_t* serial;
  int32_t* count; int32_t* closed;
  const float* scale;
  int32_t min_words;        /* EOS is offered only at *pos >= min_words (the caption would hold *pos words) */
  int32_t early_stopping;   /* != 0: an image closes as soon as its pool is full */
} odic_pool_args;
int odic_pool_reset(const odic_pool_args* pool, int32_t n_img, void* stream);
int odic_pool_beam_step(const float* cand_val, const int32_t* cand_idx, const float* logp, int64_t ldl,
                        const odic_pool_args* pool, const odic_beam_state* st, const odic_embed_args* emb,
                        int32_t n_img, int32_t beams, int32_t T, int64_t eos_idx, int32_t V, void* stream);
int odic_pool_beam_finalize(const odic_pool_args* pool, const odic_beam_state* st, int32_t* order, float* score,
                            int32_t n_img, int32_t beams, int32_t T, void* stream);

/* Initial state of a search (captioning_model.py:117-125): tokens[:, :, 0] = sos, logprobs[:, :, 0] = 0,
 * next_tok = sos, row_valid = 1, *pos = *done = *ctr = 0; with emb, also the input of position 0 (the embedded
 * start token).  One launch instead of six fills on the latency-bound decode stream. */
int odic_beam_reset(const odic_beam_state* st, const odic_embed_args* emb, int32_t n_img, int32_t beams, int32_t T,
                    int64_t sos_idx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Starting a search from a given prefix (csrc/decoder_prefill.hip): the whole-sequence pass over the
 * prefix fills the step caches, and the reset below puts the beam state at position P.  Both are additions to ABI 26.
 * ------------------------------------------------------------------------------------------- */

/* The per-position caches of odic_dynexp_step for positions 0..P-1 of n_seq known sequences, from the `lin` rows of the
 * whole-sequence pass — what P calls of odic_dynexp_step on those rows would have cached, without computing any y.
 *   lin fp32 [n_seq·P, >=5d] (ldlin), sequence-major as odic_dynexp_seq reads it (row = i·P + t); qexp fp32 [E, d].
 *   There is no dec_len: every sequence has P valid positions (a shorter prefix is a smaller P), all n_seq·P rows are read
 *   and nothing behind the last of them is.
 *   Sequence i writes cache slot s = i·rows_per_image of caches laid out for N_cache sequences and T_cache positions
 *   (cond_c, key_c, va_c, vb_c [T_cache, N_cache, d]; qk_c [T_cache, N_cache, E]; wfa_c, wfb_c [T_cache, N_cache, T_cache, E]):
 *     cond/key/va/vb[t][s] = lin columns 0..4d of row i·P + t;   qk[t][s][e] = qexp[e]·key_t;
 *     wfa[t][s][j][e] = relu(z)/(Σ_{j<=t} relu(z) + eps),  z = (qexp[e]·key_j + cond_t·key_j)/sqrt(d),  j <= t  (wfb: -z)
 *   with the step kernel's expressions and summation order for the normaliser; the dot products are the 4 x 4 register
 *   tiles of odic_dynexp_seq.  Entries with j > t, positions >= P and every other slot are not written
 *   (tests/test_prefix_kernels_gpu.py runs every cache in a guarded, poisoned buffer).
 *   1 <= P < T_cache <= 128, E in {4, 8, 16, 32}, d a multiple of 64, (n_seq-1)·rows_per_image < N_cache, ldlin a multiple
 *   of 4 and >= 5d, lin / qexp 16-byte aligned: ODIC_EINVAL before any launch otherwise, with nothing written.
 *   One 1024-thread block per sequence; (E + P)·P' + 2·P·E words of LDS, P' = P rounded up to 1 mod 4. */
int odic_dynexp_fill_caches(const float* lin, int64_t ldlin, const float* qexp, float* cond_c, float* key_c, float* va_c,
                            float* vb_c, float* wfa_c, float* wfb_c, float* qk_c, int32_t n_seq, int32_t P,
                            int32_t rows_per_image, int32_t N_cache, int32_t T_cache, int32_t d, int32_t E, float eps,
                            void* stream);

/* The beam state of a search that starts behind a given prefix of P words (the sibling of odic_beam_reset):
 *   prefix int64 [n_img, P] (ids inside the embedding table: the caller checks), prefix_logp fp32 [n_img, P] (the model's
 *   log-prob of every prefix word given the ones before it).  For every row n = b·beams + r:
 *     tokens[n][0] = sos, tokens[n][1..P] = prefix[b];  logprobs[n][0] = 0, logprobs[n][1..P] = prefix_logp[b];
 *     anc[n][j] = b·beams for j < P (the slot odic_dynexp_fill_caches writes with rows_per_image = beams);
 *     n_elem = P + 1, has_eos = 0, row_valid = 1, next_tok = prefix[b][P-1];
 *     cumul = Σ_j logprobs[n][j] in position order when r % group_beams == 0, else -INFINITY;
 *   *pos = P, *done = 0, *ctr = 0; with emb, y[n] = embed[prefix[b][P-1]]·scale + pos_table[P].
 *   odic_beam_step (group_beams = beams) and odic_group_beam_step never rank a total of -inf, so the step at position P
 *   chooses among the candidates of one row per group: the seeding of *pos == 0, from position P.
 *   1 <= P <= T - 2, beams % group_beams == 0, emb->pos_rows > P, and odic_beam_step's limits on beams, T and n_img:
 *   ODIC_EINVAL otherwise, before any launch.  All stores stay inside the compact state arrays and columns [0, d) of y. */
int odic_beam_reset_prefix(const odic_beam_state* st, const odic_embed_args* emb, const int64_t* prefix,
                           const float* prefix_logp, int32_t n_img, int32_t beams, int32_t group_beams, int32_t T,
                           int32_t P, int64_t sos_idx, void* stream);

/* Final selection (captioning_model.py:225-241): score = cumul / n_elem, descending order per
 * image → order int32 [n_img, beams], score fp32 [n_img, beams].
 * order[b] is always a permutation of 0 .. beams-1: score descending, a tie to the lower row, and -inf against -inf is a
 * tie — dead and EMPTY rows (score -inf) come last, in row order.  odic_beam_finalize_best emits row order[b][0], which
 * is row 0 when every row of the image is dead. */
int odic_beam_finalize(const odic_beam_state* st, int32_t* order, float* score, int32_t n_img,
                       int32_t beams, void* stream);

/* odic_beam_finalize + the best caption of every image in the fixed-shape form the multi-GPU gather
 * ships (captioning_model.py:225-241 with how_many_outputs = 1; test.py:216-224 takes output_words[i][0]):
 * out_tok int32 [n_img, T] = tokens of the best beam, positions >= its length filled with pad_idx;
 * out_len int32 [n_img] = its length (SOS and EOS included). */
int odic_beam_finalize_best(const odic_beam_state* st, int32_t* order, float* score, int32_t* out_tok,
                            int32_t* out_len, int32_t n_img, int32_t beams, int32_t T, int32_t pad_idx,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * CIDEr-D on word ids (csrc/cider.hip): the self-critical reward and consensus reranking.
 *   N-gram key: the n-gram (id_0 … id_{k-1}), k = 1..4, is the uint64 Σ_j (id_j + 1) << (16·j); unused high fields are 0,
 *   so the order is the index of the highest non-zero field and keys of different orders never collide.  ids lie in
 *   [0, ODIC_CIDER_MAX_ID].  Keys are compared and sorted as UNSIGNED values (an id >= 32767 in field 3 sets bit 63).
 *   Workspace: one row of ODIC_CIDER_ROW_WORDS 8-byte words per caption, row pitch ldw words:
 *     words [0, 512)      uint64  the caption's unique keys, ascending; entries [0, count) are written
 *     words [512, 1024)   fp64    w = tf·idf of the key at the same index; entries [0, count) are written
 *     words [1024, 1028)  fp64    per-order norms sqrt(Σ w²), orders 1..4
 *     word  1028          int32 count, int32 length — `length` is what the Gaussian penalty compares: the number of
 *                         BIGRAM tokens of the caption, max(L − 1, 0) (the reference's quirk, cider.py's docstring)
 * --------------------------------------------------------------------------------------------- */
#define ODIC_CIDER_MAX_LEN 128      /* words per caption: the decoder's position limit */
#define ODIC_CIDER_MAX_KEYS 512     /* >= 128 + 127 + 126 + 125 = 506 n-grams */
#define ODIC_CIDER_MAX_ID 65533
#define ODIC_CIDER_ROW_WORDS 1029
#define ODIC_CIDER_SIGMA 6.0

/* R captions → their workspace rows, one block per caption: the n-grams of orders 1..4 are sorted in LDS, run-length
 * encoded into unique keys with their term frequency, and weighted with the IDF of the table.
 *   tokens int32 [R, ld], lengths int32 [R]: caption r is tokens[r][0 .. L), L = lengths[r] clamped into [0, max_len]; an
 *   id in the device data is clamped into [0, max_id] — neither is trusted.
 *   Table: df_keys uint64 [n_table] ascending, df_idf fp64 [n_table], the IDF of each key as the host computed it (the
 *   kernel takes no logarithm).  A key outside the table gets default_idf; n_table == 0: every key does.
 *   ODIC_ENULL: tokens, lengths or ws NULL, or n_table > 0 with a table pointer NULL.  ODIC_EINVAL: R <= 0, n_table < 0,
 *   max_len outside [0, 128], ld < max_len, max_id outside [0, 65533], ldw < ODIC_CIDER_ROW_WORDS, default_idf NaN.  Both
 *   before any launch.  All stores stay inside words [0, ODIC_CIDER_ROW_WORDS) of the R rows. */
int odic_cider_vectorize(const int32_t* tokens, int64_t ld, const int32_t* lengths, int32_t R, int32_t max_len,
                         int32_t max_id, const uint64_t* df_keys, const double* df_idf, int32_t n_table,
                         double default_idf, uint64_t* ws, int64_t ldw, void* stream);

/* Clipped cosine similarities of vectorised rows, one wave per (hypothesis, reference slot).  Hypothesis h is workspace row
 * h (the hypotheses are the first H rows); its references are the rows [ref_begin[h], ref_end[h]).  For slot s < max_refs,
 * with j = ref_begin[h] + s:
 *   sim[h][s] = 10 · ¼ Σ_{order} ( Σ_g min(w_h[g], w_j[g])·w_j[g] / (norm_h·norm_j) ) · exp(−Δ² / (2σ²))
 *   over the hypothesis's keys g, the division only where both norms are non-zero, Δ = length_h − length_j, σ = 6;
 *   sim[h][s] = 0 where j >= ref_end[h] or j lies outside [0, R) (a reference count above max_refs is cut at max_refs).
 * sim fp64 [H, lds]: every column [0, max_refs) of every row is written, nothing else.  Fixed reduction tree, no atomics:
 * two runs give the same bits.
 *   ODIC_ENULL for a NULL pointer; ODIC_EINVAL for R <= 0, H <= 0, H > R, max_refs <= 0, ldw < ODIC_CIDER_ROW_WORDS or
 *   lds < max_refs.  Both before any launch. */
int odic_cider_pairs(const uint64_t* ws, int64_t ldw, int32_t R, const int32_t* ref_begin, const int32_t* ref_end,
                     int32_t H, int32_t max_refs, double* sim, int64_t lds, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BLEU-1..4 and ROUGE-L on word ids (csrc/caption_metrics.hip): the integer parts of both metrics; the
 * scores are a few fp64 operations on them (metrics.py).  Both kernels reduce integers in a fixed tree, without atomics:
 * two runs give the same bits.
 * --------------------------------------------------------------------------------------------- */
#define ODIC_BLEU_STAT_WORDS 12

/* The BLEU components of Q queries, one wave per query.  Query q is (hyp_row[q], ref_begin[q], ref_end[q]): workspace row
 * hyp_row[q] is the hypothesis, the rows [ref_begin[q], ref_end[q]) are its references.  Any row may be the hypothesis of
 * any number of queries (one query per image for evaluation, N·N single-reference queries per image for pairwise scores).
 *   REQUIRED MODE of the workspace: the rows odic_cider_vectorize writes with n_table = 0 and default_idf = 1.0.  The stored
 *   weight is then the term frequency, an exact small integer in fp64, and is read as one.  With any other weights the
 *   counts are meaningless (nothing is read or written out of bounds).
 *   lengths int32 [R]: the captions' lengths again (the row records only the bigram count), clamped into [0, max_len] as
 *   vectorize clamps them; pass the max_len the rows were vectorised with.
 *   stats int32 [Q, lds], words [0, ODIC_BLEU_STAT_WORDS) of every row are written, nothing else.  With L the hypothesis
 *   length:
 *     [0..3]  correct_k, k = 1..4: Σ over the hypothesis's unique k-grams of min(tf_hyp, max over the references of tf_ref)
 *             — clipped against the MAXIMUM over the references, not their sum
 *     [4..7]  guess_k = max(0, L − k + 1)
 *     [8]     testlen = L
 *     [9]     the closest reference length: the l that minimises (|l − L|, l), a tie going to the shorter reference
 *     [10]    the shortest reference length        [11]  the sum of the reference lengths (modulo 2^32)
 *   A reference index outside [0, R) is skipped, never dereferenced.  An empty range (or one that lies outside [0, R))
 *   gives 0 in [0..3] and [9..11].  A hyp_row outside [0, R) gives a row of twelve zeros.
 *   ODIC_ENULL for a NULL pointer; ODIC_EINVAL for Q <= 0, R <= 0, ldw < ODIC_CIDER_ROW_WORDS, lds < ODIC_BLEU_STAT_WORDS
 *   or max_len outside [0, 128].  Both before any launch. */
int odic_bleu_stats(const uint64_t* ws, int64_t ldw, const int32_t* lengths, int32_t R, int32_t max_len,
                    const int32_t* hyp_row, const int32_t* ref_begin, const int32_t* ref_end, int32_t Q, int32_t* stats,
                    int64_t lds, void* stream);

/* Longest-common-subsequence lengths straight from token rows, one wave per (hypothesis, reference slot), bit-parallel
 * (Hyyrö's bit-vector recurrence on 128 bits, the match masks from two ballots per hypothesis token).
 *   tokens int32 [R, ld], lengths int32 [R]: caption r is tokens[r][0 .. L), L = lengths[r] clamped into [0, max_len].  The
 *   ids may be ANY int32: words are only compared, there is no key and no id limit.
 *   Rows [0, H) are the hypotheses; the references of hypothesis h are the rows [ref_begin[h], ref_end[h]) — the convention
 *   of odic_cider_pairs.  For slot s < max_refs, with j = ref_begin[h] + s:
 *     lcs[h][s] = the LCS length of rows h and j; 0 where either is empty;
 *     lcs[h][s] = 0 where j >= ref_end[h] or j lies outside [0, R) (a reference count above max_refs is cut at max_refs).
 *   lcs int32 [H, ldl]: every column [0, max_refs) of every row is written, nothing else.
 *   ODIC_ENULL for a NULL pointer; ODIC_EINVAL for R <= 0, H <= 0, H > R, max_refs <= 0, ldl < max_refs, max_len outside
 *   [0, 128] or ld < max_len.  Both before any launch. */
int odic_lcs_pairs(const int32_t* tokens, int64_t ld, const int32_t* lengths, int32_t R, int32_t max_len,
                   const int32_t* ref_begin, const int32_t* ref_end, int32_t H, int32_t max_refs, int32_t* lcs, int64_t ldl,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ODIC_HIP_H */
