/* rdmi.h — C ABI of librdmi.so, the MI355X (gfx950) HIP kernels of RollingDepth's
 * snippet-denoise hot path.
 *
 * The reference (yizuo417/RollingDepth) has no native code and no FFI: its hot path is implicit
 * PyTorch library kernels issued from Python.  Each entry point below
 * replaces one such implicit op (or a fused group of them) and names the reference call site it
 * stands in for.  The Python host package `rollingdepth_amd` binds these through ctypes
 * (INTEGRATION.md shows the binding a maintainer of the reference would add).
 *
 * Conventions:
 *  - plain pointers (device memory owned by the caller), sizes and strides in ELEMENTS, and a
 *    hipStream_t passed as `void*` (0 = the null stream);
 *  - activations are NHWC / token-major [B, S, C]; f16 storage with f32 accumulation unless a
 *    parameter says otherwise; norm affine parameters and biases are f32;
 *  - every call returns 0 or an error code (RDMI_E_* for bad arguments, else the hipError_t of
 *    the launch); rdmi_last_error() returns a thread-local message; nothing synchronises the
 *    device, allocates, frees, or retains a pointer after return, so every call is graph-capturable.
 */
#ifndef RDMI_H
#define RDMI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDMI_OK 0
#define RDMI_E_ARG 1001         /* bad shape / stride / null pointer */
#define RDMI_E_ALIGN 1002       /* pointer or leading dimension not 16-byte aligned */
#define RDMI_E_UNSUPPORTED 1003 /* configuration this build does not implement */

/* storage dtype codes of the `dtype` arguments (f32 is the paper preset's arithmetic, run_video.py:444-449) */
#define RDMI_F16 0
#define RDMI_F32 1
#define RDMI_U8 2 /* decoded video frames (rdmi_resize input) */
/* rdmi_gemm / rdmi_conv2d only: f32 activations and output, weights pre-split into bf16 hi/lo parts,
 * products a_hi·w_hi + a_hi·w_lo + a_lo·w_hi on the bf16 MFMA with f32 accumulation (≈2^-16 relative
 * error per product; the paper preset's fast f32 engine, RDMI_F32_X3=1 in rollingdepth_amd) */
#define RDMI_F32_X3 3
/* rdmi_attention_fwd (round 5): f32 q/k/v/o and softmax, both products on the bf16 MFMA over a three-way
 * bf16 split of each f32 operand (hi + mid + lo, six partial products kept): a few 2^-24 relative per
 * product — f32's own product rounding, the reference's exact-fp32 SDPA precision — at ≈0.4 of the
 * exact f32-input MFMA's matrix time */
#define RDMI_F32_X6 4

/* rdmi_resize modes: torchvision InterpolationMode NEAREST / BILINEAR / BICUBIC */
#define RDMI_RESIZE_NEAREST 0
#define RDMI_RESIZE_BILINEAR 1
#define RDMI_RESIZE_BICUBIC 2

#define RDMI_EPI_NONE 0
#define RDMI_EPI_GEGLU 1 /* out[:, n] = (h + b_h) * gelu_erf(g + b_g), weights row-interleaved */
#define RDMI_EPI_SILU 2  /* out = silu(acc·alpha + bias ...) (TimestepEmbedding act, embeddings.py:543) */

/* ---------------------------------------------------------------------------------------
 * Library
 */
const char* rdmi_last_error(void);
int rdmi_version(void);

/* ---------------------------------------------------------------------------------------
 * GEMM (Linear layers): C[b] = alpha * A[b] · W[b]ᵀ (+ bias[n]) (+ rowbias[m / rows_per_group][n])
 *                                                     (+ residual[b][m][n])
 * A [M, K] f16 (lda), W [N, K] f16 (ldw ≥ K), K % 8 == 0, C f16 or f32 (ldc).
 * Replaces torch.nn.Linear / F.linear in Attention.to_q/k/v/to_out
 * (diffusers/models/attention_processor.py:2226-2261), FeedForward/GEGLU
 * (diffusers/models/attention.py:1116, activations.py:113-123), Transformer2DModel.proj_in/out
 * (transformers/transformer_2d.py:485-533) and TimestepEmbedding (embeddings.py:543).
 */
typedef struct rdmi_gemm_args {
  const void* A; long lda; long strideA;
  const void* W; long ldw; long strideW;
  void* C; long ldc; long strideC; int c_f32;
  const float* bias;
  const void* residual; long ldr; long strideR;
  const float* rowbias; int rows_per_group; long rowbias_ld;
  float alpha;
  int M, N, K, batch;
  int epilogue;
  /* optional GroupNorm moments of the f16 output (batch == 1, f16 C, N % 4 == 0, M % 32 == 0):
   * gn_part[v * gn_ld + 2*r + {0,1}] = (Σ, Σ²) over output rows 32r..32r+31 and channels
   * 4v..4v+3, summed in a fixed order (rdmi_groupnorm_stats_partials consumes them).  NULL: off. */
  float* gn_part; long gn_ld;
  /* storage dtype of A, W, C and residual: RDMI_F16 (f16 MFMA, f32 accumulate; C f32 when c_f32) or
   * RDMI_F32 (the paper preset: f32-input MFMA v_mfma_f32_16x16x4_f32, exact f32 products, C / residual
   * f32; K % 4 == 0; no GroupNorm moments) or RDMI_F32_X3 (as RDMI_F32, W the bf16 split layout:
   * row n holds, per 32-deep K-tile t, bf16(w[n, 32t..32t+31]) then bf16(w − that), so ldw / strideW
   * count bf16 elements, ldw % 64 == 0 and ldw ≥ 2·ceil(K/32)·32) */
  int dtype;
} rdmi_gemm_args;
int rdmi_gemm(const rdmi_gemm_args* args, void* stream);

/* ---------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on NHWC f16 (MFMA 16x16x32 f16, f32 accumulate).
 * y[b, ho, wo, co] = alpha * Σ w[co, dy, dx, ci] x[b, ho*s - pt + dy, wo*s - pl + dx, ci]
 *                    (+ bias[co]) (+ rowbias[b * rowbias_ld + co]) (+ residual[b, ho, wo, co])
 * `upsample`=1 reads x through a nearest ×2 upsample (Upsample2D, upsampling.py:141-190) without
 * materialising it.  Cin % 8 == 0 (pad channels).  Weight layout, zero padded to Kp % 32 == 0:
 *   kh*kw > 1 and Cin % 64 == 0: [Cout][Cin/64][kh][kw][64] (channel-block major: one K-tile of 64
 *     is one tap of a 64-channel block, i.e. one full 128-B line per output pixel, and the taps of
 *     a block are adjacent in K, so the implicit-im2col re-reads of a block hit L2);
 *   otherwise:                    [Cout][kh][kw][Cin].
 * Replaces the cuDNN conv2d of ResnetBlock2D.conv1/conv2/conv_shortcut (resnet.py:320-373),
 * Downsample2D (downsampling.py:132-148, including the VAE's F.pad(0,1,0,1) via pad_top/left=0
 * with the extra row/column read as zero), Upsample2D.conv, conv_in/conv_out of the UNet and VAE.
 */
typedef struct rdmi_conv_args {
  const void* x; const void* w; void* y;
  const float* bias; const void* residual; const float* rowbias;
  int B, H, W, Cin, Cout, kh, kw, stride, pad_top, pad_left, upsample, Ho, Wo, Kp;
  long y_ld; long res_ld; float alpha; long rowbias_ld; /* 0: one row shared by all images */
  float* gn_part; long gn_ld; /* GroupNorm moments of y, laid out as in rdmi_gemm_args; rows = B·Ho·Wo */
  /* GroupNorm (+SiLU) of the INPUT applied as x is read (the norm1/norm2 → conv1/conv2 pairs of
   * ResnetBlock2D, resnet.py:326-352): the conv sees silu?(x·sc + sh) with sc = rstd·gamma[c],
   * sh = beta[c] − mean·sc per image b (in_mean_rstd as rdmi_groupnorm_stats writes it), the
   * padding still zero; the same values rdmi_groupnorm_apply writes.  NULL in_mean_rstd: off.
   * Shapes that support it: rdmi_conv2d_in_gn_supported (otherwise RDMI_E_UNSUPPORTED). */
  const float* in_mean_rstd; const float* in_gamma; const float* in_beta; int in_groups, in_silu;
  /* RDMI_F16 or RDMI_F32 (x, w, y, residual).  f32 weights are always [Cout][kh][kw][Cin] (tap-major,
   * Kp % 32 == 0), Cin % 4 == 0, no input GroupNorm and no GroupNorm moments.  RDMI_F32_X3: f32 x, y,
   * residual; w in the bf16 split layout that rdmi_gemm_args describes, rows of 2·Kp bf16 (Kp still counts f32 K). */
  int dtype;
  /* Optional, upsample = 1 only: the same conv's weights for the phase-decomposed form — the ×2
   * nearest upsample + 3×3 conv computed as four 2×2 convs on the source grid, one per output
   * phase (a, c) = (y & 1, x & 1), the 3×3 taps that read the same source pixel merged
   * (rows {0 | 1,2} for a = 0, {0,1 | 2} for a = 1; columns likewise).  A merged weight Σw (sum in
   * f32 of 2 or 4 f16 taps) is stored as hi = f16(Σw) and lo = f16(Σw − hi), so every product is
   * exact in the f32 accumulator: the result is the 9-tap conv's up to f32 accumulation order (and
   * lo's f16 rounding where Σw − hi is subnormal or wider than 11 bits), in 7/9 of the MFMA work.
   * Layout [4 phases (2a + c)][Cout][Cin/64][7][64] f16 (row stride 7·Cin): per 64-channel block
   * the hi parts of taps (dy, dx) = (0,0), (0,1), (1,0), (1,1), then the lo parts of those taps other
   * than (a, c) (a single 3×3 weight, exact in f16), in the same order.  Used where the halo engine
   * runs the conv (f16, Cin % 64 == 0, Ho % 32 == 0, Wo % 32 == 0, no input GroupNorm); elsewhere
   * `w` is used.  NULL: off. */
  const void* w_up2;
  /* Optional with in_mean_rstd (round 5): the input GroupNorm's per-channel scale / shift as
   * rdmi_groupnorm_affine writes them, [B][Cin/64][2][64] f32 — per image and 64-channel block the 64
   * scales sc = rstd·gamma[c], then the 64 shifts sh = beta[c] − mean·sc.  With it the
   * two-workgroups-per-CU halo engine fuses the norm for any Cin % 64 == 0 (each wave loads the block's
   * 8 + 8 values of its lanes with the halo refill); without it only for Cin ≤ 256 (the table built in
   * LDS).  The values are the ones the kernel would compute itself: bitwise the same results. */
  const float* in_affine;
} rdmi_conv_args;
int rdmi_conv2d(const rdmi_conv_args* args, void* stream);
/* 1 if rdmi_conv2d fuses an input GroupNorm for this shape (in_groups set; pointers not read) */
int rdmi_conv2d_in_gn_supported(const rdmi_conv_args* args);

/* ---------------------------------------------------------------------------------------
 * GroupNorm on NHWC f16 / f32 (dtype RDMI_F16 / RDMI_F32): statistics then apply (optionally fused SiLU).
 * Replaces F.group_norm (+ SiLU) of ResnetBlock2D.norm1/norm2 (resnet.py:326,351),
 * Transformer2DModel.norm (transformer_2d.py:175-177), conv_norm_out of UNet/VAE, and the VAE
 * mid-block Attention.group_norm (attention_processor.py:2221-2222).
 * stats: mean_rstd[b*G + g] = {mean, rstd}; workspace ≥ rdmi_groupnorm_workspace(B, G) floats.
 */
long rdmi_groupnorm_workspace(int B, int G);
int rdmi_groupnorm_stats(const void* x, int dtype, int B, long HW, int C, int G, float eps,
                         float* mean_rstd, float* workspace, void* stream);
/* Statistics from the 32-row × 4-channel moments a producing GEMM/conv emitted (gn_part): for
 * image b (rows b·HW .. b·HW+HW-1, HW % 32 == 0) and group g ((C/G) % 4 == 0), an f64 sum over the
 * group's partials in a fixed order — independent of how many images share the tensor. */
int rdmi_groupnorm_stats_partials(const float* part, long part_ld, int B, long HW, int C, int G, float eps,
                                  float* mean_rstd, void* stream);
/* Input-GroupNorm scale / shift table for rdmi_conv_args.in_affine: out [B][C/64][2][64] f32, per image b
 * and 64-channel block the scales rstd·gamma[c] then the shifts beta[c] − mean·(rstd·gamma[c]) — the f32
 * arithmetic of rdmi_groupnorm_apply (mean_rstd as rdmi_groupnorm_stats writes it; C % 64 == 0). */
int rdmi_groupnorm_affine(const float* mean_rstd, const float* gamma, const float* beta, int B, int C, int G,
                          float* out, void* stream);
int rdmi_groupnorm_apply(const void* x, void* y, int dtype, int B, long HW, int C, int G,
                         const float* mean_rstd, const float* gamma, const float* beta, int silu,
                         void* stream);

/* GroupNorm apply (+ SiLU when silu = 1) fused with a 3×3, stride-1, pad-1 convolution to ONE output
 * channel: y[b, h, w] = bias + Σ_{dy,dx,c} w[3dy+dx][c] · n(x)[b, h+dy-1, w+dx-1, c], n = the
 * normalised (+SiLU) input, zero outside the image.  x [B][H][W][C] in `dtype` (RDMI_F16 / RDMI_F32),
 * y [B][H][W] in `y_dtype` (RDMI_F16 / RDMI_F32: the f16 pipeline keeps its decoded depth in f32, so
 * the f16 rounding of the depth map does not reach the aligner and the min/max renormalisation),
 * w [9][C] f32, workspace ≥ rdmi_conv3x3_to1_gn_workspace(B, H, W) floats.  Replaces the decoder's
 * conv_norm_out → conv_act → conv_out (vae.py:335-347) followed by the depth pipeline's mean over
 * the RGB outputs (rollingdepth_pipeline.py:737), which is linear and folded into w / bias. */
long rdmi_conv3x3_to1_gn_workspace(int B, int H, int W);
int rdmi_conv3x3_to1_gn(const void* x, int dtype, int B, int H, int W, int C, int G, const float* mean_rstd,
                        const float* gamma, const float* beta, int silu, const float* w, float bias,
                        void* y, int y_dtype, float* workspace, void* stream);

/* LayerNorm over the last dim (BasicTransformerBlock.norm1/2/3, attention.py:445,495,522). */
int rdmi_layernorm(const void* x, void* y, int dtype, long M, int C, const float* gamma, const float* beta,
                   float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused multi-head attention forward, softmax(q kᵀ · scale) v, non-causal, no mask, D = 64; dtype
 * RDMI_F16 (f16 MFMA, f32 softmax), RDMI_F32 (f32-input MFMA, f32 softmax; the paper preset) or
 * RDMI_F32_X3 (f32 q/k/v/o and softmax, both products as bf16-split triples on the bf16 MFMA) or
 * RDMI_F32_X6 (the same with three-part splits and six products: f32-equivalent products).
 * Token-major q/k/v/o with row strides (ld*) and batch strides (bs*), head h at column h*D.
 * With the num_view fold done by the caller's strides (one "batch" = one snippet of n frames,
 * S = n·h·w), this is the cross-frame self-attention of the modified AttnProcessor2_0
 * (attention_processor.py:2208-2266) / XFormersAttnProcessor (:1989-2050).
 */
int rdmi_attention_fwd(const void* q, const void* k, const void* v, void* o, int B, int H, int Sq,
                       int Sk, int D, long q_ld, long k_ld, long v_ld, long o_ld, long q_bs,
                       long k_bs, long v_bs, long o_bs, float scale, int dtype, void* stream);

/* Attention against a short key set (L ≤ 16 keys, e.g. the 2-token empty-text context of the
 * UNet cross-attention attn2, attention.py:508-516); k/v [Bkv][L][H*D] contiguous, Bkv ∈ {1, B}. */
int rdmi_attention_smallkv(const void* q, const void* k, const void* v, void* o, int B, int H,
                           int Sq, int L, int D, long q_ld, long o_ld, long q_bs, long o_bs,
                           long kv_bs, float scale, int dtype, void* stream);

/* BasicTransformerBlock's norm2 → attn2 → +residual against a TWO-token shared context
 * (attention.py:480-492, attention_processor.py:2172-2276 with Sk = 2), collapsed by exact algebra:
 * y = x + c + Σ_h σ(LN(x)·w_h) u_h with w = scale·Wq_hᵀ(K1−K0)_h and u_h = Wo_h(V1−V0)_h
 * ([H, C] f32 each, 16-B aligned), c = Wo·V0 + bo ([C] f32).  x, y: [M, C] f16 rows (C ≤ 1536,
 * 2·H·C·4 B ≤ 64 KiB).  Replaces LN + q GEMM + rdmi_attention_smallkv + out GEMM for that case. */
int rdmi_cross_attn_pair(const void* x, void* y, long M, int C, int H, const float* ln_gamma,
                         const float* ln_beta, float eps, const float* w, const float* u, const float* c,
                         void* stream);

/* Row softmax: p[r, :] = softmax(scale * s[r, :]) (f32 in, p_dtype out: RDMI_F16 / RDMI_F32).  Used with two rdmi_gemm
 * calls for the single-head d=C VAE mid-block attention (unet_2d_blocks.py:680-697). */
/* p[r·p_ld + c] = softmax_c(scale·s[r·cols + c]) for c < cols, 0 for cols ≤ c < p_ld (so a PV GEMM
 * can run on K = p_ld, a multiple of 8, when the key count is not). */
int rdmi_softmax_rows(const float* s, void* p, long rows, long cols, long p_ld, float scale, int p_dtype,
                      void* stream);

/* ---------------------------------------------------------------------------------------
 * Layout / elementwise helpers (f16 NHWC unless stated)
 */
/* NCHW (f32 if x_f32 else f16, batch/channel strides in elements; x_cstride = 0 replicates one
 * channel, e.g. the depth → 3-channel repeat before re-encoding, rollingdepth_pipeline.py:327)
 * → NHWC in y_dtype (RDMI_F16 / RDMI_F32) with channel padding to Cpad (zeros), y = x*scale */
int rdmi_nchw_to_nhwc(const void* x, int x_f32, void* y, int y_dtype, int B, int C, int H, int W, int Cpad,
                      float scale, long x_bstride, long x_cstride, void* stream);
/* NHWC in dtype (ld = channel stride) → NCHW f32, first C channels, y = x*scale + shift */
int rdmi_nhwc_to_nchw_f32(const void* x, int dtype, long ld, float* y, int B, int C, int H, int W,
                          float scale, float shift, void* stream);
/* The helpers below take the storage dtype (RDMI_F16 / RDMI_F32) of every activation operand. */
/* y[p, 0:Ca] = a[p, :], y[p, Ca:Ca+Cb] = b[p, :]  (torch.cat dim=1 of CrossAttn/UpBlock skips);
 * Ca, Cb multiples of one 16-B vector (8 f16 / 4 f32) */
int rdmi_concat_channels(const void* a, int Ca, const void* b, int Cb, void* y, long P, int dtype, void* stream);
/* NHWC f16 nearest resize to an explicit size: y[b,yo,xo] = x[b, ⌊yo·H/Ho⌋, ⌊xo·W/Wo⌋] (f32 scale,
 * clamped) — F.interpolate(size=…, mode="nearest") of Upsample2D when the UNet forwards an
 * upsample size (latent not a multiple of 2^levels; unet_2d_condition.py forward_upsample_size,
 * upsampling.py:167-178).  C % 8 == 0. */
int rdmi_resize_nearest(const void* x, int B, int H, int W, int C, void* y, int Ho, int Wo, int dtype,
                        void* stream);
/* 2-D transpose per batch: dst[b][c][r] = src[b][r][c] */
int rdmi_transpose(const void* src, void* dst, int batch, long rows, long cols, long src_ld,
                   long dst_ld, int dtype, void* stream);
/* Build the 8-channel UNet input of single_step (rollingdepth_pipeline.py:646-651):
 * out[i, p, 0:4] = rgb[frame_idx[i], p, 0:4], out[i, p, 4:8] = depth[dsel(i), p, 0:4]
 * (depth_ld: frame stride of `depth` in elements; depth_bcast=1 uses depth frame 0 for all). */
int rdmi_gather_unet_input(const void* rgb, long rgb_frame_ld, const void* depth,
                           long depth_frame_ld, int depth_bcast, const int* frame_idx, int count,
                           long HW, void* out, int dtype, void* stream);
/* DDIM step (eta = 0) / add_noise as the affine map they reduce to (scheduling_ddim.py:402-448,
 * :471-495): y = (ca·x + cb·e) * out_scale; x, e: [P] pixel rows with strides, y [P, ld_y]
 * channels 0..C-1, channels C..Cpad-1 of y zeroed; e_period > 0 broadcasts e over pixel rows
 * (the shared init noise of every frame, :282-288). */
int rdmi_ddim_combine(const void* x, long ld_x, const void* e, long ld_e, void* y, long ld_y,
                      long P, int C, int Cpad, float ca, float cb, float out_scale, long e_period,
                      int dtype, void* stream);
/* Refine averaging (rollingdepth_pipeline.py:586-629): out[f] = mean over the snippets s = f − j·stride
 * (0 ≤ s < n) of src[s][j]; src [n][w][P][ld], out [N][P][ld] f16 (channels ≥ C zeroed).  The sum is
 * taken in f64: exact for f16 terms (hence independent of the order of addition); for f32 terms
 * order-independent except when the terms' exponents span more than ≈29 bits (rare). */
int rdmi_snippet_average(const void* src, int n, int w, int stride, int N, long P, int C, int ld,
                         void* out, int dtype, void* stream);
/* Depth colourisation (src/util/colorize.py:12-93, the CLI's visualisation): rgb [n][3] u8 =
 * lut[idx(d)] with idx as matplotlib's Colormap.__call__ computes it for the normalised depth
 * ((d - minmax[0]) / (minmax[1] - minmax[0]) clipped to [0, 1], evaluated in the depth's dtype),
 * lut [(lut_n + 3)][3] = (colormap table · 255) as uint8 incl. the under / over / bad entries.  minmax =
 * {min, max − min} in the depth's dtype (the range as the reference's numpy forms it).  index != NULL:
 * write the table index per pixel instead (lut / rgb unused). */
int rdmi_colorize(const void* depth, int dtype, long n, const void* minmax, const unsigned char* lut, int lut_n,
                  unsigned char* rgb, int* index, void* stream);
/* Sharded refine averaging (the loop above split over ranks): sum [N][P][C] f64 =
 * per frame the sum over THIS rank's snippets k0 .. k0+nloc-1 (src [nloc][w][P][ld], dtype RDMI_F16 /
 * RDMI_F32), zero where none covers the frame; after an all-reduce SUM over ranks,
 * rdmi_snippet_finish divides by the frame's cover count over all n snippets → out [N][P][ld]
 * (channels ≥ C zeroed).  The f64 sums are exact for f16 terms, so every world size and every
 * all-reduce order reproduces rdmi_snippet_average bitwise; with f32 terms the same holds except in rare
 * rounding cases (terms whose exponents span more than ≈29 bits). */
int rdmi_snippet_accumulate(const void* src, int dtype, int k0, int nloc, int w, int stride, int N, long P, int C,
                            int ld, double* sum, void* stream);
int rdmi_snippet_finish(const double* sum, int n, int w, int stride, int N, long P, int C, int ld, void* out,
                        int dtype, void* stream);
/* The three refine averaging calls above for a strided refine step (since rdmi_version 4;
 * csrc/refine_index.h): inside each
 * residue class of the frames mod `stride` (frames r, r + stride, ...; positions 0, 1, 2, ...) the
 * snippets start every start_step positions, plus the class's last window when that misses it; src rows
 * are in class-major order (class ascending, then position).  Slot j of frame f is filled by the snippet
 * that starts at frame f − j·stride, its row found in closed form (arguments by value, no table in
 * memory); a frame no snippet covers comes out as zeros.  Sum, division and rounding as above, so
 * accumulate (any shards, any all-reduce order) + finish reproduce average bitwise, and start_step 1 is
 * rdmi_snippet_average on the rows sorted by start frame.  1 ≤ start_step ≤ w (a larger step leaves
 * frames uncovered) and n = the map's snippet count (k0 + nloc ≤ it) are checked, RDMI_E_ARG before any
 * launch. */
int rdmi_snippet_average_strided(const void* src, int n, int w, int stride, int start_step, int N, long P, int C,
                                 int ld, void* out, int dtype, void* stream);
int rdmi_snippet_accumulate_strided(const void* src, int dtype, int k0, int nloc, int w, int stride, int start_step,
                                    int N, long P, int C, int ld, double* sum, void* stream);
int rdmi_snippet_finish_strided(const double* sum, int n, int w, int stride, int start_step, int N, long P, int C,
                                int ld, void* out, int dtype, void* stream);
/* Global min/max of an f16 or f32 buffer → minmax[2] f32 (workspace ≥ 2*1024 floats)
 * (the `min([snippet.min() ...])` of depth_aligner.py:78 and the min/max of :316-317). */
int rdmi_minmax(const void* x, int x_f32, long n, float* minmax, float* workspace, void* stream);
/* In place: x = (x - mn) / (mx - mn) * 2 - 1 with mn,mx read from device (re-normalise, :316-318) */
int rdmi_renormalize_f32(float* x, long n, const float* minmax, void* stream);

/* ---------------------------------------------------------------------------------------
 * DepthAligner (rollingdepth/depth_aligner.py) — co-alignment of dilated snippets.
 * Snippet layout: one f32 buffer per dilation, x_d [n_d][w_d][P] (border-cropped, stride-subsampled,
 * min-shifted; depth_aligner.py:78-92).  Parameters s_d, t_d are f32 [n_d].  Snippet lengths w_d may
 * differ per dilation (rollingdepth_pipeline.py:221-226): the loss then follows the reference's
 * scatter of dilation i's slot j into row i·w_i + j of [Σw, N, P] (depth_aligner.py:169-188) —
 * coinciding rows are overwritten by the later dilation, and a layout whose rows run past Σw
 * (the reference's IndexError) is rejected with RDMI_E_ARG.
 *
 * Start step (since rdmi_version 2): the snippets of dilation d start every start_step[d] frames
 * (get_snippet_indice's `stride`, rollingdepth_pipeline.py:465-502; `stride` here stays the frame step
 * INSIDE a snippet, the dilation).  With win = (w_d − 1)·stride_d + 1 and last = seq_len − win, snippet k
 * starts at frame min(k·start_step, last) and n_d = last / start_step + 1, plus 1 when start_step does
 * not divide last (the reference appends the last window) — csrc/aligner_index.h.  start_step 0 means 1.
 * With every start step 1 the calls run the kernels of version 1 unchanged.  Only when some start step
 * is > 1 is the layout checked, before any launch: a negative start step, seq_len < win or an n_d other
 * than the count above → RDMI_E_ARG with a rdmi_last_error text.  The loss still means over the full
 * [Σw, seq_len, P] tensor.  rdmi_aligner_workspace depends only on the arguments (seq_len, P, Σ n_d,
 * iters, history or not — csrc/aligner_ws.h), never on the environment or the start steps: a workspace
 * sized once serves every later call with the same arguments.  The sharded merge calls
 * (partial_window / finish_pieces) keep start step 1; since rdmi_version 3 their _strided forms take the
 * start steps, with the same check before any launch.
 */
typedef struct rdmi_aligner_args {
  int n_dil;                 /* number of dilations (≤ 8) */
  const float* x[8];         /* subsampled snippets per dilation [n_d][w_d][P] */
  float* s[8]; float* t[8];  /* scales / translations [n_d] (in: init, out: result) */
  int n[8]; int stride[8];   /* snippets per dilation, frame stride (dilation) */
  int w[8];                  /* snippet length per dilation (Σ w_d ≤ 64) */
  int seq_len; long P;
  float lr, beta1, beta2, eps, lmda2, lmda3, depth_w, loss_scale;
  int iters;
  float* history;            /* [iters][3] (loss, min summ, max summ) or NULL */
  float* workspace;          /* ≥ rdmi_aligner_workspace(...) floats */
  int start_step[8];         /* frames between snippet starts per dilation (0 = 1; see above) */
} rdmi_aligner_args;
long rdmi_aligner_workspace(const rdmi_aligner_args* a);
/* Adam loop of DepthAligner.optimize (:123-229) fully on device, no host sync. */
int rdmi_aligner_optimize(const rdmi_aligner_args* a, void* stream);
/* Border crop + stride subsample + min shift of one dilation's decoded snippets
 * x [n][w][H][W] (f16/f32) → out [n][w][P] f32 with out = dtype(x - shift[0]) (:78-92). */
int rdmi_aligner_prepare(const void* x, int x_f32, int n, int w, int H, int W, int border,
                         int factor, const float* shift, float* out, void* stream);
/* merge_scaled_triplets (:231-262): full-resolution snippets per dilation xf_d [n_d][w_d][HW]
 * (w: snippet length per dilation)
 * (x_f32 = 1: f32 snippets; 0: f16 snippets in the reference's f16 arithmetic; 2: f16 snippets with
 * the shift and s·x+t in f32 — no intermediate f16 rounding; the min shift read from shift[0] is
 * applied first),
 * s/t f32 → out [seq_len][HW] f32 (s·x+t rounded through the snippet dtype exactly where the
 * reference computes in it; the per-frame mean is accumulated in f32). */
int rdmi_aligner_merge(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                       const float* const* t, const int* n, const int* stride, const int* w, int seq_len,
                       long HW, const float* shift, float* out, void* stream);
/* rdmi_aligner_merge for snippets that start every start_step[d] frames (see the start-step note
 * above; all ones: exactly rdmi_aligner_merge). */
int rdmi_aligner_merge_strided(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                               const float* const* t, const int* n, const int* stride, const int* start_step,
                               const int* w, int seq_len, long HW, const float* shift, float* out, void* stream);

/* Sharded merge over frame windows: each rank sums s·x+t of ITS full-resolution
 * snippets — rows k0[d] .. k0[d]+nloc[d]-1 of dilation d, xf_d [nloc_d][w_d][HW] — over only frames
 * f0 .. f0+nf-1 (the window its snippets cover) into sum_out [nf][HW] f64 (the per-slot arithmetic of
 * rdmi_aligner_merge, zero where no local slot covers a frame), sends every other rank the rows of that
 * rank's frame chunk (an all-to-all of uneven row counts), and rdmi_aligner_merge_finish_pieces adds the
 * received pieces per frame in source-rank order and divides by the frame's cover count over all n[d]
 * snippets: piece q = frames piece_f0[q] .. piece_f0[q]+piece_nf[q]-1 of one source, pieces stored back
 * to back in recv [Σ piece_nf][HW] f64, all inside this rank's frames f0 .. f0+nf-1 → out [nf][HW] f32.
 * Any piece count (the launch is split by frame range where more than 64 pieces arrive; a single frame
 * touched by more than 64 pieces → RDMI_E_UNSUPPORTED).  With f32 arithmetic (x_f32 1 / 2) the f64 sums
 * reproduce rdmi_aligner_merge bitwise in practice (exact while a frame's terms span ≤ ≈29 exponent bits). */
int rdmi_aligner_merge_partial_window(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                      const float* const* t, const int* n, const int* stride, const int* k0,
                                      const int* nloc, const int* w, int f0, int nf, long HW, const float* shift,
                                      double* sum_out, void* stream);
int rdmi_aligner_merge_finish_pieces(int n_dil, const int* n, const int* stride, const int* w, int f0, int nf, long HW,
                                     int npieces, const int* piece_f0, const int* piece_nf, const double* recv,
                                     float* out, void* stream);
/* The two calls above for snippets that start every start_step[d] frames of seq_len (since rdmi_version 3;
 * see the start-step note above): k0 / nloc still count snippets, snippet k starting at frame
 * min(k·start_step, last), and the cover count is that of the strided layout (0 at a frame no snippet
 * reaches: out is 0 there).  The window / chunk f0 .. f0+nf-1 must lie inside the seq_len frames.  The
 * layout is checked as in rdmi_aligner_merge_strided, RDMI_E_ARG before any launch; all-ones start steps
 * launch exactly what the calls above launch. */
int rdmi_aligner_merge_partial_window_strided(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                              const float* const* t, const int* n, const int* stride,
                                              const int* start_step, const int* k0, const int* nloc, const int* w,
                                              int seq_len, int f0, int nf, long HW, const float* shift,
                                              double* sum_out, void* stream);
int rdmi_aligner_merge_finish_pieces_strided(int n_dil, const int* n, const int* stride, const int* start_step,
                                             const int* w, int seq_len, int f0, int nf, long HW, int npieces,
                                             const int* piece_f0, const int* piece_nf, const double* recv,
                                             float* out, void* stream);

/* Merge with the per-pixel spread of the merged terms (since rdmi_version 6).  The covering terms of frame f
 * and pixel p are a_i = s_k·(x − shift) + t_k, i = 1 … c, exactly the values rdmi_aligner_merge forms in
 * each x_f32 mode.  mean_out [seq_len][HW] f32 is rdmi_aligner_merge's out, bitwise; std_out [seq_len][HW]
 * f32 is their population standard deviation sqrt(max(0, Σa²/c − (Σa/c)²)): Σa and Σa² accumulated in f64
 * in the merge's (d, j) order, evaluated in f64 and rounded once, 0 where c ≤ 1.  One pass over the
 * snippets.  With HW % 4 == 0 and every base pointer (snippets, outputs) 16-byte aligned a lane takes 4
 * consecutive pixels with 16-byte loads (8-byte for f16 rows); otherwise one pixel per lane.
 * These calls always take start steps (all ones: snippets start at every frame), every one ≥ 1, and always
 * check the layout against the index map before any launch (the checks of rdmi_aligner_merge_strided): a
 * start step < 1, a window that does not fit seq_len, an n_d other than the map's count or a null output
 * → RDMI_E_ARG.  Σ w_d ≤ 64 (RDMI_E_UNSUPPORTED beyond).
 * Sharded form: rdmi_aligner_merge_partial_window_moments writes mom_out [nf][2][HW] f64 — per frame Σa
 * then Σa² over the rank's rows (k0 / nloc as rdmi_aligner_merge_partial_window; in mode 0 Σa is the f64
 * sum of the f16-rounded terms) — so a frame stays one row of the all-to-all; and
 * rdmi_aligner_merge_finish_pieces_moments adds the received pieces recv [Σ piece_nf][2][HW] per frame
 * in source-rank order for both moments, divides by the cover count and writes mean and std (piece tables
 * wider than 64 are split by frame range as in rdmi_aligner_merge_finish_pieces; nf = 0 needs no outputs).
 * The means reproduce rdmi_aligner_merge as the sharded merge does; the f64 sums of squares can depend on
 * the order of addition in their last bits. */
int rdmi_aligner_merge_moments(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                               const float* const* t, const int* n, const int* stride, const int* start_step,
                               const int* w, int seq_len, long HW, const float* shift, float* mean_out,
                               float* std_out, void* stream);
int rdmi_aligner_merge_partial_window_moments(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                              const float* const* t, const int* n, const int* stride,
                                              const int* start_step, const int* k0, const int* nloc, const int* w,
                                              int seq_len, int f0, int nf, long HW, const float* shift,
                                              double* mom_out, void* stream);
int rdmi_aligner_merge_finish_pieces_moments(int n_dil, const int* n, const int* stride, const int* start_step,
                                             const int* w, int seq_len, int f0, int nf, long HW, int npieces,
                                             const int* piece_f0, const int* piece_nf, const double* recv,
                                             float* mean_out, float* std_out, void* stream);
/* In place: x = (x / (mx − mn)) · 2 with mn, mx read from the device — rdmi_renormalize_f32 without its
 * offsets: a spread of the merged map in the units of the renormalised one (since rdmi_version 6). */
int rdmi_scale_spread_f32(float* x, long n, const float* minmax, void* stream);

/* Median merge (since rdmi_version 7): the per-pixel median of a frame's covering terms in place of their
 * mean, and optionally their median absolute deviation (MAD) as the spread.
 *   Terms.   The covering terms of frame f and pixel p are a_1 … a_c, the f32 values rdmi_aligner_merge_moments
 *            forms in each x_f32 mode (0 / 1 / 2).  The coverage rule, the start steps and the layout checks
 *            before any launch are those of rdmi_aligner_merge_moments; Σ w_d ≤ 64, so c ≤ 64.
 *   Median.  The terms sorted ascending.  c odd: the middle term.  c even:
 *            (float)(((double)lo + (double)hi) * 0.5) of the two middle terms.  c = 0: 0.
 *   MAD.     d_i = fabsf(a_i − med), one f32 subtraction; MAD is the median of the d_i by the same rule, 0 for
 *            c ≤ 1.  It is the raw MAD: no 1.4826 factor is applied.
 *   Inputs are finite: NaN and the sign of a zero are not part of the contract.  The result depends only on
 *   the multiset of terms, never on their order.
 * rdmi_aligner_merge_median: the fused single-GPU form, one pass over the snippets → med_out [seq_len][HW]
 * f32 and, unless NULL, mad_out [seq_len][HW] f32.  With HW % 4 == 0, every base pointer 16-byte aligned and
 * at most 16 terms on any frame a lane takes 4 consecutive pixels, otherwise one.  A null med_out → RDMI_E_ARG.
 * Sharded form.  rdmi_aligner_merge_partial_window_terms writes the covering terms of this rank's snippets
 * (k0 / nloc as rdmi_aligner_merge_partial_window_moments) unreduced: those of frame f0 + i go to rows
 * row_off[i] … row_off[i + 1] − 1 of terms_out [rows][HW] f32 in the merge's (d ascending, j descending)
 * order.  row_off [nf + 1] lives on the device; the library recounts the rows on the host from the index map
 * and returns RDMI_E_ARG when `rows` differs; the kernel never writes more than row_off[i + 1] − row_off[i] rows
 * for a frame, nor beyond `rows`.  rows = 0 launches nothing.
 * rdmi_aligner_median_rows: frame i selects over rows row_idx[frame_off[i] … frame_off[i + 1]) of `rows`
 * [n_rows][HW] f32 (frame_off [nf + 1] and row_idx on the device) → med_out [nf][HW] and, unless NULL, mad_out.
 * The count is clamped to max_count (1 … 64, else RDMI_E_ARG), indices outside [0, n_rows) are skipped, a
 * frame with no rows gives 0; nf < 0 → RDMI_E_ARG; nf = 0 launches nothing and needs no outputs. */
int rdmi_aligner_merge_median(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                              const float* const* t, const int* n, const int* stride, const int* start_step,
                              const int* w, int seq_len, long HW, const float* shift, float* med_out,
                              float* mad_out, void* stream);
int rdmi_aligner_merge_partial_window_terms(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                            const float* const* t, const int* n, const int* stride,
                                            const int* start_step, const int* k0, const int* nloc, const int* w,
                                            int seq_len, int f0, int nf, long HW, const float* shift,
                                            const int* row_off, long rows, float* terms_out, void* stream);
int rdmi_aligner_median_rows(const float* rows, long n_rows, const int* frame_off, const int* row_idx, int nf,
                             long HW, int max_count, float* med_out, float* mad_out, void* stream);

/* Single-head flash attention for head dim 512 (f16): the VAE mid-block attention
 * (unet_2d_blocks.py:680-697 through AttnProcessor2_0's 4-D path, attention_processor.py:2172-2276 —
 * one head, d = C = 512) as one pass over K / Vᵀ instead of f32 scores → softmax → PV.
 * q [B][Sq][512] (row stride q_ld), k [B][Sk][512] (k_ld), vt = Vᵀ [B][512][Skp] (row stride vt_ld ≥
 * Skp, Skp = Sk rounded up to 32, columns Sk..Skp-1 zero), o [B][Sq][512] (o_ld); batch strides in
 * elements; o = softmax(q kᵀ · scale) v with f32 accumulation and f32 softmax statistics.
 * flags: int workspace of B·ceil(Sq / 128) entries (no initialisation needed) enabling the
 * 32-query-per-wave pass with a fixed running max and a fix-up pass over the blocks it flags; NULL
 * runs the 16-query kernel (running max with rescale) alone.  Same result either way. */
int rdmi_attention_d512(const void* q, const void* k, const void* vt, void* o, int B, int Sq, int Sk, int Skp,
                        long q_ld, long k_ld, long vt_ld, long o_ld, long q_bs, long k_bs, long vt_bs, long o_bs,
                        float scale, int* flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * Frame ingest / resize.  Replaces load_video_frames' per-frame resize_max_res + normalisation
 * (rollingdepth/video_io.py:38-67, 104-123: torchvision resize(antialias=True) of the decoded
 * float frame, then (x / 255)·2 − 1) and __call__'s restore_res resizes
 * (rollingdepth_pipeline.py:155-173).  x element (n, c, y, x) at x + n·sn + c·sc + y·sy + x·sx
 * (elements) of dtype RDMI_U8 (decoded rgb24 frames, e.g. sn = H·W·3, sc = 1, sy = W·3, sx = 3) or
 * RDMI_F32; y f32 [N, C, Ho, Wo] contiguous.  mode RDMI_RESIZE_*: the antialiased separable
 * filter of F.interpolate(antialias=True) for BILINEAR / BICUBIC (width pass, then height pass;
 * a dimension whose size does not change is not resampled), ATen nearest indexing for NEAREST.
 * normalize != 0: y = (v / 255)·2 − 1.  Downscale factor ≤ 9 (bicubic ≤ 4.5).  workspace ≥
 * rdmi_resize_workspace(...) bytes (f32 intermediate when both dimensions change).
 */
size_t rdmi_resize_workspace(int N, int C, int H, int W, int Ho, int Wo);
int rdmi_resize(const void* x, int x_dtype, long sn, long sc, long sy, long sx, int N, int C, int H, int W, int Ho,
                int Wo, int mode, int normalize, float* y, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * Depth metrics (since rdmi_version 5): affine-invariant evaluation of a depth video against a target —
 * the least-squares scale and shift per video or per frame, then AbsRel, SqRel, MAE, RMSE and δ < 1.25ᵏ
 * on the valid pixels.  The reference ships evaluation split lists (data_split/) and no evaluation code;
 * this is the protocol its paper reports.
 *
 * pred, target [N][P] contiguous, each RDMI_F16 or RDMI_F32 (any element-aligned pointer, any P ≥ 1);
 * mask [N][P] u8 or NULL.  A pixel is VALID when the mask is absent or ≠ 0 there, pred and target are
 * finite, and lo < target < hi (hi may be +inf).  All arithmetic is f64, in which the product of two
 * f16 / f32 values is exact.  workspace ≥ rdmi_depth_metrics_workspace(N, P) doubles, a function of N and P
 * alone; the three calls share it and run in stream order: moments → fit → errors.
 *
 * The summation order is fixed by P alone: a grid of (blocks per frame, N) workgroups whose blocks per
 * frame depend only on P, a fixed assignment of a frame's pixels to lanes counted from the frame's first
 * element, a cross-lane butterfly, the waves of a workgroup in wave order, the workgroups of a frame in
 * block order, and no atomics.  So the sums do not depend on the device, on N, on the other frames, or
 * on the alignment of the buffers (a frame whose base is not 16-byte aligned is read element by element
 * in the same assignment instead of with 16-byte loads): repeated calls, and a frame evaluated alone or
 * inside a video, give the same bits.  N ≤ 65535 (RDMI_E_UNSUPPORTED beyond).
 *
 * RDMI_E_ARG before any launch: a null pred / target / workspace / output, N or P < 1, a dtype other than
 * RDMI_F16 / RDMI_F32, an unknown mode, lo ≥ hi, clip_lo > clip_hi (a NaN bound fails both tests).
 */
#define RDMI_FIT_NONE 0  /* (s, t) = (1, 0) */
#define RDMI_FIT_FRAME 1 /* one fit per frame */
#define RDMI_FIT_VIDEO 2 /* one fit for all N frames, written into every row */
long rdmi_depth_metrics_workspace(int N, long P);
/* Per workgroup, the six sums n, Σp, Σg, Σp², Σpg, Σg² over its valid pixels → workspace. */
int rdmi_depth_moments(const void* pred, int pred_dtype, const void* target, int target_dtype,
                       const unsigned char* mask, int N, long P, float lo, float hi, double* workspace, void* stream);
/* One workgroup.  moments [N][6] (out) = each frame's workspace rows added in block order; st [N][2] (out)
 * = (s, t) minimising Σ (s·p + t − g)² over the valid pixels: det = n·Σp² − (Σp)², s = (n·Σpg − Σp·Σg) / det,
 * t = (Σp²·Σg − Σp·Σpg) / det.  RDMI_FIT_FRAME solves per frame; RDMI_FIT_VIDEO adds the frames' moments in
 * frame order and writes the one solution into every row; n < 2 or det ≤ 0 (of the frame, or in video mode
 * of the video) gives (NaN, NaN).  RDMI_FIT_NONE writes (1, 0) and needs no moments pass: workspace and
 * moments may then both be NULL. */
int rdmi_depth_fit(const double* workspace, int N, long P, int mode, double* moments, double* st, void* stream);
/* With a = fma(s, p, t) — ONE rounding of s·p + t, which a check against this call has to reproduce —
 * clamped to [clip_lo, clip_hi] (−inf, +inf: no clip; the target is never clipped), sums [N][8] (out) = per
 * frame over the valid pixels: n, Σ|a − g|, Σ|a − g|/g, Σ(a − g)², Σ(a − g)²/g (accumulated as
 * |a − g| · (|a − g|/g)), and the counts of max(a/g, g/a) < 1.25, < 1.25², < 1.25³ (decided as
 * max(a, g) < c·min(a, g); a ≤ 0 or g ≤ 0 counts as above every threshold).  st [N][2] as written by rdmi_depth_fit; a frame
 * whose s or t is NaN contributes nothing: its row is zero, n included.  With lo < 0 a valid target may be
 * ≤ 0 and the two relative sums are then not meaningful (inf / NaN); the others are. */
int rdmi_depth_errors(const void* pred, int pred_dtype, const void* target, int target_dtype,
                      const unsigned char* mask, int N, long P, float lo, float hi, const double* st, float clip_lo,
                      float clip_hi, double* workspace, double* sums, void* stream);

/* Alignment space (since rdmi_version 8): the fit taken against φ(target) and the aligned value brought back to
 * depth through φ⁻¹ — the protocol for ground truth stored as disparity and for predictors that are affine in
 * disparity or in log-depth.  φ(g) = g, 1 / g, ln g and φ⁻¹(d) = d, 1 / d, exp d, all in f64 (1 / x the IEEE
 * division).  An unknown space → RDMI_E_ARG before any launch; RDMI_SPACE_DEPTH launches exactly what the calls
 * above launch. */
#define RDMI_SPACE_DEPTH 0
#define RDMI_SPACE_DISPARITY 1
#define RDMI_SPACE_LOG 2
/* rdmi_depth_moments with the six moments taken of (p, φ(g)): n, Σp, Σφ, Σp², Σpφ, Σφ².  Outside RDMI_SPACE_DEPTH a
 * valid pixel also needs g > 0 (it matters when lo < 0), and p·φ and φ² are rounded products.  rdmi_depth_fit reads
 * the workspace as it is; its (s, t) then live in the fit space. */
int rdmi_depth_moments_space(const void* pred, int pred_dtype, const void* target, int target_dtype,
                             const unsigned char* mask, int N, long P, float lo, float hi, int space,
                             double* workspace, void* stream);
/* rdmi_depth_errors with a = φ⁻¹(d), d = fma(s, p, t) (one rounding, as above), then clamped to [clip_lo, clip_hi];
 * the same eight sums against g, in depth; validity as in rdmi_depth_moments_space.  RDMI_SPACE_DISPARITY: d ≤ 0 has
 * no finite depth and gives a = +inf, which the clamp brings to clip_hi.  With clip_hi = +inf such a pixel stays
 * in n, counts as above every δ threshold, and the four error sums become inf: name a depth cap. */
int rdmi_depth_errors_space(const void* pred, int pred_dtype, const void* target, int target_dtype,
                            const unsigned char* mask, int N, long P, float lo, float hi, const double* st, int space,
                            float clip_lo, float clip_hi, double* workspace, double* sums, void* stream);

/* Temporal consistency (since rdmi_version 8): pair i = 0 … N − k − 1 compares frame f = i with frame f' = i + k
 * (k = frame_step ≥ 1) of pred / target [N][H][W]; target may be NULL (target_dtype is then ignored).
 *
 * a(frame, pixel) = φ⁻¹(fma(s, p, t)) clamped to [clip_lo, clip_hi], with that frame's own row of st [N][2]
 * (rdmi_depth_fit's output for the fit of `space`).  A pixel of a frame is valid by the rule of
 * rdmi_depth_errors_space; without a target only the mask and the finiteness of pred count, and lo / hi are
 * ignored.  A pixel of frame f enters pair i when it is valid, pair_mask [N − k][H·W] (u8 or NULL) is ≠ 0 there,
 * and its sample in f' exists:
 *   flow == NULL: the same pixel of f', which must be valid in f';
 *   flow [N − k][H][W][2] = (dx, dy) in pixels, f32: X = x + (double)dx, Y = y + (double)dy, x0 = floor(X),
 *     y0 = floor(Y), wx = X − x0, wy = Y − y0; the taps (y0 + i, x0 + j) carry the weights
 *     (1 − wy | wy)·(1 − wx | wx).  A tap of weight exactly 0 is neither read nor required; every other tap must lie
 *     inside the frame and be valid in f', else the pixel is left out, as it is for a non-finite dx or dy.  No
 *     address is formed from a tap outside the frame.  a' = (1 − wy)·((1 − wx)·a₀₀ + wx·a₀₁) + wy·((1 − wx)·a₁₀ +
 *     wx·a₁₁) of the taps' aligned, clamped values, each operation rounded once, terms of weight 0 left out: a
 *     single tap of weight 1 gives a' = a_tap exactly.  g' is the same formula on the taps' targets.
 * With Δa = a' − a and Δg = g' − g, sums [N − k][8] (out) = n, Σ|Δa|, ΣΔa², Σ|Δa − Δg|, Σ(Δa − Δg)², Σ|Δg|, ΣΔg²,
 * ΣΔa·Δg per pair (the last five 0 without a target).  A pair one of whose two st rows holds a NaN contributes
 * nothing: its row is zero, n included.
 *
 * workspace ≥ rdmi_depth_metrics_workspace(N − k, H·W) doubles.  The tiling, the lane assignment over frame f and
 * the two-stage reduction are those of the passes above (grid (blocks per frame, N − k), no atomics), so the same
 * inputs give the same bits on every call, for a pair evaluated alone or inside a longer video, and for
 * 16-byte-aligned or unaligned bases.  Frame f is read with 16-byte loads, the taps of f' with scalar loads.
 *
 * RDMI_E_ARG before any launch: a null pred / st / workspace / sums, N < 2, H or W < 1, frame_step < 1 or ≥ N, a
 * dtype other than RDMI_F16 / RDMI_F32, an unknown space, lo ≥ hi with a target, clip_lo > clip_hi (a NaN bound
 * fails both tests).  N − frame_step ≤ 65535 (RDMI_E_UNSUPPORTED beyond). */
int rdmi_depth_temporal(const void* pred, int pred_dtype, const void* target, int target_dtype,
                        const unsigned char* mask, const float* flow, const unsigned char* pair_mask, int N, int H,
                        int W, int frame_step, float lo, float hi, const double* st, int space, float clip_lo,
                        float clip_hi, double* workspace, double* sums, void* stream);

/* ---------------------------------------------------------------------------------------
 * Exact order statistics (since rdmi_version 9): the value of a given rank among the elements of an f16 / f32
 * buffer, by a most-significant-digit radix select that reads the data rdmi_select_passes() times, sorts nothing
 * and never waits on the host.  The robust range of the depth pipeline's renormalisation (percentiles in place of
 * min / max; the reference has only the latter, rollingdepth_pipeline.py:316-318) and of the colouriser.
 *
 * x [n] f32 (x_f32 = 1) or f16 (0, widened exactly), any element-aligned pointer: elements before the first
 * 16-byte boundary and after the last whole vector are read singly, the rest with 16-byte loads.  mask [n] u8 or
 * NULL, one byte per element, ≠ 0 = keep.  NaNs are skipped like masked-out elements; −0 counts as +0; ±inf are
 * ordered like any value.  For a fraction q in [0, 1] and cnt counted values the result is the data value of
 * 0-based rank floor(q · (double)(cnt − 1)) — no interpolation; numpy's method="lower" whenever both rank formulas
 * are exact — and NaN when cnt = 0.  Up to RDMI_SELECT_MAX quantiles are found together, so each pass reads the data
 * once for all of them.  Key, digits, rank rule and the histogram walk: csrc/select_key.h.  All counts are
 * integers (LDS atomics per wave, one 64-bit global atomic add per workgroup and non-empty bin), so the results
 * are bitwise reproducible, on one device or summed over many.
 *
 * rdmi_select_hist: pass `pass` (0 … rdmi_select_passes() − 1) of the counting.  For quantile j < k it ADDS to
 *   hist[j][rdmi_select_bins()] (64-bit, zeroed by the caller) the counts, per value of the pass's key digit, of
 *   the kept elements whose higher digits equal quantile j's prefix in `state`; pass 0 counts every kept element
 *   and does not read `state`.  Histograms of several buffers (ranks, chunks) may be added before the pick.
 * rdmi_select_pick: one small launch.  Pass 0 takes cnt = Σ hist[0] and turns each q[j] (f64, device memory)
 *   into a rank; every pass finds the bin holding quantile j's remaining rank, extends its prefix in `state` and
 *   keeps the rank inside the bin; the last pass writes the values to out[k] (f32).  `state`: rdmi_select_state_bytes()
 *   bytes of device memory, 8-byte aligned, written by pass 0 (no initialisation needed).
 * rdmi_quantiles: the single-device chain zero, hist, pick, hist, pick … on one stream; workspace ≥
 *   rdmi_quantiles_workspace() bytes, 8-byte aligned (RDMI_E_ALIGN otherwise), no initialisation needed.
 * RDMI_E_ARG before any launch: a null x / state / hist / q / out / workspace, n ≤ 0, k outside
 * 1 … RDMI_SELECT_MAX, pass outside its range.  n ≥ 2^42 → RDMI_E_UNSUPPORTED. */
#define RDMI_SELECT_MAX 4
int rdmi_select_bins(void);
int rdmi_select_passes(void);
long rdmi_select_state_bytes(void);
long rdmi_quantiles_workspace(void);
int rdmi_select_hist(const void* x, int x_f32, const unsigned char* mask, long n, const void* state, int pass, int k,
                     long long* hist, void* stream);
int rdmi_select_pick(const long long* hist, const double* q, int pass, int k, void* state, float* out, void* stream);
int rdmi_quantiles(const void* x, int x_f32, const unsigned char* mask, long n, const double* q, int k, float* out,
                   void* workspace, void* stream);
/* In place: rdmi_renormalize_f32's arithmetic in its order (v = x − lo; v = v / (hi − lo); v·2 − 1) with
 * lohi = {lo, hi} read from the device, then clamped to [−1, 1] (a NaN stays NaN).  With lohi = the buffer's
 * {min, max} the clamp never fires and the result is rdmi_renormalize_f32's, bitwise.  hi = lo divides by zero:
 * elements equal to lo become NaN, the others ±1. */
int rdmi_renormalize_clip_f32(float* x, long n, const float* lohi, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optical flow (since rdmi_version 10): a classical, deterministic, dense pyramidal Lucas–Kanade estimator with
 * template gradients, and a forward–backward consistency check — the flow and the occlusion mask that
 * rdmi_depth_temporal's `flow` and `pair_mask` arguments were made for, from nothing but the RGB frames.  An
 * evaluation instrument: exact to the specification below, bit for bit reproducible, no learned part.  The
 * reference has no counterpart.  All arithmetic is f32, each operation rounded once or contracted to an fma.
 *
 * Luma.  Y = 0.299 R + 0.587 G + 0.114 B of frames given by a base pointer, a dtype (RDMI_F16, RDMI_F32, RDMI_U8) and
 *   four ELEMENT strides (frame, channel, row, column): [N, 3, H, W] floats, [N, H, W, 3] bytes and any strided or
 *   offset view of either are the same call.  Any affine range of the values gives the same flow (up to the 1e-12
 *   below).
 * Pyramid.  Level 0 is the luma; level l + 1 has ⌈H_l / 2⌉ × ⌈W_l / 2⌉ pixels, each ¼ · ((a + b) + (c + d)) of the
 *   2 × 2 block at (2y, 2x), indices clamped to the image.  The level rule: with s = 4 · (2r + 1), level l exists
 *   while l < 5 and (l = 0 or min(H_l, W_l) ≥ s); rdmi_flow_levels clamps a request of `levels` ≥ 1 to that count,
 *   ≤ 0 asks for it.  The other calls take 1 … RDMI_FLOW_MAX_LEVELS levels as given (a level deeper than the rule's
 *   only has more truncated windows) and read ≤ 0 (rdmi_flow_estimate, rdmi_flow_workspace) as the rule's count;
 *   the Python surface clamps a caller's request by the rule first.  pyr holds the levels one after the other: level l is [N][H_l][W_l] at the offset Σ_{j<l} N·H_j·W_j floats.
 * One level, pixel p = (x, y), radius r, window = the (2r + 1)² taps q = p + (i, j), |i|, |j| ≤ r, in row-major
 *   order (j outer), of which only those inside the image count:
 *     Ix(q) = ½ · (I0(qx + 1, qy) − I0(qx − 1, qy)), Iy alike, neighbour indices clamped to the image;
 *     Axx = Σ Ix², Axy = Σ Ix·Iy, Ayy = Σ Iy²;  λ = damping · (½ · (Axx + Ayy)) + 1e-12;
 *     a11 = Axx + λ, a22 = Ayy + λ, det = a11·a22 − Axy²;
 *   u(p) starts at 0 on the coarsest level and else at 2 · the coarse flow sampled bilinearly at
 *   ((x + ½)/2 − ½, (y + ½)/2 − ½), clamped to the coarse image; then `iterations` times
 *     b = Σ_q ∇I0(q) · (I1(q + u(p)) − I0(q)), with X = min(max(qx + ux, 0), W − 1), Y alike, x0 = ⌊X⌋, wx = X − x0,
 *       x1 = min(x0 + 1, W − 1), and I1(X, Y) = (1 − wy)·((1 − wx)·I00 + wx·I01) + wy·((1 − wx)·I10 + wx·I11);
 *     du = (−(a22·bx − Axy·by) / det, −(a11·by − Axy·bx) / det); where |du| > 1, du ← du / |du|;  u ← u + du.
 *   max / min return the other operand for a NaN, so no address is formed outside the image whatever the frames
 *   hold.  The flow of p moves the whole window of p: a pixel never reads a neighbour's flow within a level, its
 *   sums run in one lane in the fixed order above, and nothing is atomic — the same frames give the same bits,
 *   for a pair alone or in a batch, forward or as the backward flow of the reversed video.
 * Flow.  f32 [pairs][H][W][2] = (dx, dy) in pixels from frame i to frame i + k, rdmi_depth_temporal's convention.
 * Forward–backward check.  valid [pairs][H][W] (u8, 1 / 0): with X = x + uf.x, Y = y + uf.y, pixel p is valid iff
 *   0 ≤ X ≤ W − 1 and 0 ≤ Y ≤ H − 1 and, for ub = the backward flow sampled bilinearly at (X, Y) (formula above),
 *   |uf + ub|² ≤ α · (|uf|² + |ub|²) + β.  A NaN anywhere fails the tests: invalid.
 *
 * rdmi_flow_levels: the level rule (host arithmetic only; 0 for H, W < 1 or r outside 1 … 7).
 * rdmi_flow_workspace: bytes rdmi_flow_estimate needs (0 for arguments it would refuse): the pyramid of all N
 *   frames and, per direction, the flows of the levels above 0.
 * rdmi_flow_pyramid: luma and every level of all N frames into pyr (f32, 4-byte aligned), 1 + (levels − 1) launches.
 * rdmi_flow_lk_level: one level, one direction, all pairs in ONE launch: pair i takes frame first0 + i of img
 *   [N][Hl][Wl] as I0 and frame first1 + i as I1 (forward: 0 and k; backward: k and 0), starts from `coarse`
 *   [pairs][Hc][Wc][2] (NULL: zero; else Hc = ⌈Hl/2⌉, Wc = ⌈Wl/2⌉ is required) and writes flow [pairs][Hl][Wl][2].
 *   A workgroup owns a 32 × 8 pixel tile of one pair, stages I0 with an r + 1 halo in LDS, derives Ix, Iy there,
 *   and each lane then runs all iterations in registers; I1 is read through the caches.
 * rdmi_flow_fb_check: the check above, one launch.
 * rdmi_flow_estimate: pyramid, then per level from the coarsest the forward and (backward ≠ 0) the backward launch,
 *   then the check, on one stream.  flow_bwd and valid are written only when backward ≠ 0.
 * RDMI_E_ARG before any launch: a null frames / pyr / img / flow / fwd / bwd / valid / workspace (flow_bwd and valid
 *   only when backward ≠ 0), N < 1 (rdmi_flow_estimate: N < 2), H, W, pairs or iterations < 1, frame_step < 1 or ≥ N,
 *   first0 / first1 < 0 or + pairs > N, r outside 1 … 7, levels outside 1 … RDMI_FLOW_MAX_LEVELS (pyramid; estimate: above it), a dtype
 *   outside the three, a coarse size other than the halved one, damping < 0 or NaN, α or β < 0 or NaN.
 * RDMI_E_ALIGN: pyr / img not 4-byte, flow / coarse / fwd / bwd not 8-byte, workspace not 16-byte aligned.
 * RDMI_E_UNSUPPORTED: H·W > 2^30 or more than 65535 pairs.  Frame bases are 64-bit: N·H·W is not limited. */
#define RDMI_FLOW_MAX_LEVELS 5
#define RDMI_FLOW_MAX_RADIUS 7
int rdmi_flow_levels(int H, int W, int radius, int levels);
long rdmi_flow_workspace(int N, int H, int W, int frame_step, int radius, int levels, int backward);
int rdmi_flow_pyramid(const void* frames, int dtype, long stride_n, long stride_c, long stride_y, long stride_x, int N,
                      int H, int W, int levels, float* pyr, void* stream);
int rdmi_flow_lk_level(const float* img, int N, int Hl, int Wl, int first0, int first1, int pairs,
                       const float* coarse, int Hc, int Wc, float* flow, int radius, int iterations, float damping,
                       void* stream);
int rdmi_flow_fb_check(const float* fwd, const float* bwd, int pairs, int H, int W, float alpha, float beta,
                       unsigned char* valid, void* stream);
int rdmi_flow_estimate(const void* frames, int dtype, long stride_n, long stride_c, long stride_y, long stride_x,
                       int N, int H, int W, int frame_step, int levels, int radius, int iterations, float damping,
                       int backward, float alpha, float beta, float* flow, float* flow_bwd, unsigned char* valid,
                       void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * Guided upsampling (since rdmi_version 11): joint bilateral upsampling (Kopf et al. 2007) of low-resolution maps
 * along a full-resolution guide image — the edge-aware alternative to rdmi_resize for restore_res: a depth
 * discontinuity lands where the image edge is instead of becoming a ramp.  Deterministic, no learned part; the
 * reference has no counterpart.
 *
 * values [N][C][h][w] contiguous, RDMI_F16 (widened exactly) or RDMI_F32, C = 1 … 4 channels that share one set of
 *   weights.  guide_lo [N][3][h][w] f32 contiguous: the guide at the values' resolution.  guide_hi: element
 *   (n, c, Y, X) at guide_hi + n·sn + c·sc + Y·sy + X·sx (elements; rdmi_resize's addressing, so rgb24 frames
 *   [N][H][W][3] and planar f32 are the same call) of dtype RDMI_U8 or RDMI_F32; G = (float)element · guide_scale,
 *   one rounding (1/255 for u8 frames against a guide_lo in [0, 1]).  out [N][C][H][W] f32 contiguous.
 * Output pixel (Y, X) of frame n.  All arithmetic is f32; every operation below is rounded once, and only where an
 *   fma is written are a product and a sum contracted.
 *     yl = ((float)Y + 0.5)·(h / H) − 0.5 with h / H the f32 quotient of the two sizes converted to f32, product and
 *       difference rounded separately; xl alike with w / W.  y0 = ⌊yl⌋, x0 = ⌊xl⌋.
 *     Taps q = (qy, qx), qy = y0 − r + 1 … y0 + r (outer), qx = x0 − r + 1 … x0 + r (inner), both ascending: (2r)² taps
 *       in row-major order.  A tap outside the h × w image is skipped; at least one always lies inside.
 *     cs = log₂e / (2·σs²) and cr = log₂e / (2·σr²), each formed in f64 and rounded to f32 once (the exponent is
 *       kept in base 2: the weight below is 2^−(e − m), which is exp(−(e − m)) of the natural-base exponent).
 *     e_q = min(fma(D, cr, (qy − yl)²·cs + (qx − xl)²·cs), FLT_MAX), D = fma(d₂, d₂, fma(d₁, d₁, d₀·d₀)),
 *       d_c = G[n, c, Y, X] − guide_lo[n, c, q]; (qy − yl)²·cs is ((qy − yl)·(qy − yl))·cs.  The min, which returns
 *       FLT_MAX for a NaN, only matters for a σ so small that cs or cr overflows: the exponents stay finite.
 *     m = min_q e_q over the taps inside the image; w_q = exp2(m − e_q), the hardware v_exp_f32 (1 ulp).
 *     out[n, k, Y, X] = Σ_q w_q·v[n, k, q] / Σ_q w_q, evaluated as v_b + (Σ_q w_q·(v_q − v_b)) / (Σ_q w_q) with v_b the
 *       value at the base tap (min(max(y0, 0), h − 1), min(max(x0, 0), w − 1)), which is always one of the taps: both
 *       sums start at +0 and run over the taps in the order above, the numerator as acc = fma(w_q, v_q − v_b, acc);
 *       the quotient is the IEEE division.  So a constant plane comes out exactly, and the rounding errors scale
 *       with the range of the values over the taps, not with |v|.
 *   The largest weight is exactly 1, so Σw ≥ 1 and no σ gives 0/0.  Inputs are finite: NaN is not part of the
 *   contract.
 * One launch: a workgroup owns a 16 × 64 tile of output pixels of one frame and stages the tile's low-resolution
 *   footprint (at most (16 + 2r + 1) × (64 + 2r + 1) pixels since h ≤ H and w ≤ W) in LDS.  No atomics, no workspace,
 *   no allocation, nothing synchronises: graph-capturable like every other entry point.  A pixel's arithmetic is that
 *   of one lane in the fixed order above and reads that frame's inputs only, element by element (there is no
 *   wide-load path): the bits do not depend on N, on the other frames, on C (a channel computed alone equals the same
 *   channel computed among four), on the pointers' alignment, or on the call.
 * RDMI_E_ARG before any launch: a null values / guide_lo / guide_hi / out, N, h, w, H or W < 1, C outside 1 … 4,
 *   radius outside 1 … RDMI_JBU_MAX_RADIUS, a σ that is ≤ 0 or NaN, a values dtype other than RDMI_F16 / RDMI_F32, a
 *   guide dtype other than RDMI_U8 / RDMI_F32.
 * RDMI_E_UNSUPPORTED (rdmi_last_error says which): H < h or W < w — an upsampler; equal sizes are allowed and make it
 *   a joint bilateral filter — or more than 2^31 − 1 tiles in all N frames. */
#define RDMI_JBU_MAX_RADIUS 3
int rdmi_joint_bilateral_upsample(const void* values, int values_dtype, const float* guide_lo, const void* guide_hi,
                                  int guide_dtype, long sn, long sc, long sy, long sx, float guide_scale, int N, int C,
                                  int h, int w, int H, int W, int radius, float sigma_spatial, float sigma_range,
                                  float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Depth boundaries (since rdmi_version 12): precision / recall counts of the occluding contours of an aligned
 * depth video against those of a target — after Depth Pro's scale-invariant boundary F1, restated from its
 * definition.  A ramp two pixels wide costs almost nothing in AbsRel or δ₁; it costs recall here.  The reference has
 * no counterpart.
 *
 * pred, target [N][H][W] contiguous, each RDMI_F16 or RDMI_F32 (any element-aligned pointer); mask [N][H][W] u8 or
 * NULL; st [N][2] f64 in device memory as written by rdmi_depth_fit for the fit of `space`.
 * Aligned prediction.  a = φ⁻¹(fma(s, p, t)) clamped to [clip_lo, clip_hi] with the frame's own (s, t), exactly
 *   rdmi_depth_errors_space's value (clip bounds are doubles here); g is the target.
 * Valid pixel.  The rule of rdmi_depth_errors_space — mask absent or ≠ 0, p and g finite, lo < g < hi, g > 0 outside
 *   RDMI_SPACE_DEPTH, a frame whose s and t are not NaN — and in addition a finite and a > 0.
 * Pair.  Two valid pixels that are horizontal or vertical neighbours in one frame; nothing crosses a row end or a
 *   frame.  pairs [N][2] (out) = the frame's horizontal and vertical pairs.
 * Edge.  thresholds [M] (HOST memory, read before the launch): 1 … RDMI_BOUNDARY_MAX_THRESHOLDS finite values > 1,
 *   strictly rising.  Pixel i has an edge of map d in direction k — 0 R (x + 1), 1 L (x − 1), 2 D (y + 1), 3 U
 *   (y − 1) — at τ iff its neighbour j in that direction forms a pair with it and d(j) > τ·d(i): one f64 product,
 *   one comparison, no division; i is the near side.  The test is taken as written for every pair, also for a
 *   target ≤ 0 (possible with lo < 0 in RDMI_SPACE_DEPTH), where it no longer says anything about a ratio.
 * counts [N][M][4][3] (out, 64-bit) = per frame, threshold and direction: TP = #(edge of a and edge of g),
 *   NP = #edge of a, NG = #edge of g.  A frame without a fit has zero rows.
 * edges (NULL or out, u8 [N][H][W]) = for threshold edge_index: bits 0–3 the edge of a in R, L, D, U at this
 *   pixel, bits 4–7 the same for g; 0 for a pixel that is not valid.  Every byte is written, by plain stores.
 *
 * One launch reads the operands once for all thresholds and keeps 32-bit integer histograms in LDS; each workgroup
 * writes one row to workspace (≥ rdmi_depth_boundary_workspace(N, H, W, M) BYTES, 16-byte aligned, no
 * initialisation needed; 0 for arguments the call would refuse) and a second small launch adds a frame's rows in
 * 64-bit.  Integer addition is exact and order-free, so all outputs are bitwise reproducible and do not depend on
 * N, on the other frames or on the alignment of the buffers; a pixel's aligned value comes from one function
 * whichever pair reads it.  Nothing synchronises, allocates or uses floating-point atomics.
 *
 * RDMI_E_ARG before any launch: a null pred / target / st / thresholds / counts / pairs / workspace, N, H or W < 1,
 * a dtype other than RDMI_F16 / RDMI_F32, an unknown space, lo ≥ hi, clip_lo > clip_hi (a NaN bound fails both
 * tests), M outside 1 … RDMI_BOUNDARY_MAX_THRESHOLDS, a threshold that is not finite, not > 1 or not above the one
 * before it, edge_index outside 0 … M − 1 when edges is given.  RDMI_E_ALIGN: workspace not 16-byte aligned.
 * RDMI_E_UNSUPPORTED: N > 65535, or a frame of more than 2^31 − 256 eight-pixel × four-row tiles. */
#define RDMI_BOUNDARY_MAX_THRESHOLDS 16
long rdmi_depth_boundary_workspace(int N, int H, int W, int M);
int rdmi_depth_boundary(const void* pred, int pred_dtype, const void* target, int target_dtype,
                        const unsigned char* mask, int N, int H, int W, float lo, float hi, const double* st,
                        int space, double clip_lo, double clip_hi, const double* thresholds, int M, long long* counts,
                        long long* pairs, unsigned char* edges, int edge_index, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------
 * Temporal filter (since rdmi_version 13): a motion-compensated bilateral filter over time — each pixel of a depth
 * video is averaged with the depths its neighbouring frames hold where a given flow says the pixel went, with
 * weights that fall off with the frame distance and with the depth difference.  The flow and its occlusion mask are
 * operands (rdmi_flow_lk_level / rdmi_flow_fb_check produce them; any other source serves).  Deterministic, no
 * learned part; the reference has no counterpart.
 *
 * depth [N][H][W] contiguous, RDMI_F16 (widened exactly) or RDMI_F32: the whole video.  Output frames are
 *   i = f0 … f0 + n − 1 (0 ≤ f0, n ≥ 1, f0 + n ≤ N); out [n][H][W] f32.
 * Slots.  s = 0 … 2R − 1 stands for the frame offset k = −R, …, −1, +1, …, +R in that order (R = radius).
 *   flow [2R][n][H][W][2] f32: row i − f0 of slot s holds (dx, dy) in pixels from frame i to frame i + k at the
 *   pixels of frame i (rdmi_depth_temporal's convention).  valid [2R][n][H][W] u8, or NULL for all ones.  Row i − f0
 *   of slot s is never read when i + k lies outside [0, N).
 * Constants.  ct = log₂e / (2·σt²) and cd = log₂e / (2·σd²), each formed in f64 and rounded to f32 once (σt =
 *   sigma_time in frames, σd = sigma_depth in the units of depth; the exponent is kept in base 2).
 * Output pixel p = (x, y) of frame i.  All arithmetic is f32; every operation below is rounded once, and only where
 *   an fma is written are a product and a sum contracted.
 *     d0 = D_i(p).  If d0 is not finite, out = d0 and nothing else is read.
 *     acc = +0, wsum = +0; then for the slots in ascending order whose j = i + k lies in [0, N):
 *       1. skip if valid = 0;
 *       2. X = (float)x + dx, Y = (float)y + dy; skip unless 0 ≤ X ≤ W − 1 and 0 ≤ Y ≤ H − 1 — a NaN fails the test,
 *          so no address is ever formed from one;
 *       3. x0 = min((int)X, W − 1), x1 = min(x0 + 1, W − 1), wx = X − (float)x0; y0, y1, wy alike;
 *       4. with a00 = D_j(x0, y0), a01 = D_j(x1, y0), a10 = D_j(x0, y1), a11 = D_j(x1, y1):
 *          t0 = fma(wx, a01 − a00, a00), t1 = fma(wx, a11 − a10, a10), d_k = fma(wy, t1 − t0, t0) — the lerp form, not
 *          the (1 − w)·a + w·b of the flow check's bilerp: equal taps give exactly that value whatever wx and wy
 *          are, so a constant video comes out bit for bit;
 *       5. skip if d_k is not finite (a NaN or ∞ among the taps that the weights do not cancel);
 *       6. δ = d_k − d0; e = fma(δ·δ, cd, (float)(k·k)·ct); w = exp2(−e), the hardware v_exp_f32 (1 ulp);
 *       7. acc = fma(w, δ, acc); wsum = wsum + w.
 *     out = d0 + acc / (1 + wsum), the IEEE division: the frame's own weight is the 1, so no σ gives 0/0.
 *   Consequences: a constant video is reproduced exactly; N = 1, all-invalid neighbours and flows that all leave the
 *   frame are the identity, bitwise; the rounding errors scale with the spread of the taps around d0, not with |d|.
 *   Finite depths are expected to differ by less than FLT_MAX (δ finite).
 * One launch covers all n frames and all 2R neighbours: a workgroup owns a 32 × 8 pixel tile of one output frame
 *   (256 lanes, lanes along x), d0 is read once and out written once, the taps are element loads through the caches.
 *   No atomics, no workspace, no allocation, nothing synchronises: graph-capturable like every other entry point.
 *   Frame bases are 64-bit: N·H·W is not limited.  A pixel's result is one lane's chain in the fixed order above,
 *   element by element (there is no wide path over pixels): the bits do not depend on n, on f0 (given the same depth
 *   and the same rows of flow / valid), on the pointers' alignment, or on the call.
 * RDMI_E_ARG before any launch: a null depth / flow / out, N, H, W or n < 1, f0 < 0 or f0 + n > N, radius outside
 *   1 … RDMI_TFILTER_MAX_RADIUS, a depth dtype other than RDMI_F16 / RDMI_F32, a σ that is ≤ 0 or NaN or for which ct
 *   or cd is not finite and positive in f32 (σ below about 4.6e-20 or above about 3e22).
 * RDMI_E_ALIGN: flow not 8-byte aligned, or out not 4-byte aligned.
 * RDMI_E_UNSUPPORTED: H·W > 2^30, or more than 2^31 − 1 tiles in the n frames. */
#define RDMI_TFILTER_MAX_RADIUS 3
int rdmi_temporal_filter(const void* depth, int depth_dtype, int N, int H, int W, int f0, int n, int radius,
                         const float* flow, const unsigned char* valid, float sigma_time, float sigma_depth,
                         float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDMI_H */
