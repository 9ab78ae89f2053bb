/* mmgt_hip.h — C ABI of libmmgt_hip.so: the MI355X (gfx950) kernels behind MMGT's Stage-2 denoising path.
 *
 * This is the drop-in boundary.  The reference has no native layer at all: every call below replaces arithmetic that
 * the reference reaches through PyTorch / diffusers modules, cited per entry point (paths relative to the reference
 * checkout).  A maintainer binds these with ctypes; mmgt_amd/hip.py is exactly such a binding.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless stated; inputs are borrowed and never written; outputs are caller-owned.
 *  - `dtype` selects the storage type of activations and weights: MMGT_BF16 (product) or MMGT_F32 (the fp32-I/O parity
 *    mode of the same kernels).  Accumulation is always fp32.  Bias / norm affine / mask / scale vectors are fp32.
 *  - Activations are channels-last: an image tensor is (N, H, W, C) == a token matrix (N*H*W, C), row stride given.
 *  - `stream` is a hipStream_t (0 = default stream).  Calls only enqueue work; nothing synchronises, allocates or frees,
 *    so sequences of calls may be captured into a hipGraph.
 *  - Return 0 on success, non-zero on error with a message in mmgt_last_error() (thread-local).  Unsupported shapes are
 *    errors; there is no fallback path.
 *  - ONE DEVICE PER PROCESS, calls from one thread at a time: the library caches per-kernel launch state (the > 64 KB
 *    dynamic-LDS opt-in and the resident-workgroup count of each GEMM tile) for the device current at the first call.
 *    This is the deployment model of the path (one process per GPU); a process that switches devices must
 *    not reuse the library.
 */
#ifndef MMGT_HIP_H
#define MMGT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MMGT_F32 0
#define MMGT_BF16 1

#define MMGT_ACT_NONE 0
#define MMGT_ACT_GEGLU 1 /* weights packed per 64 rows as [32 h | 32 gate]; output has N/2 columns */
#define MMGT_ACT_SILU 2
#define MMGT_ACT_RELU 3
#define MMGT_ACT_QUICK_GELU 4 /* x * sigmoid(1.702 x): the CLIP vision tower's MLP (transformers activations.py) */
#define MMGT_ACT_GELU 5       /* exact-erf GELU: SMGA's feed-forward blocks (src/audio2pose_model/SMGA.py:92) */
#define MMGT_ACT_MISH 6       /* x * tanh(softplus(x)): SMGA's time MLP (src/audio2pose_model/model.py:370-374) */

int mmgt_abi_version(void);
const char* mmgt_last_error(void);
/* Benchmark-only knobs (A/B measurements and tests; the defaults are the product):
 *   "gemm_cfg" = 0 (heuristic tile choice) or 1, 3, 6, 9, 12, 16, 17, 19, 20 (force a GEMM / conv tile configuration; 19 = gemm16's 192 x 320 tile,
 *                20 = its 256 x 128 tile: measured slower than the 128 x 128 tile everywhere, kept for the record);
 *   "bm192"    = 1 (default) / 0: the 192-row gemm16 tile for shapes whose 256-row tile count leaves the last round of the grid half empty;
 *   "attn64"   = 1 (default) / 0: the 64-queries-per-wave spatial attention kernel at head_dim 40;
 *   "attn_nomax" = 1 (default) / 0: that kernel without the running maximum (the softmax reference stays what a row's first 32 keys set it to; a
 *                workgroup in which a denominator ends beyond 2^100 runs its tile loop again with the running maximum: csrc/attn64.hip);
 *   "attn80"   = 1 (default) / 0: head_dim 80 on the LDS-DMA-staged kernel of csrc/attn80.hip (0: attention.hip's register-staged kernel);
 *   "gn_slab"  = 1 (default) / 0: GroupNorm below the 64 x 64 level with the image x group slab in registers, one read of the tensor
 *                (0: the multi-pass kernels);
 *   "g16_stagger" = -1 (default: by shape) / 0 / n: every second CU's gemm16 workgroup starts n x 512 clocks late (short reductions with a
 *                residual epilogue: the chip is then not in the tile-end phase all at once); timing only, results are bitwise the same;
 *   "gn_rows"  = 0 (default: measured choice) or the GroupNorm rows per workgroup;
 *   "splitk"   = 1 (default) / 0: split-K of long reductions on grids of at most half a tile per CU (the 8x8-level convs);
 *   "ffn_dbg", "tleg_abl", "gnconv_abl", "rowgemm_dbg" 1 .. 4: timing ablations whose RESULTS ARE GARBAGE.  The product library does not
 *   contain them and refuses the keys with an error; they exist in libmmgt_hip_abl.so only (`make -C mmgt_amd/csrc abl`, -DMMGT_ABLATE),
 *   which the instruments under tools/ build and load explicitly (tools/abl_lib.py).
 *   "tailsplit" = 1 (default) / 0: convs whose tile count leaves the last round of the persistent grid half empty run that round's rows
 *               as a second launch with the reduction split in two (A/B switch).
 * One kernel per family ships: the measured-slower variants of earlier rounds (gemm16s / gemm16v, the phased and register-staged
 * head_dim-40 attention kernels, the producer / consumer FeedForward) are records under tools/micro/. */
int mmgt_tune(const char* key, int value);
/* Host-side switches kept in the same table (what mmgt_amd/unet3d.py, pipeline.py and smga.py consult; all default 1, 0 = the
 * unfused / stateless form, for same-box A/Bs): "fused_ff", "twin_attention", "shared_rows", "oz3", "rowgemm", "tleg", "up2" (the up-sampling convs in the four-phase form), "conv_out_taps" (conv_norm_out + SiLU + conv_out as a 36-column GEMM + a gather), "sc_cat" (conv_shortcut over [x | skip] as one two-source launch), "ffpo_cat" (ff2 + proj_out of a block as one two-source GEMM), "rconv" (a mask: 1 the 320-wide resnets, 2 the 640-wide, 4 the 1280-wide), "gnconv" (mmgt_amd/vae.py),
 * "zero_audio_skip", "window_state", "smga_graph".  mmgt_tune sets them, mmgt_tune_get reads them: one state describes a run. */
int mmgt_tune_get(const char* key, int* value);
/* Box calibration for bench.py's `box_calib` (csrc/calib.hip): a bare v_mfma_f32_16x16x32_bf16 loop on random operands, one wave per SIMD,
 * launched back to back for `warm_seconds` (0 .. 10); *mfma_mhz = the in-kernel clock of the last launch (delta s_memtime / delta
 * s_memrealtime, median over the workgroups), *mfma_tflops = the rate of the last batch of launches.  Measures the BOX (boxes differ by
 * several per cent in the clock they hold under load), not the product.  Host pointers; synchronises the stream. */
int mmgt_box_calib(float warm_seconds, float* mfma_mhz, float* mfma_tflops, void* stream);
/* Debug only (tools/trace_gemm16.py): p = device buffer of u64 [grid][32 tiles][2 wave groups][4] that gemm16's workgroups fill
 * with 100-MHz stamps at their tile phases; NULL (the default) switches the stamps off. */
void mmgt_gemm16_set_trace(void* p);
/* Debug only (tools/trace_ffn.py): u64 [workgroups][64] shader-clock stamps of mmgt_ff_fused's phases (wave 0); NULL = off. */
void mmgt_ffn_set_trace(void* p);

/* out[M,N] = epi(A[M,K] . W[N,K]^T):  v = acc + bias[n] + bias2[m / bias2_rows][n]; v = act(v);
 * v *= row_scale[m] * alpha; v += residual[m][n].   Optional batch (grid.z) with element strides bs*.
 * Replaces: nn.Linear / 1x1 nn.Conv2d / diffusers Attention.to_q,to_k,to_v,to_out / FeedForward(GEGLU) call sites
 * src/models/transformer_3d.py:176,253; src/models/attention.py:323-349,361,465,568-626,730-769;
 * src/models/motion_module.py:161,172,233,256; src/models/resnet.py:211-215,226,243; src/models/unet_3d.py:502. */
int mmgt_gemm(const void* A, long lda, const void* W, const float* bias, const float* bias2, int bias2_rows,
              const float* row_scale, float alpha, const void* residual, long ldr, void* out, long ldo, int M, int N,
              int K, int act, int batch, long bsA, long bsW, long bsR, long bsO, int dtype, void* stream);

/* The same with a second bias added AFTER the row scale:  v = (acc + bias[n]) * row_scale[m] * alpha + bias_post[n] +
 * residual[m][n].  Lets MM-HAA's  zero_conv_i(mask_i * to_out_i(a_i))  (attention.py:730-760: a 320x320 Linear, a per-token
 * mask multiply and a 1x1 conv per branch) run as ONE GEMM per branch on the host-merged weight W_z W_o: bias = W_z b_o,
 * row_scale = mask, alpha = motion_scale, bias_post = motion_scale * b_z. */
int mmgt_gemm_post(const void* A, long lda, const void* W, const float* bias, const float* row_scale, float alpha,
                   const float* bias_post, const void* residual, long ldr, void* out, long ldo, int M, int N, int K,
                   int dtype, void* stream);

/* 3x3 / pad 1 convolution on channels-last input as implicit GEMM.  x0 (NB,IH,IW,C0) and optional x1 (NB,IH,IW,C1) are
 * read as one (C0+C1)-channel tensor (the UNet skip concat, unet_3d_blocks.py:894,1057); `upsample` = the conv sees the
 * nearest-2x upsampled input (Upsample3D, resnet.py:70-88); stride 2 = Downsample3D (resnet.py:112-120).
 * stride -2 = stride 2 with the padding on the high side only (diffusers Downsample2D(padding=0): F.pad(x, (0,1,0,1)),
 * the AutoencoderKL encoder's downsampler).
 * upsample = 2: the same function as upsample = 1 from the FOUR-PHASE weight image [4][Cout][2][2][C0] (mmgt_amd/packing.py pack_conv3x3_up2): output
 * pixel (2 y + a, 2 x + b) reads the stored pixels (y + a - 1 .. y + a, x + b - 1 .. x + b) through the 3 x 3 taps summed per stored pixel -- four
 * 2 x 2 convs on the stored image (one per phase, grid.z), 16 instead of 36 multiply-adds per stored pixel and channel pair; bf16, one source,
 * bias only, Cout a multiple of 256 or 320 (the up-sampling convs of the UNet, the ReferenceNet and the VAE decoder).
 * Wp: [Cout][3][3][C0+C1].  out (NB,OH,OW,Cout) = act(conv + bias + bias2[pixel / bias2_rows]) + residual.
 * Replaces: InflatedConv3d (src/models/resnet.py:9-17) in ResnetBlock3D.conv1/conv2 (resnet.py:223,240), conv_in /
 * conv_out (unet_3d.py:517,620), PoseGuider convs (pose_guider.py:47-57), AutoencoderKL decoder convs (diffusers). */
int mmgt_conv3x3_nhwc(const void* x0, int C0, const void* x1, int C1, int NB, int IH, int IW, int stride, int upsample,
                      const void* Wp, const float* bias, const float* bias2, int bias2_rows, const void* residual,
                      void* out, int Cout, int act, int dtype, void* stream);

/* 1 x 1 conv over the channel concatenation of two channels-last tensors, out[p][o] = bias[o] + Wp[o] . [x0[p] | x1[p]] (+ residual[p][o]): the
 * resnets' conv_shortcut over [hidden | skip] (resnet.py:243-245; unet_3d_blocks.py:941-969 concatenates first) as one launch -- the conv gather's
 * two-source reduction with a single tap -- instead of two dense GEMMs chained through a residual.  bf16; `rows` pixels; C0, C1 multiples of 64, Cout a
 * multiple of 256 or 320; Wp [Cout][C0 + C1]; residual / out (rows, Cout). */
int mmgt_conv1x1_cat_nhwc(const void* x0, int C0, const void* x1, int C1, long rows, const void* Wp, const float* bias, const void* residual, void* out,
                          int Cout, int dtype, void* stream);

/* A 3 x 3 / pad 1 conv with FOUR output channels (conv_out, unet_3d.py:620) as a GEMM + this gather: Y (NB, H, W, ldY) bf16 holds, per pixel, the 36
 * products W[o][tap] . x[pixel] in column 4 tap + o (one GEMM over the pixel's channels for all nine taps: mmgt_rowgemm320 with norm = 3, the GroupNorm
 * tables + SiLU of conv_norm_out applied while the rows are loaded); out (NB, H, W, 8) bf16 = bias[o] + the sum over the taps of the NEIGHBOUR pixel's
 * product (out-of-image neighbours contribute nothing: the zero padding), channels 4 .. 7 zero. */
int mmgt_conv_taps_gather(const void* Y, int ldY, const float* bias, void* out, int NB, int H, int W, int dtype, void* stream);

/* GroupNorm over channels-last images, one statistic per (image, group), optional fused SiLU.
 * x,out (NB, HW, C) where C = C0 + C1 may be split over two sources (skip concat); workspace: NB*chunks*G*2 floats
 * with chunks = mmgt_groupnorm_chunks(HW).
 * Replaces: InflatedGroupNorm / nn.GroupNorm (+F.silu) at resnet.py:220-221,231,237; transformer_3d.py:174;
 * motion_module.py:156; unet_3d.py:618-619. */
int mmgt_groupnorm_chunks(int HW);
/* GroupNorm statistics only, as per-(image, channel) tables scale = rstd * gamma, shift = beta - mean * scale ([NB][C] fp32 each;
 * HW > 256): mmgt_rowgemm320(norm = 2) applies them while it loads x -- transformer_3d.py:174-188 (norm -> proj_in), motion_module.py:156-170. */
int mmgt_groupnorm_affine(const void* x, int C, const float* gamma, const float* beta, float* workspace, float* scale, float* shift,
                          int NB, int HW, int G, float eps, int dtype, void* stream);
/* ... of the channel concatenation x0 | x1 (a resnet's norm1 behind a skip connection: unet_3d_blocks.py:941-969; groups may straddle the seam);
 * x1 NULL / C1 0: one tensor. */
int mmgt_groupnorm_affine2(const void* x0, int C0, const void* x1, int C1, const float* gamma, const float* beta, float* workspace, float* scale,
                           float* shift, int NB, int HW, int G, float eps, int dtype, void* stream);
int mmgt_groupnorm_nhwc(const void* x0, int C0, const void* x1, int C1, const float* gamma, const float* beta, void* out,
                        float* workspace, int NB, int HW, int G, float eps, int silu, int dtype, void* stream);

/* LayerNorm over the last dimension of a (rows, C) token matrix, optional additive table pe[(row / pe_div) % pe_mod][C]
 * applied AFTER the affine transform (the temporal positional encoding enters q, k and v: motion_module.py:359-366).
 * With pe == NULL and pe_mod > 1, `beta` is itself a [pe_mod][C] table indexed the same way (the host folds
 * beta + pe once per model: one vector load per row less, 2x on the L0 temporal norms).
 * Replaces: nn.LayerNorm at attention.py:392-396,450-454,465,677-681,712-716,769; motion_module.py:244,256;
 * mutual_self_attention.py:122,195-199,210; audio_proj.py:119. */
int mmgt_layernorm(const void* x, long ldx, const float* gamma, const float* beta, float eps, const float* pe, int pe_div,
                   int pe_mod, void* out, long ldo, int rows, int C, int dtype, void* stream);

/* softmax(Q K^T * scale) V for `batch` x `heads` independent problems, flash style (scores never leave the chip).
 *   Q element (b, i, h, d) at q[(b / q_bdiv) * q_bs0 + (b % q_bdiv) * q_bs1 + i * q_ts + h * hd + d]; K, V, O likewise.
 *   Keys/values come from up to two segments: [K, V] with nk keys, then [K2, V2] with nk2 keys for batches
 *   b >= seg2_first_batch (the ReferenceNet feature bank that only the conditional CFG half attends to); segment 2
 *   uses batch index b / k2_bdiv2 with stride k2_bs.
 *   v_transposed = 1: V (and V2) are stored [b][h*hd + d][key] (key contiguous, row stride v_ts).
 * Replaces: diffusers Attention + AttnProcessor2_0 (F.scaled_dot_product_attention) at attention.py:323-349,568-626;
 * motion_module.py:377-383; and the bank concat + uncond recompute of mutual_self_attention.py:149-188. */
int mmgt_attention(const void* q, long q_bs0, long q_bs1, long q_ts, const void* k, long k_bs0, long k_bs1, long k_ts,
                   const void* v, long v_bs0, long v_bs1, long v_ts, void* o, long o_bs0, long o_bs1, long o_ts,
                   int bdiv, const void* k2, const void* v2, long k2_bs, long k2_ts, long v2_bs, long v2_ts, int k2_bdiv,
                   int nk2, int seg2_first_batch, int batch, int heads, int hd, int nq, int nk, float scale,
                   int v_transposed, int dtype, void* stream);

/* mmgt_attention with a per-row output multiplier per group of `os_heads` heads, applied in fp32 with the softmax normalisation:
 *   o[b][q][head] *= out_scale[(head / os_heads) * os_group_stride + b * nq + q]
 * Single key segment, row-major V, bdiv == 1.  MM-HAA (attention.py:730-760): the three masked audio cross-attentions write
 * mask_i * attn2_i(x, audio_i), so that  sum_i zero_conv_i(mask_i * to_out_i(.))  is ONE GEMM over the concatenated reduction. */
int mmgt_attention_scaled(const void* q, long q_bs0, long q_bs1, long q_ts, const void* k, long k_bs0, long k_bs1, long k_ts,
                          const void* v, long v_bs0, long v_bs1, long v_ts, void* o, long o_bs0, long o_bs1, long o_ts,
                          const float* out_scale, long os_group_stride, int os_heads, int batch, int heads, int hd, int nq, int nk,
                          float scale, int dtype, void* stream);

/* mmgt_attention whose every batch entry reads the second key segment, with a TWIN output: o_twin (o's strides) receives the attention over
 * the FIRST segment alone -- the state of the online softmax after its last tile --, o the attention over both.  The CFG pair of the first
 * reference-attention reader (mutual_self_attention.py:160-230): both rows enter with the same hidden states, the conditional row attends
 * [x | bank], the unconditional row [x]; one pass over x serves both.  bf16, head_dim 40, V transposed, nq % 256 == 0, nk % 64 == 0,
 * nk2 % 64 == 0 only (csrc/attn64.hip); anything else is an error. */
int mmgt_attention_twin(const void* q, long q_bs0, long q_bs1, long q_ts, const void* k, long k_bs0, long k_bs1, long k_ts,
                        const void* v, long v_bs0, long v_bs1, long v_ts, void* o, void* o_twin, long o_bs0, long o_bs1, long o_ts,
                        int bdiv, const void* k2, const void* v2, long k2_bs, long k2_ts, long v2_bs, long v2_ts, int k2_bdiv,
                        int nk2, int batch, int heads, int hd, int nq, int nk, float scale, int dtype, void* stream);

/* Row softmax of a (rows, cols) matrix scaled by `scale` (materialised-score attention of the VAE mid block). */
int mmgt_softmax_rows(const void* x, long ldx, void* out, long ldo, int rows, int cols, float scale, int dtype,
                      void* stream);

/* The bf16 path of the VAE mid-block attention (one 512-wide head over 4096 tokens per frame; replaces diffusers 0.24.0
 * `Attention` as called by `AutoencoderKL.decode` at pipeline_pose2vid_long.py:112-125).  Its logits reach hundreds with
 * sd-vae-ft-mse weights, so q . k keeps ~17 bits through hi / lo bf16 operand pieces on the bf16 MFMA path instead of an fp32 GEMM:
 *   mmgt_gemm_bf16_f32          out fp32 [M][ldo] = A bf16 [M][lda] . W bf16 [N][ldw]^T, raw accumulators, no epilogue
 *                               (K % 64 == 0, N % 8 == 0);
 *   mmgt_qk_split3              qk fp32 [rows][4C] = [t Wq_hi^T | t Wq_lo^T | t Wk_hi^T | t Wk_lo^T]  ->  q = qk0 + qk1 + bias_q,
 *                               k = qk2 + qk3 + bias_k,  Qp bf16 [rows][3C] = [q_hi | q_hi | q_lo],  Kp = [k_hi | k_lo | k_hi];
 *   mmgt_softmax_rows_f32_bf16  fp32 logits -> bf16 probabilities in one pass (cols a multiple of 256, at most 8192). */
int mmgt_gemm_bf16_f32(const void* A, long lda, const void* W, long ldw, float* out, long ldo, int M, int N, int K, void* stream);
int mmgt_qk_split3(const float* qk, const float* bias_q, const float* bias_k, void* Qp, void* Kp, long rows, int C, void* stream);
int mmgt_softmax_rows_f32_bf16(const float* x, long ldx, void* out, long ldo, int rows, int cols, float scale, void* stream);

/* Layout / dtype plumbing between the reference's (b, c, f, h, w) fp32 tensors and channels-last T:
 * out[(b*F + f), y, x, c] (c padded with zeros up to Cpad) <- in[b, c, f, y, x]; and the inverse (first C channels).
 * Replaces: the einops rearranges at resnet.py:13-15; transformer_3d.py:158,178-180,248-252,264. */
int mmgt_ncfhw_to_nhwc(const float* in, void* out, int B, int C, int F, int H, int W, int Cpad, float scale, int dtype,
                       void* stream);                       /* out = in * scale   (z / 0.18215 before the VAE, :114) */
int mmgt_nhwc_to_ncfhw(const void* in, float* out, int B, int C, int F, int H, int W, int Cpad, float scale, float shift,
                       int clamp01, int dtype, void* stream); /* out = clamp(in * scale + shift): (x/2+0.5).clamp(0,1), :122 */

/* Sinusoidal timestep features: out[b][0:half] = cos(t_b * f_i), out[b][half:] = sin(t_b * f_i), f_i = 10000^(-i/half).
 * Replaces: diffusers Timesteps(flip_sin_to_cos=True, shift 0) at unet_3d.py:496.  timesteps: fp32 [B] device. */
int mmgt_timestep_features(const float* timesteps, void* out, int B, int dim, int dtype, void* stream);

/* LayerNorm -> FeedForward(GEGLU) -> + residual of a transformer block as ONE launch, 320 channels, bf16 (csrc/ffn.hip):
 *   out[m] = residual[m] + bias2 + W2 . (h * gelu(g)),  [h | g] = W1 . LN(x[m]) + b1     (ln_gamma == NULL: no LayerNorm)
 * wimg: the weight image built by mmgt_amd/packing.py: pack_ff_fused (mmgt_ff_fused_image_bytes(C, inner) bytes; -1 if the shape
 * is not supported).  The hidden activations never reach memory: x is read once, out written once.
 * Replaces: the norm3 / ff_norm + `self.ff(...) + hidden_states` lines of src/models/attention.py:361,465,642,769 and
 * src/models/motion_module.py:253-254 (diffusers FeedForward) at the 64x64 level. */
int mmgt_ff_fused_image_bytes(int C, int inner);
int mmgt_ff_fused(const void* x, long ldx, const float* ln_gamma, const float* ln_beta, float eps, const void* wimg,
                  const float* bias2, const void* residual, long ldr, void* out, long ldo, int M, int C, int inner, int dtype,
                  void* stream);
/* ... and the block's proj_out on the end of the same launch:
 *   hidden = bf16(residual + bias2 + FeedForward(LN(x)))  (never stored),   out[m] = residual2[m] + bias_po + Wpo . hidden[m]
 * wpo: mmgt_amd/packing.py: pack_ff_proj_out(proj_out.weight (320, 320)), 204 800 bytes.
 * Replaces additionally: `hidden_states = self.proj_out(hidden_states)` + `output = hidden_states + residual` of
 * src/models/transformer_3d.py:262-268 and src/models/motion_module.py:178-182. */
int mmgt_ff_fused_po(const void* x, long ldx, const float* ln_gamma, const float* ln_beta, float eps, const void* wimg,
                     const float* bias2, const void* residual, long ldr, const void* wpo, const float* bias_po, const void* residual2,
                     long ldr2, void* out, long ldo, int M, int C, int inner, int dtype, void* stream);

/* [LayerNorm | GroupNorm ->] Linear(s) of the 320-channel level with the rows stationary in registers (csrc/rowgemm.hip), bf16:
 *   y[m, :] = [norm](x[m, :]) . W^T + bias [+ bias2[m / bias2_rows]] [+ residual[m, :]],   K = 320, N % 32 == 0, N <= 1920
 * norm = 0: none; 1: LayerNorm over the row (gamma [320], beta [pe_mod][320]); 2: x * gamma[g] + beta[g] with both tables
 * [pe_mod][320] and g = (m / pe_div) % pe_mod -- the second pass of a GroupNorm (tables from mmgt_groupnorm_affine, pe_div = HW,
 * pe_mod = NB) applied while the rows are loaded: the normalised tensor is never written.
 * Columns [0, n1) are written row-major to out[m * ldo + c]; columns [n1, N) TRANSPOSED per batch of n_tok rows to
 * out_t[(m / n_tok) * (N - n1) * npad + (c - n1) * npad + m % n_tok] (the V^T operand of mmgt_attention with v_transposed = 1), so the
 * q | k GEMM and the W . X^T GEMM of a self-attention and the LayerNorm in front of both are one launch that reads x once.
 * ln_gamma == NULL: no LayerNorm; ln_beta: [pe_mod][320], row (m / pe_div) % pe_mod (pe_mod <= 1: one row) -- the motion module's
 * positional encoding folded into beta as in mmgt_layernorm.  A residual needs n1 == N.  wimg: mmgt_amd/packing.py: pack_rowgemm
 * (mmgt_rowgemm320_image_bytes(N) bytes; -1 if N is not supported).
 * Replaces: norm1 / norm2 + to_q / to_k / to_v, and to_out[0] + residual, of src/models/attention.py:346-360,440-462,700-760
 * (diffusers Attention) and of src/models/motion_module.py:294-330 at the 64x64 level. */
long mmgt_rowgemm320_image_bytes(int N);
void mmgt_rowgemm_set_trace(void* stamps);   /* debug: u64 [workgroups][32] shader-clock stamps (mmgt_tune("rowgemm_dbg", 5)); NULL = off */
int mmgt_rowgemm320(const void* x, long ldx, int norm, const float* ln_gamma, const float* ln_beta, int pe_div, int pe_mod, float eps,
                    const void* wimg, const float* bias, const float* bias2, int bias2_rows, const void* residual, long ldr,
                    void* out, long ldo, int n1, void* out_t, int n_tok, int npad, int M, int N, int dtype, void* stream);

/* wav2vec2 feature extractor, element-wise pieces (csrc/wav2vec.hip; the convs / Linears / attention run on mmgt_gemm, mmgt_layernorm,
 * mmgt_attention).  x, out: (rows, C) channels-last in `dtype`.
 *   mmgt_channel_norm_gelu: out = gelu((x - mean_c) * rstd_c * gamma + beta), statistics per CHANNEL over the rows -- GroupNorm(C, C)
 *     over time + GELU of the first conv layer (transformers Wav2Vec2GroupNormConvLayer; src/models/wav2vec.py:73).
 *   mmgt_lerp_rows: rows_in -> rows_out frames, F.interpolate(mode="linear", align_corners=True) (src/models/wav2vec.py:196-209). */
int mmgt_channel_norm_gelu(const void* x, const float* gamma, const float* beta, void* out, int rows, int C, float eps, int dtype,
                           void* stream);
int mmgt_lerp_rows(const void* x, void* out, int rows_in, int rows_out, int C, int dtype, void* stream);

/* WavLM self-attention with the gated relative-position bias (csrc/wavlm.hip), per (batch b, head h, query i):
 *   o[b][i][h] = softmax_j(q_i . k_j * scale + gate[b][h][i] * tab[h][j - i + T - 1]) V,   head_dim 64, nq = nk = T in 1 .. 4096,
 *   gate = a (c grep_a[h] - 1) + 2 with (a, c) = sigmoid of the two group-of-4 sums of grep_w (8 x 64, fp32) . x[b][i][h*64 .. +63] + grep_b,
 * computed in the kernel from x, the layer input after self_attn_layer_norm (rows of stride x_ts, batch stride x_bs, in `dtype`).
 * tab: (heads, 2T - 1) fp32, the raw bias of layer 0 (compute_bias) by offset j - i.  q/k/v/o rows are strided like mmgt_attention's
 * (element strides: batch *_bs, row *_ts; head h at column h*64), so the q|k|v GEMM output is read in place.  Softmax and gate in fp32.
 * Replaces: the reference's data/wavlm/modules_wavlm.py:504-540 (gate + position bias + F.multi_head_attention_forward's softmax(QK^T + mask) V)
 * and :444-455 per layer (the bias of WavLM.py:596-601, passed from layer 0 to all layers). */
int mmgt_relpos_attention(const void* q, long q_bs, long q_ts, const void* k, long k_bs, long k_ts, const void* v, long v_bs, long v_ts,
                          void* o, long o_bs, long o_ts, const void* x, long x_bs, long x_ts, const float* grep_w, const float* grep_b,
                          const float* grep_a, const float* tab, int batch, int heads, int hd, int T, float scale, int dtype, void* stream);

/* Elementwise x -> silu(x) (time embedding activation, resnet.py:226) over n elements. */
int mmgt_silu(const void* x, void* out, long n, int dtype, void* stream);

/* One CFG + DDIM update on fp32 latents (all (1,4,F,H,W) = n elements; pred_sum holds [uncond | cond] = 2n):
 *   eps = pred_sum / counter (per frame);  v = eps_u + s (eps_c - eps_u);
 *   x0 = sa_t x - sb_t v;  e = sa_t v + sb_t x;  x_prev = sa_p x0 + sb_p e          (v-prediction, eta = 0)
 * counter: fp32 [F]; frame index of element i = (i / hw) % F.
 * Replaces: src/pipelines/pipeline_pose2vid_long.py:622-635 + diffusers DDIMScheduler.step. */
int mmgt_cfg_ddim_step(const float* pred_sum, const float* counter, const float* latents, float* latents_out, long n,
                       int F, int hw, float guidance, float sa_t, float sb_t, float sa_p, float sb_p, void* stream);

/* The sampler's general update (csrc/sampler.hip): with eps_u, eps_c and v_g = eps_u + s (eps_c - eps_u) formed exactly as mmgt_cfg_ddim_step forms
 * them,
 *   rho = rescale sqrt(Var eps_c / Var v_g) + (1 - rescale)   (variances over all n elements; rho = 1 and `moments` unread when rescale == 0)
 *   v = rho v_g;   x0 = sa_t x - sb_t v;   x_next = k_x x + k_0 x0 + k_1 prev_x0 + k_v v + k_z noise
 * prev_x0 and noise may be null (their terms are skipped; a non-zero k_1 / k_z without its tensor is refused); x0 is also written to x0_out
 * when that is not null.  rescale outside [0, 1] is refused.  The coefficients: mmgt_amd/scheduler.py `update_coefficients` (DDIM with
 * eta > 0: diffusers DDIMScheduler.step; DPM-Solver++ 2M: Lu et al. 2211.01095 Alg. 2).
 * Replaces: rescale_noise_cfg of src/pipelines/pipeline_lmks2vid_long.py + scheduler.step(..., eta) of pipeline_pose2vid_long.py:627-635. */
int mmgt_sampler_step(const float* pred_sum, const float* counter, const float* latents, const float* prev_x0, const float* noise,
                      const double* moments, float* latents_out, float* x0_out, long n, int F, int hw, float guidance, float rescale, float sa_t,
                      float sb_t, float k_x, float k_0, float k_1, float k_v, float k_z, void* stream);

/* moments[4] (fp64, device) = (sum eps_c, sum eps_c^2, sum v_g, sum v_g^2) over the n elements, for mmgt_sampler_step's rho: no host
 * synchronisation.  Summed in fp64 in a fixed order -- per workgroup into partials[blocks][4], blocks a function of n alone (at most 512 =
 * the partials_rows that always suffice), then folded by one workgroup in index order; no atomics -- so equal inputs give equal bits on
 * every launch and every rank. */
int mmgt_cfg_moments(const float* pred_sum, const float* counter, long n, int F, int hw, float guidance, double* partials, int partials_rows,
                     double* moments, void* stream);

/* ---- Re-voicing an existing clip (csrc/vid2vid.hip).
 * The noised known clip and the kept-region blend.  x0, z, x, out: fp32 [n] = (1, C, F, h, w); mask: fp32 [F * hw], broadcast over C (element i
 * belongs to frame (i / hw) % F and pixel i % hw).
 *   known = sa x0 + sb z     one fp32 expression (an fma over the rounded sb z), the same in every use; a zero scalar drops its term, so
 *                            (sa, sb) = (1, 0) returns x0's bits and (0, 1) z's
 *   x, mask null:  out = known;   else  out = x where mask == 1, known where mask == 0 (selections), mask x + (1 - mask) known in between.
 * x and mask come together.  out may alias x, not x0 or z. */
int mmgt_known_latents(const float* x0, const float* z, const float* x, const float* mask, float* out, long n, int F, int hw, float sa, float sb,
                       void* stream);

/* Pixel mask uint8 [L][H][W] (H, W multiples of 8) -> latent cell mask fp32 [L][H/8][W/8] of exact 0 / 1: a cell is 1 iff some pixel >= 128 lies
 * in a cell within Chebyshev distance grow (0 .. 8) of it; cells outside the frame do not exist. */
int mmgt_mask_to_latent(const unsigned char* mask_px, float* cells, int L, int H, int W, int grow, void* stream);

/* Cell mask fp32 [L][h][w] (a cell counts when >= 0.5) -> paste-back alpha uint8 [L][8h][8w]: the cell mask repeated x 8, box-averaged over
 * (2r + 1)^2 pixels with edge replication, a = (255 count + area / 2) / area in integers, area = (2r + 1)^2; r = 0 .. 32 (r = 0: 0 / 255).
 * alpha must be 4-byte aligned. */
int mmgt_feather_alpha(const float* cells, unsigned char* alpha, int L, int h, int w, int r, void* stream);

/* Paste back: gen, orig, out uint8 [npix][3], alpha uint8 [npix]; every byte (g a + o (255 - a) + 127) / 255 in integer division: a = 0 returns
 * orig's bytes, a = 255 gen's. */
int mmgt_composite_u8(const unsigned char* gen, const unsigned char* orig, const unsigned char* alpha, unsigned char* out, long npix, void* stream);

/* One window of Fw frames into the overlap average: pred_sum[row0 + r, :, idx[j]] = fmaf(weights[j], pred[r, :, j], pred_sum[...]) for r < rows,
 * and counter[idx[j]] += weights[j] when bump_counter; the update kernels divide the sum by counter.  pred is channels-last T ((rows*Fw), hw, Cpad)
 * as produced by the UNet, pred_sum fp32 (2, C, F, hw), idx int32 [Fw] of distinct frames (one outside [0, F) is skipped).  rows is 1 or 2 with
 * row0 + rows <= 2: the CFG pair, or one CFG row (the window-parallel sampler exchanges single rows sliced to Cpad == C and passes
 * bump_counter = 0 for a window's second row, so that counter counts windows as :624 does; rows = 1, row0 = 1 is also the conditional row of a step
 * outside the guidance interval).  weights: fp32 [Fw] on the device, the weight of each POSITION of a window (context_fuse), or NULL
 * for 1 everywhere: the plain add.  The fmaf is explicit, so all weights 1 give the bits of NULL.  Fw <= 256.
 * Replaces: src/pipelines/pipeline_pose2vid_long.py:622-624. */
int mmgt_accumulate_window(const void* pred, float* pred_sum, float* counter, const int* idx, const float* weights, int Fw, int F, int C, int Cpad,
                           int hw, int rows, int row0, int bump_counter, int dtype, void* stream);

/* The same for the B windows of one sampler group (context_batch_size = B) in one launch: pred ((rows*B*Fw), hw, Cpad) in CFG row major order
 * (rows = 2: [uncond w0 .. uncond w(B-1), cond w0 .. cond w(B-1)]; rows = 1: [w0 .. w(B-1)] of CFG row row0), idx int32 [B][Fw].  The windows may
 * share frames: a thread owns one target element and adds the windows that hold its frame in list order, and counter gets each covering window's
 * weight in that order (always; there is no bump_counter).  Bitwise what B calls of mmgt_accumulate_window on the windows' own slices give; weights
 * as there, NULL included.  A frame that no window covers keeps its bits.  No atomics.  B <= 256, F <= 65535. */
int mmgt_accumulate_windows(const void* pred, float* pred_sum, float* counter, const int* idx, const float* weights, int B, int Fw, int F, int C,
                            int Cpad, int hw, int rows, int row0, int dtype, void* stream);

/* ---- Stage-1 SMGA audio -> pose sampler: the element-wise glue between its Linear / attention / LayerNorm calls.
 * out = x rotated pairwise by the angle table cos_sin[(row % seq)][dim / 2][2] (cos, sin): RotaryEmbedding.rotate_queries_or_keys,
 * src/audio2pose_model/rotary_embedding_torch.py:38-61,106-113 (call sites model.py:121,267,298-299). */
int mmgt_rotary(const void* x, const float* cos_sin, void* out, long rows, int dim, int seq, int dtype, void* stream);
/* out = res (+ res2) + (scale[b] + 1) * x + shift[b], b = row / rows_per_batch, scale_shift fp32 rows of [scale(dim) | shift(dim)]
 * with row stride ld_ss: featurewise_affine of a DenseFiLM output plus the residual, model.py:44-64,231,246-259. */
int mmgt_film_residual(const void* x, const float* scale_shift, long ld_ss, const void* res, const void* res2, void* out, long rows,
                       int dim, int rows_per_batch, int dtype, void* stream);
/* out[b][c] (fp32) = mean over tokens of x[b][t][c]: model.py:460. */
int mmgt_mean_tokens(const void* x, float* out, int batch, int tokens, int dim, int dtype, void* stream);
/* out = act(x) element-wise for act in {MMGT_ACT_SILU, MMGT_ACT_GELU, MMGT_ACT_MISH}: DenseFiLM's Mish in front of its Linear
 * (model.py:50-52) where no GEMM epilogue can carry it. */
int mmgt_activation(const void* x, void* out, long n, int act, int dtype, void* stream);
/* x0 = clamp(u + (c - u) g, -1, 1); eps = (x sqrt(1/a) - x0) / sqrt(1/a - 1); out = last ? x0 : x0 sqrt(a') + c eps + sigma noise:
 * guided_forward + model_predictions + the DDIM update of src/audio2pose_model/diffusion.py:149-156,257-273 (fp32 sampler state). */
int mmgt_smga_ddim_step(const void* pred_uncond, const void* pred_cond, const float* x, const float* noise, float* out, long n,
                        float guidance, float sqrt_recip_acp, float sqrt_recipm1_acp, float sqrt_acp_next, float c, float sigma,
                        int last, int dtype, void* stream);

/* One launch per temporal-attention leg of a level-0 motion module (csrc/tleg.hip; src/models/motion_module.py:236-259,351-388):
 *   out = x + to_out(softmax_f(q k^T * scale) v),  q | k | v = (LayerNorm(x; ln_gamma, eps) + beta_pe[f]) . W^T   per pixel over its `frames` rows.
 * x / out (batch * frames * n_pix, 320) bf16, rows ordered (batch, frame, pixel), contiguous; out may alias x.  beta_pe (pe_rows >= frames, 320)
 * fp32 = LayerNorm bias + positional encoding of frame f.  wimg = packing.pack_tleg(Wq, Wk, Wv, Wo) (mmgt_temporal_leg320_image_bytes() bytes),
 * bias_o (320) fp32.  frames = 24 or 12 (48 rows per wave), n_pix a multiple of 4 * 48 / frames.  bf16 only: the fp32-I/O mode and every
 * other shape run rowgemm / LayerNorm + GEMM -> mmgt_attention -> GEMM + residual. */
long mmgt_temporal_leg320_image_bytes(void);
int mmgt_temporal_leg320(const void* x, void* out, const float* ln_gamma, const float* beta_pe, int pe_rows, const void* wimg, const float* bias_o,
                         int batch, int frames, int n_pix, float scale, float eps, int dtype, void* stream);

/* GroupNorm + SiLU + conv3x3 (stride 1, padding 1) in one launch for the VAE's 128- and 256-channel levels (csrc/gnconv.hip; diffusers
 * `ResnetBlock2D.forward` norm -> nonlinearity -> conv as `AutoencoderKL.decode` runs it for src/pipelines/pipeline_pose2vid_long.py:112-125):
 *   out[..., 0 .. Cout) = bias + conv3x3( silu( x * scale[n, c] + shift[n, c] ) ) (+ residual[..., 0 .. Cout))
 * x (nb, H, W, Cin) bf16 channels-last, H and W multiples of 16, smaller than 2 GiB; scale / shift (nb, Cin) fp32 = the tables of
 * mmgt_groupnorm_affine in ONE allocation (shift = scale + nb * Cin); wimg = packing.pack_gnconv(W) (mmgt_gn_silu_conv3x3_image_bytes(Cin, Cout) bytes); bias (Cout) fp32 or null;
 * residual / out: bf16 tensors of ldo >= Cout channels per pixel (a 256-wide output = two launches on its 128-channel halves), residual or null.
 * bf16; (Cin, Cout) = (128, 128), (256, 128), (128, 64: no residual).  Everything else runs mmgt_groupnorm -> mmgt_conv3x3. */
long mmgt_gn_silu_conv3x3_image_bytes(int cin, int cout);
int mmgt_gn_silu_conv3x3(const void* x, const float* scale, const float* shift, const void* wimg, const float* bias, const void* residual, void* out,
                         float* stats, int nb, int H, int W, int cin, int cout, int ldo, int dtype, void* stream);
/* `stats` (or null; Cout = 128 launches): the launch also writes, per 16 x 16 tile and 4-channel quad of its output, the pair (sum, sum of
 * squares) of the bf16 values it stores -- [nb * (H / 16) (W / 16)][ldo / 4][2] floats, a launch on the second half of a 256-wide output is handed
 * stats + 64.  mmgt_gn_stats_finalize folds them (fixed order) into the (scale, shift) tables of the GroupNorm that reads that output, so the
 * statistics pass of mmgt_groupnorm_affine over the tensor is not needed (resnet.py:20-28 `InflatedGroupNorm` / diffusers GroupNorm semantics:
 * biased variance over (H W C / G) values, eps inside the root).  scale | shift: one allocation, shift = scale + nb * C. */
int mmgt_gn_stats_finalize(const float* stats, const float* gamma, const float* beta, float* scale, float* shift, int nb, int tiles, int C, int G,
                           float eps, void* stream);

/* GroupNorm-apply + SiLU + conv3x3 (stride 1, padding 1) of the UNet's resnets in one launch (csrc/rconv.hip; ResnetBlock3D.forward,
 * src/models/resnet.py:217-247: norm1 -> nonlinearity -> conv1 (+ temb) and norm2 -> nonlinearity -> conv2 (+ shortcut), per frame as
 * InflatedGroupNorm / InflatedConv3d of :20-28, :156-196 run them):
 *   out = bias + bias2[n / b2_imgs] + conv3x3( silu( (x0 | x1) * scale[n, c] + shift[n, c] ) ) (+ residual)
 * x0 (nb, H, W, C0) and optionally x1 (nb, H, W, C1): the two halves of the channel concatenation in front of an up-block resnet; H, W multiples
 * of 16; C0, C1 multiples of 64; Cout a multiple of 320; scale_shift (2, nb, C0 + C1) fp32 = the tables of mmgt_groupnorm_affine2 in one
 * allocation; wimg = packing.pack_rconv(W) (mmgt_gn_silu_conv3x3_unet_image_bytes(C0 + C1, Cout) bytes); bias (Cout), bias2 (rows, Cout) fp32 or
 * null (the time-embedding projection: image n takes row n / b2_imgs); residual / out (nb, H, W, Cout) bf16.  bf16 only; everything else runs
 * mmgt_groupnorm_nhwc -> mmgt_conv3x3_nhwc. */
long mmgt_gn_silu_conv3x3_unet_image_bytes(int cin, int cout);
/* ... with the statistics of the GroupNorm that reads `out` from the launch's epilogue (the next leg's norm2, resnet.py:231): `stats` (or NULL) receives
 * [3][nb (H / 16) (W / 16) (16 / rows)][Cout] floats = (pivot, sum, sum of squares of the deviations from the pivot) of the bf16 values stored, per partial
 * of rows x 16 pixels and channel; rows = mmgt_gn_silu_conv3x3_unet_stats_rows(nb, H, W, Cout) (4 or 2: the cut the launch takes for this shape).
 * mmgt_gn_stats_finalize_unet combines the partials (Chan's pairwise update: no cancellation whatever the mean) into scale | shift (2, nb, C) of
 * GroupNorm(G, gamma, beta, eps) over the stored tensor (count = 16 rows values per partial and channel): no statistics pass over the tensor. */
int mmgt_gn_silu_conv3x3_unet_stats_rows(int nb, int H, int W, int cout);
int mmgt_gn_silu_conv3x3_unet_stats(const void* x0, int C0, const void* x1, int C1, const float* scale_shift, const void* wimg, const float* bias,
                                    const float* bias2, int b2_imgs, const void* residual, void* out, float* stats, int nb, int H, int W, int cout, int dtype,
                                    void* stream);
int mmgt_gn_stats_finalize_unet(const float* stats, const float* gamma, const float* beta, float* scale_shift, int nb, int parts_per_img, int count, int C,
                                int G, float eps, void* stream);
/* Debug (tools/trace_rconv.py): a device buffer of [workgroups][512] u64 receives 100-MHz stamps of the launches that follow; NULL = off. */
void mmgt_rconv_set_trace(void* buf);
int mmgt_gn_silu_conv3x3_unet(const void* x0, int C0, const void* x1, int C1, const float* scale_shift, const void* wimg, const float* bias,
                              const float* bias2, int b2_imgs, const void* residual, void* out, int nb, int H, int W, int cout, int dtype, void* stream);

/* ---- conditioning producers and the output path on the device; uint8 image buffers are device pointers.
 * blur_mask: (frames, H, W) u8 -> (frames, 64, 64) u8 = cv2.resize(64x64, bilinear) -> cv2.GaussianBlur(ksize, sigma from ksize,
 * reflect-101) -> cv2.normalize(MINMAX, 0, 255): scripts/pose2vid.py:94-114, scripts/audio2vid.py:131-151. */
int mmgt_blur_mask_u8(const unsigned char* masks, unsigned char* out, int frames, int H, int W, int ksize, void* stream);
/* (frames, S, S) u8 -> (frames, D, D): PIL's two-pass 8-bit resampling with the caller's integer coefficient tables
 * (bounds[D][2] = first tap, tap count; coeffs[D][ksize], 22 fractional bits), written as float / 255 (ToTensor) and / or u8:
 * torchvision Resize + ToTensor of src/dataset/image_processor.py:75-102,311-333. */
int mmgt_resample_u8(const unsigned char* in, float* out_f32, unsigned char* out_u8, int frames, int S, int D, const int* bounds,
                     const int* coeffs, int ksize, void* stream);
/* out[f][j] = x[clamp(f + j - half, 0, frames - 1)], j = 0 .. 2 half, rows of D floats: process_audio_emb, scripts/pose2vid.py:72-91. */
int mmgt_window_stack(const float* x, float* out, int frames, long D, int half, void* stream);
/* out (npix, 3) u8 = trunc(clamp(x[p][0..2] * scale + shift, 0, 1) * 255) from channels-last T (npix, cpad): decode_latents'
 * (x / 2 + 0.5).clamp(0, 1) (pipeline_pose2vid_long.py:121-123) fused with save_videos_grid's (x * 255).astype(uint8)
 * (src/utils/util.py:148-160). */
int mmgt_frames_to_u8(const void* x, unsigned char* out, long npix, int cpad, float scale, float shift, int dtype, void* stream);
/* ---- Motion-JPEG output path (csrc/mjpeg.hip, mmgt_amd/video_out.py): baseline sequential JPEG (ITU T.81, JFIF 1.01) of device-resident frames.
 * subsampling is 420 (MCU 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr) or 444 (MCU 8 x 8, blocks Y Cb Cr); mcu_rows / mcu_cols = ceil(H or W / MCU side);
 * quality 1 .. 100 scales the Annex K tables by the IJG rule.  Every buffer but qtables' is a device pointer.
 * dct_quant: frames (n, H, W, 3) u8 RGB -> coef (n, mcu_rows, mcu_cols, blocks per MCU, 64) int16 in zigzag order, DC in [-1024, 1023], AC in
 * [-1023, 1023]; H and W need not be MCU multiples (edge replication). */
int mmgt_jpeg_dct_quant(const unsigned char* frames, short* coef, int n, int H, int W, int subsampling, int quality, void* stream);
/* coef -> one byte-aligned, 0xFF-stuffed entropy-coded segment per (frame, MCU row) with the DC predictors reset (restart interval = one MCU
 * row, Annex K Huffman tables): segment s at segs + s * seg_stride, its byte count in sizes[s].  seg_stride >= segment_stride(W): the bound no
 * input can exceed. */
int mmgt_jpeg_entropy(const short* coef, unsigned char* segs, int* sizes, int n, int H, int W, int subsampling, long seg_stride, void* stream);
int mmgt_jpeg_segment_stride(int W, int subsampling, long* stride);
/* offsets[s] = sum over s' < s of (sizes[s'] + 2), offsets[nseg] = the total: where compact puts segment s and its marker. */
int mmgt_jpeg_scan(const int* sizes, long long* offsets, int nseg, void* stream);
/* out[offsets[s] ...] = segment s followed by RSTm (m = MCU row & 7) or, after the last MCU row of a frame, EOI: frame f's scan data with all its
 * markers is out[offsets[f * mcu_rows] : offsets[(f + 1) * mcu_rows]].  out_bytes = offsets[nseg]. */
int mmgt_jpeg_compact(const unsigned char* segs, long seg_stride, const int* sizes, const long long* offsets, unsigned char* out, long long out_bytes,
                      int nseg, int mcu_rows, void* stream);
/* Host: the luminance and chrominance quantiser tables of `quality` in zigzag order (the body of two DQT segments), 128 bytes. */
int mmgt_jpeg_qtables(int quality, unsigned char* zigzag128);
/* ---- JPEG input path (csrc/jpegdec.hip, csrc/jpegdec_core.h, mmgt_amd/video_in.py): baseline JPEG (SOF0, 8 bit, one interleaved scan)
 * of a batch of n equally sized frames -> device-resident RGB.  ncomp is 1 (hs = vs = 1) or 3 with luma sampling hs x vs = 1x1, 2x1 or 2x2 and
 * chroma 1x1; mcu_rows / mcu_cols = ceil(H / 8 vs), ceil(W / 8 hs).  Component c's plane has mcu_rows * v_c x mcu_cols * h_c blocks; a frame's
 * planes follow each other, frame_blocks blocks in all.  tables: table_ints int32 words per frame in the layout csrc/jpegdec_core.h states (table
 * selectors, four quantiser tables in natural order, MINCODE / MAXCODE / VALPTR / HUFFVAL of DC 0, DC 1, AC 0, AC 1).  Every buffer but sizes'
 * outputs is a device pointer. */
int mmgt_jpegdec_sizes(int H, int W, int ncomp, int hs, int vs, long long* frame_blocks, int* table_ints);
/* Restart segment s = data[offsets[s], offsets[s + 1]) (markers removed, 0xFF 0x00 stuffing still in) holds the MCUs [seginfo[3 s + 1],
 * seginfo[3 s + 2]) of frame seginfo[3 s]: one lane decodes it into coef (n, frame_blocks, 64) int16, natural order, zero-filled here first.
 * status[s] = 0, or 1 a code longer than 16 bits, 2 a coefficient index past 63, 3 a DC category above 11 / AC above 10, 4 an accumulated DC
 * outside [-2048, 2047], 5 data exhausted before the last block, 6 a descriptor outside the batch (nothing read).  Nothing is written out of
 * range whatever the bytes hold. */
int mmgt_jpegdec_entropy(const unsigned char* data, long long data_bytes, const long long* offsets, const int* seginfo, const int* tables,
                         short* coef, int* status, int n, int nseg, int H, int W, int ncomp, int hs, int vs, void* stream);
/* Dequantise + libjpeg's jpeg_idct_islow, + 128, clamp -> planes (n, frame_blocks * 64) uint8: component c's plane at its MCU-padded size. */
int mmgt_jpegdec_idct(const short* coef, const int* tables, unsigned char* planes, int n, int H, int W, int ncomp, int hs, int vs, void* stream);
/* libjpeg's fancy chroma up-sampling (replication when the chroma plane is 1 or 2 samples wide) + YCbCr -> RGB, cropped -> out (n, H, W, 3)
 * uint8; one component: Y in all three channels. */
int mmgt_jpegdec_color(const unsigned char* planes, unsigned char* out, int n, int H, int W, int ncomp, int hs, int vs, void* stream);
/* ---- progressive JPEG (SOF2) entropy stage (csrc/jpegprog.hip, csrc/jpegprog_core.h): fills the coefficient buffer of mmgt_jpegdec_idct
 * from the scans of n equally sized progressive frames; called once per dependency level of the batch, lowest first, with that level's restart
 * segments.  Segment s = data[offsets[s], offsets[s + 1]) holds the units [seginfo[3 s + 1], seginfo[3 s + 2]) of scan seginfo[3 s]; a unit is
 * a frame MCU in a scan of all components and one of the component's own ceil(w_c / 8) x ceil(h_c / 8) blocks, in raster order, in a scan of one.
 * scaninfo: 16 int32 words per scan (frame, component count, three component indices, Ss, Se, Ah, Al, three DC table indices, the AC table index,
 * three spare); huff: nhuff tables of 307 words each (MINCODE / MAXCODE / VALPTR / HUFFVAL as in a frame's table block), indexed by scaninfo.
 * coef: (n, frame_blocks, 64) int16 in natural order, the layout of mmgt_jpegdec_entropy; zero_fill != 0 (the first call of a batch) zero-fills
 * it on the stream first; later calls refine what earlier ones left, stream order being the only ordering.  status[s] = 0, or 1 a code longer
 * than 16 bits, 2 a coefficient index past Se, 3 a size category outside the scan type's range, 4 an EOB run past the segment's last block,
 * 5 data exhausted before the last block, 6 a descriptor outside the batch (nothing read).  Nothing is written outside the segment's own blocks. */
int mmgt_jpegprog_entropy(const unsigned char* data, long long data_bytes, const long long* offsets, const int* seginfo, const int* scaninfo,
                          const int* huff, short* coef, int* status, int n, int nseg, int nscan, int nhuff, int H, int W, int ncomp, int hs, int vs,
                          int zero_fill, void* stream);
/* ---- device image resize (csrc/resize.hip, csrc/resample_core.h): PIL's ImagingResample for 8-bit images, Image.resize with BILINEAR /
 * BICUBIC / LANCZOS, bit for bit.  in (n, Hs, Ws, C) uint8 interleaved, C = 1 or 3, every side 1 .. 16384, upscale or downscale.  The caller hands
 * in PIL's integer coefficient tables (mmgt_amd.conditioning.pil_resample_tables) per axis that changes: bounds[D][2] = (first tap, tap count) with
 * 0 <= first and first + count <= S, kk[D][ksize] = weights with 22 fractional bits, count <= ksize, 255 * sum |kk| + 2^21 < 2^31 per row.  A
 * horizontal launch runs if Wd != Ws, a vertical launch if Hd != Hs, each pass out = clip8((2^21 + sum u8 * k) >> 22) per band; when both run the
 * uint8 intermediate (n, Hs, Wd, C) goes to `tmp` (mmgt_resize_u8_workspace bytes; may be null otherwise).  A pass whose size does not change is
 * skipped.  The last launch -- or, when neither size changes, a copy launch -- writes exactly one of
 *   out_u8   (n, Hd, Wd, C) uint8 interleaved, or
 *   out_f32  (C, n, Hd, Wd) float planar, out = lut[c * 256 + value], lut = C x 256 floats from the caller (no device division).
 * in, tmp and out are different buffers; the axis tables of an unchanged axis may be null.  Bad arguments return 1 before any launch. */
int mmgt_resize_u8_workspace(int n, int Hs, int Ws, int Hd, int Wd, int C, long long* bytes);
int mmgt_resize_u8(const unsigned char* in, unsigned char* tmp, unsigned char* out_u8, float* out_f32, const float* lut, int n, int Hs, int Ws,
                   int Hd, int Wd, int C, const int* bounds_x, const int* kk_x, int ksize_x, const int* bounds_y, const int* kk_y, int ksize_y,
                   void* stream);
/* ---- GIF output path (csrc/gif.hip, mmgt_amd/video_out.py): GIF89a image data of device-resident frames with ONE palette for the clip.
 * A colour's bin is (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) (15 bits).  Every buffer is a device pointer; frames, idx, out are 4-byte aligned, lut
 * 16-byte aligned.  n, H, W >= 1, H, W <= 65535, n * H * W < 2^32.  Like every entry: 0 on success, else mmgt_last_error() has the text and
 * nothing was launched.
 * histogram: frames (n, H, W, 3) u8 RGB -> hist[32768] += pixels per bin (the caller zeroes hist). */
int mmgt_gif_histogram(const unsigned char* frames, unsigned int* hist, int n, int H, int W, void* stream);
/* idx (n, H, W) u8 = lut[bin(pixel)], lut u8[32768] (video_out.gif_lut: the nearest palette entry of each bin centre).  No dithering. */
int mmgt_gif_index(const unsigned char* frames, const unsigned char* lut, unsigned char* idx, int n, int H, int W, void* stream);
/* idx (n, H, W) u8 under Floyd-Steinberg error diffusion (csrc/gif_dither_core.h states the rule; raster order, integer, per frame): the pixel plus
 * the diffused error is clamped, looked up in lut, and leaves its difference to palette (256, 3) u8 as error.  A frame is one workgroup that takes
 * bands of mmgt_gif_dither_band() rows in sequence; frames of more than one band pass a row of errors through scratch, mmgt_gif_dither_scratch()
 * bytes (4 n W, or 0 for a single band; scratch may then be null), 4-byte aligned, contents irrelevant.  idx needs no alignment. */
int mmgt_gif_dither(const unsigned char* frames, const unsigned char* lut, const unsigned char* palette, unsigned char* idx, void* scratch,
                    long long scratch_bytes, int n, int H, int W, void* stream);
int mmgt_gif_dither_band(void);
int mmgt_gif_dither_scratch(int n, int H, int W, long long* bytes);
/* Frame differencing: out (n, H, W) u8 = 255 where idx equals the frame before at that pixel, else idx; frame 0 is compared with prev (H, W), the
 * last frame of the launch before, or copied if prev is null.  idx and out are 4-byte aligned and distinct. */
int mmgt_gif_delta(const unsigned char* idx, const unsigned char* prev, unsigned char* out, int n, int H, int W, void* stream);
/* GIF LZW (minimum code size 8, codes of 9 .. 12 bits, Clear = 256, End-of-Information = 257) of every (frame, strip): strip s of a frame is its rows
 * s * strip_rows .. min(H, (s + 1) * strip_rows) - 1, strips = ceil(H / strip_rows) <= 2048.  The strip's bits go LSB-first to
 * out + (frame * strips + s) * out_stride, their count to bits[frame * strips + s].  Every strip codes with a dictionary of its own: strip 0 opens
 * with Clear, every strip but the last closes with Clear (written at the width the decoder then holds), the last with End-of-Information, so a
 * frame's strips concatenated bit by bit are one valid GIF code stream.  out_stride >= strip_stride(W, strip_rows), a multiple of 4: the bound no
 * input can exceed, 12 (P + floor(P / 3838) + 2) bits for P = W * strip_rows pixels, in bytes rounded up to 16. */
int mmgt_gif_lzw(const unsigned char* idx, unsigned char* out, long long* bits, int n, int H, int W, int strip_rows, long out_stride, void* stream);
int mmgt_gif_strip_stride(int W, int strip_rows, long* stride);
/* Joins the strips of each frame at bit offsets (exclusive prefix sum of bits) and cuts the byte stream into GIF data sub-blocks: frame f's
 * image data, without the minimum-code-size byte, is packed[f * packed_stride : f * packed_stride + sizes[f]] = { length <= 255, bytes } ... 0x00.
 * packed_stride >= B + ceil(B / 255) + 1 with B = strips * out_stride. */
int mmgt_gif_pack(const unsigned char* out, const long long* bits, unsigned char* packed, int* sizes, int n, int strips, long out_stride,
                  long packed_stride, void* stream);
/* ---- PNG output path (csrc/png.hip, mmgt_amd/video_out.py): the zlib / deflate image data of truecolour 8-bit PNG frames.  Every buffer
 * is a device pointer.  Like every entry: 0 on success, else mmgt_last_error() has the text and nothing was launched.
 * filter: frames (n, H, W, 3) u8 RGB -> filt (n, H, 1 + 3 W): per scanline the filter type (the smallest sum of min(v, 256 - v) over the filtered
 * bytes, the lowest type on a tie; bpp = 3, the row above row 0 is zeros) and the filtered row; sums (n, H, 2) = { sum d[i], sum (L - i) d[i] } over
 * the row's L = 1 + 3 W bytes, of which the host makes the Adler-32.  n, H, W >= 1, H, W <= 16384. */
int mmgt_png_filter(const unsigned char* frames, unsigned char* filt, long long* sums, int n, int H, int W, void* stream);
/* The two passes of the deflate coder over ANY bytes: data (n, frame_bytes), every row cut into strips = ceil(frame_bytes / strip_bytes) strips of
 * strip_bytes (the last may be shorter), 1 <= frame_bytes <= 2^30.  A strip's tokens: position 0 is a literal; at p >= 1 with r = bytes from p on that
 * equal byte p - 1 (at most 258), r >= 3 is a match of length r and distance 1, else byte p is a literal; symbol 256 closes the strip.
 * histogram: hist (n * strips, 286) = how often each literal/length symbol occurs (every entry is written).
 * deflate: strip k = frame * strips + s writes header_bits[k] <= 8 * MMGT_PNG_HEADER_BYTES bits of header + k * MMGT_PNG_HEADER_BYTES, then its tokens
 * coded with codes + k * 286 (entry = the symbol's code, bit-reversed for an LSB-first stream, | its length << 16; a match is followed by its extra
 * bits and one zero bit, the single distance code), LSB-first into the words slot_off[k] .. slot_off[k + 1] - 1 of slots (slot_off has n * strips + 1
 * entries; no word outside a slot or outside slots_words is touched, every word below ceil(bits / 32) of a slot is written), and bits[k] = the bits
 * it took. */
#define MMGT_PNG_HEADER_BYTES 576
int mmgt_png_histogram(const unsigned char* data, unsigned int* hist, int n, long long frame_bytes, long long strip_bytes, void* stream);
int mmgt_png_deflate(const unsigned char* data, const unsigned int* codes, const unsigned int* header, const int* header_bits, unsigned int* slots,
                     const long long* slot_off, long long slots_words, long long* bits, int n, long long frame_bytes, long long strip_bytes,
                     void* stream);
/* Joins the strips of each frame bit by bit: bit_off (n, strips + 1) = where strip s starts in frame f's stream and, last, where the stream ends;
 * frame f's bytes go to out[out_off[f] .. out_off[f + 1] - 1] (out_off has n + 1 entries), every one of them written, the bits past the end zero.
 * Nothing outside slots_words / out_bytes is read or written. */
int mmgt_png_pack(const unsigned int* slots, const long long* slot_off, long long slots_words, const long long* bit_off, unsigned char* out,
                  const long long* out_off, long long out_bytes, int n, int strips, void* stream);
/* ---- WebP lossless output path (csrc/webp.hip, csrc/webp_core.h, mmgt_amd/video_out.py): one VP8L bitstream per RGB frame.  Every buffer
 * is a device pointer.  Like every entry: 0 on success, else mmgt_last_error() has the text and nothing was launched.
 * predict: frames (n, H, W, 3) u8 RGB -> modes (n, bh, bw) u8 with bh = ceil(H / 16), bw = ceil(W / 16): per block of 16 x 16 pixels the predictor
 * mode 0 .. 13 with the smallest sum of min(v, 256 - v) over its residuals' r, g, b, the lowest mode on a tie; res (n, H, W) = the residuals as ARGB
 * words, taken per channel mod 256 from the subtract-green pixels (255, r - g, g, b - g).  n, H, W >= 1, H, W <= 16384. */
int mmgt_webp_predict(const unsigned char* frames, unsigned char* modes, unsigned int* res, int n, int H, int W, void* stream);
/* The two passes of the coder over ANY words: res (n, frame_px), every row cut into strips = ceil(frame_px / strip_px) strips of strip_px (the last
 * may be shorter), 1 <= frame_px <= 2^28.  A strip's tokens: position 0 is a literal; at p >= 1 with r = words from p on that equal word p - 1 (at most
 * 4096), r >= 3 is a match of length r from the left pixel, else word p is a literal.
 * histogram: hist (n * strips, MMGT_WEBP_HIST_WORDS) = how often each symbol occurs: [0, 256) a literal's green, [256, 280) a match's length prefix,
 * [280, 536) a literal's red, [536, 792) its blue, [792] the matches (every entry is written).
 * code: strip s of frame f codes its tokens with codes + f * 792 (green / length, red, blue as in hist; entry = the symbol's code, bit-reversed for an
 * LSB-first stream, | its length << 16, length 0 for the symbol of a one-symbol code; a literal is green, red, blue, a match its prefix code and extra
 * bits; alpha and the distance take no bits), LSB-first into the words slot_off[k] .. slot_off[k + 1] - 1 of slots with k = f * (strips + 1) + 1 + s,
 * and bits[f * strips + s] = the bits it took.  Slot f * (strips + 1) is frame f's header: header[header_off[f] .. header_off[f + 1]) is copied there
 * (header_off has n + 1 entries, slot_off n * (strips + 1) + 1).  No word outside a slot, slots_words or header_words is touched; every word below
 * ceil(bits / 32) of a slot is written.  mmgt_png_pack joins a frame's strips + 1 slots. */
#define MMGT_WEBP_HIST_WORDS 793
int mmgt_webp_histogram(const unsigned int* res, unsigned int* hist, int n, long long frame_px, long long strip_px, void* stream);
int mmgt_webp_code(const unsigned int* res, const unsigned int* codes, const unsigned int* header, const long long* header_off, long long header_words,
                   unsigned int* slots, const long long* slot_off, long long slots_words, long long* bits, int n, long long frame_px,
                   long long strip_px, void* stream);
/* ---- WebP lossy output path (csrc/vp8.hip, csrc/vp8_core.h, mmgt_amd/video_out.py): one VP8 key frame per RGB frame.  Every buffer is a
 * device pointer unless said otherwise.  Like every entry: 0 on success, else mmgt_last_error() has the text and nothing was launched.  With
 * mbh = ceil(H / 16), mbw = ceil(W / 16): n, H, W >= 1, H, W <= 16383, n * mbh * mbw < 2^25; q = the quantiser index 0 .. 127; partitions 1, 2, 4, 8.
 * quantiser: (host pointers) quality 0 .. 100 -> its quantiser index and the default loop filter level of that index.
 * slot_bytes: (host pointers) the worst-case bytes of a first partition and of a token partition (DESIGN 4l derives them).
 * convert: frames (n, H, W, 3) u8 RGB -> Y (n, 16 mbh, 16 mbw), U, V (n, 8 mbh, 8 mbw), studio range, the frame padded by edge replication.
 * analyse: predicts (16 x 16 and chroma modes 0 DC, 1 V, 2 H, 3 TM; smallest squared error against the source, the lower mode on a tie), transforms,
 * quantises and reconstructs every macroblock: levels (n, mbh, mbw, 25, 16) int16 in scan order (blocks 0 .. 15 luma, 16 .. 19 U, 20 .. 23 V, 24 Y2),
 * modes (n, mbh, mbw, 2), nz (n, mbh, mbw) masks of the blocks with a non-zero level, skipped (n) = macroblocks whose mask is 0, and the reconstructed
 * planes ry, ru, rv shaped like Y, U, V.  One workgroup per frame; no workgroup waits for another.
 * code: per frame the first partition (header fields, skip flags, modes) and `partitions` token partitions (macroblock row r in partition
 * r mod partitions), each by a boolean coder of its own into its slot: frame f's slots start at f * (first + partitions * token) bytes of slots, the
 * first partition's, then the token partitions'.  counts (n, 1 + partitions) = each coder's bytes, -1 if its slot was too small.
 * pack: frame f's payload (frame tag, start code, sizes, first partition, partitions - 1 sizes of 3 bytes, partitions) -> out[out_off[f] ..
 * out_off[f + 1]) (out_off has n + 1 entries; 10 + 3 * (partitions - 1) + the frame's counts bytes each).  Nothing outside out_bytes is written. */
int mmgt_vp8_quantiser(int quality, int* q, int* filter_level);
int mmgt_vp8_slot_bytes(int H, int W, int partitions, long long* first_bytes, long long* token_bytes);
int mmgt_vp8_convert(const unsigned char* frames, unsigned char* Y, unsigned char* U, unsigned char* V, int n, int H, int W, void* stream);
int mmgt_vp8_analyse(const unsigned char* Y, const unsigned char* U, const unsigned char* V, unsigned char* ry, unsigned char* ru, unsigned char* rv,
                     short* levels, unsigned char* modes, unsigned int* nz, int* skipped, int n, int H, int W, int q, void* stream);
int mmgt_vp8_code(const short* levels, const unsigned int* nz, const unsigned char* modes, const int* skipped, unsigned char* slots,
                  long long slots_bytes, long long* counts, int n, int H, int W, int q, int partitions, int filter_level, void* stream);
int mmgt_vp8_pack(const unsigned char* slots, long long slots_bytes, const long long* counts, unsigned char* out, const long long* out_off,
                  long long out_bytes, int n, int H, int W, int partitions, void* stream);
/* ---- PNG input path (csrc/pngdec.hip, csrc/pngdec_core.h, mmgt_amd/video_in.py): non-interlaced PNG / APNG frames of one geometry.  Every
 * buffer is a device pointer; the status words are those of csrc/pngdec_core.h (0: fine).  Arguments outside the stated range: non-zero, nothing
 * launched, mmgt_last_error() says "range".
 * inflate: stream f is the raw deflate bytes data[offsets[f] .. offsets[f + 1]) (no zlib header or trailer; offsets has n + 1 entries; data and filt
 * 16-byte aligned, data_bytes a multiple of 16 that covers every stream) -> filt + f * frame_bytes, frame_bytes bytes at most whatever the stream
 * holds, and status[f].  One 64-thread workgroup per stream; its loop consumes at least one bit per iteration or stops. */
int mmgt_png_inflate(const unsigned char* data, long long data_bytes, const long long* offsets, unsigned char* filt, int* status, int n,
                     long long frame_bytes, void* stream);
/* unfilter: filt (n, H, 1 + ceil(W * bits per pixel / 8)) is reconstructed in place (PNG filter types 0 .. 4, the row above row 0 zeros; a type above
 * 4 sets status[f] and counts as 0); sums (n, H, 2) = { sum d[i], sum (L - i) d[i] } over each row's L FILTERED bytes, as mmgt_png_filter writes them.
 * colour type 0 or 3 at depth 1, 2, 4 or 8; 2, 4 or 6 at depth 8; sides 1 .. 16384. */
int mmgt_png_unfilter(unsigned char* filt, long long* sums, int* status, int n, int H, int W, int colour_type, int depth, void* stream);
/* expand: reconstructed rows -> out (n, H, W, 3) u8 RGB as PIL's Image.convert("RGB") gives them: grey of 1 / 2 / 4 bits times 255 / 85 / 17, alpha
 * dropped, colour type 3 looked up in palette (n, 256, 3); an index at or past plte_len[f] sets status[f] (the pixel is black).  palette and plte_len
 * may be null for the other colour types. */
int mmgt_png_expand(const unsigned char* filt, const unsigned char* palette, const int* plte_len, unsigned char* out, int* status, int n, int H, int W,
                    int colour_type, int depth, void* stream);
/* ---- GIF input path (csrc/gifdec.hip, csrc/gifdec_core.h, mmgt_amd/video_in.py): a chunk of n consecutive frames of one GIF file.  Every
 * buffer is a device pointer; the status words are those of csrc/gifdec_core.h (0: fine).  tab (n, 16) long long is one row per frame (gifdec_core.h:
 * GD_X .. GD_FILL): rectangle, index-buffer offset, code-stream byte range in data, minimum code size, interlace flag, transparent index or -1, what the
 * frame leaves pending (0 nothing, 2 a colour, 3 the canvas before it drew), that colour, first-frame flag and first-frame fill colour.  Arguments
 * outside the stated range: non-zero, nothing launched, mmgt_last_error() says "range".
 * unlzw: frame f's LZW codes data[tab[f].begin .. tab[f].end) (sub-block framing removed; data_bytes a positive multiple of 16 that covers every
 * stream; 1 <= n <= 65535) -> its W * H palette indices in stream order at idx + tab[f].idx, never more, and status[f].  A row that names bytes
 * outside data_bytes / idx_bytes, a rectangle outside 16384 x 16384 or a code size outside 2 .. 8 gives status 4 and touches nothing.  One 64-thread
 * workgroup per frame; every round of its loop consumes at least one code or stops. */
int mmgt_gif_unlzw(const unsigned char* data, long long data_bytes, const long long* tab, unsigned char* idx, long long idx_bytes, int* status, int n,
                   void* stream);
/* compose: the chunk's frames drawn in order on the H x W canvas (sides 1 .. 16384, 1 <= n <= 65535) through palette (n, 256, 3) -> out (n, H, W, 3) u8
 * RGB, as PIL's ImageSequence.Iterator + convert("RGB") gives them.  carry (2, H, W, 3) holds the canvas and what it becomes before the next frame
 * draws: read unless tab[0] is the file's first frame, written at the end, so that a file may be decoded in chunks.  A row whose rectangle leaves
 * the canvas or whose indices leave idx_bytes draws nothing. */
int mmgt_gif_compose(const long long* tab, const unsigned char* idx, long long idx_bytes, const unsigned char* palette, unsigned char* carry,
                     unsigned char* out, int n, int H, int W, void* stream);
/* ---- WebP lossless input path (csrc/webpdec.hip, csrc/webpdec_core.h, mmgt_amd/video_in.py): a set of n frames (VP8L streams) of one or
 * more files of one canvas size.  Every buffer is a device pointer; the status words are those of csrc/webpdec_core.h (0: fine).  tab (n, 16) long
 * long is one row per frame (webpdec_core.h: WD_X .. WD_PH): rectangle on the canvas, the stream's byte range in data, offset and count of its
 * scratch words, offset of its ARGB words, flags (1 blend, 2 key frame, 4 first frame of its file, 8 the frame before disposes to background) and
 * that earlier frame's rectangle.  Arguments outside the stated range: non-zero, nothing launched, mmgt_last_error() says "range".
 * decode: frame f's VP8L stream data[tab[f].begin .. tab[f].end) (data_bytes a positive multiple of 16 that covers every stream, data and scratch
 * 16-byte aligned; 1 <= n <= 65535) -> its scratch words scratch[tab[f].scr .. + tab[f].cap): a header block of 32 words (the transforms in the
 * order read), the sub-images, the prefix-code groups where there are several, and the entropy-coded main image; and status[f].  Nothing is
 * written outside those words; a row that names bytes or words outside the buffers gives status 12 and touches nothing.  A frame whose
 * prefix-code groups (known only once its entropy image is decoded) do not fit its scratch words gives a NEGATIVE status: minus the words with
 * which it decodes, for the caller to come again.  One 64-thread workgroup per stream; every round of its loops consumes a bit, produces a pixel
 * or stops. */
int mmgt_webp_decode(const unsigned char* data, long long data_bytes, const long long* tab, unsigned int* scratch, long long scratch_words, int* status,
                     int n, void* stream);
/* untransform: each frame's transforms undone in its own order (frames of one call may differ in them) -> the ARGB words (A in the high byte) of its
 * own rectangle, W * H of them at argb + tab[f].pix, and status[f]; a frame whose decode left no valid header block gives status 13 and writes
 * nothing.  The scratch words are used up.  One 64-thread workgroup per frame. */
int mmgt_webp_untransform(const long long* tab, unsigned int* scratch, long long scratch_words, unsigned int* argb, long long argb_words, int* status,
                          int n, void* stream);
/* compose: the call's frames drawn in order on the H x W canvas (sides 1 .. 16384, 1 <= n <= 65535) as libwebp's WebPAnimDecoder composes them
 * -> out (n, H, W, 3) u8 RGB.  carry (H, W) words holds the RGBA canvas (R in the low byte): read unless tab[0] is its file's first frame, written
 * at the end, so that a file may be decoded in several sets of launches.  A row whose rectangle leaves the canvas or whose words leave argb_words
 * draws nothing. */
int mmgt_webp_compose(const long long* tab, const unsigned int* argb, long long argb_words, unsigned int* carry, unsigned char* out, int n, int H, int W,
                      void* stream);
/* ---- WebP lossy input path (csrc/vp8dec.hip, csrc/vp8dec_core.h, mmgt_amd/video_in.py): a set of n VP8 key frames.  Every buffer is a
 * device pointer; the status words are those of csrc/vp8dec_core.h (0: fine).  tab (n, 8) long long is one row per frame (vp8dec_core.h: V8D_BEGIN
 * .. V8D_H): the `VP8 ` payload's byte range in data, offset and count of its scratch words (v8d_frame_words(W, H) at least, the offset a
 * multiple of 4), offset of its ARGB words, width and height (1 .. 16383).  A row that names bytes or words outside the buffers gives status 1 and
 * touches nothing.  Arguments outside the stated range: non-zero, nothing launched, mmgt_last_error() says "range".
 * parse: frame header, first partition (segments, filter, quantisers, probability updates, every macroblock's segment, skip flag and modes) and
 * token partitions -> header block (64 words), 32 bytes and 384 int16 dequantised coefficients per macroblock; data_bytes a positive multiple of
 * 16, scratch 16-byte aligned, 1 <= n <= 65535.  One 512-thread workgroup per frame; its loops run mbw * mbh rounds and
 * ceil(mbh / partitions) * max(mbw, partitions) + partitions steps, whatever the stream says. */
int mmgt_vp8dec_parse(const unsigned char* data, long long data_bytes, const long long* tab, unsigned int* scratch, long long scratch_words, int* status,
                      int n, void* stream);
/* reconstruct: prediction plus residual of every macroblock along the fronts x + 2 y -> the unfiltered Y, U, V planes (padded to whole
 * macroblocks) behind the coefficients; a frame whose parse left no valid header block gives status 7 and writes nothing.  One 64-thread
 * workgroup per frame, mbw + 2 (mbh - 1) fronts. */
int mmgt_vp8dec_reconstruct(const long long* tab, unsigned int* scratch, long long scratch_words, int* status, int n, void* stream);
/* filter: the simple or the normal loop filter in place, along the same fronts, in libwebp's order within a macroblock. */
int mmgt_vp8dec_filter(const long long* tab, unsigned int* scratch, long long scratch_words, int* status, int n, void* stream);
/* output: fancy upsampling and YUV -> RGB -> the ARGB words (alpha 255) of each frame's own rectangle, W * H of them at argb + tab[f].pix, as
 * mmgt_webp_compose takes them.  max_pixels: the largest W * H among the rows (1 .. 16383 * 16383); one thread per pixel. */
int mmgt_vp8dec_output(const long long* tab, unsigned int* scratch, long long scratch_words, unsigned int* argb, long long argb_words, int* status, int n,
                       long long max_pixels, void* stream);
/* SMGA key points -> the four frame streams of Stage 2, drawn on the device: kp (frames, 134, 3) fp32 = SMGA's normalised
 * (x, y, score) features.  Replaces data/extract_movment_mask_all.py:319-321 `pose_vid_generator` (denormalize :128-132, mask_leg :66-89,
 * process_keypoints :98-119), src/dwpose/__init__.py:220-283 `DWposeDetector_movment_mask.__call__` with draw_pose / draw_pose_mask_head /
 * _lips / _hand (:133-196) and src/dwpose/util.py:79-157,160-206,208-230,291-302,349-388 (cv2.ellipse2Poly, fillConvexPoly, line, circle
 * restated), and the mp4 write / read round trip of scripts/audio2vid.py:386,426-430.  pose (frames, 512, 512, 3) u8; hands / lips / face
 * masks (frames, 512, 512) u8 (face = face box + hand boxes with the reference's uint8 wrap-around).  H = W = 512 (the reference's canvas). */
int mmgt_dwpose_draw(const float* kp, unsigned char* pose, unsigned char* hands_mask, unsigned char* lips_mask, unsigned char* face_mask,
                     int frames, int H, int W, void* stream);
/* ---- Audio input (csrc/audio.hip, csrc/audio_core.h, mmgt_amd/audio_in.py): what librosa.load(path, sr=16000) does for the reference
 * (data/audio_extraction/wavlm_features.py:61,128, src/dataset/audio_processor.py:106,142) on a WAV file's `data` chunk that is already on the
 * device.  Every buffer is a device pointer.
 * decode_mono: raw = n_frames interleaved little-endian frames of `channels` (1 .. 16) samples of format fmt (audio_core.h: 0 U8, 1 S16, 2 S24,
 * 3 S32, 4 F32, 5 F64) at ANY byte address -> out (n_frames,) fp32 in [-1, 1): the channels summed in fp32 in channel order, one division by the
 * channel count, full scale a power of two (U8 and S16 sum the raw integers and scale last; the other formats scale first).  Reads exactly
 * n_frames * channels * sample bytes, writes exactly n_frames floats. */
int mmgt_audio_decode_mono(const unsigned char* raw, float* out, long long n_frames, int channels, int fmt, void* stream);
/* resample: y[j] = sum_i x[i] h[j down - i up + half] for j < n_out = ceil(n_in up / down), zeros beyond both ends of x; up != down, reduced by
 * their gcd; h = 2 half + 1 taps on the up-sampled grid, handed over phase-major as `taps`: up rows of 2 half / up + 1 floats, row p =
 * h[p], h[p + up], ..., zero where the index passes 2 half.  One fp32 fma chain per output in ascending tap order; no atomics: the result does not
 * depend on the grid.  A workgroup's input span must fit 64 KiB of LDS (ratios up to 16 with the Kaiser-best filter do); n_in below 2^31. */
int mmgt_audio_resample(const float* x, long long n_in, const float* taps, int up, int down, int half, float* y, long long n_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
