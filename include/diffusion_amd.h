/* diffusion_amd.h - C ABI of libdiffusion_amd.so: the MI355X (gfx950) kernels behind the Stable Diffusion 2
 * U-Net training step.
 *
 * Boundary contract.  The reference (fanzhongyi/diffusion) is pure Python and has no
 * FFI of its own: its hot path enters native code through torch / diffusers / xformers calls made from
 *   diffusion/models/stable_diffusion.py:177-183   (timestep draw, add_noise, unet(...)['sample'])
 *   diffusion/models/stable_diffusion.py:185-187   (F.mse_loss)
 *   diffusion/train.py:33 + yamls/hydra-yamls/SD-2-base-256.yaml:55-58  (torch.optim.AdamW)
 *   diffusion/models/models.py:109-111             (xformers memory-efficient attention)
 *   diffusion/train.py:91-108                      (Composer low-precision GroupNorm / LayerNorm)
 * Every entry point below replaces one of those native ops; the comment on each names the call site.
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless said otherwise
 *   - activations are bf16, "NHWC": a tensor [B,H,W,C] is a row-major matrix [B*H*W rows][C] whose row
 *     stride (ld*, in ELEMENTS) may exceed C, so column slices of wider buffers (fused QKV, concat) are
 *     addressed without copies.  C, ld* and every column offset are multiples of 8 (16-byte vectors).
 *   - statistics, biases, norm affine parameters, master weights and gradients are fp32
 *   - no hidden allocation, no host synchronisation: scratch buffers are passed in, work is enqueued on
 *     `stream` (a hipStream_t) and the call returns immediately; safe under hipGraph stream capture
 *   - return value: 0 ok, DA_ERR_SHAPE (1) rejected arguments (nothing launched), DA_ERR_LAUNCH (2) HIP error
 */
#ifndef DIFFUSION_AMD_H
#define DIFFUSION_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* da_stream_t; /* == hipStream_t */

/* C[M,N] = alpha * gather(A)[M,K] . W[N,K]^T (+bias[N]) (+rowbias[image(m)][N]) (+R[M,N]).
 * Replaces torch.nn.Conv2d 3x3/1x1 (cuDNN) and torch.nn.Linear (cuBLAS) inside diffusers ResnetBlock2D /
 * Transformer2DModel, reached from stable_diffusion.py:183; with the transposed weight shadow it is also
 * their dgrad in backward.  K = ksize*ksize*Cin; W is [N][kh][kw][Cin]; M = B*Hout*Wout.
 * mode 0: stride 1 (pad 1 when ksize 3); 1: stride 2 pad 1 (Downsample2D); 2: dgrad of mode 1 (A = dY at
 * Hin x Win = half resolution); 3: 3x3 conv over the nearest-2x upsampled A (Upsample2D), Hout = 2*Hin; 4: stride 2 with
 * zero padding at the bottom / right only (AutoencoderKL encoder Downsample2D: F.pad(x, (0,1,0,1)) + conv stride 2).
 * out_fp32: C is float* (else bf16).  splitk_ws (may be NULL): fp32 workspace of splitk_ws_floats elements; when the
 * tile grid alone would leave most CUs idle (small M) the K loop is split over up to 8 workgroups per tile whose
 * partial slabs (splits*M*N floats) are summed by a fused finalize pass. */
int da_gemm_nt(const void* A, long lda, const void* W, void* C, long ldc, const float* bias, const void* rowbias,
               long ldrb, const void* R, long ldr, int M, int N, int K, int Cin, int Hin, int Win, int Hout, int Wout,
               int ksize, int mode, int out_fp32, float alpha, float* splitk_ws, long splitk_ws_floats,
               da_stream_t stream);

/* Feed-forward input projection with its GEGLU activation fused (diffusers FeedForward.net.0 = GEGLU.proj + gelu gate,
 * reached from stable_diffusion.py:183): F[M][2*inner] = A[M][K] . W[2*inner][K]^T + bias (bf16, kept for backward) and
 * G[M][inner] = F[:, :inner] * gelu_erf(F[:, inner:]) in one launch; bit-identical to da_gemm_nt followed by
 * da_geglu_fwd.  Requires inner % 160 == 0 and K % 64 == 0 (DA_ERR_SHAPE otherwise: use the two calls). */
int da_gemm_nt_geglu(const void* A, long lda, const void* W, void* F, long ldf, void* G, long ldg, const float* bias,
                     int M, int inner, int K, da_stream_t stream);

/* Backward counterpart on the dgrad of FeedForward.net.2: dG[M][inner] = dY[M][K] . Wt[inner][K]^T is gated against the
 * saved pre-activation F[M][2*inner] in the epilogue and leaves as dF[M][2*inner] (= da_geglu_bwd(F, dG)) without dG
 * ever reaching HBM; bit-identical to da_gemm_nt followed by da_geglu_bwd.  Requires inner % 320 == 0, K % 64 == 0. */
int da_gemm_nt_geglu_bwd(const void* dY, long lddy, const void* Wt, const void* F, long ldf, void* dF, long lddf, int M,
                         int inner, int K, da_stream_t stream);

/* tuning / test hooks (process-wide; 0 is always the shipped behaviour unless noted).  Returns DA_ERR_SHAPE for unknown keys.
 *   "gemm_nt_variant"   0 auto | 1 the 128x128 register-staged kernel | 4 / 5 / 10 / 14 / 12 force the 256x128 / 256x160 /
 *                       256x320 (8-wave) / 256x256 / 256x320 (16-wave) LDS-DMA form where eligible (Cin % 64 == 0) |
 *                       11 the 4-wave 128x320x32 form | 15 / 16 the 256x320 tile on 32x32x16 MFMAs (16 waves as 8x2 / 8 waves as 4x2) |
 *                       18 the 16-wave 384x128 form (N <= 128: VAE encoder)
 *   "gemm_nt_mfma32"    0 (default) never | -1 variant 12 becomes 15 for K <= 320 | 1 always
 *   "gemm_nt_dispatch"  1 (default) cost model over (tile form, split-K) | 0 the round-1 fill thresholds
 *   "gemm_nt_korder"    1 (default) 3x3 K loop walks a 64-channel chunk through its 9 taps | 0 tap-major
 *   "gemm_nt_splitk"    1 (default) split-K allowed | 0 never split
 *   "gemm_nt_persist"   -1 (default) linears / fused GEGLU run as one resident workgroup per CU walking the tile list |
 *                       n > 0 that many resident workgroups | 0 one workgroup per tile
 *   "gemm_nt_persist_conv" 1 (default) 3x3 convolutions with more tiles than CUs also run as a resident tile walk (next tile's
 *                       descriptors + first K-step ahead of the epilogue; +0...1.4 %, bit-identical) | 0 one workgroup per tile
 *   "gemm_nt_de"        1 (default) the convolution forms leave through the direct register -> HBM epilogue | 0 the LDS strip
 *                       epilogue everywhere | 2 / 3 also the linears without / with a residual (measured slower).  Bit-identical.
 *   "gemm_nt_ws"        bit mask, default 1: bit 0 the K = 320 linears (N = 320 ... 1280, M % 32 == 0, >= 8 row tiles per CU) run in
 *                       the weight-stationary kernel (W in the registers of four waves; gemm_nt_ws.hip) | bit 1 the K = 640 linears
 *                       too | bit 2 the fused GEGLU forward at K = 320 too | bit 3 the K = 640 form as two unpipelined workgroups per
 *                       CU (all three measured +-0 in the step).  Bit-identical.
 *   "gemm_nt_stream"    0 (default) | 1 / 2 the streaming short-K linear kernel (gemm_nt_v3.hip; slower) where it measured best /
 *                       wherever eligible; "gemm_nt_stream_lw" 4 | 16 its loader waves.  Bit-identical.
 *   "gemm_tn_ring"      0 (default) | 4 | 5: linear-layer weight gradients with a ring of 32-pixel half-stages (+-3 %).  Bit-identical.
 *   "gemm_tn_ungroup"   0 (default) da_gemm_tn_wgrad_group runs eligible items as grouped launches | 1 every item through the
 *                       per-layer path, one by one (the launches of da_gemm_tn_wgrad; A/B of the grouped form in one build)
 *   "attn_fused_bwd"    1 (default) da_attn_bwd runs as ONE kernel for Nk <= 128 (cross-attention, the 64-token level) | 0 the
 *                       dK/dV + dQ pair | 2 also 129 ... 256 keys on an 8-wave form (slower)
 *   "gemm_tn_variant"   0 auto | 1 the 128x128x32 wgrad kernel | 2 the 320x192x64 LDS-DMA wgrad kernel
 *   "gn_resident"       n (default 192): da_groupnorm_fwd / _bwd run as ONE kernel that holds a workgroup's (image, whole groups)
 *                       slab in registers - x (and dy) are read once - when the slab fits and the launch has >= n workgroups;
 *                       0 never (always the reduce / finalize / apply passes), 1 whenever the slab fits
 *   "gn_resident_min_slab" bytes (default 65536) of one tensor per workgroup below which the multi-pass form runs
 *   "gn_resident_form"  0 (default) auto | 1 16-wave backward forms only | 2 the 12-wave backward form above 8 vectors/thread
 *   "grad_overwrite"    0 (default) the gradient-producing entry points ADD to their outputs, as documented below | 1 they WRITE
 *                       them (da_gemm_tn_wgrad's dW and dbias, da_colsum_accum, da_image_colsum's db, dgamma / dbeta of
 *                       da_groupnorm_bwd / da_layernorm_bwd): set by the host around the first backward of an optimizer step,
 *                       which then needs no zero fill of the gradient buffer
 *   "reserve_cus"       R in [0, 128] (default 0): every grid sized to one round of the chip (persistent GEMM tile walks,
 *                       weight-gradient pixel splits, the dispatch cost model) uses #CUs - R, leaving R CUs to the RCCL
 *                       channels of an overlapping gradient all-reduce (set by the trainer when world size > 1) */
int da_set_option(const char* key, int value);
/* which kernel da_gemm_nt dispatches to for (M, N, K, Cin) given a split-K workspace of that many floats: 1 = gemm_nt_kernel (128x128 tile), 4 / 5 / 10 =
 * gemm_nt2_kernel with a 256x128 / 256x160 / 256x320 tile, 12 = the 16-wave 256x320 form, 14 = the 16-wave 256x256 form,
 * 15 = the 16-wave 256x320 form on 32x32x16 MFMAs (profiling labels only) */
int da_gemm_nt_variant_for(int M, int N, int K, int Cin, long splitk_ws_floats);

/* dW[N][ksize*ksize*Cin] += sum_m dY[m][n] * gather(X)[m][k]   (fp32).
 * Replaces the cuDNN/cuBLAS wgrad kernels autograd runs for the same layers (loss.backward() driven by
 * Composer).  modes 0, 1, 3 as above.  If dbias != NULL, dbias[n] += sum_m dY[m][n] as well
 * (fused into the large-tile kernel; the small-shape path uses da_colsum_accum with `scratch`, >= 256*N*2 floats).
 * When the pixel range is split over workgroups, the partial tiles AND the partial bias gradients are stored in split_ws
 * (fp32, caller-owned, may be shared with da_gemm_nt's split-K workspace on the same stream; ~128 MiB covers every split
 * grid of both wgrad kernels) and summed in a fixed order: dW and dbias are then bitwise reproducible run to run.  With
 * split_ws == NULL or too small they are accumulated with fp32 atomics instead (order-dependent last bits). */
int da_gemm_tn_wgrad(const void* dY, long lddy, const void* X, long ldx, float* dW, float* dbias, float* scratch, int M,
                     int N, int Cin, int Hin, int Win, int Hout, int Wout, int ksize, int mode, float* split_ws,
                     long split_ws_floats, da_stream_t stream);

/* which kernel da_gemm_tn_wgrad dispatches to (test / profiling label): 1 = gemm_tn_kernel (128x128x32, register-staged),
 * 2 = gemm_tn2_kernel<192, generic gather>, 3 = gemm_tn2_kernel<192, FAST> (uniform source stride + periodic border mask) */
int da_gemm_tn_variant_for(int M, int N, int Cin, int Hin, int Win, int Hout, int Wout, int ksize, int mode);

/* One linear layer (ksize 1, mode 0) of a grouped weight gradient: dW[N][Cin] += dY[M][N]^T . X[M][Cin], and
 * dbias[N] += column sums of dY when dbias != NULL.  lddy / ldx: row strides in elements. */
typedef struct DaWgradItem {
  const void* dY;
  long lddy;
  const void* X;
  long ldx;
  float* dW;
  float* dbias;
  int N;
  int Cin;
} DaWgradItem;

/* The weight (and bias) gradients of n_items linear layers that share their row count M - the linears of one transformer
 * block - with the contract of n_items da_gemm_tn_wgrad calls.  Items the 320x192x64 kernel takes on its FAST path
 * (da_gemm_tn_variant_for == 3, M % 64 == 0) run, in list order and up to 16 at a time, as one or two launches whose
 * workgroups cover the tiles of all their items: a layer alone has 2-28 tiles and needs 9-125 pixel splits to fill the chip,
 * each storing a whole fp32 slab; together they need 1-13.  One split count per launch; it and the cut of a run into two
 * launches are a pure function of the shapes (cost model in gemm_tn_v2.hip); with splits > 1 one reduce launch sums the
 * slabs of all items in a fixed order, so dW and dbias are bitwise reproducible.  Same bf16 products, fp32 sums; only the summation order differs from the per-layer path.
 * The per-layer path (bit-identical to da_gemm_tn_wgrad) takes: items that are not eligible, a run of fewer than two
 * eligible items, every item when split_ws is NULL, and a run the cost model finds cheaper per layer (which includes a
 * workspace too small for the split count worth having).  The small-shape kernel's bias column sum takes its scratch
 * (256*N*2 floats) from the tail of split_ws: DA_ERR_SHAPE when such an item finds no room.  Nothing is allocated; the item
 * table is copied into the kernel arguments, so the call may be captured into a graph. */
int da_gemm_tn_wgrad_group(const DaWgradItem* items, int n_items, int M, float* split_ws, long split_ws_floats,
                           da_stream_t stream);

/* the plan of da_gemm_tn_wgrad_group for these shapes under the current options (host only; pointers in the items are not
 * read except dbias != NULL): returns the number of grouped launches (-1: arguments the entry rejects), the pixel splits of
 * launch g in splits[g] for g < cap, and, when group_of != NULL, group_of[i] = launch of item i or -1 for the per-layer path */
int da_gemm_tn_group_plan(const DaWgradItem* items, int n_items, int M, long split_ws_floats, int* splits, int cap,
                          int* group_of);

/* softmax(Q K^T * scale) V for head_dim 64, heads at column offsets h*64 of Q/K/V/O; L2[B][H][Nq] receives the
 * per-row log2-sum-exp.  Replaces xformers memory_efficient_attention (models.py:109-111) / diffusers
 * attention for attn1 (self) and attn2 (cross, Nk = 77). */
int da_attn_fwd(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                float* L2, int B, int H, int Nq, int Nk, float scale, da_stream_t stream);
/* the same with a causal mask (key j <= query q), Nq == Nk == N: the self-attention of the frozen text encoder
 * (transformers CLIPTextModel behind stable_diffusion.py:168,172); forward only. */
int da_attn_fwd_causal(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                       float* L2, int B, int H, int N, float scale, da_stream_t stream);
/* the forward for head_dim D = 512 (the only D accepted; heads at column offsets h*D, every ld a multiple of 8 and >= H*D,
 * else DA_ERR_SHAPE with nothing launched): the single mid-block attention head of the frozen VAE, encoder and decoder
 * (diffusers AutoencoderKL behind stable_diffusion.py:167,171 `vae.encode` and :380 `vae.decode`); forward only. */
int da_attn_fwd_wide(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                     float* L2, int B, int H, int D, int Nq, int Nk, float scale, da_stream_t stream);
/* backward of da_attn_fwd; Delta[B][H][Nq] is scratch (rowsum(dO*O)). */
int da_attn_bwd(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, const void* O, long ldo,
                const void* dO, long lddo, const float* L2, float* Delta, void* dQ, long lddq, void* dK, long lddk,
                void* dV, long lddv, int B, int H, int Nq, int Nk, float scale, da_stream_t stream);

/* floats of scratch the norm / colsum entry points need for (B, HW, C) */
long da_norm_scratch_floats(int B, int HW, int C);

/* GroupNorm (+ optional fused SiLU) over [B][HW][C], G groups.  Replaces torch.nn.GroupNorm / Composer
 * LPGroupNorm (train.py:91-99) + F.silu in ResnetBlock2D / Transformer2DModel / conv_norm_out.
 * mean_rstd[B][G][2] is saved for backward; scale_shift is unused and never written, by either form (the argument
 * stays for the ABI; NULL is fine).
 * Single pass (see "gn_resident"): a 1024-thread workgroup owns HW pixels x CW channels (whole groups) of one image in
 * registers, so the tensor crosses HBM once in and once out; otherwise statistics, finalize and apply are three launches. */
int da_groupnorm_fwd(const void* X, long ldx, void* Y, long ldy, const float* gamma, const float* beta,
                     float* mean_rstd, float* scale_shift, float* scratch, int B, int HW, int C, int G, float eps,
                     int silu, da_stream_t stream);
/* dX = GN(+SiLU) backward (+ Radd if non-null); dgamma/dbeta accumulated (+=); coef[B][G][2] scratch.  In the single-pass
 * form x and dy stay in registers between the group sums and the dx sweep, and Radd is added to the bf16-rounded dX (as a
 * separate add of two bf16 tensors would); the multi-pass form adds it in fp32 before rounding. */
int da_groupnorm_bwd(const void* X, long ldx, const void* dY, long lddy, const void* Radd, long ldr, void* dX,
                     long lddx, const float* gamma, const float* beta, const float* mean_rstd, float* dgamma,
                     float* dbeta, float* coef, float* scratch, int B, int HW, int C, int G, int silu,
                     da_stream_t stream);
/* which GroupNorm form da_groupnorm_fwd (bwd = 0) / da_groupnorm_bwd (bwd = 1) runs for (B, HW, C, G) under the current
 * "gn_resident*" options, with ld_min / ld_max the smallest / largest row stride of its tensors (test / profiling label;
 * changes nothing): 1 = single pass, 0 = multi-pass, -1 = arguments the entry points reject.  out[7] receives
 * {threads, NL instantiation launched, CW, parts, peers8, P, nchunks}: the single-pass workgroup size, data vectors per
 * thread, channels per workgroup, workgroups per image, 8-apart part placement and pixel lanes (nchunks 0), or for the
 * multi-pass form {0, 0, C, 1, 0, 0, pixel chunks per image of the statistics pass}. */
int da_groupnorm_plan_for(int B, int HW, int C, int G, long ld_min, long ld_max, int bwd, int* out);

/* LayerNorm over rows of C.  Replaces torch.nn.LayerNorm / Composer LPLayerNorm (train.py:100-108) in
 * BasicTransformerBlock.  mean_rstd[M][2] saved for backward. */
int da_layernorm_fwd(const void* X, long ldx, void* Y, long ldy, const float* gamma, const float* beta,
                     float* mean_rstd, int M, int C, float eps, da_stream_t stream);
int da_layernorm_bwd(const void* X, long ldx, const void* dY, long lddy, const void* Radd, long ldr, void* dX,
                     long lddx, const float* gamma, const float* mean_rstd, float* dgamma, float* dbeta,
                     float* scratch, int M, int C, da_stream_t stream);

/* out[c] += sum_m X[m][c]  (bias gradients of every conv / linear) */
int da_colsum_accum(const void* X, long ldx, float* out, float* scratch, int M, int C, da_stream_t stream);

/* out[b][c] = sum over the HW pixels of image b of X (bf16, row stride ldo) and db[c] += sum_b out[b][c]:
 * gradient of the broadcast timestep-FiLM add (h + time_emb_proj(temb)[:, :, None, None]) and of conv1's bias. */
int da_image_colsum(const void* X, long ldx, void* out, long ldo, float* db, float* scratch, int B, int HW, int C,
                    da_stream_t stream);

/* GEGLU feed-forward gate: in = [a | g] (2*Cout columns), out = a * gelu_erf(g).  Replaces diffusers GEGLU. */
int da_geglu_fwd(const void* in, long ldi, void* out, long ldo, int M, int Cout, da_stream_t stream);
int da_geglu_bwd(const void* in, long ldi, const void* dout, long lddo, void* din, long lddi, int M, int Cout,
                 da_stream_t stream);

/* SiLU on the timestep embedding (ResnetBlock2D nonlinearity(temb), TimestepEmbedding act) */
int da_silu_fwd(const void* x, long ldx, void* y, long ldy, int M, int C, da_stream_t stream);
/* erf-GELU (the text encoder's MLP activation, CLIPTextConfig.hidden_act = "gelu"); forward only */
int da_gelu_fwd(const void* x, long ldx, void* y, long ldy, int M, int C, da_stream_t stream);
int da_silu_bwd(const void* x, long ldx, const void* dy, long lddy, void* dx, long lddx, int M, int C,
                da_stream_t stream);
/* quick-GELU x * sigmoid(1.702 x) (CLIP ViT-L/14 text encoder, CLIPTextConfig.hidden_act = "quick_gelu": the encoder
 * the pixel models build at diffusion/models/models.py:136,197); forward only, may run in place (y == x) */
int da_quick_gelu_fwd(const void* x, long ldx, void* y, long ldy, int M, int C, da_stream_t stream);

/* strided add / copy: residual gradient sums and torch.cat([h, skip], dim=1) of the up blocks */
int da_add(const void* a, long lda, const void* b, long ldb, void* o, long ldo, int M, int C, da_stream_t stream);
int da_copy2d(const void* a, long lda, void* o, long ldo, int M, int C, da_stream_t stream);

/* nearest-neighbour 2x upsample of [B,H,W,C] (diffusers Upsample2D / F.interpolate) and its backward */
int da_upsample2x_fwd(const void* x, void* y, int B, int H, int W, int C, da_stream_t stream);
int da_upsample2x_bwd(const void* dy, void* dx, int B, int H, int W, int C, da_stream_t stream);

/* diffusers Timesteps(flip_sin_to_cos=True, freq_shift=0): out[B][dim] = [cos | sin] (bf16); t is int64 */
int da_timestep_embed(const long long* t, void* out, int B, int dim, da_stream_t stream);
/* the same on fp32 t (continuous-time pixel diffusion, t in [0, pi/2): pixel_diffusion.py:78 draws t_max * rand, and
 * the U-Net embeds the angle unrounded).  Integer-valued t gives the same bits as da_timestep_embed. */
int da_timestep_embed_f32(const float* t, void* out, int B, int dim, da_stream_t stream);

/* DDPMScheduler.add_noise (stable_diffusion.py:180) fused with the NCHW fp32 -> NHWC(8) bf16 relayout and
 * the training target (eps, or get_velocity when v_pred - pixel_diffusion.py:90-91).
 * x0, eps: [B][4][HW] fp32; xt: [B*HW][8] bf16 (channels 4..7 zero); target: [B*HW][8] fp32.
 * DA_ERR_SHAPE for a NULL t or table and for an xt or target that is not 16-byte aligned, as da_add_noise_ex (such
 * arguments were undefined behaviour while this entry did not check them). */
int da_add_noise(const float* x0, const float* eps, const long long* t, const float* sqrt_ac,
                 const float* sqrt_1mac, void* xt, float* target, int B, int HW, int v_pred, da_stream_t stream);

/* The pixel-space noising of pixel_diffusion.py:81-93 (scheduler.add_noise + the target of prediction_type) fused with the
 * relayout, for C = 1..8 channels.  x0, eps: [B][C][HW] fp32; xt: [B*HW][8] bf16 (channels C..7 zero); target:
 * [B*HW][8] fp32 (channels C..7 zero); xt and target 16-byte aligned.
 *   t_is_f32 = 0: t is int64 [B], sqrt_ac / sqrt_1mac the DDPM tables (DDPMScheduler.add_noise / get_velocity);
 *   t_is_f32 = 1: t is fp32 [B] angles, the tangent schedule of schedulers.py:10-24 / :64-79 in the kernel:
 *                 x_t = cos t x0 + sin t eps, v = -sin t x0 + cos t eps; the tables are not read (may be NULL).
 * target_kind: 0 eps, 1 v (v_prediction), 2 x0 (sample).  For C = 4, t_is_f32 = 0 and target_kind 0 / 1 the result is
 * that of da_add_noise up to the rounding of x_t: da_add_noise fuses a x0 + (s eps) into one FMA, so a bf16 x_t in a
 * million or so differs by one ulp.  DA_ERR_SHAPE for C outside 1..8, an unknown target_kind, a
 * NULL t, missing tables (t_is_f32 = 0) or a misaligned xt / target. */
int da_add_noise_ex(const float* x0, const float* eps, const void* t, int t_is_f32, const float* sqrt_ac,
                    const float* sqrt_1mac, void* xt, float* target, int B, int C, int HW, int target_kind,
                    da_stream_t stream);

/* One denoising step of generate() after the U-Net call: classifier-free guidance, the scheduler update and the next U-Net
 * input.  Every step of DDIMScheduler (eta = 0) and ContinuousTimeScheduler is linear in (sample, model output, noise
 * draw); step_coefficients() of the schedulers gives the three coefficients.
 *   pred   fp32 [(cfg ? 2 : 1) * npix][8], forward_features' output; with cfg rows [0, npix) are the unconditional half and
 *          rows [npix, 2 npix) the conditional half (the torch.cat([uncond, text]) order of generate());
 *   x      fp32 [npix][8], the sampler's state in NHWC-8; x_out the same shape, may be x itself;
 *   noise  NULL, or fp32 NCHW [npix / HW][C][HW] (the Euler-Maruyama draw, in the layout da_add_noise reads);
 *   coef   DEVICE pointer to four floats {cx, cm, cn, guidance}: the launch can sit in a captured graph;
 *   xt_out NULL, or bf16 [copies * npix][8]: bf16(x_out) written `copies` (1 or 2) times, the next U-Net input.
 * Per pixel and channel c < C: m = cfg ? pu + g (pt - pu) : p, x_out = cx x + cm m (+ cn z) in fp32.  Channels C..7 of
 * both outputs are exactly 0 whatever the inputs hold there.  DA_ERR_SHAPE for C outside 1..8, copies outside {1, 2},
 * npix <= 0 or no multiple of HW, a NULL pred / x / coef / x_out, or a pointer that is not 16-byte aligned. */
int da_sampler_step(const float* pred, const float* x, const float* noise, const float* coef, float* x_out, void* xt_out,
                    long npix, int HW, int C, int cfg, int copies, da_stream_t stream);
/* The same step for a two-step scheduler (DPMSolverMultistepScheduler, DPM-Solver++ 2M): one operand wider, the previous
 * step's data prediction.  pred / x / x_out / xt_out / npix / C / cfg / copies as in da_sampler_step; there is no noise draw.
 *   hist   fp32 [npix][8], read (second-order steps only) and then overwritten in place with this step's data prediction;
 *   coef   DEVICE pointer to eight floats {ax, am, kx, k0, k1, guidance, 0, 0} (step_coefficients_ms of the scheduler).
 * Per pixel and channel c < C, in fp32 and in this order: m = cfg ? pu + g (pt - pu) : p; x0 = ax x + am m;
 * v = kx x + k0 x0; if k1 != 0: v += k1 hist; then hist = x0, x_out = v, xt = bf16(v).  With k1 == 0 (a first-order step)
 * hist is not read at all: it may hold anything, NaN included.  Channels C..7 of x_out, hist and xt_out are exactly 0
 * whatever the inputs hold there.  Every load of a pixel precedes its first store: x_out may be x.  DA_ERR_SHAPE as for
 * da_sampler_step, and for a NULL or misaligned hist. */
int da_sampler_step_ms(const float* pred, const float* x, float* hist, const float* coef, float* x_out, void* xt_out,
                       long npix, int HW, int C, int cfg, int copies, da_stream_t stream);
/* The masked (inpainting) forms of both steps.  Everything as in da_sampler_step / da_sampler_step_ms, then, with v the
 * value those would store and m the pixel's mask value (broadcast over the channels):
 *   kn = bA known8 + bS eps8;   x_out = m v + (1 - m) kn  (in exactly this form);   xt = bf16(x_out)
 *   known8 fp32 [npix][8], the clean sample, and eps8 fp32 [npix][8], its noise draw (da_sampler_init writes both);
 *   mask   fp32 [npix]: 1 repaints the pixel, 0 keeps it, fractions blend;
 *   coef   DEVICE pointer to eight floats: {cx, cm, cn, guidance, bA, bS, 0, 0} for da_sampler_step_blend,
 *          {ax, am, kx, k0, k1, guidance, bA, bS} for da_sampler_step_ms_blend; (bA, bS) re-noises the known sample to the
 *          level of the next timestep, (1, 0) on the last step.
 * m == 1 stores v's bits, m == 0 stores kn's, and with (bA, bS) = (1, 0) kn is known8's bits, however the compiler contracts
 * the FMAs (all operands finite).  hist of the two-step form is the unblended data prediction, as in da_sampler_step_ms.
 * Every load of a pixel precedes its first store: x_out may be x.  DA_ERR_SHAPE as for the unmasked forms, and for a NULL or
 * misaligned known8 / eps8 / mask. */
int da_sampler_step_blend(const float* pred, const float* x, const float* noise, const float* coef, const float* known8,
                          const float* eps8, const float* mask, float* x_out, void* xt_out, long npix, int HW, int C,
                          int cfg, int copies, da_stream_t stream);
int da_sampler_step_ms_blend(const float* pred, const float* x, float* hist, const float* coef, const float* known8,
                             const float* eps8, const float* mask, float* x_out, void* xt_out, long npix, int HW, int C,
                             int cfg, int copies, da_stream_t stream);
/* Guidance rescale (Lin et al., arXiv:2305.08891, section 3.4; diffusers' rescale_noise_cfg): the statistics pass.  With pt
 * the conditional half of pred (rows [npix, 2 npix)), pu the unconditional half, g = coef[g_index] read on the device (3 for
 * the da_sampler_step rows, 5 for the da_sampler_step_ms rows) and m = pu + g (pt - pu), per sample b over its C valid
 * channels and HW pixels:
 *   factor[b] = phi * std(pt) / std(m) + (1 - phi)          exactly 1 when std(m) == 0
 *   pred   fp32 [2 npix][8];  factor fp32 [npix / HW];  phi in [0, 1], a launch argument (not device data).
 * Both standard deviations have the same count, so the Bessel factor cancels.  One workgroup per sample; m and the sums are
 * formed in fp64 from the fp32 operands, on data shifted by the sample's first value, in a fixed order: every call gives the same bits, and |mean| >> std costs no
 * accuracy.  Channels C..7 of pred are not used, whatever they hold.  DA_ERR_SHAPE for npix <= 0 or no multiple of HW, C
 * outside 1..8, g_index outside 0..7, phi outside [0, 1], a NULL pointer, or pred / coef not 16-byte aligned. */
int da_guidance_rescale(const float* pred, const float* coef, int g_index, float phi, float* factor, long npix, int HW,
                        int C, da_stream_t stream);
/* The four step forms with guidance rescale: everything as in the entry without _rs, except that m is multiplied by
 * factor[pixel / HW] (fp32 [npix / HW], what da_guidance_rescale wrote) before the scheduler update, so HW must be the pixel
 * count of one sample also where there is no noise draw.  A factor of exactly 1 gives the bits of the plain entry.
 * DA_ERR_SHAPE as for the plain entry, and for a NULL factor. */
int da_sampler_step_rs(const float* pred, const float* x, const float* noise, const float* coef, const float* factor,
                       float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies, da_stream_t stream);
int da_sampler_step_ms_rs(const float* pred, const float* x, float* hist, const float* coef, const float* factor,
                          float* x_out, void* xt_out, long npix, int HW, int C, int cfg, int copies, da_stream_t stream);
int da_sampler_step_blend_rs(const float* pred, const float* x, const float* noise, const float* coef, const float* known8,
                             const float* eps8, const float* mask, const float* factor, float* x_out, void* xt_out,
                             long npix, int HW, int C, int cfg, int copies, da_stream_t stream);
int da_sampler_step_ms_blend_rs(const float* pred, const float* x, float* hist, const float* coef, const float* known8,
                                const float* eps8, const float* mask, const float* factor, float* x_out, void* xt_out,
                                long npix, int HW, int C, int cfg, int copies, da_stream_t stream);
/* The counter-based normal generator of the stochastic samplers, unfused: Philox4x32-10 (Salmon et al., SC'11; multipliers
 * 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds) and Box-Muller.  For image b, pixel
 * pix = h W + w and channel block k = c / 4:
 *   key     = (seeds[b] & 0xffffffff, seeds[b] >> 32)
 *   counter = (pix, draw, stream, k)                 stream 0: step noise, 1: initial latents
 *   (r0, r1) -> channels 4k, 4k + 1 and (r2, r3) -> channels 4k + 2, 4k + 3: for a pair (ra, rb)
 *   u = ((ra >> 9) + 0.5) 2^-23 (exact, in (0, 1)),  theta = 2 pi (rb >> 8) 2^-24,
 *   z_even = sqrt(-2 ln u) cos theta,  z_odd = sqrt(-2 ln u) sin theta              |z| <= 5.77; channels >= C are dropped
 * in fp32 with the accurate logf / sincospif / sqrtf.  So a value depends on (seed of its image, draw, stream, pixel, channel)
 * and on nothing else: not on B, not on the image's place in the batch.
 *   seeds  DEVICE uint64 [B], 8-byte aligned;  out fp32 NCHW [B][C][H][W], 16-byte aligned;
 *   kind 0 writes the normals, kind 1 the raw words r0..r3 as bit patterns in their place (needs C % 4 == 0).
 * da_sampler_step_rng draws the same values inside the step.  DA_ERR_SHAPE for B, H or W <= 0, H W > 2^31 - 1, C outside
 * 1..8, stream outside {0, 1}, kind outside {0, 1}, kind 1 with C % 4, a NULL or misaligned pointer. */
int da_randn_philox(const unsigned long long* seeds, unsigned draw, unsigned stream, float* out, int B, int C, int H, int W,
                    int kind, da_stream_t hip_stream);
/* The training step's noising with every draw made inside the launch: da_add_noise_ex without a noise operand.  x0 fp32
 * NCHW [B][C][HW], C = 1..8; xt bf16 [B HW][8] and target fp32 [B HW][8] laid out as da_add_noise_ex lays them out, channels
 * C..7 exactly +0; t int64 [B] (t_is_f32 = 0, with the tables sqrt_ac / sqrt_1mac of T entries) or fp32 [B] angles
 * (t_is_f32 = 1, tables not read), in DEVICE memory: written with the drawn timesteps when draw_t, else read and left as it is.
 * Per sample b the key is seeds[b] (DEVICE uint64 [B], 8-byte aligned) and the stream 0 of da_randn_philox; the draw number
 * says what a draw is for:
 *   draw 0  counter (pix, 0, 0, c / 4)   n,  the noise: the bits of da_randn_philox(seeds, 0, 0, [B, C, H, W])
 *   draw 1  counter (pix, 1, 0, c / 4)   z2, the perturbation draw, made iff perturbation != 0
 *   draw 2  counter (0, 2, 0, c / 4)     zc, one normal per (sample, channel), made iff noise_offset != 0: the bits of
 *                                        da_randn_philox(seeds, 2, 0, [B, C, 1, 1])
 *   draw 3  counter (0, 3, 0, 0)         word r0: the timestep, made iff draw_t
 * Each product and each sum below is rounded once (no FMA):
 *   n1 = n  + noise_offset zc[c]         the target's noise  (diffusers --noise_offset: noise += offset randn(B, C, 1, 1))
 *   n2 = n1 + perturbation z2            the noise of x_t only  (Ning et al., arXiv:2301.11706; diffusers --input_perturbation)
 *   x_t    = what da_add_noise_ex gives for (x0, eps = n2, t);   target = what it gives for (x0, eps = n1, t)
 * so with both options 0 the launch gives the bits of da_add_noise_ex fed da_randn_philox's draw 0.
 * Timesteps (draw_t): slot NULL and n_slots 0 draw uniformly; else slot is DEVICE int32 [B], the sample's stratum among
 * n_slots (values outside [0, n_slots) are clamped into it).
 *   discrete, integers 0 <= t_lo < t_hi <= T, R = t_hi - t_lo:
 *     uniform      t = t_lo + ((uint64) r0 R >> 32)
 *     stratified   t = t_lo + ((slot 2^32 + r0) R) / (n_slots 2^32)      in uint64; needs n_slots R < 2^32
 *   continuous, t_lo < t_hi both fp32 values, u = (r0 >> 8) 2^-24, every operation rounded to fp32:
 *     uniform      t = t_lo + (t_hi - t_lo) u
 *     stratified   the same with u' = (slot + u) / n_slots              n_slots <= 2^24
 * Both integer forms land in [t_lo, t_hi), the stratified one in [t_lo + floor(slot R / n_slots), t_lo + ceil((slot + 1) R /
 * n_slots)).  The timestep of sample b is written by the one thread that owns its pixel 0; no thread reads what another wrote,
 * and the launch allocates nothing and synchronises nothing: it may sit in a captured graph.  Without draw_t the range, slot and
 * n_slots are not used.  DA_ERR_SHAPE, with nothing written, for C outside 1..8, an unknown target_kind, B or HW <= 0,
 * (draw_t) t_lo >= t_hi, a discrete range that is fractional or outside [0, T], a continuous bound that is no fp32 value,
 * n_slots < 0, slot without n_slots or the reverse, n_slots R >= 2^32 (discrete) or n_slots > 2^24 (continuous), a NULL x0 /
 * seeds / t / xt / target, a misaligned pointer (seeds 8 bytes; xt, target 16), missing tables or T < 1 with t_is_f32 = 0,
 * a noise_offset or perturbation that is not finite. */
int da_add_noise_rng(const float* x0, const unsigned long long* seeds, const int* slot, int n_slots, void* t, int t_is_f32,
                     int draw_t, double t_lo, double t_hi, const float* sqrt_ac, const float* sqrt_1mac, int T,
                     float noise_offset, float perturbation, void* xt, float* target, int B, int C, int HW, int target_kind,
                     da_stream_t stream);
/* The stochastic step: any of the eight forms above with the noise term drawn inside the kernel.  `form` is a mask:
 * 1 two-step (hist), 2 blended (known8 / eps8 / mask), 4 rescaled (factor); the operands of a form that is not selected are
 * not read and may be NULL.  seeds: DEVICE uint64 [npix / HW], 8-byte aligned, required; HW is the pixel count of one
 * sample.  The row is wider, and the draw number travels in it as a uint32 BIT PATTERN in a float slot (write it through an
 * integer view, never through a float conversion):
 *   first order   eight floats  {cx, cm, cn, guidance, bA, bS, draw, 0}             (bA, bS read by the blended form only)
 *   two-step      twelve floats {ax, am, kx, k0, k1, guidance, bA, bS, kn, draw, 0, 0}
 * With z = da_randn_philox(seeds, draw, stream 0) at the pixel, the order is guidance, rescale, the update, then
 *   first order:  v = cx x + cm m + cn z            the bits da_sampler_step* gives when fed z as its noise operand
 *   two-step:     v = (kx x + k0 x0 (+ k1 hist)) + kn z            product and sum each rounded (no FMA)
 * then the blend; hist keeps the unblended, noise-free data prediction.  The kernel draws iff the noise coefficient (cn, kn)
 * is not 0 - one test for the whole launch - and a row with a zero coefficient gives the deterministic entry's bits.
 * DA_ERR_SHAPE as for the entry of the same form, and for form outside 0..7, a NULL or misaligned seeds, HW > 2^31 - 1. */
int da_sampler_step_rng(const float* pred, const float* x, float* hist, const float* coef, const float* known8,
                        const float* eps8, const float* mask, const float* factor, const unsigned long long* seeds,
                        float* x_out, void* xt_out, long npix, int HW, int C, int form, int cfg, int copies,
                        da_stream_t stream);
/* The start of a sample that begins from an image (image-to-image, inpainting), one launch:
 *   known   fp32 NCHW [B][C][H][W], the clean sample (latent models: already scaled); noise the same shape;
 *   mask_px NULL, or fp32 [B][f H][f W], the mask at f x f pixels per state pixel, f a power of two in 1..16;
 *   coef    DEVICE pointer to four floats {a0, s0, 0, 0}: add_noise at the first executed timestep;
 *   known8, eps8  NULL (both), or fp32 [B H W][8]: bit-exact NHWC-8 relayouts of known and noise;
 *   mask    fp32 [B H W], given iff mask_px is: the f x f box mean, summed row by row from the top left (a fixed order) and
 *           multiplied by the exact 1 / f^2;
 *   x       fp32 [B H W][8] = a0 known + s0 noise;  xt NULL, or bf16 [copies * B H W][8] = bf16(x), `copies` (1 or 2) times.
 * Channels C..7 of every [.][8] output are exactly 0.  DA_ERR_SHAPE for B, H or W <= 0, H W > 2^23, C outside 1..8, f no
 * power of two in 1..16, copies outside {1, 2}, a NULL known / noise / coef / x, mask without mask_px or known8 without eps8
 * (or the reverse), or a pointer that is not 16-byte aligned. */
int da_sampler_init(const float* known, const float* noise, const float* mask_px, const float* coef, float* known8,
                    float* eps8, float* mask, float* x, void* xt, int B, int H, int W, int C, int f, int copies,
                    da_stream_t stream);

/* LargestCenterSquare(R) + ToTensor + Normalize(0.5,0.5) of B packed RGB uint8 images (transforms.py:9-21, laion.py:159-164):
 * PIL's antialiased bilinear resize of the shorter side to R (the longer one to floor(R*long/short)), the centre crop with
 * its origin rounded half to even, then v / 127.5 - 1.  src: tightly packed HWC images (row stride 3*w); off[b]: byte offset
 * of image b, any alignment; hw[b] = {h, w}, 1 <= h, w <= 65535 (an image outside that range is skipped: nothing is written
 * for it); the caller guarantees off[b] + 3*h*w <= size of src - every read lies inside that range of its own image.
 * out_kind 0: bf16 [B*R*R][8] NHWC, channels 3..7 exact zeros, 16-byte aligned (what the VAE encoder's conv_in reads);
 * out_kind 1: fp32 [B][3][R][R].  Kind 0 is the round-to-nearest-even bf16 of kind 1's value.  Filter weights are exact
 * integers and the sums run in fp64 (a constant image stays exactly constant); unlike PIL nothing is rounded to uint8
 * between the passes, so the result is within one uint8 step (2/255) of the reference pipeline.  No workspace.
 * DA_ERR_SHAPE for B < 1, R outside 1..4096, an unknown out_kind or a misaligned out. */
int da_image_ingest(const unsigned char* src, const long long* off, const int* hw, int B, int R, void* out, int out_kind,
                    da_stream_t stream);
/* The da_image_ingest contract for a rectangular target of Rh rows x Rw columns: resize to cover, then centre crop.  With
 * w*Rh <= h*Rw the width is resized to Rw and the height to floor(Rw*h/w), else the height to Rh and the width to
 * floor(Rh*w/h), so the resized image is never smaller than the target on either axis; the crop origin per axis is
 * round((n - R)/2), halves rounded to even.  Same filter, arithmetic and argument rules.
 * out_kind 0: bf16 [B*Rh*Rw][8] NHWC, 16-byte aligned; out_kind 1: fp32 [B][3][Rh][Rw].  At Rh == Rw == R every bit of
 * either output is da_image_ingest's.  DA_ERR_SHAPE for B < 1, Rh or Rw outside 1..4096, an unknown out_kind or a
 * misaligned out. */
int da_image_ingest_rect(const unsigned char* src, const long long* off, const int* hw, int B, int Rh, int Rw, void* out,
                         int out_kind, da_stream_t stream);
/* da_image_ingest_rect with the crop window and a horizontal flip chosen per image (random-crop / flip augmentation).  aug
 * is a device table int32 [B][3] = (top, left, flip): the origins are in pixels of the resized (nh x nw) image,
 * 0 <= top <= nh - Rh and 0 <= left <= nw - Rw, and out[Y][X] = resized[top + Y][c] with c = left + X for flip 0 and
 * c = nw - 1 - (left + X) for flip 1, which is the crop at `left` of the horizontally mirrored image.  The kernel clamps
 * both origins into range, so no table makes it read outside an image; an image whose flip is neither 0 nor 1 is skipped
 * (nothing written for it), as one with a side above 65535 is.  The centre origins of da_image_ingest_rect with flip 0
 * give its bits; flip 1 gives the bits of the mirrored source.  Resize rule, filter, arithmetic, outputs and argument
 * rules are da_image_ingest_rect's.  DA_ERR_SHAPE (nothing launched) for a null aug and for everything
 * da_image_ingest_rect rejects.  The table lives on the device: callers validate it on their host copy (ops.py does). */
int da_image_ingest_aug(const unsigned char* src, const long long* off, const int* hw, const int* aug, int B, int Rh,
                        int Rw, void* out, int out_kind, da_stream_t stream);
/* The same kernel with the transform as three independent switches (every combination is valid); src, off, hw, out and
 * out_kind are da_image_ingest_rect's, and da_image_ingest_rect is this entry with (0, 0, 0).
 *   geometry 0: resize to cover Rh x Rw, then the centre crop;  1: stretch, each axis resized on its own to Rw and Rh;
 *   filter   0: the antialiased triangle filter (Pillow's; F.interpolate(mode='bilinear', antialias=True));
 *            1: two-tap bilinear, F.interpolate(mode='bilinear', align_corners=False, antialias=False): for output index
 *               i of an n_in -> n_out axis num = max((2i+1) n_in - n_out, 0), i0 = num / (2 n_out), r = num - 2 n_out i0,
 *               weights (2 n_out - r) / (2 n_out) on i0 and r / (2 n_out) on min(i0 + 1, n_in - 1);
 *   range    0: v / 127.5 - 1 (ToTensor + Normalize(0.5, 0.5));  1: v / 255 (ToTensor alone): a constant image of level c
 *               comes out as exactly float(c) / float(255).
 * Weights are exact integers and the sums run in fp64 for both filters.  DA_ERR_SHAPE (nothing launched) for any other
 * value of geometry, filter or range, and for everything da_image_ingest_rect rejects. */
int da_image_resize(const unsigned char* src, const long long* off, const int* hw, int B, int Rh, int Rw, void* out,
                    int out_kind, int geometry, int filter, int range, da_stream_t stream);

/* F.mse_loss(pred, target) (stable_diffusion.py:187) over the 4 valid channels of NHWC(8) fp32 tensors and its
 * gradient dpred = grad_coef * (pred - target) (bf16, NHWC(8)).  loss[0] (+)= weight * mean.  scratch >= 1024 floats;
 * pred, target, dpred 16-byte aligned (DA_ERR_SHAPE otherwise). */
int da_mse_loss(const float* pred, const float* target, void* dpred, float* loss, float* scratch, long total_pix,
                float grad_coef, float weight, int accumulate, da_stream_t stream);
/* the da_mse_loss contract over C = 1..8 valid channels (the 3-channel pixel models' F.mse_loss, pixel_diffusion.py:98):
 * the mean is over total_pix * C values; dpred is exactly 0 in channels C..7, so the padded conv_out rows get a zero
 * gradient.  pred, target, dpred 16-byte aligned; DA_ERR_SHAPE for C outside 1..8. */
int da_mse_loss_c(const float* pred, const float* target, void* dpred, float* loss, float* scratch, long total_pix,
                  int C, float grad_coef, float weight, int accumulate, da_stream_t stream);
/* the da_mse_loss_c contract with a weight per sample, looked up by the sample's timestep (Min-SNR-gamma weighting, Hang et
 * al., arXiv:2303.09556): with b = pixel / HW and w_b = wtab[t[b]],
 *   dpred = grad_coef * w_b * (pred - target)  (bf16, exactly 0 in channels C..7),
 *   loss[0] (+)= weight * (1 / (C * total_pix)) * sum_b w_b sum (pred - target)^2.
 * t (int64 [total_pix / HW]) and wtab (fp32 [T]) are DEVICE pointers, so the launch can sit in a captured graph.  A timestep
 * outside [0, T) is clamped into the table, never read outside it.  Same two launches and fixed summation order as
 * da_mse_loss_c (two calls give the same bits; scratch >= 1024 floats); with a table of ones dpred and the loss are
 * da_mse_loss_c's bits.  DA_ERR_SHAPE for total_pix no multiple of HW, HW <= 0, T <= 0, a NULL t or wtab, C outside 1..8, or
 * a misaligned pred / target / dpred. */
int da_mse_loss_w(const float* pred, const float* target, void* dpred, float* loss, float* scratch, long total_pix, int C,
                  int HW, const long long* t, const float* wtab, int T, float grad_coef, float weight, int accumulate,
                  da_stream_t stream);

/* torch.optim.AdamW step (train.py:33; SD-2-base-256.yaml:55-58) on flat fp32 master/moment buffers, gradient
 * pre-scaled by grad_scale; also writes the bf16 compute shadow.  If ema != NULL the exponential moving average of
 * the weights (diffusion/algorithms/ema.py:26-76 compute_ema: ema = s*ema + (1-s)*w) is updated in the same pass. */
int da_adamw(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_smoothing, long n,
             float lr, float beta1, float beta2, float eps, float wd, int step, float grad_scale, da_stream_t stream);

/* The device record the gradient-norm pass writes and da_adamw_dev reads (8 words, 4-byte aligned):
 *   sumsq          sum of squares of the raw buffer (all segments)
 *   norm           sqrt(sumsq) * grad_scale: the global gradient norm (grad_scale = 1 / world: the buffer holds the rank sum)
 *   grad_mult      the gradient multiplier AdamW is to use: grad_scale * min(1, max_norm / (norm + 1e-6)), which is
 *                  torch.nn.utils.clip_grad_norm_'s rule; exactly grad_scale when max_norm <= 0 or norm <= max_norm
 *                  (norm and grad_mult are worked out in fp64 from the fp64 total and rounded once; "norm <= max_norm" is
 *                  decided on the fp32 norm stored here)
 *   finite         1.0 when sumsq is finite, else 0.0 (da_adamw_dev then leaves every buffer untouched)
 *   skipped_steps  incremented by one each time a pass finds sumsq non-finite; the owner zeroes it once */
#define DA_SUMSQ_CHUNK 8192 /* floats per chunk of da_segment_sumsq: the host's chunk tables are cut to this */
typedef struct DaGradStats {
  float sumsq, norm, grad_mult, finite;
  int skipped_steps;
  int reserved[3];
} DaGradStats;

/* Sum of squares of every segment of a flat fp32 buffer, their total, and the clip coefficient / step guard derived from
 * it (Composer's GradientClipping(clipping_type='norm'), OptimizerMonitor's l2_norm/grad metrics and the inf/NaN check of
 * the reference's GradScaler, train.py:118-128 + SD-2-base-256.yaml:80-81).  Nothing returns to the host.
 * A segment is a run (offset, numel) of x; the host cuts each into chunks of at most DA_SUMSQ_CHUNK floats that never cross
 * a segment.  chunk_desc: n_chunks records {long off (floats from x), int n, int seg}, segment-major in offset order;
 * seg_desc: n_segs records {int first_chunk, int n_chunks}.  Only words inside a chunk are read: whatever lies between
 * segments (alignment gaps) never enters a sum.  Up to three launches on `stream`, no atomics:
 *   1. chunk_partials[c] = fp32 sum of squares of chunk c (>= da_segment_sumsq_scratch_floats(n_chunks) floats);
 *   2. seg_sumsq[s] = the segment's partials summed in fp64, stored as fp32;
 *   3. stats (a DaGradStats, may be NULL: launch 3 is then left out) from the fp64 sum of seg_sumsq, grad_scale, max_norm.
 * Every sum's order is a function of the tables alone: the result does not depend on the grid, on "reserve_cus" or on
 * what else runs.  DA_ERR_SHAPE (nothing launched) for n_chunks <= 0, n_segs <= 0, a NULL table / output or x not 16-byte
 * aligned.  The tables are trusted: the caller guarantees every chunk lies inside x. */
int da_segment_sumsq(const float* x, const void* chunk_desc, int n_chunks, const void* seg_desc, int n_segs,
                     float* chunk_partials, float* seg_sumsq, float* stats, float grad_scale, float max_norm,
                     da_stream_t stream);
long da_segment_sumsq_scratch_floats(int n_chunks);

/* da_adamw with the gradient multiplier and a "skip this step" flag read from device memory: grad_scale = stats[2]
 * (DaGradStats.grad_mult), and when stats[3] (finite) is 0 the kernel returns without writing p, m, v, shadow or ema.  The
 * arithmetic is da_adamw's (one shared body).  `step` is the host's count and is used for the bias correction whether or
 * not the device skips.  Same rejections as da_adamw, plus a NULL stats. */
int da_adamw_dev(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_smoothing, long n,
                 float lr, float beta1, float beta2, float eps, float wd, int step, const float* stats, da_stream_t stream);

/* The reference's CLIPImageProcessor (scripts/fid-clip-evaluation.py: torchmetrics CLIPScore's processor) on planar uint8
 * images src [B, 3, H, W], all of one size: PIL's 8-bit bicubic resize of the shorter side to R, the centre crop to R x R,
 * * 1/255 and (x - mean[c]) / std[c] (mean, std: 3 HOST floats each).  The resampling is Pillow's integer arithmetic: the
 * host passes one coefficient table per axis, xtab [R][xld] / ytab [R][yld] int32 on the device, row i = {lo, count,
 * k[count]} for cropped output index i: first source index, tap count and the 22-bit fixed-point weights.  One pass is
 * clamp((2^21 + sum k * v) >> 22, 0, 255) in int32, horizontal first, rounded to a uint8 level between the passes.  lo and
 * count are clamped to the image and to the row length before use, so no table makes the kernel read outside src.
 *   out_kind 0: the patch matrix bf16 [B * (Np + 1)][Kp], Np = (R / P)^2, Kp = 3 P P rounded up to a multiple of 8; row
 *               b (Np + 1) is the class-token slot (zeros), row b (Np + 1) + 1 + py (R / P) + px, column c P P + iy P + ix is
 *               pixel (c, py P + iy, px P + ix); pad columns are zeros.  Every element is written exactly once.
 *   out_kind 1: the reference's pixel_values, fp32 [B, 3, R, R].
 * DA_ERR_SHAPE (nothing launched) for R % P != 0, P > 32, R > 448, sides outside 1..65535, xld / yld < 3, a NULL pointer
 * or out not 16-byte (kind 0) / 4-byte (kind 1) aligned. */
int da_clip_preprocess(const unsigned char* src, int B, int H, int W, int R, int P, const int* xtab, int xld,
                       const int* ytab, int yld, const float* mean, const float* std, void* out, int out_kind,
                       da_stream_t stream);

/* CLIP score of B (image, text) embedding pairs, fp32 rows of D values with leading dimensions ldi / ldt:
 * scores[i] = 100 * dot(a_i, b_i) / (|a_i| |b_i|) (no epsilon, no per-sample clamp: torchmetrics clamps the mean), then
 * state[0] += the scores summed in index order and state[1] += B.  One workgroup, every reduction in a fixed order: two runs
 * on the same inputs are bit-identical.  Nothing returns to the host. */
int da_clip_score(const float* img, long ldi, const float* txt, long ldt, int B, int D, float* scores, float* state,
                  da_stream_t stream);

/* ---- the FID metric: Inception-v3 tower (models/inception_hip.py) and float64 feature moments (metrics/fid.py) ----
 *
 * Convolution + folded BatchNorm + ReLU of the FID Inception network (torch-fidelity's FeatureExtractorInceptionV3: every
 * BasicConv2d is F.relu(bn(conv(x))), eps 1e-3; the BatchNorm is folded into W and bias at load time):
 *   Y[b, oh, ow, n] = act(bias[n] + sum_{i < kh, j < kw, c < Cin} X[b, oh s - ph + i, ow s - pw + j, c] W[n][i][j][c])
 * X: bf16 NHWC rows of ldx elements, Y: bf16 rows of ldy >= Cout elements (a branch writes its column slice of the block's
 * concat buffer, which replaces torch.cat), W: bf16 [Cout][kh][kw][Cin] contiguous, bias: fp32 [Cout] or NULL.  bf16 MFMA
 * with fp32 accumulation over k = (i, j, c) in that order, + bias in fp32, ReLU if relu = 1, one RNE rounding to bf16.
 * kh, kw in 1..7, stride 1 or 2, ph, pw in 0..3, Cin % 8 == 0, Cout % 8 == 0, ldx % 8 == 0, ldy % 8 == 0; X, W, Y and
 * bias 16-byte aligned.  Hout and Wout must equal (Hin + 2 ph - kh) / s + 1 and (Win + 2 pw - kw) / s + 1 (floor; the
 * padded image must hold one window).  tile_n: 0 takes the column tile da_conv2d_tile_for(Cout) picks, 32 / 64 / 96
 * force one (the summation order of an output element does not depend on the tile).  No workspace, no host synchronisation.  DA_ERR_SHAPE (nothing launched) for anything else, and for
 * B Hout Wout or B Hin Win >= 2^31. */
int da_conv2d_relu_fwd(const void* X, long ldx, const void* W, const float* bias, void* Y, long ldy, int B, int Hin,
                       int Win, int Hout, int Wout, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw,
                       int relu, int tile_n, da_stream_t stream);
/* the column tile (32, 64 or 96) da_conv2d_relu_fwd uses for Cout at tile_n = 0; 0 for a Cout it rejects */
int da_conv2d_tile_for(int Cout);

/* F.max_pool2d(x, 3, stride) (kind 0) and F.avg_pool2d(x, 3, stride, padding, count_include_pad=False) (kind 1) on bf16
 * NHWC rows: stride 1 or 2, pad 0 or 1, C % 8 == 0, ldx, ldy >= C and multiples of 8, Hout = (Hin + 2 pad - 3) / s + 1.
 * The average is the fp32 sum of the in-bounds taps in row-major tap order, one fp32 DIVISION by their count (not a
 * reciprocal multiply), one RNE rounding to bf16.  The maximum ignores taps outside the image. */
int da_pool2d_fwd(const void* X, long ldx, void* Y, long ldy, int B, int Hin, int Win, int Hout, int Wout, int C,
                  int stride, int pad, int kind, da_stream_t stream);

/* F.adaptive_avg_pool2d(x, 1) of bf16 NHWC rows into fp32: out[b][c] = (sum over the HW rows of image b, in row order,
 * fp32) / HW.  out rows of ldo >= C floats. */
int da_avgpool_global_f32(const void* X, long ldx, float* out, long ldo, int B, int HW, int C, da_stream_t stream);

/* The input transform of the FID Inception (torch-fidelity: interpolate_bilinear_2d_like_tensorflow1x(x, (299, 299),
 * align_corners=False), then (x - 128) / 128) of planar images src [B, 3, H, W]: src_kind 0 uint8 levels, 1 fp32 in [0, 1]
 * turned into levels by floor(clamp(255 x, 0, 255)) (torchmetrics normalize=True: (x * 255).byte()).  Per axis
 * scale = float(in / 299), src = dst * scale in fp32 (no half-pixel offset), lo = floor(src), hi = min(lo + 1, in - 1);
 * fp32 lerp lo + (hi - lo) * frac along x on both rows, then along y; no antialiasing.  This is NOT da_image_resize's
 * filter.  out: bf16 [B * 299 * 299][8] NHWC, channels 3..7 zero, 16-byte aligned. */
int da_inception_preprocess(const void* src, int src_kind, int B, int H, int W, void* out, da_stream_t stream);

/* torchmetrics' FID state update on fp32 features F [B][D] (rows of ldf floats, ldf % 4 == 0, 16-byte aligned):
 * sum[d] += sum_b F[b][d], cov[d][e] += sum_b F[b][d] F[b][e], n[0] += B, all float64 in device memory (sum [D], cov
 * [D][D], n [1]).  Every output element is owned by one thread that adds the batch in index order to the stored value:
 * no atomics, identical bits run to run.  D % 8 == 0, D <= 16384. */
int da_feature_moments(const float* F, long ldf, int B, int D, double* sum, double* cov, double* n, da_stream_t stream);

/* torch-fidelity's `logits_unbiased` head of the FID Inception (F.linear(features, fc.weight), no bias), which
 * torchmetrics' InceptionScore(feature='logits_unbiased') runs: out[b][c] = sum_k F[b][k] W[c][k].  F fp32 [B][K] (rows of
 * ldf floats, ldf % 4 == 0), W fp32 [C][K] contiguous, out fp32 [B][C] (rows of ldo >= C floats); F and W 16-byte aligned.
 * The sum is float64 FMAs in an order fixed by K alone, rounded once to fp32.  K % 4 == 0, any C >= 1. */
int da_fc_logits_f32(const float* F, long ldf, const float* W, float* out, long ldo, int B, int K, int C,
                     da_stream_t stream);

/* torchmetrics' InceptionScore.compute() after its permutation: rows perm[0..N) of logits fp32 [.][C] (rows of ld floats;
 * the row offset perm[i] * ld is 64-bit) are cut as torch.chunk(splits) does - chunks of ceil(N / splits) rows, the last
 * may be short and there may be fewer than `splits` - and per chunk p = softmax(row) (float64 log-softmax with the
 * maximum subtracted), m = mean_i p_i, score = exp(mean_i sum_c p_ic (log p_ic - log m_c)); terms with p_ic == 0 are 0.
 * scores float64 [splits] in device memory, the first *chunks entries are written; *chunks (host memory) is set before
 * returning.  perm int32 [N] in device memory, every entry a valid row: the caller checks that.  1 <= C <= 4096.  Fixed
 * summation order, no atomics. */
int da_inception_score(const float* logits, long ld, const int* perm, int N, int C, int splits, double* scores, int* chunks,
                       da_stream_t stream);

/* the number of float64 elements da_poly_mmd needs in ws for (subsets, m); 0 for a pair it rejects */
long da_poly_mmd_workspace(int subsets, int m);

/* torchmetrics' KernelInceptionDistance.compute() per subset (poly_mmd of poly_kernel blocks): with x_i = Fr[idx_r[s][i]],
 * y_j = Ff[idx_f[s][j]] and k(a, b) = (gamma <a, b> + coef)^degree,
 *   out[s] = (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m (m - 1)) - 2 sum_{i, j} k(x_i, y_j) / m^2.
 * Fr fp32 [Nr][D], Ff fp32 [Nf][D] (rows of ldr / ldf floats, multiples of 4, 16-byte aligned bases; row offsets are
 * 64-bit), idx_r, idx_f int32 [subsets][m] in device memory with 0 <= idx < Nr / Nf: the caller checks that.  Dot products
 * and sums are float64 (v_mfma_f64_16x16x4_f64 over rows gathered into LDS, no gathered copy in memory); the diagonal is
 * skipped, not subtracted; per-tile sums go to ws and are added in tile order: identical bits run to run.  out float64
 * [subsets].  2 <= m <= 65536, subsets <= 65535, D % 4 == 0, 1 <= degree <= 8, gamma > 0, coef >= 0,
 * ws_doubles >= da_poly_mmd_workspace(subsets, m). */
int da_poly_mmd(const float* Fr, long ldr, int Nr, const float* Ff, long ldf, int Nf, const int* idx_r, const int* idx_f,
                int subsets, int m, int D, int degree, double gamma, double coef, double* out, double* ws, long ws_doubles,
                da_stream_t stream);

int da_cast_f32_bf16(const float* src, void* dst, long n, da_stream_t stream);

/* dst[c][T-1-t][n] = src[n][t][c]: the weight layout da_gemm_nt needs for dgrad */
int da_transpose_weight(const void* src, void* dst, int N, int T, int C, da_stream_t stream);

/* the same for many tensors in one launch.  desc: device array of ntensors records
 * {long src_off, long dst_off (elements from the bases), int N, int T, int C, int first_block}; tensor i owns blocks
 * [first_block_i, first_block_i + T*ceil(N/64)*ceil(C/64)); total_blocks = their sum. */
int da_transpose_weights_batched(const void* src_base, void* dst_base, const void* desc, int ntensors, int total_blocks,
                                 da_stream_t stream);

/* ---- LoRA adapters on the merged-shadow path (csrc/lora.hip, diffusion_amd/lora.py) ----
 *
 * One adapted matrix: W [N][K] is a contiguous row range of a storage of the flat master / shadow / grad buffers (K = T C in
 * the kernel layout of a weight, ld = K always), A [r][K] and B [N][r] live in a flat fp32 adapter buffer.  All offsets are
 * 64-bit element counts from the bases (the flat fp32 buffer is 3.46 GB).  first_merge / first_da / first_db: the item's
 * first workgroup in the three tile families, running sums in item order of
 *   merge  ceil(N / 32) ceil(K / 128)      dA  ceil(r / 32) ceil(K / 128)      dB  ceil(N / 32)
 * The host builds the table once and uploads it (ops.LoraTables checks every item against the buffers; the kernels trust
 * it, as da_segment_sumsq trusts its tables).  1 <= r <= 128. */
typedef struct DaLoraItem {
  long long w_off, a_off, b_off;
  int N, K, r;
  float scale;
  int first_merge, first_da, first_db, reserved;
} DaLoraItem;

/* shadow[w_off + n K + k] = bf16_rne(v), v = master[...] + scale * sum_j B[n][j] A[j][k] for every item, one launch.  The
 * sum is an fp32 fmaf chain from 0 with j ascending (f32-input MFMA), then one fmaf onto the master value; a sum that is
 * exactly 0 leaves v = the master value, so B = 0 reproduces da_cast_f32_bf16 bit for bit.  vout (may be NULL; may be
 * master itself) receives the same v in fp32 at the same offsets: a master fused this way casts to these shadow bits.  Only
 * elements of the items' row ranges are written.  Ragged tiles and an r that is odd or no multiple of the chunk are zero
 * padded in LDS, never in memory.  DA_ERR_SHAPE (nothing launched) for n_items <= 0, total_tiles <= 0 (= the sum of the
 * items' merge tiles), a NULL master / adapters / items / shadow, fp32 pointers not 4-byte or items not 8-byte aligned. */
int da_lora_merge(const float* master, const float* adapters, const void* items, int n_items, int total_tiles,
                  void* shadow, float* vout, da_stream_t stream);

/* The adapter gradients from the dense weight gradient dW (fp32, at w_off of grad), one launch, OVERWRITING adapter_grad
 * at the items' a_off / b_off:  dA[j][k] = scale * sum_n B[n][j] dW[n][k],  dB[n][j] = scale * sum_k dW[n][k] A[j][k].
 * Since W' = W + scale B A this is exactly the chain rule.  Every output element is owned by one lane and is one fp32 fmaf
 * chain from 0 over the ascending reduction index, times scale: no atomics, nothing depends on the grid or on
 * "reserve_cus", two runs give identical bits.  tiles_da / tiles_db: the sums of the items' tiles of the two families.
 * DA_ERR_SHAPE (nothing launched) for non-positive counts, a NULL pointer, adapter_grad == adapters, misaligned pointers. */
int da_lora_project(const float* grad, const float* adapters, const void* items, int n_items, int tiles_da, int tiles_db,
                    float* adapter_grad, da_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
