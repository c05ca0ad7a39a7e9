/*
 * libebc_hip.so — C-ABI of the MI355X-native CLIP-EBC hot path (gfx950 / CDNA4).
 *
 * The reference (Yiming-M/CLIP-EBC) is pure Python on PyTorch; it has no FFI.  Its boundary
 * is the Python API.  These entry points are what that API binds to through
 * ctypes (clip-ebc_amd/ebc_amd/_lib.py); each cites the reference interface it replaces.
 *
 * Conventions (all entry points):
 *   - every pointer is caller-owned DEVICE memory (torch-allocated), except where noted;
 *   - no allocation, no host<->device synchronisation, no device sync inside a call; work is
 *     enqueued on `stream` (a hipStream_t passed as void*), so calls are graph-capturable;
 *   - return 0 (EBC_OK) or a negative EBC_E_* code; numerical roll-backs are reported per
 *     crop through `status`, never as an error;
 *   - `dtype` selects the GEMM/attention input type: EBC_F32 (parity mode, exact-f32 MFMA),
 *     EBC_F16 (the reference's AMP dtype) or EBC_BF16.
 */
#ifndef EBC_HIP_H
#define EBC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ebc_stream_t;

enum { EBC_F32 = 0, EBC_F16 = 1, EBC_BF16 = 2 };
enum { EBC_OK = 0, EBC_E_ARG = -1, EBC_E_LAUNCH = -2, EBC_E_UNSUPPORTED = -3 };
enum { EBC_COUNT_DMCOUNT = 0, EBC_COUNT_MAE = 1, EBC_COUNT_MSE = 2, EBC_COUNT_OT_ONLY = 3 };

/* Library version / self-description (host-only, no device work). */
int ebc_version(void);

/* ------------------------------------------------------------------------------------------
 * DACE loss with DMCount, fused, one workgroup per crop, all Sinkhorn iterations on device.
 *
 * Replaces DACELoss.forward (losses/dace_loss.py:49-70) with its DMLoss
 * (losses/dm_loss.py:99-124), OTLoss (losses/dm_loss.py:38-79) and
 * sinkhorn (losses/bregman_pytorch.py:11-144), forward AND backward:
 *   pred_class     [B, N, g, g] f32 logits      (g = size / reduction)
 *   pred_density   [B, 1, g, g] f32
 *   target_density [B, 1, size, size] f32 dot map (or already [B,1,g,g] if target_is_reduced)
 *   points         [sum(n_b), 2] f32 (x, y) pixels, packed;  offsets [B+1] int32 (device)
 *   bins_lo/hi     [N] f32 (device), inclusive bins; hi may be +inf
 *   order          [B] int32 (device) crop processing order (heaviest first), or NULL
 * Outputs:
 *   grad_class   [B, N, g, g]  d loss / d pred_class  (for upstream grad 1)
 *   grad_density [B, 1, g, g]  d loss / d pred_density
 *   losses       [5] f32: loss, ot_loss, tv_loss, count_loss, ce_loss (loss_info keys)
 *   crop_stats   [B, 8] f32: ce_b, tv_b*n_b, count_b, ot_b, wd_b, iters, rolled_back, err_last
 *   beta_out     [B, g*g] f32 or NULL;  status [B] int32 or NULL (iterations, negative = rollback)
 * count_mode: EBC_COUNT_DMCOUNT / _MAE / _MSE (DACELoss count_loss="dmcount"/"mae"/"mse"), or
 *   EBC_COUNT_OT_ONLY: OTLoss.forward alone (losses/dm_loss.py:38-79): grad_density = the OT gradient
 *   (weight_count_loss * weight_ot times it), losses[1] = sum of the crops' OT losses, no TV / count terms.
 * size / reduction (the density grid g) may be any integer up to 64 (e.g. 28 / 14 / 7 for 224 crops at reduction
 * 8 / 16 / 32, 56 / 28 / 14 for 448, 48 for 384 at 8, 64 for 512 at 8; the kernel runs on an LDS grid
 * G in {8,16,24,28,32,40,48,56,64} >= g whose extra cells are dead); EBC_E_UNSUPPORTED above 64.
 * grid cell k sits at k * reduction + reduction / 2 (dm_loss.py:31).
 * norm_cood: OTLoss norm_cood (dm_loss.py:31-34,51): coordinates mapped to [-1, 1].
 * workspace: ebc_dace_workspace_bytes(B, offsets[B], size, reduction) bytes of device memory.  A crop with more
 *   points than fit LDS (ebc_dace_plan's dense path 3) keeps its (2G + 6) * n_b factor floats there, at float
 *   offset (2G + 6) * offsets[b].  ebc_dace_loss_h knows the offsets and returns EBC_E_ARG, before any device work,
 *   when some crop can reach that path and workspace is NULL or workspace_bytes is below that size (and when the
 *   offsets decrease).  ebc_dace_loss cannot check it, its offsets being device memory: there a NULL or short
 *   workspace with such a crop is the caller's out-of-bounds write.  Crops that stay in LDS never touch it.
 */
size_t ebc_dace_workspace_bytes(int B, int total_points, int size, int reduction);
/* The plan the fused loss runs for one crop of n points at this geometry (host-only, no device work; computed by
 * the functions the launch and the kernel branch on): returns the LDS grid G in {8,16,24,28,32,40,48,56,64}, or 0
 * when the geometry is unsupported (reduction <= 0, size not a positive multiple of it, size / reduction > 64,
 * n < 0), and writes out[6] (out may be NULL):
 *   out[0]  the Sinkhorn path tried first: 0 bucketed with full factor rows, 1 bucketed with compact 12-cell rows,
 *           2 dense in LDS, 3 dense from the workspace (a crop with n = 0 runs no Sinkhorn at all);
 *   out[1]  lanes per 4x4 cell block of the bucketed path (8 or 16), 0 when out[0] is dense;
 *   out[2]  the dense path (2 or 3) taken when the bucketed one refuses the crop (a factor window wider than 9
 *           cells), and by out[0] >= 2 itself;
 *   out[3]  lds_cap_s: most points of path 0;  out[4]  lds_cap_c: most points of path 1 (equal to lds_cap_s where
 *           compact rows are no shorter, G = 8);  out[5]  lds_cap: most points of path 2. */
int ebc_dace_plan(int size, int reduction, int n, int* out);
/* a_out[i] = a[i] * *s, b_out[i] = b[i] * *s (s a device scalar): the loss gradients times the upstream gradient of the
 * loss (GradScaler's scale) in one launch */
int ebc_scale2(const float* s, const float* a, float* a_out, long na, const float* b, float* b_out, long nb,
               ebc_stream_t stream);
int ebc_dace_loss(const float* pred_class, const float* pred_density, const float* target_density,
                  int target_is_reduced, const float* points, const int* offsets, const int* order,
                  const float* bins_lo, const float* bins_hi, int B, int N, int size, int reduction,
                  int count_mode, int norm_cood, float weight_count_loss, float weight_ot, float weight_tv,
                  float reg, int max_iter, float stop_thr, int eval_freq,
                  float* grad_class, float* grad_density, float* losses, float* crop_stats,
                  float* beta_out, int* status, void* workspace, size_t workspace_bytes,
                  ebc_stream_t stream);
/* The same with the crop offsets [B+1] and order [B] in HOST memory (B <= 64): passed to the kernel as launch
 * arguments, so the label metadata needs no host-to-device copy. */
int ebc_dace_loss_h(const float* pred_class, const float* pred_density, const float* target_density,
                    int target_is_reduced, const float* points, const int* offsets_host, const int* order_host,
                    const float* bins_lo, const float* bins_hi, int B, int N, int size, int reduction,
                    int count_mode, int norm_cood, float weight_count_loss, float weight_ot, float weight_tv,
                    float reg, int max_iter, float stop_thr, int eval_freq,
                    float* grad_class, float* grad_density, float* losses, float* crop_stats,
                    float* beta_out, int* status, void* workspace, size_t workspace_bytes,
                    ebc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * General dense Sinkhorn-Knopp, one problem: replaces sinkhorn(a, b, C, reg, maxIter, stopThr, verbose,
 * log, eval_freq, print_freq) (losses/bregman_pytorch.py:11-144) for callers of that function itself
 * (the DMCount path uses ebc_dace_loss, whose cost is separable).  a [na], b [nb], C [na, nb] f32.
 * Outputs (each may be NULL except info): P [na, nb] = u K v; u [na], v [nb]; alpha = reg log(u + 1e-16),
 * beta = reg log(v + 1e-16); err [ceil(max_iter / eval_freq)] (the log's err list, only when log != 0);
 * info [2] int32 = {iterations run (negative: NaN/Inf rollback at that iteration), err entries}.
 * workspace: ebc_sinkhorn_workspace_bytes(na, nb) bytes (0 when K fits LDS).  EBC_E_UNSUPPORTED when
 * u and v together exceed LDS (na + nb beyond ~20000). */
size_t ebc_sinkhorn_workspace_bytes(int na, int nb);
int ebc_sinkhorn(const float* a, const float* b, const float* C, int na, int nb, float reg, int max_iter,
                 float stop_thr, int eval_freq, int log, float* P, float* u, float* v, float* alpha, float* beta,
                 float* err, int* info, void* workspace, size_t workspace_bytes, ebc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = A[M,K] . B[N,K]^T (+bias[N]) with a fused epilogue.  A, B of `dtype`; K % 64 == 0
 * (K % 32 for f32), N % 64 == 0.  Replaces the nn.Linear / nn.MultiheadAttention projections of
 * ResidualAttentionBlock (models/clip/_clip/blocks.py:22-42), the patch-embed conv1
 * (image_encoder.py:141, as im2col-GEMM) and the 1x1 projection (models/clip/model.py:91-95).
 *   epilogue 0 STORE:    C = acc + bias                      (C of dtype, or f32 if out_f32)
 *   epilogue 1 GELU:     aux = acc + bias; C = QuickGELU(aux) (blocks.py:17-19)
 *   epilogue 2 RESID:    C = resid(f32) + acc + bias          (C f32: the residual stream, may be in place;
 *                                                              C in dtype when !out_f32)
 *   epilogue 3 GELU_BWD: C = acc * QuickGELU'(aux)           (MLP backward, dX only)
 * bias may be NULL (none); aux may be NULL for GELU (the pre-activation is not kept).
 * EBC_E_ARG, before any device work: an epilogue outside EBC_EPI_STORE .. EBC_EPI_GELU_BWD, a dtype that is none of
 * EBC_F32 / EBC_F16 / EBC_BF16, M, N or K <= 0, K % 64 (K % 32 for f32) or N % 64 nonzero, NULL A / B / C, RESID
 * without resid, GELU_BWD without aux.  EBC_E_UNSUPPORTED, before any device work: GELU or GELU_BWD with out_f32 on
 * a 16-bit dtype.
 */
enum { EBC_EPI_STORE = 0, EBC_EPI_GELU = 1, EBC_EPI_RESID = 2, EBC_EPI_GELU_BWD = 3 };
int ebc_gemm(int dtype, int epilogue, int out_f32, const void* A, const void* B, void* C,
             const float* bias, const float* resid, void* aux, int M, int N, int K, ebc_stream_t stream);
/* The STORE product with a row-mapped A operand: output row r reads A row
 * (r / rows_per_group) * group_stride + group_offset + r % rows_per_group (rows_per_group 0: row r), e.g. the prompt
 * rows 1 .. P of every crop's L token rows (rows_per_group P, group_stride L, group_offset 1).  C [M][N] is dense.
 * EBC_E_ARG, before any device work: what ebc_gemm rejects, rows_per_group < 0, and rows_per_group > 0 with
 * group_offset < 0 or group_offset + rows_per_group > group_stride. */
int ebc_gemm_rows(int dtype, int out_f32, const void* A, const void* B, void* C, const float* bias, int M, int N, int K,
                  int rows_per_group, int group_stride, int group_offset, ebc_stream_t stream);
/* The tile configuration ebc_gemm dispatches for this shape (host-only, no device work): returns the
 * configuration id (> 0; a function of dtype and shape alone) and writes out[3] = {tile rows, tile columns, 1}
 * (these products never split K).  Lets tests pin which kernel instance a shape runs. */
int ebc_gemm_tile_config(int dtype, int M, int N, int K, int* out);
/* Weight-gradient GEMM for a long reduction (K = pixels), f32 output:  C[M,N] = A[M,K] . B[N,K]^T
 * with A, B in `dtype` (K-contiguous: the transposed activations / output gradients).  Replaces the
 * projection's dW = dZ^T Y of models/clip/model.py:91-95 (nn.Conv2d 1x1 backward).  Splits K over
 * workgroups (deterministic last-arriver sum).  `workspace` (>= ebc_gemm_wgrad_workspace_bytes; 0 = no
 * split for this shape) must be zero-filled before its first use and is then owned by the stream: every
 * call leaves its leading 16 KiB counter block zero again, the rest is scratch.
 * EBC_E_ARG, before any device work: NULL A / B / C, a bad dtype, M, N or K <= 0, K % 64 (K % 32 for f32) or N % 64
 * nonzero, and a shape whose plan splits K with a workspace that is NULL or smaller than
 * ebc_gemm_wgrad_workspace_bytes. */
size_t ebc_gemm_wgrad_workspace_bytes(int dtype, int M, int N, int K);
int ebc_gemm_wgrad(int dtype, const void* A, const void* B, float* C, int M, int N, int K,
                   void* workspace, size_t workspace_bytes, ebc_stream_t stream);
/* The plan ebc_gemm_wgrad runs for this shape (host-only, no device work; mirrors ebc_gemm_tile_config): returns the
 * tile configuration id and writes out[3] = {tile rows, tile columns, splits}: splits 1 = K is not split, 2 = two
 * pieces summed by the last one to arrive, negative = -splits pieces stored as f32 partials and summed by a reduce
 * launch. */
int ebc_gemm_wgrad_tile_config(int dtype, int M, int N, int K, int* out);
/* out[c][r] = in[r][c] for in [R][C] (16-bit or f32 elements; C and the output row stride ld_out >= R
 * multiples of 8, any R): the K-contiguous operand copies for ebc_gemm_wgrad.  Columns r >= R of out are left as they
 * are.  EBC_E_ARG, before any device work: NULL in / out, a bad dtype, R or C <= 0, C % 8, ld_out < R, ld_out % 8. */
int ebc_transpose(int dtype, const void* in, void* out, int R, int C, long ld_out, ebc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLIP ViT-B/16 and ViT-B/32 + deep VPT encoder: CLIP_EBC._forward_vpt (models/clip/model.py:142-189), whole
 * forward and dX-only backward (frozen encoder: gradients reach the VPT tokens only), one call each.
 * Weight pointers are device memory of `dtype` (matrices, nn.Linear [out, in] layout) or f32
 * (biases, LayerNorm, embeddings); wt_* are the transposed matrices [in, out] used by backward.
 * The EbcVitWeights / EbcVitLayer structs themselves live in HOST memory.
 */
typedef struct {
    const void* w_qkv;  const float* b_qkv;    /* attn.in_proj_weight [2304,768], in_proj_bias */
    const void* w_out;  const float* b_out;    /* attn.out_proj [768,768] */
    const void* w_fc;   const float* b_fc;     /* mlp.c_fc [3072,768] */
    const void* w_proj; const float* b_proj;   /* mlp.c_proj [768,3072] */
    const float* ln1_g; const float* ln1_b; const float* ln2_g; const float* ln2_b;
    const void* wt_qkv; const void* wt_out; const void* wt_fc; const void* wt_proj;   /* transposes */
    /* optional (16-bit; all null: ln_1 / ln_2 run as LayerNorm launches): ln_1 / ln_2 folded into the QKV / c_fc
     * products -- the weight rows pre-scaled by gamma (W' = W diag(gamma), [out, 768] in dtype), the folded bias
     * b + W beta and the row sums W'.1 (f32 [out]); the layer's input rows are then normalised in those products'
     * epilogues from row statistics the previous residual product writes */
    const void* w_qkv_ln; const float* b_qkv_ln; const float* s_qkv_ln;
    const void* w_fc_ln;  const float* b_fc_ln;  const float* s_fc_ln;
    /* optional (16-bit, with the fold above; null: LayerNorm-backward launches): the transposes of the folded weights,
     * (W')^T [768, out], so the dX products after the GELU' / attention backward produce g = dX_ln (.) gamma and finish
     * the LayerNorm backward in their epilogues (row sums from the GELU' product's partials, vit.hip) */
    const void* wt_qkv_ln; const void* wt_fc_ln;
} EbcVitLayer;

typedef struct {
    int layers, width, heads, patch, num_vpt;   /* width 768, heads 12; patch 16 (ViT-B/16) or 32 (ViT-B/32) */
    const void* w_patch;                        /* conv1.weight as [768, 3*patch*patch] */
    const float* cls;                           /* class_embedding [768] */
    const float* pos;                           /* positional_embedding [G+1, 768] for this input size */
    const float* ln_pre_g; const float* ln_pre_b; const float* ln_post_g; const float* ln_post_b;
    const EbcVitLayer* layer;                   /* host array [layers] */
} EbcVitWeights;

/* Workspace (device bytes) holding the saved activations (training) or the ping-pong buffers. */
size_t ebc_vit_workspace_bytes(int B, int H, int W, int layers, int num_vpt, int dtype, int training);
/* The same for a given patch size (16 or 32; the call above means 16): the token grid is (H/patch) x (W/patch) and the
 * patch rows are 3*patch*patch wide.  0 for a patch size the encoder does not take. */
size_t ebc_vit_workspace_bytes_p(int B, int H, int W, int patch, int layers, int num_vpt, int dtype, int training);
/* image [B,3,H,W] f32 (H, W multiples of w->patch) -> feat [B, (H/patch)*(W/patch), 768] f32 (= ln_post of the patch tokens, NHWC).
 * vpt: host array [layers] of device pointers ([num_vpt,768] f32, or [B,num_vpt,768] with
 * vpt_bstride = num_vpt*768 elements for per-crop prompts); vpt[l] == NULL for l > 0 keeps the
 * previous block's prompt outputs (shallow VPT, model.py:177-178). */
int ebc_vit_forward(const EbcVitWeights* w, const float* image, int B, int H, int W,
                    const float* const* vpt, long vpt_bstride, int dtype, int training,
                    void* workspace, size_t workspace_bytes, float* feat, ebc_stream_t stream);
/* dfeat [B, G, 768] f32 -> dvpt[l] ([num_vpt,768] f32, summed over crops; per crop if vpt_bstride).
 * Layer 0's backward stops at its prompt rows (the frozen embedding below takes no gradient: dQ/dK/dV of the first
 * query/key block, dH and ln_1' of the prompt rows only); flags & EBC_VIT_BWD_FULL_LAYER0 runs it over every row
 * instead, which must give bit-identical prompt gradients (a parity hook for tests/test_gpu_model.py).
 * flags & EBC_VIT_BWD_NO_LN_FOLD runs ln_2's backward as a LayerNorm launch even when wt_fc_ln is set (A/B, tests). */
enum { EBC_VIT_BWD_FULL_LAYER0 = 1, EBC_VIT_BWD_NO_LN_FOLD = 2 };
int ebc_vit_backward(const EbcVitWeights* w, int B, int H, int W, int dtype, void* workspace,
                     size_t workspace_bytes, const float* dfeat, float* const* dvpt, long vpt_bstride, int flags,
                     ebc_stream_t stream);

/* LayerNorm over D = 768 (the ViT) or 512 (the text tower) channels (models/clip/_clip/blocks.py:8-14, fp32 math, eps
 * 1e-5); any other D: EBC_E_UNSUPPORTED.
 * Row r of the output reads input row (r / rows_per_group) * group_stride + group_offset +
 * r % rows_per_group (rows_per_group = 0: identity), e.g. ln_post on the patch rows only.
 * The map is one-sided: the forward reads x at the mapped row and writes out / out_f32 / mean / rstd dense (row r);
 * the backward reads dy, mean and rstd dense, and reads x and dx_in, and writes dx_out and dx_out_t, at the mapped
 * row (rows outside the groups are not written).  M need not be a multiple of rows_per_group.
 * Optional (NULL): one of out / out_f32, mean together with rstd (rstd alone is never written), dx_in (taken as 0),
 * dx_out_t.  dy_f32 != 0: dy is f32 whatever dtype is (dtype f32: always).
 * EBC_E_ARG, before any device work: NULL x / gamma / beta, out and out_f32 both NULL, mean without rstd; NULL dy / mean /
 * rstd / dx_out; rows_per_group > 0 with group_offset < 0 or group_offset + rows_per_group > group_stride. */
int ebc_layernorm_fwd(int dtype, const float* x, int rows_per_group, int group_stride, int group_offset,
                      const float* gamma, const float* beta, void* out, float* out_f32, float* mean,
                      float* rstd, int M, int D, ebc_stream_t stream);
int ebc_layernorm_bwd(int dtype, int dy_f32, const void* dy, const float* x, int rows_per_group,
                      int group_stride, int group_offset, const float* mean, const float* rstd,
                      const float* gamma, const float* dx_in, float* dx_out, void* dx_out_t, int M, int D,
                      ebc_stream_t stream);
/* Multi-head attention on the packed qkv [B*L, 3*H*64] (nn.MultiheadAttention, need_weights=False,
 * blocks.py:35-37): out [B*L, H*64], lse [B,H,L]; backward writes dqkv [B*L, 3*H*64].
 * L <= 256: K/V (and Q/dO) resident in LDS, one workgroup per (crop, head); 256 < L <= 16384 (the position
 * embedding interpolated for larger inputs, image_encoder.py:183-198): K/V streamed through LDS in 256-row chunks
 * with an online softmax; longer sequences return EBC_E_UNSUPPORTED.
 * lse may be NULL in the forward.  delta_ws [B,H,L] f32 (rowsum(dout * out)) is written and read by the f32 backward
 * at every L (its dQ kernel publishes it for the dK/dV kernel) and by the streamed backward (L > 256) of every dtype:
 * there NULL is EBC_E_ARG.  The 16-bit backward at L <= 256 (one workgroup per (crop, head), delta kept in LDS) never
 * touches it and takes NULL.  NULL qkv / out (forward) or qkv / dout / out / lse / dqkv (backward): EBC_E_ARG. */
int ebc_attention_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int L, int H, ebc_stream_t stream);
int ebc_attention_bwd(int dtype, const void* qkv, const void* dout, const void* out, const float* lse,
                      float* delta_ws, void* dqkv, int B, int L, int H, ebc_stream_t stream);
/* Blockwise image-text similarity head (head.hip; models/clip/model.py:200-217):
 * Z [P=B*HW, embed] projected features (NHWC rows) -> logits [B,NB,HW], exp [B,1,HW]; text [NB, embed];
 * embed = the CLIP joint width: 512 (ViT-B/16, ViT-B/32) or 1024 (ResNet-50), 1 <= NB <= EBC_HEAD_MAX_BINS (32: the
 * reference's largest bin table has 20).  Up to 16 bins run the 16-slot kernel instances, 17 .. 32 bins the 32-slot ones
 * (per-pixel register arrays of 32; normalised text rows in up to 64 KiB / 128 KiB of LDS at embed 512 / 1024, the
 * backward 16 KiB + 16 B more); NB outside 1 .. 32 or another embed is EBC_E_UNSUPPORTED before any device work.
 * Backward: dZ (element type dtype_dz), d projection bias (column sums), d logit_scale; gscale (device scalar) scales the
 * upstream gradients (NULL = 1).  d bias / d logit_scale are summed deterministically (per-block partials in `workspace`,
 * ebc_head_bwd_workspace_bytes(P, embed) bytes, reduced in block order); workspace may be NULL when both are NULL.
 * Replaces the autograd backward of model.py:198-217 (F.normalize, cosine logits x exp(logit_scale), softmax, expectation)
 * and the projection bias's column sum.
 * EBC_E_ARG, before any device work: P <= 0, HW <= 0 or P % HW != 0 (P is B whole images); NULL Z / text / logit_scale /
 * anchors / logits / expo (forward) or Z / text / logit_scale / anchors / dlogits / dexp / dZ (backward); dbias or dscale
 * given with a workspace that is NULL or too small.  ebc_cast_f32: NULL in / out, n % 4 != 0. */
#define EBC_HEAD_MAX_BINS 32
int ebc_head_fwd(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                 float* logits, float* expo, int P, int HW, int NB, int embed, ebc_stream_t stream);
size_t ebc_head_bwd_workspace_bytes(int P, int embed);
int ebc_head_bwd(int dtype_z, int dtype_dz, const void* Z, const float* text, const float* logit_scale,
                 const float* anchors, const float* dlogits, const float* dexp, const float* gscale, void* dZ,
                 float* dbias, float* dscale, int P, int HW, int NB, int embed, void* workspace, size_t workspace_bytes,
                 ebc_stream_t stream);
/* The head's gradient with respect to the text features, for a trainable text tower (freeze_text_encoder=False,
 * models/clip/model.py:201-208: text_encoder(text_prompts) runs in every forward and its output is normalised inside the
 * head, so the loss reaches every text parameter through it).  Same operands as ebc_head_bwd; writes
 *   dtext [NB, embed] f32 = d (logits, exp) / d text, the RAW rows (the F.normalize backward of each row is applied:
 *   dt_k = (g_k - tn_k <tn_k, g_k>) / max(||t_k||, 1e-12), g_k = exp(logit_scale) sum_p dl[p,k] zn_p; g_k / 1e-12 for a
 *   row whose norm is at or below the clamp).
 * Deterministic: per-workgroup partial sums in `workspace` (ebc_head_bwd_text_workspace_bytes(P, NB, embed) bytes, plain
 * stores), then a fixed-order sum; no float atomics.  A launch of its own: ebc_head_bwd and its outputs do not change.
 * EBC_E_ARG, before any device work: NULL Z / text / logit_scale / anchors / dlogits / dexp / dtext, P <= 0, HW <= 0,
 * P % HW != 0, a dtype_z that is none of the three, a workspace that is NULL or too small.  EBC_E_UNSUPPORTED, before any
 * device work: NB outside 1..16, embed other than 512 / 1024 (the workspace size of such a call is 0). */
size_t ebc_head_bwd_text_workspace_bytes(int P, int NB, int embed);
int ebc_head_bwd_text(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                      const float* dlogits, const float* dexp, const float* gscale, float* dtext, int P, int HW, int NB,
                      int embed, void* workspace, size_t workspace_bytes, ebc_stream_t stream);
/* ebc_head_bwd_text for up to EBC_HEAD_MAX_BINS bins: the same operands, the same dtext and the same contract (raw-row
 * gradient through the head's own F.normalize, g_k / 1e-12 on a clamped row, per-workgroup partials in plain stores
 * summed in a fixed order, no float atomics, ebc_head_bwd's outputs untouched, the same EBC_E_ARG cases), with
 * 1 <= NB <= 32 at embed 512 / 1024; EBC_E_UNSUPPORTED and a workspace size of 0 outside that.  ebc_head_bwd_text keeps
 * its 16-bin bound and its arithmetic; this entry point passes the normalised text rows through LDS in groups of
 * 16384 / embed rows, so its sums are formed in another order (equal within rounding, not bit-equal, at NB <= 16).
 * Workspace: ceil(P / 64) workgroup partials of (NB * embed + 32) floats each -- [NB][embed] sums of dl[p][k] zn_p,
 * then 32 slots of sum_p dl[p][k] logits[p][k] (slots k >= NB are zero):
 *   ebc_head_bwd_text_wide_workspace_bytes(P, NB, embed) = ceil(P / 64) * (NB * embed + 32) * 4.
 * (ebc_head_bwd_text's: ceil(P / 64) * (NB * embed + 16) * 4.) */
size_t ebc_head_bwd_text_wide_workspace_bytes(int P, int NB, int embed);
int ebc_head_bwd_text_wide(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                           const float* dlogits, const float* dexp, const float* gscale, float* dtext, int P, int HW, int NB,
                           int embed, void* workspace, size_t workspace_bytes, ebc_stream_t stream);
int ebc_cast_f32(int dtype, const float* in, void* out, size_t n, ebc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLIP text tower, trained (freeze_text_encoder=False, models/clip/model.py:100-115,201): CLIPTextEncoder
 * (models/clip/_clip/text_encoder.py:7-53) over ResidualAttentionBlock (blocks.py:22-42) with the causal mask
 * (text_encoder.py:33-39), forward and the backward of every parameter.  Width 512, 8 heads of 64, context <= 77.
 *
 * The text feature of prompt k is row eot_k of its tokens and the mask is causal, so rows past a prompt's EOT never reach
 * the output and take exactly zero gradient: the tower runs Lt = max_k eot_k + 1 tokens a prompt (ids [NB][Lt], the
 * first Lt of each prompt's context tokens).  This is exact.
 *
 * Kernels (text.hip).  No float atomics: every sum runs in a fixed order and two launches agree bit for bit.
 *   ebc_attention_causal_fwd / _bwd: ebc_attention_fwd / _bwd with keys j <= i only, L <= 77 (EBC_E_UNSUPPORTED above),
 *     one workgroup per (prompt, head); delta_ws is never touched (NULL is fine), lse may be NULL in the forward.
 *     EBC_E_ARG: NULL qkv / out (forward) or qkv / dout / out / lse / dqkv (backward), B, L or H <= 0, a bad dtype.
 *   ebc_layernorm_param_grad: dgamma[c] = sum_r dy[r][c] xhat[r][c], dbeta[c] = sum_r dy[r][c] over M dense rows, xhat =
 *     (x - mean[r]) rstd[r]; dy of dtype, or f32 when dy_f32.  D 512 or 768 (EBC_E_UNSUPPORTED otherwise); EBC_E_ARG: a
 *     NULL pointer, M <= 0, a bad dtype.
 *   ebc_colsum: out[c] = sum_r a[r][c] for a [M][N] of dtype (f32 when in_f32): the bias gradients.  EBC_E_ARG: NULL a /
 *     out, M or N <= 0, a bad dtype.
 *     Both sum rows r = g (mod 8) in ascending order for g = 0 .. 7, then the eight partial sums in that order.
 *   ebc_text_embed_fwd: x[p][t] = token_embedding[ids[p][t]] + positional_embedding[t] (text_encoder.py:42-44), t < Lt.
 *   ebc_text_embed_bwd: the dense gradients, every element written: dtoken [vocab][512], row v = the sum of the dx rows
 *     rows[offs[u] .. offs[u + 1]) in list order where v = uniq[u], zero for a v not in uniq; dpos [context][512], row t =
 *     sum_p dx[p][t] in prompt order, zero for t >= Lt.  uniq [nu] ascending, offs [nu + 1], rows [NB * Lt] (values p * Lt
 *     + t) are device arrays the caller builds once from the ids (the inverted index of the embedding gather).
 *     Both: EBC_E_ARG for a NULL pointer, vocab <= 0 (and context < Lt or > 77, nu outside 1 .. NB * Lt in the backward);
 *     EBC_E_UNSUPPORTED for NB outside 1 .. 16, Lt outside 1 .. 77, width other than 512. */
int ebc_attention_causal_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int L, int H, ebc_stream_t stream);
int ebc_attention_causal_bwd(int dtype, const void* qkv, const void* dout, const void* out, const float* lse,
                             float* delta_ws, void* dqkv, int B, int L, int H, ebc_stream_t stream);
int ebc_layernorm_param_grad(int dtype, int dy_f32, const void* dy, const float* x, const float* mean, const float* rstd,
                             float* dgamma, float* dbeta, int M, int D, ebc_stream_t stream);
int ebc_colsum(int dtype, int in_f32, const void* a, float* out, int M, int N, ebc_stream_t stream);
int ebc_text_embed_fwd(const float* token_embedding, const float* positional_embedding, const int* ids, float* x, int NB,
                       int Lt, int width, int vocab, ebc_stream_t stream);
int ebc_text_embed_bwd(const float* dx, const int* uniq, const int* offs, const int* rows, int nu, float* dtoken,
                       float* dpos, int NB, int Lt, int context, int width, int vocab, ebc_stream_t stream);

/* The whole tower, one call each way.  Every parameter is the f32 tensor being trained (device memory; the structs
 * themselves live in HOST memory): the parameters change every step, so each forward makes its compute-dtype and
 * transposed copies in the workspace.  The residual stream, its gradient and the LayerNorm statistics are f32, GEMM and
 * attention operands are of `dtype`.
 *   ids [NB][Lt] int32, eot [NB] int32 (the EOT position of each prompt, < Lt): device arrays.
 *   features [NB][embed] f32 = ln_final(x)[k, eot_k] @ text_projection (text_encoder.py:50-52).
 *   training 1 keeps every layer's activations in the workspace for ebc_text_backward, which must be given the same
 *   workspace, untouched, and the same w, ids, eot, NB, Lt and dtype; 0 keeps nothing.
 *   ebc_text_backward writes EVERY gradient in g (f32, the parameters' shapes; the embedding gradients dense, zero rows
 *   included) from dfeatures [NB][embed] f32; uniq / offs / rows / nu as for ebc_text_embed_bwd.
 * EBC_E_ARG, before any device work: a NULL pointer (structs, their fields, ids, eot, workspace, features / dfeatures, the
 * index arrays), layers <= 0, heads != 8, vocab <= 0, context < Lt or > 77, nu outside 1 .. NB * Lt, a bad dtype, a
 * workspace smaller than ebc_text_workspace_bytes.  EBC_E_UNSUPPORTED, before any device work: NB outside 1 .. 16, Lt
 * outside 1 .. 77, width other than 512, embed other than 512 / 1024 (the workspace size of such a call is 0). */
typedef struct {
    const float* w_qkv;  const float* b_qkv;    /* attn.in_proj_weight [1536,512], in_proj_bias */
    const float* w_out;  const float* b_out;    /* attn.out_proj [512,512] */
    const float* w_fc;   const float* b_fc;     /* mlp.c_fc [2048,512] */
    const float* w_proj; const float* b_proj;   /* mlp.c_proj [512,2048] */
    const float* ln1_g; const float* ln1_b; const float* ln2_g; const float* ln2_b;
} EbcTextLayer;
typedef struct {
    int layers, width, heads, embed, vocab, context;   /* width 512, heads 8, embed 512 | 1024, context <= 77 */
    const float* token_embedding;                      /* [vocab, 512] */
    const float* positional_embedding;                 /* [context, 512] */
    const float* ln_final_g; const float* ln_final_b;
    const float* text_projection;                      /* [512, embed] */
    const EbcTextLayer* layer;                         /* host array [layers] */
} EbcTextWeights;
typedef struct {
    float* w_qkv;  float* b_qkv;
    float* w_out;  float* b_out;
    float* w_fc;   float* b_fc;
    float* w_proj; float* b_proj;
    float* ln1_g; float* ln1_b; float* ln2_g; float* ln2_b;
} EbcTextLayerGrads;
typedef struct {
    float* token_embedding; float* positional_embedding; float* ln_final_g; float* ln_final_b; float* text_projection;
    const EbcTextLayerGrads* layer;                    /* host array [layers] */
} EbcTextGrads;
size_t ebc_text_workspace_bytes(int NB, int Lt, int layers, int embed, int dtype, int training);
int ebc_text_forward(const EbcTextWeights* w, const int* ids, const int* eot, int NB, int Lt, int dtype, int training,
                     void* workspace, size_t workspace_bytes, float* features, ebc_stream_t stream);
int ebc_text_backward(const EbcTextWeights* w, const EbcTextGrads* g, const int* ids, const int* eot, const int* uniq,
                      const int* offs, const int* rows, int nu, int NB, int Lt, int dtype, void* workspace,
                      size_t workspace_bytes, const float* dfeatures, ebc_stream_t stream);

/* Patch rows of the patch-embedding GEMM (conv1 as im2col-GEMM, image_encoder.py:141): x [B,3,H,W] f32 ->
 * out [B*(H/patch)*(W/patch), 3*patch*patch] of dtype, column k = c*patch*patch + kh*patch + kw (conv1.weight's
 * order); patch % 4 == 0 and 3*patch*patch <= 4096 (one float4 a lane, up to 1024 lanes a row). */
int ebc_im2col(int dtype, const float* x, void* out, int B, int H, int W, int patch, ebc_stream_t stream);

/* Sliding-window evaluation (utils/eval_utils.py:26-96).  Tiles t = i*cols + j, rows/cols =
 * ceil((H-wh)/sh)+1, last row/column snapped to the border.
 * gather:   tiles [tile_count, C, wh, ww] <- image [C, H, W], tiles tile_begin .. +tile_count
 * assemble: out [Cp, H/r, W/r] = per-pixel mean of preds [rows*cols, Cp, wh/r, ww/r] */
int ebc_tile_gather(const float* image, float* tiles, int C, int H, int W, int wh, int ww, int sh, int sw,
                    int tile_begin, int tile_count, ebc_stream_t stream);
int ebc_tile_assemble(const float* preds, float* out, int Cp, int H, int W, int wh, int ww, int sh, int sw,
                      int reduction, ebc_stream_t stream);

/* Evaluation of a split from raw images (datasets/crowd.py:141-162, datasets/transforms.py:69-134,
 * utils/eval_utils.py:26-96, eval.py:27).  One descriptor per image; the tile list is global and runs across the
 * images in order (image i owns tiles tile0 .. tile0 + rows*cols, tile0 = the tiles before it), so a model batch
 * may span images.  The tiling is ebc_tile_gather's, on the fitted size Hf x Wf (rows/cols = ceil((Hf-wh)/sh)+1).
 *   layout U8_HWC   [H][W][3] bytes (a decoded JPEG);  U8_CHW  [3][H][W] bytes (the reference's .npy images)
 *          F32_CHW  [3][H][W] f32 already normalised (a resized image: ebc_u8_to_chw01, then one ebc_augment_crops
 *                   descriptor whose crop is the whole image, out_h x out_w the fitted size, normalize = 1)
 * Both batch entry points take the descriptor array twice, on the device (what the kernels read) and on the host
 * (what the checks and the grid sizes read; only read during the call).
 * EBC_E_ARG, before any device work: a NULL pointer, Hf < wh or Wf < ww, Hf < H or Wf < W, a layout that is none of
 * the three, rows / cols / tile0 that are not the tiling's, a tile range outside the list, ww % 4, a src that is not
 * 4-byte or tiles that are not 16-byte aligned, an F32_CHW src_off % 4, and any size past int32 (3 Hf Wf of an
 * image, the tile count, 3 wh ww tile_count, the elements of preds or of the maps). */
enum { EBC_EVAL_U8_HWC = 0, EBC_EVAL_U8_CHW = 1, EBC_EVAL_F32_CHW = 2 };
typedef struct {
    int64_t src_off;                     /* byte offset of the image in src */
    int64_t map_off;                     /* element offset of its assembled map [Cp][Hf/r][Wf/r] in maps */
    int32_t H, W;                        /* stored size */
    int32_t Hf, Wf;                      /* fitted size (>= stored: the rest is ZeroPad2Multiple's right/bottom zeros) */
    int32_t tile0, rows, cols;
    int32_t layout;
} EbcEvalImage;
/* tiles [tile_count][3][wh][ww] f32 <- tiles tile_begin .. + tile_count of the global list.  u8 sources:
 * ((float)u / 255 - mean[c]) / std[c], three f32 operations, bit-equal to the reference's CPU tensors; pixels with
 * y >= H or x >= W are (0 - mean[c]) / std[c] (fill = 0 before Normalize).  mean / std: 3 host floats each.  src is
 * read in aligned dwords, so its allocation ends on a multiple of 4 bytes. */
int ebc_tiles_from_raw(const void* src, const EbcEvalImage* desc, const EbcEvalImage* desc_host, int n_images, int wh,
                       int ww, int sh, int sw, int tile_begin, int tile_count, const float* mean, const float* std,
                       float* tiles, ebc_stream_t stream);
/* out [3][H][W] f32 = u8 / 255 of one U8_HWC or U8_CHW image (crowd.py:144 / to_tensor): the resize branch's input.
 * EBC_E_ARG: NULL src / out, H or W <= 0, another layout, src or out not 4-byte aligned, 3 H W past int32. */
int ebc_u8_to_chw01(const void* src, int layout, int H, int W, float* out, ebc_stream_t stream);
/* ebc_tile_assemble's arithmetic for every image, into maps + map_off, from preds [tiles][Cp][wh/r][ww/r] of the
 * whole list; counts[i] = the sum of image i's map, added in a fixed order (no atomics: two calls give the same
 * bits). */
int ebc_tiles_assemble_batch(const float* preds, const EbcEvalImage* desc, const EbcEvalImage* desc_host, int n_images,
                             int Cp, int wh, int ww, int sh, int sw, int reduction, float* maps, float* counts,
                             ebc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-crop augmentation on device (the reference runs it on CPU in
 * DataLoader workers, utils/data_utils.py:14-26).  One descriptor per output crop (device array);
 * the host samples the random parameters with the reference's RNG calls:
 *   crop window + resize  RandomResizedCrop / _crop / _resize (datasets/transforms.py:9-43,133-171):
 *                         torch F.interpolate(bicubic, antialias=True) taps; src == NULL skips it
 *   flip                  RandomHorizontalFlip (transforms.py:174-187), on the resize store
 *   jitter_ops            ColorJitter order (transforms.py:190-201 -> torchvision ColorJitter):
 *                         3 bits per slot (up to 4 slots), 1 brightness, 2 contrast, 3 saturation, 4 hue
 *                         (torchvision adjust_hue: _rgb2hsv, h = (h + hue) % 1, _hsv2rgb, per pixel)
 *   blur                  GaussianBlur(kernel_size, sigma=(sx, sy)) (transforms.py:217-223), reflect pad
 *   noise                 PepperSaltNoise (transforms.py:242-255) over uniforms u[3][out_h][out_w]:
 *                         noise_off >= 0: u = noise + noise_off, a field the host drew with the reference's own
 *                         `torch.rand_like(image)` (transforms.py:252), so the host RNG stream stays the reference's;
 *                         noise_off < 0: u = counter-based uniforms from `seed` (no host draw, no upload)
 *   normalize             Normalize(ImageNet mean/std) (datasets/crowd.py:64,162)
 * workspace: per crop tmp_off .. + max(3*crop_h*out_w, 3*out_h*out_w) floats (caller-assigned).
 * noise: the device uniform fields noise_off indexes; NULL = every crop takes the counter-based uniforms. */
#define EBC_AUG_MAX_BLUR 31
typedef struct {
    int64_t src_off, out_off, tmp_off;   /* element offsets: source image [3][src_h][src_w], output [3][out_h][out_w], scratch */
    int64_t noise_off;                   /* element offset of this crop's uniform field in `noise`, or -1 (hash of seed) */
    int32_t src_h, src_w, top, left, crop_h, crop_w, out_h, out_w;
    int32_t flip, jitter_ops;
    float brightness, contrast, saturation;
    int32_t blur, noise;
    float saltiness, spiciness;
    uint32_t seed;
    int32_t normalize;
    float hue;                           /* ColorJitter hue factor in [-0.5, 0.5] (op 4) */
} EbcCropDesc;
typedef struct {
    float mean[3], std[3];
    int32_t blur_k;                      /* odd, <= EBC_AUG_MAX_BLUR */
    float sigma_x, sigma_y;
} EbcAugConst;
/* max_crop_h / max_out_h: maxima over the descriptors (grid sizing) */
int ebc_augment_crops(const float* src, const EbcCropDesc* desc, int n, int max_crop_h, int max_out_h, float* out,
                      float* workspace, const float* noise, EbcAugConst k, ebc_stream_t stream);
/* ebc_augment_crops from stored images as they are: the same six launches, but the horizontal pass reads crop i's
 * window through csrc[i] -- uint8 [H][W][3] (a decoded JPEG) or [3][H][W] (the reference's .npy images,
 * datasets/crowd.py:141-148), or f32 [3][H][W] in [0, 1] (a pre-resized image) -- with the layout codes of
 * EbcEvalImage; one launch may mix the three.  A uint8 sample is (float)u / 255.0f (crowd.py:144), every output value
 * the float pass's fmaf chain over the float pass's taps, so the result is bit-equal to ebc_augment_crops on
 * u8.float() / 255.  desc[i].top / left / crop_h / crop_w address the stored source; src_off, src_h and src_w of
 * EbcCropDesc are unused.  A workgroup stages the byte spans of its rows in LDS (aligned dwords for the body, single
 * bytes for head and tail: no byte outside the window's rows is read, so a source may end on the last byte of its
 * allocation) and windows wider than the staging rows are processed in column chunks.
 * Both arrays are taken twice, on the device (what the kernels read) and on the host (what the checks and the grid
 * sizes read; only read during the call).
 * EBC_E_ARG, before any device work: NULL src / csrc / desc (either copy) / out / workspace, n < 0 or n > 21845, a
 * layout that is none of the three, src_off < 0, an F32_CHW source whose src_off or src is not 4-byte aligned, H or W
 * <= 0, a window that leaves its source (top < 0, left < 0, top + crop_h > H, left + crop_w > W), crop_h / crop_w /
 * out_h / out_w <= 0, blur_k as ebc_augment_crops, and any size past int32 (3 H W of a source, 3 crop_h out_w,
 * 3 out_h out_w). */
typedef struct {
    int64_t src_off;                     /* byte offset of the stored source in src */
    int32_t layout;                      /* EBC_EVAL_U8_HWC / EBC_EVAL_U8_CHW / EBC_EVAL_F32_CHW */
    int32_t H, W;                        /* stored height and row length, in pixels */
    int32_t reserved;
} EbcCropSrc;
int ebc_augment_crops_raw(const void* src, const EbcCropSrc* csrc, const EbcCropSrc* csrc_host, const EbcCropDesc* desc,
                          const EbcCropDesc* desc_host, int n, float* out, float* workspace, const float* noise,
                          EbcAugConst k, ebc_stream_t stream);
/* generate_density_map(label, H, W, sigma=None) (datasets/utils.py:11-28) for B crops: out [B][1][H][W]
 * = 1 at (clamp(int y), clamp(int x)) of points [sum n, 2] (x, y), offsets [B+1] (device) */
int ebc_point_map(const float* points, const int* offsets, int B, int H, int W, int max_points, float* out,
                  ebc_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Decoder BasicBlock (models/utils.py:254-303, cfg [768] for vit_b_16, models/clip/model.py:250-251)
 * with the reduction adapt F.interpolate(x2, bilinear, align_corners=False) (model.py:195-196),
 * training-mode BatchNorm2d (batch statistics, running stats; SyncBatchNorm = caller all-reduces
 * `colsum` / `sums` between the two calls that bracket them) and the whole backward.
 * Layouts (T = dtype): feat [B][h][w][C] f32; padded NHWC images [Q][C] T with Q = B*Hp*Wp;
 * z / dx / y [B*H*W][C] T; transposed images xT3 [3][C][Qs], dzT [N][Qs] T; conv weights
 * [N][3][3][C] T (forward) and [C][3][3][N] T (flipped, data gradient); dw [N][C][3][3] f32 (nn.Conv2d layout).
 * ebc_dec_geometry writes {Hp, Wp, HWp, Kq, Q, Qs}: the padded image is Hp = H+2 rows of Wp >= W+2 positions
 * (Wp a multiple of 8, at least 32), Q = B*Hp*Wp; HWp = H*W rounded up to 8 (at least 64) is one image's column
 * count in dzT, Kq = B*HWp rounded up to 64 the columns ebc_bn_bwd_apply writes, Qs the row stride.
 * The workspace's first 16 KiB must be zero before the first call (split-K arrival counters, re-armed by
 * every call); it is stream-owned scratch. */
int ebc_dec_geometry(int dtype, int B, int H, int W, int C, long* out6);
size_t ebc_dec_workspace_bytes(int dtype, int B, int H, int W, int C, int N);
/* xpad = zero-padded bilinear x`up` upsample of feat (H = h*up) */
int ebc_dec_upsample_pad(int dtype, const float* feat, void* xpad, int B, int h, int w, int C, int up,
                         ebc_stream_t stream);
/* out[B*H*W][N] = conv3x3(xpad, weight) (nn.Conv2d(C, N, 3, padding=1, bias=False)); colsum != NULL:
 * also the f64 column sums [2][N] (sum, sum of squares) for BatchNorm; add_gy/add_y != NULL (data
 * gradient of conv1): out += add_gy * (add_y > 0), the residual branch's gradient through the final ReLU */
int ebc_conv3x3_fwd(int dtype, const void* xpad, const void* weight, void* out, double* colsum, const void* add_gy,
                    const void* add_y, void* ws, size_t wsb, int B, int H, int W, int C, int N, ebc_stream_t stream);
/* The implicit-GEMM tile configuration of a decoder conv product (mode 1: forward / data gradient,
 * M = B*H*W rows, N output channels, K = 9*C; mode 2: weight gradient, M = N channels, N = 9*C,
 * K = interior pixel rows): returns its id, out[3] = {tile rows, tile columns, split-K ways}; out[2] = -G: stream-K,
 * G workgroups share the k-tiles of the tiles past the last whole wave of 256 (those run first as a plain
 * launch). Host-only. */
int ebc_conv_tile_config(int dtype, int mode, int M, int N, int K, int* out);
/* dw[N][C][3][3] f32 = weight gradient from dzT and xT3.
 * Padding contract: the product runs over all Kq columns of dzT, and column b*HWp + r meets position
 * b*Pimg + ky*W + r of xT3's rows, which for r >= H*W is the image's next rows (input data for ky < 2) and the
 * zeros behind them.  So dzT's padding columns inside Kq -- r >= H*W of every image and the columns past B*HWp --
 * MUST be zero (ebc_bn_bwd_apply writes them so); xT3 is taken as ebc_dec_transpose3 writes it, and the positions
 * of its rows that belong to no image row (past (H+2)*W of an image, past the last image) meet only those zero
 * columns, so their content does not reach dw as long as it is finite.  dzT's columns >= Kq are never read. */
int ebc_conv3x3_wgrad(int dtype, const void* dzT, const void* xT3, float* dw, void* ws, size_t wsb, int B, int H,
                      int W, int C, int N, ebc_stream_t stream);
/* BatchNorm2d statistics -> mean, rstd, scale = gamma*rstd, shift = beta - mean*scale; running stats
 * updated (momentum, unbiased variance) when colsum != NULL, read (eval) when colsum == NULL.
 * count < 0: the element count is the DEVICE value colsum[2*C] (SyncBatchNorm: each rank stores its own
 * count there and all-reduces it with the sums, so ranks may hold different batch sizes, as
 * torch.nn.SyncBatchNorm allows); num_batches_tracked (int64, may be NULL) is incremented by the same launch */
int ebc_bn_finalize(const double* colsum, double count, float eps, float momentum, const float* gamma,
                    const float* beta, float* mean, float* rstd, float* scale, float* shift, float* running_mean,
                    float* running_var, long long* num_batches_tracked, int C, ebc_stream_t stream);
/* ebc_conv3x3_fwd with the BatchNorm statistics epilogue + ebc_bn_finalize (count = B*H*W, running stats updated,
 * num_batches_tracked incremented when non-NULL) for BatchNorms with no SyncBatchNorm exchange between the two: the
 * conv's per-tile column sums are reduced and finalized in one launch; colsum_out (may be NULL) gets the f64 sums */
int ebc_conv3x3_fwd_bn(int dtype, const void* xpad, const void* weight, void* out, void* ws, size_t wsb, int B, int H,
                       int W, int C, int N, float eps, float momentum, const float* gamma, const float* beta,
                       float* mean, float* rstd, float* scale, float* shift, float* running_mean, float* running_var,
                       long long* num_batches_tracked, double* colsum_out, ebc_stream_t stream);
/* hpad = zero-padded relu(z*scale + shift) */
int ebc_bn_relu_pad(int dtype, const void* z, const float* scale, const float* shift, void* hpad, int B, int H,
                    int W, int C, ebc_stream_t stream);
/* y = relu(z*scale + shift + bilinear_up(feat)) */
int ebc_bn_add_relu(int dtype, const void* z, const float* scale, const float* shift, const float* feat, int up,
                    void* y, int B, int H, int W, int C, ebc_stream_t stream);
/* sums[2][C] f64 = (sum g, sum g*xhat), g = gy * relu'(mask_y, or z*scale+shift when mask_y == NULL), relu'(0) = 0.
 * P >= 1 rows (EBC_E_ARG otherwise); C a multiple of 8 up to 4096 (EBC_E_UNSUPPORTED otherwise) */
int ebc_bn_bwd_reduce(int dtype, const void* gy, const void* mask_y, const void* z, const float* mean,
                      const float* rstd, const float* scale, const float* shift, double* sums, void* ws, size_t wsb,
                      long P, int C, ebc_stream_t stream);
/* dgamma, dbeta (may be NULL) and coef[3][C] for ebc_bn_bwd_apply; count < 0: device count at sums[2*C] */
int ebc_bn_bwd_finalize(const double* sums, double count, const float* gamma, const float* rstd, float* dgamma,
                        float* dbeta, float* coef, int C, ebc_stream_t stream);
/* dz = BatchNorm input gradient -> dzpad (padded NHWC) and dzT (transposed) */
int ebc_bn_bwd_apply(int dtype, const void* gy, const void* mask_y, const void* z, const float* mean,
                     const float* rstd, const float* scale, const float* shift, const float* coef, void* dzpad,
                     void* dzT, int B, int H, int W, int C, ebc_stream_t stream);
/* xT3 = kx-shifted transposed copies of a padded NHWC image (weight-gradient operand) */
int ebc_dec_transpose3(int dtype, const void* xpad, void* xT3, int B, int H, int W, int C, ebc_stream_t stream);
/* conv weight [N][C][3][3] f32 -> wk [N][3][3][C] (forward) and wf [C][3][3][N] (flipped, data gradient) */
int ebc_dec_prep_weights(int dtype, const float* w, void* wk, void* wf, int N, int C, ebc_stream_t stream);
/* dfeat [B][h][w][C] f32 = bilinear_up^T(g), g [B*H*W][C] (up = 1, 2 or 4; other factors: EBC_E_UNSUPPORTED) */
int ebc_dec_upsample_bwd(int dtype, const void* g, float* dfeat, int B, int h, int w, int C, int up,
                         ebc_stream_t stream);
/* Flat-layout helpers of the ResNet-50 decoder Bottleneck (models/utils.py:306-363 with expansion 1, cfg [2048],
 * models/clip/model.py:234-246): its 1x1 convs are ebc_gemm products on unpadded rows [P = B*H*W][C]; the middle
 * 3x3 conv uses ebc_conv3x3_* above.
 *   ebc_dec_upsample:      x [P][C] T = bilinear x`up` upsample of feat [B][h][w][C] f32 (unpadded)
 *   ebc_bn_stats:          colsum [2][C] f64 = (sum z, sum z*z) over the P rows of z (BatchNorm batch statistics);
 *                          workspace as ebc_bn_bwd_reduce's (>= ebc_dec_workspace_bytes for that geometry)
 *   ebc_bn_relu:           out [P][C] T = relu(z*scale + shift)
 *   ebc_bn_bwd_apply_flat: dz [P][C] T = BatchNorm input gradient (coef from ebc_bn_bwd_finalize), g = gy * relu'(mask_y,
 *                          or z*scale+shift when mask_y == NULL); gmask != NULL also receives g [P][C] f32 (the
 *                          identity branch's gradient). */
int ebc_dec_upsample(int dtype, const float* feat, void* x, int B, int h, int w, int C, int up, ebc_stream_t stream);
int ebc_bn_stats(int dtype, const void* z, double* colsum, void* ws, size_t wsb, long P, int C, ebc_stream_t stream);
/* ebc_bn_stats + ebc_bn_finalize (count = P) in two launches instead of three, for BatchNorms whose statistics need no
 * SyncBatchNorm exchange between the two (models/utils.py / _clip/image_encoder.py BatchNorm2d, train mode);
 * colsum_out (may be NULL) receives the f64 sums ebc_bn_stats would. */
int ebc_bn_stats_finalize(int dtype, const void* z, void* ws, size_t wsb, long P, int C, float eps, float momentum,
                          const float* gamma, const float* beta, float* mean, float* rstd, float* scale, float* shift,
                          float* running_mean, float* running_var, double* colsum_out, long long* num_batches_tracked,
                          ebc_stream_t stream);
/* ebc_bn_bwd_reduce + ebc_bn_bwd_finalize (count = P) in two launches instead of three (no SyncBatchNorm exchange) */
int ebc_bn_bwd_reduce_finalize(int dtype, const void* gy, const void* mask_y, const void* z, const float* mean,
                               const float* rstd, const float* scale, const float* shift, const float* gamma,
                               float* dgamma, float* dbeta, float* coef, void* ws, size_t wsb, long P, int C,
                               ebc_stream_t stream);
int ebc_bn_relu(int dtype, const void* z, const float* scale, const float* shift, void* out, long P, int C,
                ebc_stream_t stream);
int ebc_bn_bwd_apply_flat(int dtype, const void* gy, const void* mask_y, const void* z, const float* mean,
                          const float* rstd, const float* scale, const float* shift, const float* coef, void* dz,
                          float* gmask, long P, int C, ebc_stream_t stream);
/* ModifiedResNet encoder blocks on HIP (models/clip/_clip/image_encoder.py:10-115, blocks.py:56-101: 1x1 -> 3x3 ->
 * avgpool(stride) -> 1x1, downsample = avgpool + 1x1 + BN), NHWC rows [B*H*W][C], C % 8 == 0, H, W even:
 *   ebc_bn_relu_avgpool:  out [B][H/2][W/2][C] = AvgPool2d(2)(relu(z*scale + shift))      (bn2 -> relu2 -> avgpool)
 *   ebc_avgpool2:         out = AvgPool2d(2)(x), same element type                        (downsample "-1" pool)
 *   ebc_avgpool2_bwd:     gx [B][H][W][C] = g[b][y/2][x/2] / 4 (g f32 or the compute dtype -> gx in dtype_out)
 *   ebc_bn_add_relu_flat: y = relu(z*scale + shift + idt*iscale + ishift) (iscale == NULL: + idt)  (bn3 + identity) */
int ebc_bn_relu_avgpool(int dtype, const void* z, const float* scale, const float* shift, void* out, int B, int H, int W,
                        int C, ebc_stream_t stream);
int ebc_avgpool2(int dtype_in, int dtype_out, const void* x, void* out, int B, int H, int W, int C, ebc_stream_t stream);
int ebc_avgpool2_bwd(int dtype_in, int dtype_out, const void* g, void* gx, int B, int H, int W, int C, ebc_stream_t stream);
int ebc_bn_add_relu_flat(int dtype, const void* z, const float* scale, const float* shift, const void* idt,
                         const float* iscale, const float* ishift, void* y, long P, int C, ebc_stream_t stream);
/* 1x1 conv weight [N][K] f32 (nn.Conv2d [N][K][1][1]) -> wk [N][K] and wt [K][N] in dtype (the GEMM operands of the
 * forward and of the data gradient), one launch; N, K multiples of 32 */
int ebc_prep_weights_1x1(int dtype, const float* w, void* wk, void* wt, int N, int K, ebc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer step: Adam with the GradScaler folded in.  Replaces the reference's
 * Adam(params, lr, weight_decay) (utils/train_utils.py:80-85) driven under GradScaler (trainer.py:123) as
 * grad_scaler.step(optimizer); grad_scaler.update() (train.py:54-57), i.e. torch.optim.Adam (L2 weight decay,
 * no amsgrad / maximize) + torch.amp.GradScaler's inf check, unscale, skip and scale update.
 * tensors[n]: HOST array of f32 device tensors (param, grad, exp_avg, exp_avg_sq, numel), any n.
 * step: DEVICE float[2], the optimizer's step count; scaler: DEVICE float[2][3] = {scale, growth_tracker,
 *   found_inf} x 2, or NULL (no loss scaling: bf16 / fp32 training).  A call reads entry [parity] of each and
 *   writes entry [1 - parity] (the next step count; the next scale and tracker and a cleared found_inf), so the
 *   caller flips each parity after every call.
 * With a scaler, any non-finite gradient skips the update (params, moments and step count unchanged) and backs
 *   the scale off; otherwise the gradients are divided by the scale (and, write_unscaled_grad = 1, written back
 *   unscaled as GradScaler.unscale_ leaves them) and the scale grows by growth_factor every growth_interval
 *   applied steps.
 * Two launches (check, update) per 32 tensors; arithmetic as torch's fused Adam (tests/test_gpu_optim.py). */
typedef struct {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long numel;
} EbcAdamTensor;
int ebc_adam_step(const EbcAdamTensor* tensors, int n, float* step, int step_parity, float* scaler, int scaler_parity,
                  double lr, double beta1, double beta2, double eps, double weight_decay, double growth_factor,
                  double backoff_factor, int growth_interval, int write_unscaled_grad, ebc_stream_t stream);
/* The same step in two calls, for several parameter groups sharing one GradScaler (torch skips the WHOLE optimizer
 * step when any group has a non-finite gradient): ebc_amp_check over every group's tensors first (found_inf of entry
 * [scaler_parity]), then ebc_adam_update per group (the update launch alone; each call writes the same next scaler
 * state). */
int ebc_amp_check(const EbcAdamTensor* tensors, int n, float* scaler, int scaler_parity, ebc_stream_t stream);
int ebc_adam_update(const EbcAdamTensor* tensors, int n, float* step, int step_parity, float* scaler, int scaler_parity,
                    double lr, double beta1, double beta2, double eps, double weight_decay, double growth_factor,
                    double backoff_factor, int growth_interval, int write_unscaled_grad, ebc_stream_t stream);

/* Weight touch (performance only; the results do not change): the encoder's attention launches read onto the die the
 * frozen weights of the GEMMs after them (attention.hip touch_issue).  mode 1 (default): on; 0: off (A/B, tests). */
int ebc_set_weight_touch(int mode);

/* ------------------------------------------------------------------------------------------
 * Measurement (bench.py): in-step kernel durations and profile windows.  Not on the reference's
 * surface; the reference has no instrumentation.
 * ebc_probe_begin(capacity): from now on every launch of the instrumented kernels is bracketed by HIP
 *   events on its own stream (at most `capacity` launches recorded).
 * ebc_probe_end(out, capacity): stops recording, waits for the last event and writes one record per
 *   launch (returns the number recorded; records beyond `capacity` are dropped).
 * ebc_marker(id, stream): launches the named empty kernel `ebc_marker_kernel` (profile window edges). */
enum { EBC_PROBE_GEMM = 1, EBC_PROBE_DACE = 2, EBC_PROBE_ATTN_FWD = 3, EBC_PROBE_ATTN_BWD_DQ = 4,
       EBC_PROBE_ATTN_BWD_DKV = 5, EBC_PROBE_LN_FWD = 6, EBC_PROBE_LN_BWD = 7, EBC_PROBE_HEAD_BWD_TEXT = 8 };
typedef struct {
    int kind;                 /* EBC_PROBE_* */
    int epi, bm, bn, mode;    /* GEMM: epilogue, tile, MODE (0 plain, 1 implicit 3x3 conv, 2 conv weight gradient) */
    int m, n, k;              /* GEMM: problem; DACE: B, total points, grid g; attention: B, L, heads; LN: rows */
    float ms;                 /* measured duration */
} EbcProbeRecord;
int ebc_probe_begin(int capacity);
int ebc_probe_end(EbcProbeRecord* out, int capacity);
int ebc_marker(int id, ebc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EBC_HIP_H */
