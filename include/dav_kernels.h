/* C ABI of libdavfusion_hip.so — the MI355X (gfx950) kernels behind the DeepAVFusion / AVMAE
 * pre-training step.
 *
 * The reference (stoneMo/DeepAVFusion) has no FFI of its own: every device op on this path is a
 * stock ATen call issued from Python.  This header is the boundary one level below the Python
 * modules that mirror the reference's classes: each entry point replaces the ATen/cuDNN/cuBLAS/SDPA
 * work behind the reference lines cited on it (paths relative to the reference repo).
 *
 * Conventions:
 *  - plain pointers and sizes only; the caller owns every buffer (inputs, outputs, workspaces);
 *    the library never allocates, frees or keeps a pointer past return;
 *  - all work is enqueued on `stream`; no host synchronisation, no host callbacks; safe to call from
 *    several host threads on distinct streams, and inside hipGraph stream capture;
 *  - return 0 on success, a negative DAV_ERR_* code otherwise (never aborts).  Arguments are validated BEFORE any HIP call:
 *    empty input (a size of 0) is a bad shape (-1) for every kernel entry point, an unsupported dtype combination -2, a
 *    workspace that is too small -3, a HIP launch failure -4 (text: dav_last_error_string), a misaligned pointer or stride
 *    -5; a refused call has enqueued nothing (tests/test_cabi_and_host.py checks every entry point, without a GPU);
 *  - "bf16" buffers are raw uint16 bfloat16; index tensors are int64 where the reference exposes
 *    them (ids_keep / ids_restore) with int32 twins for in-kernel use; row strides are in elements.
 *  - a "row map" is an int[3] {rows_per_batch, batch_stride_rows, row_offset} (NULL = identity):
 *    logical row m -> physical row (m / rpb) * bs + off + m % rpb.  It lets a GEMM read or write a
 *    sub-range of a [B, rows, D] activation without cat/split copies.
 */
#ifndef DAV_KERNELS_H_
#define DAV_KERNELS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
typedef struct ihipStream_t* hipStream_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define DAV_ABI_VERSION 9   /* 9: dropout (dav_attn_drop_fwd / _bwd (+ _f32), dav_dropout_rows); 8: LayerNorm folded into the GEMMs either side of it (dav_gemm_nt_ln_bf16, dav_ln_fold_grouped, dav_rowstats_cast, dav_layernorm_bwd_twin); 2: DavTnProblem.flags, dav_adamw_flat keep_grad + gscale_dev, dav_step_guard; 3: dav_attn_bwd_ctx, dav_add_cast; 4: fused fusion tails, grouped cast-transpose; 5: dav_gemm_tn_grouped_adamw_bf16; 6: dav_gemm_tn_gang_bf16; 7: the fused fusion tails and dav_gemm_tn_grouped_adamw_bf16 are gone (measured slower, DESIGN_HISTORY section 11) (9 also: dav_mean_l2n_f32, dav_knn_topk_f32, dav_frame_transform_u8, dav_knn_topk_wide_f32, dav_knn_vote_f32) */
int dav_abi_version(void);
int dav_build_flags(void);   /* bit 0: experimental build (make EXPERIMENTAL=1): the rejected GEMM tile configurations exist */
/* text of the last HIP error latched by a kernel launch of the calling thread (diagnostics) */
const char* dav_last_error_string(void);
/* launch-geometry knobs for tuning experiments (1: LayerNorm-backward waves per workgroup {2,4,8}; 2: its grid cap;
 * 3: query tiles per wave of the attention forward, 0 = automatic, 1, 2;
 * 5: the attention backward of short problems, 0 = the fit rule (one launch when the whole (batch, head) problem fits 80 KB of LDS,
 *    head widths (64, 64) / (16, 64), no bias / dropout, not recorded into a lane of a launch batch), 1 = always the dQ + dK/dV kernel pair, 2 = one pass whenever it fits.
 * (4 belonged to a probe that is gone.)  An unknown knob or value returns DAV_ERR_SHAPE. */
int dav_tune(int knob, int value);

/* ---- GEMM --------------------------------------------------------------------------------- */
/* C[M,N] = epi(alpha * A[M,K] . B[N,K]^T): every nn.Linear forward on the path (timm Attention.qkv/proj,
 * Mlp.fc1/fc2; models/fusion_blocks.py:41-44 q/kv/proj, :227-232 q/k/v/proj; models/avmae.py:31,59
 * decoder_embed, :60,88 decoder_pred; the patch-embed conv of models/vits.py:27 as a GEMM over
 * gathered patches) and, with B = W^T, their input gradients.
 * epilogue order: v = alpha*acc + bias[n]; [C2 mode 1]; act 1 = exact (erf) GELU [C2 mode 4: the twin is GELU'(v)
 * of the pre-activation v], act 2 = v *= GELU'(aux[m,n]), act 3 = v *= aux[m,n] (fc1 backward, with aux = the pre-activation
 * or the mode-4 twin of the forward); [C2 mode 2]; + fp32 residual (row map or explicit row list: the block residual adds
 * and "+ pos_embed[ids_keep]"); beta != 0 adds the old fp32 C; store C (fp32 or bf16, through
 * c_rowmap; may be NULL); [C2 mode 3].  C2 is a dense bf16 [M, ldc2] twin for the next GEMM.
 * variant bit12: B is given as [K, N] row-major (ldb = row stride; K % 64 == 0, N % 8 == 0) — the dgrad reads
 * W itself through transposing LDS reads, no W^T copy; bits 4-11: explicit tile configuration (benchmarks);
 * bit0: register-staged loads instead of global->LDS DMA; bit1: force 64x64 tiles (first-generation kernel). */
int dav_gemm_nt_bf16(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const int* a_rowmap,
                     const float* bias, int act, const void* aux, int ldaux, const float* res, int ldres,
                     const int* res_rowmap, const int* res_rows, void* C, int ldc, int c_is_bf16, const int* c_rowmap,
                     void* C2, int ldc2, int c2_mode, int beta, float alpha, int variant, hipStream_t stream);

/* dav_gemm_nt_bf16 with the LayerNorm between two GEMMs folded into them (ABI 8) — timm Block.norm1 / norm2 in front of attn.qkv /
 * mlp.fc1 (models/vits.py:32-34, models/avmae.py:53-57, 83-87), norm1_img / norm1_aud / norm2 of the fusion blocks
 * (models/fusion_blocks.py:281-288), decoder_norm in front of decoder_pred (models/avmae.py:59-60,177-178): no LayerNorm launch and no
 * normalised tensor in memory on the forward path.
 *  PRODUCER side (stats_out / twin_out; C must be fp32, N % 64 == 0): besides C the epilogue writes, for every row, the partial sums
 *   stats_out[crow * (N / 64) + s] = {sum, sum of squares} of the FINAL fp32 values of columns [64 s, 64 s + 64) (crow = the C row after
 *   c_rowmap) and the bf16 twin twin_out[crow * ld_twin + n] of the final value.  Fixed summation order, no atomics.
 *  CONSUMER side (stats): A holds RAW rows — such a twin — and B the weight with the LayerNorm's gamma folded in (dav_ln_fold_grouped:
 *   B[n, k] = bf16(gamma[k] W[n, k]) from the fp32 master W, ln_c[n] = sum_k B[n, k], bias := b[n] + sum_k beta[k] W[n, k]); the epilogue starts from
 *   v = rstd[m] * (acc[m, n] - mean[m] * ln_c[n]) + bias[n] with mean / rstd formed from the K / 64 partial sums of row m
 *   (mean = sum / K, var = sumsq / K - mean^2 clamped at 0, rstd = 1 / sqrt(var + eps)); K % 64 == 0, K <= 1024, alpha == 1.
 *   The statistics row of A row m is the physical A row (through a_rowmap).  a_r0 > 0: every batch element's rows are a_r0 rows of
 *   (A, stats) followed by a_r1 rows of (A2, stats2), both dense and with row stride lda — the cat((x_fusion, x_mod)) of
 *   models/deepavfusion.py:104-105; a_rowmap must be NULL and M a multiple of a_r0 + a_r1.
 * Everything else as dav_gemm_nt_bf16 (b_kn and explicit first-generation variants are refused). */
typedef struct DavNtLn {
  const float* stats; const float* stats2; const void* A2; const float* ln_c; float eps; int a_r0, a_r1;   /* consumer */
  float* stats_out; void* twin_out; int ld_twin;                                                          /* producer */
} DavNtLn;
int dav_gemm_nt_ln_bf16(const void* A, const void* B, int M, int N, int K, int lda, int ldb, const int* a_rowmap,
                        const float* bias, int act, const void* aux, int ldaux, const float* res, int ldres,
                        const int* res_rowmap, const int* res_rows, void* C, int ldc, int c_is_bf16, const int* c_rowmap,
                        void* C2, int ldc2, int c2_mode, int beta, float alpha, int variant, const DavNtLn* ln, hipStream_t stream);

/* Diagnostics for benchmarks: log which launches the NT family issues (grouped or single).  enable 1 / 0 with out == NULL
 * starts (and clears) / stops logging (process-wide: autograd runs the backward on its own thread); with out != NULL the log is copied: entries of
 * {tile configuration, b_kn, n, n x (M, N, K, epilogue flags)}; returns the number of ints, or -needed when capacity is too small.
 * flags = act | c_is_bf16 << 2 | has_res << 3 | c2_mode << 4 | beta << 8. */
int dav_nt_issue_log(int enable, int* out, int capacity);

/* Tuned tile-configuration table for grouped NT launches (the role cuBLAS' / hipBLASLt's per-size solution tables play
 * behind torch's F.linear in the reference, models/vits.py:32-34): `blob` holds entries in dav_nt_issue_log's format; a
 * group recorded between dav_batch_begin / dav_batch_end whose b_kn + sorted (M, N, K, flags) list matches an entry is issued
 * with that entry's tile configuration, any other group by the built-in rules.  n_ints == 0 clears.  Returns the number of
 * entries held, or a negative DAV_ERR_*.  Written by tools/mix_sweep.py, loaded by deepavfusion_amd/_lib.py. */
int dav_nt_tune_set(const int* blob, int n_ints);

/* C[N,K] (+)= A[Mc,N]^T . B[Mc,K] in fp32: the weight gradient of every nn.Linear above (autograd of
 * F.linear).  beta != 0 accumulates into the live gradient (split over the contraction with fp32
 * atomics); bias_grad (optional) receives the column sums of A (atomic accumulate).
 * variant bit0: scalar LDS reads instead of ds_read_b64_tr_b16. */
int dav_gemm_tn_bf16(const void* A, const void* B, int Mc, int N, int K, int lda, int ldb, const int* a_rowmap,
                     const int* b_rowmap, float* C, int ldc, int beta, float* bias_grad, int variant, hipStream_t stream);

/* Several weight-gradient problems (C_i[N_i,K_i] += A_i^T . B_i, optional bias_grad_i) in ONE launch — the deferred
 * wgrads of a whole layer — so that every 128x128 output tile is owned by one workgroup over (most of) its
 * contraction: no or very few split-K atomics.  count <= 40; every Mc_i % 64 == 0.  Row maps as above
 * ({0,0,0} = identity).  The table is read on the host during the call only. */
typedef struct DavTnProblem {
  const void* A; const void* B;       /* bf16 [Mc, N] (lda), bf16 [Mc, K] (ldb) */
  float* C; float* bias_grad;         /* fp32 [N, K] (ldc), fp32 [N] or NULL; both accumulated */
  int Mc, N, K, lda, ldb, ldc;
  int a_rowmap[3], b_rowmap[3];
  int flags;                          /* bit 0: C is WRITTEN, its old contents ignored (the first contribution to a gradient
                                         that the optimizer pass did not zero-fill, see dav_adamw_flat keep_grad); bias_grad
                                         is accumulated regardless.  Such a problem is never split over the contraction. */
} DavTnProblem;
int dav_gemm_tn_grouped_bf16(const DavTnProblem* problems, int count, hipStream_t stream);

/* The same problems (any number up to 4096: the queued weight gradients of SEVERAL layers, autograd of every nn.Linear on the path —
 * models/fusion_blocks.py:41-44,227-232, timm Block of models/vits.py:32-34, models/avmae.py:53-60,83-88) as ONE persistent launch of
 * 256 x 256 tiles, one workgroup per CU: every problem's tile grid is cut into gangs of <= 32 tiles that share operand panels, the
 * gangs are dealt out to eight per-XCD ticket queues (longest contraction first) and the workgroups of an XCD draw the tiles of one gang
 * together, so that a panel crosses the fabric once per XCD instead of once per tile.  One owner per tile over the whole contraction:
 * no atomics on C, bit-repeatable.  Any Mc > 0 (a contraction that is not a multiple of 64 rows — B x tokens at batch 32 — is padded with
 * zeros on the fly).  flags bit 0 as above; other bits: DAV_ERR_SHAPE.  Two problems of one call must not
 * address the same C.  workspace: caller-owned device memory of dav_gemm_tn_gang_workspace_bytes(problems, count) bytes (0 = invalid
 * problems), 16-byte aligned, written and read on `stream` only (it must stay untouched until the launch has run). */
size_t dav_gemm_tn_gang_workspace_bytes(const DavTnProblem* problems, int count);
int dav_gemm_tn_gang_bf16(const DavTnProblem* problems, int count, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* The two launches above with flags bit 0 decided ON THE DEVICE when the launch runs: a flagged problem is written while
 * write_gate[0] != 0 and accumulated while it is 0 (an unflagged one is accumulated either way) — one captured launch serves every
 * micro-step of a gradient-accumulation window (util/misc.py:96-136, accum_iter > 1), the gate open on the first only.  write_gate:
 * one int32 in device memory, read on `stream` when the launch runs; NULL: DAV_ERR_SHAPE.  Plans, splits (a flagged problem is never
 * split), workspace size and every other error code as for the ungated entry points. */
int dav_gemm_tn_grouped_bf16_gated(const DavTnProblem* problems, int count, const int* write_gate, hipStream_t stream);
int dav_gemm_tn_gang_bf16_gated(const DavTnProblem* problems, int count, void* workspace, size_t workspace_bytes, const int* write_gate,
                                hipStream_t stream);

/* ---- attention ---------------------------------------------------------------------------- */
/* softmax(scale * Q K^T) V per (batch, head); element (b, n, h, d) of X is X[b*x_bs + n*x_rs + h*dX + d].
 * (dqk, dv) in {(64,64), (32,32), (16,64)}.  Replaces F.scaled_dot_product_attention inside timm
 * Attention (models/vits.py:32-34 blocks, models/avmae.py:53-55,83-85 decoder blocks), CrossAttention
 * (models/fusion_blocks.py:50-56) and the factorised pair attention (:250-258).
 * LSE [B,H,Nq] (log-sum-exp of the scaled scores) is saved for the backward. */
int dav_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int Nq, int Nk, int dqk,
                 int dv, long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, float scale,
                 hipStream_t stream);
/* Delta [B,H,Nq] is scratch written by the first kernel and read by the second. */
int dav_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, float* Delta,
                 void* dQ, void* dK, void* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs, int q_rs, long k_bs,
                 int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs, long dq_bs, int dq_rs, long dk_bs,
                 int dk_rs, long dv_bs, int dv_rs, float scale, hipStream_t stream);
/* the same in two calls: part 1 = the dQ (+ Delta) kernel, part 2 = the dK/dV kernel (reads Delta), part 3 = both */
int dav_attn_bwd_part(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, float* Delta,
                 void* dQ, void* dK, void* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs, int q_rs, long k_bs,
                 int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs, long dq_bs, int dq_rs, long dk_bs,
                 int dk_rs, long dv_bs, int dv_rs, float scale, int part, hipStream_t stream);

/* dav_attn_bwd_part for a query buffer that is the tail of a longer key / value buffer (the tower blocks' fused qkv: the fusion
 * tokens are context rows — keys and values only, models/deepavfusion.py:104-105): dQ has dq_ctx_rows rows BEFORE its first query
 * row in every batch element (dQ - dq_ctx_rows * dq_rs must be valid memory); the dQ kernel (part & 1) zero-fills the dqk columns
 * of every head in them, so that the fused gradient buffer can go into the qkv GEMMs without a fill pass of its own. */
int dav_attn_bwd_ctx(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, float* Delta,
                 void* dQ, void* dK, void* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs, int q_rs, long k_bs,
                 int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs, long dq_bs, int dq_rs, long dk_bs,
                 int dk_rs, long dv_bs, int dv_rs, float scale, int dq_ctx_rows, int part, hipStream_t stream);

/* Window attention of the Swin decoder blocks (models/swin.py:55-87; decoder_arch == 'swin', models/avmae.py:37-51): the same
 * kernels with an additive logit bias.  bias [bias_nb][H][Nq][bias_ld] fp32 in LOG2 units (natural value x log2 e), zero
 * padded to bias_ld >= Nk rounded up to 32; batch element b uses table b % bias_nb (the shift mask differs per window,
 * :75-78).  Backward: dS [B][H][Nq][bias_ld] (optional) receives the gradient of the biased logits in natural units — what
 * dav_relpos_bias_bwd reduces into the relative-position table's gradient; its columns [Nk, Nk rounded up to 32) receive finite
 * values (the zero-padded keys' share, to be ignored), the columns beyond are left untouched (the fp32 twin writes [0, Nk) only). */
int dav_attn_bias_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int Nq, int Nk, int dqk,
                      int dv, long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, float scale,
                      const float* bias, int bias_nb, int bias_ld, hipStream_t stream);
int dav_attn_bias_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, float* Delta,
                      void* dQ, void* dK, void* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs, int q_rs, long k_bs,
                      int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs, long dq_bs, int dq_rs, long dk_bs,
                      int dk_rs, long dv_bs, int dv_rs, float scale, const float* bias, int bias_nb, int bias_ld, float* dS,
                      int part, hipStream_t stream);

/* Attention dropout (nn.Dropout on the softmax probabilities: timm Attention.attn_drop of the tower blocks, models/vits.py:33, and
 * models/fusion_blocks.py:14,25,42,54,99,112,164,181,231,256 — the fine-tuning constructors' attn_drop > 0; every pre-training
 * config has 0): O = (P .* keep * keep_scale) V with P the full softmax (LSE unchanged).  keep: bytes 0 / 1,
 * [B][H][Nq][keep_ld], keep_ld >= Nk rounded up to 32 and a multiple of 4, 4-byte aligned; keep_scale = 1 / (1 - p).  The draw
 * itself is the caller's (torch's generator): the kernels are deterministic in the mask.  Kernels of their own (the head widths
 * of dav_attn_fwd): the pre-training kernels carry no dropout code.  Backward: dP = keep * keep_scale * (dO V^T),
 * Delta = dO . O as without dropout; dq_ctx_rows as dav_attn_bwd_ctx, part as dav_attn_bwd_part. */
int dav_attn_drop_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int Nq, int Nk, int dqk,
                      int dv, long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, float scale,
                      const void* keep, int keep_ld, float keep_scale, hipStream_t stream);
int dav_attn_drop_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, float* Delta,
                      void* dQ, void* dK, void* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs, int q_rs, long k_bs,
                      int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs, long dq_bs, int dq_rs, long dk_bs,
                      int dk_rs, long dv_bs, int dv_rs, float scale, const void* keep, int keep_ld, float keep_scale,
                      int dq_ctx_rows, int part, hipStream_t stream);

/* ---- Swin decoder data movers (csrc/swin.hip) --------------------------------------------- */
/* A decoder activation is [B][nF fusion rows | L = nW * A token rows][C]; a window sequence is [A window tokens | nF fusion
 * tokens], B * nW of them.  rows[w * A + i] = token (0-based, within the L token rows) at slot i of window w after the cyclic
 * shift (torch.roll + timm window_partition, models/swin.py:172-179); inv = its inverse permutation.
 * dav_window_unfold: sequences <- rows (the fusion rows repeated per window and scaled by fusion_scale; models/swin.py:183-185;
 *   with fusion_scale = 1 / nW also the backward of the fold's mean).  src fp32 -> out bf16 or fp32, src bf16 -> out bf16
 *   (bf16 -> fp32 returns DAV_ERR_DTYPE).
 * dav_window_fold: rows <- sequences (+ res): token rows through inv (window_reverse + roll back, :191-197), fusion rows =
 *   fusion_scale x the sum over the windows (1 / nW: the mean of :199; 1: the backward of the unfold's repeat). */
int dav_window_unfold(const void* src, int src_is_bf16, const int* rows, int B, int nW, int A, int nF, int L, int C,
                      float fusion_scale, void* out, int out_is_bf16, hipStream_t stream);
int dav_window_fold(const float* t, const int* inv, const float* res, int B, int nW, int A, int nF, int L, int C,
                    float fusion_scale, float* out, hipStream_t stream);
/* out[w][h][q][k] = mul * (table[index[q * A + k]][h] + mask[w][q][k]) for q, k < A, 0 elsewhere ([nb][H][N][ld]; mask NULL
 * for unshifted blocks, then nb = 1): models/swin.py:49-53 + :66-78 (the reference pads both with zeros to the N = A + nF
 * sequence).  dav_relpos_bias_bwd: dtable[e][h] += sum over the Bw sequences and the (q, k) with index == e of dS; A * A <= 1024
 * (windows up to 5 x 5; a larger A returns DAV_ERR_SHAPE). */
int dav_relpos_bias_build(const float* table, const int* index, const float* mask, int nb, int H, int A, int N, int ld, float mul,
                          float* out, hipStream_t stream);
int dav_relpos_bias_bwd(const float* dS, const int* index, int Bw, int H, int A, int N, int ld, int T, float* dtable,
                        hipStream_t stream);

/* ---- LayerNorm ---------------------------------------------------------------------------- */
/* nn.LayerNorm over D on rows taken from two fp32 sources per batch element (r0 rows of x0, then r1
 * rows of x1; r1 may be 0): folds torch.cat((x_fusion, x_mod), 1) of models/deepavfusion.py:104-105
 * into Block.norm1.  Writes bf16 and/or fp32 outputs ([B*(r0+r1), D]) and the row statistics. */
int dav_layernorm_fwd(const float* x0, long x0_bs, int r0, const float* x1, long x1_bs, int r1, int B, int D,
                      const float* gamma, const float* beta, float eps, void* y_bf16, float* y_f32, float* mean, float* rstd,
                      hipStream_t stream);
/* total dy = dy_bf16 + dy_f32 (either may be NULL).  For each source segment s: dx_s (=|+=) LN'(dy)
 * (+ res_s), optional bf16 copy; dx_s NULL skips the segment.  dgamma/dbeta are accumulated (+=) from
 * per-workgroup partial rows staged in `workspace` (two kernels, no atomics). */
int dav_layernorm_bwd(const float* x0, long x0_bs, int r0, const float* x1, long x1_bs, int r1, int B, int D,
                      const void* dy_bf16, const float* dy_f32, const float* gamma, const float* mean, const float* rstd,
                      float* dx0, long dx0_bs, int acc0, const float* res0, long res0_bs, void* dx0_bf16, long dx0_bf_bs,
                      float* dx1, long dx1_bs, int acc1, const float* res1, long res1_bs, void* dx1_bf16, long dx1_bf_bs,
                      float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t dav_layernorm_bwd_workspace_bytes(int rows, int D);   /* rows = B * (r0 + r1) */
/* Deferred form: call dav_layernorm_bwd with dgamma = dbeta = NULL and a workspace (only the per-workgroup
 * partial rows are written), then reduce up to 64 such workspaces into their dgamma/dbeta (+=) in ONE launch. */
/* rows > 0: the LayerNorm backward ran over `rows` rows (its own grid decides how many partial rows the workspace holds);
 * rows < 0 (ABI 4): the workspace holds exactly -rows partial rows [2 D] */
typedef struct DavLnReduce { const void* workspace; float* dgamma; float* dbeta; int rows; int D; } DavLnReduce;
int dav_layernorm_bwd_reduce_grouped(const DavLnReduce* items, int count, hipStream_t stream);

/* ---- LayerNorm folded into its neighbour GEMMs (ABI 8; see dav_gemm_nt_ln_bf16) ------------------------------------------- */
/* Per (Linear, LayerNorm-in-front-of-it) pair, from the fp32 master weight w [N, K] (one rounding, as for the plain bf16 mirror):
 * w_ln[n, k] = bf16(gamma[k] * w[n, k]), ln_c[n] = sum_k float(w_ln[n, k]) (the ROUNDED values the GEMM contracts with: acc - mean * ln_c
 * is an exact centring), ln_d[n] = (bias ? bias[n] : 0) + sum_k beta[k] * w[n, k].  One launch for up to 48 pairs (one wave per output
 * row); the table is read on the host during the call only.  K % 8 == 0. */
typedef struct DavLnFold {
  const float* w; const float* gamma; const float* beta; const float* bias;   /* [N, K] fp32, [K], [K], [N] or NULL */
  void* w_ln_bf16; float* ln_c; float* ln_d;                                   /* [N, K] bf16, [N], [N] */
  int N, K;
} DavLnFold;
int dav_ln_fold_grouped(const DavLnFold* items, int count, hipStream_t stream);
/* Row statistics + bf16 twin of an fp32 activation that no GEMM epilogue produced (the decoder input after the un-shuffle, the
 * expanded fusion tokens, DropPath outputs): rows r of [B][rows][D] at x + b * x_bs + r * D (x_bs in elements, 0 = broadcast) ->
 * twin[(b * rows + r) * D + ...] bf16, stats[(b * rows + r) * (D / 64) + s] = {sum, sum of squares} over columns [64 s, 64 s + 64).
 * D % 64 == 0, D <= 1024. */
int dav_rowstats_cast(const float* x, long x_bs, int B, int rows, int D, void* twin_bf16, float* stats, hipStream_t stream);
/* dav_layernorm_bwd for a LayerNorm that was folded away on the forward path: x comes as the bf16 twin (two dense segments per batch
 * element, batch strides in elements as there) with its statistics partials (st*: row b * (st*_bs / D) + r), mean / rstd are re-formed
 * as dav_gemm_nt_ln_bf16 forms them, and h_out (optional, bf16 [B * (r0 + r1), D]) receives gamma * xhat + beta — the operand the weight
 * gradient of the consuming Linear contracts with, produced here instead of being kept from the forward.  Everything else as
 * dav_layernorm_bwd (dgamma / dbeta partial rows in `workspace`, reduced by dav_layernorm_bwd_reduce_grouped or at once). */
int dav_layernorm_bwd_twin(const void* xb0, long xb0_bs, const float* st0, int r0, const void* xb1, long xb1_bs, const float* st1, int r1,
                           int B, int D, float eps, const void* dy_bf16, const float* dy_f32, const float* gamma, const float* beta,
                           float* dx0, long dx0_bs, int acc0, const float* res0, long res0_bs, void* dx0_bf16, long dx0_bf_bs,
                           float* dx1, long dx1_bs, int acc1, const float* res1, long res1_bs, void* dx1_bf16, long dx1_bf_bs,
                           void* h_out_bf16, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- masking / gather / scatter ------------------------------------------------------------ */
/* AVMAE.random_masking (models/avmae.py:120-142) for given noise [N,L]: argsort twice, keep the first
 * len_keep, un-shuffled 0/1 mask.  Bit-exact with torch.argsort for tie-free noise. */
int dav_mask_build(const float* noise, int N, int L, int len_keep, int64_t* ids_keep, int64_t* ids_restore, float* mask,
                   int* ids_keep32, int* ids_restore32, hipStream_t stream);
/* im2row of the kept 16x16 patches only (timm PatchEmbed + the gather of models/vits.py:100):
 * A[b*nk+t, c*256+py*16+px] bf16; ids NULL = all patches in order. */
int dav_patch_gather(const float* img, int B, int C, int H, int W, const int* ids_keep32, int nk, void* A_bf16, hipStream_t stream);
/* the same for clips [B,C,T,H,W] and (pt,16,16) tubelets (PatchEmbed3D, util/pos_embed.py:123-146, used by
 * models/video_vits.py:218-220): token = (gt*gH + gy)*gW + gx, A[b*nk+t, ((c*pt + dt)*16 + py)*16 + px] */
int dav_patch_gather3d(const float* video, int B, int C, int T, int H, int W, int pt, const int* ids_keep32, int nk,
                       void* A_bf16, hipStream_t stream);
/* models/avmae.py:161-165: out[b, off+r] = (restore[b,r] < nk ? emb[b*nk+restore[b,r]] : mask_token) + pos[r] */
int dav_unshuffle_fwd(const float* emb, const float* mask_token, const float* pos, const int* ids_restore32, int B, int L, int nk,
                      int D, float* out, long out_bs, int out_row_off, hipStream_t stream);
/* out[b*n+t] = bf16(x[b, row_off + (ids ? ids[b*n+t] : t)]) — backward of the gather / of x[:, nF:] slices */
int dav_rows_gather_cast(const float* x, long x_bs, int row_off, const int* ids32, int B, int n, int D, void* out_bf16,
                         hipStream_t stream);
/* DropPath (timm; models/vits.py:32-34, models/fusion_blocks.py:69,130,199,278 when drop_path > 0 — fine-tuning) with a
 * per-sample scale s[b] in {0, 1/keep}: forward out[b,r,:] = res[b,r,:] + s[b]*y[b,r,:] (fp32; out may alias res); backward of
 * the branch side out_bf16[b,r,:] = bf16(s[b]*g[b,r,:]) (the residual side passes g through unchanged). */
int dav_rows_axpy(const float* res, const float* y, const float* scale, int B, int rows, int D, float* out, hipStream_t stream);
int dav_rows_scale_cast(const float* g, const float* scale, int B, int rows, int D, void* out_bf16, hipStream_t stream);
/* Dropout on activations (timm Mlp.drop1 / drop2, the attention modules' proj_drop; fine-tuning constructors' drop > 0), DropPath
 * folded in: out[b,r,:] = (res ? res[b,r,:] : 0) + (rowscale ? rowscale[b] : 1) * (keep[b,r,:] ? keep_scale : 0) * in[b,r,:].
 * keep: bytes 0 / 1 [B*rows][D] (null = all kept), in / out bf16 (in_f32 / out_f32 = 0) or fp32 (1), D % 4 == 0; out may alias
 * in or res.  Alignment: res and fp32 in / out 16 bytes, bf16 in / out 8 bytes, keep 4 bytes (else DAV_ERR_ALIGN).  The backward is the same call on the gradient (res = null). */
int dav_dropout_rows(const void* in, int in_f32, const float* res, const void* keep, float keep_scale, const float* rowscale,
                     int B, int rows, int D, void* out, int out_f32, hipStream_t stream);
/* dpos[r] += sum_b dx[b, off+r]; dmask_token += sum over masked (b, r) */
int dav_unshuffle_bwd_reduce(const float* dx, long dx_bs, int row_off, const int* ids_restore32, int B, int L, int nk, int D,
                             float* dpos, float* dmask_token, hipStream_t stream);

/* ---- loss --------------------------------------------------------------------------------- */
/* AVMAE.patchify + forward_loss (models/avmae.py:182-214) without a patchified target tensor:
 * per-patch MSE against the (optionally norm-pix, unbiased variance) target read from NCHW,
 * loss = sum(loss_patch * mask) / sum(mask). */
int dav_patch_mse_fwd(const float* img, const float* pred, const float* mask, int B, int C, int H, int W, int norm_pix,
                      float* loss_patch, float* tmean, float* trstd, float* loss, float* mask_sum, hipStream_t stream);
int dav_patch_mse_bwd(const float* img, const float* pred, const float* mask, const float* tmean, const float* trstd,
                      const float* mask_sum, const float* gout, int B, int C, int H, int W, void* dpred_bf16, hipStream_t stream);

/* ---- factorised (v,a) pairs (models/fusion_blocks.py:245-252) ------------------------------- */
int dav_pair_expand(const float* Pv, const float* Pa, int B, int nv, int na, int Wd, void* out_bf16, hipStream_t stream);
int dav_pair_reduce(const void* d_bf16, int B, int nv, int na, int Wd, void* dPv_bf16, void* dPa_bf16, hipStream_t stream);

/* ---- casts, grad norm, optimizer ----------------------------------------------------------- */
int dav_cast_bf16(const float* x, void* y_bf16, long n, hipStream_t stream);
/* out = a + b (fp32, n % 4 == 0) and out_bf16 = bf16(out) in one pass: the gradient w.r.t. the fusion tokens is the sum of what the
 * image tower and the audio tower return (models/deepavfusion.py:104-105 feeds the same tokens to both), and the next block's
 * backward wants it in both precisions.  (ABI 3) */
int dav_add_cast(const float* a, const float* b, float* out, void* out_bf16, long n, hipStream_t stream);
int dav_cast_transpose_bf16(const float* x, void* y_bf16, int R, int C, hipStream_t stream);   /* y[c,r] = x[r,c] */
/* the same for several matrices in ONE launch (ABI 4): y_bf16 [C, R] = bf16(x [R, C] fp32) per item */
typedef struct DavTranspose { const float* x; void* y_bf16; int R; int C; } DavTranspose;
int dav_cast_transpose_grouped(const DavTranspose* items, int count, hipStream_t stream);
/* get_grad_norm_ (util/misc.py:151-163) over one flat fp32 buffer: out = scale * ||x||_2 */
size_t dav_l2norm_workspace_bytes(long n);
int dav_l2norm(const float* x, long n, float scale, float* out, void* workspace, size_t workspace_bytes, hipStream_t stream);
/* torch.optim.AdamW(betas=(0.9,0.95)) step (train.py:93) over flat param/grad/state buffers with
 * per-segment {lr, weight_decay}; bias_corr = {1-beta1^t, sqrt(1-beta2^t)} in device memory.  The same pass can
 * (a) accumulate sum(g^2) of the unscaled gradients into *sumsq_out (zeroed first; the grad norm of
 * util/misc.py:151-163 is its square root), (b) rewrite the bf16 weight mirror p_bf16, (c) zero the gradients
 * (Trainer.zero_grad) — one trip over the buffers instead of three.  keep_grad (NULL or one byte per segment): segments
 * with a non-zero byte are NOT zero-filled — their next gradient will be written, not accumulated (DavTnProblem.flags bit 0),
 * which saves the fill here and the read there (values other than 0 / 1 are not defined).  All accesses are 16-byte ones: the buffers must be
 * 16-byte aligned (p_bf16 8-byte), n and every seg_end a multiple of 4 (FlatParams aligns segments to 64 elements).
 * gscale_dev (optional): device scalar from dav_step_guard, see there. */
int dav_adamw_flat(float* p, float* g, float* m, float* v, void* p_bf16, long n, const long* seg_end, const float* hyper,
                   int nseg, float beta1, float beta2, float eps, const float* bias_corr, float grad_scale, float* sumsq_out,
                   int zero_grad, const unsigned char* keep_grad, const float* gscale_dev, hipStream_t stream);

/* Device-side guard of a captured (hipGraph) step, replaces the host checks of train.py:166-167 (non-finite loss aborts before the
 * optimizer step) and util/misc.py:118-120 (clip_grad_norm_) that a replayed graph cannot run:
 *   out_scale[0] = 0                                    if loss_a + loss_b (either may be NULL) or gnorm[0] is not finite,
 *                = min(1, clip / (gnorm[0] * grad_scale + 1e-6))   if gnorm != NULL (the global gradient norm, dav_l2norm) and
 *                                                                   clip > 0,   = 1 otherwise;
 * bad_count[0] (optional) is incremented when the scale is 0.  dav_adamw_flat(gscale_dev = out_scale) multiplies the gradients
 * by it and, when it is 0, leaves parameters, moments and the bf16 mirror untouched (gradients are still zero-filled). */
int dav_step_guard(const float* loss_a, const float* loss_b, const float* gnorm, float clip, float grad_scale, float* out_scale,
                   int* bad_count, hipStream_t stream);

/* ---- log-mel front-end (csrc/mel.hip) ------------------------------ */
/* out[b, m, t] = log10(mel_m(|STFT_t(wave[b])|^2) + eps): the reference's audio transform
 * aT.MelSpectrogram(sample_rate, n_fft, hop_length, n_mels) -> aT.Log() (train.py:50-54, util/audio_transforms.py:29-35) and
 * the [:, :, :-1] of datasets.py:242, computed on the device from raw waveforms [B, S] instead of in CPU loader workers.
 * Semantics of torchaudio's Spectrogram + MelScale defaults: centre padding by reflection, the caller's window of n_fft
 * samples (periodic Hann), one-sided power spectrum, dense filterbank fbank[n_fft/2+1, n_mels] with each filter's non-zero bin
 * range [band_lo[m], band_hi[m]); cos_tab / sin_tab[n] = cos / sin(2 pi n / n_fft).  frames = S / hop + 1; drop_last removes
 * the final frame (out is [B, n_mels, frames - drop_last]); apply_log = 0 returns the mel power itself. */
int dav_logmel(const float* wave, int B, int S, int n_fft, int hop, int n_mels, const float* window, const float* cos_tab,
               const float* sin_tab, const float* fbank, const int* band_lo, const int* band_hi, float eps, int apply_log,
               int drop_last, float* out, hipStream_t stream);
int dav_log10_eps(const float* x, float eps, long n, float* y, hipStream_t stream);      /* aT.Log: y = log10(x + eps) */

/* ---- frame transform of the input stage (csrc/data/frames.hip) -------------------------------- */
/* The reference's frame transforms on the device, from uint8 frames instead of PIL images in CPU loader workers:
 * RandomResizedCrop -> RandomHorizontalFlip -> ToTensor -> Normalize (train.py:45-49) and Resize -> CenterCrop -> ToTensor ->
 * Normalize (util/knn_probe.py:31-36).  frames uint8 [B, H, W, 3] (HWC, dense) -> out fp32 [B, 3, S, S] (CHW, dense).
 * params int32 [B, 9] on the device, per sample: source window (i, j, h, w) = (top row, left column, rows, columns); virtual
 * output size (RH, RW) the window is resampled to; origin (top, left) of the emitted S x S window inside the virtual output;
 * flip (non-zero: the emitted window is mirrored left-right).  Resized crop: window = crop box, (RH, RW) = (S, S), origin (0, 0);
 * resize + centre crop: window = whole frame, (RH, RW) = resized size, origin = crop offset.
 * Resampling: the antialiased bilinear (triangle) filter of PIL's Image.resize(BILINEAR) / F.interpolate(mode='bilinear',
 * antialias=True), separable, per axis scale = n_in / n_out, support = max(scale, 1), centre c = (o + 0.5) scale, taps
 * k in [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)) INSIDE the window (pixels outside the crop box never
 * contribute), weight max(0, 1 - |k - c + 0.5| / support) divided by the sum of the weights; the weights are formed exactly
 * (integers over 2 max(n_in, n_out)), sums in fp32, NO rounding to uint8 between the passes or at the end (PIL does both).
 * Then out = (v / 255 - mean_c) / std_c.  Every index is clamped into the frame and every parameter into range: a bad row gives
 * a wrong picture, never an out-of-bounds access.  B <= 65535; H, W, S <= 16384; S a multiple of 16; std_c > 0 (else -1);
 * out 16-byte, params 4-byte aligned (else -5).  One launch, no workspace. */
int dav_frame_transform_u8(const uint8_t* frames, int B, int H, int W, const int* params, int S, float mean0, float mean1,
                           float mean2, float std0, float std1, float std2, float* out, hipStream_t stream);

/* ---- audio resampling of the input stage (csrc/data/resample.hip) ----------------------------- */
/* The reference's loader resamples every track from its own rate (datasets.py:176-181, torchaudio's default windowed-sinc
 * polyphase Resample), then Pad -> RandomVol (util/audio_transforms.py:8-27); here the three are ONE launch over a batch.
 * With o = orig / gcd, n = new / gcd, K = 2 width + o taps per phase and the waveform x zero-padded by `width` in front:
 *   r[f n + p] = sum_k taps[p][k] xpad[f o + k], cut to R = ceil(n L / o) samples   (fp32, one k-ordered fmaf chain per sample)
 *   out[b][j] = c(gain[b] r_b[m(j)]),  m(j) = j' < R ? j' : 2 R - 1 - j',  j' = j mod 2 R   (Pad's mirror; a plain cut for
 *   out_len <= R);  c clamps to [-1, 1] when `clamp` is set; gain NULL = 1.
 * wave: fp32, or int16 (wave_is_i16; scaled by 2^-15, exact), [B][L] with a row stride of in_rs elements.  taps_kn: the fp32
 * table K-MAJOR, [K][n] (lanes read consecutive phases).  out fp32 [B][out_len], row stride out_rs elements.
 * o, n <= dav_resample_max_ratio and K <= 14336 (56 KB of staged samples), B <= 65535, L, out_len <= 2^30, in_rs >= L,
 * out_rs >= out_len (else -1); wave aligned to its element, taps_kn, gain and out to 4 bytes (else -5; no wider access is
 * made, so the strides carry no alignment of their own).  dav_wave_resample_tile: the number of frames (of o input samples) one
 * workgroup owns at this geometry — the seam of the tiling, for tests — or -1 for a refused geometry. */
enum { dav_resample_max_ratio = 1024 };   /* the cap on o and n */
int dav_wave_resample_tile(int o, int n, int width);
int dav_wave_resample(const void* wave, int wave_is_i16, int B, int L, long in_rs, const float* taps_kn, int o, int n, int width,
                      const float* gain, int clamp, float* out, int out_len, long out_rs, hipStream_t stream);

/* ---- source-separation audio (csrc/sep/stft.hip) ---------------------------------------------- */
/* The reference's SpectrogramMasking (eval_avsrcsep.py:264-277, applied per sample and per source on the host, :245-254):
 *   aT.Spectrogram(n_fft, hop_length, power=None) -> sigmoid(mask), one zero frame appended -> einsum('bmt,fm->bft', mask,
 *   mel_scale.fb) -> mask * stft -> aT.InverseSpectrogram(n_fft, hop_length)  (torch.stft / torch.istft underneath).
 * All fp32, direct DFTs with cos_tab / sin_tab[n] = cos / sin(2 pi n / n_fft) looked up at (k n) mod n_fft, window = the
 * caller's n_fft samples (periodic Hann): the tables of dav_logmel.  n_freqs = n_fft / 2 + 1.
 *
 * dav_stft_c32 (:268, :273): wave [B][S] fp32, row stride wave_rs >= S -> spec [B][n_freqs][frames] interleaved re / im (torch's
 *   complex64), frames = S / hop + 1, bin rows spec_rs >= frames COMPLEX elements apart, batch elements n_freqs * spec_rs.
 *   Framing exactly dav_logmel's: center = True, reflect padding, one-sided, not normalised.  A workgroup owns dav_stft_frames
 *   consecutive frames.
 * dav_istft_c32 (:269, :276): spec as above -> out [B][hop (frames - 1)] fp32, row stride out_rs:
 *   torch.istft(center=True, normalized=False, onesided=True, length=None).  Per frame
 *     x[n] = (1/N) [Re X_0 + (-1)^n Re X_{N/2} + 2 sum_{k=1}^{N/2-1} (Re X_k cos(2 pi k n / N) - Im X_k sin(2 pi k n / N))]
 *   (the imaginary parts of the DC and Nyquist bins are ignored, as irfft ignores them), times the window, overlap-added, divided
 *   by the envelope sum w^2, n_fft / 2 samples dropped at each end.  The overlap-add is a gather: every output sample adds the
 *   at most ceil(n_fft / hop) frames that cover it in increasing frame order; no atomics; two calls agree bit for bit.  The
 *   envelope must be non-zero over the kept samples (torch's NOLA check; aT.InverseSpectrogram checks it) — a zero divides.
 *   A workgroup holds dav_istft_frames frames in LDS, 2 h + 1 of them halo, h = (n_fft / 2 - 1) / hop, and owns the
 *   hop * (dav_istft_frames - 2 h - 1) output samples they cover completely (9 hops at 800 / 250 and 400 / 125).
 * dav_sep_mask_istft (:272-277 in one launch): wave [B][S] (the mixtures), logits [B][K][n_mels][T] dense (K >= 1 masks per
 *   mixture), fbank [n_freqs][n_mels] with band_lo / band_hi [n_mels] as dav_logmel takes them -> out [B][K][hop (frames - 1)],
 *   row (b, k) at (b K + k) out_rs.  Per (b, frame t): the STFT X once; per k:  M[f] = sum_m fbank[f][m] s(logit[b][k][m][t]) over
 *   the filters m with band_lo[m] <= f < band_hi[m] in increasing m, s(x) = 1 / (1 + expf(-x)) (exactly 0 / 1 at -+100);
 *   Y = M X; then as dav_istft_c32.  The mask of the last frame is zero (the appended column): T + 1 == frames is required.
 *   Neither X, M nor Y is written to memory; the tiling is dav_istft_c32's (halo frames are transformed again).
 * -1: an empty input (B, S, K, n_mels, T < 1; B or K > 65535), n_fft odd or < 2, hop <= 0, S <= n_fft / 2 (torch refuses such a
 *     reflect pad), frames < 2, T + 1 != frames, a stride below its row, a NULL operand, a geometry with 2 h + 1 >=
 *     dav_istft_frames or whose tile does not fit 160 KiB of LDS (both reference geometries fit: 800 / 250 takes 58 KB, 87 KB and
 *     135 KB for the three calls, 400 / 125 half of that);
 * -5: spec not 8-byte aligned, any other pointer not 4-byte aligned.  Sizes are judged before alignment and both before any HIP
 * call.  No workspace. */
enum { dav_stft_frames = 8 };      /* frames per workgroup of dav_stft_c32: frames t and t + 1 with (t + 1) % 8 == 0 meet at a seam */
enum { dav_istft_frames = 12 };    /* frames per workgroup of the inverse, halo included: hop * (12 - 2 h - 1) samples per workgroup */
int dav_stft_c32(const float* wave, int B, int S, long wave_rs, int n_fft, int hop, const float* window, const float* cos_tab,
                 const float* sin_tab, float* spec, long spec_rs, hipStream_t stream);
int dav_istft_c32(const float* spec, long spec_rs, int B, int frames, int n_fft, int hop, const float* window,
                  const float* cos_tab, const float* sin_tab, float* out, long out_rs, hipStream_t stream);
int dav_sep_mask_istft(const float* wave, int B, int S, long wave_rs, const float* logits, int K, int n_mels, int T, int n_fft,
                       int hop, const float* window, const float* cos_tab, const float* sin_tab, const float* fbank,
                       const int* band_lo, const int* band_hi, float* out, long out_rs, hipStream_t stream);

/* ---- nearest-neighbour probe (csrc/probe/knn.hip) ------------------------------------------- */
/* out[b, :] = v / max(||v||_2, 1e-12) with v = mean over l of x[b, l, :]: the x.mean(dim=1) + F.normalize(p=2, dim=1) of
 * util/knn_probe.py:102-110.  x fp32 [B, L, D] with row stride ld_row (>= D) and batch stride ld_batch (elements); out dense
 * fp32 [B, D].  The mean is a sequential fp32 sum over l divided by L; an all-zero v gives zeros. */
int dav_mean_l2n_f32(const float* x, int B, int L, int D, long ld_row, long ld_batch, float* out, hipStream_t stream);
/* Fused similarity + top-k of util/knn_probe.py:117-131 (the einsum('qd,nd->qn') of each modality, scores_v + scores_a + scores_mm,
 * torch.topk(k, sorted=True)), without a score matrix in memory.  M in {1, 2, 3} modality pairs (q_m [Nq, D] row stride ldq,
 * x_m [N, D] row stride ldx, fp32; q_m may alias x_m): s_m(i, n) = sum_d q_m[i, d] x_m[n, d] as an fp32 FMA chain (exact-fp32 MFMA,
 * no rounding of the operands).  sum_view = 1 adds view M: s(i, n) = (s_0 + s_1) + s_2 (pass image, audio, fusion in that order
 * for the reference's sum).  Outputs top_val [V, Nq, k] fp32 and top_idx [V, Nq, k] int32, V = M + sum_view, each row sorted by
 * score descending, ties to the LOWER bank index; no self-exclusion (the probe reads position 1).  NaN scores are never selected.
 * 1 <= k <= min(8, N); D % 4 == 0; q_m / x_m 16-byte aligned, ldq / ldx multiples of 4 (else -5).
 * The bank is cut into `splits` (1 .. 65535) runs of 128-row tiles, each keeping its own top-k list in the workspace, and a second
 * launch merges them: workspace_bytes >= splits * V * Nq * k * 8 (8-byte aligned).  The result is bitwise the same for every split
 * count and every chunking of the queries.  Suggested split count (deepavfusion_amd.ops.knn_splits): enough workgroups to cover
 * the 256 CUs twice, splits = min(ceil(N / 128), max(1, ceil(512 / ceil(Nq / 128)))). */
int dav_knn_topk_f32(const float* q0, const float* x0, const float* q1, const float* x1, const float* q2, const float* x2, int M,
                     int Nq, int N, int D, long ldq, long ldx, int sum_view, int k, int splits, float* top_val, int* top_idx,
                     void* workspace, size_t workspace_bytes, hipStream_t stream);
/* The weighted k-NN probe (Wu et al. 2018, DINO; csrc/probe/knn_wide.hip) — not in the reference, whose probe stops at the nearest
 * other clip.  dav_knn_topk_wide_f32 is dav_knn_topk_f32 with 1 <= k <= min(64, N): the same operands, views, splits and output
 * layout, the same score chains in the same order (the two share their tile code), the same strict order (score descending, ties to
 * the LOWER bank index).  So for k <= 8 it equals dav_knn_topk_f32 bit for bit, the first 8 entries of a longer list equal that
 * kernel's k = 8 result, and the result is the same for every split count, query chunking and arrival order of the bank rows.
 * The lists live in the workspace while the bank streams by, one per (split, view, query); a second launch merges the splits:
 * workspace_bytes >= splits * V * Nq * k * 8 (8-byte aligned) — the formula of dav_knn_topk_f32 (deepavfusion_amd.ops
 * .knn_workspace_bytes).  No [Nq, N] score matrix exists in memory.
 * -1: an empty input, M outside 1..3, k < 1, k > 64, k > N, D % 4, a stride below D, splits outside 1..65535, a NULL operand or
 * output; -3: a NULL or short workspace; -5: q_m / x_m not 16-byte aligned, ldq / ldx not multiples of 4, outputs not 4-byte,
 * workspace not 8-byte aligned. */
int dav_knn_topk_wide_f32(const float* q0, const float* x0, const float* q1, const float* x1, const float* q2, const float* x2,
                          int M, int Nq, int N, int D, long ldq, long ldx, int sum_view, int k, int splits, float* top_val,
                          int* top_idx, void* workspace, size_t workspace_bytes, hipStream_t stream);
/* The vote over such lists.  top_val / top_idx [V, Nq, kk] as either top-k kernel writes them (V in 1..4).  For every (view v,
 * query q) the entries are walked in order; an entry whose index is q + self_offset is skipped (self_offset = -1: none is — the
 * bank is another set; 0: the bank is the query set itself); the first k remaining entries j vote with the weight
 * w_j = expf(top_val_j * inv_t[v]) for the class labels[idx_j] (labels int32 [N]) or for every set class of the row
 * multihot[idx_j, :] (uint8 [N, C]); exactly one of labels / multihot is given.  inv_t is a HOST array of V floats, read before the
 * call returns (1 / T for a modality; 1 / (T M) for the sum view votes on the mean similarity; 0 gives plain counts).
 * scores fp32 [V, Nq, C] (every element written); pred int32 [V, Nq] = the class of the largest score, ties to the LOWER class
 * (required with labels, ignored with multihot).  The k weights of a class are added in entry order, so the result is repeatable
 * bit for bit.  An index outside [0, N) and a label outside [0, C) vote for nothing.  1 <= k <= min(64, kk), and k <= kk - 1 when
 * self_offset >= 0: k entries must remain whatever the exclusion removes.
 * -1: an empty input, V outside 1..4, k outside that range, C < 1, self_offset < -1, a NULL top_val / top_idx / inv_t / scores,
 * neither or both of labels / multihot, labels without pred; -5: top_val, top_idx, labels, scores or pred not 4-byte aligned.
 * One launch, no workspace. */
int dav_knn_vote_f32(const float* top_val, const int* top_idx, int V, int Nq, int kk, int k, const int* labels,
                     const uint8_t* multihot, int N, int C, const float* inv_t, int self_offset, float* scores, int* pred,
                     hipStream_t stream);
/* The multi-label metrics of the probe (util/misc.py:312-327 / util/knn_probe.py:133-150 of the reference; csrc/probe/ap_auc.hip):
 * per-class average precision and ROC AUC of V (1..4) score views over n rows against the multi-hot truth y (uint8 [n, C], row
 * stride ldy >= C, nonzero = positive), as sklearn's average_precision_score / roc_auc_score (average=None) define them: scores
 * descending, TIES GROUPED into one threshold.
 *   ap[V, C]  fp64: sum over the thresholds t of (R_t - R_{t-1}) P_t; 0.0 for a column without a positive.
 *   auc[V, C] fp64: the trapezoid area under the distinct-threshold ROC from (0, 0), computed as the count of (positive, negative)
 *             pairs the score orders correctly, ties counting half, over P * Nneg: an exact integer and ONE rounding.  NaN for a
 *             column without a positive or without a negative (where sklearn raises).
 *   pos[C]    int32: the positives of each class.
 * The score of (view v, row i, class c) comes in exactly one of two forms:
 *   dense:     scores[v * score_vs + i * score_rs + c], fp32, score_rs >= C, score_vs >= 0 (elements; the [V, Nq, C] of
 *              dav_knn_vote_f32 or a view of wider rows);
 *   neighbour: nbr int32 [V, n], nbr_val fp32 [V, n], nbr_labels uint8 [N, C] (dense): nbr_labels[nbr[v, i], c] * nbr_val[v, i] — the
 *              value where the label is set, zero elsewhere (whatever the value) and for an index outside [0, N).
 * Scores are ordered through a monotone integer image of their bits, never compared as floats: -0.0 and +0.0 are ONE threshold,
 * subnormals stay distinct from zero and from each other.  All counts are integers; the fp64 terms of the AP are added in a fixed
 * order, so two calls on the same input agree bit for bit.  A NaN score leaves the ap / auc of its column unspecified (pos stays
 * exact) and touches no memory outside the operands.  One workgroup holds a whole column in LDS: n <= dav_ap_auc_max_rows.
 * The workspace holds the truth as one bit mask per class: workspace_bytes >= C * ((n + 31) / 32) * 4 (4-byte aligned;
 * deepavfusion_amd.ops.ap_auc_workspace_bytes).  Two launches.
 * -1: n, C or V < 1, V > 4, n > dav_ap_auc_max_rows, ldy or score_rs < C, score_vs < 0, a NULL y / ap / auc / pos, both forms or
 * neither (any of nbr / nbr_val / nbr_labels counts as the neighbour form), the neighbour form without all three or with N < 1;
 * -3: a NULL or short workspace; -5: scores, nbr, nbr_val, pos or the workspace not 4-byte, ap or auc not 8-byte aligned. */
enum { dav_ap_auc_max_rows = 32768 };   /* the cap on n */
int dav_ap_auc_f64(const uint8_t* y, long ldy, int n, int C, int V, const float* scores, long score_rs, long score_vs,
                   const int* nbr, const float* nbr_val, const uint8_t* nbr_labels, int N, double* ap, double* auc, int* pos,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- fp32-operand twins (csrc/f32_path.hip) ------------------------------------------------ */
/* The same contracts as the bf16 entry points above with every operand, second output and intermediate in fp32 (plain
 * one-thread-per-output kernels, untuned).  They exist so that the whole hand-written forward / backward can run in fp32
 * (engine.set_precision('fp32')) and be compared with the oracle and the reference's fixtures at 1e-4 instead of bf16's
 * 2e-2 — SURVEY.md section 8(b) "fp32-everything variants for tight parity tests".  b_kn as variant bit 12 above; part as
 * dav_attn_bwd_part.  LayerNorm, the loss forward, unshuffle and the optimizer are fp32 already. */
int dav_gemm_nt_f32(const float* A, const float* B, int M, int N, int K, int lda, int ldb, const int* a_rowmap,
                    const float* bias, int act, const float* aux, int ldaux, const float* res, int ldres,
                    const int* res_rowmap, const int* res_rows, float* C, int ldc, const int* c_rowmap, float* C2, int ldc2,
                    int c2_mode, int beta, float alpha, int b_kn, hipStream_t stream);
int dav_gemm_tn_f32(const float* A, const float* B, int Mc, int N, int K, int lda, int ldb, const int* a_rowmap,
                    const int* b_rowmap, float* C, int ldc, int beta, float* bias_grad, hipStream_t stream);
int dav_attn_fwd_f32(const float* Q, const float* K, const float* V, float* O, float* LSE, int B, int H, int Nq, int Nk, int dqk,
                     int dv, long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, float scale,
                     hipStream_t stream);
int dav_attn_bwd_f32(const float* Q, const float* K, const float* V, const float* O, const float* dO, const float* LSE,
                     float* Delta, float* dQ, float* dK, float* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs,
                     int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs, long dq_bs,
                     int dq_rs, long dk_bs, int dk_rs, long dv_bs, int dv_rs, float scale, int part, hipStream_t stream);
/* fp32 twins of dav_attn_bias_fwd / dav_attn_bias_bwd; bias in NATURAL units here, bias_ld >= Nk */
int dav_attn_bias_fwd_f32(const float* Q, const float* K, const float* V, float* O, float* LSE, int B, int H, int Nq, int Nk,
                          int dqk, int dv, long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs,
                          float scale, const float* bias, int bias_nb, int bias_ld, hipStream_t stream);
int dav_attn_bias_bwd_f32(const float* Q, const float* K, const float* V, const float* O, const float* dO, const float* LSE,
                          float* Delta, float* dQ, float* dK, float* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs,
                          int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs,
                          long dq_bs, int dq_rs, long dk_bs, int dk_rs, long dv_bs, int dv_rs, float scale, const float* bias,
                          int bias_nb, int bias_ld, float* dS, int part, hipStream_t stream);
int dav_attn_drop_fwd_f32(const float* Q, const float* K, const float* V, float* O, float* LSE, int B, int H, int Nq, int Nk,
                          int dqk, int dv, long q_bs, int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs,
                          float scale, const void* keep, int keep_ld, float keep_scale, hipStream_t stream);   /* keep_ld >= Nk */
int dav_attn_drop_bwd_f32(const float* Q, const float* K, const float* V, const float* O, const float* dO, const float* LSE,
                          float* Delta, float* dQ, float* dK, float* dV, int B, int H, int Nq, int Nk, int dqk, int dv, long q_bs,
                          int q_rs, long k_bs, int k_rs, long v_bs, int v_rs, long o_bs, int o_rs, long do_bs, int do_rs,
                          long dq_bs, int dq_rs, long dk_bs, int dk_rs, long dv_bs, int dv_rs, float scale, const void* keep,
                          int keep_ld, float keep_scale, int part, hipStream_t stream);
int dav_patch_gather_f32(const float* img, int B, int C, int T, int H, int W, int pt, const int* ids_keep32, int nk, float* A,
                         hipStream_t stream);
int dav_rows_gather_f32(const float* x, long x_bs, int row_off, const int* ids32, int B, int n, int D, float* out, long out_bs,
                        hipStream_t stream);      /* out_bs: batch stride of out in elements (0 = dense) */
int dav_pair_expand_f32(const float* Pv, const float* Pa, int B, int nv, int na, int Wd, float* out, hipStream_t stream);
int dav_pair_reduce_f32(const float* d, int B, int nv, int na, int Wd, float* dPv, float* dPa, hipStream_t stream);
int dav_patch_mse_bwd_f32(const float* img, const float* pred, const float* mask, const float* tmean, const float* trstd,
                          const float* mask_sum, const float* gout, int B, int C, int H, int W, float* dpred, hipStream_t stream);
int dav_add_f32(const float* a, const float* b, float* out, long n, hipStream_t stream);   /* out = a + b */

/* ---- launch batching ---------------------------------------------------------------------- */
/* The reference runs the image block, the audio block and the fusion block of a layer one after the other although they
 * only depend on the layer's inputs (models/deepavfusion.py:104-107), and likewise the two MAE decoders
 * (models/avmae.py:147-180).  Between dav_batch_begin() and dav_batch_end() every entry point of this library RECORDS its
 * kernel launches (per calling thread) instead of issuing them; dav_batch_lane() starts a new LANE — a sequence of
 * launches the caller declares independent of the other lanes.  dav_batch_end() issues the lanes in lockstep: the k-th
 * launches of all lanes go out together, those of one kernel family (NT GEMM, LayerNorm forward / backward, attention
 * forward / dQ / dK-dV) as ONE grouped grid whose workgroups look their problem up in a table passed by value, the rest
 * individually; the order inside a lane is kept.  With auto_lanes != 0 every recorded launch is its own lane (a region of
 * mutually independent launches).  Requirements on the caller: lanes must not depend on each other; every buffer a recorded
 * launch touches must stay allocated until dav_batch_end() returns; all launches of a batch use the stream they were
 * recorded with.  No nesting.  dav_batch_stats reports the last batch: launches recorded / launches issued.
 * dav_batch_region(1) .. dav_batch_region(0): the launches recorded in between are independent of each other and form ONE
 * step of the current lane (e.g. the q / kv projections of both aggregation cross-attentions of a fusion block). */
int dav_batch_begin(int auto_lanes);
int dav_batch_lane(void);
int dav_batch_region(int begin);
/* the current lane idles for `steps` steps (aligns its later launches with equal launches of a longer lane) */
int dav_batch_skip(int steps);
/* on != 0: launches are issued at once although a batch is open (for work that nothing recorded so far depends on and
 * that later recorded launches need, e.g. refreshing a bf16 weight copy); on == 0: recording resumes. */
int dav_batch_suspend(int on);
int dav_batch_end(void);
int dav_batch_abort(void);
int dav_batch_stats(int* recorded_ops, int* issued_launches);

#ifdef __cplusplus
}
#endif
#endif /* DAV_KERNELS_H_ */
