/* vipant_hip.h -- C ABI of libvipant_hip.so, the MI355X (gfx950) hot path of the VIP-ANT
 * bimodal contrastive training step.
 *
 * Conventions (SURVEY.md section 8b, row B-c):
 *   - every entry point returns int32_t: 0 = ok, negative = VIPANT_E*; vipant_last_error()
 *     returns a thread-local message for the last failure;
 *   - arguments are raw DEVICE pointers + explicit dims + a hipStream_t passed as void*;
 *   - no allocation, no ownership transfer, no implicit synchronisation: the caller (PyTorch)
 *     owns every buffer, including workspaces whose size the *_workspace_bytes() queries return;
 *   - bf16 tensors are passed as uint16_t* (raw bfloat16 bits), row-major, last dim contiguous;
 *   - token-major activations are [M, D] with M = batch * tokens (batch-first row order
 *     m = b * S + s; the reference's seq-first [S, b, D] is the same math on permuted storage,
 *     cvap/module/encoder/clip_head.py:108-110).
 *
 * Each function cites the reference interface it replaces (paths relative to the reference root).
 */
#ifndef VIPANT_HIP_H
#define VIPANT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIPANT_OK 0
#define VIPANT_EBADSHAPE (-1)
#define VIPANT_EBADDTYPE (-2)
#define VIPANT_EALIGN (-3)
#define VIPANT_EHIP (-4)
#define VIPANT_ENOWORKSPACE (-5)

/* GEMM epilogues (vipant_gemm_nt). */
#define VIPANT_EPI_BF16 0          /* C_bf16 = acc (+bias) */
#define VIPANT_EPI_F32 1           /* C_f32  = acc (+bias) */
#define VIPANT_EPI_RESIDUAL_F32 2  /* C_f32  = acc + bias + R_f32   (out_proj / c_proj + residual) */
#define VIPANT_EPI_QUICKGELU 3     /* U_bf16 = acc + bias ; C_bf16 = U * sigmoid(1.702 U)  (c_fc) */
#define VIPANT_EPI_DQUICKGELU 4    /* C_bf16 = acc * dQuickGELU(U_bf16)        (backward of c_fc act) */
#define VIPANT_EPI_SCALE_F32 5     /* C_f32  = alpha * acc */
#define VIPANT_EPI_QUICKGELU_D8 6  /* as QUICKGELU, but aux receives uint8 codes of QuickGELU'(U) instead of U (1 B / element) */
#define VIPANT_EPI_DQUICKGELU_D8 7 /* C_bf16 = acc * decode(aux uint8): backward of c_fc act from the 8-bit derivative code */
/* OR-ed into `epilogue`: the rows of this launch are ONE ROW PER ITEM of a batch (the last block on its read-out rows, the read-out
 * projection).  Such launches take 64 x 64 tiles with K split over the waves of a workgroup instead of 256 x 256 tiles (21-91 us ->
 * 9-30 us at 512 rows).  A property of the call site, not of M: a row's result must not depend on how many rows travel with it
 * (`running.micro_batch` reproduces the full-batch loss to 1e-6), so the kernel choice may not either.  Epilogues: BF16, F32,
 * RESIDUAL_F32, QUICKGELU_D8, DQUICKGELU_D8. */
#define VIPANT_EPI_FEW_ROWS 0x100

const char* vipant_last_error(void);
int32_t vipant_version(void);
/* 0 when the current device is gfx950 and the code object loads; VIPANT_EHIP otherwise. */
int32_t vipant_device_check(void);

/* ---- dense contractions (torch.nn.Linear / F.conv2d-as-GEMM / nn.MultiheadAttention projections:
 *      cvap/module/val.py:500-506, 245-247, 288-289) ------------------------------------------------
 * C[M,N] = A[M,K] . B[N,K]^T  (both operands K-contiguous, bf16; fp32 accumulate on MFMA).
 * K % 64 == 0, N % 4 == 0.  bias (fp32 [N]) may be NULL.  `aux` is R (EPI_RESIDUAL_F32, may alias C),
 * U out (EPI_QUICKGELU) or U in (EPI_DQUICKGELU), or the uint8 [M, N] matrix of QuickGELU' codes (the _D8 epilogues: the backward
 * needs only the derivative, code = round((QuickGELU'(U) + 0.1) * 212.5), error <= 2.4e-3).  ldc applies to C and aux (elements). */
int32_t vipant_gemm_nt(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc,
                       const float* bias, void* aux, float alpha, int64_t M, int64_t N, int64_t K,
                       int32_t epilogue, void* stream);

/* Weight-gradient contraction (autograd of nn.Linear weight): C[P,Q] (+)= A[M,P]^T . B[M,Q], reduction
 * over the token dimension M (both operands M-major).  Q % 4 == 0 (P arbitrary).  fp32 output;
 * accumulate != 0 adds into C.  Deterministic split over M through `workspace`
 * (vipant_gemm_tn_workspace_bytes).  a_colsum (optional fp32 [P]) (+)= sum_m A[m, p]: the bias gradient of the
 * same Linear, taken from the A tiles while they sit in LDS (no extra pass over dY). */
size_t vipant_gemm_tn_workspace_bytes(int64_t M, int64_t P, int64_t Q);
int32_t vipant_gemm_tn(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc,
                       int64_t M, int64_t P, int64_t Q, int32_t accumulate, float* a_colsum, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Two contractions of one shape in one launch: C0 = A0^T . B0 and C1 = A1^T . B1 (the two feature gradients of the InfoNCE loss,
 * cvap/module/decoder/loss_head.py:276-283: together they fill the chip with half the splits of two separate launches). */
size_t vipant_gemm_tn_pair_workspace_bytes(int64_t M, int64_t P, int64_t Q);
int32_t vipant_gemm_tn_pair(const uint16_t* A0, const uint16_t* B0, float* C0, const uint16_t* A1, const uint16_t* B1, float* C1,
                            int64_t lda, int64_t ldb, int64_t ldc, int64_t M, int64_t P, int64_t Q, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Column sums over tokens (bias gradients): out[N] (+)= sum_m X[m, n]; X bf16 [M, N]. */
size_t vipant_colsum_workspace_bytes(int64_t M, int64_t N);
int32_t vipant_colsum_bf16(const uint16_t* X, int64_t ldx, float* out, int64_t M, int64_t N, int32_t accumulate,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- LayerNorm (clip/model.py:154-160: fp32 statistics, eps 1e-5) -----------------------------------
 * x rows (fp32, or fp16 with VIPANT_STREAM_IN_F16 in `stream_flags`, below; row stride ldx elements) -> y bf16 [M, D] (optional);
 * mean / rstd fp32 [M] saved for backward.  y_f32 (optional, may be NULL) receives the fp32 result as well (ln_pre writes the
 * residual stream).
 * add (optional bf16 [M, D]): the residual add `x + branch` of ResidualAttentionBlock.forward (cvap/module/val.py:520-521)
 * fused in front of the norm; sum_out (optional [M, D], fp32 or -- VIPANT_STREAM_OUT_F16 -- fp16) receives x + add (the new
 * residual stream).
 * q / qscale (optional, both or neither; here and in vipant_layernorm_bwd): the block quantisation of the bf16 output fused into the
 * pass (the row is in registers anyway): q bytes [M, D] / qscale bytes [vipant_mx_scale_bytes(M, D)] = vipant_quant_e4m3_mx of y
 * resp. dx_bf16, bit for bit. */
int32_t vipant_layernorm_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, uint16_t* y, float* y_f32,
                             float* mean, float* rstd, int64_t M, int64_t D, const uint16_t* add, void* sum_out, uint8_t* q,
                             uint8_t* qscale, int32_t stream_flags, void* stream);
/* Precision of the residual stream INSIDE the transformer stack (`stream_flags` of the operators below): fp32, or fp16 -- the
 * reference's own autocast precision (clip/model.py:157-160 casts the fp32 LayerNorm result back to the fp16 stream) -- with fp32
 * statistics and the norm taken on the unrounded sum.  IN: the `x` argument is fp16; OUT: the `x_out` / `sum_out` argument is. */
#define VIPANT_STREAM_IN_F16 1
#define VIPANT_STREAM_OUT_F16 2
#define VIPANT_STREAM_FEW_ROWS 0x100 /* (vipant_ln_mlp_quickgelu_bwd) its contractions are VIPANT_EPI_FEW_ROWS launches */
#define VIPANT_STREAM_ACT_Q 0x200 /* (vipant_ln_qkv_bwd) the plan's activation scratch already holds dqkv's e4m3 form (vipant_mha_bwd) */
/* out fp32 [M, D] = x (fp32, or fp16 with VIPANT_STREAM_IN_F16) + add bf16 (the last block's residual add, no norm behind it). */
int32_t vipant_residual_add(const void* x, const uint16_t* add, float* out, int64_t n, int32_t stream_flags, void* stream);
/* dx[M,D] = dres (optional residual-stream gradient) + LN'(dy); outputs dx_f32 (optional) and dx_bf16 (optional).
 * flags: VIPANT_LN_DY_F32 -- dy is fp32 [M,D] (else bf16); VIPANT_LN_DRES_BF16 -- dres is bf16 [M,D] (row stride D; may be the
 * same buffer as dx_bf16), else fp32 with row stride lddx (may alias dx_f32).  dgamma / dbeta fp32 [D] (+)= column reductions;
 * dx_colsum (optional fp32 [D]) (+)= sum over rows of the produced dx: the bias gradient of the Linear whose
 * output gradient this dx is (out_proj / c_proj), for free in the same pass. */
size_t vipant_layernorm_bwd_workspace_bytes(int64_t M, int64_t D);
#define VIPANT_LN_DY_F32 1
#define VIPANT_LN_DRES_BF16 2
#define VIPANT_LN_X_F16 4 /* x rows are fp16 (a saved fp16 stream) */
int32_t vipant_layernorm_bwd(const void* dy, int32_t flags, const void* x, int64_t ldx, const float* mean,
                             const float* rstd, const float* gamma, const void* dres, float* dx_f32, int64_t lddx,
                             uint16_t* dx_bf16, float* dgamma, float* dbeta, float* dx_colsum, int32_t accumulate,
                             int64_t M, int64_t D, void* workspace, size_t workspace_bytes, uint8_t* q, uint8_t* qscale,
                             void* stream);

/* ---- multi-head attention core (nn.MultiheadAttention inside ResidualAttentionBlock,
 *      cvap/module/val.py:511-517): softmax(q k^T / sqrt(64) [+ causal mask]) v, head dim 64 -----------
 * qkv bf16 [batch*S, 3*D] packed q|k|v (in_proj row order), out bf16 [batch*S, D]; lse fp32 [batch, H, S]
 * (natural-log row log-sum-exp of the scaled scores, saved for backward).
 * out_q / out_scale and dqkv_q / dqkv_scale (optional, both or neither; H even, i.e. D % 128 == 0): the call also leaves the e4m3 +
 * block-scale form of its result for the contraction that follows (out_proj; in_proj^T): `out` [M, D] and the dQ columns of `dqkv`
 * [M, 3 D] -- made by a pass behind the kernel -- in the block-uniform form (vipant_quant_e4m3_mx32, bit for bit; round 6), the
 * dK | dV columns the streamed backward emits from its own epilogue in the row-wise form (vipant_quant_e4m3_mx, bit for bit):
 * vipant_mx_uniform32_cols makes those uniform too where a weight gradient wants them.  The streamed single-pass backward
 * (224 < S <= 320, no mask) emits the dK | dV columns from its own epilogue; everything else -- dQ, the other backward shapes, the
 * forward -- is the stand-alone pass enqueued behind the kernel.  No reference counterpart (BASELINE.json configs[4]). */
int32_t vipant_mha_fwd(const uint16_t* qkv, uint16_t* out, float* lse, uint8_t* out_q, uint8_t* out_scale, int64_t batch, int64_t S,
                       int64_t H, int32_t causal, void* stream);
/* dqkv bf16 [batch*S, 3*D] from dout bf16 [batch*S, D]; delta fp32 [batch, H, S] is scratch. */
int32_t vipant_mha_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta,
                       uint16_t* dqkv, uint8_t* dqkv_q, uint8_t* dqkv_scale, int64_t batch, int64_t S, int64_t H, int32_t causal,
                       void* stream);

/* The patch embedding written straight into the token matrix (ViTPreEncoder, cvap/module/val.py:249-257): for m = item * P + patch,
 * tokens[item * (P + 1) + patch + 1, :] = A[m, :] . B^T + pos[patch + 1, :] (fp32, ldc = N); the class-token rows
 * tokens[item * S, :] = cls + pos[0, :] are vipant_tokens_cls_rows'. */
int32_t vipant_gemm_nt_tokens(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* tokens, const float* pos,
                              int64_t b, int64_t P, int64_t N, int64_t K, void* stream);
int32_t vipant_tokens_cls_rows(const float* cls, const float* pos, float* tokens, int64_t b, int64_t S, int64_t D, void* stream);

/* ---- the same attention for ONE query per (item, head): the last block of a tower on its read-out rows ----------
 * Both read-outs take one token per item from the stack's output (the class token, cvap/module/val.py:288-289; the
 * end-of-text token, val.py:143-145), so only that row of the last block's output is ever read and only it carries a
 * gradient: the block's per-token work runs on `batch` rows, and its attention has one query per (item, head) against all
 * keys (exact: dead rows eliminated, nothing approximated).  Row of item i: i * S + idx[i] (idx == NULL: the first row).
 * q_rows bf16 [batch, D]: the projected queries of those rows; qkv bf16 [batch*S, 3*D]: only its K and V column blocks are
 * read; causal: keys <= the row.  out_rows bf16 [batch, D]; probs fp32 [batch, H, S]: the softmax rows, saved for backward. */
int32_t vipant_mha_rows_fwd(const uint16_t* q_rows, const uint16_t* qkv, const int64_t* idx, uint16_t* out_rows, float* probs,
                            int64_t batch, int64_t S, int64_t H, int32_t causal, void* stream);
/* dq_rows bf16 [batch, D]; dK / dV of EVERY key row written into the K / V column blocks of dqkv bf16 [batch*S, 3*D] (zero
 * rows behind a causal limit); the Q column block of dqkv is not touched. */
int32_t vipant_mha_rows_bwd(const uint16_t* q_rows, const uint16_t* qkv, const int64_t* idx, const float* probs,
                            const uint16_t* dout_rows, uint16_t* dq_rows, uint16_t* dqkv, int64_t batch, int64_t S, int64_t H,
                            int32_t causal, void* stream);
/* The same one-query attention with the K / V projection folded into the query side (csrc/readout_ctx.hip): with one query per
 * (item, head) the scores are (W_k,h^T q_h) . h1_j / 8 (+ a constant the softmax drops) and the head's output is
 * W_v,h (sum_j p_j h1_j) + b_v,h, so the kernels run against the LayerNorm output h1 bf16 [batch*S, D] itself and the key / value
 * projection of every token (nn.MultiheadAttention's in_proj, clip/model.py:170-187 via cvap/module/val.py:519-522) is never formed.
 * qk bf16 [batch*H, D]: row (i, h) = W_k,h^T q_(i,h);  ctx bf16 [batch*H, D]: row (i, h) = sum_j p_j h1[i, j, :];
 * probs fp32 [batch, H, S] as above.  H = 8, 12 or 16 heads of 64 (D = 64 H); S <= 1024 (an item's raw scores wait
 * in LDS beside the staged rows: 64 KiB at H = 16).
 * pair != 0 (round 5, the step's default): qk, ctx (and dqk below; not dctx) are bf16 PAIRS, x = hi + lo, stored as two planes
 * [2][batch*H, D] (hi plane first): these per-(item, head) vectors carry 16 instead of 8 mantissa bits between the kernels that
 * produce and consume them, so the folded form adds no rounding the reference's attention does not have. */
int32_t vipant_rows_ctx_fwd(const uint16_t* qk, const uint16_t* h1, const int64_t* idx, uint16_t* ctx, float* probs, int64_t batch,
                            int64_t S, int64_t H, int32_t causal, int32_t pair, void* stream);
/* dctx bf16 [batch*H, D] (a single plane also with pair != 0): row (i, h) = W_v,h^T dout_(i,h).  dh1 bf16 [batch*S, D]: the attention's
 * gradient for EVERY token's h1 row (zeros behind a causal limit; all rows written);  dqk bf16 [batch*H, D] (a pair with pair != 0):
 * gradient of qk;  dbk fp32 [D] or NULL: the key bias's gradient, exact zeros (a bias on the keys cannot move a softmax over keys). */
int32_t vipant_rows_ctx_bwd(const uint16_t* qk, const uint16_t* dctx, const uint16_t* ctx, const uint16_t* h1, const int64_t* idx,
                            const float* probs, uint16_t* dh1, uint16_t* dqk, float* dbk, int64_t batch, int64_t S, int64_t H,
                            int32_t causal, int32_t pair, void* stream);
/* H independent products in one launch, C_h[M, N] = A_h[M, K] . B_h[N, K]^T (+ bias_h), bf16 in and out, operand h starting
 * h * stride elements behind operand 0: the per-head contractions of the folded form (a head's 64 columns of the `batch` read-out
 * rows against that head's block of W_k / W_v, and back) without the block-sparse [batch * H, D] operand of vipant_head_expand.
 * a_lo / c_lo != 0: A / C is a bf16 pair (see vipant_rows_ctx_fwd) whose lo plane lies a_lo / c_lo elements behind the hi plane: a
 * pair in A contributes both planes to the product, a pair in C receives bf16(acc) and bf16(acc - hi). */
int32_t vipant_gemm_nt_heads(const uint16_t* A, int64_t lda, int64_t stride_a, int64_t a_lo, const uint16_t* B, int64_t ldb,
                             int64_t stride_b, uint16_t* C, int64_t ldc, int64_t stride_c, int64_t c_lo, const float* bias,
                             int64_t stride_bias, int64_t M, int64_t N, int64_t K, int64_t H, void* stream);
/* rows bf16 [n, 64 H] -> out bf16 [n*H, 64 H]: row (i, h) = row i with every column outside head h's 64 zeroed -- the operand that
 * makes "per-head slice times the head's weight block" one dense contraction.  The step uses it for the two weight gradients of
 * the folded form (dW_v = expand(do)^T ctx, dW_k = expand(q)^T dqk through vipant_gemm_tn); the activations' products go through
 * vipant_gemm_nt_heads. */
int32_t vipant_head_expand(const uint16_t* rows, uint16_t* out, int64_t n, int64_t H, void* stream);
/* its inverse on a product: rows[i, 64 h + c] = full[(i, h), 64 h + c] (+ bias[64 h + c]); full bf16 or fp32 [n*H, 64 H]. */
int32_t vipant_head_extract(const void* full, int32_t full_is_f32, const float* bias, uint16_t* rows, int64_t n, int64_t H,
                            void* stream);
/* dst row i <- src row (i * rows_per_item + idx[i]) (idx == NULL: + 0); rows of row_bytes bytes, a multiple of 16. */
int32_t vipant_gather_rows_bytes(const void* src, const int64_t* idx, void* dst, int64_t n, int64_t rows_per_item, int64_t row_bytes,
                           void* stream);
/* x bf16 [*, D]: row (i * rows_per_item + idx[i]) <- bf16(row + add row i); add compact [n, D], fp32 (add_is_f32) or bf16. */
int32_t vipant_add_rows_bf16(uint16_t* x, const int64_t* idx, const void* add, int32_t add_is_f32, int64_t n,
                             int64_t rows_per_item, int64_t D, void* stream);

/* ---- elementwise / layout helpers ------------------------------------------------------------------
 * fp32 -> bf16 cast of a [R, C] matrix; dst_t (optional) receives the transpose [C, R]. */
int32_t vipant_cast_bf16(const float* src, uint16_t* dst, uint16_t* dst_t, int64_t R, int64_t C, void* stream);
/* The same for a list of matrices in one launch (all weight matrices of a tower once per step): device arrays of ntensors device
 * pointers src / dst / dst_t (entries of dst or dst_t may be NULL), row / column counts R, C, and tile_start[ntensors + 1], the
 * running sum of ceil(R/64) * ceil(C/64); total_tiles = tile_start[ntensors]. */
int32_t vipant_cast_bf16_multi(const float* const* src, uint16_t* const* dst, uint16_t* const* dst_t, const int32_t* R,
                               const int32_t* C, const int32_t* tile_start, int64_t ntensors, int64_t total_tiles, void* stream);
/* bf16 -> fp32 widening of n elements (n % 4 == 0). */
int32_t vipant_cast_f32(const uint16_t* src, float* dst, int64_t n, void* stream);
/* fp8 operands (BASELINE.json configs[4], "fp8 MFMA weights"; the reference has no counterpart -- its contractions are the
 * fp16 autocast matmuls of clip/model.py:170-187 -- so parity is against an exact emulation of this quantiser, tests/test_fp8_gpu.py).
 * bf16 rows x [M, K] -> OCP e4m3 rows q [M, K] with one power-of-two scale per row: scale[m] = e + 127 where e is the smallest
 * exponent with max|x[m, :]| / 2^e <= 448, q = round-to-nearest-even(x / 2^e).  K % 8 == 0, K <= 8192. */
int32_t vipant_quant_e4m3_rows(const uint16_t* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* scale, int64_t M, int64_t K,
                               void* stream);
/* The block format for ACTIVATIONS (round 5; what v_mfma_scale_f32_16x16x128_f8f6f4's scale operands take): one power-of-two scale per
 * 32 consecutive elements of a row, e = the smallest exponent with max|block| / 2^e <= 448, byte = e + 127, so that a producer can
 * quantise the 32 columns it holds without knowing the rest of the row.  The scale bytes are stored in the order the contraction
 * consumes them: byte of (row m, block kb = k / 32) at (((m / 128) * (K / 128) + kb / 4) * 16 + m % 16) * 32 + (kb % 4) * 8 + (m % 128) / 16;
 * vipant_mx_scale_bytes(M, K) = ceil(M / 128) * (K / 128) * 512 bytes (0 if K % 128 != 0).  K % 128 == 0. */
size_t vipant_mx_scale_bytes(int64_t M, int64_t K);
int32_t vipant_quant_e4m3_mx(const uint16_t* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* scale, int64_t M, int64_t K,
                             void* stream);
/* The same for K columns (K % 32 == 0) that start at column 32 * kb0 of rows 128 * kt_row elements long in the scale layout; x and q
 * point at the first of those columns. */
int32_t vipant_quant_e4m3_mx_cols(const uint16_t* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* scale, int64_t M, int64_t K,
                                  int64_t kt_row, int64_t kb0, void* stream);
/* Block-UNIFORM scales (round 6): the same bytes-plus-scales format with every scale shared by an aligned block of 32 rows x 32
 * columns (the byte is stored for each of the 32 rows, in the layout above, so the NT contractions read the matrix unchanged).  One
 * scale per (32 tokens, 32 columns) is also one scale per 32 k of a COLUMN, which is what v_mfma_scale_f32_16x16x128_f8f6f4 needs when k
 * runs along the token axis: the operand format of vipant_gemm_tn_e4m3.  vipant_quant_e4m3_mx32: from bf16 (e = the smallest exponent
 * with max|block| / 2^e <= 448 over the 32 x 32 block).  vipant_mx_uniform32: IN PLACE on an e4m3 matrix with row-wise block scales (what
 * the producers emit): the block's scale becomes the largest of its rows' scales, the other rows' bytes are divided by the power of
 * two -- exact unless a value falls below e4m3's normal range.  No reference counterpart (BASELINE.json configs[4]). */
int32_t vipant_quant_e4m3_mx32(const uint16_t* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* scale, int64_t M, int64_t K,
                               void* stream);
int32_t vipant_mx_uniform32(uint8_t* q, int64_t ldq, uint8_t* scale, int64_t M, int64_t K, void* stream);
/* The same two for K columns (K % 32 == 0) that start at column 32 * kb0 of rows 128 * kt_row elements long in the scale layout; x and q
 * point at the first of those columns (as vipant_quant_e4m3_mx_cols). */
int32_t vipant_quant_e4m3_mx32_cols(const uint16_t* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* scale, int64_t M, int64_t K,
                                    int64_t kt_row, int64_t kb0, void* stream);
int32_t vipant_mx_uniform32_cols(uint8_t* q, int64_t ldq, uint8_t* scale, int64_t M, int64_t K, int64_t kt_row, int64_t kb0, void* stream);
/* Weight-gradient contraction on e4m3 operands (BASELINE.json configs[4]; the autograd of nn.Linear weight, cvap/module/val.py:500-506,
 * as vipant_gemm_tn): C[P, Q] fp32 (+)= dequant(A, sa)^T dequant(B, sb), reduction over the token dimension M.  A [M, P], B [M, Q]:
 * token-major e4m3 bytes with block-uniform scales (above); lda / ldb = the row length of the quantised matrices (what their scale
 * layouts were written with), P and Q multiples of 128.  fp32 accumulation, deterministic split over M through `workspace`.
 * a_colsum (optional fp32 [P]) (+)= sum_m dequant(A)[m, p], taken from the A tiles while they sit in LDS, as in vipant_gemm_tn. */
size_t vipant_gemm_tn_e4m3_workspace_bytes(int64_t M, int64_t P, int64_t Q);
int32_t vipant_gemm_tn_e4m3(const uint8_t* A, int64_t lda, const uint8_t* sa, const uint8_t* B, int64_t ldb, const uint8_t* sb, float* C,
                            int64_t ldc, int64_t M, int64_t P, int64_t Q, int32_t accumulate, float* a_colsum, void* workspace,
                            size_t workspace_bytes, void* stream);
/* C[M, N] (bf16) = dequant(A, sa) dequant(B, sb)^T (+ bias) on v_mfma_scale_f32_16x16x128_f8f6f4 (fp32 accumulation; the scales ride
 * the instruction's block-scale operands).  A [M, K] e4m3: an activation, sa = its BLOCK scales (vipant_quant_e4m3_mx layout); B [N, K]
 * e4m3: a weight matrix, sb = one scale per row (vipant_quant_e4m3_rows).  Epilogues: VIPANT_EPI_BF16, VIPANT_EPI_QUICKGELU_D8,
 * VIPANT_EPI_DQUICKGELU_D8, meaning as in vipant_gemm_nt.  cq / cq_scale (both or neither; the two QuickGELU epilogues, N % 128 == 0):
 * the epilogue ALSO leaves the e4m3 form of its bf16 result, bytes [M, N] (row length N) + block scales in the MX layout, in the
 * BLOCK-UNIFORM form of vipant_quant_e4m3_mx32: one scale per aligned block of 32 rows x 32 columns.  The scale is taken from a bound
 * on the block (the largest |acc + bias| of the wave that holds it, times 1.01, resp. 1.11 for QuickGELU'), not from the block's exact
 * maximum: it is never below what the block's largest element needs (nothing saturates) and at most two binades above it, so the
 * scales are NOT those of vipant_quant_e4m3_mx32 bit for bit; the bytes are C / 2^e rounded to e4m3 under the scale written.  Bytes
 * and scale bytes are written for rows below M only (in a last 32-row block that straddles M, the rows beyond M keep whatever
 * cq_scale held).  It is the next
 * contraction's A operand quantised where it is produced; with cq set, C may be NULL (only the e4m3 form is wanted), and with
 * VIPANT_EPI_QUICKGELU_D8 aux too (no codes).  K % 128 == 0, K >= 256, N % 8 == 0, leading dimensions (in elements = bytes) multiples of 16. */
int32_t vipant_gemm_nt_e4m3(const uint8_t* A, int64_t lda, const uint8_t* sa, const uint8_t* B, int64_t ldb, const uint8_t* sb,
                            void* C, int64_t ldc, const float* bias, void* aux, uint8_t* cq, uint8_t* cq_scale, int64_t M, int64_t N,
                            int64_t K, int32_t epilogue, void* stream);
/* conv1.weight [O, Cin, kh, kw] fp32 -> effective GEMM weight bf16 [O, Cout*kh*kw]; mean_channels != 0
 * averages the Cin stored channels into one (cvap/module/val.py:236-244), else Cout = Cin. */
int32_t vipant_conv_weight_prep(const float* w, uint16_t* out, int64_t O, int64_t Cin, int64_t khw,
                                int32_t mean_channels, void* stream);
/* im2col for the patch conv (cvap/module/val.py:245-252): x fp32 [b, C, T, F] -> bf16 [b*nrow*ncol, C*ph*pw],
 * patch (i, j) at (i*sh, j*sw), row order t-major (token = i*ncol + j). */
int32_t vipant_im2col(const float* x, uint16_t* out, int64_t b, int64_t C, int64_t T, int64_t F, int64_t ph,
                      int64_t pw, int64_t sh, int64_t sw, void* stream);
/* backward of the token assembly tokens[b, 0, :] = cls + pos[0]; tokens[b, 1+p, :] = patches[b*P + p, :] + pos[1+p] (val.py:253-257;
 * the forward is vipant_gemm_nt_tokens + vipant_tokens_cls_rows): dpatches bf16 [b*P, D], dcls [D] and dpos [S, D] fp32 (+)=. */
int32_t vipant_assemble_tokens_bwd(const float* dtokens, uint16_t* dpatches, float* dcls, float* dpos,
                                   int32_t accumulate, int64_t b, int64_t P, int64_t D, void* stream);
/* effective-kernel gradient [O, khw] fp32 -> conv1.weight.grad [O, Cin, khw] (+)= g / Cin per channel. */
int32_t vipant_conv_weight_grad(const float* g, float* wgrad, int64_t O, int64_t Cin, int64_t khw,
                                int32_t accumulate, void* stream);
/* y = x / ||x||_2 per row (clip_head.py:117-118); norm fp32 [M] saved. fp32 [M, E]. */
int32_t vipant_l2norm_fwd(const float* x, float* y, float* norm, int64_t M, int64_t E, void* stream);
/* dx = (dy - y * <dy, y>) / norm; dx_bf16 optional copy. */
int32_t vipant_l2norm_bwd(const float* dy, const float* y, const float* norm, float* dx, uint16_t* dx_bf16,
                          int64_t M, int64_t E, void* stream);
/* token_embedding[text] + pos[:L]  (GPTPreEncoder, val.py:117-121): tokens i64 [b, L] -> x fp32 [b*L, D];
 * eot i64 [b] = argmax over the row. */
int32_t vipant_embed_tokens(const int64_t* tokens, const float* table, const float* pos, float* x, int64_t* eot,
                            int64_t b, int64_t L, int64_t D, void* stream);
/* gather rows: out[i, :] = x[i * rows_per_item + idx[i], :] (EOT read-out, val.py:145); idx NULL = row 0. fp32. */
int32_t vipant_gather_rows(const float* x, const int64_t* idx, float* out, int64_t n, int64_t rows_per_item,
                           int64_t D, void* stream);
/* scatter-add of the read-out gradient back into a zeroed token-major gradient (backward of gather_rows). */
int32_t vipant_scatter_rows_bf16(const float* g, const int64_t* idx, uint16_t* dx_bf16, uint16_t* compact_bf16, int64_t n,
                                 int64_t rows_per_item, int64_t D, void* stream);
int32_t vipant_scatter_rows(const float* g, const int64_t* idx, float* dx, int64_t n, int64_t rows_per_item,
                            int64_t D, void* stream);

/* ---- InfoNCE (CELossHead.forward, cvap/module/decoder/loss_head.py:265-284) ---------------------------
 * x1, x2 fp32 [B, E] (L2-normalised); logit_scale is the raw parameter (s = min(exp(.), scale_max),
 * scale_max <= 0 means +inf).  loss = mean_i CE(s x1 x2^T, i) + mean_i CE(s x2 x1^T, i).
 * Gradients are produced for rows [row0, row0+nrows) only (the rank's slice of an all-gathered batch):
 * dx1, dx2 fp32 [nrows, E], scaled by grad_scale; dlogit_scale is the full-batch value * grad_scale.
 * Any of dx1 / dx2 / dlogit_scale may be NULL (forward only).  E % 64 == 0.  Up to 768 clips at E = 512 the call is three
 * launches of row-block kernels (no B x B operand in HBM but the fp32 logits themselves, 2 B^2 floats); above, 256 x 256 tile
 * kernels whose s.dZ makes a bf16 round trip.  Same results within the rounding of the bf16 gradient operands.
 * Strip form (round 5; B > 768, 0 < nrows <= 768, E = 512 -- one rank of an N-GPU step): pass 1 keeps the fp32-grade logits of the
 * strip's rows of Z and of Z^T (2 nrows B floats), one launch forms the strip's gradients from them; nothing B x B is stored, and
 * vipant_infonce_strip_workspace_bytes(B, E, nrows) (55 MB at B = 4096 / 512 rows against 181 MB) is enough workspace. */
size_t vipant_infonce_workspace_bytes(int64_t B, int64_t E);
size_t vipant_infonce_strip_workspace_bytes(int64_t B, int64_t E, int64_t nrows);
int32_t vipant_infonce_fwd_bwd(const float* x1, const float* x2, const float* logit_scale, float scale_max,
                               float* loss, float* dx1, float* dx2, float* dlogit_scale, float grad_scale,
                               int64_t B, int64_t E, int64_t row0, int64_t nrows, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- Several InfoNCE terms over shared operands (VACELossHead.forward, cvap/module/decoder/loss_head.py:572-598) ----
 * x: HOST table of nop <= 5 device matrices, fp32 [B, E], L2-normalised.  pair_a / pair_b: HOST tables of npair <= 5 operand indices,
 * a_k != b_k; pair k is vipant_infonce_fwd_bwd(x[a_k], x[b_k]) with the raw logit_scale[k] (DEVICE, [npair]) and the HOST values
 * scale_max[k] (<= 0: none) and weight[k].
 *   loss[k]          (DEVICE, [npair + 1]) the unweighted loss of pair k, the single-pair call's; loss[npair] = sum_k weight[k] loss[k],
 *                    summed in ascending k on the device;
 *   dx[i]            (HOST table of device pointers; the table or an entry may be NULL: no gradient for that operand) fp32 [nrows, E]
 *                    = grad_scale * sum_{k with i in pair k} weight[k] * dloss_k/dx_i for the rows [row0, row0 + nrows): written in
 *                    full, summed in ascending k, no atomics -- the same bits on every call;
 *   dlogit_scale[k]  (DEVICE, [npair], or NULL) = weight[k] * grad_scale * dloss_k/dlogit_scale_k, 0 where the clamp is active.
 * Refused with VIPANT_EBADSHAPE before anything is written: an operand with a gradient pointer that is in no pair, an index out of
 * range, a_k == b_k, nop or npair outside 1 .. 5, E % 64 != 0.
 * B <= 768 at E = 512 (the step's own batch): three launches whatever the pair count -- one split / transpose of every operand, one
 * log-sum-exp launch over all (pair, side), one gradient launch whose workgroups own (operand, 16 rows, 128 columns) and walk the
 * operand's pairs with s_k w_k dZ_k as the bf16 MFMA operand into ONE set of accumulators.  npair = 1, weight 1 gives the bits of
 * vipant_infonce_fwd_bwd.  Every other shape: the pairs one after another through vipant_infonce_fwd_bwd into workspace temporaries,
 * added into dx in ascending k.  No allocation and no synchronisation in the call.
 * Workspace: vipant_infonce_multi_workspace_bytes(B, E, nop, npair, nrows) is enough for any gradient table; the nrows = 0 size is
 * enough for a call that produces no feature gradient (nrows = 0, or no gradient pointer). */
size_t vipant_infonce_multi_workspace_bytes(int64_t B, int64_t E, int32_t nop, int32_t npair, int64_t nrows);
int32_t vipant_infonce_multi_fwd_bwd(const float* const* x, int32_t nop, const int32_t* pair_a, const int32_t* pair_b,
                                     int32_t npair, const float* logit_scale, const float* scale_max, const float* weight,
                                     float* loss, float* const* dx, float* dlogit_scale, float grad_scale, int64_t B,
                                     int64_t E, int64_t row0, int64_t nrows, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* ---- Retrieval evaluation (LossHead.report / retrieval_eval, cvap/module/decoder/loss_head.py:71-168) ----
 * x1 fp32 [N1, E] queries, x2 fp32 [N2, E] candidates (both L2-normalised by the caller), gold int32 [N1, G]
 * with entries in [0, N2).  Replaces `(x1 @ x2.t()).argsort(descending=True)` + `torch.where(ind == label)`:
 *   ranks[i, g] = #{ j : sim[i, j] > sim[i, gold[i, g]] }   (0-based position of the gold column in the sort)
 *   top1[i]     = argmax_j sim[i, j] (lowest j on ties); may be NULL.
 * The N1 x N2 similarity matrix is never stored.  E % 64 == 0, 1 <= G <= 64. */
size_t vipant_retrieval_workspace_bytes(int64_t N1, int64_t N2, int64_t E, int64_t G);
int32_t vipant_retrieval_ranks(const float* x1, const float* x2, const int32_t* gold, int32_t* ranks, int32_t* top1,
                               int64_t N1, int64_t N2, int64_t E, int64_t G, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- Log-mel front-end (cvap/data/audio/transform.py:12-35 -> torchaudio.compliance.kaldi.fbank with the parameters
 * of cvap/data/image_audio.py:119-126; padding / normalisation / SpecAugment masks of image_audio.py:183-207) ----
 * wave fp32 [b, wave_stride] (clip i valid for nsamples[i] samples), out fp32 [b, T, F] (= [b, 1, T, F]).
 * Frames: snip_edges, window_size / window_shift samples, zero-padded to nfft (512 / 1024 / 2048); per-frame DC removal,
 * pre-emphasis, `window` [window_size] (symmetric Hann for the reference), power spectrum, `banks` fp32 [F, nfft/2+1]
 * triangular mel weights whose non-zero support of row m is [bank_start[m], bank_start[m] + bank_len[m]), log with the
 * fp32-epsilon floor.  Frames past a clip's last whole window are 0 before normalisation.  zero_mean != 0 subtracts the
 * clip mean first (zero_mean_wf).  norm_std != 0: (x - norm_mean) / norm_std.  masks int32 [b, 4] = f0, f1, t0, t1
 * (SpecAugment: bins [f0, f1) and frames [t0, t1) set to 0), or NULL. */
size_t vipant_fbank_workspace_bytes(int64_t b);
int32_t vipant_fbank(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                     const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                     int64_t b, int64_t T, int64_t F, int32_t window_size, int32_t window_shift, int32_t nfft,
                     float preemphasis, int32_t zero_mean, float norm_mean, float norm_std, void* workspace,
                     size_t workspace_bytes, void* stream);
/* vipant_fbank with waveform mixup inside the launch (cvap/data/audioset_cls.py:374-398; zero_mean is implied).  mix_index int32
 * [b] = the partner clip IN THIS BATCH or -1 for "not mixed", mix_lambda fp32 [b]; both on the device.  With c_i = w_i - mean(w_i
 * over nsamples[i]): an unmixed clip is c_i; a mixed one is x[j] = lambda c_i[j] + (1 - lambda) (j < nsamples[p] ? c_p[j] : 0) for
 * j < nsamples[i] -- the partner truncated or zero-padded to the clip's length, always the ORIGINAL clip p, never its mixed
 * version -- minus the mean of x over nsamples[i].  From there on the pipeline is vipant_fbank's.  The mixed waveform is never
 * stored: the frame loader forms the samples from the two sources on the way into LDS; `workspace`
 * (vipant_fbank_mix_workspace_bytes(b)) holds the per-clip means only.  The mean reductions are fixed-order, no float atomics: two
 * runs are bit-identical, and a clip with mix_index -1 gets the bits of vipant_fbank(..., zero_mean = 1).  A mix_index outside
 * [-1, b) cannot be seen by the host: the kernel clamps it into the range (below -1: not mixed; b and above: clip b - 1) before
 * any use.  A NULL argument (masks excepted) or a bad shape is refused and nothing is written. */
size_t vipant_fbank_mix_workspace_bytes(int64_t b);
int32_t vipant_fbank_mix(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                         const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                         const int32_t* mix_index, const float* mix_lambda, int64_t b, int64_t T, int64_t F,
                         int32_t window_size, int32_t window_shift, int32_t nfft, float preemphasis, float norm_mean,
                         float norm_std, void* workspace, size_t workspace_bytes, void* stream);
/* vipant_fbank_mix whose partners may lie OUTSIDE the batch (the reference draws a clip's partner from the whole dataset in the loader
 * worker, audioset_cls.py:374-400; a file loader hands the device b clips plus up to b partner clips).  wave fp32 [nsrc, wave_stride]
 * and nsamples int64 [nsrc] with nsrc >= b; out fp32 [b, T, F] is made from rows 0 .. b-1 only: rows b .. nsrc-1 are read as
 * partners and produce no output (a row nobody points at is never read past its mean).  mix_index int32 [b] takes values in
 * [-1, nsrc); the kernel clamps what the host cannot see (below -1: not mixed; nsrc and above: row nsrc - 1).  The mix rule, the
 * fixed-order reductions and everything after them are vipant_fbank_mix's: with nsrc == b the two entry points give the same bits,
 * and for any partner layout the result equals rows 0 .. b-1 of vipant_fbank_mix over all nsrc rows with mix_index -1 for rows >= b.
 * Workspace: vipant_fbank_mix_src_workspace_bytes(nsrc, b) (nsrc clip means and b mixed means).  Refused before any launch, nothing
 * written: a NULL argument (masks excepted), b < 1, nsrc < b, wave_stride < 1, a bad T / F / nfft / window. */
size_t vipant_fbank_mix_src_workspace_bytes(int64_t nsrc, int64_t b);
int32_t vipant_fbank_mix_src(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                             const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                             const int32_t* mix_index, const float* mix_lambda, int64_t nsrc, int64_t b, int64_t T, int64_t F,
                             int32_t window_size, int32_t window_shift, int32_t nfft, float preemphasis, float norm_mean,
                             float norm_std, void* workspace, size_t workspace_bytes, void* stream);
/* vipant_fbank on a VIEW of every clip: the reference's waveform transforms and its crop rule (cvap/data/audio/transform.py:75-202
 * and :24-28) inside the launch.  A clip passes, in this order, through
 *   flip     s1[i] = s0[n0-1-i] when its flip draw is >= 0.5;
 *   scale    by the factor c of its draw: n2 = int(n1 c) (product in double, at most 2^24 - 1), base = float(j) / float(c) (IEEE
 *            fp32 division), r1 = trunc(base), r2 = min(r1 + 1, n1 - 1), r = base - r1, s2[j] = (1 - r) s1[r1] + r s1[r2]
 *            (one product and one fused multiply-add);
 *   pad      to pad_len when shorter: left = min(floor(u (pad_len - n2)), pad_len - n2 - 1); filled with s2[0] / s2[n2-1], or
 *            with padding_value when has_padding_value;
 *   crop     to crop_len when longer, by the CROP RULE: left = min(floor(u (n - len)), n - len - 1); with unbiased standard
 *            deviations, when the window's is below half the whole signal's the head [0, len) is taken instead, and when the
 *            head's is lower still, the tail;
 *   noise    when its snr draw is >= 0: sigma = sqrt(10^((10 log10(mean(s4^2)) - snr) / 10) + 1e-7), s5[k] = s4[k] + sigma z(k), z a
 *            counter-based normal: Philox4x32-10, key (seed low word, seed high word ^ clip), counter (k >> 2, 0, 0, 0), output word
 *            k & 3 for sample k; Box-Muller over the word pairs (0, 1) and (2, 3) with u = ((word >> 9) + 0.5) 2^-23:
 *            sqrt(-2 log u) cospi(2 v) for the even member of a pair, sinpi for the odd one;
 *   the pipeline's crop to final_len by the same rule (drawn when `train`; otherwise centred, left = 0.5 (n - len) rounded half
 *            to even) -- always;
 *   minus the mean of the result when zero_mean.
 * `stages` (VIPANT_VIEW_*) enables flip / scale / pad / crop / noise for the whole batch.  draws fp64 [b, 6] on the device =
 * (flip, scale, pad u, crop u, snr or < 0 for "no noise", final u) per clip.  The host cannot see them: a u outside [0, 1) is
 * clamped into it and a scale that is not positive leaves the clip unscaled.  None of the intermediate signals is stored:
 * `workspace` (vipant_fbank_view_workspace_bytes(b)) holds one 64-byte plan per clip, resolved by one reduction launch (fixed
 * order, statistics in double, no float atomics), and the frame loader maps each sample back to its one or two source samples.
 * A plan is sixteen 32-bit words: int32 n0, n2 (after scale), n3 (after pad), n4 (after crop), n_out, flags (1 flipped, 2 scaled,
 * 4 noisy), pad_left, crop_left, final_left (the lefts of what the rule TOOK); fp32 c, fill_l, fill_r, sigma, mean; the Philox key.
 * A clip no stage touches (and no longer than final_len) gets the bits of vipant_fbank(..., zero_mean).  From the waveform on the
 * pipeline is vipant_fbank's.  vipant_wave_view writes the final waveform itself (same plan, same sample function, same bits):
 * wave_out fp32 [b, out_stride], zero beyond a clip's length, and the lengths (at most out_stride) as nsamples_out int64 [b].
 * A NULL argument (masks excepted), b = 0 or a bad shape is refused and nothing is written. */
#define VIPANT_VIEW_FLIP 1
#define VIPANT_VIEW_SCALE 2
#define VIPANT_VIEW_PAD 4
#define VIPANT_VIEW_CROP 8
#define VIPANT_VIEW_NOISE 16
typedef struct vipant_view_params {
    int64_t pad_len, crop_len, final_len;
    uint64_t seed;
    float padding_value;
    int32_t has_padding_value, train, zero_mean, stages, reserved;
} vipant_view_params;
size_t vipant_fbank_view_workspace_bytes(int64_t b);
int32_t vipant_fbank_view(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                          const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                          int64_t b, int64_t T, int64_t F, int32_t window_size, int32_t window_shift, int32_t nfft,
                          float preemphasis, float norm_mean, float norm_std, vipant_view_params view, const double* draws,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Two masked views of ONE filter-bank evaluation: what the siamese dataset's FbankTransform returns (cvap/data/audio/transform.py:223-258,
 * called at cvap/data/image_audio.py:256-285) -- the same log-mel under two SpecAugment mask sets.  Arguments, vipant_view_params, draws
 * and workspace are vipant_fbank_view's; out / masks belong to the first view and out2 / masks2 to the second, each fp32 [b, T, F] /
 * int32 [b, 4] (f0, f1, t0, t1), either mask NULL = no mask for that view.  One plan launch, one filter-bank launch.  Per view and row:
 * a live row (inside the clip's frames and outside that view's time mask) holds the value, 0 under that view's frequency mask; a row
 * inside that view's time mask holds 0; a row beyond the clip's frames holds the padding value, 0 under that view's frequency mask.
 * out has the bits of vipant_fbank_view(masks) and out2 those of vipant_fbank_view(masks2) for the same draws: a pair of frames that
 * is live alike in both views is transformed once and stored twice; where a time-mask edge of one view splits a pair, each view gets
 * a transform with exactly its own live frames (at most four such pairs per clip).  Every element of both outputs is written once.
 * out2 NULL, or out2 overlapping out, is refused before any launch, as is everything vipant_fbank_view refuses. */
int32_t vipant_fbank_view_pair(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, float* out2,
                               const float* window, const float* banks, const int32_t* bank_start, const int32_t* bank_len,
                               const int32_t* masks, const int32_t* masks2, int64_t b, int64_t T, int64_t F, int32_t window_size,
                               int32_t window_shift, int32_t nfft, float preemphasis, float norm_mean, float norm_std,
                               vipant_view_params view, const double* draws, void* workspace, size_t workspace_bytes, void* stream);
int32_t vipant_wave_view(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* wave_out, int64_t out_stride,
                         int64_t* nsamples_out, int64_t b, vipant_view_params view, const double* draws, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- PCM ingest (vipant_amd/csrc/pcm.hip): decoded 16-bit PCM -> the fp32 mono waveform of the front-end ----
 * What torchaudio.load(normalize=True) and the head of _extract_kaldi_spectrogram (cvap/data/audio/transform.py:15-21) compute per
 * file, for a ragged batch in one launch.  pcm int16 [b, pcm_stride] on the device: clip i holds nframes[i] frames of channels[i]
 * interleaved samples; nframes int64 [b] and channels int32 [b] are DEVICE arrays.  wave fp32 [b, wave_stride], nsamples_out int64 [b].
 *   VIPANT_PCM_FIRST  w[j] = pcm[j ch] * 2^-15 (channel 0: what kaldi.fbank takes when mean_channel is off, image_audio.py)
 *   VIPANT_PCM_MEAN   w[j] = (float(sum_c pcm[j ch + c]) * 2^-15) / float(ch): int32 sum, exact product, one IEEE fp32 division --
 *                     the bits of torch's (x.float() / 32768).mean(0) on the CPU
 * tile_len > 0 and 0 < n < tile_len: the clip is repeated to n * ceil(tile_len / n) samples (the reference's slice after torch.tile
 * truncates nothing).  A length above wave_stride is clamped to it.  nsamples_out[i] = the resulting length; wave[i, j] = 0 from there
 * to wave_stride; nothing outside [b, wave_stride] is written.  The host cannot see the device values: channels[i] is clamped into
 * [1, 8] before any use and nframes[i] into [0, pcm_stride / channels], so nothing outside a clip's row of pcm is read.
 * Refused with VIPANT_EBADSHAPE before any launch, nothing written: a NULL argument, b < 1, a stride < 1, tile_len < 0, an unknown mode.
 * No workspace; the same input gives the same bits on every run. */
#define VIPANT_PCM_FIRST 0
#define VIPANT_PCM_MEAN 1
int32_t vipant_pcm_wave(const int16_t* pcm, int64_t pcm_stride, const int64_t* nframes, const int32_t* channels, int32_t mode,
                        int64_t tile_len, float* wave, int64_t wave_stride, int64_t* nsamples_out, int64_t b, void* stream);

/* ---- image views (vipant_amd/csrc/image.hip): the image towers' input stage --------------------------------
 * Decoded uint8 frames in, normalised fp32 [b, 3, n, n] out: what the reference's loaders do per frame in PIL
 * (cvap/data/image/transform.py:11-18 make_clip_image_transform, :146-200 BarlowImageTransform; image_audio.py:117, 170-171, 232-237).
 * frames uint8 [b, max_h, max_w, 3] on the device with element strides (stride_b, stride_h, stride_w, 1); frame i occupies the top
 * left hw[i] = (h, w) pixels, the rest is padding nobody reads.  hw int32 [b, 2] and draws fp64 [b, 16] are HOST arrays (the loader
 * that decoded the frames knows both): every refusal is made on the host before anything is written, and the launch copies them
 * into the workspace on `stream` (from pageable memory such a copy cannot be captured into a graph; the caller keeps both arrays
 * alive until the stream has passed the call).
 *   draws = NULL: the `clip` chain.  Resize(n) (shorter side to n, longer to int(n * long / short)) + CenterCrop(n) (offset
 *            int(round((size - n) / 2.0)), half to even); only the output pixels inside the crop are computed, with the
 *            coefficients of the full resize.
 *   draws[i] = (box top, left, height, width; flip; the order of the four jitter operations 0 brightness, 1 contrast,
 *            2 saturation, 3 hue, or -1 for "no jitter"; their four factors in that numbering; gray; sigma, 0 = no blur; solarise):
 *            the integer box is cut from the frame and resampled to n x n, then flipped horizontally, jittered, turned gray,
 *            blurred and solarised as the row says.  params.chain (VIPANT_IMAGE_*) enables each stage for the whole batch.
 * The resample is PIL's Image.resize(BICUBIC) byte for byte: two separable passes, horizontal first, uint8 in between; per output
 * index scale = in / out, fs = max(scale, 1), support = 2 fs, center = (i + 0.5) scale, xmin = max(0, int(center - support + 0.5)),
 * xmax = min(in, int(center + support + 0.5)), weights bicubic((x - center + 0.5) / fs) (a = -0.5) normalised by their sum in double,
 * k = int(w 2^22 +- 0.5), result clip8((2^21 + sum k pixel) >> 22).  The photometric stages run on fp32 code values in [0, 255] and
 * nothing is quantised between them: L = floor((19595 r + 38470 g + 7471 b) / 65536 + 0.5) (PIL's convert("L")); brightness,
 * contrast, saturation = clip(deg + factor (x - deg)) with deg = 0, floor(mean(L) + 0.5), L (PIL's ImageEnhance); hue = colorsys
 * rgb -> hsv, h = frac(h + factor), -> rgb; blur = PIL's GaussianBlur(sigma): three extended box passes along the rows, then three
 * along the columns, clamp to the edge (s2 = sigma^2 / 3, L = sqrt(12 s2 + 1), l = floor((L - 1) / 2),
 * a = (2l + 1)(l (l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)), a pass = (inner 2l + 1 taps + a (the two outer taps)) / (2 (l + a) + 1));
 * a jitter operation whose factor is neutral (1, hue: 0) is skipped;
 * solarise = x >= 128 -> 255 - x; last ((x / 255) - mean) / std as three rounded fp32 operations.  The same input gives the same bits
 * on every run and in every batch.
 * Limits: n <= 224, and per axis a source extent (the frame's side for `clip`, the box's otherwise) of at most 8 times the resized
 * extent.  Refused with VIPANT_EBADSHAPE, nothing written: a frame or box beyond that, h or w < 1 or beyond max_h / max_w, a box that
 * is not an integer box inside its frame, a jitter order that is no permutation, a NULL argument (draws excepted), b < 1. */
#define VIPANT_IMAGE_FLIP 1
#define VIPANT_IMAGE_JITTER 2
#define VIPANT_IMAGE_GRAY 4
#define VIPANT_IMAGE_BLUR 8
#define VIPANT_IMAGE_SOLARISE 16
typedef struct vipant_image_params {
    int32_t n;
    float mean[3], std[3];
    int32_t chain;
} vipant_image_params;
size_t vipant_image_view_workspace_bytes(int64_t b, int64_t n, int64_t max_h, int64_t max_w);
int32_t vipant_image_view(const uint8_t* frames, int64_t stride_b, int64_t stride_h, int64_t stride_w, int64_t max_h, int64_t max_w,
                          const int32_t* hw, const double* draws, vipant_image_params params, float* out, int64_t b,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- LARS (cvap/module/lars.py:43-72), one fused pass per tensor list ---------------------------------
 * For tensor i (n[i] elements): dp = g + wd*p (adapt[i]); q = eta*|p|/|dp| (adapt[i], both norms > 0);
 * mu = momentum*mu + q*dp; p -= lr[i]*mu.  ptrs are device arrays of device pointers. */
size_t vipant_lars_workspace_bytes(int64_t ntensors);
int32_t vipant_lars_step(float* const* p, const float* const* g, float* const* mu, const int64_t* n,
                         const int32_t* adapt, const float* lr, int64_t ntensors, float weight_decay,
                         float momentum, float eta, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Barlow Twins loss head (BarlowLossHead, cvap/module/decoder/loss_head.py:287-328) -----------------------------------
 * Batch normalisation over the batch dimension (torch.nn.BatchNorm1d, training mode, loss_head.py:296-303, 313): x fp32 [M, N]
 * (row stride ldx) -> y bf16 [M, N] (row stride N) = [ReLU]((x - mean) * rstd [* gamma + beta]); mean / rstd fp32 [N] are the
 * biased batch statistics, saved for the backward.  gamma / beta (fp32 [N]) both NULL = affine=False; relu != 0 fuses the
 * projector's ReLU.  running_mean / running_var (optional, fp32 [N]) are updated in the same launches with `momentum` and the
 * unbiased variance; num_batches_tracked (optional, int64 [1]) is incremented.  M >= 2 (VIPANT_EBADSHAPE otherwise, as torch
 * refuses a one-row batch in training).  Deterministic: the column reductions are two-level through `workspace`
 * (vipant_batchnorm_workspace_bytes), no float atomics. */
size_t vipant_batchnorm_workspace_bytes(int64_t M, int64_t N);
int32_t vipant_batchnorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, int32_t relu, uint16_t* y,
                             float* mean, float* rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                             float momentum, float eps, int64_t M, int64_t N, void* workspace, size_t workspace_bytes,
                             void* stream);
/* dx bf16 [M, N] (row stride N) from dy fp32 [M, N] (row stride lddy, the gradient of the normalised [and rectified] output) and
 * the saved pre-normalisation x, mean, rstd; the ReLU mask is recomputed from x, gamma, beta.  The column sums dx needs run over
 * all M rows; dgamma / dbeta (fp32 [N], optional, (+)= with accumulate) are summed over rows [row0, row0 + nrows) only -- the
 * rows a replica owns.  Same workspace as the forward. */
int32_t vipant_batchnorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, int32_t relu, uint16_t* dx, float* dgamma, float* dbeta,
                             int64_t row0, int64_t nrows, int32_t accumulate, int64_t M, int64_t N, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The cross-correlation loss (loss_head.py:305-311, 318-327): c fp32 [N, N] = zn1^T zn2 un-scaled (vipant_gemm_tn over the batch,
 * K = M); the kernel applies 1 / M.  loss fp32 [3] = {on + lambd * off, on, off}, on = sum_i (c_ii - 1)^2, off = sum_{i != j} c_ij^2.
 * G / Gt (optional, together, bf16 [N, N]) receive g = d loss / d c * (1 / M) * grad_scale[0] (grad_scale: optional device fp32
 * scalar, the upstream gradient) and its transpose: dzn1 = zn2 . G^T and dzn2 = zn1 . G are two vipant_gemm_nt calls (B = G, Gt).
 * Deterministic two-level reduction through `workspace` (vipant_barlow_loss_workspace_bytes). */
size_t vipant_barlow_loss_workspace_bytes(int64_t N);
int32_t vipant_barlow_loss(const float* c, int64_t ldc, int64_t M, float lambd, float* loss, const float* grad_scale, uint16_t* G,
                           uint16_t* Gt, int64_t N, void* workspace, size_t workspace_bytes, void* stream);

/* ==== Classification loss heads (vipant_amd/csrc/classify.hip) ==============================================================
 * Both take the UNSCALED fp32 logits z [B, ldz] (C <= ldz valid columns) of the head's last Linear and the log temperature
 * `logit_scale` (device fp32 scalar), score rows [row0, row0 + nrows) and write, in one pass over a row held by one wave:
 * loss fp32 [1] = the sum of the scored rows' terms over the FULL denominator (B, or B * C), so the losses of disjoint row
 * ranges add up to the whole batch's; dz bf16 [B, ldd] (optional; scored rows only) = grad_scale * d loss / d z with columns
 * C .. ldd-1 written as zeros (the class dimension padded for the contractions); dscale fp32 [1] (optional) = grad_scale *
 * d loss / d logit_scale (the parameter is the log: the factor exp(logit_scale) is included).  Deterministic: fixed-order
 * two-level reductions through `workspace` (vipant_*_workspace_bytes(nrows)), no float atomics.
 *
 * vipant_softmax_ce: nn.CrossEntropyLoss()(exp(ls) * z, labels), cvap/module/decoder/loss_head.py:416-418.  labels int64 [B] on
 * the device; a label outside [0, C) cannot be seen by the host and is clamped into the range by the kernel.  pred int32 [B]
 * (optional) = arg-max column, the lowest index on exact ties (torch.argmax, loss_head.py:356-357).
 * vipant_bce_logits: nn.BCEWithLogitsLoss()(exp(ls) * z, targets), cvap/module/decoder/loss_more.py:66-69, 140-142, in the
 * overflow-safe max(x, 0) - x t + log1p(exp(-|x|)) form.  targets uint8 [B, ldt] (non-zero = 1); logit_scale may be NULL
 * (scale 1: `scaling: False`; dscale must then be NULL); prob fp32 [B, ldp] (optional) = sigmoid(exp(ls) * z).
 * vipant_bce_logits_soft: the same against SOFT targets fp32 [B, ldt] (mixup's lambda y + (1 - lambda) y', audioset_cls.py:400);
 * same arguments, same workspace (vipant_bce_logits_workspace_bytes).  dz = grad_scale * s * (sigmoid(x) - t) / (B C).  An
 * element whose target is exactly 0 or 1 takes vipant_bce_logits' arithmetic, so float {0, 1} targets give its outputs bit for
 * bit.  Targets outside [0, 1] are NOT clamped: the formula is evaluated as it stands. */
size_t vipant_softmax_ce_workspace_bytes(int64_t nrows);
int32_t vipant_softmax_ce(const float* z, int64_t ldz, const int64_t* labels, const float* logit_scale, float* loss, uint16_t* dz,
                          int64_t ldd, float* dscale, int32_t* pred, int64_t row0, int64_t nrows, float grad_scale, int64_t B,
                          int64_t C, void* workspace, size_t workspace_bytes, void* stream);
size_t vipant_bce_logits_workspace_bytes(int64_t nrows);
int32_t vipant_bce_logits(const float* z, int64_t ldz, const uint8_t* targets, int64_t ldt, const float* logit_scale, float* loss,
                          uint16_t* dz, int64_t ldd, float* dscale, float* prob, int64_t ldp, int64_t row0, int64_t nrows,
                          float grad_scale, int64_t B, int64_t C, void* workspace, size_t workspace_bytes, void* stream);
int32_t vipant_bce_logits_soft(const float* z, int64_t ldz, const float* targets, int64_t ldt, const float* logit_scale, float* loss,
                               uint16_t* dz, int64_t ldd, float* dscale, float* prob, int64_t ldp, int64_t row0, int64_t nrows,
                               float grad_scale, int64_t B, int64_t C, void* workspace, size_t workspace_bytes, void* stream);
/* Tagging targets from ragged class-id lists (the reference builds multi-hot rows of 527 as Python lists per item in the loader worker
 * and mixes them there, audioset_cls.py:400).  ids int32 [total]; offsets int32 [nsrc + 1]: row r's classes are
 * ids[offsets[r] : offsets[r+1]]; mix_index int32 [b] / mix_lambda fp32 [b] as in vipant_fbank_mix_src, or both NULL; y fp32 [b, C]:
 *   y[i, c] = lam_i [c in L_i] + (1 - lam_i) [c in L_p],  p = mix_index[i]
 * in fp32 with 1 - lam, each product and the sum rounded separately (the bits of lam * y + (1 - lam) * y[partner] on dense rows).
 * Without mix arguments, or with p < 0, y[i, c] is exactly [c in L_i].  Every element of y is written once by the one thread that
 * owns it (no memset-then-scatter: a duplicate id gives 1).  An id outside [0, C) is ignored; offsets are clamped so that nothing
 * outside ids[0 : total] is read (a decreasing pair is an empty list); mix_index is clamped like vipant_fbank_mix_src's.  One launch,
 * no workspace, no allocation, no synchronisation.  Refused, nothing written: NULL ids / offsets / y, total < 0, b < 1, nsrc < b,
 * C < 1, exactly one of the two mix pointers NULL. */
int32_t vipant_multihot_mix(const int32_t* ids, int64_t total, const int32_t* offsets, const int32_t* mix_index,
                            const float* mix_lambda, float* y, int64_t nsrc, int64_t b, int64_t C, void* stream);

/* ==== The fused operator set: one entry point per reference operator group, forward and backward ==========
 * Host-side compositions of the kernels above (vipant_amd/csrc/block.hip): same stream, no allocation, no synchronisation.
 * Fusion plan: a residual add rides on the NEXT LayerNorm pass (`add` bf16 [M,D] = the previous branch output, `x_out` fp32
 * [M,D] = x + add, both NULL for the first block); QuickGELU / QuickGELU' are epilogues of the c_fc / c_proj^T contractions;
 * bias gradients are column sums taken inside the weight-gradient contraction or inside the LayerNorm backward (`dx_colsum`).
 * Weights are bf16 copies of the fp32 parameters: `w` as stored ([out, in]), `w_t` transposed ([in, out]).
 * `workspace` of the backward entry points: vipant_block_workspace_bytes(M, D) bytes, 256-byte aligned. */
size_t vipant_block_workspace_bytes(int64_t M, int64_t D);

/* The `plan` argument of the block operators: e4m3 operands in their NT contractions (BASELINE.json configs[4], "fp8 MFMA weights").
 * plan == NULL: the bf16 operator.  Otherwise `plan` carries the pre-quantised weights (vipant_quant_e4m3_rows of the SAME matrices,
 * in the SAME orientation, as the bf16 weight arguments, which are then unused and may be NULL) and the scratch the operator
 * quantises its activation into; every NT contraction becomes vipant_gemm_nt_e4m3 on an activation block-quantised by its producer
 * (a LayerNorm pass, the epilogue of the contraction before it) or, for the two attention outputs, by vipant_mha_fwd / vipant_mha_bwd.
 * The weight-gradient contractions (unless tn_e4m3, below), LayerNorm, the attention core and the residual stream are unchanged
 * (bf16 / fp32).
 * w_q / w_scale: the operator's (first) weight; w2_q / w2_scale: the second weight of the MLP operators (forward: w_fc then w_proj;
 * backward: w_proj_t then w_fc_t), one scale per row; act_q: bytes [M, 4D] (the widest activation); act_scale: its block scales, one
 * per 32 elements of a row in the MX layout of vipant_quant_e4m3_mx, vipant_mx_scale_bytes(M, 4D) bytes. */
typedef struct vipant_fp8_plan {
    const uint8_t* w_q;
    const uint8_t* w_scale;
    const uint8_t* w2_q;
    const uint8_t* w2_scale;
    uint8_t* act_q;
    uint8_t* act_scale;
    /* optional (both or neither), bytes [M, 4D] + vipant_mx_scale_bytes(M, 4D): where the epilogue of an MLP operator's first
     * contraction (c_fc + QuickGELU forward, c_proj^T * QuickGELU' backward) leaves the e4m3 form of its result for the second one
     * (round 5: the producer quantises, no pass over the [M, 4D] activation).  NULL: the result is block-quantised by a separate pass. */
    uint8_t* emit_q;
    uint8_t* emit_scale;
    /* backward operators, optional (both or neither): bytes [M, D] + vipant_mx_scale_bytes(M, D) that accompany the bf16 stream gradient `dx_bf16` between
     * operators.  On entry they hold the quantised form of the incoming gradient (the operator's first contraction then skips its
     * quantisation pass); an operator that produces a new stream gradient (its LayerNorm backward) writes the new one's there. */
    uint8_t* dy_q;
    uint8_t* dy_scale;
    /* round 6, backward operators: tn_e4m3 != 0 -- the operator's WEIGHT-GRADIENT contractions run on e4m3 operands too
     * (vipant_gemm_tn_e4m3; emit_q / emit_scale are then required as a second scratch).  Operands whose e4m3 form the operator has at
     * hand (dy_q; du in emit_q; dqkv in act_q) are made block-uniform in place (vipant_mx_uniform32); the kept forward activation
     * -- g (MLP), the attention output (out_proj), ln_1's output (in_proj) -- is read from keep_q / keep_scale, ln_2's output from
     * keep2_q / keep2_scale, if the forward kept their block-uniform e4m3 forms, and is otherwise quantised from the bf16 argument
     * (vipant_quant_e4m3_mx32) into scratch.  The bias gradients (in_proj, c_fc) ride on the contraction as in the bf16 operators. */
    int64_t tn_e4m3;
    const uint8_t* keep_q;
    const uint8_t* keep_scale;
    const uint8_t* keep2_q;
    const uint8_t* keep2_scale;
} vipant_fp8_plan;

/* K2 -- ln_1 + packed in_proj of nn.MultiheadAttention (cvap/module/val.py:519-520, 500; clip/model.py:154-160).
 * h bf16 [M,D] = LN(x (+ add)), mean / rstd fp32 [M], qkv bf16 [M,3D] = h . w_qkv^T + b_qkv.  x / x_out: fp32, or fp16 as
 * `stream_flags` (VIPANT_STREAM_*) says. */
int32_t vipant_ln_qkv_fwd(const void* x, const uint16_t* add, void* x_out, const float* gamma, const float* beta,
                          const uint16_t* w_qkv, const float* b_qkv, uint16_t* h, float* mean, float* rstd, uint16_t* qkv,
                          int64_t M, int64_t D, const vipant_fp8_plan* plan, int32_t stream_flags, void* stream);
/* dstream fp32 [M,D]: in = gradient of the residual stream after this block's attention branch, out = gradient before the block
 * (in place); dx_bf16 its bf16 copy.  dstream == NULL: the gradient stream is kept in bf16 only -- dx_bf16 is read as the incoming
 * gradient and overwritten with the outgoing one (the forward stream stays fp32 or fp16; profiles/r2_stream_precision.md, model D).
 * dh bf16 [M,D] scratch; dw fp32 [3D,D], db fp32 [3D], dgamma / dbeta fp32 [D];
 * dx_colsum (optional fp32 [D]) = column sums of the produced gradient (= d c_proj.bias of the block below). */
int32_t vipant_ln_qkv_bwd(const uint16_t* dqkv, const uint16_t* w_qkv_t, const uint16_t* h, const void* x, const float* mean,
                          const float* rstd, const float* gamma, float* dstream, uint16_t* dx_bf16, uint16_t* dh, float* dw,
                          float* db, float* dgamma, float* dbeta, float* dx_colsum, int64_t M, int64_t D, void* workspace,
                          size_t workspace_bytes, const vipant_fp8_plan* plan, int32_t stream_flags, void* stream);

/* K4 -- out_proj (cvap/module/val.py:517, 520).  residual == NULL: out bf16 [M,N] = a . w^T + bias (the step's form: the add
 * happens in the next LayerNorm pass; a == NULL with a plan: vipant_mha_fwd has left the operand's e4m3 form in the plan's scratch);
 * residual fp32 [M,N]: out fp32 [M,N] = a . w^T + bias + residual (stand-alone form, plan == NULL only). */
int32_t vipant_gemm_bias_residual_fwd(const uint16_t* a, const uint16_t* w, const float* bias, const float* residual, void* out,
                                      int64_t M, int64_t N, int64_t K, const vipant_fp8_plan* plan, void* stream);
/* da bf16 [M,K] = dy . w (w_t = w^T, [K,N]); dw fp32 [N,K] = dy^T a.  (d bias = column sums of dy: see dx_colsum above.) */
int32_t vipant_gemm_bias_residual_bwd(const uint16_t* dy, const uint16_t* w_t, const uint16_t* a, uint16_t* da, float* dw,
                                      int64_t M, int64_t N, int64_t K, void* workspace, size_t workspace_bytes,
                                      const vipant_fp8_plan* plan, void* stream);

/* K5 -- ln_2 + c_fc + QuickGELU + c_proj (cvap/module/val.py:502-506, 521; clip/model.py:163-165).
 * h bf16 [M,D] = LN(x (+ add)); u = h . w_fc^T + b_fc; g bf16 [M,4D] = u * sigmoid(1.702 u); dcode uint8 [M,4D] = 8-bit code of
 * QuickGELU'(u) (all the backward needs of u: VIPANT_EPI_QUICKGELU_D8); y bf16 [M,D] = g . w_proj^T + b_proj. */
int32_t vipant_ln_mlp_quickgelu_fwd(const void* x, const uint16_t* add, void* x_out, const float* gamma, const float* beta,
                                    const uint16_t* w_fc, const float* b_fc, const uint16_t* w_proj, const float* b_proj,
                                    uint16_t* h, float* mean, float* rstd, uint8_t* dcode, uint16_t* g, uint16_t* y, int64_t M,
                                    int64_t D, const vipant_fp8_plan* plan, int32_t stream_flags, void* stream);
/* dcode, g again from the saved h (activation-memory plan `running.recompute_mlp`). */
int32_t vipant_mlp_quickgelu_recompute(const uint16_t* h, const uint16_t* w_fc, const float* b_fc, uint8_t* dcode, uint16_t* g,
                                       int64_t M, int64_t D, const vipant_fp8_plan* plan, void* stream);
/* dy bf16 [M,D] = gradient of the MLP branch output (= bf16 copy of the stream gradient); dstream as in vipant_ln_qkv_bwd;
 * du bf16 [M,4D], dh bf16 [M,D] scratch; dw_proj fp32 [D,4D], dw_fc fp32 [4D,D], db_fc fp32 [4D];
 * dx_colsum (optional fp32 [D]) = d out_proj.bias. */
int32_t vipant_ln_mlp_quickgelu_bwd(const uint16_t* dy, const uint16_t* w_proj_t, const uint16_t* w_fc_t, const uint8_t* dcode,
                                    const uint16_t* g, const uint16_t* h, const void* x, const float* mean, const float* rstd,
                                    const float* gamma, float* dstream, uint16_t* dx_bf16, uint16_t* du, uint16_t* dh,
                                    float* dw_proj, float* dw_fc, float* db_fc, float* dgamma, float* dbeta, float* dx_colsum,
                                    int64_t M, int64_t D, void* workspace, size_t workspace_bytes, const vipant_fp8_plan* plan,
                                    int32_t stream_flags, void* stream);

/* K1 -- ViTPreEncoder.forward (cvap/module/val.py:228-259): patch conv as im2col + contraction, cls token, positional table,
 * ln_pre.  x fp32 [b,C,T,F]; conv_w fp32 [Dw,Cw,ph,pw] (mean_channels != 0: the Cw stored channels are averaged, val.py:236-244);
 * scratch / saved: w_eff bf16 [Dw,kcols], patches bf16 [b*P,kcols], tokens fp32 [b*S,Dw] (kcols =
 * (mean_channels ? 1 : Cw)*ph*pw, P = nrow*ncol, S = P+1); out fp32 [b*S,Dw] = the residual stream; mean / rstd fp32 [b*S]. */
int32_t vipant_patch_embed_ln_fwd(const float* x, const float* conv_w, const float* cls, const float* pos, const float* gamma,
                                  const float* beta, uint16_t* w_eff, uint16_t* patches, float* tokens, float* out,
                                  float* mean, float* rstd, int64_t b, int64_t C, int64_t T, int64_t F, int64_t Dw, int64_t Cw,
                                  int64_t ph, int64_t pw, int64_t sh, int64_t sw, int32_t mean_channels, void* stream);
size_t vipant_patch_embed_ln_bwd_workspace_bytes(int64_t b, int64_t P, int64_t Dw, int64_t kcols);
/* dtokens fp32 [b*S,Dw], dpatches bf16 [b*P,Dw], dw_eff fp32 [Dw,kcols] scratch; dconv fp32 [Dw,Cw,khw] (mean_channels; else
 * dw_eff IS the weight gradient); dcls fp32 [Dw]; dpos fp32 [rows >= S, Dw] must arrive zeroed. */
/* dout: gradient of the residual stream the stack hands back -- fp32 [b*S,Dw], or (dout_bf16 != 0) its bf16 stream gradient as is. */
int32_t vipant_patch_embed_ln_bwd(const void* dout, int32_t dout_bf16, const float* tokens, const float* mean, const float* rstd, const float* gamma,
                                  const uint16_t* patches, float* dtokens, uint16_t* dpatches, float* dw_eff, float* dconv,
                                  float* dcls, float* dpos, float* dgamma, float* dbeta, int64_t b, int64_t P, int64_t Dw,
                                  int64_t Cw, int64_t khw, int32_t mean_channels, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* K6 / K7 -- the read-outs: ViTPostEncoder.forward (cvap/module/val.py:288-289) and GPTPostEncoder.forward (val.py:136-146) +
 * MetaHead's normalisation (clip_head.py:117-118).  (GPTPreEncoder.forward, val.py:109-122, is vipant_embed_tokens.)
 * feat fp32 [batch,E] = LN(x[b, idx_b]) . proj (proj_t = proj^T bf16 [E,D]); idx == NULL reads row 0 (cls) in place, else (the
 * end-of-text rows) the rows are gathered into `rows` fp32 [batch,D]; normalized != 0: out = feat / |feat|, norm fp32 [batch] (else out is unused). */
int32_t vipant_cls_ln_proj_l2norm_fwd(const float* x, const int64_t* idx, const float* gamma, const float* beta,
                                      const uint16_t* proj_t, float* rows, uint16_t* y, float* mean, float* rstd, float* feat,
                                      float* out, float* norm, int64_t batch, int64_t S, int64_t D, int64_t E, int32_t normalized,
                                      void* stream);
size_t vipant_cls_ln_proj_l2norm_bwd_workspace_bytes(int64_t batch, int64_t D, int64_t E);
/* dout fp32 [batch,E]; proj bf16 [D,E]; dfeat bf16 [batch,E], dy bf16 [batch,D], drows fp32 [batch,D] scratch; dx fp32 [batch*S,D]
 * zeroed by the caller; dproj fp32 [D,E]. */
/* dx (token-major, zeroed by the caller) receives the read-out rows' gradient; or, compact form: `drows` fp32 [batch, D] receives
 * them (always for idx != NULL; for the cls read-out when drows != NULL) and dx may be NULL -- the transformer stack's backward
 * scatters them into its bf16 stream gradient itself (vipant_scatter_rows_bf16) instead of reading a dense fp32 matrix of zeros. */
int32_t vipant_cls_ln_proj_l2norm_bwd(const float* dout, const float* out, const float* norm, const float* x, const int64_t* idx,
                                      const float* rows, const uint16_t* y, const float* mean, const float* rstd,
                                      const float* gamma, const uint16_t* proj, uint16_t* dfeat, uint16_t* dy, float* drows,
                                      float* dx, float* dproj, float* dgamma, float* dbeta, int64_t batch, int64_t S, int64_t D,
                                      int64_t E, int32_t normalized, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIPANT_HIP_H */
