/* astts_train.h -- C ABI of libastts_train.so: the backward and optimizer kernels of LoRA fine-tuning (gfx950 only).
 *
 * A second library beside libastts.so (include/astts.h, whose ABI it leaves alone), with that ABI's conventions: every call returns
 * an int status (ASTTS_OK or a negative ASTTS_ERR_*; the message: astts_train_last_error_string), pointers are device pointers,
 * workspaces are explicit (sized by the *_workspace_bytes query beside the call), the stream is the last argument, nothing
 * synchronises.  No kernel here uses a floating-point atomic: reductions that span workgroups write fixed partial planes that a
 * second kernel merges in a fixed order, so every result is bit-for-bit repeatable.
 */
#ifndef ASTTS_TRAIN_H
#define ASTTS_TRAIN_H

#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 1: the version counts changes that break a caller.  The regulariser entry points and astts_train_lora_merge at the end of this header
 * were added under it; every earlier prototype is unchanged. */
#define ASTTS_TRAIN_ABI_VERSION 1

int32_t astts_train_abi_version(void);
const char* astts_train_last_error_string(void);

/* Causal grouped-query attention backward, head_dim d = 64 or 128 (any other value: ASTTS_ERR_UNSUPPORTED), batch-major rows [b, t].
 * qkv: fp16 [b * t, ld_qkv] = q (heads * d, RoPE applied) | k (kv_heads * d, RoPE applied) | v (kv_heads * d);
 * dout: fp16 [b * t, ld_dout], the gradient of the attention output (heads * d columns); lens: int32 [b] or NULL (right padding:
 * keys at or beyond are masked, queries at or beyond take and give no gradient); dqkv: fp16 [b * t, ld_dqkv] = dq | dk | dv, every
 * row of it written (zeros in the padding).  scale: 1 / sqrt(d).  The softmax statistics are recomputed: the workspace holds
 * the log-sum-exp and sum_j P_ij dP_ij of every (row, head, query).  All products (S, dP twice; dQ, dK, dV once) are
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation; P and dS are rounded to fp16 where they become MFMA operands. */
size_t astts_train_attn_gqa_bwd_workspace_bytes(int32_t b, int32_t t, int32_t heads);
int astts_train_attn_gqa_bwd(const void* qkv_f16, const void* dout_f16, const int32_t* lens, void* dqkv_f16, int32_t b, int32_t t,
                             int32_t heads, int32_t kv_heads, int32_t head_dim, int64_t ld_qkv, int64_t ld_dout, int64_t ld_dqkv,
                             float scale, void* workspace, size_t workspace_bytes, astts_stream_t stream);

/* y = x * rsqrt(mean(x^2) + eps) * w with w frozen: dres[rows, c] += dx(dy, x, w).  All fp32, rows contiguous. */
int astts_train_rmsnorm_bwd(const float* dy, const float* x, const float* w, float* dres, int64_t rows, int32_t c, float eps,
                            astts_stream_t stream);

/* out = silu(gate) * up: d(gate | up) fp16 [rows, 2f] from dout fp16 [rows, f] and gate | up fp16 [rows, 2f]. */
int astts_train_swiglu_bwd(const void* dout_f16, const void* gate_up_f16, void* dgate_up_f16, int64_t rows, int32_t f,
                           astts_stream_t stream);

/* In place on fp32 logits [rows, vocab] (row stride ld): (exp(logit - lse[row]) - onehot(targets[row])) * scale; a row whose
 * target is -1 becomes zeros.  lse: the log-sum-exp astts_op_head_logprob returns. */
int astts_train_xent_grad(float* logits, int64_t ld, const float* lse, const int32_t* targets, int64_t rows, int32_t vocab,
                          float scale, astts_stream_t stream);

/* G[n, k] (fp32, row stride ldg) = (accumulate ? G : 0) + alpha * sum_row U[row, n] * X[row, k].  U: fp16, or fp32 (u_f32 = 1:
 * rounded to fp16 as it is read) [rows, n] with row stride ldu; X: fp16 [rows, k] with row stride ldx.  MFMA with fp32 accumulation
 * over row slabs of astts_train_lora_grad_row_split() rows; the slabs' planes (workspace) are added in slab order. */
int32_t astts_train_lora_grad_row_split(void);
size_t astts_train_lora_grad_workspace_bytes(int64_t rows, int32_t n, int32_t k);
int astts_train_lora_grad(const void* u, int32_t u_f32, int64_t ldu, const void* x_f16, int64_t ldx, float* g, int64_t ldg,
                          int64_t rows, int32_t n, int32_t k, float alpha, int32_t accumulate, void* workspace,
                          size_t workspace_bytes, astts_stream_t stream);

/* out[0] = sum x[i]^2 over a flat fp32 buffer (two stages of fixed order, fp64 accumulation): the squared global gradient norm,
 * and not finite exactly when some x[i] is not. */
size_t astts_train_sumsq_workspace_bytes(int64_t n);
int astts_train_sumsq(const float* x, int64_t n, float* out, void* workspace, size_t workspace_bytes, astts_stream_t stream);

/* One AdamW step (decoupled weight decay) on flat fp32 buffers, with g' = grad_mul * g (clipping and loss un-scaling):
 *   p *= 1 - lr * weight_decay;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / bias_corr1) * m / (sqrt(v) / sqrt(bias_corr2) + eps),   bias_corr = 1 - beta^step (computed by the caller).
 * The hyper-parameters are doubles: 1 - beta, lr * weight_decay, lr / bias_corr1 and sqrt(bias_corr2) are formed in fp64 and rounded
 * once, as torch.optim.AdamW forms them; the element-wise arithmetic is fp32. */
int astts_train_adamw(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                      double weight_decay, double bias_corr1, double bias_corr2, double grad_mul, astts_stream_t stream);

/* ---- The regularisers of the reference's recipe: LoRA dropout and NEFTune, from a counter-based generator (csrc/train/philox.h).
 * Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds); no state, no atomics, no
 * stored masks -- a mask is regenerated wherever it is consumed.
 *   key     = the 64 bits of `seed`, low word then high word
 *   counter = (group low word, group high word, rng_stream, draw)
 *   rng_stream = layer * 8 + the projection's position in astts.llm.peft.PROJ for dropout (part j of a fused call uses
 *             rng_stream + j: the projections that share an input are neighbours in PROJ), 0xFFFFFFFF for NEFTune
 *   draw    = the number of training forwards run before this one (one per micro-batch, skipped steps included)
 * Dropout: a group is 8 consecutive columns of one row of the [rows, cin] input, group = (row * cin + col) / 8 (cin a multiple of
 * 8); element e of the group takes 16 bits of output word e >> 1, the low half when e is even, the high half when e is odd, and is
 * kept iff those bits are >= floor(p * 65536).  The scale 1 / (1 - p) multiplies fp32 accumulators, never an fp16 operand.
 * NEFTune: a group is 4 consecutive fp32 elements, element i uses word i & 3 of group i >> 2: u = ((bits >> 8) + 0.5) * 2^-24,
 * x += mag * (2 u - 1).  0 <= p < 1 everywhere; p = 0 keeps every element. */

/* The keep mask of one (seed, rng_stream, draw, p) as uint8 [rows, cin] (1 = kept).  The test hook that pins the generator. */
int astts_train_dropout_mask(void* mask_u8, int64_t rows, int32_t cin, double p, int64_t seed, uint32_t rng_stream, uint32_t draw,
                             astts_stream_t stream);

/* In place on the fp32 [rows, hidden] embedding output (hidden a multiple of 4): x += mag * (2 u - 1); the caller forms
 * mag = alpha / sqrt(T * hidden), T the micro-batch's padded length (trl's neftune_post_forward_hook; padding rows get noise too). */
int astts_train_neftune(float* x, int64_t rows, int32_t hidden, float mag, int64_t seed, uint32_t draw, astts_stream_t stream);

/* t[rows, parts * r] (fp16, row stride ldt): column block j = (mask_j o x) A_j^T / (1 - p).  x: fp16 [rows, cin] (row stride ldx);
 * a: the stacked fp16 [parts * r, cin] (row stride lda); parts <= 3, r a multiple of 8 up to 64; strides multiples of 8.  Every x
 * fragment is read once and masked per part in registers; v_mfma_f32_32x32x16_f16, fp32 accumulation, one rounding at the store. */
int astts_train_lora_down(const void* x_f16, int64_t ldx, const void* a_f16, int64_t lda, void* t_f16, int64_t ldt, int64_t rows,
                          int32_t cin, int32_t parts, int32_t r, double p, int64_t seed, uint32_t rng_stream, uint32_t draw,
                          astts_stream_t stream);

/* astts_train_lora_grad with n = parts * r, k = cin and the masks applied to X as it is read: rows j * r .. (j + 1) * r of G use
 * mask j, and alpha / (1 - p) scales the merged sum.  The same row slabs, workspace (astts_train_lora_grad_workspace_bytes(rows,
 * parts * r, cin)) and slab-order merge: bit-for-bit repeatable. */
int astts_train_lora_grad_dropout(const void* u, int32_t u_f32, int64_t ldu, const void* x_f16, int64_t ldx, float* g, int64_t ldg,
                                  int64_t rows, int32_t parts, int32_t r, int32_t cin, float alpha, int32_t accumulate, double p,
                                  int64_t seed, uint32_t rng_stream, uint32_t draw, void* workspace, size_t workspace_bytes,
                                  astts_stream_t stream);

/* dx[rows, cin] = residual + (1 / (1 - p)) * sum_j mask_j o (dt_j A_j), the masks applied in the epilogue.  dt: fp16
 * [rows, parts * r] (row stride lddt); at: the TRANSPOSED stack, fp16 [cin, parts * r] (row stride ldat); residual: fp32 [rows, cin]
 * contiguous; dx: fp32 (may be the residual itself) or fp16 (dx_f16 = 1) [rows, cin] contiguous.  One pass, 16-byte accesses. */
int astts_train_lora_dx_dropout(const void* dt_f16, int64_t lddt, const void* at_f16, int64_t ldat, const float* residual, void* dx,
                                int32_t dx_f16, int64_t rows, int32_t cin, int32_t parts, int32_t r, double p, int64_t seed,
                                uint32_t rng_stream, uint32_t draw, astts_stream_t stream);

/* ---- Evaluation while training: the live adapter merged into a second weight image (added under ABI 1, as the regularisers were).
 *   out[o, i] = fp16_rn(float(w[o, i]) + scaling * sum_{k < r} b[o, k] * a[part(o) * r + k, i]),   o < n, i < cin
 *   part(o)   = (o >= g1) + (o >= g2): the parts of a fused projection (q | k | v, gate | up); g1 = g2 = n for a single one
 * w, out: fp16 [n_pad, cin_pad] in astts_op_pack_weight's layout (n_pad a multiple of 128, cin_pad of 64); the padding rows and
 * columns of out are written as zeros.  a: the fp32 master [parts * r, cin]; b: the fp32 master [n, r] (the parts' B matrices back to
 * back); r a multiple of 8; g1 and g2 multiples of 32 (or n), 0 < g1 <= g2 <= n, equal only at n (two parts: g2 = n).  out may not overlap w: the frozen base survives.
 * fp32 throughout: one fma chain over k = 0 .. r - 1 per element, one more fma joins the base, one rounding to fp16; no atomics, so
 * the image is bit-for-bit repeatable. */
int astts_train_lora_merge(const void* w_f16, const float* a, const float* b, void* out_f16, int32_t n, int32_t cin, int32_t n_pad,
                           int32_t cin_pad, int32_t r, int32_t g1, int32_t g2, float scaling, astts_stream_t stream);

/* ---- Qwen3: the transpose of astts_op_qknorm_rope (include/llm/astts_qknorm.h; added under ABI 1), batch-major rows [b, t].
 * dqkv: fp16 [b * t, ld_dqkv], whose first (heads + kv_heads) * head_dim columns hold d(rotated q | k) as astts_train_attn_gqa_bwd
 * leaves them; they are overwritten with d(pre-norm q | k), the columns beyond (dv, padding) are not touched.  x_pre: the fp16 q | k
 * the forward op READ (kept by the trainer), [b * t, ld_x].  Per head, in one pass and in fp32: the rotation's transpose,
 * g = w o that, r = rsqrt(mean(x^2) + eps) and xh = x r recomputed from x_pre, dx = r (g - xh mean(g xh)), one rounding to fp16.
 * The norm weights are frozen: no weight gradient.  xh is never recovered from an output divided by w (w may hold zeros).  Fixed-order
 * sums inside the wave, no atomics: bit-for-bit repeatable.  head_dim 64 or 128 (else ASTTS_ERR_UNSUPPORTED); cos / sin fp32
 * [>= pos0 + t, head_dim / 2]; all pointers 16-byte aligned, the strides multiples of 8. */
int astts_train_qknorm_rope_bwd(void* dqkv_f16, int64_t ld_dqkv, const void* x_pre_f16, int64_t ld_x, const float* cos_tab,
                                const float* sin_tab, const float* q_norm_w, const float* k_norm_w, int32_t b, int32_t t, int32_t heads,
                                int32_t kv_heads, int32_t head_dim, int32_t pos0, float eps, astts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ASTTS_TRAIN_H */
