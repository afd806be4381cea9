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

#define ASTTS_TRAIN_ABI_VERSION 1

int32_t astts_train_abi_version(void);
const char* astts_train_last_error_string(void);

/* Causal grouped-query attention backward, head_dim 128, batch-major rows [b, t].
 * qkv: fp16 [b * t, ld_qkv] = q (heads * 128, RoPE applied) | k (kv_heads * 128, RoPE applied) | v (kv_heads * 128);
 * dout: fp16 [b * t, ld_dout], the gradient of the attention output (heads * 128 columns); lens: int32 [b] or NULL (right padding:
 * keys at or beyond are masked, queries at or beyond take and give no gradient); dqkv: fp16 [b * t, ld_dqkv] = dq | dk | dv, every
 * row of it written (zeros in the padding).  scale: 1 / sqrt(128).  The softmax statistics are recomputed: the workspace holds
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

#ifdef __cplusplus
}
#endif
#endif /* ASTTS_TRAIN_H */
