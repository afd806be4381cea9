/* astts_qknorm.h -- the per-head q / k RMSNorm of Qwen3, fused with RoPE (libastts.so, ABI 6; an addition to include/astts.h, which stays
 * as it is: the symbol here is exported by the same library and bound by astts/_lib_llm.py).
 *
 * In place on the q | k part of a fused q | k | v buffer x (fp16 [b * t, ld]): `heads` query heads then `kv_heads` key heads of
 * head_dim columns each, from column 0.  Per (row, head), all in fp32 on the head's head_dim fp16 values:
 *   r = rsqrt(mean(x^2) + eps)            the sum in a fixed order (same bits every run, no atomics)
 *   y = (x * r) * w                       w = q_norm_w for a query head, k_norm_w for a key head (fp32 [head_dim])
 *   out[i]        = y[i] cos_i - y[i + h] sin_i
 *   out[i + h]    = y[i + h] cos_i + y[i] sin_i        h = head_dim / 2, cos / sin fp32 [positions, h] as astts_op_rope_llama takes them
 * and ONE rounding to fp16 at the store.  Columns at and beyond (heads + kv_heads) * head_dim (v, row padding up to ld) are not touched.
 * A row of zeros stays zeros.  The position of a row is that of astts_op_rope_llama_ex: time_major says whether row = t * b_count + b or
 * b * t_count + t, and position = max(pos0 + t - shift[b], 0) with shift int32 [b] or NULL; time_major = 0 with shift = NULL is
 * astts_op_rope_llama's calling form.  The tables must cover every position used (pos0 + t rows).
 * head_dim 64 or 128 (any other value: ASTTS_ERR_UNSUPPORTED); x, the tables and the weights 16-byte aligned, ld a multiple of 8. */
#ifndef ASTTS_QKNORM_H
#define ASTTS_QKNORM_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

int astts_op_qknorm_rope(void* x_f16, const float* cos_tab, const float* sin_tab, const float* q_norm_w, const float* k_norm_w,
                         const int32_t* shift, int32_t b, int32_t t, int32_t time_major, int32_t heads, int32_t kv_heads, int32_t ld,
                         int32_t head_dim, int32_t pos0, float eps, astts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ASTTS_QKNORM_H */
