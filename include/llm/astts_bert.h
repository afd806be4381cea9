/* astts_bert.h -- the two row operators of a post-LayerNorm (BERT-family) encoder (libastts.so, ABI 6; an addition to include/astts.h,
 * which stays as it is: the symbols here are exported by the same library and bound by astts/_lib_bert.py).
 *
 * Both compute, per row of c fp32 values v, in fp32:
 *   m  = sum(v) / c;  d = v - m;  d = d - sum(d) / c      the mean first, then the centred values centred once more: the second step
 *                                                          removes the rounding of m itself (half an ulp of m, which for a row at
 *                                                          100 +- 0.01 is 4e-4 of its standard deviation)
 *   var = sum(d^2) / c                                     of the centred values; never E[v^2] - m^2
 *   y  = d * rsqrt(var + eps) * gamma + beta               (var + eps == 0: y = beta)
 * and write y twice: as fp32 (the residual stream) and as that same value rounded ONCE to fp16 (the next GEMM's operand).  Either
 * output may be NULL, not both.  The row is read once and stays in registers between the passes; every sum runs in a fixed order
 * (a lane's values in index order, then a butterfly over the lanes): no atomics, the same bits every launch.  A constant row gives
 * beta exactly.  c % 8 == 0 and 8 <= c <= 4096, any other c: ASTTS_ERR_UNSUPPORTED.  Every pointer 16-byte aligned, fp32 strides a
 * multiple of 4 and the fp16 stride a multiple of 8 elements, every stride >= c; anything else: ASTTS_ERR_INVALID.  An error launches nothing.
 *
 * astts_op_layernorm_dual: v = x[r, :] (fp32 [rows, ldx]).  y32 may be x itself (in place, ldy32 == ldx).
 *
 * astts_op_bert_embed_ln: v = word[ids[b, j]] + pos[pos_offset + j] + type[type_ids[b, j]] for j < lens[b]; rows at j >= lens[b] are
 * written as zeros.  ids / type_ids int32 [b, t] (type_ids NULL: type 0), lens int32 [b] (NULL: every row has t tokens), the tables
 * fp32 and contiguous ([vocab, c], [max_pos, c], [n_types, c]), the outputs contiguous [b * t, c].  pos_offset is 0 for BERT and
 * pad_token_id + 1 for RoBERTa / XLM-R on right-padded rows.  Every index is clamped into its table inside the kernel: no input reads
 * out of bounds (a host that wants an error for a bad id checks before the call). */
#ifndef ASTTS_BERT_H
#define ASTTS_BERT_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

int astts_op_layernorm_dual(const float* x, const float* gamma, const float* beta, float* y32, void* y16, int64_t rows, int32_t c,
                            int32_t ldx, int32_t ldy32, int32_t ldy16, float eps, astts_stream_t stream);

int astts_op_bert_embed_ln(const float* word, const float* pos, const float* type, const int32_t* ids, const int32_t* type_ids,
                           const int32_t* lens, const float* gamma, const float* beta, float* out32, void* out16, int32_t b, int32_t t,
                           int32_t c, int32_t vocab, int32_t max_pos, int32_t n_types, int32_t pos_offset, float eps, astts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ASTTS_BERT_H */
