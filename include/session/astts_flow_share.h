/* astts_flow_share.h -- the two launches a joined pass of a flow session shares among its batches (libastts.so; an addition to
 * include/astts.h, which stays as it is: the symbols here are exported by the same library and bound by astts/_lib_session.py).
 *
 * A batch's result in a flow session must equal astts_flow_solve of that batch alone bit for bit.  Two operators made a row's bits
 * depend on the launch it ran in: astts_op_tfm_ffn_fused (a 32-row tile starts its sum over the hidden chunks at a chunk given by the
 * tile's index in the launch) and astts_op_gemm (kernel family and tile are planned from the row count).  The entry points here run
 * ONE launch over the rows of several batches in which every row runs the instruction sequence of its batch's own launch. */
#ifndef ASTTS_FLOW_SHARE_H
#define ASTTS_FLOW_SHARE_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* astts_op_tfm_ffn_fused over n_seg (1..4) row segments in one launch: segment s is rows [row0[s], row0[s] + rows[s]) of x / out /
 * attn_f16 (host arrays; ascending, without overlap, rows[s] >= 1).  Every segment is cut into 32-row tiles of its own, counted from its
 * own first tile: its rows get the bits of astts_op_tfm_ffn_fused(x + row0[s] * c, ..., m = rows[s]).  The other arguments are those
 * of astts_op_tfm_ffn_fused; out == x is allowed.  One segment: that very launch. */
int astts_op_tfm_ffn_fused_seg(const float* x, const void* w1_frag_f16, const float* b1, const void* w2_frag_f16, const float* b2, float* out,
                               int32_t n_seg, const int64_t* row0, const int64_t* rows, int32_t c, int32_t hidden, float eps,
                               const void* attn_f16, const void* wo_frag_f16, const float* bo, int32_t k0, const void* pf_ptr,
                               uint32_t pf_bytes, astts_stream_t stream);

/* astts_op_gemm with the kernel planned for plan_m rows (1 <= plan_m <= m) and launched over all m rows: kernel family and tile are
 * those astts_op_gemm chooses for a call of plan_m rows, grid and bounds follow m.  Launched over the rows of several batches of plan_m
 * rows each, every row gets the bits of its batch's own astts_op_gemm -- with act == ASTTS_ACT_NONE: the activation epilogue of a tile that
 * lies wholly inside the output and that of an edge tile evaluate GELU differently (fast erf / erff), so with an activation a batch whose
 * rows do not fill whole tiles keeps its bits only in a launch of its own.  ASTTS_ERR_UNSUPPORTED (nothing is launched) when the plan of
 * plan_m rows is the m <= 32 family and m > 32: that family does not serve more rows than it was planned for. */
int astts_op_gemm_planned(const void* x, int32_t x_f16, const void* w_f16, const float* bias, const float* residual,
                          const float* row_scale, void* out, int32_t out_f16, int64_t m, int32_t n, int32_t cin, int32_t cin_pad,
                          int32_t taps, int32_t lda, int32_t ldc, int32_t ldr, int32_t t_in, int32_t t_out,
                          int32_t stride, int32_t dil, int32_t pad, int32_t act, float alpha, float slope, const int32_t* in_lens,
                          int64_t plan_m, astts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
