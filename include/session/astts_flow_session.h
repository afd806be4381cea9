/* astts_flow_session.h -- flow sessions of the Euler solver engine (libastts.so; an addition to include/astts.h, which stays as it
 * is: the symbols here are exported by the same library and bound by astts/_lib_flow_session.py).
 *
 * astts_flow_solve runs ONE batch through all its Euler steps in one call.  A session is a chain of estimator passes that further
 * batches of the same frame count can JOIN while earlier ones are still being solved: every launch of a pass then carries the
 * sequences of all admitted batches, each batch at its own Euler step.  The estimator keeps no state between steps except the batch's
 * own x, the time projection and the guidance update are per sequence, and every estimator kernel is per row or per sequence, so a
 * batch's result is bit-identical to astts_flow_solve of that batch alone.  The convolutions of the ResNet blocks
 * (astts_op_resnet_conv), the attention (astts_op_tfm_attn_fused), the feed-forward launch (astts_op_tfm_ffn_fused_seg: one launch
 * over a table of the batches' row segments) and every astts_op_gemm of batches whose plans agree (astts_op_gemm_planned) run once
 * for all batches (astts_flow_share.h; the environment's ASTTS_FLOW_SHARE=0, read per call, issues the last two per batch again).
 * astts_op_groupnorm, whose grid form depends on the sequence count, the input packing and the guidance + Euler update run once per
 * batch over the batch's own rows.
 *
 * A session holding one batch issues the launches of astts_flow_solve.  Everything is enqueued on the session's stream and no call
 * waits for the device.  Calls on one session are not thread-safe. */
#ifndef ASTTS_FLOW_SESSION_H
#define ASTTS_FLOW_SESSION_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct astts_flow_session astts_flow_session_t;

/* bytes of the workspace astts_flow_session_create takes (0: bad arguments) */
size_t astts_flow_session_bytes(const astts_flow_t* h, int32_t t, int32_t n_slots, int32_t rows_max, int32_t steps_max);
/* t: the frame count of every batch; n_slots 1..4; rows_max: guided rows of all admitted batches together; steps_max 1..32: the longest
 * solve.  workspace: 256-byte aligned device memory that lives as long as the session, as does the engine handle. */
int astts_flow_session_create(astts_flow_t* h, int32_t t, int32_t n_slots, int32_t rows_max, int32_t steps_max, void* workspace,
                              size_t workspace_bytes, astts_stream_t stream, astts_flow_session_t** out);
int astts_flow_session_destroy(astts_flow_session_t* s);
/* would astts_flow_session_admit take this batch now?  >= 0: the slot; -2: another frame count; -3: every slot taken; -4: not enough
 * free rows; -5: more steps than steps_max; -1: bad arguments */
int astts_flow_session_can_admit(const astts_flow_session_t* s, int32_t b, int32_t t, int32_t n_steps);
/* One batch -- the arguments of astts_flow_solve -- joins: its time path is evaluated for all its steps.  x, mu, spk and cond are
 * read (x updated in place) by every pass until the batch's last step; lens, t_host and dt_host are free when the call returns
 * (lens in stream order).  slot_out: the bit of this batch in astts_flow_session_step's mask. */
int astts_flow_session_admit(astts_flow_session_t* s, float* x, const float* mu, const float* spk, const float* cond, const int32_t* lens,
                             int32_t b, int32_t t, int32_t n_steps, const float* t_host, const float* dt_host, float cfg_rate,
                             int32_t* slot_out);
/* Enqueue up to k estimator passes over the sequences of all admitted batches, each followed by every batch's own guidance + Euler
 * update (fewer when all batches end earlier).  A batch whose last step falls inside is retired: its bit is set in finished_mask_out
 * and its slot and rows are free. */
int astts_flow_session_step(astts_flow_session_t* s, int32_t k, uint32_t* finished_mask_out);
/* out8: active-slot mask, guided rows in use, passes enqueued so far, batches carried by those passes (their sum), steps left of
 * slots 0..3 */
int astts_flow_session_state(const astts_flow_session_t* s, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif
