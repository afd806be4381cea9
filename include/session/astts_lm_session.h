/* astts_lm_session.h -- decode sessions of the acoustic-transformer engine (libastts.so, ABI 6; an addition to include/astts.h, which
 * stays as it is: the symbols here are exported by the same library and bound by astts/_lib_session.py).
 *
 * astts_lm_decode runs ONE group of rows, all at the same step, from one cache, for one call.  A session is a decode chain that a
 * second batch can JOIN while the first is still decoding: the chain's launches (72 per token at 14 layers, each a latency link) then
 * carry the rows of both, and neither batch waits for the other.  A row's tokens and logits are bit-identical to astts_lm_decode of its
 * batch alone: every decode kernel is row-independent, and a batch that joins at chain position P has its prefix keys placed at
 * [P - pos0, P) with its first valid key raised by the same shift, which the attention kernel does not see (it addresses keys and
 * position rows relative to the query and splits the key range from the row's first valid key).
 *
 * Memory: the session owns one time-major arena [t_arena][rows_max][2 d] fp16 per layer plus the workspace of rows_max rows --
 * layers * t_arena * rows_max * 4 d bytes: 0.94 GB at 14 layers, d = 1024, 1024 positions, 16 rows.  t_arena must be at least TWICE
 * the longest window (pos0 + n_steps - 1) that will be admitted: the chain runs from position t_arena / 2 to t_arena and is then moved
 * back (one copy kernel), which by that rule never overlaps.
 *
 * Only the decode-step kernels serve a session (<= 32 rows, fp16 cache and tables, d <= 1024); everything is enqueued on the
 * session's stream and no call waits for the device or for another thread.  Calls on one session are not thread-safe. */
#ifndef ASTTS_LM_SESSION_H
#define ASTTS_LM_SESSION_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct astts_lm_session astts_lm_session_t;

/* device bytes astts_lm_session_create allocates (0: bad arguments) */
size_t astts_lm_session_bytes(const astts_lm_t* h, int32_t rows_max, int32_t t_arena);
/* rows_max 1..32; t_arena / 2 may not pass the position tables (cfg.pos_center).  The engine handle must outlive the session. */
int astts_lm_session_create(astts_lm_t* h, int32_t rows_max, int32_t t_arena, astts_stream_t stream, astts_lm_session_t** out);
/* waits for the session's stream, then frees */
int astts_lm_session_destroy(astts_lm_session_t* s);
/* would astts_lm_session_admit take this batch now?  >= 0: the slot; -2: window longer than t_arena / 2; -3: both slots taken;
 * -4: no free rows beside the running group; -1: bad arguments */
int astts_lm_session_can_admit(const astts_lm_session_t* s, int32_t b, int32_t pos0, int32_t n_steps);
/* One prefilled batch -- the arguments of astts_lm_decode (kv_cache[l]: fp16 [t_max, b, 2d], rows < pos0 filled) -- joins the chain:
 * one copy kernel moves its valid prefix keys into the arena, logits0 goes to its rows of the workspace.  The prefill's cache and
 * logits0 are free once that is done (stream order); uniforms, forced_tokens, eos_min_rows, tokens_out and logits_out are used until
 * the batch's last step.  slot_out: 0 or 1, the bit of this batch in astts_lm_session_step's mask. */
int astts_lm_session_admit(astts_lm_session_t* s, const float* logits0, void* const* kv_cache, const int32_t* key_start, int32_t t_max,
                           int32_t b, int32_t pos0, int32_t n_steps, const float* uniforms, const int32_t* forced_tokens,
                           int32_t eos_min_steps, const int32_t* eos_min_rows, int32_t* tokens_out, float* logits_out, int32_t* slot_out);
/* Enqueue up to k token steps of every admitted batch as ONE chain over their rows (fewer when all batches end earlier).  A batch
 * whose last step falls inside only samples there and is retired: its bit is set in finished_mask_out and its slot is free. */
int astts_lm_session_step(astts_lm_session_t* s, int32_t k, uint32_t* finished_mask_out);
/* out6: active-slot mask, chain position, steps left of slot 0, of slot 1, rebases so far, longest admissible window */
int astts_lm_session_state(const astts_lm_session_t* s, int32_t* out6);

#ifdef __cplusplus
}
#endif
#endif
