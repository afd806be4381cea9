/* astts_knn_mutable.h -- a style bank that changes while it stays resident in HBM (libastts.so, ABI 6; an addition to include/astts.h,
 * which stays as it is: the symbols here are exported by the same library and bound by astts/_lib_knn.py).
 *
 * astts_knn_create packs an n x d bank once.  These calls append rows behind it, tombstone rows and squeeze the tombstones out,
 * without packing a row a second time: the per-row packing of the handle (tiled fp16 scan image, row-major exact plane, fp64 norm,
 * inverse norm, L2 bias) depends on the row alone, so a bank that grew returns, bit for bit, the ids and scores of a bank created at
 * once from the same rows.  The cost of an append is O(new rows), plus one copy of the bank whenever the capacity has to grow (at least
 * doubled, so amortised O(1) per row).
 *
 * The handle holds `capacity` rows, a multiple of 128 and >= n; rows [n, capacity) of its scan planes are zero.  astts_knn_create
 * allocates exactly align_up(n, 128).
 *
 * astts_knn_reserve, _append, _set_deleted and _compact synchronise `stream` before they return, as astts_knn_create does, and may
 * free and replace the handle's device memory.  They must not overlap an astts_knn_search of the same handle on another stream or
 * thread; this is the caller's duty and is not enforced.  A workspace sized by astts_knn_workspace_bytes before one of them may be too
 * small after it: ask again (it follows the current n, and a handle with tombstones adds the combined row mask). */
#ifndef ASTTS_KNN_MUTABLE_H
#define ASTTS_KNN_MUTABLE_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Grow every plane to at least `capacity` rows (rounded up to a multiple of 128), contents preserved.  Never shrinks: a capacity at
 * or below the current one is a no-op.  ASTTS_ERR_UNSUPPORTED past the row limit of astts_knn_create (1024 * 8192). */
int astts_knn_reserve(astts_knn_t* h, int64_t capacity, astts_stream_t stream);
/* rows: device [m][d], ASTTS_DTYPE_F16 or ASTTS_DTYPE_F32; they become rows n .. n + m - 1 and *first_row (may be NULL) the old n.
 * Grows by at least doubling when the capacity is short.  ASTTS_ERR_RANGE for a batch with a non-finite value, ASTTS_ERR_UNSUPPORTED
 * past the row limit: in both cases the handle -- n, capacity, every plane -- is as it was (the batch is checked before anything is
 * written).  A batch that is not fp16-exact promotes an fp16-exact handle: it gets the fp32 exact plane (old rows widened, which is
 * lossless), every row its power-of-two scale, and the certification bound its 2^-11 term -- the handle astts_knn_create builds from
 * the whole fp32 matrix.  m = 0 is a no-op. */
int astts_knn_append(astts_knn_t* h, const void* rows, int64_t m, int32_t dtype, astts_stream_t stream, int64_t* first_row);
/* Tombstone the m rows rows_host[0 .. m) (host memory): no search returns them any more, under any row mask and at any k.
 * ASTTS_ERR_INVALID for an index outside [0, n), with nothing deleted.  A row deleted twice counts once.  From the first delete to
 * the next astts_knn_compact every search of the handle runs as a masked one (astts_knn_route: masked = 1). */
int astts_knn_set_deleted(astts_knn_t* h, const int64_t* rows_host, int64_t m, astts_stream_t stream);
/* Remove the tombstoned rows from every plane; the survivors keep their order, the vacated tail is zeroed, the capacity stays, the
 * live mask is freed and the largest row norm recomputed.  A handle that is not fp16-exact stays so.  *new_n (may be NULL): rows left;
 * old_to_new_host (may be NULL): host int64 [old n], the new index of every old row, -1 for a removed one.  ASTTS_ERR_UNSUPPORTED when
 * no row would be left (a handle holds at least one row: destroy it instead); the handle is unchanged then. */
int astts_knn_compact(astts_knn_t* h, astts_stream_t stream, int64_t* new_n, int64_t* old_to_new_host);
/* rows, rows not tombstoned, rows allocated (outputs may be NULL) */
int astts_knn_stats(const astts_knn_t* h, int64_t* n, int64_t* live, int64_t* capacity);

#ifdef __cplusplus
}
#endif
#endif
