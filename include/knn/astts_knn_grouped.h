/* astts_knn_grouped.h -- grouped and ranged search of a style bank (libastts.so, ABI 6; an addition to include/astts.h, which stays as
 * it is: the symbols here are exported by the same library and bound by astts/_lib_knn_grouped.py).
 *
 * Replaces MilvusClient.search(..., group_by_field=, group_size=, offset=, search_params={"params": {"radius":, "range_filter":}}).
 *
 * Result definition.  Take a query and the rows its row mask and the handle's tombstones allow.  Order them as astts_knn_search does:
 * closest first under the handle's metric, ties by row index ascending, scores evaluated in fp64.  Every row has a group code
 * group_of[row] in [0, n_groups).
 *   1. Range.  A row is eligible when its score lies inside the range; the bounds are compared, as doubles, with the fp64 score of the
 *      definition (the value out_score64 returns):
 *        COSINE / IP               radius < score <= range_filter
 *        L2 (squared distance)     range_filter <= score < radius
 *      Either bound may be absent.
 *   2. Groups.  The selected groups are the `limit` groups whose best eligible row comes first in that order.  Every selected group
 *      returns its `group_size` first eligible rows.
 *   3. Layout.  The outputs are [nq, limit * group_size]; groups appear in the order of their best rows; slot g * group_size + j holds the
 *      j-th row of the g-th group.  Missing rows and missing groups are idx -1 and score -inf (+inf for L2), as in astts_knn_search.
 *      Without grouping (group_of == NULL) every row is its own group; with group_size = 1 the result is then the plain search
 *      restricted to the range.
 * The ids are bit-exact with respect to this definition, and out_score / out_score64 of a hit are, bit for bit, what astts_knn_search
 * returns for that row under the same query: unlike Milvus' strict_group_size = False this is not an approximation.
 *
 * How it runs.  Queries are taken in chunks of at most 256.  A chunk runs in ROUNDS over per-query row masks held in the workspace:
 * a round is one astts_knn_search of the chunk under those masks (every scan route, the fp64 re-score, the certification and the exact
 * path as they are; tombstones are ANDed in there), knn_group_accept walks each query's hits in order and fills its slots, and
 * knn_group_mask takes out of each unfinished query's mask what can no longer be a hit: rows of full groups and, once `limit` groups
 * are open, rows of every other group (the rows the round returned have left the mask in knn_group_accept).  The round size is the
 * host's choice and not part of the result: 32 hits first (the single-pass finish), then 128, 512 and 1024.  The typical request --
 * limit 1..3 over many groups -- ends in one round.  Every round scans the bank again.
 *
 * After each round the host READS BACK the number of unfinished queries: one 4-byte copy and a synchronisation of `stream` per round
 * (as astts_knn_create synchronises).  This call is therefore not a launch-path call, cannot be captured into a graph, and is not the
 * ~22 us search: a round costs an astts_knn_search at k = 32 plus two small launches and that synchronisation.
 *
 * The handle must not be mutated (astts_knn_mutable.h) while the call runs. */
#ifndef ASTTS_KNN_GROUPED_H
#define ASTTS_KNN_GROUPED_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASTTS_KNN_GROUPED_DEFAULT_ROUNDS 64

/* Bytes of workspace astts_knn_search_grouped needs; 0 for arguments it would refuse.  n_groups = 0: no group codes (group_of NULL).
 * Follows the current n and the tombstone state of the handle, as astts_knn_workspace_bytes does. */
size_t astts_knn_grouped_workspace_bytes(const astts_knn_t* h, int32_t nq, int32_t limit, int32_t group_size, int32_t n_groups);
/* queries: fp32 [nq, d] device.  group_of: device int32 [n], NULL = every row its own group (n_groups is then not used beyond its
 * check); a row whose code lies outside [0, n_groups) is never returned.  radius / range_filter: HOST doubles, NULL = absent.
 * out_idx int64, out_score fp32, out_score64 fp64 (may be NULL): device [nq, limit * group_size].  row_mask / mask_stride, flags: as in
 * astts_knn_search.  workspace: 256-byte aligned device memory of at least astts_knn_grouped_workspace_bytes(h, nq, limit, group_size,
 * group_of ? n_groups : 0).  max_rounds: 0 = ASTTS_KNN_GROUPED_DEFAULT_ROUNDS.  *rounds_host (may be NULL): the rounds the chunk that
 * needed most of them took.
 * ASTTS_ERR_INVALID: limit * group_size outside 1..ASTTS_KNN_MAX_K, n_groups < 1, a non-null group_of with n_groups > n, an empty range
 * (COSINE / IP: radius >= range_filter; L2: range_filter >= radius; a NaN bound).
 * ASTTS_ERR_UNSUPPORTED: max_rounds ran out with queries unfinished (the message names how many); the outputs are then incomplete and
 * must not be used -- a partial answer is never returned as if it were whole. */
int astts_knn_search_grouped(astts_knn_t* h, const float* queries, int32_t nq, int32_t limit, int32_t group_size,
                             const int32_t* group_of, int32_t n_groups, const double* radius, const double* range_filter,
                             int64_t* out_idx, float* out_score, double* out_score64, const uint8_t* row_mask, int64_t mask_stride,
                             void* workspace, size_t workspace_bytes, int32_t flags, int32_t max_rounds, int32_t* rounds_host,
                             astts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
