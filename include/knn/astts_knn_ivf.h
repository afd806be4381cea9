/* astts_knn_ivf.h -- an IVF_FLAT index over a style bank: k-means lists, nprobe search (libastts.so, ABI 6; an addition to
 * include/astts.h, which stays as it is: the symbols here are exported by the same library and bound by astts/_lib_knn_ivf.py).
 *
 * Replaces create_index(..., {"index_type": "IVF_FLAT", "params": {"nlist": N}}) and search(..., param={"nprobe": P}) of a MilvusClient.
 *
 * The index over a bank handle h is: `nlist` centroids (fp32 [nlist, d]), list_of[row] for every row of h, and per list the ascending
 * row indices that belong to it.
 *
 * Assignment rule (holds after astts_knn_ivf_create and after every astts_knn_ivf_assign): list_of[row] is the centroid closest to the
 * row under the handle's metric, and "closest" is exactly what astts_knn_search with k = 1 returns for that row as a query against a
 * bank made of the centroids (fp64 scores, ties to the lowest list index).  The centroids are held as an astts_knn_t of their own: the
 * coarse step, at build and at search, IS astts_knn_search.
 *
 * Search result for (query, nprobe, k).  The probed lists P(q) are the min(nprobe, nlist) hits of astts_knn_search(centroid bank, q).
 * The result is the k closest rows among {row : list_of[row] in P(q)} that the row mask and the tombstones allow, ordered as
 * astts_knn_search orders them (fp64 score, ties by row index ascending); out_score / out_score64 of a hit are, bit for bit, what
 * astts_knn_search returns for that row under the same call (same queries, nq, k); missing hits are idx -1 and score -inf (+inf for L2).
 * So with nprobe >= nlist the result IS that of astts_knn_search, and for any nprobe it is that of astts_knn_search under the row mask
 * isin(list_of, P(q)): the index never returns a wrong row, it returns the exact answer over a smaller set.
 *
 * Training is deterministic (no atomics, fixed summation order): building twice gives byte-identical centroids and lists.
 *   nlist_eff = min(nlist, live rows); initial centroids = the caller's first nlist_eff rows, or the live rows at positions
 *   floor(i * live / nlist_eff); then `niter` Lloyd iterations -- assign by the rule above, then every centroid becomes the fp32 mean of
 *   its live rows taken in ascending row order (COSINE: of the rows scaled to unit norm; IP / L2: the plain mean; an empty list keeps its
 *   centroid) -- then one final assignment.  niter = 0 with given centroids is a pure assignment.
 * Nothing is promised about faiss' or Milvus' centroids: their seeding and their splitting of empty clusters are not restated here.
 *
 * astts_knn_ivf_create, _assign and _remap synchronise `stream` before they return, as astts_knn_create does.  astts_knn_ivf_search is a
 * launch-path call: it enqueues on `stream`, does not synchronise and reads nothing back.  None of them may overlap a mutation of h. */
#ifndef ASTTS_KNN_IVF_H
#define ASTTS_KNN_IVF_H
#include "../astts.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct astts_knn_ivf astts_knn_ivf_t;

#define ASTTS_KNN_IVF_DEFAULT_NITER 20 /* this project's choice, not a claim about Milvus */
#define ASTTS_KNN_IVF_SLICE_ROWS 64    /* rows of one list that one workgroup of the list scan owns */
#define ASTTS_KNN_IVF_MAX_NLIST 65535 /* lists are one dimension of the scan's grid */
#define ASTTS_KNN_IVF_MAX_DP 16384     /* d rounded up to 64 may not exceed this (one staged fp32 query = 64 KB of LDS) */

/* 1 <= nlist <= ASTTS_KNN_IVF_MAX_NLIST, niter >= 0.  init_centroids_host: HOST fp32 [nlist, d] (its first nlist_eff rows are used), or NULL.
 * ASTTS_ERR_INVALID: bad arguments, a handle without a live row.  ASTTS_ERR_UNSUPPORTED: d beyond ASTTS_KNN_IVF_MAX_DP. */
int astts_knn_ivf_create(astts_knn_t* h, int32_t nlist, int32_t niter, const float* init_centroids_host, astts_stream_t stream,
                         astts_knn_ivf_t** out);
int astts_knn_ivf_destroy(astts_knn_ivf_t* ivf);
/* lists (nlist_eff), rows of h the index covers, rows of the longest list (tombstoned rows count); outputs may be NULL */
int astts_knn_ivf_info(const astts_knn_ivf_t* ivf, int32_t* nlist, int64_t* n_indexed, int64_t* max_list_len);
/* centroids_host: HOST fp32 [nlist_eff, d]; list_of_host: HOST int32 [n_indexed]; either may be NULL.  Synchronises the device. */
int astts_knn_ivf_export(const astts_knn_ivf_t* ivf, float* centroids_host, int32_t* list_of_host);
/* After astts_knn_append: assigns rows [n_indexed, h.n) by the rule and rebuilds the list tables.  O(new rows) of scoring plus O(n)
 * integers for the tables; the centroids do not move. */
int astts_knn_ivf_assign(astts_knn_ivf_t* ivf, astts_knn_t* h, astts_stream_t stream);
/* After astts_knn_compact: old_to_new_host is what it returned (HOST int64 [n_indexed], -1 = removed), new_n the rows left.  The
 * survivors keep their lists; no retraining. */
int astts_knn_ivf_remap(astts_knn_ivf_t* ivf, const int64_t* old_to_new_host, int64_t new_n, astts_stream_t stream);
/* Bytes of workspace astts_knn_ivf_search needs; 0 for arguments it would refuse.  Follows max_list_len and min(nprobe, nlist). */
size_t astts_knn_ivf_workspace_bytes(const astts_knn_ivf_t* ivf, const astts_knn_t* h, int32_t nq, int32_t k, int32_t nprobe);
/* queries: fp32 [nq, d] device.  out_idx int64, out_score fp32, out_score64 fp64 (may be NULL): device [nq, k].  row_mask / mask_stride:
 * as in astts_knn_search.  workspace: 256-byte aligned device memory of at least astts_knn_ivf_workspace_bytes.
 * ASTTS_ERR_INVALID: h's row count is not the index's n_indexed (astts_knn_ivf_assign / _remap was forgotten), nprobe < 1, k outside
 * 1..ASTTS_KNN_MAX_K.  ASTTS_ERR_UNSUPPORTED: min(nprobe, nlist) > ASTTS_KNN_MAX_K (the coarse search returns no more).  Queries run in
 * chunks of at most 256. */
int astts_knn_ivf_search(astts_knn_ivf_t* ivf, astts_knn_t* h, const float* queries, int32_t nq, int32_t k, int32_t nprobe,
                         int64_t* out_idx, float* out_score, double* out_score64, const uint8_t* row_mask, int64_t mask_stride,
                         void* workspace, size_t workspace_bytes, astts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
