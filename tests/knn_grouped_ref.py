"""CPU reference of the grouped and ranged style-bank search (include/knn/astts_knn_grouped.h), for tests only.

It restates the definition directly on ``oracle.knn.scores_f64``: per query every allowed row is sorted fully by (closest, row) and the
list is walked once.  No rounds, no masks that change, no candidate lists: it shares no structure with the implementation.
"""
from __future__ import annotations

import numpy as np

from oracle import knn as oknn

METRIC_ID = {"COSINE": oknn.METRIC_COSINE, "IP": oknn.METRIC_IP, "L2": oknn.METRIC_L2}


def metric_scores(bank, queries, metric: str) -> np.ndarray:
    """fp64 ``[Q, N]`` of the metric's own value (L2: the squared distance, positive -- scores_f64 returns it negated)."""
    s = oknn.scores_f64(bank, queries, METRIC_ID[metric])
    return -s if metric == "L2" else s


def sorted_rows(scores_q: np.ndarray, metric: str) -> np.ndarray:
    """Row indices of one query, closest first, ties by row index ascending."""
    key = scores_q if metric == "L2" else -scores_q
    return np.lexsort((np.arange(scores_q.size), key))


def grouped_search(bank, queries, limit: int, group_size: int = 1, group_of=None, metric: str = "COSINE", radius=None,
                   range_filter=None, row_mask=None, scores=None):
    """-> (idx int64, score fp64) ``[Q, limit * group_size]``; -1 / -inf (+inf for L2) where a row or a group is missing.
    ``group_of``: ``[N]`` group codes, None = every row its own group.  ``row_mask``: ``[N]`` or ``[Q, N]``, non-zero = allowed (the
    tombstones of a bank are part of it here).  ``scores``: ``metric_scores`` of the same bank and queries, to share between cases."""
    sc = metric_scores(bank, queries, metric) if scores is None else scores
    nq, n = sc.shape
    allowed = np.ones((nq, n), bool) if row_mask is None else np.broadcast_to(np.asarray(row_mask) != 0, (nq, n))
    codes = np.arange(n) if group_of is None else np.asarray(group_of)
    slots = limit * group_size
    idx = np.full((nq, slots), -1, np.int64)
    val = np.full((nq, slots), np.inf if metric == "L2" else -np.inf, np.float64)
    for qi in range(nq):
        order = sorted_rows(sc[qi], metric)
        s = sc[qi, order]
        if metric == "L2":
            ok = (True if range_filter is None else range_filter <= s) & (True if radius is None else s < radius)
        else:
            ok = (True if radius is None else radius < s) & (True if range_filter is None else s <= range_filter)
        order = order[allowed[qi, order] & ok]            # the eligible rows, closest first
        codes_o = codes[order]
        uniq, first = np.unique(codes_o, return_index=True)
        chosen = uniq[np.argsort(first)][:limit]          # the groups in the order of their best rows
        for g, code in enumerate(chosen):
            members = order[codes_o == code][:group_size]
            idx[qi, g * group_size:g * group_size + members.size] = members
            val[qi, g * group_size:g * group_size + members.size] = sc[qi, members]
    return idx, val
