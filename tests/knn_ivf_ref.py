"""numpy helpers of the IVF_FLAT tests (include/knn/astts_knn_ivf.h): the probed lists and the membership mask of a query from an index's
exported centroids / list_of, through oracle.knn.  The index needs no oracle of its own: its result is, by definition, the exact search
under the row mask ``isin(list_of, probes)``.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from oracle import knn as oknn

METRIC_ID = {"COSINE": oknn.METRIC_COSINE, "IP": oknn.METRIC_IP, "L2": oknn.METRIC_L2}


def probes(centroids, queries, nprobe: int, metric: str) -> np.ndarray:
    """int64 ``[Q, min(nprobe, nlist)]``: the lists a query probes, closest centroid first (ties to the lowest list index)."""
    return oknn.knn_search(centroids, queries, min(int(nprobe), len(centroids)), METRIC_ID[metric])[0]


def membership(list_of, probed) -> np.ndarray:
    """bool ``[Q, N]``: row n belongs to one of query q's probed lists."""
    list_of = np.asarray(list_of)
    return (list_of[None, None, :] == np.asarray(probed)[:, :, None]).any(axis=1)


def assignment(centroids, rows, metric: str) -> np.ndarray:
    """int64 ``[M]``: the closest centroid of every row (the k = 1 hit of the row against the centroids)."""
    return oknn.knn_search(centroids, np.asarray(rows, dtype=np.float32), 1, METRIC_ID[metric])[0][:, 0]


def sse(bank, centroids, list_of) -> float:
    """fp64 sum of squared distances of every row to its assigned centroid"""
    df = np.asarray(bank, dtype=np.float64) - np.asarray(centroids, dtype=np.float64)[np.asarray(list_of)]
    return float((df * df).sum())
