"""GPU tests of the IVF_FLAT index (include/knn/astts_knn_ivf.h, astts.knn.StyleBank.build_index / search_ivf*, MilvusClient(use_index=True)).

The bars are exact.  The index returns, by definition, the exact search over the rows of the probed lists, so every IVF search is compared
BITWISE -- ids, fp32 scores, fp64 scores -- with the brute-force search of the same bank under the row mask ``isin(list_of, probes)``
(probes and mask built in numpy from the EXPORTED centroids and list_of through oracle.knn: tests/knn_ivf_ref.py), and its ids with
oracle.knn under that mask.  The oracle's fp64 scores are summed in another order than the kernels': they are compared within
``d * 2^-52`` of the product of the norms (the rounding of a d-term fp64 sum), not bitwise.

Shapes: d = 16 (one 64-wide piece, padded), 200 (dp = 256: padding inside a row), 6144 (the shipped width: sixteen pieces per lane, the
DIRECT route of the brute-force search and its own query norm), 96 in fp32 that is not fp16-exact (the fp32 exact plane).  nlist = 8 over
1000 rows gives lists of ~125 rows: two workgroup slices of ASTTS_KNN_IVF_SLICE_ROWS = 64 each.  nq = 257 crosses the 256-query chunk,
k = 33 and 100 the 32 hits of a brute-force pass and the 64 of an IVF selection pass."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import knn_ivf_ref as ref
from oracle import knn as oknn

pytestmark = pytest.mark.gpu

ALL_METRICS = ["COSINE", "IP", "L2"]
SLICE = 64          # ASTTS_KNN_IVF_SLICE_ROWS: rows of a list per workgroup of the scan
NQS = (1, 8, 257)
KS = (1, 3, 32, 33, 100)


# ------------------------------------------------------------------------------------------ cases (built once, never changed)
@functools.lru_cache(maxsize=None)
def case(key):
    """-> (bank, 257 queries, how many of the queries the oracle scores)"""
    n, d, dtype, seed = {"b16": (1000, 16, np.float16, 21), "b200": (1000, 200, np.float16, 22), "b6144": (520, 6144, np.float16, 23),
                         "b96f32": (300, 96, np.float32, 24)}[key]
    rng = np.random.default_rng(seed)
    bank = rng.standard_normal((n, d)).astype(dtype)
    if dtype == np.float32:
        assert not np.array_equal(bank.astype(np.float16).astype(np.float32), bank)
    q = (bank[rng.integers(0, n, 257)].astype(np.float32) + 0.7 * rng.standard_normal((257, d))).astype(np.float32)
    bank.setflags(write=False)
    q.setflags(write=False)
    return bank, q, (8 if d == 6144 else 257)


CASES = ["b16", "b200", "b6144", "b96f32"]
_SCORES, _BANKS = {}, {}


def oracle_scores(key, metric):
    """oracle.knn.scores_f64 of a case (larger = closer), computed once"""
    if (key, metric) not in _SCORES:
        bank, q, nor = case(key)
        _SCORES[(key, metric)] = oknn.scores_f64(bank, q[:nor], ref.METRIC_ID[metric])
        _SCORES[(key, metric)].setflags(write=False)
    return _SCORES[(key, metric)]


def indexed_bank(key, metric):
    """the case's bank on the GPU with an index of 8 lists, 3 Lloyd iterations; built once, never mutated"""
    from astts.knn import StyleBank

    if (key, metric) not in _BANKS:
        sb = StyleBank(case(key)[0], metric=metric)
        info = sb.build_index(8, niter=3)
        assert info == {"index_type": "IVF_FLAT", "nlist": 8, "n_indexed": sb.n, "max_list_len": info["max_list_len"]}
        assert info["max_list_len"] > SLICE or sb.n < 8 * SLICE      # a list longer than one workgroup's slice
        _BANKS[(key, metric)] = (sb,) + sb.index_export()
    return _BANKS[(key, metric)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def oracle_topk(sc, k, allowed, metric):
    """oracle.knn.knn_search from precomputed scores: -> (idx, fp64 score in the metric's own sign)"""
    idx, val = oknn.topk_from_scores(np.where(allowed, sc, -np.inf), k)
    idx = np.where(np.isneginf(val), -1, idx)
    return idx, (-val if metric == "L2" else val)


def check(sb, cent, list_of, bank, q, k, nprobe, metric, sc=None, mask=None, dead=None):
    """One IVF search against the definition: bitwise against the brute-force search under the membership mask, ids (and scores
    within the rounding of the sums) against the oracle for the first ``len(sc)`` queries.  ``mask``: the caller's row mask ([n] or
    [nq, n]); ``dead``: rows deleted from ``sb`` (the brute-force search skips them itself, the oracle gets them in its mask).
    -> (ids, probes)"""
    nq, n = q.shape[0], bank.shape[0]
    probed = ref.probes(cent, q, nprobe, metric)
    allowed = ref.membership(list_of, probed)
    if mask is not None:
        allowed = allowed & (np.broadcast_to(np.asarray(mask) != 0, (nq, n)))
    dev = sb.device
    qt = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    mt = None if mask is None else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).astype(np.uint8)).to(dev)
    idx, s32, s64 = (t.cpu().numpy() for t in sb.search_ivf_device(qt, k, nprobe, row_mask=mt, return_f64=True))
    at = torch.from_numpy(np.ascontiguousarray(allowed).astype(np.uint8)).to(dev)
    eidx, es32, es64 = (t.cpu().numpy() for t in sb.search_device(qt, k, row_mask=at, return_f64=True))
    assert np.array_equal(idx, eidx), (metric, nq, k, nprobe, np.argwhere(idx != eidx)[:5])
    assert np.array_equal(_bits(s32), _bits(es32)), (metric, nq, k, nprobe, np.argwhere(_bits(s32) != _bits(es32))[:5])
    assert np.array_equal(_bits(s64), _bits(es64)), (metric, nq, k, nprobe, np.argwhere(_bits(s64) != _bits(es64))[:5])
    none = np.inf if metric == "L2" else -np.inf
    assert np.all(s32[idx < 0] == none) and np.all(s64[idx < 0] == none)
    if sc is not None:
        nor = min(nq, sc.shape[0])
        live = np.ones(n, bool)
        if dead is not None:
            live[np.asarray(dead)] = False
        oidx, oval = oracle_topk(sc[:nor], k, allowed[:nor] & live, metric)
        kk = oidx.shape[1]
        assert np.array_equal(idx[:nor, :kk], oidx), (metric, nq, k, nprobe)
        hit = oidx >= 0
        bn = np.sqrt((np.asarray(bank, np.float64) ** 2).sum(1)).max()
        qn = np.sqrt((np.asarray(q[:nor], np.float64) ** 2).sum(1)).max()
        scale = 1.0 if metric == "COSINE" else qn * bn if metric == "IP" else (qn + bn) ** 2
        assert np.all(np.abs(s64[:nor, :kk][hit] - oval[hit]) <= 4 * bank.shape[1] * 2.0 ** -52 * scale)
    return idx, probed


# ------------------------------------------------------------------------------------------ the search against its definition
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("key", CASES)
def test_full_probe_equals_brute_force(key, metric):
    bank, q, _ = case(key)
    sb, cent, list_of = indexed_bank(key, metric)
    sc = oracle_scores(key, metric)
    for nprobe in (8, 13):                                  # nlist, and nlist + 5 (clamped)
        for nq in NQS:
            for k in KS:
                qt = torch.from_numpy(np.ascontiguousarray(q[:nq])).to(sb.device)
                got = sb.search_ivf_device(qt, k, nprobe, return_f64=True)
                exp = sb.search_device(qt, k, return_f64=True)              # no mask at all: StyleBank.search itself
                for g, e in zip(got, exp):
                    assert np.array_equal(_bits(g.cpu().numpy()), _bits(e.cpu().numpy())), (nprobe, nq, k)
                if nprobe == 8 and k in (3, 33):
                    check(sb, cent, list_of, bank, q[:nq], k, nprobe, metric, sc)
    hidx, hs = sb.search_ivf(q[:8], 3, 8)                   # the host convenience
    eidx, es = sb.search(q[:8], 3)
    assert np.array_equal(hidx, eidx) and np.array_equal(_bits(hs), _bits(es))


@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("key", CASES)
def test_partial_probe_equals_masked_brute_force(key, metric):
    bank, q, _ = case(key)
    sb, cent, list_of = indexed_bank(key, metric)
    sc = oracle_scores(key, metric)
    for nprobe in (1, 3):
        for nq in NQS:
            for k in KS:
                idx, probed = check(sb, cent, list_of, bank, q[:nq], k, nprobe, metric, sc)
                assert probed.shape == (nq, nprobe)
                assert np.all(np.isin(list_of[idx[idx >= 0]], np.arange(8)))
    # the index answers over a smaller set: with one probe of eight, some query's brute-force top hit lies outside its list (at d = 16,
    # where the lists' regions are small against the queries' noise; at d = 6144 every query probes the list of the row it was made from)
    if key == "b16":
        idx1, _ = check(sb, cent, list_of, bank, q, 1, 1, metric)
        assert np.any(idx1[:, 0] != sb.search(q, 1)[0][:, 0])


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_k_larger_than_the_candidates(metric):
    bank, q, _ = case("b16")
    sb, cent, list_of = indexed_bank("b16", metric)
    sc = oracle_scores("b16", metric)
    longest = int(np.bincount(list_of, minlength=8).max())
    for k in (longest + 1, 1000):                           # above every probed list, and far above (sixteen selection passes)
        idx, probed = check(sb, cent, list_of, bank, q[:8], k, 1, metric, sc)
        for qi in range(8):
            have = int((list_of == probed[qi, 0]).sum())
            assert np.all(idx[qi, :have] >= 0) and np.all(idx[qi, have:] == -1)


# ------------------------------------------------------------------------------------------ degenerate lists (centroids given, niter = 0)
def test_one_list_holds_every_row():
    from astts.knn import StyleBank

    bank, q, _ = case("b16")
    cent = np.full((8, 16), 1000.0, np.float32) * np.arange(8, dtype=np.float32)[:, None]      # list 0 at the origin, the rest far away
    sb = StyleBank(bank, metric="L2")
    info = sb.build_index(8, niter=0, centroids=cent)
    c2, list_of = sb.index_export()
    assert np.array_equal(c2, cent) and np.all(list_of == 0)
    assert info["max_list_len"] == 1000 and 1000 > 15 * SLICE          # sixteen slices of one list, seven lists without a row
    sc = oracle_scores("b16", "L2")
    for nq in (8, 257):
        for k in (3, 100):
            check(sb, cent, list_of, bank, q[:nq], k, 1, "L2", sc)      # every query probes list 0: the whole bank
            check(sb, cent, list_of, bank, q[:nq], k, 8, "L2", sc)
    # queries next to centroid 3: its list is empty, and with one probe there is nothing to return
    far = (cent[3] + q[:4]).astype(np.float32)
    idx, probed = check(sb, cent, list_of, bank, far, 3, 1, "L2")
    assert np.all(probed == 3) and np.all(idx == -1)
    sb.close()


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_as_many_lists_as_rows(metric):
    from astts.knn import StyleBank

    rng = np.random.default_rng(31)
    bank = rng.standard_normal((130, 32)).astype(np.float16)
    q = (bank[rng.integers(0, 130, 9)].astype(np.float32) + 0.3 * rng.standard_normal((9, 32))).astype(np.float32)
    cent = bank[:128].astype(np.float32)
    cent[5] = cent[4]                                       # a duplicate centroid: the tie goes to list 4, list 5 stays empty
    sb = StyleBank(bank, metric=metric)
    info = sb.build_index(128, niter=0, centroids=cent)
    _, list_of = sb.index_export()
    lens = np.bincount(list_of, minlength=128)
    assert info["nlist"] == 128 and lens[5] == 0 and lens.sum() == 130 and info["max_list_len"] == lens.max()
    assert lens.max() >= 2                                  # rows 5, 128 and 129 have no centroid of their own
    if metric != "IP":                                      # (under IP a long row can draw many rows; else a row's own centroid is its closest)
        assert lens.max() <= 4 and (lens == 1).sum() >= 121
    sc = oknn.scores_f64(bank, q, ref.METRIC_ID[metric])
    for nprobe in (1, 10, 128):
        for k in (1, 3, 40):
            check(sb, cent, list_of, bank, q, k, nprobe, metric, sc)
    # more lists asked for than rows: one list per live row
    sb.delete_rows([7, 8])
    info = sb.build_index(200, niter=0)
    cent, list_of = sb.index_export()
    assert info["nlist"] == 128 and cent.shape == (128, 32) and info["n_indexed"] == 130
    assert np.array_equal(cent, bank[np.delete(np.arange(130), [7, 8])].astype(np.float32))      # positions floor(i * 128 / 128) of the live rows
    check(sb, cent, list_of, bank, q, 3, 10, metric, sc, dead=[7, 8])
    sb.close()


def test_all_queries_probe_the_same_list():
    bank, _, _ = case("b200")
    sb, cent, list_of = indexed_bank("b200", "L2")
    rng = np.random.default_rng(32)
    q = (cent[2] + 0.01 * rng.standard_normal((40, 200))).astype(np.float32)       # forty queries beside one centroid
    for k in (3, 33):
        idx, probed = check(sb, cent, list_of, bank, q, k, 1, "L2")
        assert np.all(probed == 2) and np.all(list_of[idx] == 2)


# ------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_ties_across_lists_are_ordered_by_row(metric):
    from astts.knn import StyleBank

    rng = np.random.default_rng(33)
    bank = rng.integers(-2, 3, (600, 16)).astype(np.float16)        # every score is a small integer: exact in every summation order
    q = rng.integers(-2, 3, (9, 16)).astype(np.float32)
    sb = StyleBank(bank, metric=metric)
    sb.build_index(8, niter=2)
    cent, list_of = sb.index_export()
    sc = oknn.scores_f64(bank, q, ref.METRIC_ID[metric])
    for nprobe in (3, 8):
        for k in (10, 70):
            idx, _ = check(sb, cent, list_of, bank, q, k, nprobe, metric, sc)
            tied = 0
            for qi in range(9):
                s = sc[qi, idx[qi]]
                same = s[1:] == s[:-1]
                assert np.all(idx[qi, 1:][same] > idx[qi, :-1][same])
                tied += int((same & (list_of[idx[qi, 1:]] != list_of[idx[qi, :-1]])).sum())
            assert tied > 0                                 # equal scores that sit in different lists
    sb.close()


# ------------------------------------------------------------------------------------------ masks and tombstones
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_masks_and_tombstones(metric):
    from astts.knn import StyleBank

    rng = np.random.default_rng(34)
    bank = rng.standard_normal((600, 40)).astype(np.float16)
    q = (bank[rng.integers(0, 600, 9)].astype(np.float32) + 0.5 * rng.standard_normal((9, 40))).astype(np.float32)
    sc = oknn.scores_f64(bank, q, ref.METRIC_ID[metric])
    sb = StyleBank(bank, metric=metric)
    sb.build_index(8, niter=3)
    cent, list_of = sb.index_export()
    shared = rng.random(600) < 0.5
    per_query = rng.random((9, 600)) < 0.3
    first = ref.probes(cent, q, 1, metric)[:, 0]
    whole_list = list_of != first[0]                        # every row of query 0's closest list is masked
    for dead in (None, np.unique(np.concatenate([rng.permutation(600)[:60], np.flatnonzero(list_of == first[1])[:5]]))):
        if dead is not None:
            sb.delete_rows(dead)
        for mask in (None, shared, per_query, whole_list):
            for nprobe, k in ((1, 3), (3, 40), (8, 3)):
                idx, _ = check(sb, cent, list_of, bank, q, k, nprobe, metric, sc, mask=mask, dead=dead)
                if dead is not None:
                    assert not np.isin(idx, dead).any()
        idx, _ = check(sb, cent, list_of, bank, q[:1], 3, 1, metric, sc[:1], mask=whole_list, dead=dead)
        assert np.all(idx == -1)
    sb.close()


# ------------------------------------------------------------------------------------------ the index itself
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("key", ["b16", "b96f32"])
def test_assignment_invariant_and_repeatable_build(key, metric):
    from astts.knn import StyleBank

    bank, _, _ = case(key)
    dead = np.array([3, 50, 51, 299])
    sb = StyleBank(bank, metric=metric)
    for niter, with_dead in ((0, False), (3, False), (3, True)):
        if with_dead:
            sb.delete_rows(dead)
        sb.build_index(8, niter=niter)
        cent, list_of = sb.index_export()
        sb.build_index(8, niter=niter)
        cent2, list_of2 = sb.index_export()
        assert cent.tobytes() == cent2.tobytes() and list_of.tobytes() == list_of2.tobytes()
        assert cent.shape == (8, bank.shape[1]) and list_of.shape == (bank.shape[0],)
        live = np.ones(bank.shape[0], bool)
        if with_dead:
            live[dead] = False
        if niter == 0:                                      # the start: live rows at positions floor(i * live / nlist)
            rows = np.flatnonzero(live)[(np.arange(8) * int(live.sum())) // 8]
            assert np.array_equal(cent, bank[rows].astype(np.float32))
        cb = StyleBank(cent, metric=metric)
        by_search = cb.search(bank.astype(np.float32), 1)[0][:, 0]
        cb.close()
        assert np.array_equal(list_of[live], by_search[live])
        assert np.array_equal(list_of[live], ref.assignment(cent, bank, metric)[live])
    sb.close()


def test_training_descends():
    from astts.knn import StyleBank

    rng = np.random.default_rng(35)
    centres = 20.0 * rng.standard_normal((8, 32))
    bank = (centres[rng.integers(0, 8, 1000)] + rng.standard_normal((1000, 32))).astype(np.float16)
    sb = StyleBank(bank, metric="L2")
    sse = []
    for niter in (0, 5):
        sb.build_index(8, niter=niter)
        cent, list_of = sb.index_export()
        sse.append(ref.sse(bank, cent, list_of))
    print(f"sum of squared distances: niter 0 {sse[0]:.6g}, niter 5 {sse[1]:.6g}")
    assert sse[1] <= sse[0]
    sb.close()


def test_append_compact_and_a_forgotten_assign():
    from astts import _lib, _lib_knn, _lib_knn_ivf
    from astts.knn import StyleBank

    bank, q, _ = case("b200")
    q = q[:9]
    sb = StyleBank(bank[:600], metric="COSINE")
    sb.build_index(8, niter=3)
    cent, _ = sb.index_export()
    assert sb.append(bank[600:]) == 600
    assert sb.index_info()["n_indexed"] == 1000
    c1, list_of = sb.index_export()
    assert np.array_equal(c1, cent)                         # the centroids do not move
    whole = StyleBank(bank, metric="COSINE")
    whole.build_index(8, niter=0, centroids=cent)
    _, list_of_whole = whole.index_export()
    assert np.array_equal(list_of, list_of_whole)
    for nprobe, k in ((2, 10), (8, 40)):
        got, exp = sb.search_ivf(q, k, nprobe, return_f64=True), whole.search_ivf(q, k, nprobe, return_f64=True)
        assert all(np.array_equal(_bits(g), _bits(e)) for g, e in zip(got, exp))
        check(sb, cent, list_of, bank, q, k, nprobe, "COSINE", oracle_scores("b200", "COSINE")[:9])
    whole.close()
    # delete, then compact: a fresh bank of the survivors with the same centroids
    dead = np.random.default_rng(36).permutation(1000)[:120]
    sb.delete_rows(dead)
    check(sb, cent, list_of, bank, q, 10, 2, "COSINE", oracle_scores("b200", "COSINE")[:9], dead=dead)
    old_to_new = sb.compact()
    keep = np.flatnonzero(old_to_new >= 0)
    assert sb.n == 880 and sb.index_info()["n_indexed"] == 880
    fresh = StyleBank(bank[keep], metric="COSINE")
    fresh.build_index(8, niter=0, centroids=cent)
    c2, list_of2 = sb.index_export()
    assert np.array_equal(c2, cent) and np.array_equal(list_of2, fresh.index_export()[1]) and np.array_equal(list_of2, list_of[keep])
    for nprobe, k in ((2, 10), (8, 40)):
        got, exp = sb.search_ivf(q, k, nprobe, return_f64=True), fresh.search_ivf(q, k, nprobe, return_f64=True)
        assert all(np.array_equal(_bits(g), _bits(e)) for g, e in zip(got, exp))
    fresh.close()
    # an append at the C level, the assign forgotten: the search refuses, the bank stays usable, the assign repairs it
    rows = torch.from_numpy(np.ascontiguousarray(bank[:5])).to(sb.device)
    _lib.check(_lib_knn.load().astts_knn_append(sb._h, rows.data_ptr(), 5, _lib.DTYPE_F16, _lib.stream_ptr(), None))
    sb._refresh()
    assert sb.n == 885
    with pytest.raises(_lib.AsttsError, match="astts_knn_ivf_assign") as e:
        sb.search_ivf(q, 3, 2)
    assert e.value.code == _lib.ERR_INVALID
    idx, _ = sb.search(q, 3)
    assert np.array_equal(idx, oknn.knn_search(np.concatenate([bank[keep], bank[:5]]), q, 3)[0])
    _lib.check(_lib_knn_ivf.load().astts_knn_ivf_assign(sb._ivf, sb._h, _lib.stream_ptr()))
    c3, list_of3 = sb.index_export()
    assert list_of3.shape == (885,) and np.array_equal(list_of3[:880], list_of2)
    check(sb, c3, list_of3, np.concatenate([bank[keep], bank[:5]]), q, 3, 2, "COSINE")
    for bad in ({"k": 0}, {"k": 1025}, {"nprobe": 0}):
        with pytest.raises(ValueError):
            sb.search_ivf(q, **{"k": 3, "nprobe": 2, **bad})
    sb.drop_index()
    assert sb.index_info() is None
    with pytest.raises(RuntimeError):
        sb.search_ivf(q, 3, 2)
    sb.close()


# ------------------------------------------------------------------------------------------ the client, end to end
NAME = "embeddings_biographies_collection"


def test_milvus_client_end_to_end(golden_dir, real_bank):
    from astts.compat.pymilvus import MilvusClient
    from astts.milvus_filter import row_mask

    db = os.path.join(golden_dir, "milvus_demo.db")
    rng = np.random.default_rng(2)
    q = (real_bank[[29, 3, 77]].astype(np.float32) + 0.5 * rng.standard_normal((3, 6144))).astype(np.float32)
    request = dict(data=q.tolist(), limit=3, output_fields=["file_id"], anns_field="vector", param={"nprobe": 10})
    # without the keyword, and with it off: what the call returns today -- the exact search, nprobe ignored
    plain_client = MilvusClient(db, persist=False)
    plain = plain_client.search(NAME, **request)
    assert [[h["row"] for h in hits] for hits in plain] == oknn.knn_search(real_bank, q, 3)[0].tolist()
    off = MilvusClient(db, persist=False, use_index=False)
    off.create_index(NAME, "vector", {"index_type": "IVF_FLAT", "params": {"nlist": 128}})
    assert off.search(NAME, **request) == plain and off._get(NAME).bank().index_info() is None
    filt = "id >= 3"
    assert off.search(NAME, filter=filt, **request) == plain_client.search(NAME, filter=filt, **request)
    off.close()
    # with it: the recorded AUTOINDEX is brute force, an IVF_FLAT request builds the index
    client = MilvusClient(db, persist=False, use_index=True)
    assert client.search(NAME, **request) == plain and client._get(NAME).bank().index_info() is None
    client.create_index(NAME, "vector", {"index_type": "IVF_FLAT", "metric_type": "COSINE", "params": {"nlist": 128}})
    coll = client._get(NAME)
    bank = coll.bank()
    assert bank.index_info()["nlist"] == 128 and bank.index_info()["n_indexed"] == 130
    cent, list_of = bank.index_export()
    mask = np.asarray(row_mask(filt, coll.pk_field, coll.pks, coll.metas)) != 0
    assert 0 < mask.sum() < 130
    for nprobe, param in ((10, {"nprobe": 10}), (8, None), (4, {"metric_type": "COSINE", "params": {"nprobe": 4}})):
        allowed = ref.membership(list_of, ref.probes(cent, q, nprobe, "COSINE"))
        for f, m in ((None, allowed), (filt, allowed & mask)):
            hits = client.search(NAME, data=q.tolist(), limit=3, output_fields=["file_id"], param=param, filter=f)
            eidx, esc = bank.search(q, 3, row_mask=m)
            assert np.array_equal(eidx, oknn.knn_search(real_bank, q, 3, row_mask=m)[0])
            assert [[(h["row"], h["distance"]) for h in hs] for hs in hits] == \
                [[(int(i), float(s)) for i, s in zip(eidx[qi], esc[qi]) if i >= 0] for qi in range(3)]
            assert all("file_id" in h["entity"] for hs in hits for h in hs)
    # grouped and ranged searches stay on the brute-force path
    grouped = client.search(NAME, data=q.tolist(), limit=3, group_by_field="id", param={"nprobe": 1})
    assert grouped == plain_client.search(NAME, data=q.tolist(), limit=3, group_by_field="id")
    # insert / delete / compact keep the index in step
    client.insert(NAME, [{"id": 900, "vector": q[0].tolist(), "file_id": "new"}])
    assert bank.index_info()["n_indexed"] == 131
    hits = client.search(NAME, data=[q[0].tolist()], limit=1, output_fields=["file_id"], param={"nprobe": 1})
    assert hits[0][0]["row"] == 130 and hits[0][0]["entity"]["file_id"] == "new"       # a row's own list is its closest: probed first
    client.delete(NAME, ids=[900])
    assert client.search(NAME, data=[q[0].tolist()], limit=1, param={"nprobe": 128})[0][0]["row"] == plain[0][0]["row"]
    assert client.compact(NAME) == 1 and bank.index_info()["n_indexed"] == 130
    assert [[h["row"] for h in hs] for hs in client.search(NAME, data=q.tolist(), limit=3, param={"nprobe": 128})] == \
        [[h["row"] for h in hs] for hs in plain]
    client.create_index(NAME, "vector", {"index_type": "FLAT"})
    assert bank.index_info() is None and client.search(NAME, **request) == plain
    client.close()
    plain_client.close()


def test_search_embeddings_cli_with_use_index(golden_dir, real_bank, tmp_path, capsys):
    from astts.cli import search_embeddings as drv

    qf = tmp_path / "q.json"
    qf.write_text(json.dumps(real_bank[29].astype(np.float32).tolist()))
    db = os.path.join(golden_dir, "milvus_demo.db")
    plain = drv.main(drv.build_parser().parse_args(["--query_embedding", str(qf), "--db_path", db]))
    capsys.readouterr()
    res = drv.main(drv.build_parser().parse_args(["--query_embedding", str(qf), "--db_path", db, "--use_index", "--nlist", "128", "--nprobe",
                                                  "128"]))
    out = capsys.readouterr().out
    assert res == plain                                    # every list probed: the exact answer
    lines = out.splitlines()
    assert lines[0] == f"Connected to Milvus at '{db}'." and lines[1] == f"Loaded query embedding from '{qf}'."
    assert "Top 3 results for Query 1:" in lines and lines[-1] == "-" * 50
    assert [ln for ln in lines if ln.startswith("File ID: ")] == \
        [f"File ID: {h['entity']['file_id']}, Distance: {h['distance']}, Text: {h['entity']['text']}" for h in res[0]]
    one = drv.main(drv.build_parser().parse_args(["--query_embedding", str(qf), "--db_path", db, "--use_index", "--nprobe", "1"]))
    capsys.readouterr()
    assert one[0][0]["row"] == 29 and one[0][0] == plain[0][0]      # the query is row 29: its own list is probed first


def test_client_index_over_a_bank_that_empties_and_refills(tmp_path):
    """An index needs a live row: a request that arrives while every row is deleted is built by the first search after an insert."""
    from astts.compat.pymilvus import MilvusClient

    rng = np.random.default_rng(37)
    vec = rng.standard_normal((7, 4)).astype(np.float32)
    client = MilvusClient(str(tmp_path / "ivf.db"), persist=False, use_index=True)
    client.create_collection("c", dimension=4, metric_type="L2")
    client.insert("c", [{"id": i, "vector": vec[i].tolist()} for i in range(5)])
    client.create_index("c", "vector", {"index_type": "IVF_FLAT", "params": {"nlist": 2}})
    coll = client._get("c")
    assert coll._bank is None
    hits = client.search("c", data=[vec[0].tolist()], limit=2, param={"nprobe": 2})
    assert [h["row"] for h in hits[0]] == oknn.knn_search(vec[:5], vec[:1], 2, oknn.METRIC_L2)[0][0].tolist()
    assert coll.bank().index_info()["nlist"] == 2
    client.delete("c", ids=list(range(5)))
    client.create_index("c", "vector", {"index_type": "IVF_FLAT", "params": {"nlist": 3}})      # no live row: nothing to train on yet
    assert client.search("c", data=[vec[0].tolist()], limit=2, param={"nprobe": 2}) == [[]]
    client.insert("c", [{"id": 5 + i, "vector": vec[5 + i].tolist()} for i in range(2)])
    hits = client.search("c", data=[vec[6].tolist()], limit=2, param={"nprobe": 3})
    assert [h["row"] for h in hits[0]] == [6, 5] and hits[0][0]["distance"] == 0.0
    assert coll.bank().index_info() == {"index_type": "IVF_FLAT", "nlist": 2, "n_indexed": 7, "max_list_len": coll.bank().index_info()["max_list_len"]}
    client.close()
