"""GPU tests of the grouped and ranged search (include/knn/astts_knn_grouped.h, astts.knn.StyleBank.search_grouped*, the MilvusClient
keywords on top).

The bars are exact.  Ids must EQUAL the reference of tests/knn_grouped_ref.py (a full sort per query on oracle.knn.scores_f64), -1
slots included.  The fp32 score of every hit must equal, bit for bit, what the plain search returns for that row under the same query,
and the fp64 score that search's fp64 output: a round of the grouped search IS a plain search, so nothing may differ.  Range thresholds
lie halfway between two adjacent fp64 scores of the reference that are more than 1e-9 (relative) apart -- seven orders of magnitude
above the difference between the reference's and the kernels' fp64 sums -- so no row's eligibility depends on the last bits.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import knn_grouped_ref as ref
from oracle import knn as oknn

pytestmark = pytest.mark.gpu

ALL_METRICS = ["COSINE", "IP", "L2"]


# ------------------------------------------------------------------------------------------ cases (built once, never changed)
@functools.lru_cache(maxsize=None)
def small_case():
    """n = 300, d = 100 (no multiple of 64), 7 groups of which group 0 holds 60 % of the rows; 33 queries."""
    rng = np.random.default_rng(11)
    bank = rng.standard_normal((300, 100)).astype(np.float16)
    groups = np.where(rng.random(300) < 0.6, 0, rng.integers(1, 7, 300)).astype(np.int32)
    groups[:7] = np.arange(7)                                   # every group exists
    q = (bank[rng.integers(0, 300, 33)].astype(np.float32) + 0.8 * rng.standard_normal((33, 100))).astype(np.float32)
    assert abs((groups == 0).mean() - 0.6) < 0.08
    return bank, groups, q


@functools.lru_cache(maxsize=None)
def dominated_case():
    """n = 2000, d = 64: group 0 is 200 rows built as the query direction plus small noise, so it owns the top 200 of every query under
    every metric (checked here); the other 1800 rows are Gaussian, in 20 groups."""
    rng = np.random.default_rng(12)
    u = rng.standard_normal(64)
    u *= 8.0 / np.linalg.norm(u)
    bank = rng.standard_normal((2000, 64))
    own = rng.permutation(2000)[:200]
    bank[own] = u + 0.05 * rng.standard_normal((200, 64))
    bank = bank.astype(np.float16)
    groups = rng.integers(1, 21, 2000).astype(np.int32)
    groups[own] = 0
    q = (u + 0.05 * rng.standard_normal((5, 64))).astype(np.float32)
    for metric in ALL_METRICS:
        sc = scores(("dominated", metric), bank, q, metric)
        for qi in range(5):
            assert set(ref.sorted_rows(sc[qi], metric)[:200].tolist()) == set(own.tolist())
    return bank, groups, q


@functools.lru_cache(maxsize=None)
def large_case():
    """n = 20 000, d = 768, 500 groups, 64 queries: the rounds' searches take a GEMM scan."""
    rng = np.random.default_rng(13)
    bank = rng.standard_normal((20000, 768)).astype(np.float16)
    groups = rng.integers(0, 500, 20000).astype(np.int32)
    q = (bank[rng.integers(0, 20000, 64)].astype(np.float32) + 1.5 * rng.standard_normal((64, 768))).astype(np.float32)
    return bank, groups, q


_SCORES = {}


def scores(key, bank, q, metric):
    """the reference's fp64 scores of a case, computed once"""
    if key not in _SCORES:
        _SCORES[key] = ref.metric_scores(bank, q, metric)
        _SCORES[key].setflags(write=False)
    return _SCORES[key]


_BANKS = {}


def bank_on_gpu(key, bank, metric):
    from astts.knn import StyleBank

    if (key, metric) not in _BANKS:
        _BANKS[(key, metric)] = StyleBank(bank, metric=metric)
    return _BANKS[(key, metric)]


def threshold(sc_q, metric, after):
    """Halfway between the `after`-th closest row of a query and the next one whose fp64 score is more than 1e-9 (relative) away.
    -> (threshold, rows closer than it).  The pair must exist."""
    order = ref.sorted_rows(sc_q, metric)
    s = sc_q[order]
    for j in range(after, s.size):
        if abs(s[j] - s[j - 1]) > 1e-9 * max(abs(s[j]), abs(s[j - 1])):
            return float((s[j] + s[j - 1]) / 2), j
    raise AssertionError("no pair of adjacent scores far enough apart")


# ------------------------------------------------------------------------------------------ the check
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def check(sb, bank, q, sc, limit, group_size, groups, metric, radius=None, range_filter=None, mask=None, dead=None, **kw):
    """One grouped search against the reference (ids equal) and against the plain search (scores bit for bit).  ``mask``: the caller's
    row mask; ``dead``: rows deleted from ``sb``.  -> ids."""
    dev = sb.device
    qt = torch.from_numpy(q).to(dev)
    gt = None if groups is None else torch.from_numpy(groups).to(dev)
    mt = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(dev)
    n_groups = None if groups is None else int(groups.max()) + 1
    idx, s32, s64 = (t.cpu().numpy() for t in sb.search_grouped_device(qt, limit, group_size, gt, n_groups, radius, range_filter, mt,
                                                                       return_f64=True, **kw))
    allowed = np.ones((q.shape[0], bank.shape[0]), bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0, (q.shape[0], bank.shape[0]))
    if dead is not None:
        allowed = allowed & ~np.isin(np.arange(bank.shape[0]), dead)[None, :]
    eidx, _ = ref.grouped_search(bank, q, limit, group_size, groups, metric, radius, range_filter, allowed, scores=sc)
    assert np.array_equal(idx, eidx), (metric, limit, group_size, radius, range_filter, np.argwhere(idx != eidx)[:5].tolist(), idx[idx != eidx][:5], eidx[idx != eidx][:5])
    none = np.inf if metric == "L2" else -np.inf
    assert np.all(s32[idx < 0] == none) and np.all(s64[idx < 0] == none)
    # the plain search restricted to exactly the rows that were returned gives every one of them its plain score
    slots = limit * group_size
    only = np.zeros((q.shape[0], bank.shape[0]), np.uint8)
    for qi in range(q.shape[0]):
        only[qi, idx[qi][idx[qi] >= 0]] = 1
    pidx, p32, p64 = (t.cpu().numpy() for t in sb.search_device(qt, slots, return_f64=True, row_mask=torch.from_numpy(only).to(dev)))
    for qi in range(q.shape[0]):
        a, b = np.argsort(idx[qi], kind="stable"), np.argsort(pidx[qi], kind="stable")
        assert np.array_equal(idx[qi][a], pidx[qi][b])
        assert np.array_equal(_bits(s32[qi][a]), _bits(p32[qi][b])) and np.array_equal(_bits(s64[qi][a]), _bits(p64[qi][b]))
    return idx


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("nq", [1, 8, 33])
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_small_shape(metric, nq):
    bank, groups, q = small_case()
    sb = bank_on_gpu("small", bank, metric)
    sc = scores(("small", metric), bank, q, metric)[:nq]
    for limit in (1, 3, 7, 9):                # 9: more groups than exist
        for group_size in (1, 3):
            idx = check(sb, bank, q[:nq], sc, limit, group_size, groups, metric)
            if limit == 1 and group_size == 1:
                assert sb.last_rounds == 1     # the first 32 hits hold the best row
            if limit == 9:
                assert np.all(idx[:, 7 * group_size:] == -1) and np.all(idx[:, ::group_size][:, :7] >= 0)


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_dominated_bank_runs_the_masking_path(metric):
    bank, groups, q = dominated_case()
    sb = bank_on_gpu("dominated", bank, metric)
    sc = scores(("dominated", metric), bank, q, metric)
    idx = check(sb, bank, q, sc, 3, 2, groups, metric)
    assert sb.last_rounds >= 2                 # group 0 fills from the first 32 hits; groups 2 and 3 lie behind its 200 rows
    assert np.all(groups[idx[:, 0]] == 0) and np.all(groups[idx[:, 2:]] != 0)
    check(sb, bank, q, sc, 3, 2, None, metric)      # every row its own group: group_size 2 leaves every second slot empty
    assert sb.last_rounds == 1


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_degenerate_groupings(metric):
    bank, groups, q = small_case()
    sb = bank_on_gpu("small", bank, metric)
    sc = scores(("small", metric), bank, q, metric)[:8]
    idx = check(sb, bank, q[:8], sc, 3, 4, np.zeros(300, np.int32), metric)           # one group: group_size hits, then -1
    assert np.all(idx[:, :4] >= 0) and np.all(idx[:, 4:] == -1)
    qt = torch.from_numpy(q[:8]).to(sb.device)
    for limit in (5, 40, 300):                                                       # no groups: the plain search at k = limit
        got = sb.search_grouped_device(qt, limit, return_f64=True)
        plain = sb.search_device(qt, limit, return_f64=True)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), limit
        eidx, _ = oknn.knn_search(bank, q[:8], limit, ref.METRIC_ID[metric])
        assert np.array_equal(got[0].cpu().numpy(), eidx)
    assert sb.last_rounds >= 3                                                       # 300 hits: 32 + 128 + 512


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_masks_and_tombstones(metric):
    from astts.knn import StyleBank

    bank, groups, q = small_case()
    q = q[:8]
    sb = bank_on_gpu("small", bank, metric)
    sc = scores(("small", metric), bank, q, metric)[:8]
    rng = np.random.default_rng(5)
    shared = rng.random(300) < 0.5
    per_query = rng.random((8, 300)) < 0.3
    few = np.isin(groups, [2, 5])                         # leaves two groups where three are asked for
    nothing = np.zeros(300, bool)
    for mask in (shared, per_query):
        for limit, group_size in ((3, 2), (7, 3)):
            check(sb, bank, q, sc, limit, group_size, groups, metric, mask=mask)
    idx = check(sb, bank, q, sc, 3, 2, groups, metric, mask=few)
    assert np.all(idx[:, :4] >= 0) and np.all(idx[:, 4:] == -1)
    idx = check(sb, bank, q, sc, 3, 2, groups, metric, mask=nothing)
    assert np.all(idx == -1) and sb.last_rounds == 1
    check(sb, bank, q, sc, 5, 1, None, metric, mask=per_query)
    # 25 % of the rows deleted: a bank of its own
    dead = rng.permutation(300)[:75]
    tomb = StyleBank(bank, metric=metric)
    tomb.delete_rows(dead)
    for mask in (None, shared, per_query):
        check(tomb, bank, q, sc, 3, 2, groups, metric, mask=mask, dead=dead)
        check(tomb, bank, q, sc, 7, 3, groups, metric, mask=mask, dead=dead)
    check(tomb, bank, q, sc, 40, 1, None, metric, dead=dead)
    tomb.close()


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_range(metric):
    bank, groups, q = small_case()
    sb = bank_on_gpu("small", bank, metric)
    sc_all = scores(("small", metric), bank, q, metric)
    for qi in (0, 3, 17):                                 # the thresholds are a query's own: one query per call
        sc, q1 = sc_all[qi:qi + 1], q[qi:qi + 1]
        near, n_near = threshold(sc[0], metric, 40)        # more than 32 rows are closer than `near`
        far, n_far = threshold(sc[0], metric, 90)
        assert 40 <= n_near < n_far < 300
        radius_only = {"radius": far}
        filter_only = {"range_filter": near}
        both = {"radius": far, "range_filter": near}
        for g, limit, group_size in ((None, 10, 1), (groups, 3, 2), (groups, 7, 3)):
            idx = check(sb, bank, q1, sc, limit, group_size, g, metric, **radius_only)
            assert set(idx[idx >= 0].tolist()) <= set(ref.sorted_rows(sc[0], metric)[:n_far].tolist())
            idx = check(sb, bank, q1, sc, limit, group_size, g, metric, **filter_only)
            assert sb.last_rounds >= 2                     # the first 32 hits are all closer than range_filter
            assert not set(idx[idx >= 0].tolist()) & set(ref.sorted_rows(sc[0], metric)[:n_near].tolist())
            check(sb, bank, q1, sc, limit, group_size, g, metric, **both)
        idx = check(sb, bank, q1, sc, 300, 1, None, metric, **both)      # the whole band, and nothing else
        assert (idx >= 0).sum() == n_far - n_near
    # several queries under one threshold that is clear of every score of every one of them
    sc, q8 = sc_all[:8], q[:8]
    t, _ = threshold(sc[0], metric, 60)
    assert np.abs(sc - t).min() > 1e-9 * abs(t)
    check(sb, bank, q8, sc, 3, 2, groups, metric, radius=t)
    check(sb, bank, q8, sc, 3, 2, groups, metric, range_filter=t)


def test_larger_shape_on_a_gemm_route():
    bank, groups, q = large_case()
    sb = bank_on_gpu("large", bank, "COSINE")
    assert sb.route(64, 32, masked=True)[0][1].startswith("GEMM")
    sc = scores(("large", "COSINE"), bank, q, "COSINE")
    check(sb, bank, q, sc, 3, 2, groups, "COSINE")
    assert 1 <= sb.last_rounds <= 8
    _BANKS.pop(("large", "COSINE")).close()


def test_group_table_gathered_from_global_memory_and_unaligned_codes():
    """More groups than the LDS staging of knn_group_mask takes (8192): the table is gathered from global memory.  And group codes
    at an address that is no multiple of 16 bytes: the mask kernel reads them one by one."""
    from astts.knn import StyleBank

    rng = np.random.default_rng(14)
    bank = rng.standard_normal((9000, 32)).astype(np.float16)
    groups = rng.integers(0, 9000, 9000).astype(np.int32)       # ~5700 distinct codes below 9000: most groups hold one or two rows
    groups[0] = 8999
    q = rng.standard_normal((4, 32)).astype(np.float32)
    sb = StyleBank(bank, metric="IP")
    sc = ref.metric_scores(bank, q, "IP")
    check(sb, bank, q, sc, 3, 2, groups, "IP")
    assert sb.last_rounds >= 2                                   # a group with one row never fills: its query ends by exhaustion
    sb.close()
    bank, groups, q = small_case()
    sb = bank_on_gpu("small", bank, "COSINE")
    shifted = torch.zeros(301, dtype=torch.int32, device=sb.device)
    shifted[1:] = torch.from_numpy(groups).to(sb.device)
    assert shifted[1:].data_ptr() % 16 == 4
    qt = torch.from_numpy(q[:8]).to(sb.device)
    got = sb.search_grouped_device(qt, 7, 3, shifted[1:], 7)
    want = sb.search_grouped_device(qt, 7, 3, torch.from_numpy(groups).to(sb.device), 7)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    eidx, _ = ref.grouped_search(bank, q[:8], 7, 3, groups, "COSINE", scores=scores(("small", "COSINE"), bank, q, "COSINE")[:8])
    assert np.array_equal(got[0].cpu().numpy(), eidx)


def test_max_rounds_runs_out_loudly_and_the_bank_stays_usable():
    from astts._lib import AsttsError, ERR_INVALID, ERR_UNSUPPORTED

    bank, groups, q = dominated_case()
    sb = bank_on_gpu("dominated", bank, "COSINE")
    qt, gt = torch.from_numpy(q).to(sb.device), torch.from_numpy(groups).to(sb.device)
    with pytest.raises(AsttsError, match=r"5 of 5 queries unfinished after max_rounds=1") as e:
        sb.search_grouped_device(qt, 3, 2, gt, 21, max_rounds=1)
    assert e.value.code == ERR_UNSUPPORTED and sb.last_rounds == 1
    idx, _ = sb.search(q, 5)
    assert np.array_equal(idx, oknn.knn_search(bank, q, 5)[0])
    check(sb, bank, q, scores(("dominated", "COSINE"), bank, q, "COSINE"), 3, 2, groups, "COSINE")
    # argument errors of the library
    for kw in ({"radius": 0.5, "range_filter": 0.5}, {"radius": 0.9, "range_filter": 0.1}, {"radius": float("nan")}):
        with pytest.raises(AsttsError, match="range") as e:
            sb.search_grouped_device(qt, 3, 2, gt, 21, **kw)
        assert e.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        sb.search_grouped_device(qt, 3, 2, gt, 2001)      # more groups than rows
    with pytest.raises(ValueError):
        sb.search_grouped_device(qt, 33, 32, gt, 21)      # 1056 slots


def test_milvus_client_end_to_end(golden_dir, real_bank):
    """On the parent commit this fails: the keywords are swallowed and several rows of one key come back."""
    from astts.compat.pymilvus import MilvusClient

    client = MilvusClient(os.path.join(golden_dir, "milvus_demo.db"), persist=False)
    name = "embeddings_biographies_collection"
    coll = client._get(name)
    pks = np.asarray(coll.pks)                               # the fixture's primary key restarts per speaker: 21 keys on 130 rows
    assert len(set(pks.tolist())) < 130
    codes = np.unique(pks, return_inverse=True)[1].astype(np.int32)
    rng = np.random.default_rng(2)
    q = (real_bank[[29, 3, 77]].astype(np.float32) + 0.5 * rng.standard_normal((3, 6144))).astype(np.float32)
    sc = ref.metric_scores(real_bank, q, "COSINE")
    # the plain call first: what it returns today, and it goes on returning exactly that after grouped calls
    plain = client.search(name, data=q.tolist(), limit=3, output_fields=["file_id"], anns_field="vector", param={"nprobe": 10})
    bidx, bsc = coll.bank().search(q, 3)
    assert np.array_equal(bidx, oknn.knn_search(real_bank, q, 3)[0])
    assert [[(h["row"], h["distance"]) for h in hits] for hits in plain] == [[(int(i), float(s)) for i, s in zip(bidx[qi], bsc[qi])] for qi in range(3)]
    # grouped by the key, two rows per key, the first key skipped
    hits = client.search(name, data=q.tolist(), limit=3, group_by_field="id", group_size=2, offset=1, output_fields=["file_id"])
    eidx, _ = ref.grouped_search(real_bank, q, 4, 2, codes, "COSINE", scores=sc)
    for qi in range(3):
        want = [int(i) for i in eidx[qi, 2:] if i >= 0]
        assert [h["row"] for h in hits[qi]] == want
        assert [h["entity"]["id"] for h in hits[qi]] == [int(pks[i]) for i in want] and all(h["id"] == h["entity"]["id"] for h in hits[qi])
        assert len({h["id"] for h in hits[qi]}) == 3 and all("file_id" in h["entity"] for h in hits[qi])
        assert [h["distance"] for h in hits[qi]] == [float(coll.bank().search(q[qi:qi + 1], 1, row_mask=np.arange(130) == i)[1][0, 0]) for i in want]
    # a radius, per query (the threshold is the query's own)
    for qi in range(3):
        r, n_in = threshold(sc[qi], "COSINE", 12)
        hits = client.search(name, data=[q[qi].tolist()], limit=5, group_by_field="id", search_params={"params": {"radius": r}})
        eidx, _ = ref.grouped_search(real_bank, q[qi:qi + 1], 5, 1, codes, "COSINE", radius=r, scores=sc[qi:qi + 1])
        assert [h["row"] for h in hits[0]] == [int(i) for i in eidx[0] if i >= 0]
        hits = client.search(name, data=[q[qi].tolist()], limit=40, search_params={"params": {"radius": r}})
        assert [h["row"] for h in hits[0]] == ref.sorted_rows(sc[qi], "COSINE")[:n_in].tolist()
    again = client.search(name, data=q.tolist(), limit=3, output_fields=["file_id"], anns_field="vector", param={"nprobe": 10})
    assert again == plain
    client.close()


def test_search_embeddings_cli_groups(golden_dir, real_bank, tmp_path, capsys):
    from astts.cli import search_embeddings as drv

    qf = tmp_path / "q.json"
    qf.write_text(json.dumps(real_bank[29].astype(np.float32).tolist()))
    db = os.path.join(golden_dir, "milvus_demo.db")
    res = drv.main(drv.build_parser().parse_args(["--query_embedding", str(qf), "--db_path", db, "--group_by_field", "id", "--group_size", "2",
                                                  "--top_k", "3"]))
    out = capsys.readouterr().out
    keys = [h["entity"]["id"] for h in res[0]]
    assert len(res[0]) == 6 and keys[0::2] == keys[1::2] and len(set(keys)) == 3          # three distinct keys, two rows of each
    assert out.count("Group id=") == 6 and all(f"Group id={k!r}: File ID: " in out for k in keys)
    plain = drv.main(drv.build_parser().parse_args(["--query_embedding", str(qf), "--db_path", db]))
    assert "Group" not in capsys.readouterr().out and len(plain[0]) == 3
