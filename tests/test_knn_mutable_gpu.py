"""GPU tests of the style bank that changes while resident (include/knn/astts_knn_mutable.h, astts.knn.StyleBank.append /
delete_rows / compact, the MilvusClient calls on top).

Two bars.  The PROJECT bars are those of tests/test_knn_gpu.py: ids bit-exact against oracle.knn.knn_search, scores within its
SCORE_ATOL = 1e-6 (times max(1, |largest score|), as there).  The STRICT bar: a bank that grew and a bank created at once from the
same rows return torch.equal ids, fp32 scores and fp64 scores.  It is derived, not measured: the per-row packing is row-independent
(the append runs the build kernels of astts_knn_create on the new rows alone), the returned scores come from the fp64 re-score, which
sums in a fixed order over dp, and the certified top-k does not depend on the route that proposed the candidates.
"""
import numpy as np
import pytest
import torch

from oracle import knn as oknn

pytestmark = pytest.mark.gpu

SCORE_ATOL = 1e-6
METRICS = {"COSINE": oknn.METRIC_COSINE, "IP": oknn.METRIC_IP, "L2": oknn.METRIC_L2}
ALL_METRICS = ["COSINE", "IP", "L2"]


def _bank130(real_bank, which):
    """130 fp16-exact rows: the committed 6144-wide bank, or Gaussian rows with d = 64 / d = 200 (padded to 256: no multiple of 64)."""
    if which == "real":
        return real_bank
    d = {"d64": 64, "d200": 200}[which]
    return np.random.default_rng(d).standard_normal((130, d)).astype(np.float16)


def _queries(bank, nq, seed=1):
    rng = np.random.default_rng(seed)
    b = np.asarray(bank, dtype=np.float32)
    return (b[rng.integers(0, b.shape[0], nq)] + 0.3 * b.std() * rng.standard_normal((nq, b.shape[1]))).astype(np.float32)


def _dev(sb, q, k, **kw):
    mask = kw.pop("mask", None)
    if mask is not None:
        mask = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(sb.device)
    return sb.search_device(torch.from_numpy(q).to(sb.device), k, return_f64=True, row_mask=mask, **kw)


def _strict(a, b, q, k, mask_a=None, mask_b=None, **kw):
    """the strict bar between two banks"""
    ra, rb = _dev(a, q, k, mask=mask_a, **kw), _dev(b, q, k, mask=mask_b, **kw)
    for name, x, y in zip(("idx", "score", "score64"), ra, rb):
        assert torch.equal(x, y), (name, k, kw, (x != y).nonzero()[:5].tolist())
    return ra


def _bars(sb, bank_np, q, k, metric, mask=None, oracle_mask=None, force_exact=False):
    """the project bars of tests/test_knn_gpu.py (_check_metric) against the oracle under oracle_mask (default: mask)"""
    idx, sc = sb.search(q, k, force_exact=force_exact, row_mask=mask)
    eidx, esc = oknn.knn_search(bank_np, q, k, METRICS[metric], row_mask=mask if oracle_mask is None else oracle_mask)
    kk = eidx.shape[1]
    assert np.array_equal(idx[:, :kk], eidx), (metric, np.argwhere(idx[:, :kk] != eidx)[:5])
    live = eidx >= 0
    scale = max(1.0, float(np.abs(esc[live]).max())) if live.any() else 1.0
    assert np.allclose(sc[:, :kk][live], esc[live], atol=SCORE_ATOL * scale, rtol=0)
    dead = ~live
    if dead.any():
        assert np.all(np.isposinf(sc[:, :kk][dead]) if metric == "L2" else np.isneginf(sc[:, :kk][dead]))
    if kk < k:
        assert np.all(idx[:, kk:] == -1)
    return idx, sc


@pytest.mark.parametrize("which", ["real", "d64", "d200"])
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_append_equals_create(real_bank, metric, which):
    """37 rows, then appends of 1, 90 and 2: the totals cross the 32-, 64- and 128-row tile edges and the capacity of 128 rows that
    astts_knn_create allocated is outgrown.  The grown bank equals the bank created from all 130 rows on the strict bar."""
    from astts.knn import StyleBank

    rows = _bank130(real_bank, which)
    sb = StyleBank(rows[:37], metric=metric)
    assert (sb.n, sb.live, sb.capacity) == (37, 37, 128)
    assert sb.append(rows[37:38]) == 37 and (sb.n, sb.capacity) == (38, 128)
    assert sb.append(rows[38:128]) == 38 and (sb.n, sb.capacity) == (128, 128)
    assert sb.append(rows[128:130].astype(np.float32)) == 128        # (an fp32 upload of exact rows: the kernel decides exactness)
    assert (sb.n, sb.live, sb.capacity) == (130, 130, 256) and sb.scan_plane_exact
    fresh = StyleBank(rows, metric=metric)
    assert (fresh.n, fresh.capacity) == (130, 256)
    q = _queries(rows, 16)
    _strict(sb, fresh, q, 5)
    _strict(sb, fresh, q, 5, force_exact=True)
    _strict(sb, fresh, q, 33)
    _bars(sb, rows, q, 5, metric)
    sb.reserve(1000)
    assert (sb.n, sb.capacity) == (130, 1024)
    sb.reserve(10)                                                   # never shrinks
    assert sb.capacity == 1024
    _strict(sb, fresh, q, 5)
    with pytest.raises(ValueError):
        sb.search(q, 3, row_mask=np.ones(37, np.uint8))              # the mask's shape follows n


@pytest.mark.parametrize("which", ["real", "d200"])
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_promotion(real_bank, metric, which):
    """An fp16-exact bank meets fp32 rows that are not: among them rows of norm ~1e-2 and ~1e-3 (elements below fp16's normal range)
    and a row with finite elements beyond 65504.  Afterwards it is the handle created from the whole fp32 matrix."""
    from astts.knn import StyleBank

    base = _bank130(real_bank, which)[:100]
    d = base.shape[1]
    rng = np.random.default_rng(17)
    new = rng.standard_normal((30, d)).astype(np.float32) * np.float32(base.astype(np.float32).std())
    new[3] *= np.float32(1e-2 / np.linalg.norm(new[3]))
    new[4] *= np.float32(1e-3 / np.linalg.norm(new[4]))
    new[5] *= np.float32(2e5 / np.abs(new[5]).max())
    assert (np.abs(new[4]) < 6.1e-5).mean() > 0.4 and np.isfinite(new[5]).all() and np.abs(new[5]).max() > 65504
    full = np.concatenate([base.astype(np.float32), new])
    sb = StyleBank(base, metric=metric)
    assert sb.scan_plane_exact
    assert sb.append(new) == 100 and sb.n == 130 and sb.capacity == 256
    assert not sb.scan_plane_exact
    fresh = StyleBank(full, metric=metric)
    assert not fresh.scan_plane_exact
    q = np.concatenate([_queries(base, 8), full[[103, 104, 105]] * np.float32(1.01), _queries(new[6:], 5)]).astype(np.float32)
    _strict(sb, fresh, q, 5)
    _strict(sb, fresh, q, 5, force_exact=True)
    _strict(sb, fresh, q, 33)
    _bars(sb, full, q, 5, metric)
    if metric == "COSINE":
        idx, _ = sb.search(q[8:11], 1)
        assert idx[:, 0].tolist() == [103, 104, 105]                 # rows of any norm are found
    # a handle that is inexact already: only the new rows are packed and rescaled
    more = rng.standard_normal((7, d)).astype(np.float32)
    assert sb.append(more) == 130
    _strict(sb, StyleBank(np.concatenate([full, more]), metric=metric), q, 5)


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_refused_appends(real_bank, metric):
    """A batch with a NaN (or an infinity) is refused with ASTTS_ERR_RANGE and changes nothing -- not n, not the capacity (the batch
    would have outgrown it), not a search.  A valid append afterwards still meets the strict bar: a dirty tail would show here."""
    from astts import _lib
    from astts.knn import StyleBank

    sb = StyleBank(real_bank[:100], metric=metric)
    q = _queries(real_bank, 16)
    before = _dev(sb, q, 5)
    for bad_value in (np.nan, np.inf):
        bad = np.tile(real_bank[100:130].astype(np.float32), (2, 1))
        bad[41, 77] = bad_value                                      # 60 rows: 100 + 60 > 128
        with pytest.raises(_lib.AsttsError) as e:
            sb.append(bad)
        assert e.value.code == _lib.ERR_RANGE
        assert (sb.n, sb.live, sb.capacity) == (100, 100, 128) and sb.scan_plane_exact
        after = _dev(sb, q, 5)
        assert all(torch.equal(x, y) for x, y in zip(before, after))
    with pytest.raises(ValueError):
        sb.append(np.zeros((2, 100), np.float32))                    # wrong width
    assert sb.append(real_bank[100:130]) == 100
    fresh = StyleBank(real_bank, metric=metric)
    _strict(sb, fresh, q, 5)
    _strict(sb, fresh, q, 33)


def _deleted_rows(sb, q, n):
    top1 = sb.search(q, 1)[0][:, 0]
    return sorted({0, 31, 32, 127, 128, n - 1} | {int(i) for i in top1})


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_tombstones(real_bank, metric):
    """Deleted rows are never hits: at tile edges (0, 31, 32, 127, 128, n - 1) and every query's current best row; alone, under a
    shared and under a per-query caller mask, through the k > 32 passes with fewer live rows than k, and with every row deleted."""
    from astts import _lib
    from astts.knn import StyleBank, route

    n = 130
    sb, plain = StyleBank(real_bank, metric=metric), StyleBank(real_bank, metric=metric)
    q = _queries(real_bank, 16)
    assert sb.route(16, 5) == route(n, 6144, 16, 5, masked=False)    # a handle that never deleted: its search is the unmasked one
    dead = _deleted_rows(sb, q, n)
    sb.delete_rows(dead)
    sb.delete_rows(dead[:3])                                         # twice: not an error, not counted twice
    assert (sb.n, sb.live, sb.capacity) == (n, n - len(dead), 256)
    with pytest.raises(_lib.AsttsError) as e:
        sb.delete_rows([5, n])                                       # out of range: refused, and row 5 stays
    assert e.value.code == _lib.ERR_INVALID and sb.live == n - len(dead)
    assert sb.route(16, 5) == route(n, 6144, 16, 5, masked=True)
    live = np.ones(n, np.uint8)
    live[dead] = 0
    idx, _ = _bars(sb, real_bank, q, 5, metric, oracle_mask=live)
    assert not np.isin(idx, dead).any()
    _bars(sb, real_bank, q, 5, metric, oracle_mask=live, force_exact=True)
    _strict(sb, plain, q, 5, mask_b=live)
    rng = np.random.default_rng(9)
    shared = (rng.random(n) < 0.6).astype(np.uint8)
    per_q = (rng.random((16, n)) < 0.4).astype(np.uint8)
    for m in (shared, per_q):
        _bars(sb, real_bank, q, 5, metric, mask=m, oracle_mask=m & live)
        _strict(sb, plain, q, 5, mask_a=m, mask_b=m & live)
        _strict(sb, plain, q, 40, mask_a=m, mask_b=m & live)         # k > 32 under both masks
    # k = 70 with fewer than 70 live rows: the multi-pass path; the tail is idx -1 and score -inf (+inf for L2)
    more = [i for i in range(40, 110) if live[i]]
    sb.delete_rows(more)
    live[more] = 0
    assert sb.live == int(live.sum()) < 70
    idx, sc = _bars(sb, real_bank, q, 70, metric, oracle_mask=live)
    assert np.all(idx[:, sb.live:] == -1) and np.all(idx[:, :sb.live] >= 0)
    assert np.all(np.isposinf(sc[:, sb.live:]) if metric == "L2" else np.isneginf(sc[:, sb.live:]))
    _strict(sb, plain, q, 70, mask_b=live)
    sb.delete_rows(np.arange(n))
    assert sb.live == 0
    for k in (5, 70):
        idx, sc = sb.search(q, k)
        assert np.all(idx == -1) and np.all(np.isposinf(sc) if metric == "L2" else np.isneginf(sc))


@pytest.mark.parametrize("which", ["real", "d200"])
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_compact(real_bank, metric, which):
    """compact() after those deletes: the map old -> new, the project bars on the survivors, ids and scores that map onto the masked
    search before it; then an append, against a fresh bank of (survivors + new rows) -- stale rows in the vacated tail would show."""
    from astts.knn import StyleBank, route

    rows = _bank130(real_bank, which)
    n = 130
    sb = StyleBank(rows[:120], metric=metric)
    sb.append(rows[120:])
    q = _queries(rows, 16)
    dead = _deleted_rows(sb, q, n)
    sb.delete_rows(dead)
    keep = np.asarray([i for i in range(n) if i not in dead])
    pre = _dev(sb, q, 5)
    old_to_new = sb.compact()
    want = np.full(n, -1, np.int64)
    want[keep] = np.arange(len(keep))
    assert old_to_new.dtype == np.int64 and np.array_equal(old_to_new, want)
    assert (sb.n, sb.live, sb.capacity) == (len(keep), len(keep), 256)
    assert sb.route(16, 5) == route(len(keep), rows.shape[1], 16, 5, masked=False)      # no tombstones left: the unmasked search
    survivors = rows[keep]
    _bars(sb, survivors, q, 5, metric)
    post = _dev(sb, q, 5)
    assert torch.equal(torch.from_numpy(old_to_new).to(pre[0].device)[pre[0]], post[0])
    assert torch.equal(pre[1], post[1]) and torch.equal(pre[2], post[2])
    fresh = StyleBank(survivors, metric=metric)
    _strict(sb, fresh, q, 5)
    _strict(sb, fresh, q, 33)
    new = np.random.default_rng(4).standard_normal((len(dead) - 2, rows.shape[1])).astype(np.float16)   # fewer than were removed
    assert sb.append(new) == len(keep)
    both = np.concatenate([survivors, new])
    fresh = StyleBank(both, metric=metric)
    _strict(sb, fresh, q, 5)
    _strict(sb, fresh, q, 5, force_exact=True)
    _bars(sb, both, q, 5, metric)
    assert np.array_equal(sb.compact(), np.arange(sb.n))             # nothing deleted: the identity


def test_compact_keeps_a_promoted_bank_promoted(real_bank):
    """A promoted bank whose inexact rows are all deleted stays inexact through compact (no demotion): against a fresh, fp16-exact
    bank of the survivors the project bars hold, not the strict one."""
    from astts.knn import StyleBank

    sb = StyleBank(real_bank[:100])
    new = np.random.default_rng(2).standard_normal((10, 6144)).astype(np.float32)
    sb.append(new)
    sb.append(real_bank[100:])
    assert not sb.scan_plane_exact and sb.n == 140
    sb.delete_rows(np.arange(100, 110))
    old_to_new = sb.compact()
    assert np.array_equal(old_to_new[:100], np.arange(100)) and np.all(old_to_new[100:110] == -1) and old_to_new[139] == 129
    assert sb.n == 130 and not sb.scan_plane_exact
    fresh = StyleBank(real_bank)
    assert fresh.scan_plane_exact
    q = _queries(real_bank, 16)
    idx, sc = _bars(sb, real_bank, q, 5, "COSINE")
    fidx, fsc = fresh.search(q, 5)
    assert np.array_equal(idx, fidx) and np.allclose(sc, fsc, atol=SCORE_ATOL, rtol=0)


@pytest.mark.parametrize("nq,scan", [(64, ("REGISTER", "SELECT_MERGE")), (128, ("GEMM_BLOCKS", "BLOCKS"))])
def test_gemm_scan_route_on_a_grown_bank(nq, scan):
    """8192 x 64 rows created, 130 appended (the score row now has two selection segments).  With 128 queries the group takes the
    GEMM scan with block maxima, which reads the row-major plane in whole tiles behind the bank; 64 queries stay below the GEMM
    threshold of this shape (a 64-row query tile x 131 bank tiles < 256 tiles) and take the register scan with per-segment selection.
    Both: project bars against the oracle, strict bar against a fresh bank; again after deleting 200 rows (masked: GEMM + streaming
    selection for the large group)."""
    from astts.knn import StyleBank

    rng = np.random.default_rng(64)
    rows = rng.standard_normal((8192 + 130, 64)).astype(np.float16)
    sb = StyleBank(rows[:8192])
    assert sb.capacity == 8192 and sb.append(rows[8192:]) == 8192 and (sb.n, sb.capacity) == (8322, 16384)
    assert sb.route(nq, 5) == [(nq,) + scan]
    q = _queries(rows, nq)
    q[:8] = _queries(rows[8192:], 8)                                 # some queries next to the appended rows
    fresh = StyleBank(rows)
    _bars(sb, rows, q, 5, "COSINE")
    _strict(sb, fresh, q, 5)
    must = np.unique(np.concatenate([np.arange(8180, 8230), sb.search(q, 1)[0][:, 0]]))      # across the segment edge, every top-1
    dead = np.concatenate([must, np.setdiff1d(rng.permutation(8322)[:400], must)[:200 - len(must)]])
    assert len(dead) == len(np.unique(dead)) == 200
    sb.delete_rows(dead)
    assert sb.live == 8322 - 200
    if nq == 128:
        assert sb.route(nq, 5) == [(nq, "GEMM", "STREAM")]
    live = np.ones(8322, np.uint8)
    live[dead] = 0
    idx, _ = _bars(sb, rows, q, 5, "COSINE", oracle_mask=live)
    assert not np.isin(idx, dead).any()
    _strict(sb, fresh, q, 5, mask_b=live)


def _client_rows(vecs, first_id=0):
    return [{"id": first_id + i, "vector": v.tolist(), "speaker": "ABC"[(first_id + i) % 3], "text": f"utt {first_id + i}"}
            for i, v in enumerate(vecs)]


def _same_as_fresh_client(c, q, limit=5):
    """the search of the maintained collection == the search of a fresh client populated with its live rows (ids by primary key,
    scores on the project bar)"""
    from astts.compat.pymilvus import MilvusClient

    coll = c._get("bank")
    live = coll.live_rows()
    f = MilvusClient("unused.db", persist=False)
    f.create_collection("bank", dimension=coll.dim, metric_type=coll.metric)
    f.insert("bank", [dict(coll.metas[i], id=coll.pks[i], vector=coll.vectors[i]) for i in live])
    got = c.search("bank", data=q.tolist(), limit=limit, output_fields=["speaker"])
    want = f.search("bank", data=q.tolist(), limit=limit, output_fields=["speaker"])
    f.close()
    assert len(got) == len(want) == len(q)
    for g, w in zip(got, want):
        assert [h["id"] for h in g] == [h["id"] for h in w] and len(g) == min(limit, len(live))
        assert [h["entity"] for h in g] == [h["entity"] for h in w]
        assert [live[h["row"]] for h in w] == [h["row"] for h in g]
        assert np.allclose([h["distance"] for h in g], [h["distance"] for h in w], atol=SCORE_ATOL, rtol=0)
    return got


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_client_end_to_end(tmp_path, metric):
    """insert, search, insert, search on ONE resident bank; delete by filter, upsert, query, get, compact -- after every step the
    search equals that of a fresh client holding the live rows; the file behind the client shows them after reopening."""
    from astts.compat.pymilvus import MilvusClient

    rng = np.random.default_rng(33)
    d = 64
    vecs = rng.standard_normal((200, d)).astype(np.float32)
    q = (vecs[[3, 50, 120, 160]] + 0.2 * rng.standard_normal((4, d))).astype(np.float32)
    path = str(tmp_path / "bank.db")
    c = MilvusClient(path)
    c.create_collection("bank", dimension=d, metric_type=metric)
    c.insert("bank", _client_rows(vecs[:100]))
    _same_as_fresh_client(c, q)
    bank = c._get("bank")._bank
    assert bank is not None and bank.n == 100
    c.insert("bank", _client_rows(vecs[100:150], 100))
    assert c._get("bank")._bank is bank and bank.n == 150 and bank.capacity == 256      # appended in place, the bank grew
    got = _same_as_fresh_client(c, q)
    assert got[2][0]["id"] == 120
    # delete by filter
    n_a = sum(1 for i in range(150) if i % 3 == 0)
    assert c.delete("bank", filter='speaker == "A"') == {"delete_count": n_a}
    assert c.get_collection_stats("bank") == {"row_count": 150 - n_a} and c.describe_collection("bank")["num_entities"] == 150 - n_a
    assert bank.n == 150 and bank.live == 150 - n_a
    got = _same_as_fresh_client(c, q)
    assert all(h["entity"]["speaker"] != "A" for hits in got for h in hits) and got[2][0]["id"] != 120
    # upsert: two existing keys (one of them deleted) and a new one
    up = [{"id": 50, "vector": vecs[150].tolist(), "speaker": "B", "text": "new 50"},
          {"id": 120, "vector": vecs[120].tolist(), "speaker": "B", "text": "back"},
          {"id": 999, "vector": vecs[151].tolist(), "speaker": "C", "text": "fresh"}]
    assert c.upsert("bank", up)["upsert_count"] == 3
    assert c._get("bank")._bank is bank and bank.n == 153 and bank.live == 150 - n_a + 2
    got = _same_as_fresh_client(c, q)
    assert got[2][0]["id"] == 120 and got[2][0]["row"] == 151 and got[2][0]["entity"] == {"speaker": "B"}
    assert c.query("bank", filter="id == 50", output_fields=["*"]) == [{"id": 50, "speaker": "B", "text": "new 50"}]
    assert c.get("bank", [120, 0, 999], output_fields=["text"]) == [{"id": 120, "text": "back"}, {"id": 999, "text": "fresh"}]
    # delete by ids, compact: rows are renumbered, the search is the same
    assert c.delete("bank", ids=[1, 2, 3])["delete_count"] == 2      # 3 was an "A"
    before = _same_as_fresh_client(c, q, limit=40)
    assert c.compact("bank") == 153 - bank.live and bank.n == bank.live == c.get_collection_stats("bank")["row_count"]
    after = _same_as_fresh_client(c, q, limit=40)
    assert [[(h["id"], h["distance"]) for h in hits] for hits in before] == [[(h["id"], h["distance"]) for h in hits] for hits in after]
    c.insert("bank", _client_rows(vecs[160:170], 2000))
    _same_as_fresh_client(c, q)
    live_ids = [c._get("bank").pks[i] for i in c._get("bank").live_rows()]
    c.close()
    r = MilvusClient(path)
    assert r._get("bank").pks == live_ids and r.get_collection_stats("bank") == {"row_count": len(live_ids)}
    r.close()
