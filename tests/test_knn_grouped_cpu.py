"""CPU tests of the grouped and ranged search: the reference of tests/knn_grouped_ref.py against the plain oracle and a hand-written
example, the host logic of the MilvusClient shim (group codes and their cache, offset, range keywords, errors) with the StyleBank
replaced by that reference, and the binding of include/knn/astts_knn_grouped.h.  No GPU is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import knn_grouped_ref as ref
from oracle import knn as oknn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 8


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("metric", ["COSINE", "IP", "L2"])
def test_reference_without_groups_is_the_plain_oracle(metric):
    rng = np.random.default_rng(3)
    bank = rng.standard_normal((57, 24)).astype(np.float16)
    bank[40] = bank[7]                                        # a duplicate row: a tie
    q = rng.standard_normal((5, 24)).astype(np.float32)
    q[0] = bank[7]
    for k in (1, 4, 57, 60):
        idx, val = ref.grouped_search(bank, q, k, 1, np.arange(57), metric)
        eidx, eval_ = oknn.knn_search(bank, q, k, ref.METRIC_ID[metric])
        kk = eidx.shape[1]
        assert np.array_equal(idx[:, :kk], eidx) and np.array_equal(val[:, :kk], eval_)
        assert np.all(idx[:, kk:] == -1)
        idx2, val2 = ref.grouped_search(bank, q, k, 1, None, metric)        # None = every row its own group
        assert np.array_equal(idx2, idx) and np.array_equal(val2, val)
    mask = rng.random((5, 57)) < 0.4
    idx, _ = ref.grouped_search(bank, q, 6, 1, None, metric, row_mask=mask)
    eidx, _ = oknn.knn_search(bank, q, 6, ref.METRIC_ID[metric], row_mask=mask)
    assert np.array_equal(idx, eidx)


#      row:  0  1  2  3  4  5  6  7  8  9 10 11
HAND_SCORE = [9, 7, 7, 5, 8, 3, 7, 1, 6, 2, 4, 0]      # IP against q = (1, 0); rows 1 and 2 are DUPLICATES in different groups
HAND_GROUP = [0, 1, 2, 0, 0, 1, 2, 3, 3, 1, 2, 0]
# closest first: 0(g0) 4(g0) 1(g1) 2(g2) 6(g2) 8(g3) 3(g0) 10(g2) 5(g1) 9(g1) 7(g3) 11(g0)


def test_reference_on_a_hand_written_example():
    bank = np.array([[s, 0.0] for s in HAND_SCORE], np.float32)
    q = np.array([[1.0, 0.0]], np.float32)

    def ids(limit, gs, **kw):
        idx, val = ref.grouped_search(bank, q, limit, gs, np.array(HAND_GROUP), "IP", **kw)
        assert all(val[0, j] == HAND_SCORE[i] for j, i in enumerate(idx[0]) if i >= 0) and np.all(np.isneginf(val[0][idx[0] < 0]))
        return idx[0].tolist()

    assert ids(1, 1) == [0]
    assert ids(2, 1) == [0, 1]                                  # the tie of rows 1 and 2: the lower row wins, and so does its group
    assert ids(2, 2) == [0, 4, 1, 5]
    assert ids(3, 2) == [0, 4, 1, 5, 2, 6]
    assert ids(4, 2) == [0, 4, 1, 5, 2, 6, 8, 7]
    assert ids(2, 3) == [0, 4, 3, 1, 5, 9]
    assert ids(5, 3) == [0, 4, 3, 1, 5, 9, 2, 6, 10, 8, 7, -1, -1, -1, -1]      # group 3 has two rows, a fifth group does not exist
    assert ids(3, 2, radius=2.5, range_filter=8.5) == [4, 3, 1, 5, 2, 6]        # 2.5 < score <= 8.5
    assert ids(3, 2, range_filter=7.0) == [1, 5, 2, 6, 8, 7]                    # the upper bound is inclusive
    assert ids(3, 2, radius=7.0) == [0, 4, -1, -1, -1, -1]                      # the lower bound is not
    assert ids(2, 2, row_mask=np.array(HAND_SCORE) != 9) == [4, 3, 1, 5]
    l2, _ = ref.grouped_search(bank, np.array([[9.0, 0.0]], np.float32), 2, 2, np.array(HAND_GROUP), "L2", radius=9.0, range_filter=1.0)
    assert l2[0].tolist() == [4, -1, 1, -1]                                     # 1 <= squared distance < 9: rows 4 (g0), 1 (g1), 2 and 6 (g2)


# ------------------------------------------------------------------------------------------ the client's host logic
class _RefBank:
    """Stands in for astts.knn.StyleBank: the reference answers, and every call is logged."""

    def __init__(self, coll):
        self.coll, self.calls = coll, []

    def _bank(self):
        return np.stack(self.coll.vectors).astype(np.float32)

    def search(self, q, k, row_mask=None):
        self.calls.append(("search", k))
        live = np.asarray(self.coll.live)
        idx, sc = oknn.knn_search(self._bank(), q, k, ref.METRIC_ID[self.coll.metric], row_mask=live if row_mask is None else live & (row_mask != 0))
        return idx, sc.astype(np.float32)

    def search_grouped(self, q, limit, group_size=1, groups=None, n_groups=None, radius=None, range_filter=None, row_mask=None):
        self.calls.append(("search_grouped", limit, group_size, None if groups is None else n_groups, radius, range_filter))
        live = np.asarray(self.coll.live)
        if groups is not None:
            assert groups.dtype == np.int32 and groups.shape == (len(live),) and groups.min() >= 0 and groups.max() < n_groups
        idx, sc = ref.grouped_search(self._bank(), q, limit, group_size, groups, self.coll.metric, radius, range_filter,
                                     live if row_mask is None else live & (np.asarray(row_mask) != 0))
        return idx, sc.astype(np.float32)

    def append(self, rows):
        pass

    def delete_rows(self, rows):
        pass

    def compact(self):
        live = np.asarray(self.coll.live)
        return np.where(live, np.cumsum(live) - 1, -1)

    def close(self):
        pass


def _rows(ids, seed=0):
    rng = np.random.default_rng(seed)
    return [{"id": int(i), "vector": rng.standard_normal(D).astype(np.float32).tolist(), "speaker": "ABC"[int(i) % 3], "dur": float(i) / 10}
            for i in ids]


def _client(n=12, metric="COSINE"):
    from astts.compat.pymilvus import MilvusClient

    c = MilvusClient("unused.db", persist=False)
    c.create_collection("bank", dimension=D, metric_type=metric)
    c.insert("bank", _rows(range(n)))
    coll = c._get("bank")
    coll._bank = _RefBank(coll)
    return c, coll


def test_group_codes_for_int_str_bool_and_missing_values():
    from astts.compat.pymilvus import MilvusClient

    c = MilvusClient("unused.db", persist=False)
    c.create_collection("t", dimension=2)
    vals = [{"n": 1, "s": "a", "b": True}, {"n": 2, "s": "b", "b": False}, {"n": 1, "s": "a", "b": True}, {"s": "1"},
            {"n": True, "s": "b", "b": 1}, {"n": 2}, {}]
    c.insert("t", [{"id": 10 + (i % 3), "vector": [1.0, float(i)], **v} for i, v in enumerate(vals)])
    coll = c._get("t")
    codes, n = coll.group_codes("n")
    assert codes.dtype == np.int32 and codes.tolist() == [0, 1, 0, 2, 3, 1, 4] and n == 5       # True is not 1; a missing value is alone
    assert coll.group_codes("s") == coll.group_codes("s") and coll.group_codes("s")[0] is coll.group_codes("s")[0]      # cached
    assert coll.group_codes("s")[0].tolist() == [0, 1, 0, 2, 1, 3, 4] and coll.group_codes("s")[1] == 5      # "1" is not 1
    assert coll.group_codes("b")[0].tolist() == [0, 1, 0, 2, 3, 4, 5]                                # 1 is not True
    assert coll.group_codes("id")[0].tolist() == [0, 1, 2, 0, 1, 2, 0] and coll.group_codes("id")[1] == 3      # the primary key


def test_group_code_cache_is_dropped_when_the_rows_change():
    c, coll = _client()
    first = coll.group_codes("speaker")[0]
    assert first.tolist() == [0, 1, 2] * 4 and set(coll._group_codes) == {"speaker"}
    c.insert("bank", [{**_rows([12])[0], "speaker": "D"}])
    assert coll._group_codes == {} and coll.group_codes("speaker")[0].tolist() == [0, 1, 2] * 4 + [3]
    c.delete("bank", ids=[0])
    assert coll._group_codes == {}
    coll.group_codes("speaker")
    c.upsert("bank", _rows([3], seed=4))
    assert coll._group_codes == {}
    coll.group_codes("speaker")
    assert c.compact("bank") == 2
    assert coll._group_codes == {}
    codes = coll.group_codes("speaker")[0]
    assert len(codes) == len(coll.pks) == 12 and [coll.metas[i]["speaker"] for i in range(12)] == ["BCBCABCABCDA"[i] for i in range(12)]
    assert codes.tolist() == [0, 1, 0, 1, 2, 0, 1, 2, 0, 1, 3, 2]      # dense again, in the order of the first rows


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_client_grouping_offset_and_range_against_the_reference(metric):
    c, coll = _client(30, metric)
    bank = np.stack(coll.vectors)
    rng = np.random.default_rng(1)
    q = rng.standard_normal((3, D)).astype(np.float32)
    codes = np.array([i % 3 for i in range(30)])
    # grouped, with an offset: limit + offset groups are searched, the first `offset` groups sliced away
    hits = c.search("bank", q, limit=2, group_by_field="speaker", group_size=3, offset=1, output_fields=["dur"])
    assert coll._bank.calls[-1] == ("search_grouped", 3, 3, 3, None, None)
    eidx, eval_ = ref.grouped_search(bank, q, 3, 3, codes, metric)
    for qi in range(3):
        assert [h["row"] for h in hits[qi]] == eidx[qi, 3:].tolist()
        assert [h["distance"] for h in hits[qi]] == [float(np.float32(v)) for v in eval_[qi, 3:]]
        assert all(h["entity"] == {"dur": coll.metas[h["row"]]["dur"], "speaker": "ABC"[h["row"] % 3]} for h in hits[qi])      # the group field rides along
        assert len({h["entity"]["speaker"] for h in hits[qi]}) == 2
    # offset alone: the plain hits behind the first `offset`
    idx, _ = c.search_rows("bank", q, limit=4, offset=2)
    assert coll._bank.calls[-1] == ("search_grouped", 6, 1, None, None, None)
    assert np.array_equal(idx, ref.grouped_search(bank, q, 6, 1, None, metric)[0][:, 2:])
    # the range, from each of the three places it may be given in, with and without a filter
    sc = ref.metric_scores(bank, q[:1], metric)[0]
    s = np.sort(sc)
    lo, hi = float((s[10] + s[11]) / 2), float((s[20] + s[21]) / 2)
    radius, range_filter = (hi, lo) if metric == "L2" else (lo, hi)
    want = ref.grouped_search(bank, q[:1], 30, 1, None, metric, radius, range_filter)[0]
    assert (want >= 0).sum() == 10
    for kw in ({"search_params": {"params": {"radius": radius, "range_filter": range_filter}}},
               {"param": {"metric_type": metric, "params": {"radius": radius, "range_filter": range_filter}}},
               {"search_params": {"radius": radius, "range_filter": range_filter}}):
        idx, _ = c.search_rows("bank", q[:1], limit=30, **kw)
        assert coll._bank.calls[-1] == ("search_grouped", 30, 1, None, radius, range_filter) and np.array_equal(idx, want)
    idx, _ = c.search_rows("bank", q[:1], limit=5, filter='speaker != "B"', group_by_field="id", search_params={"params": {"radius": radius}})
    assert coll._bank.calls[-1] == ("search_grouped", 5, 1, 30, radius, None)
    assert np.array_equal(idx, ref.grouped_search(bank, q[:1], 5, 1, np.arange(30), metric, radius, None, codes != 1)[0])
    # strict_group_size is accepted and changes nothing
    a = c.search_rows("bank", q, limit=2, group_by_field="speaker", group_size=2, strict_group_size=False)
    b = c.search_rows("bank", q, limit=2, group_by_field="speaker", group_size=2, strict_group_size=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], ref.grouped_search(bank, q, 2, 2, codes, metric)[0])
    # deleted rows are no hits, and the codes follow the rows
    c.delete("bank", filter='speaker == "A"')
    idx, _ = c.search_rows("bank", q, limit=3, group_by_field="speaker")
    assert np.array_equal(idx, ref.grouped_search(bank, q, 3, 1, codes, metric, row_mask=codes != 0)[0]) and np.all(idx[:, 2] == -1)


def test_a_call_without_the_new_keywords_takes_the_plain_path():
    c, coll = _client()
    q = np.ones((2, D), np.float32)
    c.search("bank", q, limit=3)
    c.search("bank", q, limit=3, group_size=4, strict_group_size=True, offset=0, search_params={"metric_type": "COSINE", "params": {"nprobe": 10}})
    c.search_rows("bank", q, limit=3, filter="id > 2", param={"nprobe": 10})
    assert coll._bank.calls == [("search", 3)] * 3
    assert c.search("bank", q, limit=3)[0][0]["entity"] == {}


def test_offset_cap_and_errors():
    from astts.compat.pymilvus import MilvusException

    c, coll = _client(40)
    q = np.ones((1, D), np.float32)
    n_calls = len(coll._bank.calls)

    def refused(match, **kw):
        with pytest.raises(MilvusException, match=match) as e:
            c.search("bank", q, **kw)
        assert e.value.code == 1100

    # (limit + offset) * group_size <= 1024, after limit + offset and group_size are cut to the 40 live rows: the wording of limit > 1024
    refused("is not supported by this build: at most 1024 hits per query", limit=20, offset=20, group_size=26, group_by_field="speaker")
    refused("is not supported by this build: at most 1024 hits per query", limit=2000, group_size=30, group_by_field="id")
    assert c.search_rows("bank", q, limit=2000, group_size=25, group_by_field="id")[0].shape == (1, 1000)
    assert c.search_rows("bank", q, limit=10, offset=35)[0].shape == (1, 5) and c.search_rows("bank", q, limit=10, offset=50)[0].shape == (1, 0)
    n_calls += 3
    refused("groupBy field not found", limit=3, group_by_field="nope")
    refused("vector field", limit=3, group_by_field="vector")
    refused("must be greater than radius", limit=3, search_params={"params": {"radius": 0.5, "range_filter": 0.5}})
    refused("must be greater than radius", limit=3, param={"params": {"radius": 0.9, "range_filter": 0.1}})
    refused("invalid", limit=3, offset=-1)
    refused("invalid", limit=3, group_by_field="speaker", group_size=0)
    c2, coll2 = _client(8, "L2")
    with pytest.raises(MilvusException, match="must be less than radius") as e:
        c2.search("bank", q, limit=3, search_params={"params": {"radius": 1.0, "range_filter": 2.0}})
    assert e.value.code == 1100
    assert len(coll._bank.calls) == n_calls and coll2._bank.calls == []      # every refusal came before any search


# ------------------------------------------------------------------------------------------ the binding
def test_binding_covers_the_header_and_the_library_exports_it():
    from astts import _lib, _lib_knn_grouped

    text = open(os.path.join(ROOT, "include", "knn", "astts_knn_grouped.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(astts_[a-z0-9_]+)\s*\(", text))
    want = {"astts_knn_grouped_workspace_bytes", "astts_knn_search_grouped"}
    assert declared == want
    sigs = _lib_knn_grouped.signatures()
    assert set(sigs) == want                                                      # no prototype escapes the parser
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in want)
    i32, i64, ptr, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    assert sigs["astts_knn_grouped_workspace_bytes"] == (sz, [ptr, i32, i32, i32, i32])
    assert sigs["astts_knn_search_grouped"] == (i32, [ptr, ptr, i32, i32, i32, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, i64, ptr, sz, i32, i32,
                                                      ptr, ptr])
    assert int(re.search(r"#define ASTTS_KNN_GROUPED_DEFAULT_ROUNDS (\d+)", open(_lib_knn_grouped.HEADER_PATH).read()).group(1)) \
        == _lib_knn_grouped.DEFAULT_ROUNDS == 64
    lib = _lib_knn_grouped.load()
    # the top-level ABI is as it was: none of the new names in include/astts.h, version 6
    assert not want & set(_lib.declared_symbols()) and len(_lib.declared_symbols()) == 89 and lib.astts_abi_version() == 6
    # null handles are refused without touching the GPU
    assert lib.astts_knn_grouped_workspace_bytes(None, 1, 1, 1, 1) == 0
    assert lib.astts_knn_search_grouped(None, None, 1, 1, 1, None, 1, None, None, None, None, None, None, 0, None, 0, 0, 0, None, None) == _lib.ERR_INVALID
