"""CPU tests of the collection-maintenance calls of the MilvusClient shim (delete / upsert / query / get / stats / compact) and of
the binding of include/knn/astts_knn_mutable.h.  No search is issued, so no bank is built and no GPU is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 8


def _rows(ids, seed=0):
    rng = np.random.default_rng(seed)
    return [{"id": int(i), "vector": rng.standard_normal(D).astype(np.float32).tolist(), "speaker": "ABC"[int(i) % 3], "dur": float(i) / 10}
            for i in ids]


def _client(tmp_path=None, n=12):
    from astts.compat.pymilvus import MilvusClient

    c = MilvusClient(str(tmp_path / "m.db") if tmp_path else "unused.db", persist=tmp_path is not None)
    c.create_collection("bank", dimension=D)
    c.insert("bank", _rows(range(n)))
    return c


def _live_ids(c):
    coll = c._get("bank")
    return [coll.pks[i] for i in coll.live_rows()]


def test_delete_by_ids_and_by_filter():
    from astts.compat.pymilvus import MilvusException

    c = _client()
    assert c.delete("bank", ids=[1, 2, 100]) == {"delete_count": 2}
    assert c.delete("bank", ids=2) == {"delete_count": 0}                         # gone already
    assert c.delete("bank", filter='speaker == "A" and id > 0') == {"delete_count": 3}      # 3, 6, 9
    assert _live_ids(c) == [0, 4, 5, 7, 8, 10, 11]
    assert c.get_collection_stats("bank") == {"row_count": 7} and c.describe_collection("bank")["num_entities"] == 7
    coll = c._get("bank")
    assert len(coll.pks) == len(coll.vectors) == len(coll.metas) == len(coll.live) == 12      # rows keep their index until compact
    assert coll._bank is None                                                     # nothing here built a bank
    for kw in ({}, {"ids": [4], "filter": "id == 4"}):
        with pytest.raises(MilvusException):
            c.delete("bank", **kw)                                                # exactly one of ids / filter
    with pytest.raises(MilvusException):
        c.delete("bank", filter="id === 4")
    with pytest.raises(MilvusException):
        c.delete("nope", ids=[1])
    assert _live_ids(c) == [0, 4, 5, 7, 8, 10, 11]


def test_upsert_replaces_every_row_with_the_key():
    c = _client(n=6)
    c.insert("bank", _rows([2], seed=5))                                          # keys need not be unique: two live rows with id 2
    new = _rows([2, 40, 40], seed=9)
    new[2]["speaker"] = "last"
    assert c.upsert("bank", new)["upsert_count"] == 3
    coll = c._get("bank")
    assert len(coll.pks) == 10 and coll.live == [True, True, False, True, True, True, False, True, False, True]
    assert _live_ids(c) == [0, 1, 3, 4, 5, 2, 40] and c.get_collection_stats("bank") == {"row_count": 7}
    assert c.get("bank", 40, output_fields=["speaker"]) == [{"id": 40, "speaker": "last"}]      # of two rows of one request the last
    got = c.get("bank", [2], output_fields=["vector"])
    assert len(got) == 1 and np.allclose(got[0]["vector"], new[0]["vector"])


def test_query_and_get_rules():
    from astts.compat.pymilvus import MilvusException

    c = _client()
    c.delete("bank", ids=[4])
    assert c.query("bank", filter="id >= 3 and id < 6") == [{"id": 3}, {"id": 5}]       # the primary key always, live rows only
    assert c.query("bank", filter="id == 3", output_fields=["*"]) == [{"id": 3, "speaker": "A", "dur": 0.3}]
    assert c.query("bank", filter="id == 3", output_fields=["dur", "absent"]) == [{"id": 3, "dur": 0.3}]
    one = c.query("bank", filter="id == 3", output_fields=["*"])[0]
    assert "vector" not in one                                                    # the vector only when it is named
    vec = c.query("bank", filter="id == 3", output_fields=["vector", "speaker"])[0]
    assert set(vec) == {"id", "vector", "speaker"} and isinstance(vec["vector"], list) and len(vec["vector"]) == D
    assert np.allclose(vec["vector"], c._get("bank").vectors[3])
    with pytest.raises(MilvusException):
        c.query("bank")                                                           # an empty filter needs a limit
    with pytest.raises(MilvusException):
        c.query("bank", filter="", limit=0)
    assert [r["id"] for r in c.query("bank", limit=5)] == [0, 1, 2, 3, 5]
    assert [r["id"] for r in c.query("bank", filter='speaker == "C"', limit=2)] == [2, 5]
    assert c.query("bank", ids=[5, 4, 0]) == [{"id": 0}, {"id": 5}]
    assert c.get("bank", ids=[7, 4], output_fields=["speaker"]) == [{"id": 7, "speaker": "B"}]
    assert c.get("bank", ids=4) == []


def test_compact_renumbers_the_host_rows():
    c = _client()
    assert c.compact("bank") == 0
    c.delete("bank", ids=[0, 5, 11])
    assert c.compact("bank") == 3
    coll = c._get("bank")
    assert coll.pks == [1, 2, 3, 4, 6, 7, 8, 9, 10] and coll.live == [True] * 9 and coll.n_live == 9
    assert [m["speaker"] for m in coll.metas] == ["ABC"[i % 3] for i in coll.pks] and len(coll.vectors) == 9
    c.delete("bank", filter="id >= 0")
    assert c.get_collection_stats("bank") == {"row_count": 0}
    assert c.compact("bank") == 9 and coll.pks == [] and coll.live == []
    assert c.insert("bank", _rows([77]))["ids"] == [77] and _live_ids(c) == [77]


def test_persistence_after_delete_upsert_and_compact(tmp_path):
    """The Milvus-Lite file shows the live rows, in order, after each of the three (the collection is rewritten through the writer)."""
    from astts.compat.pymilvus import MilvusClient

    def reopened():
        r = MilvusClient(str(tmp_path / "m.db"))
        coll = r._get("bank")
        out = (list(coll.pks), [m["speaker"] for m in coll.metas], np.stack(coll.vectors) if coll.vectors else None)
        assert r.get_collection_stats("bank") == {"row_count": len(coll.pks)} and coll.metric == "COSINE" and coll.dim == D
        r.close()
        return out

    def live(c):
        coll = c._get("bank")
        rows = coll.live_rows()
        return [coll.pks[i] for i in rows], [coll.metas[i]["speaker"] for i in rows], np.stack([coll.vectors[i] for i in rows])

    def same(a, b):
        return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])

    c = _client(tmp_path)
    c.delete("bank", filter='speaker == "B"')
    assert same(reopened(), live(c)) and reopened()[0] == [0, 2, 3, 5, 6, 8, 9, 11]
    up = _rows([3, 50], seed=3)
    c.upsert("bank", up)
    assert same(reopened(), live(c)) and reopened()[0] == [0, 2, 5, 6, 8, 9, 11, 3, 50]
    assert np.allclose(reopened()[2][-2], up[0]["vector"])
    c.delete("bank", ids=[0])
    assert c.compact("bank") == 6
    c.insert("bank", _rows([60], seed=4))
    assert same(reopened(), live(c)) and reopened()[0] == [2, 5, 6, 8, 9, 11, 3, 50, 60]
    c.close()
    assert reopened()[0] == [2, 5, 6, 8, 9, 11, 3, 50, 60]


def test_binding_covers_the_header_and_the_library_exports_it():
    from astts import _lib, _lib_knn

    text = open(os.path.join(ROOT, "include", "knn", "astts_knn_mutable.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(astts_[a-z0-9_]+)\s*\(", text))
    want = {"astts_knn_reserve", "astts_knn_append", "astts_knn_set_deleted", "astts_knn_compact", "astts_knn_stats"}
    assert declared == want
    sigs = _lib_knn.signatures()
    assert set(sigs) == want                                                      # no prototype escapes the parser
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in want)
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert sigs["astts_knn_reserve"] == (i32, [ptr, i64, ptr])
    assert sigs["astts_knn_append"] == (i32, [ptr, ptr, i64, i32, ptr, ptr])
    assert sigs["astts_knn_set_deleted"] == (i32, [ptr, ptr, i64, ptr])
    assert sigs["astts_knn_compact"] == (i32, [ptr, ptr, ptr, ptr])
    assert sigs["astts_knn_stats"] == (i32, [ptr, ptr, ptr, ptr])
    lib = _lib_knn.load()
    assert lib.astts_knn_append.argtypes == sigs["astts_knn_append"][1]
    # the top-level ABI is as it was: none of the new names in include/astts.h, version 6
    assert not want & set(_lib.declared_symbols()) and len(_lib.declared_symbols()) == 89 and lib.astts_abi_version() == 6
    # null handles are refused without touching the GPU
    assert lib.astts_knn_stats(None, None, None, None) == _lib.ERR_INVALID
    assert lib.astts_knn_append(None, None, 0, _lib.DTYPE_F32, None, None) == _lib.ERR_INVALID
