"""CPU tests of the IVF_FLAT index: the binding of include/knn/astts_knn_ivf.h, the numpy helpers of tests/knn_ivf_ref.py, and the host
logic of the MilvusClient shim under ``use_index`` (construction, create_index, describe_collection, nprobe parsing).  No GPU is
needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import knn_ivf_ref as ref
from oracle import knn as oknn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_parses_and_the_library_exports_every_symbol():
    from astts import _lib, _lib_knn_ivf

    sigs = _lib_knn_ivf.signatures()
    want = {"astts_knn_ivf_create", "astts_knn_ivf_destroy", "astts_knn_ivf_info", "astts_knn_ivf_export", "astts_knn_ivf_assign",
            "astts_knn_ivf_remap", "astts_knn_ivf_workspace_bytes", "astts_knn_ivf_search"}
    assert set(sigs) == want
    i32, i64, ptr, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    assert sigs["astts_knn_ivf_create"] == (i32, [ptr, i32, i32, ptr, ptr, ptr])
    assert sigs["astts_knn_ivf_destroy"] == (i32, [ptr])
    assert sigs["astts_knn_ivf_info"] == (i32, [ptr, ptr, ptr, ptr])
    assert sigs["astts_knn_ivf_export"] == (i32, [ptr, ptr, ptr])
    assert sigs["astts_knn_ivf_assign"] == (i32, [ptr, ptr, ptr])
    assert sigs["astts_knn_ivf_remap"] == (i32, [ptr, ptr, i64, ptr])
    assert sigs["astts_knn_ivf_workspace_bytes"] == (sz, [ptr, ptr, i32, i32, i32])
    assert sigs["astts_knn_ivf_search"] == (i32, [ptr, ptr, ptr, i32, i32, i32, ptr, ptr, ptr, ptr, i64, ptr, sz, ptr])
    text = open(_lib_knn_ivf.HEADER_PATH).read()
    for name, value in (("DEFAULT_NITER", _lib_knn_ivf.DEFAULT_NITER), ("SLICE_ROWS", _lib_knn_ivf.SLICE_ROWS),
                        ("MAX_NLIST", _lib_knn_ivf.MAX_NLIST)):
        assert int(re.search(rf"#define ASTTS_KNN_IVF_{name} (\d+)", text).group(1)) == value
    assert _lib_knn_ivf.DEFAULT_NITER == 20 and _lib_knn_ivf.DEFAULT_NPROBE == 8
    lib = _lib_knn_ivf.load()                      # getattr of every name: an AttributeError if libastts.so does not export it
    for name in want:
        assert getattr(lib, name).argtypes == sigs[name][1]
    # the top-level ABI is as it was: none of the new names in include/astts.h, 89 symbols, version 6
    assert not want & set(_lib.declared_symbols()) and len(_lib.declared_symbols()) == 89 and lib.astts_abi_version() == 6
    # null handles are refused without touching the GPU
    assert lib.astts_knn_ivf_workspace_bytes(None, None, 1, 1, 1) == 0
    assert lib.astts_knn_ivf_search(None, None, None, 1, 1, 1, None, None, None, None, 0, None, 0, None) == _lib.ERR_INVALID
    assert lib.astts_knn_ivf_create(None, 8, 0, None, None, ctypes.byref(ctypes.c_void_p())) == _lib.ERR_INVALID
    assert lib.astts_knn_ivf_info(None, None, None, None) == _lib.ERR_INVALID
    assert lib.astts_knn_ivf_destroy(None) == _lib.OK


def test_reference_helpers_on_a_hand_written_example():
    cent = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]], np.float32)
    bank = np.array([[1, 0], [9, 1], [0, 8], [5, 0], [11, 0], [1, 9]], np.float32)      # row 3 is as far from list 0 as from list 1
    list_of = ref.assignment(cent, bank, "L2")
    assert list_of.tolist() == [0, 1, 2, 0, 1, 2]                                      # the tie goes to the lowest list index
    q = np.array([[9.0, 0.0], [0.0, 6.0]], np.float32)
    assert ref.probes(cent, q, 1, "L2").tolist() == [[1], [2]]
    assert ref.probes(cent, q, 2, "L2").tolist() == [[1, 0], [2, 0]]
    assert ref.probes(cent, q, 5, "L2").shape == (2, 3)                                # clamped to the lists that exist
    m = ref.membership(list_of, ref.probes(cent, q, 1, "L2"))
    assert m.tolist() == [[False, True, False, False, True, False], [False, False, True, False, False, True]]
    assert ref.membership(list_of, ref.probes(cent, q, 3, "L2")).all()
    # the definition: the exact search under that mask
    idx, _ = oknn.knn_search(bank, q, 3, oknn.METRIC_L2, row_mask=m)
    assert idx.tolist() == [[1, 4, -1], [2, 5, -1]]
    assert ref.sse(bank, cent, list_of) == 1 + 2 + 4 + 25 + 1 + 2


def _client(tmp_path, **kw):
    from astts.compat.pymilvus import MilvusClient

    return MilvusClient(str(tmp_path / "ivf.db"), persist=False, **kw)


def test_client_with_use_index_behaves_as_without_it_off_the_gpu(tmp_path, golden_dir):
    """Construction, create_index and describe_collection touch no GPU: the index is built when the bank goes resident."""
    from astts.compat.pymilvus import MilvusClient, MilvusException

    seen = []
    for kw in ({}, {"use_index": True}):
        c = _client(tmp_path, **kw)
        c.create_collection("c", dimension=4)
        c.insert("c", [{"id": i, "vector": [float(i), 1.0, 0.0, 0.0], "tag": "a"} for i in range(5)])
        c.create_index("c", "vector", {"index_type": "IVF_FLAT", "metric_type": "COSINE", "params": {"nlist": 128}})
        coll = c._get("c")
        assert coll._bank is None and coll.use_index is bool(kw)
        assert coll.ivf_nlist() == 128
        seen.append((c.describe_collection("c"), dict(coll.index_params), c.get_collection_stats("c"), c.query("c", filter="id >= 3")))
        c.create_index("c", "vector", {"index_type": "IVF_FLAT", "nlist": 16})
        assert coll.ivf_nlist() == 16
        c.create_index("c", "vector", {"index_type": "FLAT"})
        assert coll.ivf_nlist() is None
        c.close()
    assert seen[0] == seen[1]
    # a collection loaded from a file: its recorded index type (AUTOINDEX in the fixture) is no IVF_FLAT request
    c = MilvusClient(os.path.join(golden_dir, "milvus_demo.db"), persist=False, use_index=True)
    coll = c._get("embeddings_biographies_collection")
    assert coll.use_index and coll.ivf_nlist() is None and coll._bank is None
    assert c.describe_collection(coll.name) == MilvusClient(os.path.join(golden_dir, "milvus_demo.db"), persist=False).describe_collection(coll.name)
    c.create_index(coll.name, "vector", {"index_type": "IVF_FLAT", "params": {"nlist": 128}})
    assert coll.ivf_nlist() == 128 and coll._bank is None
    # a bad nlist is refused by the client that would build it
    with pytest.raises(MilvusException):
        c.create_index(coll.name, "vector", {"index_type": "IVF_FLAT", "params": {"nlist": 0}})
    c.close()


def test_nprobe_parsing():
    from astts.compat.pymilvus import MilvusClient, MilvusException

    f = MilvusClient._nprobe_of
    assert f(None, None) == 8 and f({}, {}) == 8 and f({"metric_type": "COSINE"}, {"params": {}}) == 8
    assert f(None, {"nprobe": 10}) == 10                                   # the reference: param={"nprobe": 10}
    assert f(None, {"metric_type": "COSINE", "params": {"nprobe": 4}}) == 4
    assert f({"params": {"nprobe": 3}}, None) == 3
    assert f({"nprobe": 5}, None) == 5
    assert f({"params": {"nprobe": 3}}, {"params": {"nprobe": 7}}) == 7    # ``param`` wins over ``search_params``
    assert f({"params": {"radius": 0.5}}, {"nprobe": "12"}) == 12
    for bad in (0, -1, "x"):
        with pytest.raises(MilvusException):
            f(None, {"nprobe": bad})
        with pytest.raises(MilvusException):
            f({"params": {"nprobe": bad}}, None)


def test_cli_flags_default_off():
    from astts.cli import search_embeddings as drv

    a = drv.build_parser().parse_args(["--query_embedding", "q.json"])
    assert a.use_index is False and a.nlist is None and a.nprobe == 10
    a = drv.build_parser().parse_args(["--query_embedding", "q.json", "--use_index", "--nlist", "16", "--nprobe", "2"])
    assert a.use_index is True and a.nlist == 16 and a.nprobe == 2
