"""CPU tests: the C-ABI library loads and exports every symbol include/astts.h declares (no compute
calls without a GPU), the ctypes signatures and struct mirrors agree with that header, and the host-side
logic (Milvus-Lite reader, MilvusClient shim surface)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    syms = set()
    inc = os.path.join(ROOT, "include")
    for fn in os.listdir(inc):
        if fn.endswith(".h"):
            text = open(os.path.join(inc, fn)).read()
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            syms |= set(re.findall(r"\b(astts_[a-z0-9_]+)\s*\(", text))
    return sorted(syms)


# ABI 6 folded these forms into the base name, which took the general form's signature: base name -> suffixes that are gone
FOLDED_IN_ABI_6 = {"astts_knn_search": ("_f64", "_masked"), "astts_op_gemm": ("_ex", "_lens"), "astts_op_gemm_fused": ("_ws",),
                   "astts_op_layernorm": ("_ex", "_relu"), "astts_op_groupnorm": ("_ex",), "astts_op_interp_linear": ("_ex",),
                   "astts_op_attn_relpos": ("_ex",), "astts_op_attn_mha": ("_ex",), "astts_op_stft16": ("_lens",),
                   "astts_op_istft16": ("_lens",), "astts_op_conv1d_snake": ("_lens",), "astts_op_tfm_attn_fused": ("_pf",),
                   "astts_op_tfm_ffn_fused": ("_pf",), "astts_op_resnet_conv": ("_pf",), "astts_lm_decode": ("_range",)}


def test_library_exports_every_declared_symbol():
    from astts import _lib

    assert os.path.exists(_lib.LIB_PATH), "libastts.so not built: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    assert "astts_knn_search" in syms and len(syms) >= 8
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"declared in include/*.h but not exported: {missing}"
    # the ctypes signatures are parsed from the header: no prototype may escape the parser
    assert set(_lib.declared_symbols()) == set(syms)
    assert len(syms) == 89
    removed = [base + suffix for base, suffixes in FOLDED_IN_ABI_6.items() for suffix in suffixes]
    assert len(removed) == 18 and set(FOLDED_IN_ABI_6) <= set(syms)
    for name in removed:
        assert name not in syms and not hasattr(lib, name), name
    lib2 = _lib.load()
    assert lib2.astts_abi_version() == 6


def test_prototype_parser_on_literals():
    from ctypes import c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_void_p

    from astts._lib import parse_prototypes

    text = """
    /* a comment with a call in it: astts_not_a_prototype(int32_t x); */
    #define ASTTS_SOMETHING 3
    typedef void* astts_stream_t;
    typedef struct { int32_t d, heads; const float *g_w, *g_b; } astts_cfg_t;
    int astts_abi_version(void);
    const char* astts_last_error_string(void);
    size_t astts_ws_bytes(const astts_cfg_t* h, int64_t rows, int32_t k);
    int astts_read(int32_t kind, double* ms_sum,
                   int64_t* launches,
                   float scale, astts_stream_t stream);
    int astts_prefetch(const void* const* pf_ptrs, const uint32_t* pf_bytes, uint32_t n_pf, float eps, double tol);
    """
    assert parse_prototypes(text) == {
        "astts_abi_version": (c_int32, []),
        "astts_last_error_string": (c_char_p, []),
        "astts_ws_bytes": (c_size_t, [c_void_p, c_int64, c_int32]),
        "astts_read": (c_int32, [c_int32, c_void_p, c_void_p, c_float, c_void_p]),
        "astts_prefetch": (c_int32, [c_void_p, c_void_p, c_uint32, c_float, c_double]),
    }


@pytest.mark.parametrize("proto", ["int astts_f(unsigned x);", "int astts_f(int32_t a, long b);", "bool astts_f(void);",
                                   "int astts_f(astts_cfg_t by_value);"])
def test_prototype_parser_has_no_silent_defaults(proto):
    from astts._lib import parse_prototypes

    with pytest.raises(ValueError, match="astts_f"):
        parse_prototypes(proto)


def _header_structs():
    """typedef name -> [(field, kind)] of every ``typedef struct { ... } name;`` of the header; kind is "pointer", "int32_t", "float"
    or the name of a nested struct."""
    text = open(os.path.join(ROOT, "include", "astts.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *rest = decl.split(",")
            *type_words, first_name = first.replace("*", " * ").split()
            base = [w for w in type_words if w not in ("const", "*")]
            assert len(base) == 1, decl
            for item in [("*" if "*" in type_words else "") + first_name] + rest:
                item = item.replace(" ", "")
                fields.append((item.lstrip("*"), "pointer" if item.startswith("*") else base[0]))
        out[name] = fields
    return out


def test_ctypes_structs_mirror_the_header():
    from astts import ops

    mirrors = {"astts_lm_config_t": ops.LmConfig, "astts_lm_globals_t": ops.LmGlobals, "astts_lm_layer_t": ops.LmLayer,
               "astts_weight_t": ops.Weight, "astts_flow_resnet_t": ops.FlowResnet, "astts_flow_tfm_t": ops.FlowTfm,
               "astts_flow_block_t": ops.FlowBlock, "astts_flow_config_t": ops.FlowConfig}
    structs = _header_structs()
    assert set(structs) == set(mirrors)            # every struct of the header has a mirror, and the other way round
    in_ops = {v for v in vars(ops).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    assert in_ops == set(mirrors.values())
    by_class = {cls: name for name, cls in mirrors.items()}

    def kind(t):
        if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
            return "pointer"
        return {ctypes.c_int32: "int32_t", ctypes.c_float: "float"}.get(t) or by_class[t]

    for name, cls in mirrors.items():
        assert [(f, kind(t)) for f, t in cls._fields_] == structs[name], name


def test_product_path_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from astts.knn import StyleBank

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StyleBank(np.zeros((4, 64), np.float16))


def test_milvus_lite_reader_on_shipped_db(golden_dir, real_bank):
    from astts.milvus_lite import MilvusLiteFile

    f = MilvusLiteFile(os.path.join(golden_dir, "milvus_demo.db"))
    assert sorted(f.collections()) == ["demo_collection", "embeddings_biographies_collection"]
    info = f.info("embeddings_biographies_collection")
    assert info.dim == 6144 and info.metric_type == "COSINE" and info.pk_field == "id"
    assert info.index_params["index_type"] == "AUTOINDEX"
    assert [x.name for x in info.fields][:3] == ["id", "vector", "$meta"]
    v, pks, metas = f.load("embeddings_biographies_collection")
    assert v.dtype == np.float32 and np.array_equal(v, real_bank.astype(np.float32))
    assert pks[0] == 1 and len(pks) == 130
    assert metas[0] == {"file_id": "tonight1_0h2m4dot86s_0h2m7dot13s", "text": "What are you talking about?!"}
    assert f.info("demo_collection").dim == 768
    v2, _, _ = f.load("demo_collection")
    assert v2.shape == (0, 768)
    with pytest.raises(KeyError):
        f.info("nope")
    f.close()


def test_milvus_client_surface_cpu(golden_dir, tmp_path):
    import shutil

    from astts.compat.pymilvus import MilvusClient, MilvusException

    db = str(tmp_path / "milvus_demo.db")        # writes go through to the file: work on a copy
    shutil.copy(os.path.join(golden_dir, "milvus_demo.db"), db)
    c = MilvusClient(db)
    assert c.has_collection(collection_name="embeddings_biographies_collection")
    assert not c.has_collection(collection_name="missing")
    info = c.get_collection_info("embeddings_biographies_collection")
    assert info["num_entities"] == 130 and info["fields"][1]["params"]["dim"] == 6144
    # argument validation happens before any GPU work
    with pytest.raises(MilvusException):
        c.search("missing", data=[[0.0] * 6144], limit=1)
    with pytest.raises(MilvusException):
        c.search("embeddings_biographies_collection", data=[[0.0] * 10], limit=1)
    with pytest.raises(MilvusException):
        c.search("embeddings_biographies_collection", data=[[0.0] * 6144], limit=1, metric_type="L2")
    with pytest.raises(MilvusException):
        c.search("embeddings_biographies_collection", data=[[0.0] * 6144], limit=1, anns_field="emb")
    assert c.search("demo_collection", data=[[0.0] * 768], limit=3) == [[]]  # empty collection
    # bank-construction calls of RAG.py:49-57,541-544
    c.create_collection(collection_name="t", dimension=8)
    r = c.insert(collection_name="t", data=[{"id": 1, "vector": [1.0] * 8, "file_id": "a", "text": "x"}])
    assert r["insert_count"] == 1
    with pytest.raises(MilvusException):
        c.insert(collection_name="t", data=[{"id": 2, "vector": [1.0] * 7}])
    c.drop_collection("t")
    assert not c.has_collection("t")
    c.close()


def test_milvus_lite_writer_reproduces_shipped_blobs(golden_dir):
    """Re-encoding the schema, index and all 130 row blobs of the shipped DB gives the same BYTES."""
    import sqlite3

    from astts import milvus_lite as ml

    con = sqlite3.connect(f"file:{os.path.join(golden_dir, 'milvus_demo.db')}?mode=ro&immutable=1", uri=True)
    con.text_factory = bytes
    n_meta = 0
    for name, mt, blob, sf in con.execute("select collection_name, meta_type, blob_field, string_field from collection_meta"):
        name = name.decode()
        if mt == b"schema":
            _, fields = ml._parse_schema(blob)
            dim = int([f for f in fields if f.data_type == ml.DT_FLOAT_VECTOR][0].params["dim"])
            assert ml.encode_schema(name, dim) == blob and sf == b"id"
        else:
            p = ml._parse_index(blob)
            assert ml.encode_index(int(p["dim"]), p["metric_type"], index_id=ml._first(blob, 2)) == blob and sf == b"vector"
        n_meta += 1
    assert n_meta == 4
    n = 0
    for mid, blob in con.execute('select milvus_id, data from "embeddings_biographies_collection" order by id'):
        r = ml.parse_row(blob)
        assert ml.encode_row(r["id"], r["vector"], r["$meta"], r["RowID"], r["Timestamp"]) == blob
        assert mid.decode() == str(r["id"])
        n += 1
    assert n == 130
    con.close()


def test_milvus_client_persists_bank_like_rag_py(tmp_path, real_bank, golden_dir):
    """RAG.py:49-57,541-544: create_collection + insert into a fresh file; a new client sees the same bank."""
    from astts.compat.pymilvus import MilvusClient
    from astts.milvus_lite import MilvusLiteFile

    meta = json.load(open(os.path.join(golden_dir, "style_bank_meta.json")))
    db = str(tmp_path / "fresh.db")
    c = MilvusClient(db)
    assert not c.has_collection(collection_name="bank")
    c.create_collection(collection_name="bank", dimension=6144)
    c.create_collection(collection_name="scratch", dimension=4, metric_type="IP")
    data = [{"id": i + 1, "vector": real_bank[i].astype(np.float32).tolist(), **meta["rows"][i]} for i in range(20)]
    assert c.insert(collection_name="bank", data=data[:12])["insert_count"] == 12
    assert c.insert(collection_name="bank", data=data[12:])["ids"] == list(range(13, 21))
    c.insert(collection_name="scratch", data={"id": 7, "vector": [1, 2, 3, 4], "tag": "a/b \u00e9"})
    c.drop_collection("scratch")
    c.close()
    f = MilvusLiteFile(db)
    assert f.collections() == ["bank"]
    info = f.info("bank")
    assert info.dim == 6144 and info.metric_type == "COSINE" and info.pk_field == "id"
    v, pks, metas = f.load("bank")
    assert np.array_equal(v, real_bank[:20].astype(np.float32)) and list(pks) == list(range(1, 21))
    assert metas == meta["rows"][:20]
    f.close()
    c2 = MilvusClient(db)
    assert c2.get_collection_info("bank")["num_entities"] == 20
    c2.insert(collection_name="bank", data=[{"id": 21, "vector": real_bank[20].astype(np.float32).tolist(), "text": "x"}])
    c2.close()
    assert MilvusClient(db, persist=False).get_collection_info("bank")["num_entities"] == 21


def test_compat_install_aliases():
    import sys

    from astts import compat

    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "pymilvus" or k.startswith("cosyvoice")}
    try:
        compat.install()
        from pymilvus import MilvusClient  # noqa: F401  (milvus/search_embeddings.py:3)
        from cosyvoice.cli.cosyvoice import CosyVoice  # noqa: F401  (tts_with_rag.py:1)
        from cosyvoice.utils.file_utils import load_wav  # noqa: F401  (tts_with_rag.py:2)
    finally:
        for k in list(sys.modules):
            if k == "pymilvus" or k.startswith("cosyvoice"):
                sys.modules.pop(k)
        sys.modules.update(saved)


def test_milvus_client_explicit_schema_variant(tmp_path):
    """milvus/insert_embeddings.py:52-79,519: FieldSchema / CollectionSchema / DataType, create_collection(schema=),
    create_index(...), auto-generated primary keys, VARCHAR fields returned through output_fields."""
    from astts.compat import pymilvus as pm

    db = str(tmp_path / "explicit.db")
    client = pm.MilvusClient(db)
    fields = [pm.FieldSchema(name="id", dtype=pm.DataType.INT64, is_primary=True, auto_id=True),
              pm.FieldSchema(name="file_id", dtype=pm.DataType.VARCHAR, max_length=500, description="File identifier"),
              pm.FieldSchema(name="vector", dtype=pm.DataType.FLOAT_VECTOR, dim=16, description="Combined embedding vector"),
              pm.FieldSchema(name="text", dtype=pm.DataType.VARCHAR, max_length=1000, description="Conversation text")]
    schema = pm.CollectionSchema(fields=fields, description="Embeddings and biographies collection", metric_type="COSINE")
    client.create_collection(collection_name="c", schema=schema)
    client.create_index(collection_name="c", field_name="vector", index_params={"index_type": "IVF_FLAT", "params": {"nlist": 128}})
    rng = np.random.default_rng(0)
    rows = [{"file_id": f"f{i}", "vector": rng.standard_normal(16).astype(np.float32).tolist(), "text": f"t{i}"} for i in range(5)]
    r = client.insert(collection_name="c", data=rows)
    assert r["insert_count"] == 5 and r["ids"] == [1, 2, 3, 4, 5]            # auto_id
    info = client.describe_collection("c")
    assert info["num_entities"] == 5 and info["fields"][1]["params"]["dim"] == 16 and info["metric_type"] == "COSINE"
    client.close()
    c2 = pm.MilvusClient(db)                                               # persisted: metadata comes back from the file
    c = c2._get("c")
    assert c.pks == [1, 2, 3, 4, 5] and c.metas[2] == {"file_id": "f2", "text": "t2"}
    with pytest.raises(pm.MilvusException):
        pm.CollectionSchema(fields=fields[:2])                             # no vector field


def test_lm_workspace_bytes_layout():
    """astts_lm_workspace_bytes is host arithmetic on the handle's config (no GPU): the narrow layout (<= 32 rows, shared by the v1 and
    v2 step engines) and the wide one (33 .. ASTTS_LM_MAX_ROWS), every slot rounded up to 256 bytes.  Callers hold workspaces of these
    sizes and the logits slot hands one range of steps over to the next, so the closed forms are restated here."""
    from astts import _lib, ops

    lib = _lib.load()

    def up(x):
        return (x + 255) // 256 * 256

    splitk = int(lib.astts_op_gemm_fused_workspace_bytes())
    assert int(lib.astts_lm_workspace_bytes(None, 8)) == 0
    for d, heads, ffn, layers, vocab_out in [(128, 2, 256, 2, 65), (1024, 16, 4096, 14, 4097)]:
        cfg = ops.LmConfig(d=d, heads=heads, ffn=ffn, layers=layers, vocab_out=vocab_out, speech_vocab=vocab_out - 1)
        glob = ops.LmGlobals()                   # null pointer fields: create copies the structs, the size query reads cfg only
        lay = (ops.LmLayer * layers)()
        h = ctypes.c_void_p()
        assert lib.astts_lm_create(ctypes.byref(cfg), ctypes.byref(glob), lay, ctypes.byref(h)) == 0 and h.value
        try:
            for b in (1, 3, 32, 33, 97, 256):
                if b <= 32:
                    want = 4 * up(4 * b * d) + up(4 * b * ffn) + up(4 * b * vocab_out) + 2 * up(4 * b) + up(splitk)
                else:
                    want = 3 * up(4 * b * d) + up(2 * b * d) + 2 * up(4 * b * d) + up(2 * b * ffn) + up(4 * b * vocab_out) + up(4 * b)
                assert int(lib.astts_lm_workspace_bytes(h, b)) == want, (d, b)
            for b in (0, -1, 257):
                assert int(lib.astts_lm_workspace_bytes(h, b)) == 0, (d, b)
        finally:
            lib.astts_lm_destroy(h)


# astts_flow_workspace_bytes at (b, t) and astts_flow_session_bytes at (t, n_slots, rows_max, steps_max), as built from commit 918bc54
FLOW_BYTES = {
    "tiny": ((64, 2, 2, 2, 2),
             {(1, 2): 341760, (1, 33): 727296, (1, 385): 5102592, (1, 688): 8868608,
              (8, 2): 2728448, (8, 33): 5810688, (8, 385): 40814080, (8, 688): 70942208,
              (32, 2): 10912256, (32, 33): 23241216, (32, 385): 163254784, (32, 688): 283767296},
             {(33, 1, 1, 1): 737792, (344, 4, 32, 10): 159400448, (688, 2, 16, 32): 151854592}),
    "full": ((256, 8, 2, 12, 2),
             {(1, 2): 1755904, (1, 33): 3046144, (1, 385): 17694208, (1, 688): 30302976,
              (8, 2): 14041600, (8, 33): 24361472, (8, 385): 141547008, (8, 688): 242417152,
              (32, 2): 56164864, (32, 33): 97444352, (32, 385): 566186496, (32, 688): 969667072},
             {(33, 1, 1, 1): 3098624, (344, 4, 32, 10): 577782272, (688, 2, 16, 32): 537796096}),
}


@pytest.mark.parametrize("name", list(FLOW_BYTES))
def test_flow_workspace_and_session_bytes_layout(name):
    """astts_flow_workspace_bytes and astts_flow_session_bytes are host arithmetic on the handle's config and block counts (no GPU;
    astts_flow_create with null weight pointers copies structs only).  Callers allocate by these figures and the engine carves its
    buffers in the same walk, so a change of any slot's size or order shows here: the values are recorded from commit 918bc54."""
    from astts import _lib_session, ops

    lib = _lib_session.load()
    (ch, heads, n_down, n_mid, n_up), solve_bytes, session_bytes = FLOW_BYTES[name]
    cfg = ops.FlowConfig(mel=80, channels=ch, heads=heads, groups=8, time_in=320, time_dim=4 * ch, n_down=n_down, n_mid=n_mid, n_up=n_up)

    def blocks(kinds):
        arr = (ops.FlowBlock * len(kinds))()
        for blk, kind in zip(arr, kinds):
            blk.resample_kind = kind
        return arr

    down = blocks([ops.FLOW_RESAMPLE_DOWN] * (n_down - 1) + [ops.FLOW_RESAMPLE_CONV])
    mid = blocks([ops.FLOW_RESAMPLE_NONE] * n_mid)
    up = blocks([ops.FLOW_RESAMPLE_UP] * (n_up - 1) + [ops.FLOW_RESAMPLE_CONV])
    h = ctypes.c_void_p()
    assert lib.astts_flow_create(ctypes.byref(cfg), down, mid, up, ctypes.byref(h)) == 0 and h.value
    try:
        for (b, t), want in solve_bytes.items():
            assert int(lib.astts_flow_workspace_bytes(h, b, t)) == want, (b, t)
        for args, want in session_bytes.items():
            assert int(lib.astts_flow_session_bytes(h, *args)) == want, args
        for b, t in ((0, 33), (-1, 33), (8, 0), (8, -1)):
            assert int(lib.astts_flow_workspace_bytes(h, b, t)) == 0, (b, t)
        assert int(lib.astts_flow_workspace_bytes(None, 8, 33)) == 0
        assert int(lib.astts_flow_session_bytes(None, 344, 4, 32, 10)) == 0
        assert int(lib.astts_flow_session_bytes(h, 344, 4, 32, 33)) == 0          # steps_max > 32
        assert int(lib.astts_flow_session_bytes(h, 344, 5, 32, 10)) == 0          # n_slots > 4
    finally:
        lib.astts_flow_destroy(h)
