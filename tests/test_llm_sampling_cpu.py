"""CPU side of the sampled LLM generation: the numpy statement of astts_op_sample_topk_topp (tests/llm_sampling_ref.py) against
transformers' warpers and against the committed answers, the operator's place in the ABI, and the two drivers that use it
(astts.cli.search_json --generate_biographies, astts.cli.rag) with a stub embedder and oracle/knn.py in the place of the GPU search."""
import hashlib
import json
import os

import numpy as np
import pytest

import llm_sampling_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_reference_equals_transformers_warpers(case):
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, the order generate() applies: what they keep is the reference's
    nucleus, and the softmax over what they keep is its q (1e-6).  Covers the 64-row 128 256-wide case, top_k in {1, 1024}, top_p = 1.0
    and the 1 000-entry vocabulary."""
    pytest.importorskip("transformers")
    import torch
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    name, seed, rows, vocab, ld, scales, temperature, top_k, top_p = case
    x, u = ref.case_inputs(case)
    x = x[:, :vocab]
    scores = torch.from_numpy(np.ascontiguousarray(x))
    for w in (TemperatureLogitsWarper(temperature), TopKLogitsWarper(top_k), TopPLogitsWarper(top_p)):
        scores = w(None, scores)
    probs = torch.softmax(scores.double(), -1).numpy()
    kept = np.isfinite(scores.numpy())
    _, margin, answers = ref.sample_rows(x, u, temperature, top_k, top_p)
    assert margin >= ref.MARGIN
    for r, a in enumerate(answers):
        assert sorted(np.nonzero(kept[r])[0].tolist()) == sorted(a.ids.tolist()), (name, r)
        assert np.abs(probs[r, a.ids] - a.q).max() <= 1e-6, (name, r)
        assert abs(a.q.sum() - 1.0) <= 1e-12 and a.token in a.ids


def test_committed_answers_are_the_references():
    """tests/golden/sampling_kats.npz (written by tests/golden/make_sampling_fixtures.py) holds what the reference computes today."""
    fx = np.load(os.path.join(GOLD, "sampling_kats.npz"))
    for case in ref.CASES:
        tokens, margin, rows = ref.case_answers(case)
        assert margin >= ref.MARGIN, case[0]
        assert np.array_equal(fx[case[0] + "/tokens"], tokens), case[0]
        sizes = fx[case[0] + "/sizes"]
        assert sizes.tolist() == [len(r.ids) for r in rows]
        assert np.array_equal(fx[case[0] + "/ids"], np.concatenate([r.ids for r in rows]))
        assert np.abs(fx[case[0] + "/q"].astype(np.float64) - np.concatenate([r.q for r in rows])).max() <= 1e-7      # stored as float32


def test_reference_definition_on_a_row_done_by_hand():
    """logits ln(4, 3, 2, 1) at T = 1: p = .4 .3 .2 .1; top_p .65 keeps exclusive prefixes 0, .4 (< .65) and drops .7: q = 4/7, 3/7."""
    x = np.log(np.array([1.0, 4.0, 2.0, 3.0], np.float32))
    r = ref.sample_row(x, 0.5, 1.0, 50, 0.65)
    assert r.ids.tolist() == [1, 3] and np.allclose(r.q, [4 / 7, 3 / 7], atol=1e-7) and r.token == 1
    assert ref.sample_row(x, 0.6, 1.0, 50, 0.65).token == 3
    assert ref.sample_row(x, 0.99, 1.0, 2, 1.0).ids.tolist() == [1, 3]                       # top_k cuts first
    assert ref.sample_row(np.zeros(5, np.float32), 0.5, 1.0, 2, 1.0).ids.tolist() == [0, 1]  # ties: the lower id first, exactly top_k kept
    assert ref.sample_row(x, 0.0, 0.7, 1, 0.9).token == 1
    assert abs(ref.uniform_for(x, 3, 1.0, 50, 0.65) - (4 / 7 + 1) / 2) < 1e-6


def test_operator_is_declared_exported_and_registered():
    """include/astts.h declares astts_op_sample_topk_topp, libastts.so exports it, astts.ops registers its signature and has the wrapper."""
    import ctypes
    import re

    from astts import _lib, ops

    header = open(os.path.join(ROOT, "include", "astts.h")).read()
    assert re.search(r"\bint astts_op_sample_topk_topp\(const float\* logits, int64_t ld, const float\* uniforms, int32_t\* out_tokens", header)
    assert "top_k = 0" in header and "tied with the k-th" in header                           # the two stated deviations
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "astts_op_sample_topk_topp")
    assert "astts_op_sample_topk_topp" in _lib.declared_symbols()
    assert callable(ops.sample_topk_topp)
    assert _lib.load().astts_abi_version() == 6


def test_operator_refuses_bad_arguments_before_any_launch():
    """Argument checks come before the launch, so they hold without a GPU: null pointers, temperature, top_p, top_k (0 = "off" included)."""
    import ctypes

    from astts import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    call = lambda lg=p, u=p, out=p, rows=1, vocab=4, ld=4, t=0.7, k=50, tp=0.9: lib.astts_op_sample_topk_topp(lg, ld, u, out, rows, vocab, t, k, tp, None)
    assert call(lg=None) == _lib.ERR_INVALID and call(u=None) == _lib.ERR_INVALID and call(out=None) == _lib.ERR_INVALID
    assert call(ld=3) == _lib.ERR_INVALID and call(vocab=0) == _lib.ERR_INVALID and call(rows=0) == _lib.ERR_INVALID
    assert call(t=0.0) == _lib.ERR_RANGE and call(t=-1.0) == _lib.ERR_RANGE
    assert call(tp=0.0) == _lib.ERR_RANGE and call(tp=1.5) == _lib.ERR_RANGE
    assert call(k=0) == _lib.ERR_RANGE and call(k=1025) == _lib.ERR_RANGE


# ------------------------------------------------------------------------------------------------------------ the drivers
class _StubEmbedder:
    """Stand-in for LlamaEmbedder: canned biographies, labels and fixed random vectors that are pure functions of the text."""

    class cfg:
        hidden = 32

    def __init__(self, fail=()):
        self.bio_calls, self.fail = [], set(fail)

    @staticmethod
    def _vec(text):
        h = int.from_bytes(hashlib.sha256(text.encode("utf-8")).digest()[:8], "little")
        return np.random.default_rng(h).standard_normal(32).astype(np.float32)

    def generate_biographies(self, items, max_new_tokens=250, seed=0, batch=32, first_index=0):
        self.bio_calls.append(([s for _, s in items], max_new_tokens, seed, first_index))
        if any(s in self.fail for _, s in items):
            raise RuntimeError("generation failed")
        return [f"{s} is the speaker of {len(c.splitlines())} lines ({max_new_tokens})." for c, s in items]

    def generate_emotion_labels(self, texts, max_new_tokens=10):
        return [f"label {hashlib.sha256(t.encode()).hexdigest()[:6]}" for t in texts]

    def get_embeddings(self, texts):
        return np.stack([self._vec(t) for t in texts])


class _OracleBank:
    def __init__(self, m):
        self.m = m

    def search(self, q, k):
        from oracle import knn as oknn

        idx, sc = oknn.knn_search(self.m.astype(np.float32), np.asarray(q, np.float32), k)
        return idx, sc.astype(np.float32)

    def close(self):
        pass


@pytest.fixture
def cpu_search(monkeypatch):
    from astts.compat import pymilvus as pm

    monkeypatch.setattr(pm._Collection, "bank", lambda self: _OracleBank(self.matrix()))


def _bank64(path, rows=20):
    """A 64-d bank (the stub embedder's 2 x 32) in a fresh Milvus-Lite file."""
    from astts.compat.pymilvus import MilvusClient

    rng = np.random.default_rng(1)
    c = MilvusClient(path)
    c.create_collection(collection_name="embeddings_biographies_collection", dimension=64)
    c.insert(collection_name="embeddings_biographies_collection",
             data=[{"id": i + 1, "vector": rng.standard_normal(64).astype(np.float32).tolist(), "file_id": f"f{i}", "text": f"t{i}"} for i in range(rows)])
    c.close()
    return path


def test_search_json_parser_knows_the_biography_flags():
    from astts.cli import search_json

    a = search_json.build_parser().parse_args(["--input_json", "x"])
    assert a.generate_biographies is False and a.max_new_tokens == 250 and a.biography_out == ""
    a = search_json.build_parser().parse_args(["--input_json", "x", "--generate_biographies", "--max_new_tokens", "40", "--biography_out", "b.json"])
    assert a.generate_biographies is True and a.max_new_tokens == 40 and a.biography_out == "b.json"


def test_search_json_generates_one_biography_per_speaker(tmp_path, cpu_search):
    from astts.cli import search_json

    rows = [{"zh_text": "one", "speaker": "A"}, {"zh_text": "two", "speaker": "B"}, {"zh_text": "three", "speaker": "A"},
            {"zh_text": "", "speaker": "D"}, {"zh_text": "four", "speaker": "C"}, {"zh_text": "five", "speaker": "B"}]
    inp = tmp_path / "in.jsonl"
    inp.write_text("".join(json.dumps(r) + "\n" for r in rows))
    (tmp_path / "given.json").write_text(json.dumps({"B": "B's own biography."}))
    out = tmp_path / "bios.json"
    emb = _StubEmbedder(fail={"C"})
    db = _bank64(str(tmp_path / "bank64.db"))
    args = search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db, "--generate_biographies",
                                                  "--max_new_tokens", "40", "--llm_batch", "1", "--seed", "9", "--biography_json", str(tmp_path / "given.json"),
                                                  "--biography_out", str(out)])
    res = search_json.main(args, embedder=emb)
    assert len(res) == 5 and all(r["retrieved_file_id"].startswith("f") for r in res)
    # A and C are generated (B comes from the file, D has no text), one per decode; C's decode raised: the placeholder, no second try
    assert emb.bio_calls == [(["A"], 40, 9, 0), (["C"], 40, 9, 1)]
    bios = search_json.load_biographies(str(out))
    assert bios == {"A": "A is the speaker of 2 lines (40).", "C": search_json.PLACEHOLDER_BIOGRAPHY, "B": "B's own biography."}
    assert search_json.speaker_conversations(rows) == {"A": "one\nthree", "B": "two\nfive", "C": "four"}
    # the query halves use them
    kept = [r for r in rows if r["zh_text"]]
    q, labels, failed = search_json.embed_rows(kept, emb, bios)
    assert not failed.any()
    for r, v in zip(kept, q):
        assert np.array_equal(v[32:], emb._vec(bios[r["speaker"]]))
    # and reading the written file back gives the same run without generating
    emb2 = _StubEmbedder()
    args2 = search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db, "--biography_json", str(out)])
    assert search_json.main(args2, embedder=emb2) == res and emb2.bio_calls == []


def _utterances(n=12):
    with open(os.path.join(GOLD, "iemocap_test_sentences.json")) as f:
        sents = [s for s in json.load(f)["all"] if s.strip()][:n]
    return [{"speaker": ["Ann", "Bob", "Cy"][i % 3], "zh_text": s, "file_id": f"utt_{i:03d}"} for i, s in enumerate(sents)]


def test_rag_builds_a_bank_the_other_drivers_open(tmp_path, cpu_search, capsys):
    from astts.cli import rag, search_json
    from astts.compat.pymilvus import MilvusClient

    utts = _utterances()
    (tmp_path / "a.json").write_text(json.dumps(utts[:7] + [{"speaker": "Ann", "zh_text": "no file id"}]))
    (tmp_path / "b.jsonl").write_text("".join(json.dumps(u) + "\n" for u in utts[7:]))
    db, dump = str(tmp_path / "bank.db"), str(tmp_path / "out" / "dump.json")
    args = rag.build_parser().parse_args(["--data_folder", str(tmp_path / "a.json"), str(tmp_path / "b.jsonl"), "--db_path", db, "--output_file", dump,
                                          "--max_new_tokens", "30", "--search_text", "hello there", "--top_k", "2"])
    emb = _StubEmbedder()
    got = rag.main(args, embedder=emb)
    text = capsys.readouterr().out
    assert len(got["inserted"]) == 12 and emb.bio_calls == [(["Ann", "Bob", "Cy"], 30, 42, 0)]
    # primary keys restart per speaker (RAG.py:507); rows are grouped by speaker
    assert [r["id"] for r in got["inserted"]] == [1, 2, 3, 4] * 3
    recs = json.load(open(dump))
    assert len(recs) == 12 and all(set(r) == {"file_id", "speaker", "text", "emotion", "biography", "combined_embedding_shape"} for r in recs)
    assert recs[0]["combined_embedding_shape"] == [64] and recs[0]["biography"] == "Ann is the speaker of 4 lines (30)."
    assert open(dump).read().startswith("[\n  {\n")                                               # indent=2
    # self-retrieval: every row is its own top-1
    lines = [l for l in text.splitlines() if l.startswith("Query ID: ")]
    assert len(lines) == 12
    for i, (l, ins) in enumerate(zip(lines, got["inserted"])):
        assert l.startswith(f"Query ID: {i + 1}, Retrieved ID: {ins['id']}, Distance: ") and f"File ID: {ins['file_id']}, Text: {ins['text']}" in l
        assert got["verify"][i][0]["row"] == i and abs(got["verify"][i][0]["distance"] - 1.0) < 1e-5
    assert "Top 2 results for the query 'hello there':" in text and len(got["search"][0]) == 2
    # a fresh client and search_json open the file unchanged
    c = MilvusClient(db)
    info = c.describe_collection(rag.COLLECTION)
    assert info["num_entities"] == 12 and info["fields"][1]["params"]["dim"] == 64 and info["metric_type"] == "COSINE"
    c.close()
    inp = tmp_path / "q.jsonl"
    inp.write_text("".join(json.dumps({"zh_text": r["text"], "speaker": r["speaker"]}) + "\n" for r in recs))
    np.save(tmp_path / "q.npy", np.asarray([r["vector"] for r in got["inserted"]], np.float32))
    sargs = search_json.build_parser().parse_args(["--input_json", str(inp), "--query_npy", str(tmp_path / "q.npy"), "--db_path", db])
    assert [r["retrieved_file_id"] for r in search_json.main(sargs)] == [r["file_id"] for r in recs]
    # a second build into the same file replaces the collection
    rag.main(args, embedder=_StubEmbedder())
    assert MilvusClient(db).describe_collection(rag.COLLECTION)["num_entities"] == 12


def _dist_worker(rank, world, port, work):
    import sys

    import torch

    for p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port), "ASTTS_DIST_BACKEND": "gloo"})
    torch.set_num_threads(1)
    from astts import parallel
    from astts.cli import search_json
    from astts.compat import pymilvus as pm

    pm._Collection.bank = lambda self: _OracleBank(self.matrix())
    emb = _StubEmbedder()
    args = search_json.build_parser().parse_args(["--input_json", os.path.join(work, "in.jsonl"), "--db_path", os.path.join(work, "bank64.db"),
                                                  "--generate_biographies", "--max_new_tokens", "20",
                                                  "--llm_batch", "2", "--biography_out", os.path.join(work, f"bios_w{world}.json"),
                                                  "--output_file", os.path.join(work, f"out_w{world}.jsonl")])
    assert len(search_json.main(args, embedder=emb)) == 9
    with open(os.path.join(work, f"bio_calls_w{world}_r{rank}.json"), "w") as f:
        json.dump(emb.bio_calls, f)
    parallel.shutdown()


def test_search_json_generates_on_rank_0_and_every_rank_gets_the_map(tmp_path):
    """Under the data-parallel launch (two gloo ranks started as torch.distributed.run starts them) rank 0 alone generates, for the
    speakers of ALL rows; the map reaches rank 1 (its rows' query halves use it: the JSONL equals the one-process run's), and the
    --biography_out file is the one-process run's too."""
    import socket

    import torch.multiprocessing as mp

    def port():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            return s.getsockname()[1]

    work = str(tmp_path)
    with open(os.path.join(work, "in.jsonl"), "w") as f:
        for i in range(9):
            f.write(json.dumps({"zh_text": f"line {i}", "speaker": ["A", "B", "C"][(i * i) % 3] if i < 6 else "D"}) + "\n")
    _bank64(os.path.join(work, "bank64.db"))
    mp.spawn(_dist_worker, args=(1, port(), work), nprocs=1, join=True)
    mp.spawn(_dist_worker, args=(2, port(), work), nprocs=2, join=True)
    read = lambda n: open(os.path.join(work, n), "rb").read()
    assert read("out_w1.jsonl") == read("out_w2.jsonl") and read("out_w1.jsonl").count(b"\n") == 9 and b"Error" not in read("out_w1.jsonl")
    assert read("bios_w1.json") == read("bios_w2.json") and set(json.loads(read("bios_w2.json"))) == {"A", "B", "D"}
    assert json.loads(read("bio_calls_w2_r0.json")) == json.loads(read("bio_calls_w1_r0.json")) and len(json.loads(read("bio_calls_w2_r0.json"))) == 2
    assert json.loads(read("bio_calls_w2_r1.json")) == []
