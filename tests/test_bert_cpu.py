"""The host side of the BERT-family encoder track without a GPU (DESIGN.md section 2 "BERT-family encoders"): config.json and
sentence-transformers parsing with their refusals, the checkpoint loader's key mapping, the restatement of tests/bert_ref.py against the
committed transformers fixture, the length-sorted batching, and the ``--embed_model_path`` wiring of the three retrieval commands."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bert_ref as ref  # noqa: E402
from astts.llm.bert_dir import SentenceSetup, bert_shape_from_config, is_bert_dir, is_encoder_dir, sentence_setup  # noqa: E402
from astts.llm.config import BertShape  # noqa: E402
from astts.llm.peft import ConfigError  # noqa: E402
from astts.llm.weights import bert_weight_shapes, load_bert_weights, make_bert_weights, map_bert_keys  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _config_dir(tmp_path, name, **changes):
    d = tmp_path / name
    d.mkdir()
    shape = changes.pop("shape", BertShape.bert_tiny())
    conf = {**ref.config_json(shape), **changes}
    (d / "config.json").write_text(json.dumps({k: v for k, v in conf.items() if v is not ...}))
    return str(d)


# ------------------------------------------------------------------------------------------------------------ config
@pytest.mark.parametrize("name", ["bert_tiny", "xlmr_tiny", "m3e_base"])
def test_accepted_configs_parse(tmp_path, name):
    shape = getattr(BertShape, name)()
    d = _config_dir(tmp_path, name, shape=shape)
    assert is_bert_dir(d) and bert_shape_from_config(d) == shape
    assert shape.head_dim == 64 and shape.pos_offset == (2 if name == "xlmr_tiny" else 0) and shape.max_tokens == (160 if name != "m3e_base" else 512)


def test_config_defaults_and_the_roberta_family(tmp_path):
    # a RoBERTa config: pad_token_id 1 -> positions from 2; an absent pad_token_id means 1 there and 0 for BERT; absent optional keys
    rob = BertShape(model_type="roberta", vocab=300, hidden=128, layers=1, heads=2, ffn=256, max_positions=66, type_vocab=1, ln_eps=1e-5, pad_token_id=1)
    got = bert_shape_from_config(_config_dir(tmp_path, "rob", shape=rob, pad_token_id=...))
    assert got == rob and got.pos_offset == 2 and got.max_tokens == 64
    bert = bert_shape_from_config(_config_dir(tmp_path, "bert", pad_token_id=..., hidden_act=..., position_embedding_type=..., layer_norm_eps=...))
    assert bert.pad_token_id == 0 and bert.pos_offset == 0 and bert.ln_eps == 1e-12


@pytest.mark.parametrize("changes,key", [
    ({"model_type": "albert"}, "model_type"), ({"model_type": "distilbert"}, "model_type"), ({"model_type": "mpnet"}, "model_type"),
    ({"model_type": "nomic_bert"}, "model_type"), ({"model_type": "llama"}, "model_type"),
    ({"num_attention_heads": 4}, "num_attention_heads"),                       # head dimension 32 (MiniLM, bge-small)
    ({"hidden_size": 136}, "hidden_size"),                                     # not divisible
    ({"hidden_act": "gelu_new"}, "hidden_act"), ({"hidden_act": "relu"}, "hidden_act"),
    ({"position_embedding_type": "relative_key"}, "position_embedding_type"), ({"position_embedding_type": "rotary"}, "position_embedding_type"),
    ({"is_decoder": True}, "is_decoder"), ({"add_cross_attention": True}, "add_cross_attention"),
    ({"max_position_embeddings": 1}, "max_position_embeddings"),
])
def test_every_refusal_names_its_key(tmp_path, changes, key):
    with pytest.raises(ConfigError) as e:
        bert_shape_from_config(_config_dir(tmp_path, "bad", **changes))
    assert key in str(e.value)
    assert is_bert_dir(_config_dir(tmp_path, "bad2", **changes)) == (changes.get("model_type") is None)


# ------------------------------------------------------------------------------------------------------------ loader
def test_seeded_weights_are_repeatable_and_complete():
    shape = BertShape.bert_tiny()
    a, b = make_bert_weights(shape, 3), make_bert_weights(shape, 3)
    assert list(a) == list(bert_weight_shapes(shape)) and all(torch.equal(a[k], b[k]) and tuple(a[k].shape) == s for k, s in bert_weight_shapes(shape).items())
    assert not torch.equal(a["embeddings.word_embeddings.weight"], make_bert_weights(shape, 4)["embeddings.word_embeddings.weight"])


@pytest.mark.parametrize("prefix", ["", "bert.", "roberta."])
@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_loader_maps_prefixed_and_unprefixed_keys(tmp_path, prefix, fmt):
    shape = BertShape.bert_tiny() if prefix != "roberta." else BertShape.xlmr_tiny()
    sd = make_bert_weights(shape, 5)
    extra = {prefix + "pooler.dense.weight": torch.zeros(4, 4), prefix + "pooler.dense.bias": torch.zeros(4), "cls.predictions.bias": torch.zeros(3),
             "lm_head.bias": torch.zeros(3), prefix + "embeddings.position_ids": torch.arange(shape.max_positions)[None]}
    d = ref.write_dir(str(tmp_path / "ckpt"), shape, sd, prefix=prefix, extra=extra)
    if fmt == "bin":
        from safetensors.torch import load_file

        torch.save(load_file(os.path.join(d, "model.safetensors")), os.path.join(d, "pytorch_model.bin"))
        os.remove(os.path.join(d, "model.safetensors"))
    got = load_bert_weights(d)
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert set(load_bert_weights(d, shape)) == set(sd)


def test_loader_rejects_missing_unknown_and_misshaped_tensors():
    shape = BertShape.bert_tiny()
    sd = make_bert_weights(shape, 5)
    with pytest.raises(ValueError, match="lacks.*encoder.layer.1.output.dense.bias"):
        map_bert_keys({k: v for k, v in sd.items() if k != "encoder.layer.1.output.dense.bias"}, shape)
    with pytest.raises(ValueError, match="does not apply.*encoder.layer.2.output.dense.bias"):
        map_bert_keys({**sd, "bert.encoder.layer.2.output.dense.bias": torch.zeros(128)}, shape)        # a third layer
    with pytest.raises(ValueError, match="does not apply.*embeddings.extra"):
        map_bert_keys({**sd, "embeddings.extra.weight": torch.zeros(1)}, shape)
    with pytest.raises(ValueError, match="do not fit.*word_embeddings"):
        map_bert_keys({**sd, "embeddings.word_embeddings.weight": torch.zeros(shape.vocab + 1, shape.hidden)}, shape)


# ------------------------------------------------------------------------------------------------------------ sentence-transformers
def test_sentence_transformers_directory_is_read(tmp_path):
    shape = BertShape.bert_tiny()
    plain = _config_dir(tmp_path, "plain")
    assert sentence_setup(plain, shape) == SentenceSetup("mean", False, 160)                     # min(512, the table)
    assert sentence_setup(plain, BertShape.m3e_base()) == SentenceSetup("mean", False, 512)
    assert sentence_setup(plain, BertShape.xlmr_tiny()) == SentenceSetup("mean", False, 160)     # 162 positions - offset 2
    for mode, pooling in (("pooling_mode_mean_tokens", "mean"), ("pooling_mode_cls_token", "cls")):
        for normalize in (False, True):
            d = _config_dir(tmp_path, f"st_{pooling}_{normalize}")
            ref.write_sentence_files(d, mode, normalize, 64)
            assert sentence_setup(d, shape) == SentenceSetup(pooling, normalize, 64)
    d = _config_dir(tmp_path, "long")
    ref.write_sentence_files(d, "pooling_mode_mean_tokens", True, 512)
    assert sentence_setup(d, shape).max_seq_length == 160                                        # never beyond the position table


@pytest.mark.parametrize("mode", ["pooling_mode_max_tokens", "pooling_mode_mean_sqrt_len_tokens", "pooling_mode_weightedmean_tokens",
                                  "pooling_mode_lasttoken"])
def test_refused_pooling_modes_raise_by_name(tmp_path, mode):
    d = _config_dir(tmp_path, "st")
    ref.write_sentence_files(d, mode, False, 64)
    with pytest.raises(ConfigError, match=mode):
        sentence_setup(d, BertShape.bert_tiny())


def test_dense_module_and_two_poolings_are_refused(tmp_path):
    d = _config_dir(tmp_path, "dense")
    ref.write_sentence_files(d, "pooling_mode_mean_tokens", True, 64, dense=True)
    with pytest.raises(ConfigError, match="Dense"):
        sentence_setup(d, BertShape.bert_tiny())
    d = _config_dir(tmp_path, "two")
    ref.write_sentence_files(d, "pooling_mode_mean_tokens", False, 64)
    p = os.path.join(d, "1_Pooling", "config.json")
    conf = json.load(open(p))
    conf["pooling_mode_cls_token"] = True
    json.dump(conf, open(p, "w"))
    with pytest.raises(ConfigError, match="exactly one"):
        sentence_setup(d, BertShape.bert_tiny())


# ------------------------------------------------------------------------------------------------------------ reference vs fixture
@pytest.fixture(scope="module")
def fixture_file():
    return np.load(os.path.join(GOLD, "bert_tiny.npz"))


@pytest.mark.parametrize("name", ref.SHAPES)
def test_restatement_reproduces_the_transformers_fixture(fixture_file, name):
    """fp32 bert_ref against transformers' BertModel / XLMRobertaModel: to rounding (2e-6: twenty times the 1e-7 to 1e-6 the fixture
    script prints); the three wrong restatements are far outside it on the tiny shapes' hidden states, tanh-GELU included."""
    fx = fixture_file
    shape = getattr(BertShape, name)()
    sd = make_bert_weights(shape, int(fx["seed"]))
    ids, lens, types = ref.make_batch(shape, tuple(int(n) for n in fx["lens"]), int(fx["batch_seed"]))
    assert np.array_equal(ids.numpy(), fx[f"{name}.ids"]) and np.array_equal(types.numpy(), fx[f"{name}.types"])
    assert int(ids.min()) == 0 and int(ids.max()) == shape.vocab - 1 and (shape.type_vocab == 1 or int(types.max()) == 1)
    got = ref.outputs(sd, shape, ids, lens, types)
    keys = [k for k in ("hidden",) + ref.POOLED if f"{name}.{k}" in fx]
    assert keys == (["hidden"] if name in ref.TINY else []) + list(ref.POOLED)
    for k in keys:
        assert ref.rel_l2(got[k], fx[f"{name}.{k}"]) < 2e-6, k
    if name in ref.TINY:
        for kw in ({"pos_shift": 1}, {"drop_types": True}, {"tanh_gelu": True}):
            assert ref.rel_l2(ref.outputs(sd, shape, ids, lens, types, **kw)["hidden"], fx[f"{name}.hidden"]) > 1e-5, kw


def test_operator_restatements_agree_with_torch():
    g = torch.Generator().manual_seed(0)
    x, ga, be = torch.randn(7, 136, generator=g, dtype=torch.float64), torch.randn(136, generator=g, dtype=torch.float64), torch.randn(136, generator=g, dtype=torch.float64)
    y, y16 = ref.layernorm_dual(x, ga, be, 1e-12)
    assert ref.rel_l2(y, torch.nn.functional.layer_norm(x, (136,), ga, be, 1e-12)) < 1e-14 and torch.equal(y16, y.half())


# ------------------------------------------------------------------------------------------------------------ batching
def test_length_sorted_batches_restore_the_callers_order():
    from astts.llm.encoder_bert import embed_in_length_order

    rng = np.random.default_rng(0)
    seqs = [[int(v) for v in rng.integers(3, 90, size=n)] for n in (9, 2, 250, 5, 5, 31, 2, 120, 7, 64, 3)]
    calls = []

    def embed(ids, lens):                          # the stand-in encoder: (sum of the real ids, count, first id), and what it was given
        assert ids.dtype == torch.int64 and lens.dtype == torch.int32 and ids.shape[1] == int(lens.max())
        for r, n in enumerate(lens.tolist()):
            assert bool((ids[r, n:] == 1).all())                                                  # padded with pad_id
        calls.append(lens.tolist())
        return np.stack([[float(ids[r, :n].sum()), float(n), float(ids[r, 0])] for r, n in enumerate(lens.tolist())])

    out = embed_in_length_order(seqs, embed, batch=4, pad_id=1, width=3)
    assert out.dtype == np.float32 and out.shape == (11, 3)
    assert out.tolist() == [[float(sum(s)), float(len(s)), float(s[0])] for s in seqs]
    assert calls == [[2, 2, 3, 5], [5, 7, 9, 31], [64, 120, 250]]          # sorted by length: the 5-token rows never sit beside the 250-token one
    assert embed_in_length_order([], embed, 4, 1, 3).shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------ CLI wiring
class _Cfg:
    def __init__(self, hidden):
        self.hidden = hidden


class _Stub:
    """Counts what the commands ask of it: the LLM's half and the encoder's half."""

    def __init__(self, hidden, log, name):
        self.cfg, self.log, self.name = _Cfg(hidden), log, name

    def get_embedding(self, text):
        self.log.append((self.name, "get_embedding"))
        return np.full(self.cfg.hidden, 1.0, np.float32)

    def get_embeddings(self, texts):
        self.log.append((self.name, "get_embeddings"))
        return np.stack([np.full(self.cfg.hidden, float(len(t) % 7 + 1), np.float32) for t in texts])

    def generate_emotion_labels(self, texts, max_new_tokens=10):
        self.log.append((self.name, "generate_emotion_labels"))
        return ["neutral"] * len(texts)

    def generate_biographies(self, items, max_new_tokens=250, seed=0, batch=32, first_index=0):
        self.log.append((self.name, "generate_biographies"))
        return [f"{s} speaks." for _, s in items]


@pytest.fixture
def loads(monkeypatch):
    """search_milvus.load_embedder replaced by a recorder: a 'bert' path gives the 8-d encoder stub, anything else the 16-d LLM stub."""
    from astts.cli import search_milvus

    log, calls = [], []

    def fake(model_path, allow_random_init=False, seed=42, base_model_path=None, precision=None):
        calls.append((model_path, allow_random_init, seed, base_model_path, precision))
        return _Stub(8, log, "encoder") if "bert" in str(model_path) else _Stub(16, log, "llm")

    monkeypatch.setattr(search_milvus, "load_embedder", fake)
    return log, calls


def test_parsers_know_embed_model_path():
    from astts.cli import rag, search_json, search_milvus

    for parser, need in ((search_milvus.build_parser(), []), (search_json.build_parser(), ["--input_json", "x"]), (rag.build_parser(), ["--data_folder", "x"])):
        assert parser.parse_args(need).embed_model_path == ""
        a = parser.parse_args(need + ["--embed_model_path", "/m/m3e-base", "--model_path", "/m/llama"])
        assert a.embed_model_path == "/m/m3e-base" and a.model_path == "/m/llama"


def test_search_milvus_embeds_with_the_encoder_and_leaves_the_llm_out(tmp_path, loads):
    from astts.cli import search_milvus
    from astts.compat.pymilvus import MilvusClient

    log, calls = loads
    db = str(tmp_path / "b.db")
    c = MilvusClient(db)
    c.create_collection(collection_name="embeddings_biographies_collection", dimension=16)
    c.close()
    args = search_milvus.build_parser().parse_args(["--db_path", db, "--model_path", "/m/llama", "--embed_model_path", "/m/bert", "--seed", "7"])
    search_milvus.main(args)
    assert calls == [("/m/bert", False, 42, None, None)]                      # the LLM is not loaded at all
    assert [n for n, _ in log] == ["encoder", "encoder"]
    # without the flag: the one call the command always made, with its arguments
    log.clear(), calls.clear()
    with pytest.raises(SystemExit, match="embedding model's hidden size 16"):        # 32-d query against the 16-d collection
        search_milvus.main(search_milvus.build_parser().parse_args(["--db_path", db, "--model_path", "/m/llama", "--seed", "7"]))
    assert calls == [("/m/llama", False, 7, None, None)]


def _utterances(tmp_path):
    utts = [{"speaker": ["Ann", "Bob"][i % 2], "zh_text": f"line number {i} " * (i + 1), "file_id": f"utt_{i}"} for i in range(4)]
    (tmp_path / "talk.json").write_text(json.dumps(utts))
    (tmp_path / "in.jsonl").write_text("".join(json.dumps({"zh_text": u["zh_text"], "speaker": u["speaker"]}) + "\n" for u in utts))
    return utts


class _NoSearchClient:
    """A client that records the collection's dimension and answers every search with nothing (no GPU here)."""

    def __init__(self):
        self.dim = None

    def has_collection(self, collection_name):
        return False

    def create_collection(self, collection_name, dimension):
        self.dim = dimension

    def insert(self, collection_name, data):
        self.rows = data

    def search(self, **kw):
        return [[] for _ in range(len(kw["data"]))]

    def search_rows(self, collection_name, data, limit, filter=None):
        return np.zeros((len(data), 0), np.int64), np.zeros((len(data), 0), np.float32)

    def hits_from_rows(self, collection_name, idx, score, fields):
        return [[] for _ in range(len(idx))]


def test_rag_and_search_json_split_generation_and_embedding(tmp_path, loads):
    from astts.cli import rag, search_json

    log, calls = loads
    _utterances(tmp_path)
    # rag: the LLM generates, the encoder embeds, the collection is 2 x the ENCODER's width
    client = _NoSearchClient()
    args = rag.build_parser().parse_args(["--data_folder", str(tmp_path / "talk.json"), "--model_path", "/m/llama", "--embed_model_path", "/m/bert",
                                          "--search_text", ""])
    got = rag.main(args, client=client)
    assert calls == [("/m/llama", False, 42, None, None), ("/m/bert", False, 42, None, None)]
    assert client.dim == 16 and all(len(r["vector"]) == 16 for r in got["inserted"]) and len(got["inserted"]) == 4
    assert {(n, w) for n, w in log} == {("llm", "generate_biographies"), ("llm", "generate_emotion_labels"), ("encoder", "get_embeddings")}
    # search_json: the same split
    log.clear(), calls.clear()
    sargs = search_json.build_parser().parse_args(["--input_json", str(tmp_path / "in.jsonl"), "--model_path", "/m/llama", "--embed_model_path", "/m/bert"])
    assert len(search_json.main(sargs, client=_NoSearchClient())) == 4
    assert calls == [("/m/llama", False, 42, None, None), ("/m/bert", False, 42, None, None)]
    assert {(n, w) for n, w in log} == {("llm", "generate_emotion_labels"), ("encoder", "get_embeddings")}
    # without the flag: one load, and everything asked of the LLM -- the call sequence of the commands as they were
    for main, a, want in ((rag.main, rag.build_parser().parse_args(["--data_folder", str(tmp_path / "talk.json"), "--model_path", "/m/llama", "--search_text", ""]),
                           ["generate_biographies", "generate_emotion_labels", "get_embeddings"]),
                          (search_json.main, search_json.build_parser().parse_args(["--input_json", str(tmp_path / "in.jsonl"), "--model_path", "/m/llama"]),
                           ["generate_emotion_labels", "get_embeddings"])):
        log.clear(), calls.clear()
        c = _NoSearchClient()
        main(a, client=c)
        assert calls == [("/m/llama", False, 42, None, None)]
        assert [w for n, w in log if n == "llm"] == want and all(n == "llm" for n, _ in log)
        assert c.dim in (None, 32)


def test_load_embedder_sends_a_bert_directory_to_the_encoder(tmp_path, monkeypatch):
    """A directory whose config.json says bert / roberta / xlm-roberta goes to load_bert_embedder, before anything Llama-shaped is read;
    an albert directory is refused by key; the tokenizer files of an encoder directory are looked for."""
    from astts.cli import search_milvus

    seen = []
    monkeypatch.setattr(search_milvus, "load_bert_embedder", lambda p: seen.append(p) or "an encoder")
    d = _config_dir(tmp_path, "enc")
    assert search_milvus.load_embedder(d) == "an encoder" and seen == [d]
    assert {"vocab.txt", "sentencepiece.bpe.model"} <= set(search_milvus.TOKENIZER_FILES)
    monkeypatch.undo()
    # another encoder family through the PUBLIC entry point: refused as an encoder, by key, not read as a Llama
    for i, other in enumerate(("albert", "distilbert", "mpnet", "nomic_bert")):
        bad = _config_dir(tmp_path, f"other{i}", model_type=other)
        assert is_encoder_dir(bad) and not is_bert_dir(bad)
        with pytest.raises(ConfigError, match=f"model_type='{other}'.*bert, roberta, xlm-roberta"):
            search_milvus.load_embedder(bad)
    assert not is_encoder_dir(_config_dir(tmp_path, "llama", model_type="llama")) and not is_encoder_dir(str(tmp_path / "nowhere"))


def test_stand_in_tokenizer():
    from astts.llm.encoder_bert import HashBertTokenizer

    for shape, cls, sep in ((BertShape.m3e_base(), 101, 102), (BertShape.bert_tiny(), 101, 102), (BertShape.xlmr_tiny(), 0, 2),
                            (BertShape(vocab=64, hidden=64, heads=1), 1, 2)):
        tok = HashBertTokenizer(shape)
        ids = tok.encode("a few words, and a few words")
        assert ids[0] == cls and ids[-1] == sep and len(ids) == 9 and ids[1:3] == ids[5:7]
        assert all(tok.first <= i < shape.vocab for i in ids[1:-1]) and tok.encode("") == [cls, sep]
        assert tok.encode("a b", add_special_tokens=False) == tok.encode("a b")[1:-1]
    for vocab in (3, 10, 105):
        with pytest.raises(ValueError, match="vocabulary"):
            HashBertTokenizer(BertShape(vocab=vocab))
