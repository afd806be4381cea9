"""The BERT-family sentence encoder on the GPU (DESIGN.md section 2 "BERT-family encoders"): astts.llm.encoder_bert against
tests/golden/bert_tiny.npz (transformers' BertModel / XLMRobertaModel, fp32, CPU, on seeded weights) and the commands that use it.

Bounds.  Relative L2 per tensor; every bound is 4 x the error of the fp16-rounded CPU restatement (tests/bert_ref.py, ``h16=True``)
against the transformers fixture, as tests/golden/make_bert_fixtures.py prints it; the emulated value stands in EMULATED.  The hidden-state
bounds (2.9e-4) lie three orders of magnitude below what the fixture script prints for positions shifted by one (4.7e-1) and for the
token-type table dropped (3.2e-1 to 3.5e-1); tanh-GELU in place of erf (2.9e-5 to 3.0e-5 on the tiny shapes, 2.9e-4 at BERT-base depth)
lies inside them: the fixture does not tell the two GELUs apart, and that figure is reported only."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bert_ref as ref  # noqa: E402
from astts.llm.bert_dir import SentenceSetup  # noqa: E402
from astts.llm.config import BertShape  # noqa: E402
from astts.llm.weights import make_bert_weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# emulated (fp16-rounded restatement vs the transformers fixture); every bound = 4 x
EMULATED = {
    "bert_tiny": {"hidden": 7.272e-5, "mean": 8.718e-5, "cls": 8.169e-5, "mean_norm": 8.179e-5, "cls_norm": 8.186e-5},
    "xlmr_tiny": {"hidden": 7.251e-5, "mean": 8.032e-5, "cls": 7.817e-5, "mean_norm": 7.456e-5, "cls_norm": 7.813e-5},
    "m3e_base": {"mean": 8.699e-4, "cls": 9.566e-4, "mean_norm": 8.676e-4, "cls_norm": 9.558e-4},
}
BOUND = {name: {k: 4 * v for k, v in d.items()} for name, d in EMULATED.items()}
SETUPS = {"mean": ("mean", False), "cls": ("cls", False), "mean_norm": ("mean", True), "cls_norm": ("cls", True)}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "bert_tiny.npz"))


_EMBEDDERS = {}


def _embedder(name, fx):
    """One embedder per shape for the whole module (weights regenerate from the fixture's seed); tests set ``.setup`` as they need it."""
    from astts.llm.encoder_bert import BertEmbedder

    if name not in _EMBEDDERS:
        shape = getattr(BertShape, name)()
        _EMBEDDERS[name] = BertEmbedder(make_bert_weights(shape, int(fx["seed"])), shape, DEV)
    emb = _EMBEDDERS[name]
    emb.setup = SentenceSetup("mean", False, min(512, emb.cfg.max_tokens))
    return emb


def _batch(name, fx):
    shape = getattr(BertShape, name)()
    ids, lens, types = ref.make_batch(shape, tuple(int(n) for n in fx["lens"]), int(fx["batch_seed"]))
    assert np.array_equal(ids.numpy(), fx[f"{name}.ids"])
    return ids, lens, types


def _pooled(emb, ids, lens, types) -> dict:
    out = {}
    for k, (pooling, normalize) in SETUPS.items():
        emb.setup = SentenceSetup(pooling, normalize, emb.setup.max_seq_length)
        out[k] = emb.embed_ids(ids, lens, types).cpu()
    return out


@pytest.mark.parametrize("name", ref.SHAPES)
def test_encoder_against_the_transformers_fixture(fx, name):
    emb = _embedder(name, fx)
    ids, lens, types = _batch(name, fx)
    got = _pooled(emb, ids, lens, types)
    if name in ref.TINY:
        h = emb.hidden(ids, lens, types).cpu()
        assert h.shape == (len(lens), int(lens.max()), emb.cfg.hidden) and bool(torch.isfinite(h).all())
        got["hidden"] = torch.cat([h[i, :int(n)] for i, n in enumerate(lens)])
    for k, bound in BOUND[name].items():
        err = ref.rel_l2(got[k], fx[f"{name}.{k}"])
        print(f"{name} {k}: GPU vs transformers rel L2 {err:.3e} (emulated {EMULATED[name][k]:.3e}, bound {bound:.3e})")
        assert err < bound, (name, k, err, bound)
    cos = torch.nn.functional.cosine_similarity(got["mean"].double(), torch.from_numpy(fx[f"{name}.mean"]).double(), dim=-1)
    print(f"{name}: smallest cosine of a mean-pooled embedding to the transformers fixture {float(cos.min()):.7f}")
    assert float(torch.linalg.vector_norm(got["mean_norm"], dim=-1).sub(1).abs().max()) < 1e-5


@pytest.mark.parametrize("name", ref.TINY)
def test_a_text_alone_and_inside_the_padded_batch_agree(fx, name):
    emb = _embedder(name, fx)
    ids, lens, types = _batch(name, fx)
    together = emb.embed_ids(ids, lens, types).cpu()
    for i, n in enumerate(lens.tolist()):
        alone = emb.embed_ids(ids[i:i + 1, :n], torch.tensor([n]), types[i:i + 1, :n]).cpu()
        err = ref.rel_l2(together[i], alone[0])
        print(f"{name} row {i} ({n} tokens): alone vs in the batch rel L2 {err:.3e} (bound {BOUND[name]['mean']:.3e})")
        assert err < BOUND[name]["mean"]
        no_lens = emb.embed_ids(ids[i:i + 1, :n], None, types[i:i + 1, :n]).cpu()                # lens None: every token is real
        assert torch.equal(no_lens, alone)


@pytest.mark.parametrize("name", ref.TINY)
def test_the_same_batch_twice_is_bit_for_bit_equal(fx, name):
    emb = _embedder(name, fx)
    ids, lens, types = _batch(name, fx)
    a, b = emb.hidden(ids, lens, types), emb.hidden(ids, lens, types)
    real = torch.arange(ids.shape[1])[None, :] < lens[:, None]
    assert torch.equal(a.cpu()[real].view(torch.int32), b.cpu()[real].view(torch.int32))
    assert torch.equal(emb.embed_ids(ids, lens, types).cpu().view(torch.int32), emb.embed_ids(ids, lens, types).cpu().view(torch.int32))


def test_host_checks_raise_before_anything_is_uploaded(fx):
    emb = _embedder("xlmr_tiny", fx)
    ok = torch.full((1, 4), 5)
    for bad, what in ((torch.tensor([[5, 512, 5, 5]]), "token ids"), (torch.tensor([[5, -1, 5, 5]]), "token ids"), (torch.full((1, 161), 5), "position table")):
        with pytest.raises(ValueError, match=what):
            emb.hidden(bad)
    with pytest.raises(ValueError, match="type_ids"):
        emb.hidden(ok, None, torch.tensor([[0, 1, 0, 0]]))                # XLM-R has one token type
    with pytest.raises(ValueError, match="lens"):
        emb.hidden(ok, torch.tensor([5]))
    assert emb.hidden(torch.full((1, 160), 5)).shape == (1, 160, 128)      # 160 tokens + offset 2 = the table's 162 rows


def test_texts_are_truncated_sorted_and_returned_in_order(fx):
    """A text longer than max_seq_length is cut (the closing token stays) and equals the cut text; an empty text is [CLS][SEP]; the rows
    of get_embeddings are those of get_embedding, whatever batch a text lands in."""
    emb = _embedder("bert_tiny", fx)
    emb.setup = SentenceSetup("mean", False, 16)
    words = [f"word{i}" for i in range(40)]
    long_text, cut_text = " ".join(words), " ".join(words[:14])
    assert len(emb._encode(long_text)) == 16 and emb._encode(long_text) == emb._encode(cut_text)
    assert emb._encode("") == [emb.tokenizer.cls_id, emb.tokenizer.sep_id]
    texts = [long_text, "", "happy", cut_text, "a b c d e f g", "neutral"]
    emb.batch = 4
    e = emb.get_embeddings(texts)
    assert e.shape == (6, 128) and e.dtype == np.float32 and bool(np.isfinite(e).all())
    assert ref.rel_l2(e[0], e[3]) < BOUND["bert_tiny"]["mean"]            # the same ids (asserted above), in one batch or two
    for i, t in enumerate(texts):
        err = ref.rel_l2(e[i], emb.get_embedding(t))
        assert err < BOUND["bert_tiny"]["mean"], (i, err)
    c = emb.combined_embedding("happy", long_text)
    assert c.shape == (256,) and c.dtype == np.float32 and ref.rel_l2(c, np.concatenate([e[2], e[0]])) < BOUND["bert_tiny"]["mean"]
    emb.batch = 32


# ------------------------------------------------------------------------------------------------------------ directories and commands
def _write_encoder_dir(path, name, seed, sentence=None, prefix=""):
    shape = getattr(BertShape, name)()
    sd = make_bert_weights(shape, seed)
    return ref.write_dir(str(path), shape, sd, prefix=prefix, sentence=sentence), shape, sd


def test_a_checkpoint_directory_loads_and_another_family_is_refused(tmp_path, fx):
    from astts.cli import search_milvus
    from astts.llm.encoder_bert import BertEmbedder
    from astts.llm.peft import ConfigError

    d, shape, sd = _write_encoder_dir(tmp_path / "enc", "bert_tiny", int(fx["seed"]), sentence=("pooling_mode_cls_token", True, 64), prefix="bert.")
    emb = search_milvus.load_embedder(d)
    assert isinstance(emb, BertEmbedder) and emb.cfg == shape and emb.setup == SentenceSetup("cls", True, 64)
    assert not hasattr(emb, "generate_emotion_labels") and emb.cfg.hidden == 128
    # the directory's own tokenizer (vocab.txt): [CLS] = 2, [SEP] = 3, w30 -> 30, digits in pieces
    assert [int(i) for i in emb.tokenizer.encode("w30 w40 <12>")] == [2, 30, 40, 5, 8, 19, 6, 3]
    ids, lens, types = _batch("bert_tiny", fx)
    got = emb.embed_ids(ids, lens, types).cpu()
    assert ref.rel_l2(got, fx["bert_tiny.cls_norm"]) < BOUND["bert_tiny"]["cls_norm"]           # the weights that were written, CLS + Normalize
    direct = emb.get_embedding("w30 w40 w300")
    want = emb.embed_ids(torch.tensor([[2, 30, 40, 300, 3]])).cpu().numpy()[0]
    assert np.array_equal(direct, want)
    bad = tmp_path / "albert"
    bad.mkdir()
    (bad / "config.json").write_text(json.dumps({**ref.config_json(shape), "model_type": "albert"}))
    with pytest.raises(ConfigError, match="model_type"):
        search_milvus.load_embedder(str(bad))


def test_rag_and_search_json_with_an_encoder_directory(tmp_path, fx):
    """astts.cli.rag --embed_model_path builds a 256-d bank with bert_tiny (2 x 128) while a tiny Llama generates labels and biographies;
    astts.cli.search_json --embed_model_path then returns, for each row, the file an fp64 cosine search over combined_embedding vectors returns."""
    from astts.cli import rag, search_json, search_milvus
    from astts.compat.pymilvus import MilvusClient
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights

    enc_dir, shape, _ = _write_encoder_dir(tmp_path / "enc", "bert_tiny", 11)
    cfg = LlamaShape.tiny()
    llm = LlamaEmbedder(make_llama_weights(cfg, 4), cfg, DEV)
    with open(os.path.join(GOLD, "iemocap_test_sentences.json")) as f:
        sents = [s for s in json.load(f)["all"] if s.strip()][:12]
    utts = [{"speaker": ["Ann", "Bob"][i % 2], "zh_text": s, "file_id": f"utt_{i:03d}"} for i, s in enumerate(sents[:6])]
    (tmp_path / "talk.json").write_text(json.dumps(utts))
    db = str(tmp_path / "bank.db")
    args = rag.build_parser().parse_args(["--data_folder", str(tmp_path / "talk.json"), "--db_path", db, "--embed_model_path", enc_dir,
                                          "--max_new_tokens", "8", "--llm_batch", "4", "--seed", "3", "--search_text", ""])
    got = rag.main(args, embedder=llm)
    assert len(got["inserted"]) == 6 and all(len(r["vector"]) == 256 for r in got["inserted"])
    c = MilvusClient(db)
    assert c.describe_collection(rag.COLLECTION)["fields"][1]["params"]["dim"] == 256
    c.close()
    assert [h[0]["row"] for h in got["verify"]] == list(range(6))
    # queries: six OTHER sentences, the speakers' biographies from the build
    rows = [{"zh_text": s, "speaker": ["Bob", "Ann"][i % 2]} for i, s in enumerate(sents[6:])]
    (tmp_path / "in.jsonl").write_text("".join(json.dumps(r) + "\n" for r in rows))
    (tmp_path / "bios.json").write_text(json.dumps(got["biographies"]))
    sargs = search_json.build_parser().parse_args(["--input_json", str(tmp_path / "in.jsonl"), "--db_path", db, "--embed_model_path", enc_dir,
                                                   "--biography_json", str(tmp_path / "bios.json"), "--llm_batch", "1"])
    res = search_json.main(sargs, embedder=llm)
    enc = search_milvus.load_embedder(enc_dir)
    bank = np.asarray([r["vector"] for r in got["inserted"]], np.float64)
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    assert len(res) == len(rows)
    for r, rec in zip(rows, res):
        label = llm.generate_emotion_labels([r["zh_text"]])[0]
        q = enc.combined_embedding(label, got["biographies"][r["speaker"]]).astype(np.float64)
        sims = bank @ (q / np.linalg.norm(q))
        # rows within 1e-5 of the best cosine are ties to an fp32 search (its scores carry ~1e-6)
        best = {got["inserted"][int(i)]["file_id"] for i in np.nonzero(sims >= sims.max() - 1e-5)[0]}
        assert rec["retrieved_file_id"] in best and abs(float(rec["distance"]) - float(sims.max())) < 1e-4, (rec, sorted(best), float(sims.max()))
