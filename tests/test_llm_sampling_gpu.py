"""GPU side of the sampled LLM generation: astts_op_sample_topk_topp (csrc/ops_sample.hip) against its numpy statement
(tests/llm_sampling_ref.py) and the committed answers, LlamaEmbedder.generate_sample_batch on the tiny model (fp16 and int8 + LoRA),
and the two drivers end to end.  Every comparison of tokens runs all of its rows and steps; what keeps it meaningful is asserted on the
reference side: every margin of the inputs is >= llm_sampling_ref.MARGIN (1e-5, ~10x the fp32 error of a 50-term sum and a division)."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import llm_int8_ref as i8ref
import llm_sampling_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(x, u, temperature, top_k, top_p, vocab):
    from astts import ops

    d = torch.from_numpy(x).to(DEV)
    return ops.sample_topk_topp(d[:, :vocab], torch.from_numpy(u).to(DEV), temperature, top_k, top_p).cpu().numpy()


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_operator_matches_reference_and_committed_answers(case):
    """128 256-wide rows (1, 8, 32 and all 64 at once), ld > vocab with and without 16-byte row alignment, top_k in {1, 50, 1024},
    top_p in {0.5, 0.9, 1.0}, temperature in {0.7, 1.0}, vocabularies 7 / 1 000 / 4 097: the token of every row equals the reference's."""
    name, seed, rows, vocab, ld, scales, temperature, top_k, top_p = case
    x, u = ref.case_inputs(case)
    tokens, margin, _ = ref.sample_rows(x[:, :vocab], u, temperature, top_k, top_p)
    print(f"[sampling] {name}: smallest margin {margin:.2e}")
    assert margin >= ref.MARGIN
    fx = np.load(os.path.join(GOLD, "sampling_kats.npz"))
    assert np.array_equal(fx[name + "/tokens"], tokens)
    got = _run(x, u, temperature, top_k, top_p, vocab)
    print(f"[sampling] {name}: {int((got != tokens).sum())} of {rows} rows differ")
    assert np.array_equal(got, tokens), (name, np.nonzero(got != tokens)[0].tolist())
    if name == "wide64":
        for r0, n in ((0, 1), (1, 8), (9, 32)):
            part = _run(np.ascontiguousarray(x[r0:r0 + n]), u[r0:r0 + n], temperature, top_k, top_p, vocab)
            assert np.array_equal(part, tokens[r0:r0 + n]), (r0, n)
    # the same call again: the same tokens
    assert np.array_equal(_run(x, u, temperature, top_k, top_p, vocab), got)


def test_exact_ties_resolve_by_token_id():
    """Logits drawn from nine values: thousands of exact fp32 ties at the k-th place.  The kept set is then decided by integer key and
    id comparisons alone (no rounding is involved, so the k-th-place margin does not apply); the other two margins are asserted.  A
    constant row takes the path where the candidates overflow LDS."""
    rng = np.random.default_rng(78)
    x = rng.integers(-4, 5, (6, 128256)).astype(np.float32)
    x[4] = 0.25
    x[5, 1000:] = -0.0
    x[5, :1000] = 0.0
    u = rng.random(6).astype(np.float32)
    for top_k, top_p in ((50, 0.905), (1024, 0.9703)):       # not a multiple of the tied entries' common probability
        _, _, rows = ref.sample_rows(x, u, 0.7, top_k, top_p)
        assert min(min(r.nucleus, r.draw) for r in rows) >= ref.MARGIN
        got = _run(x, u, 0.7, top_k, top_p, 128256)
        assert got.tolist() == [r.token for r in rows], (top_k, got.tolist(), [r.token for r in rows])


def test_draws_follow_the_renormalised_nucleus():
    """One 128 256-wide row at scale 1, 4 096 stratified uniforms u_i = (i + 0.5) / 4096: the drawn tokens are exactly the nucleus, and
    each count is within 2 of 4096 q (the exact stratified count is within 1; the second unit covers an fp32 cdf boundary)."""
    x = ref.normal_rows(5, 1, 128256)
    r = ref.sample_row(x[0], 0.5, 0.7, 50, 0.9)
    assert len(r.ids) >= 8 and min(r.kth, r.nucleus) >= ref.MARGIN
    d = torch.from_numpy(np.repeat(x, 256, 0)).to(DEV)
    from astts import ops

    u = (np.arange(4096, dtype=np.float64) + 0.5) / 4096
    got = np.concatenate([ops.sample_topk_topp(d, torch.from_numpy(u[i:i + 256].astype(np.float32)).to(DEV), 0.7, 50, 0.9).cpu().numpy()
                          for i in range(0, 4096, 256)])
    ids, counts = np.unique(got, return_counts=True)
    assert sorted(ids.tolist()) == sorted(r.ids.tolist())
    want = {int(t): 4096 * float(q) for t, q in zip(r.ids, r.q)}
    worst = max(abs(int(c) - want[int(t)]) for t, c in zip(ids, counts))
    print(f"[sampling] nucleus of {len(r.ids)} tokens, largest |count - 4096 q| = {worst:.2f}")
    assert worst <= 2.0


# ------------------------------------------------------------------------------------------------------------ the embedder
def _tiny(kind, tmp_path):
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights

    if kind == "fp16":
        fx = np.load(os.path.join(GOLD, "llama_tiny.npz"))
        cfg = LlamaShape.tiny()
        sd = make_llama_weights(cfg, int(fx["seed"]))
        return LlamaEmbedder(sd, cfg, DEV), sd, cfg, None
    from astts.llm.peft import load_peft_model

    cfg = LlamaShape.tiny()
    sd = make_llama_weights(cfg, 0)
    sd["model.layers.0.input_layernorm.weight"][[5, 17, 100]] = 25.0                    # activations that cross the LLM.int8 threshold
    base = i8ref.write_base(str(tmp_path / "base"), cfg, sd)
    ada = i8ref.write_adapter(str(tmp_path / "adapter"), i8ref.make_lora(cfg, 32, 1), 32, 128, base="org/not-on-this-disk")
    state, cfg2, ad, _ = load_peft_model(ada, base)
    lora = {(i, p[:-5]): ab for (i, p), ab in ad.pairs.items()}
    lin = i8ref.make_linear(state, cfg2, lora, ad.scaling, int8=True, tau=6.0)
    return LlamaEmbedder(state, cfg2, DEV, int8=True, lora=ad), state, cfg2, lin


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


PROMPT_LENS = (9, 14, 5)
N_NEW = 17


class _Run:
    """One 17-step sampled decode of three left-padded prompts with return_logits=True, and what the reference sampler makes of the
    RETURNED logits with the same uniforms (``toks``: every step of every row, also beyond a row's EOS)."""

    def __init__(self, kind, tmp_path):
        self.kind = kind
        self.emb, self.sd, self.cfg, self.lin = _tiny(kind, tmp_path)
        g = torch.Generator().manual_seed(3)
        self.prompts = [torch.randint(3, self.cfg.vocab, (n,), generator=g).tolist() for n in PROMPT_LENS]
        self.u = np.random.default_rng(1).random((N_NEW, len(self.prompts))).astype(np.float32)
        self.rows, logits = self.emb.generate_sample_batch(self.prompts, N_NEW, uniforms=torch.from_numpy(self.u), return_logits=True)
        self.lg = logits.cpu().numpy()
        self.toks, self.margin = self.replay(self.lg, self.u)

    @staticmethod
    def replay(lg, u):
        toks, worst = np.zeros(u.shape, np.int64), float("inf")
        for s in range(u.shape[0]):
            toks[s], margin, _ = ref.sample_rows(lg[s], u[s], 0.7, 50, 0.9)
            worst = min(worst, margin)
        return toks, worst

    def with_eos(self, ids):
        """The same embedder with further stop ids (``_is_eos`` and the completion poll read ``emb.cfg``)."""
        import copy

        e = copy.copy(self.emb)
        e.cfg = dataclasses.replace(self.cfg, eos_token_ids=tuple(int(i) for i in ids))
        return e


@pytest.fixture(scope="module", params=["fp16", "int8_lora"])
def run(request, tmp_path_factory):
    return _Run(request.param, tmp_path_factory.mktemp(request.param))


def test_sampled_tokens_are_the_reference_samplers_on_the_returned_logits(run):
    """The sampler apart from the model's numerics: replaying the reference on the returned logits with the same uniforms gives the
    returned tokens at every step of every row (51 draws, margins asserted)."""
    assert run.lg.shape == (N_NEW, len(run.prompts), run.cfg.vocab) and run.lg.dtype == np.float32
    print(f"[sampling] {run.kind}: smallest margin over {run.toks.size} draws {run.margin:.2e}")
    assert run.margin >= ref.MARGIN
    for j, p in enumerate(run.prompts):
        assert run.rows[j][:len(p)] == p
        new = run.rows[j][len(p):]
        assert new == run.toks[:len(new), j].tolist(), (j, new, run.toks[:, j].tolist())
        assert len(new) == N_NEW or run.emb._is_eos(new[-1])


def test_returned_logits_are_the_models_teacher_forced(run):
    """The returned logits against the model run on prompt + the GPU's tokens.  fp16: oracle/llama.py on the fixture's seeded weights --
    the fp32 restatement of transformers' Llama that tests/golden/llama_tiny.npz pins to 1e-5 (tests/test_oracle_llama.py); the
    committed fixture itself holds logits for its own greedy tokens only.  int8 + LoRA: the restatement of tests/llm_int8_ref.py.
    Bar: 1e-2 of the logits' scale, what tests/test_llm_gpu.py holds this configuration's logits to."""
    import oracle.llama as ol

    for j, p in enumerate(run.prompts):
        if run.kind == "fp16":
            forced = p + run.toks[:-1, j].tolist()
            h = ol.forward_hidden(run.sd, run.cfg, torch.tensor([forced]))[0, len(p) - 1:]
            want = (h @ run.sd["model.embed_tokens.weight"].T).numpy()
        else:
            d = i8ref.Decoder(run.sd, run.cfg, run.lin, 6.0, fp16_io=True)
            hs = [d.step(p)[-1]] + [d.step([int(t)])[-1] for t in run.toks[:-1, j]]
            want = torch.stack([d.logits(h) for h in hs]).numpy()
        e = _rel(run.lg[:, j], want)
        print(f"[sampling] {run.kind}: row {j} teacher-forced logits rel err {e:.2e}")
        assert e < 1e-2, (j, e)


def test_sampled_decode_is_repeatable_and_rows_draw_from_their_own_uniforms(run):
    emb, prompts = run.emb, run.prompts
    assert emb.generate_sample_batch(prompts, N_NEW, uniforms=torch.from_numpy(run.u)) == run.rows
    auto = emb.generate_sample_batch(prompts, N_NEW, seed=5)
    manual = torch.stack([emb.row_uniforms(5, j, N_NEW) for j in range(len(prompts))], 1)
    assert auto == emb.generate_sample_batch(prompts, N_NEW, uniforms=manual)       # default uniforms: keyed by (seed, row index)
    bad = pytest.raises(ValueError, emb.generate_sample_batch, prompts, 4, uniforms=torch.zeros(3, len(prompts)))
    assert "max_new_tokens" in str(bad.value)


def test_rows_are_cut_at_their_first_eos(run):
    """max_new_tokens 1 and 17; the stop id is a token row 0 drew at step 5."""
    one = run.emb.generate_sample_batch(run.prompts, 1, uniforms=torch.from_numpy(run.u[:1]))
    assert [r[len(p):] for r, p in zip(one, run.prompts)] == [[int(t)] for t in run.toks[0]]
    emb = run.with_eos([run.toks[5, 0]])
    cut = emb.generate_sample_batch(run.prompts, N_NEW, uniforms=torch.from_numpy(run.u))
    for j, p in enumerate(run.prompts):
        full = run.toks[:, j].tolist()
        stop = next((s for s, t in enumerate(full) if emb._is_eos(t)), N_NEW - 1)
        assert cut[j] == p + full[:stop + 1], j
    assert len(cut[0]) <= len(run.prompts[0]) + 6


def test_completion_poll_changes_no_returned_token(run):
    """40 steps with every row ended by step 3: the poll at step 32 stops the loop; the rows equal the unpolled run's, cut."""
    b = len(run.prompts)
    u40 = np.random.default_rng(9).random((40, b)).astype(np.float32)
    _, l40 = run.emb.generate_sample_batch(run.prompts, 40, uniforms=torch.from_numpy(u40), return_logits=True)      # no poll on this path
    t40, margin = run.replay(l40.cpu().numpy(), u40)
    assert margin >= ref.MARGIN
    emb = run.with_eos(t40[3])
    polled = emb.generate_sample_batch(run.prompts, 40, uniforms=torch.from_numpy(u40))
    for j, p in enumerate(run.prompts):
        full = t40[:, j].tolist()
        stop = next(s for s, t in enumerate(full) if emb._is_eos(t))
        assert stop <= 3 and polled[j] == p + full[:stop + 1], j


def test_greedy_path_is_unchanged(run):
    for p, got in zip(run.prompts, run.emb.generate_greedy_batch(run.prompts, 6)):
        assert got == run.emb.generate_greedy_recompute(p, 6)


def test_biography_prompt_and_decoding():
    """milvus/search_json.py:129-150: the prompt character for character, decoded with skip_special_tokens=True, the prompt removed."""
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights

    cfg = LlamaShape.tiny()
    seen = {}

    class Tok:
        def encode(self, text):
            seen["prompt"] = text
            return [cfg.bos_token_id] + [3 + (len(w) * 7 + ord(w[0])) % (cfg.vocab - 3) for w in text.split()]

        def decode(self, ids, skip_special_tokens=False):
            seen["decode"] = (list(ids), skip_special_tokens)
            return seen["prompt"] + "  A careful, dry-witted person. \n"

    emb = LlamaEmbedder(make_llama_weights(cfg, 7), cfg, DEV, tokenizer=Tok())
    bio = emb.generate_biography("Hi.\nHow are you?", "Ann", max_new_tokens=5, seed=3)
    assert bio == "A careful, dry-witted person."
    assert seen["prompt"] == ('\nGiven this conversation between speakers:\n"\nHi.\nHow are you?\n"\nIn overall of above conversation, what do you think about '
                              'the characteristics of speaker Ann? (Note: provide an answer within 250 words)\n')
    ids, skip = seen["decode"]
    assert skip is True and len(ids) > len(seen["prompt"].split()) + 1
    assert emb.generate_biographies([("Hi.\nHow are you?", "Ann")], 5, 3) == [bio]


# ------------------------------------------------------------------------------------------------------------ the drivers
def test_rag_and_search_json_end_to_end(tmp_path, capsys):
    """astts.cli.rag on seeded tiny weights with the stand-in tokenizer: 12 utterances of the IEMOCAP test sentences over 3 invented
    speakers -> a 12-row bank of 2 * hidden, every row its own top-1, the same command twice byte-identical; then astts.cli.search_json
    --generate_biographies against that bank, and its --biography_out read back."""
    from astts.cli import rag, search_json
    from astts.compat.pymilvus import MilvusClient
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights

    cfg = LlamaShape.tiny()
    emb = LlamaEmbedder(make_llama_weights(cfg, 4), cfg, DEV)
    with open(os.path.join(GOLD, "iemocap_test_sentences.json")) as f:
        sents = [s for s in json.load(f)["all"] if s.strip()][:12]
    utts = [{"speaker": ["Ann", "Bob", "Cy"][i % 3], "zh_text": s, "file_id": f"utt_{i:03d}"} for i, s in enumerate(sents)]
    data = tmp_path / "talk.json"
    data.write_text(json.dumps(utts))
    dumps = []
    for run in range(2):
        db, dump = str(tmp_path / f"bank{run}.db"), str(tmp_path / f"dump{run}.json")
        args = rag.build_parser().parse_args(["--data_folder", str(data), "--db_path", db, "--output_file", dump, "--max_new_tokens", "12",
                                              "--llm_batch", "2", "--seed", "3", "--top_k", "3"])
        got = rag.main(args, embedder=emb)
        dumps.append(open(dump, "rb").read())
    assert dumps[0] == dumps[1]
    out = capsys.readouterr().out
    assert len(got["inserted"]) == 12 and [r["id"] for r in got["inserted"]] == [1, 2, 3, 4] * 3
    assert all(len(r["vector"]) == 2 * cfg.hidden for r in got["inserted"])
    assert [h[0]["row"] for h in got["verify"]] == list(range(12))
    assert out.count("Query ID: ") == 24 and "Top 3 results for the query" in out
    c = MilvusClient(db)
    assert c.describe_collection(rag.COLLECTION)["num_entities"] == 12 and c.describe_collection(rag.COLLECTION)["fields"][1]["params"]["dim"] == 2 * cfg.hidden
    c.close()
    assert len(set(got["biographies"].values())) == 3 and all(got["biographies"].values())
    # search_json with generated biographies against the new bank
    inp = tmp_path / "in.jsonl"
    inp.write_text("".join(json.dumps({"zh_text": u["zh_text"], "speaker": u["speaker"]}) + "\n" for u in utts))
    a = search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db, "--generate_biographies", "--max_new_tokens", "12",
                                               "--llm_batch", "2", "--seed", "3", "--biography_out", str(tmp_path / "bios.json"),
                                               "--output_file", str(tmp_path / "hand_off.jsonl")])
    res = search_json.main(a, embedder=emb)
    recs = [json.loads(l) for l in open(tmp_path / "hand_off.jsonl")]
    assert recs == res and len(recs) == 12
    assert all(set(r) == {"zh_text", "speaker", "retrieved_file_id", "retrieved_text", "distance"} and r["retrieved_file_id"].startswith("utt_") for r in recs)
    bios = search_json.load_biographies(str(tmp_path / "bios.json"))
    # the same speakers, conversations, seed and batches as the bank's build: the same biographies
    assert bios == got["biographies"]
    b = search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db, "--biography_json", str(tmp_path / "bios.json")])
    assert search_json.main(b, embedder=emb) == res
