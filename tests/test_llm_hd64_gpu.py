"""Head dimension 64 on the GPU (DESIGN.md section 2 "Head dimension 64"): the four attention kernels in their 64 form (attn_gqa_mfma and
attn_causal_gqa of csrc/ops_llm.hip, attn_bwd_dq and attn_bwd_dkdv of csrc/train/train_attn.hip), and the decoder, the generation path,
LoRA fine-tuning and the command lines over models of Llama-3.2-1B's and Qwen2.5-0.5B's geometry.

Bounds.  Attention forward: tests/llm_attn_hd_ref.py's ATTN64_TOL per query row (3 x the measured fp16-emulation floor), pad-query rows
exactly zero.  Attention backward: the rule of tests/test_qwen2_gpu.py, 4 x (rel_l2(fp16 emulation, fp32) + 2 * 2^-11) per dq / dk / dv
against fp32 autograd.  Whole models: relative L2 per tensor, 4 x the error of the fp16-rounded CPU restatement -- for tiny64 against the
transformers fixture tests/golden/llama_hd64.npz as tests/golden/make_llama_hd64_fixtures.py prints it (the emulated value stands beside
each constant); for qwen2_tiny64 and wide64 against the fp32 restatement, both run live on the CPU."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import llama_hd64_ref as lref  # noqa: E402
import llm_attn_hd_ref as ref  # noqa: E402
import llm_int8_ref as i8  # noqa: E402
import llm_train_ref as tref  # noqa: E402
import qwen2_ref as q2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H16 = 2.0 ** -11
HD = 64

# emulated (fp16-rounded restatement vs the transformers fixture) -> bound = 4x
HIDDEN_BOUND = 4 * 6.085e-4            # last-layer hidden states of the 199 real positions
EMBED_BOUND = 4 * 5.929e-4             # mean-pooled embeddings
LOGITS_BOUND = 4 * 5.122e-4            # last-position logits
LOGPROB_BOUND = 4 * 7.295e-5           # token log-probabilities
LOSS_BOUND = 4 * 3.524e-6              # mean next-token loss with the seeded LoRA (relative)
GRAD_BOUND = 4 * 1.629e-3              # worst LoRA gradient (layer 2 q_proj B)
FIXTURE_GRAD_STORAGE = 2.0 ** -16      # the fixture's gradients keep 16 mantissa bits


# ------------------------------------------------------------------------------------------------------------ attention forward
def _attn(case, kernel):
    """One case of llm_attn_hd_ref through the kernel -> [B, heads, Tq, 64] on the CPU."""
    from astts import ops
    x = ref.build_attn(case)
    hq, hk = case.heads * HD, case.kv_heads * HD
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)
    if case.form == "bm":
        d = x.bufs["qkv"].to(DEV)
        q, k, v = d[..., :hq], d[..., hq:hq + hk], d[..., hq + hk:]
        out = ops.attn_causal_gqa(q, k, v, case.heads, case.kv_heads, HD, i32(case.lens)) if kernel == "valu" else \
            ops.attn_gqa(q, k, v, case.heads, case.kv_heads, HD, lens=i32(case.lens))
    else:
        q, cache = x.bufs["q"].to(DEV), x.bufs["cache"].to(DEV)
        out = ops.attn_gqa(q, cache[:case.tk, :, :hk], cache[:case.tk, :, hk:], case.heads, case.kv_heads, HD, lens=i32(case.lens),
                           key_start=i32(case.key_start), pos0=case.pos0, time_major=True)
    return ref.heads_first(out.cpu(), case)


FORWARD = [(c, "mfma") for c in ref.CASES_64] + [(c, "valu") for c in ref.CASES_BM_64]


@pytest.mark.parametrize("case,kernel", FORWARD, ids=[f"{k}-{c.name}" for c, k in FORWARD])
def test_attention_forward_at_64(case, kernel):
    got, want = _attn(case, kernel), ref.attn_expected(case)
    assert bool(torch.isfinite(got).all())
    err, bad = ref.row_errors(got, want)
    print(f"[parity] attention hd64 {case.name} ({kernel}): worst per-row err {float(err.max()):.2e} (bound {ref.ATTN64_TOL:.2e})")
    assert not bool(bad.any()), (case.name, kernel, "a pad-query row is not exactly zero")
    assert float(err.max()) <= ref.ATTN64_TOL, (case.name, kernel, float(err.max()))


# ------------------------------------------------------------------------------------------------------------ attention backward
@pytest.mark.parametrize("heads,kv_heads", [(8, 2), (14, 2)])
@pytest.mark.parametrize("t", [1, 33, 130])
def test_attention_backward_at_64(heads, kv_heads, t):
    """train_ops.attn_gqa_bwd against fp32 autograd through llm_train_ref.attention in both formulations; rows beyond lens exactly
    zero; two runs give the same bits."""
    from astts import train_ops as tops
    g = torch.Generator().manual_seed(640 + heads + t)
    lens = (130, 64, 5) if t == 130 else (t, max(1, t // 2))
    b, d = len(lens), HD
    w = (heads + 2 * kv_heads) * d
    qkv = torch.randn(b, t, w, generator=g).half()
    dout = torch.randn(b, t, heads * d, generator=g).half()
    ln = torch.tensor(lens)

    def cpu(expand, h16=False):
        x = qkv.float().requires_grad_(True)
        q, k, v = x[..., :heads * d], x[..., heads * d:(heads + kv_heads) * d], x[..., (heads + kv_heads) * d:]
        o = tref.attention(q.reshape(b, t, heads, d), k.reshape(b, t, kv_heads, d), v.reshape(b, t, kv_heads, d), ln, heads, kv_heads,
                           expand=expand, h16=h16)
        o.backward(dout.float())
        return x.grad

    want, want2, emu = cpu(False), cpu(True), cpu(False, h16=True)
    run = lambda: tops.attn_gqa_bwd(qkv.to(DEV), dout.to(DEV), heads, kv_heads, d, ln.to(DEV, torch.int32))
    first, second = run(), run()
    assert torch.equal(first, second)
    got = first.float().cpu()
    assert torch.isfinite(got).all()
    for i in range(b):
        assert not got[i, lens[i]:].any()
    cuts = (0, heads * d, (heads + kv_heads) * d, w)
    for name, lo, hi in zip(("dq", "dk", "dv"), cuts[:-1], cuts[1:]):
        bound = 4 * (tref.rel_l2(emu[..., lo:hi], want[..., lo:hi]) + 2 * H16)
        e1, e2 = tref.rel_l2(got[..., lo:hi], want[..., lo:hi]), tref.rel_l2(got[..., lo:hi], want2[..., lo:hi])
        print(f"[parity] attn_bwd hd64 heads={heads}/{kv_heads} t={t} {name}: rel L2 {e1:.2e} / {e2:.2e} (bound {bound:.2e})")
        assert e1 <= bound and e2 <= bound, (name, e1, e2, bound)


# ------------------------------------------------------------------------------------------------------------ Llama, tiny64
@pytest.fixture(scope="module")
def fx():
    z = {**np.load(os.path.join(GOLD, "llama_hd64.npz")), **np.load(os.path.join(GOLD, "llama_hd64_train.npz"))}
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.tiny64()
    sd = make_llama_weights(cfg, int(z["seed"]))
    return z, cfg, sd, torch.from_numpy(z["ids"]), torch.from_numpy(z["lens"])


@pytest.fixture(scope="module")
def emb64(fx):
    from astts.llm.embedder import LlamaEmbedder
    _, cfg, sd, _, _ = fx
    return LlamaEmbedder(sd, cfg, DEV)


def _forward(emb, ids, lens):
    """What the fixture records of one forward pass, from the GPU model."""
    from astts import ops
    hf = emb.hidden(ids, lens.to(DEV, torch.int32))
    last = torch.stack([hf[i, int(n) - 1] for i, n in enumerate(lens)]).contiguous()
    return {"hidden": torch.cat([hf[i, :int(n)] for i, n in enumerate(lens)]).cpu(), "embedding": emb.embed_ids(ids, lens).cpu(),
            "logits_last": ops.linear(last, emb.head).cpu(), "logprobs": emb.token_logprobs(ids, lens).cpu()}


def _cut(tokens, cfg):
    """A continuation up to and including its first EOS (where generate_greedy_batch stops a row)."""
    out = []
    for t in tokens:
        out.append(int(t))
        if int(t) == cfg.eos_token_id:
            break
    return out


def test_llama_tiny64_matches_the_transformers_fixture(fx, emb64):
    z, cfg, sd, ids, lens = fx
    assert emb64.cfg.head_dim == 64 and (cfg.heads, cfg.kv_heads) == (8, 2)
    got = _forward(emb64, ids, lens)
    errs = {k: lref.rel_l2(got[k], z[k]) for k in got}
    bounds = {"hidden": HIDDEN_BOUND, "embedding": EMBED_BOUND, "logits_last": LOGITS_BOUND, "logprobs": LOGPROB_BOUND}
    for k, e in errs.items():
        print(f"[parity] llama hd64 fp16 vs transformers: {k} rel L2 {e:.3e} (bound {bounds[k]:.3e})")
    for k, e in errs.items():
        assert e <= bounds[k], (k, e, bounds[k])
    # the same rows one text at a time (no padding), and the second attention kernel
    one = torch.cat([emb64.embed_ids(ids[i:i + 1, :int(n)]).cpu() for i, n in enumerate(lens)])
    assert lref.rel_l2(one, z["embedding"]) <= EMBED_BOUND
    emb64.mfma_attention = False
    try:
        e_v = lref.rel_l2(emb64.embed_ids(ids, lens).cpu(), z["embedding"])
    finally:
        emb64.mfma_attention = True
    print(f"[parity] llama hd64 fp16 vs transformers: embedding with the VALU attention {e_v:.3e} (bound {EMBED_BOUND:.3e})")
    assert e_v <= EMBED_BOUND


def test_llama_tiny64_greedy_cached_and_recomputed(fx, emb64):
    """The fixture's 8-token continuations through the KV-cache layout (left-padded batch, decode steps of one query over a time-major
    cache at head dimension 64), one prompt at a time, and with the prompt re-run for every token."""
    z, cfg, _, ids, lens = fx
    prompts = [ids[i, :int(n)].tolist() for i, n in enumerate(lens)]
    batch = emb64.generate_greedy_batch(prompts, lref.GEN_LEN)
    for p, got, want in zip(prompts, batch, z["greedy"]):
        assert got[len(p):] == _cut(want, cfg), (len(p), got[len(p):], want.tolist())
        assert got == emb64.generate_greedy_recompute(p, lref.GEN_LEN), (len(p), got[len(p):])
        assert got == emb64.generate_greedy(p, lref.GEN_LEN)


def _trainer(cfg, sd, lora, r, alpha, **kw):
    from astts.llm.peft import PROJ, LoraAdapter
    from astts.llm.train import LoraTrainer
    ad = LoraAdapter(r=r, lora_alpha=alpha, use_rslora=False, targets=tuple(PROJ), base_model_name_or_path="", pairs=dict(lora))
    return LoraTrainer(sd, cfg, DEV, adapter=ad, lr=1e-3, total_steps=1, warmup_ratio=0.0, loss_scale=1.0, **kw)


def test_llama_tiny64_training_loss_and_gradients(fx):
    z, cfg, sd, ids, lens = fx
    lora = lref.make_lora(cfg, int(z["r"]), int(z["lora_seed"]))
    tr = _trainer(cfg, sd, lora, int(z["r"]), float(z["lora_alpha"]))
    loss = tr.accumulate([(ids, lens)])
    want = float(z["loss"])
    print(f"[parity] llama hd64 training: loss {loss:.6f} vs {want:.6f} rel {abs(loss - want) / want:.2e} (bound {LOSS_BOUND:.2e})")
    worst, where = 0.0, None
    grads = {k: v.detach().cpu().clone() for k, v in tr.named_grads().items()}
    for (i, p, h), gr in grads.items():
        e = lref.rel_l2(gr, z[f"grad.{i}.{p}.{h}"])
        if e > worst:
            worst, where = e, (i, p, h)
    print(f"[parity] llama hd64 training: worst LoRA gradient rel L2 {worst:.3e} at {where} (bound {GRAD_BOUND:.3e})")
    assert abs(loss - want) <= LOSS_BOUND * want
    assert len(grads) == 2 * 7 * cfg.layers and worst <= GRAD_BOUND + FIXTURE_GRAD_STORAGE, (where, worst)


def test_llama_tiny64_step_repeats_and_the_adapter_reloads(fx, tmp_path):
    """Two identical steps from the same state give the same bits; the saved adapter, loaded over the written base through
    load_peft_model into LlamaEmbedder, reproduces the trainer's own forward loss."""
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.peft import load_peft_model
    from astts.llm.weights import load_llama_weights
    z, cfg, sd, ids, lens = fx
    lora = lref.make_lora(cfg, int(z["r"]), int(z["lora_seed"]))
    base = i8.write_base(str(tmp_path / "base"), cfg, sd)
    sd16 = load_llama_weights(base)
    runs = []
    for _ in range(2):
        tr = _trainer(cfg, sd16, lora, int(z["r"]), float(z["lora_alpha"]))
        tr.step([(ids[:2], lens[:2]), (ids[2:], lens[2:])])                   # two micro-batches: the accumulation path too
        runs.append((tr.grads.clone(), tr.params.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and bool(runs[0][0].any())
    tr.save_adapter(str(tmp_path / "adapter"))
    own = tr.loss(ids, lens)
    state, cfg2, ad, _ = load_peft_model(str(tmp_path / "adapter"), base)
    assert cfg2.head_dim == 64 and dataclasses.replace(cfg2, eos_token_ids=()) == cfg     # the loader adds generation_config's stop ids
    emb = LlamaEmbedder(state, cfg2, DEV, lora=ad)
    count = int((lens - 1).sum())
    inf = -float(emb.token_logprobs(ids.to(DEV), lens.to(DEV, torch.int32)).sum()) / count
    print(f"[parity] llama hd64 round trip: trainer {own:.6f} inference {inf:.6f} rel {abs(own - inf) / own:.2e} (bound {LOSS_BOUND:.2e})")
    assert abs(own - inf) <= LOSS_BOUND * own           # the two roundings of the same LoRA: a part of what LOSS_BOUND is made of


# ------------------------------------------------------------------------------------------------------------ Qwen2 and the real widths
def _against_the_restatement(name, cfg, sd, ids, lens, mod, run):
    """GPU hidden states / embedding / last logits against the fp32 CPU restatement; bound = 4 x the restatement's own fp16-rounded run."""
    from astts.llm.embedder import LlamaEmbedder
    want, emu = run(False), run(True)
    got = _forward(LlamaEmbedder(sd, cfg, DEV), ids, lens)
    for k in ("hidden", "embedding", "logits_last"):
        bound, e = 4 * mod.rel_l2(emu[k], want[k]), mod.rel_l2(got[k], want[k])
        print(f"[parity] {name} vs the fp32 restatement: {k} rel L2 {e:.3e} (emulated {bound / 4:.3e}, bound {bound:.3e})")
        assert e <= bound, (name, k, e, bound)


def test_qwen2_tiny64_matches_the_restatement():
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.qwen2_tiny64()
    sd = make_llama_weights(cfg, q2.SEED)
    ids, lens = q2.make_batch(cfg, q2.LENS, q2.BATCH_SEED)
    _against_the_restatement("qwen2_tiny64", cfg, sd, ids, lens, q2, lambda h16: q2.outputs(sd, cfg, q2.fp_linear(sd, cfg, h16=h16), ids, lens, h16=h16))


def test_wide64_matches_the_restatement():
    """Llama-3.2-1B's widths: one batch of 64 + 33 tokens."""
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.wide64()
    sd = make_llama_weights(cfg, lref.SEED)
    ids, lens = lref.make_batch(cfg, (64, 33), 7)
    _against_the_restatement("wide64", cfg, sd, ids, lens, lref, lambda h16: lref.outputs(sd, cfg, ids, lens, h16=h16))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("with_key", [False, True])
def test_clis_over_a_head_dim_64_base_directory(tmp_path, with_key):
    """A Qwen2.5-0.5B-shaped base directory (config.json with or without an explicit head_dim): search_milvus and search_json load it
    by its config.json and build a query of 2 x hidden (refused against the shipped 6144-d bank by dimension, which proves the query
    was made); ft_llm trains one step over it and writes an adapter directory that evaluate_erc loads."""
    from astts.cli import evaluate_erc, ft_llm, search_json, search_milvus
    from astts.llm.config import LlamaShape
    from astts.llm.peft import load_adapter
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.qwen2_tiny64()
    conf = q2.config_json(cfg)
    assert "head_dim" not in conf
    if with_key:
        conf["head_dim"] = 64
    base = q2.write_base(str(tmp_path / "base"), cfg, make_llama_weights(cfg, q2.SEED), config=conf)
    emb = search_milvus.load_embedder(base)
    assert emb.cfg == cfg and emb.cfg.head_dim == 64 and not emb.int8
    q = emb.combined_embedding("neutral", "A pragmatic and thoughtful person.")
    assert q.shape == (2 * 896,) and q.dtype == np.float32 and bool(np.isfinite(q).all())
    db = os.path.join(GOLD, "milvus_demo.db")                                 # the shipped bank: 6144-d
    with pytest.raises(SystemExit, match=r"1792 dimensions.*896.*6144-dimensional"):
        search_milvus.main(search_milvus.build_parser().parse_args(["--db_path", db, "--model_path", base, "--top_k", "3"]))
    inp = tmp_path / "in.jsonl"
    inp.write_text(json.dumps({"zh_text": "Fine, whatever.", "speaker": "JOHN"}) + "\n")
    with pytest.raises(SystemExit, match=r"1792 dimensions.*6144-dimensional"):
        search_json.main(search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db, "--model_path", base]))
    words = [f"w{i}" for i in range(97)]
    with open(tmp_path / "toy.train.0shot_w5_spdescV2.jsonl", "w") as f:
        for i in range(40):
            said = " ".join(words[(7 * i + j) % 97] for j in range(20 + i % 9))
            f.write(json.dumps({"messages": [{"role": "user", "content": said}, {"role": "assistant", "content": words[i % 5]}]}) + "\n")
    ft_llm.main(ft_llm.build_parser().parse_args(
        ["--do_train", "--packing", "--max_seq_len", "64", "--max_steps", "1", "--lora_r", "8", "--loss_scale", "1", "--data_name", "toy",
         "--data_folder", str(tmp_path), "--output_folder", str(tmp_path / "out"), "--ft_model_id", "ft", "--base_model_id", base]))
    out = str(tmp_path / "out" / "ft")
    log = [json.loads(line) for line in open(os.path.join(out, "train_log.jsonl"))]
    assert len(log) == 1 and np.isfinite(log[0]["loss"]) and np.isfinite(log[0]["grad_norm"]) and not log[0]["skipped"]
    ad = load_adapter(out)
    assert ad.r == 8 and len(ad.pairs) == 3 * 7
    res = evaluate_erc.main(evaluate_erc.build_parser().parse_args(
        ["--model_path", out, "--base_model_path", base, "--data_file", os.path.join(GOLD, "erc_valid_subset.jsonl"), "--limit", "3",
         "--method", "both"]))
    assert len(res["detail_pred"]) == 3 and 0.0 <= res["f1_weighted"] <= 1.0 and res["gold_label_nll"] > 0


# ------------------------------------------------------------------------------------------------------------ refusals
def test_head_dim_96_is_refused_by_name():
    from astts import _lib, _lib_train, ops
    from astts import train_ops as tops
    from astts.llm.config import LlamaShape
    from astts.llm.decoder import LlamaDecoder
    with pytest.raises(ValueError, match="96"):
        LlamaDecoder({}, dataclasses.replace(LlamaShape.tiny64(), head_dim=96), DEV)
    heads, kvh, t = 2, 1, 8
    qkv = torch.zeros(1, t, (heads + 2 * kvh) * 96, dtype=torch.float16, device=DEV)
    q, k, v = qkv[..., :heads * 96], qkv[..., heads * 96:(heads + kvh) * 96], qkv[..., (heads + kvh) * 96:]
    for call, last in ((lambda: ops.attn_causal_gqa(q, k, v, heads, kvh, 96), _lib.load().astts_last_error_string),
                       (lambda: ops.attn_gqa(q, k, v, heads, kvh, 96), _lib.load().astts_last_error_string),
                       (lambda: tops.attn_gqa_bwd(qkv, torch.zeros(1, t, heads * 96, dtype=torch.float16, device=DEV), heads, kvh, 96),
                        _lib_train.load().astts_train_last_error_string)):
        with pytest.raises(_lib.AsttsError) as exc:
            call()
        msg = last().decode()
        assert exc.value.code == _lib.ERR_UNSUPPORTED and "96" in msg and "64" in msg and "128" in msg, (exc.value.code, msg)
