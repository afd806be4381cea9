"""The Qwen2 track on the GPU (DESIGN.md section 2 "Qwen2"): the decoder with q | k | v biases, plain RoPE, an untied head and a GQA group
of 7, in fp16, in LLM.int8 + LoRA and under LoRA fine-tuning, against tests/golden/qwen2_tiny.npz / qwen2_tiny_train.npz (transformers'
Qwen2ForCausalLM, fp32, CPU) and the restatements of tests/qwen2_ref.py.

Bounds.  Relative L2 per tensor.  Every whole-model bound is 4 x the error of the fp16-rounded CPU restatement (qwen2_ref, ``h16=True``)
against the transformers fixture, as tests/golden/make_qwen2_fixtures.py prints it; the emulated value stands beside each constant.
The int8 operator is held to the fp64 restatement as tests/test_llm_int8_gpu.py::test_gemm_matches_fp64_restatement holds the
bias-less one (1e-6 of the result's scale in fp32, 1e-3 in fp16: the bias adds one fp32 addition), the attention kernels to
tests/llm_ops_ref.py's ATTN_TOL per query row and tests/test_lora_train_gpu.py's backward bound."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import llm_int8_ref as i8  # noqa: E402
import llm_ops_ref as opsref  # noqa: E402
import llm_train_ref as tref  # noqa: E402
import qwen2_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H16 = 2.0 ** -11

# emulated (fp16-rounded restatement vs the transformers fixture) -> bound = 4x
HIDDEN_BOUND = 4 * 3.947e-3            # last-layer hidden states of the 199 real positions
EMBED_BOUND = 4 * 1.597e-3             # mean-pooled embeddings
LOGITS_BOUND = 4 * 2.946e-3            # last-position logits
LOGPROB_BOUND = 4 * 7.570e-4           # token log-probabilities
LOSS_BOUND = 4 * 7.658e-5              # mean next-token loss with the seeded LoRA (relative)
GRAD_BOUND = 4 * 1.390e-2              # worst LoRA gradient (layer 2 k_proj B)
FIXTURE_GRAD_STORAGE = 2.0 ** -16      # the fixture's gradients keep 16 mantissa bits


@pytest.fixture(scope="module")
def fx():
    z = {**np.load(os.path.join(GOLD, "qwen2_tiny.npz")), **np.load(os.path.join(GOLD, "qwen2_tiny_train.npz"))}
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.qwen2_tiny()
    sd = make_llama_weights(cfg, int(z["seed"]))
    return z, cfg, sd, torch.from_numpy(z["ids"]), torch.from_numpy(z["lens"])


@pytest.fixture(scope="module")
def emb16(fx):
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


# ------------------------------------------------------------------------------------------------------------ 1, 2: the fp16 model
def test_fp16_model_matches_the_transformers_fixture(fx, emb16):
    z, cfg, sd, ids, lens = fx
    assert emb16.L[0]["wqkv"].bias is not None and emb16.L[0]["wqkv"].bias.shape == (896 + 2 * 128,) and emb16.L[0]["wo"].bias is None
    got = _forward(emb16, ids, lens)
    errs = {k: ref.rel_l2(got[k], z[k]) for k in got}
    bounds = {"hidden": HIDDEN_BOUND, "embedding": EMBED_BOUND, "logits_last": LOGITS_BOUND, "logprobs": LOGPROB_BOUND}
    for k, e in errs.items():
        print(f"[parity] qwen2 fp16 vs transformers: {k} rel L2 {e:.3e} (bound {bounds[k]:.3e})")
    prompts = [ids[i, :int(n)].tolist() for i, n in enumerate(lens)]
    gen = emb16.generate_greedy_batch(prompts, ref.GEN_LEN)
    for k, e in errs.items():
        assert e <= bounds[k], (k, e, bounds[k])
    for p, g, want in zip(prompts, gen, z["greedy"]):
        assert g[len(p):] == _cut(want, cfg), (len(p), g[len(p):], want.tolist())
    # the same rows one text at a time (no padding), and the second attention kernel
    one = torch.cat([emb16.embed_ids(ids[i:i + 1, :int(n)]).cpu() for i, n in enumerate(lens)])
    assert ref.rel_l2(one, z["embedding"]) <= EMBED_BOUND
    emb16.mfma_attention = False
    try:
        e_v = ref.rel_l2(emb16.embed_ids(ids, lens).cpu(), z["embedding"])
    finally:
        emb16.mfma_attention = True
    print(f"[parity] qwen2 fp16 vs transformers: embedding with the VALU attention {e_v:.3e} (bound {EMBED_BOUND:.3e})")
    assert e_v <= EMBED_BOUND


def test_what_the_code_computed_before_is_outside_the_bounds(fx):
    """The same checkpoint as it ran before this model type existed -- biases dropped, Llama-3 frequency scaling applied -- is far
    outside the bounds above.  Of the two, the dropped bias does nearly all of it; over these 130 positions the scaled frequencies
    alone move the last logits by 2.0e-2 and the hidden states by 1.7e-2 in the fp32 restatement (the slow frequencies they divide by
    32 have turned by at most 0.1 rad there), which the logits bound still sees; tests/test_qwen2_cpu.py pins the frequencies bit for bit."""
    from astts.llm.embedder import LlamaEmbedder
    z, cfg, sd, ids, lens = fx
    nobias = {k: v for k, v in sd.items() if not k.endswith(".bias")}
    for change in (dict(qkv_bias=False, rope_type="llama3"), dict(qkv_bias=False), dict(rope_type="llama3")):
        old = LlamaEmbedder(nobias if "qkv_bias" in change else sd, dataclasses.replace(cfg, **change), DEV)
        got = _forward(old, ids, lens)
        e = {k: ref.rel_l2(got[k], z[k]) for k in got}
        print(f"[parity] qwen2 with {change}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
        if "qkv_bias" in change:
            assert e["hidden"] > 4 * HIDDEN_BOUND and e["embedding"] > 4 * EMBED_BOUND and e["logits_last"] > 4 * LOGITS_BOUND, (change, e)
        else:
            assert e["logits_last"] > LOGITS_BOUND, (change, e)
    with pytest.raises(ValueError, match="bias"):                   # a bias that would be dropped is an error now
        LlamaEmbedder(sd, dataclasses.replace(cfg, qkv_bias=False), DEV)
    with pytest.raises(KeyError):                                   # and so is a missing one
        LlamaEmbedder(nobias, cfg, DEV)


def test_cached_and_recomputed_generation_agree(fx, emb16):
    """Left-padded prompts of 5, 64 and 130 tokens through the KV-cache layout (the bias reaches ``hidden_cached`` too) against the
    prompt-per-token form, row by row."""
    _, cfg, _, ids, lens = fx
    prompts = [ids[i, :int(n)].tolist() for i, n in sorted(enumerate(lens), key=lambda e: int(e[1]))]
    assert [len(p) for p in prompts] == [5, 64, 130]
    batch = emb16.generate_greedy_batch(prompts, ref.GEN_LEN)
    for p, got in zip(prompts, batch):
        assert got == emb16.generate_greedy_recompute(p, ref.GEN_LEN), (len(p), got[len(p):])
        assert got == emb16.generate_greedy(p, ref.GEN_LEN)


# ------------------------------------------------------------------------------------------------------------ 3: the int8 operator
def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("m", [1, 33, 70])
def test_i8_gemm_with_bias(m):
    from astts import ops
    from astts.llm.weights import BIAS_OUTLIERS

    k, outs, r, scaling, tau = 896, (896, 128, 128), 8, 4.0, 6.0
    n = sum(outs)
    g = torch.Generator().manual_seed(100 + m)
    parts = [(torch.randn(o, k, generator=g) * 0.04, torch.randn(r, k, generator=g) * 0.02, torch.randn(o, r, generator=g) * 0.02) for o in outs]
    bias = torch.randn(n, generator=g) * 0.5
    big = [o0 + at for o0 in (0, 896) for at in BIAS_OUTLIERS]          # +-16 in the q and the k part, as make_llama_weights sets them
    bias[big] = torch.tensor([16.0, -16.0] * (len(big) // 2))
    x = (torch.randn(m, k, generator=g)).to(torch.float16)
    for c in (11, k - 5):                                               # outlier columns in some rows
        x[::3, c] = 9.0
    seg = (torch.arange(m, dtype=torch.int32) // 40).to(DEV)            # 70 rows: two segments
    segs = int(seg.max()) + 1
    xd = x.to(DEV)
    W = ops.Int8Weight(parts, scaling, DEV, bias=bias)
    W0 = ops.Int8Weight(parts, scaling, DEV)
    Wz = ops.Int8Weight(parts, scaling, DEV, bias=torch.zeros(n))
    assert tuple(W.groups) == (896, 1024) and W0.bias is None
    want = torch.cat([i8.int8_linear(xd, *[t.to(DEV) for t in i8.quant_weight(w)], seg, tau, (a.to(DEV), b.to(DEV), scaling)) for w, a, b in parts], 1)
    assert want.dtype == torch.float64
    want_b = want + bias.double().to(DEV)
    small = torch.ones(n, dtype=torch.bool)
    small[big] = False
    res = torch.randn(m, n, generator=g).to(DEV)
    y, y16, yr = W(xd, seg, segs, tau), W(xd, seg, segs, tau, out_dtype=torch.float16), W(xd, seg, segs, tau, residual=res)
    e32, e32s, e16, e16s, er = _rel(y, want_b), _rel(y[:, small], want_b[:, small]), _rel(y16, want_b), _rel(y16[:, small], want_b[:, small]), _rel(yr, want_b + res.double())
    print(f"[parity] i8_gemm + bias m={m}: fp32 {e32:.2e} ({e32s:.2e} without the +-16 columns), fp16 {e16:.2e} ({e16s:.2e}), residual {er:.2e}")
    assert y16.dtype == torch.float16 and e32 <= 1e-6 and e32s <= 1e-6 and er <= 1e-6 and e16 <= 1e-3 and e16s <= 1e-3
    assert _rel(W0(xd, seg, segs, tau), want) <= 1e-6
    assert float((y - W0(xd, seg, segs, tau)).abs().max()) > 1.0         # the bias is there
    # no bias == an all-zero bias, bit for bit, in every float form; the raw accumulator never sees a bias
    for kw in (dict(), dict(out_dtype=torch.float16), dict(residual=res)):
        assert torch.equal(W0(xd, seg, segs, tau, **kw), Wz(xd, seg, segs, tau, **kw)), kw
    act = ops.i8_quantize_act(xd, seg, segs, tau)
    t = ops.i8_lora_down(xd, W.lora_a)
    kw = dict(t=t, lora_b=W.lora_b, r=W.r, groups=W.groups, scaling=scaling)
    assert torch.equal(ops.i8_gemm(act, W.cb, W.scb, n, **kw), ops.i8_gemm(act, W.cb, W.scb, n, bias=None, **kw))
    assert torch.equal(ops.i8_gemm(act, W.cb, W.scb, n, **kw), W0(xd, seg, segs, tau))
    assert torch.equal(ops.i8_gemm(act, W.cb, W.scb, n, bias=W.bias, **kw), y)
    acc = ops.i8_gemm(act, W.cb, W.scb, n, out_kind=ops.I8_OUT_ACC)
    assert torch.equal(acc, ops.i8_gemm(act, W.cb, W.scb, n, out_kind=ops.I8_OUT_ACC, bias=W.bias))
    assert torch.equal(acc.double(), act.ca.double() @ W.cb[:n].double().T)


# ------------------------------------------------------------------------------------------------------------ 4: adapter over a Qwen2 base
@pytest.fixture(scope="module")
def qwen_dirs(tmp_path_factory, fx):
    """A Qwen2 base directory (some input_layernorm channels of layer 0 raised so that their activations cross tau) and an r = 8
    adapter directory over it, loaded back through astts.llm.peft."""
    from astts.llm.peft import load_peft_model
    _, cfg, sd, _, _ = fx
    sd = dict(sd)
    sd["model.layers.0.input_layernorm.weight"] = sd["model.layers.0.input_layernorm.weight"].clone()
    sd["model.layers.0.input_layernorm.weight"][[5, 17, 100]] = 25.0
    root = tmp_path_factory.mktemp("qwen2")
    base = ref.write_base(str(root / "base"), cfg, sd)
    ada = ref.write_adapter(str(root / "adapter"), ref.make_lora(cfg, ref.R, 1), ref.R, ref.ALPHA, base="org/not-on-this-disk")
    state, cfg2, ad, _ = load_peft_model(ada, base)
    assert cfg2.qkv_bias and cfg2.rope_type == "default" and not cfg2.tie_embeddings and (cfg2.heads, cfg2.kv_heads) == (7, 1)
    return base, ada, state, cfg2, ad


def test_adapter_directory_over_a_qwen2_base(qwen_dirs):
    from astts.llm.embedder import LlamaEmbedder
    base, ada, state, cfg, ad = qwen_dirs
    emb = LlamaEmbedder(state, cfg, DEV, int8=True, lora=ad)
    assert emb.L[0]["wqkv"].bias is not None and emb.L[0]["wqkv"].r == 8 and emb.L[0]["wd"].bias is None
    g = torch.Generator().manual_seed(3)
    lens = [9, 14, 5, 12]
    texts = [torch.randint(3, cfg.vocab, (n,), generator=g) for n in lens]
    lin = ref.int8_linear(state, cfg, ad.pairs, ad.scaling, tau=6.0)
    one = []
    for t in texts:
        e = emb.embed_ids(t[None]).cpu()[0]
        with torch.no_grad():
            r = ref.pooled(ref.hidden(state, cfg, lin, t[None], torch.tensor([len(t)]), h16=True), [len(t)])[0]
        cos = float(torch.nn.functional.cosine_similarity(e.double(), r.double(), 0))
        print(f"[int8] qwen2_tiny: cosine to the restatement {cos:.6f}")
        assert cos >= 0.9999, cos                       # the bound of test_embedder_int8_lora_end_to_end at the tiny widths
        one.append(e)
    ids = torch.zeros(len(texts), max(lens), dtype=torch.int64)
    for i, t in enumerate(texts):
        ids[i, :len(t)] = t
    bat = emb.embed_ids(ids, torch.tensor(lens)).cpu()
    assert _rel(bat, torch.stack(one)) <= 1e-5          # right padding belongs to no segment
    nob = LlamaEmbedder({k: (torch.zeros_like(v) if k.endswith(".bias") else v) for k, v in state.items()}, cfg, DEV, int8=True, lora=ad)
    assert float(torch.nn.functional.cosine_similarity(nob.embed_ids(texts[0][None]).cpu()[0], one[0], 0)) < 0.99      # the bias matters
    # precision fp16: the LoRA merged into the fp16 weights == the fp16 model on weights merged beforehand
    f16 = LlamaEmbedder(state, cfg, DEV, lora=ad)
    pre = LlamaEmbedder(ref.merged(state, ad.pairs, ad.scaling), cfg, DEV)
    a, b = f16.embed_ids(ids, torch.tensor(lens)).cpu(), pre.embed_ids(ids, torch.tensor(lens)).cpu()
    assert torch.equal(a, b)
    with torch.no_grad():
        m16 = ref.merged(state, ad.pairs, ad.scaling)
        want = ref.pooled(ref.hidden(m16, cfg, ref.fp_linear(m16, cfg), ids, torch.tensor(lens)), lens)
    e = ref.rel_l2(a, want)
    print(f"[parity] qwen2 adapter merged to fp16 vs the fp32 restatement on merged weights: embedding {e:.3e} (bound {EMBED_BOUND:.3e})")
    assert e <= EMBED_BOUND


# ------------------------------------------------------------------------------------------------------------ 5: attention at a group of 7
G7 = ((7, 1), (14, 2))


def _attn(case, kernel="mfma"):
    """One case of llm_ops_ref through the kernel -> [B, heads, Tq, 128] on the CPU (as tests/test_llm_ops_gpu.py runs them)."""
    from astts import ops
    x = opsref.build_attn(case)
    hq, hk = case.heads * 128, case.kv_heads * 128
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)
    if case.form == "bm":
        d = x.bufs["qkv"].to(DEV)
        q, k, v = d[..., :hq], d[..., hq:hq + hk], d[..., hq + hk:]
        out = ops.attn_causal_gqa(q, k, v, case.heads, case.kv_heads, 128, i32(case.lens)) if kernel == "valu" else \
            ops.attn_gqa(q, k, v, case.heads, case.kv_heads, 128, lens=i32(case.lens))
        return out.cpu().reshape(case.b, case.tq, case.heads, 128).permute(0, 2, 1, 3)
    q, cache = x.bufs["q"].to(DEV), x.bufs["cache"].to(DEV)
    out = ops.attn_gqa(q, cache[:case.tk, :, :hk], cache[:case.tk, :, hk:], case.heads, case.kv_heads, 128, lens=i32(case.lens),
                       key_start=i32(case.key_start), pos0=case.pos0, time_major=True)
    return out.cpu().reshape(case.tq, case.b, case.heads, 128).permute(1, 2, 0, 3)


@pytest.mark.parametrize("heads,kv_heads", G7)
def test_attention_forward_at_a_group_of_7(heads, kv_heads):
    """Right-padded lens (130, 64, 5) on both kernels and the decode step (tq = 1) of those prompts left-padded in a 131-row cache."""
    bm = opsref._bm(heads, kv_heads, 130, (130, 64, 5))
    tm = opsref._tm(heads, kv_heads, 1, 131, (0, 66, 125))
    for case, kernel in ((bm, "mfma"), (bm, "valu"), (tm, "mfma")):
        got, want = _attn(case, kernel), opsref.attn_expected(case)
        assert bool(torch.isfinite(got).all())
        err, bad = opsref.row_errors(got, want)
        print(f"[parity] attention {case.name} ({kernel}): worst per-row err {float(err.max()):.2e} (bound {opsref.ATTN_TOL:.2e})")
        assert not bool(bad.any()) and float(err.max()) <= opsref.ATTN_TOL, (case.name, kernel, float(err.max()))
        # the head -> KV-head map: the reference with heads mapped modulo kv_heads is another function wherever there are 2 KV heads
        if kv_heads > 1:
            x = opsref.build_attn(case)
            wrong = opsref.attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens, mutate="kv_mod")
            assert float(opsref.row_errors(wrong, want)[0].max()) > 100 * opsref.ATTN_TOL


@pytest.mark.parametrize("heads,kv_heads", G7)
def test_attention_backward_at_a_group_of_7(heads, kv_heads):
    """train_ops.attn_gqa_bwd against fp32 autograd in both formulations, with the bound of tests/test_lora_train_gpu.py: the group
    loop of the dK / dV kernel runs 7 query heads per KV head."""
    from astts import train_ops as tops
    g = torch.Generator().manual_seed(70 + heads)
    b, t, d, lens = 3, 130, 128, (130, 64, 5)
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
    got = tops.attn_gqa_bwd(qkv.to(DEV), dout.to(DEV), heads, kv_heads, d, ln.to(DEV, torch.int32)).float().cpu()
    assert torch.isfinite(got).all()
    for i in range(b):
        assert not got[i, lens[i]:].any()
    cuts = (0, heads * d, (heads + kv_heads) * d, w)
    for name, lo, hi in zip(("dq", "dk", "dv"), cuts[:-1], cuts[1:]):
        bound = 4 * (tref.rel_l2(emu[..., lo:hi], want[..., lo:hi]) + 2 * H16)
        e1, e2 = tref.rel_l2(got[..., lo:hi], want[..., lo:hi]), tref.rel_l2(got[..., lo:hi], want2[..., lo:hi])
        print(f"attn_bwd heads={heads}/{kv_heads} {name}: rel L2 {e1:.2e} / {e2:.2e} (bound {bound:.2e})")
        assert e1 <= bound and e2 <= bound, (name, e1, e2, bound)


# ------------------------------------------------------------------------------------------------------------ 6: training
def _trainer(cfg, sd, lora, r, alpha, **kw):
    from astts.llm.peft import PROJ, LoraAdapter
    from astts.llm.train import LoraTrainer
    ad = LoraAdapter(r=r, lora_alpha=alpha, use_rslora=False, targets=tuple(PROJ), base_model_name_or_path="", pairs=dict(lora))
    return LoraTrainer(sd, cfg, DEV, adapter=ad, lr=1e-3, total_steps=1, warmup_ratio=0.0, loss_scale=1.0, **kw)


def test_training_loss_and_gradients_match_the_fixture(fx):
    z, cfg, sd, ids, lens = fx
    lora = ref.make_lora(cfg, int(z["r"]), int(z["lora_seed"]))
    tr = _trainer(cfg, sd, lora, int(z["r"]), float(z["lora_alpha"]))
    assert tr.dec.L[0]["wqkv"].bias is not None and tr.WT[0]["wqkv"].bias is None      # the frozen bias: forward only
    loss = tr.accumulate([(ids, lens)])
    want = float(z["loss"])
    print(f"[parity] qwen2 training: loss {loss:.6f} vs {want:.6f} rel {abs(loss - want) / want:.2e} (bound {LOSS_BOUND:.2e})")
    worst, where = 0.0, None
    grads = {k: v.detach().cpu().clone() for k, v in tr.named_grads().items()}
    for (i, p, h), gr in grads.items():
        e = ref.rel_l2(gr, z[f"grad.{i}.{p}.{h}"])
        if e > worst:
            worst, where = e, (i, p, h)
    print(f"[parity] qwen2 training: worst LoRA gradient rel L2 {worst:.3e} at {where} (bound {GRAD_BOUND:.3e})")
    assert abs(loss - want) <= LOSS_BOUND * want
    assert len(grads) == 2 * 7 * cfg.layers and worst <= GRAD_BOUND + FIXTURE_GRAD_STORAGE, (where, worst)


def test_training_step_repeats_and_the_adapter_reloads(fx, tmp_path):
    """Two identical steps from the same state give the same bits; the saved adapter, loaded over the Qwen2 base through
    load_peft_model, reproduces the trainer's own forward loss in the merged-fp16 precision and loads in the int8 one."""
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.peft import load_peft_model
    from astts.llm.weights import load_llama_weights
    z, cfg, sd, ids, lens = fx
    lora = ref.make_lora(cfg, int(z["r"]), int(z["lora_seed"]))
    base = ref.write_base(str(tmp_path / "base"), cfg, sd)
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
    assert cfg2.qkv_bias and cfg2.model_type == "qwen2"
    emb = LlamaEmbedder(state, cfg2, DEV, lora=ad)
    count = int((lens - 1).sum())
    inf = -float(emb.token_logprobs(ids.to(DEV), lens.to(DEV, torch.int32)).sum()) / count
    print(f"[parity] qwen2 round trip: trainer {own:.6f} inference {inf:.6f} rel {abs(own - inf) / own:.2e} (bound {LOSS_BOUND:.2e})")
    assert abs(own - inf) <= LOSS_BOUND * own           # the two roundings of the same LoRA: a part of what LOSS_BOUND is made of
    emb8 = LlamaEmbedder(state, cfg2, DEV, int8=True, lora=ad)
    inf8 = -float(emb8.token_logprobs(ids.to(DEV), lens.to(DEV, torch.int32)).sum()) / count
    print(f"[parity] qwen2 round trip: int8 + LoRA inference loss {inf8:.6f}")
    assert np.isfinite(inf8) and emb8.L[0]["wqkv"].bias is not None and emb8.L[0]["wqkv"].r == 8      # (its numerics: test 4)


# ------------------------------------------------------------------------------------------------------------ 7: the CLIs' loader
def test_cli_load_and_bank_dimension_message(qwen_dirs, tmp_path):
    from astts.cli import search_json, search_milvus
    base, ada, state, cfg, ad = qwen_dirs
    emb = search_milvus.load_embedder(base)                                   # a merged checkpoint directory: its own config.json
    assert emb.cfg.model_type == "qwen2" and emb.cfg.qkv_bias and emb.cfg.hidden == 896 and not emb.int8
    q = emb.combined_embedding("neutral", "A pragmatic and thoughtful person.")
    assert q.shape == (2 * 896,) and q.dtype == np.float32 and bool(np.isfinite(q).all())
    emb8 = search_milvus.load_embedder(ada, base_model_path=base)             # an adapter directory: int8 + LoRA
    assert emb8.int8 and emb8.cfg.qkv_bias and emb8.L[0]["wqkv"].bias is not None
    assert emb8.get_embedding("neutral").shape == (896,)
    db = os.path.join(GOLD, "milvus_demo.db")                                 # the shipped bank: 6144-d
    args = search_milvus.build_parser().parse_args(["--db_path", db, "--model_path", base, "--top_k", "3"])
    with pytest.raises(SystemExit, match=r"1792 dimensions.*896.*6144-dimensional"):
        search_milvus.main(args, embedder=emb)
    inp = tmp_path / "in.jsonl"
    inp.write_text(json.dumps({"zh_text": "Fine, whatever.", "speaker": "JOHN"}) + "\n")
    with pytest.raises(SystemExit, match=r"1792 dimensions.*6144-dimensional"):
        search_json.main(search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db]), embedder=emb)
