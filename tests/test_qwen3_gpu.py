"""The Qwen3 track on the GPU (DESIGN.md section 2 "Qwen3"): the fused q / k norm + RoPE kernel and its transpose against fp64
restatements, and the decoder with them in fp16, in LLM.int8 + LoRA and under LoRA fine-tuning, against tests/golden/qwen3_tiny.npz /
qwen3_tiny_train.npz (transformers' Qwen3ForCausalLM, fp32, CPU) and the restatements of tests/qwen3_ref.py.

Bounds.  The forward operator per element: 2^-11 |want| + head_dim 2^-24 max|want| over the head (one fp16 rounding of an fp32
computation).  The backward operator: relative L2 per tensor, 4 x the error of the fp16-rounded fp32 CPU restatement against fp64,
computed here.  Every whole-model bound is 4 x the error of the fp16-rounded CPU restatement (qwen3_ref, ``h16=True``) against the
transformers fixture, as tests/golden/make_qwen3_fixtures.py prints it; the emulated value stands beside each constant.  LLM.int8 + LoRA:
the cosine bound of tests/test_llm_int8_gpu.py::test_embedder_int8_lora_end_to_end."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qwen3_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# emulated (fp16-rounded restatement vs the transformers fixture) -> bound = 4x; (qwen3_tiny, qwen3_tiny_untied)
HIDDEN_BOUND = {"qwen3_tiny": 4 * 4.328e-3, "qwen3_tiny_untied": 4 * 2.042e-3}      # last-layer hidden states (199 positions; untied: the 5-token row)
EMBED_BOUND = {"qwen3_tiny": 4 * 1.774e-3, "qwen3_tiny_untied": 4 * 2.002e-3}       # mean-pooled embeddings
LOGITS_BOUND = {"qwen3_tiny": 4 * 4.014e-3, "qwen3_tiny_untied": 4 * 3.604e-3}      # last-position logits
LOGPROB_BOUND = {"qwen3_tiny": 4 * 6.668e-4, "qwen3_tiny_untied": 4 * 9.626e-4}     # token log-probabilities
LOSS_BOUND = 4 * 1.017e-5              # mean next-token loss with the seeded LoRA (relative)
GRAD_BOUND = 4 * 2.537e-2              # worst LoRA gradient (layer 2 q_proj B)
FIXTURE_GRAD_STORAGE = 2.0 ** -16      # the fixture's gradients keep 16 mantissa bits
BOUNDS = {"hidden": HIDDEN_BOUND, "embedding": EMBED_BOUND, "logits_last": LOGITS_BOUND, "logprobs": LOGPROB_BOUND}


# ------------------------------------------------------------------------------------------------------------ 1, 2: the operators
HEADS = ((8, 4), (7, 1), (5, 1), (1, 1))          # an odd head total leaves a wave half-filled (16 heads per wave at 64, 8 at 128)
BT = ((1, 1), (2, 5), (3, 130))
PAD = 24                                          # ld = the q | k | v width + 24 halfs


def _norm_weights(hd: int, g):
    from astts.llm.weights import QK_NORM_OUTLIERS
    ws = []
    for _ in range(2):
        w = 1.0 + 0.1 * torch.randn(hd, generator=g)
        for at, val in QK_NORM_OUTLIERS:              # 8.0, 0.02 and an exact 0.0
            w[at % hd] = val
        ws.append(w)
    assert float(ws[0].min()) == 0.0 and float(ws[0].max()) == 8.0
    return ws


def _tables(n: int, hd: int):
    inv = 1.0 / (1e6 ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))
    fr = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous(), fr.sin().contiguous()


def _op_case(hd, heads, kv, b, t, time_major, seed):
    """x fp16 [b, t, ld] (or [t, b, ld]) with q | k | v | padding all random, one all-zero row (a zero head where there is one row only),
    the position of every row [rows...] and the norm weights."""
    g = torch.Generator().manual_seed(seed)
    wqk, ld = (heads + kv) * hd, (heads + 2 * kv) * hd + PAD
    shape = (t, b, ld) if time_major else (b, t, ld)
    x = (torch.randn(*shape, generator=g) * torch.rand(*shape[:2], 1, generator=g).mul(3).exp()).half()     # row scales 1 .. 20
    if b * t > 1:
        x[-1, -1, :] = 0.0
    else:
        x[0, 0, wqk - hd:wqk] = 0.0
    qw, kw = _norm_weights(hd, g)
    if time_major:
        pos0 = 2
        shift = torch.tensor([(3 * i + 1) % (t + 2) for i in range(b)], dtype=torch.int32)           # differs per row; some beyond pos0 + ti
        pos = (pos0 + torch.arange(t)[:, None] - shift[None, :].long()).clamp(min=0)                 # [t, b]
    else:
        pos0, shift = 3, None
        pos = (pos0 + torch.arange(t))[None, :].expand(b, t)
    return x, qw, kw, pos0, shift, pos, wqk


def _fwd_want(x, qw, kw, cos, sin, pos, hd, heads, kv, eps):
    """fp64 restatement on the fp16 inputs and the fp32 tables and weights -> [.., .., heads + kv, hd]."""
    wqk = (heads + kv) * hd
    xh = x[..., :wqk].double().reshape(*x.shape[:2], heads + kv, hd)
    c, s = cos.double()[pos], sin.double()[pos]
    return torch.cat([ref.qknorm_rope(xh[..., :heads, :], qw.double(), c, s, eps), ref.qknorm_rope(xh[..., heads:, :], kw.double(), c, s, eps)], -2)


@pytest.mark.parametrize("b,t", BT)
@pytest.mark.parametrize("heads,kv", HEADS)
@pytest.mark.parametrize("hd", [64, 128])
def test_qknorm_rope_forward_against_fp64(hd, heads, kv, b, t):
    from astts import ops
    eps = 1e-6
    cos, sin = _tables(t + 8, hd)
    cd, sn = cos.to(DEV), sin.to(DEV)
    for time_major in (False, True):
        x, qw, kw, pos0, shift, pos, wqk = _op_case(hd, heads, kv, b, t, time_major, 1000 * hd + 10 * heads + t + int(time_major))
        want = _fwd_want(x, qw, kw, cos, sin, pos, hd, heads, kv, eps)
        runs = []
        for _ in range(2):
            xd = x.to(DEV)
            out = ops.qknorm_rope_(xd, cd, sn, qw.to(DEV), kw.to(DEV), heads, kv, hd, eps, pos0=pos0,
                                   shift=None if shift is None else shift.to(DEV), time_major=time_major)
            assert out is xd
            runs.append(xd.cpu())
        got = runs[0]
        assert torch.equal(runs[0], runs[1]), "two runs are bit-equal"
        assert torch.equal(got[..., wqk:], x[..., wqk:]), "v and the padding are bit-identical to before"
        assert bool(torch.isfinite(got.float()).all()), "no NaN"
        gh = got[..., :wqk].double().reshape(*x.shape[:2], heads + kv, hd)
        bound = 2.0 ** -11 * want.abs() + hd * 2.0 ** -24 * want.abs().amax(-1, keepdim=True)
        over = ((gh - want).abs() - bound).max()
        worst = float(((gh - want).abs() / bound.clamp_min(1e-300)).max())
        print(f"[parity] qknorm_rope hd={hd} heads={heads}/{kv} b={b} t={t} {'time-major' if time_major else 'batch-major'}: worst error "
              f"{worst:.3f} of the bound")
        assert float(over) <= 0.0, (time_major, worst)
        zero = (x[..., :wqk].reshape(*x.shape[:2], heads + kv, hd) == 0).all(-1)
        assert bool(zero.any()) and not bool(gh[zero].any()), "zeros in, zeros out"
        assert float((gh - xh_plain(x, wqk, heads, kv, hd)).abs().max()) > 0.1, "the operator did something"


def xh_plain(x, wqk, heads, kv, hd):
    return x[..., :wqk].double().reshape(*x.shape[:2], heads + kv, hd)


@pytest.mark.parametrize("b,t", BT)
@pytest.mark.parametrize("heads,kv", HEADS)
@pytest.mark.parametrize("hd", [64, 128])
def test_qknorm_rope_backward_against_fp64_autograd(hd, heads, kv, b, t):
    """dx of the restatement by fp64 autograd; the bound is 4 x the error of the same restatement run in fp32 with its result rounded
    to fp16 (what the kernel does), per tensor (dq, dk).  dv and the padding of dqkv are not touched."""
    from astts import train_ops as tops
    eps, pos0 = 1e-6, 3
    g = torch.Generator().manual_seed(7000 + 100 * hd + 10 * heads + t)
    wqk, ld = (heads + kv) * hd, (heads + 2 * kv) * hd + PAD
    cos, sin = _tables(t + 8, hd)
    pos = (pos0 + torch.arange(t))[None, :].expand(b, t)
    xpre = (torch.randn(b, t, wqk, generator=g) * torch.rand(b, t, 1, generator=g).mul(3).exp()).half()
    dy = torch.randn(b, t, ld, generator=g).half()
    if b * t > 1:                                          # a pad position: zeros in the kept q | k and in the gradient that arrives
        xpre[-1, -1] = 0.0
        dy[-1, -1] = 0.0
    qw, kw = _norm_weights(hd, g)

    def cpu(dt, h16):
        x = xpre.to(dt).requires_grad_(True)
        xh = x.reshape(b, t, heads + kv, hd)
        c, s = cos.to(dt)[pos], sin.to(dt)[pos]
        y = torch.cat([ref.qknorm_rope(xh[..., :heads, :], qw.to(dt), c, s, eps), ref.qknorm_rope(xh[..., heads:, :], kw.to(dt), c, s, eps)], -2)
        y.backward(dy[..., :wqk].to(dt).reshape(b, t, heads + kv, hd))
        return (x.grad.half() if h16 else x.grad).double()

    want, emu = cpu(torch.float64, False), cpu(torch.float32, True)
    runs = []
    for _ in range(2):
        d = dy.to(DEV)
        assert tops.qknorm_rope_bwd_(d, xpre.to(DEV), cos.to(DEV), sin.to(DEV), qw.to(DEV), kw.to(DEV), heads, kv, hd, eps, pos0=pos0) is d
        runs.append(d.cpu())
    got = runs[0]
    assert torch.equal(runs[0], runs[1]), "two runs are bit-equal"
    assert torch.equal(got[..., wqk:], dy[..., wqk:]), "dv and the padding are not touched"
    assert bool(torch.isfinite(got.float()).all()), "the exact-0 weight entry gives a finite dx"
    if b * t > 1:
        assert not bool(got[-1, -1, :wqk].any())
    for name, lo, hi in (("dq", 0, heads * hd), ("dk", heads * hd, wqk)):
        bound = 4 * ref.rel_l2(emu[..., lo:hi], want[..., lo:hi])
        e = ref.rel_l2(got[..., lo:hi].double(), want[..., lo:hi])
        print(f"[parity] qknorm_rope_bwd hd={hd} heads={heads}/{kv} b={b} t={t} {name}: rel L2 {e:.2e} (bound {bound:.2e})")
        assert e <= bound, (name, e, bound)
    # the columns of the zero weight entry: dx there is -xh r mean(g xh), not zero and not NaN
    from astts.llm.weights import QK_NORM_OUTLIERS
    z = next(at % hd for at, val in QK_NORM_OUTLIERS if val == 0.0)
    col = got[..., :wqk].double().reshape(b, t, heads + kv, hd)[..., z]
    wcol = want.reshape(b, t, heads + kv, hd)[..., z]
    assert bool(col.any()) and float((col - wcol).abs().max()) <= 2.0 ** -10 * float(wcol.abs().max()) + 1e-6


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from astts import _lib, ops
    cos, sin = (v.to(DEV) for v in _tables(8, 32))
    w = torch.ones(32, device=DEV)
    with pytest.raises(_lib.AsttsError, match="head_dim=32") as e:
        ops.qknorm_rope_(torch.zeros(1, 4, 96, dtype=torch.float16, device=DEV), cos, sin, w, w, 2, 1, 32, 1e-6)
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ 3 .. 5: the fp16 model
@pytest.fixture(scope="module")
def fixture_file():
    return {**np.load(os.path.join(GOLD, "qwen3_tiny.npz")), **np.load(os.path.join(GOLD, "qwen3_tiny_train.npz"))}


@pytest.fixture(scope="module", params=ref.SHAPES)
def fx(request, fixture_file):
    """(the shape's record out of the file, shape, seeded weights, ids, lens, name)"""
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    z = fixture_file
    cfg = getattr(LlamaShape, request.param)()
    pre = "" if cfg.tie_embeddings else "untied."
    rec = {k: z[pre + k] for k in ("hidden", "embedding", "logits_last", "logprobs", "greedy")}
    return rec, cfg, make_llama_weights(cfg, int(z["seed"])), torch.from_numpy(z["ids"]), torch.from_numpy(z["lens"]), request.param


@pytest.fixture(scope="module")
def emb16(fx):
    from astts.llm.embedder import LlamaEmbedder
    _, cfg, sd, _, _, _ = fx
    return LlamaEmbedder(sd, cfg, DEV)


def _forward(emb, ids, lens):
    """What the fixture records of one forward pass, from the GPU model (the untied shape: the hidden states of the last row only)."""
    from astts import ops
    hf = emb.hidden(ids, lens.to(DEV, torch.int32))
    last = torch.stack([hf[i, int(n) - 1] for i, n in enumerate(lens)]).contiguous()
    rows = range(len(lens)) if emb.cfg.tie_embeddings else [len(lens) - 1]
    return {"hidden": torch.cat([hf[i, :int(lens[i])] for i in rows]).cpu(), "embedding": emb.embed_ids(ids, lens).cpu(),
            "logits_last": ops.linear(last, emb.head).cpu(), "logprobs": emb.token_logprobs(ids, lens).cpu()}


def _cut(tokens, cfg):
    out = []
    for t in tokens:
        out.append(int(t))
        if int(t) == cfg.eos_token_id:
            break
    return out


def test_fp16_model_matches_the_transformers_fixture(fx, emb16):
    rec, cfg, sd, ids, lens, name = fx
    assert emb16.L[0]["qn"].shape == (128,) and emb16.L[0]["kn"].dtype == torch.float32 and emb16.L[0]["wqkv"].bias is None
    assert emb16.L[0]["wqkv"].n == 1024 + 2 * 512 and emb16.L[0]["wqkv"].cin == 640 and emb16.L[0]["wo"].cin == 1024        # hq is not hidden
    got = _forward(emb16, ids, lens)
    errs = {k: ref.rel_l2(got[k], rec[k]) for k in got}
    for k, e in errs.items():
        print(f"[parity] {name} fp16 vs transformers: {k} rel L2 {e:.3e} (bound {BOUNDS[k][name]:.3e})")
    prompts = [ids[i, :int(n)].tolist() for i, n in enumerate(lens)]
    gen = emb16.generate_greedy_batch(prompts, ref.GEN_LEN)
    for k, e in errs.items():
        assert e <= BOUNDS[k][name], (k, e, BOUNDS[k][name])
    for p, g, want in zip(prompts, gen, rec["greedy"]):
        assert g[len(p):] == _cut(want, cfg), (len(p), g[len(p):], want.tolist())
    # the same rows one text at a time (no padding), and the second attention kernel
    one = torch.cat([emb16.embed_ids(ids[i:i + 1, :int(n)]).cpu() for i, n in enumerate(lens)])
    assert ref.rel_l2(one, rec["embedding"]) <= EMBED_BOUND[name]
    emb16.mfma_attention = False
    try:
        e_v = ref.rel_l2(emb16.embed_ids(ids, lens).cpu(), rec["embedding"])
    finally:
        emb16.mfma_attention = True
    print(f"[parity] {name} fp16 vs transformers: embedding with the VALU attention {e_v:.3e} (bound {EMBED_BOUND[name]:.3e})")
    assert e_v <= EMBED_BOUND[name]


def test_what_the_code_computed_before_is_outside_the_bounds(fx):
    """The same checkpoint with qk_norm=False and the norm tensors removed -- what any earlier code would have computed had it accepted
    the model type -- lies beyond 4 x every bound above; and the decoder raises on norm weights it would drop and on missing ones."""
    from astts.llm.embedder import LlamaEmbedder
    rec, cfg, sd, ids, lens, name = fx
    bare = {k: v for k, v in sd.items() if "q_norm" not in k and "k_norm" not in k}
    assert len(bare) == len(sd) - 2 * cfg.layers
    old = LlamaEmbedder(bare, dataclasses.replace(cfg, qk_norm=False), DEV)
    assert "qn" not in old.L[0]
    got = _forward(old, ids, lens)
    for k in got:
        e = ref.rel_l2(got[k], rec[k])
        print(f"[parity] {name} without the q / k norm: {k} rel L2 {e:.3e} (4 x bound {4 * BOUNDS[k][name]:.3e})")
        assert e > 4 * BOUNDS[k][name], (k, e)
    with pytest.raises(ValueError, match="q / k norm weights"):
        LlamaEmbedder(sd, dataclasses.replace(cfg, qk_norm=False), DEV)
    with pytest.raises(ValueError, match="lacks .*norm weights"):
        LlamaEmbedder(bare, cfg, DEV)
    with pytest.raises(ValueError, match="lacks .*norm weights"):           # one layer's k_norm only
        LlamaEmbedder({k: v for k, v in sd.items() if k != "model.layers.1.self_attn.k_norm.weight"}, cfg, DEV)


def test_cached_and_recomputed_generation_agree(fx, emb16):
    """Left-padded prompts of 5, 64 and 130 tokens through the KV-cache layout (the time-major form of the fused kernel: ``shift`` differs
    per row) against the prompt-per-token form, row by row."""
    _, cfg, _, ids, lens, _ = fx
    prompts = [ids[i, :int(n)].tolist() for i, n in sorted(enumerate(lens), key=lambda e: int(e[1]))]
    assert [len(p) for p in prompts] == [5, 64, 130]
    batch = emb16.generate_greedy_batch(prompts, ref.GEN_LEN)
    for p, got in zip(prompts, batch):
        assert got == emb16.generate_greedy_recompute(p, ref.GEN_LEN), (len(p), got[len(p):])
        assert got == emb16.generate_greedy(p, ref.GEN_LEN)


# ------------------------------------------------------------------------------------------------------------ 6: adapter over a Qwen3 base
def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def tied(fixture_file):
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    z = fixture_file
    cfg = LlamaShape.qwen3_tiny()
    return z, cfg, make_llama_weights(cfg, int(z["seed"])), torch.from_numpy(z["ids"]), torch.from_numpy(z["lens"])


@pytest.fixture(scope="module")
def qwen_dirs(tmp_path_factory, tied):
    """A Qwen3 base directory (some input_layernorm channels of layer 0 raised so that their activations cross tau) and an r = 8
    adapter directory over it, loaded back through astts.llm.peft."""
    from astts.llm.peft import load_peft_model
    _, cfg, sd, _, _ = tied
    sd = dict(sd)
    sd["model.layers.0.input_layernorm.weight"] = sd["model.layers.0.input_layernorm.weight"].clone()
    sd["model.layers.0.input_layernorm.weight"][[5, 17, 100]] = 25.0
    root = tmp_path_factory.mktemp("qwen3")
    base = ref.write_base(str(root / "base"), cfg, sd)
    ada = ref.write_adapter(str(root / "adapter"), ref.make_lora(cfg, ref.R, 1), ref.R, ref.ALPHA, base="org/not-on-this-disk")
    state, cfg2, ad, _ = load_peft_model(ada, base)
    assert cfg2.qk_norm and not cfg2.qkv_bias and cfg2.rope_type == "default" and cfg2.tie_embeddings
    assert (cfg2.heads, cfg2.kv_heads, cfg2.head_dim, cfg2.hidden) == (8, 4, 128, 640)
    return base, ada, state, cfg2, ad


def test_adapter_directory_over_a_qwen3_base(qwen_dirs):
    from astts.llm.embedder import LlamaEmbedder
    base, ada, state, cfg, ad = qwen_dirs
    emb = LlamaEmbedder(state, cfg, DEV, int8=True, lora=ad)
    assert emb.L[0]["wqkv"].r == 8 and emb.L[0]["wqkv"].bias is None and emb.L[0]["qn"].shape == (128,)
    g = torch.Generator().manual_seed(3)
    lens = [9, 14, 5, 12]
    texts = [torch.randint(3, cfg.vocab, (n,), generator=g) for n in lens]
    lin = ref.int8_linear(state, cfg, ad.pairs, ad.scaling, tau=6.0)
    one = []
    for t in texts:
        e = emb.embed_ids(t[None]).cpu()[0]
        with torch.no_grad():
            r = ref.pooled(ref.hidden(state, cfg, lin, t[None], torch.tensor([len(t)]), h16=True), [len(t)])[0]
            r0 = ref.pooled(ref.hidden(state, cfg, lin, t[None], torch.tensor([len(t)]), h16=True, qk_norm=False), [len(t)])[0]
        cos = float(torch.nn.functional.cosine_similarity(e.double(), r.double(), 0))
        cos0 = float(torch.nn.functional.cosine_similarity(e.double(), r0.double(), 0))
        print(f"[int8] qwen3_tiny: cosine to the restatement {cos:.6f} (to the one without the norm {cos0:.4f})")
        assert cos >= 0.9999, cos                       # the bound of test_embedder_int8_lora_end_to_end at the tiny widths
        assert cos0 < 0.99, cos0                        # the norm matters under int8 too
        one.append(e)
    ids = torch.zeros(len(texts), max(lens), dtype=torch.int64)
    for i, t in enumerate(texts):
        ids[i, :len(t)] = t
    bat = emb.embed_ids(ids, torch.tensor(lens)).cpu()
    assert _rel(bat, torch.stack(one)) <= 1e-5          # right padding belongs to no segment
    # precision fp16: the LoRA merged into the fp16 weights == the fp16 model on weights merged beforehand
    f16 = LlamaEmbedder(state, cfg, DEV, lora=ad)
    pre = LlamaEmbedder(ref.merged(state, ad.pairs, ad.scaling), cfg, DEV)
    a, b = f16.embed_ids(ids, torch.tensor(lens)).cpu(), pre.embed_ids(ids, torch.tensor(lens)).cpu()
    assert torch.equal(a, b)
    with torch.no_grad():
        m16 = ref.merged(state, ad.pairs, ad.scaling)
        want = ref.pooled(ref.hidden(m16, cfg, ref.fp_linear(m16, cfg), ids, torch.tensor(lens)), lens)
    e = ref.rel_l2(a, want)
    print(f"[parity] qwen3 adapter merged to fp16 vs the fp32 restatement on merged weights: embedding {e:.3e} (bound {EMBED_BOUND['qwen3_tiny']:.3e})")
    assert e <= EMBED_BOUND["qwen3_tiny"]


# ------------------------------------------------------------------------------------------------------------ 7: training
def _trainer(cfg, sd, lora, r, alpha, **kw):
    from astts.llm.peft import PROJ, LoraAdapter
    from astts.llm.train import LoraTrainer
    ad = LoraAdapter(r=r, lora_alpha=alpha, use_rslora=False, targets=tuple(PROJ), base_model_name_or_path="", pairs=dict(lora))
    return LoraTrainer(sd, cfg, DEV, adapter=ad, lr=1e-3, total_steps=1, warmup_ratio=0.0, loss_scale=1.0, **kw)


def test_training_loss_and_gradients_match_the_fixture(tied):
    z, cfg, sd, ids, lens = tied
    lora = ref.make_lora(cfg, int(z["r"]), int(z["lora_seed"]))
    tr = _trainer(cfg, sd, lora, int(z["r"]), float(z["lora_alpha"]))
    assert tr.dec.L[0]["qn"].shape == (128,) and tr.WT[0]["wqkv"].cin == 2048 and tr.WT[0]["wo"].n == 1024       # dX = dY W at hq != hidden
    loss = tr.accumulate([(ids, lens)])
    want = float(z["loss"])
    print(f"[parity] qwen3 training: loss {loss:.6f} vs {want:.6f} rel {abs(loss - want) / want:.2e} (bound {LOSS_BOUND:.2e})")
    worst, where = 0.0, None
    grads = {k: v.detach().cpu().clone() for k, v in tr.named_grads().items()}
    for (i, p, h), gr in grads.items():
        e = ref.rel_l2(gr, z[f"grad.{i}.{p}.{h}"])
        if e > worst:
            worst, where = e, (i, p, h)
    print(f"[parity] qwen3 training: worst LoRA gradient rel L2 {worst:.3e} at {where} (bound {GRAD_BOUND:.3e})")
    assert abs(loss - want) <= LOSS_BOUND * want
    assert len(grads) == 2 * 7 * cfg.layers and worst <= GRAD_BOUND + FIXTURE_GRAD_STORAGE, (where, worst)


def _unpacked(pw) -> torch.Tensor:
    return pw.data[:pw.n, 0, :pw.cin].float().cpu()


def test_training_step_repeats_adapter_reloads_and_eval_model_scores(tied, tmp_path):
    """Two identical steps from the same state give the same bits; the saved adapter, loaded over the Qwen3 base through load_peft_model,
    reproduces the trainer's own forward loss in the merged-fp16 precision; eval_model() carries the norm tensors and scores exactly as a
    fresh decoder built from its merged weights."""
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.peft import load_peft_model
    from astts.llm.weights import load_llama_weights
    z, cfg, sd, ids, lens = tied
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
    assert cfg2.qk_norm and cfg2.model_type == "qwen3" and cfg2.head_dim == 128
    emb = LlamaEmbedder(state, cfg2, DEV, lora=ad)
    count = int((lens - 1).sum())
    dl, dn = ids.to(DEV), lens.to(DEV, torch.int32)
    inf = -float(emb.token_logprobs(dl, dn).sum()) / count
    print(f"[parity] qwen3 round trip: trainer {own:.6f} inference {inf:.6f} rel {abs(own - inf) / own:.2e} (bound {LOSS_BOUND:.2e})")
    assert abs(own - inf) <= LOSS_BOUND * own           # the two roundings of the same LoRA: a part of what LOSS_BOUND is made of
    ev = tr.eval_model()
    assert all(E["qn"] is L["qn"] and E["kn"] is L["kn"] for E, L in zip(ev.L, tr.dec.L))
    merged = dict(sd16)
    for i, E in enumerate(ev.L):
        q, k, v = _unpacked(E["wqkv"]).split([1024, 512, 512])
        gate, up = _unpacked(E["wgu"]).split([cfg.ffn, cfg.ffn])
        for nm, w in (("self_attn.q_proj", q), ("self_attn.k_proj", k), ("self_attn.v_proj", v), ("self_attn.o_proj", _unpacked(E["wo"])),
                      ("mlp.gate_proj", gate), ("mlp.up_proj", up), ("mlp.down_proj", _unpacked(E["wd"]))):
            assert merged[f"model.layers.{i}.{nm}.weight"].shape == w.shape
            merged[f"model.layers.{i}.{nm}.weight"] = w
    fresh = LlamaEmbedder(merged, cfg, DEV)
    a, b = ev.token_logprobs(dl, dn), fresh.token_logprobs(dl, dn)
    assert torch.equal(a, b) and bool(a.any())
    assert abs(-float(a.sum()) / count - own) <= LOSS_BOUND * own


# ------------------------------------------------------------------------------------------------------------ 8: the CLIs' loader
def test_cli_loads_a_qwen3_directory_and_refusals_name_their_key(qwen_dirs, tied, tmp_path):
    from astts.cli import search_json, search_milvus
    from astts.llm.peft import ConfigError
    base, ada, state, cfg, ad = qwen_dirs
    emb = search_milvus.load_embedder(base)                                   # a merged checkpoint directory: its own config.json
    assert emb.cfg.model_type == "qwen3" and emb.cfg.qk_norm and emb.cfg.hidden == 640 and emb.cfg.head_dim == 128 and not emb.int8
    q = emb.combined_embedding("neutral", "A pragmatic and thoughtful person.")
    assert q.shape == (2 * 640,) and q.dtype == np.float32 and bool(np.isfinite(q).all())
    emb8 = search_milvus.load_embedder(ada, base_model_path=base)             # an adapter directory: int8 + LoRA
    assert emb8.int8 and emb8.cfg.qk_norm and "qn" in emb8.L[0]
    assert emb8.get_embedding("neutral").shape == (640,)
    db = os.path.join(GOLD, "milvus_demo.db")                                 # the shipped bank: 6144-d
    inp = tmp_path / "in.jsonl"
    inp.write_text(json.dumps({"zh_text": "Fine, whatever.", "speaker": "JOHN"}) + "\n")
    # search_json --model_path <qwen3 dir>: loads the directory itself and gets as far as the bank's dimension
    with pytest.raises(SystemExit, match=r"1280 dimensions.*640.*6144-dimensional"):
        search_json.main(search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db, "--model_path", base]))
    _, cfg0, sd, _, _ = tied
    for over, key in ((dict(layer_types=["full_attention", "sliding_attention", "full_attention"]), "layer_types"),
                      (dict(use_sliding_window=True), "use_sliding_window"), (dict(model_type="qwen3_moe"), "model_type"),
                      (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), "rope_scaling")):
        bad = ref.write_base(str(tmp_path / ("bad_" + key)), cfg0, sd, config={**ref.config_json(cfg0), **over})
        with pytest.raises(ConfigError, match=key):
            search_json.main(search_json.build_parser().parse_args(["--input_json", str(inp), "--db_path", db, "--model_path", bad]))
