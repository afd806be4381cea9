"""GPU tests of LoRA fine-tuning (astts.train_ops kernels, astts.llm.train.LoraTrainer): every kernel against CPU fp32 autograd on
the same fp16-rounded inputs, the whole model against tests/golden/lora_train_kats.npz (transformers, fp32).

Bounds.  Relative L2 error per tensor.  The whole-model bounds are 4x the error of the CPU restatement run with fp16 rounding at the
points where the GPU path holds fp16 (tests/llm_train_ref.py, ``h16=True``) against its fp32 run -- the factor covers accumulation
order and exp differences; both numbers stand beside each constant and in DESIGN.md section 2.  The kernel bounds come from the
number formats and are derived where they are set."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import llm_train_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H16 = 2.0 ** -11                       # fp16 rounding, relative

# emulated (h16 restatement vs fp32) -> bound = 4x
TINY_LOSS_BOUND = 4 * 5.6e-6           # loss of the fixture batch: emulated 5.6e-6 relative
TINY_GRAD_BOUND = 4 * 1.82e-3          # worst LoRA gradient (layer 2 k_proj A): emulated 1.82e-3
TINY_TRAJ_BOUND = 4 * 3.4e-5           # worst loss of the 3-step trajectory (the last): emulated 3.3e-5 (+ the loss's own 5.6e-6 at step 0)
TINY_DELTA_BOUND = 4 * 2.32e-2 + 2.5e-4   # worst parameter change after 3 steps (layer 0 o_proj A): emulated 2.32e-2; + the fixture's fp16 storage
WIDE_GRAD_BOUND = 4 * 6.33e-3          # worst gradient of the one-layer real-width model (down_proj B): emulated 6.33e-3
FIXTURE_GRAD_STORAGE = 2.0 ** -16      # the fixture's gradients keep 16 mantissa bits


@pytest.fixture(scope="module")
def tops():
    import astts  # noqa: F401
    from astts import train_ops
    return train_ops


@pytest.fixture(scope="module")
def kats():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lora_train_kats.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny(kats):
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.tiny()
    sd = make_llama_weights(cfg, int(kats["seed"]))
    lora = ref.make_lora(cfg, int(kats["r"]), int(kats["lora_seed"]))
    return cfg, sd, lora, torch.from_numpy(kats["ids"]), torch.from_numpy(kats["lens"])


def make_trainer(cfg, sd, lora, r, alpha, lr=1e-3, **kw):
    from astts.llm.peft import PROJ, LoraAdapter
    from astts.llm.train import LoraTrainer
    ad = LoraAdapter(r=r, lora_alpha=alpha, use_rslora=False, targets=tuple(PROJ), base_model_name_or_path="", pairs=dict(lora))
    # loss scale 1: the synthetic model's gradients are O(10) already (its loss is ~150), far from fp16's underflow; warm-up off: the
    # fixture's three steps run at the full learning rate
    return LoraTrainer(sd, cfg, DEV, adapter=ad, lr=lr, total_steps=1, warmup_ratio=0.0, loss_scale=1.0, **kw)


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (6, 2)])
@pytest.mark.parametrize("t,lens", [(1, (1, 1)), (33, (33, 1)), (80, (80, 45)), (200, (200, 131))])
def test_attn_gqa_bwd(tops, t, lens, heads, kv_heads):
    g = torch.Generator().manual_seed(t * 10 + heads)
    b, d = 2, 128
    w = (heads + 2 * kv_heads) * d
    qkv = torch.randn(b, t, w, generator=g).half()
    dout = torch.randn(b, t, heads * d, generator=g).half()
    ln = torch.tensor(lens)

    def cpu(expand, h16=False):
        x = qkv.float().requires_grad_(True)
        q, k, v = x[..., :heads * d], x[..., heads * d:(heads + kv_heads) * d], x[..., (heads + kv_heads) * d:]
        o = ref.attention(q.reshape(b, t, heads, d), k.reshape(b, t, kv_heads, d), v.reshape(b, t, kv_heads, d), ln, heads, kv_heads,
                          expand=expand, h16=h16)
        o.backward(dout.float())
        return x.grad

    want, want2, emu = cpu(False), cpu(True), cpu(False, h16=True)
    got = tops.attn_gqa_bwd(qkv.to(DEV), dout.to(DEV), heads, kv_heads, d, ln.to(DEV, torch.int32)).float().cpu()
    assert torch.isfinite(got).all()
    for i in range(b):                                 # the padding takes no gradient, exactly
        assert not got[i, lens[i]:].any()
    cuts = (0, heads * d, (heads + kv_heads) * d, w)
    for name, lo, hi in zip(("dq", "dk", "dv"), cuts[:-1], cuts[1:]):
        # P (and q * scale * log2 e) rounded to fp16 as the kernel holds them: the emulated run's own error; dS and the fp16 result
        # add one fp16 rounding each (2^-11 per element, independent) -- 4x their sum covers accumulation order and exp2
        bound = 4 * (ref.rel_l2(emu[..., lo:hi], want[..., lo:hi]) + 2 * H16)
        e1, e2 = ref.rel_l2(got[..., lo:hi], want[..., lo:hi]), ref.rel_l2(got[..., lo:hi], want2[..., lo:hi])
        print(f"attn_bwd T={t} heads={heads}/{kv_heads} {name}: rel L2 {e1:.2e} / {e2:.2e} (bound {bound:.2e})")
        assert e1 <= bound and e2 <= bound, (name, e1, e2, bound)


@pytest.mark.parametrize("r", [8, 32])
@pytest.mark.parametrize("k", [512, 3072])
@pytest.mark.parametrize("rows", [1, 77, 257])
def test_lora_grad(tops, rows, k, r):
    assert tops.lora_grad_row_split() == 256          # 257: one row past the slab
    g = torch.Generator().manual_seed(rows + k + r)
    u = torch.randn(rows, k + 64, generator=g).half()            # column slices of wider planes, as the trainer passes them
    x = torch.randn(rows, r + 8, generator=g).half()
    ud, xd = u.to(DEV), x.to(DEV)
    # fp16 x fp16 products are exact in fp32; the fp32 accumulation of `rows` terms errs by at most rows * 2^-24 of sum |terms|,
    # which random signs make ~sqrt(rows) times the result: 4 * sqrt(rows) * rows * 2^-24 bounds it generously (>= 2^-22)
    bound = max(4 * rows ** 1.5 * 2.0 ** -24, 2.0 ** -22)
    for un, xn, name in ((ud[:, :k], xd[:, :r], "dB"), (xd[:, :r], ud[:, :k], "dA")):
        want = un.double().cpu().t() @ xn.double().cpu()
        got = tops.lora_grad(un, xn, alpha=0.5)
        again = tops.lora_grad(un.float(), xn, out=got.clone(), alpha=0.5, accumulate=True)      # fp32 U, accumulated on top
        e1, e2 = ref.rel_l2(got.cpu(), 0.5 * want), ref.rel_l2(again.cpu(), want)
        print(f"lora_grad rows={rows} k={k} r={r} {name}: rel L2 {e1:.2e} / {e2:.2e} (bound {bound:.2e})")
        assert e1 <= bound and e2 <= bound


def test_rmsnorm_bwd(tops):
    g = torch.Generator().manual_seed(3)
    rows, c, eps = 37, 512, 1e-5
    x, dy, w = torch.randn(rows, c, generator=g) * 3, torch.randn(rows, c, generator=g), 1 + 0.1 * torch.randn(c, generator=g)
    res0 = torch.randn(rows, c, generator=g)
    xd = x.double().requires_grad_(True)
    ref.rmsnorm(xd, w.double(), eps).backward(dy.double())
    got = tops.rmsnorm_bwd_(res0.to(DEV), dy.to(DEV), x.to(DEV), w.to(DEV), eps).cpu()
    e = ref.rel_l2(got - res0, xd.grad)
    bound = 4 * c * 2.0 ** -24                         # two fp32 sums over c terms, then a cancelling difference of O(1) terms
    print(f"rmsnorm_bwd: rel L2 {e:.2e} (bound {bound:.2e})")
    assert e <= bound


def test_swiglu_bwd(tops):
    g = torch.Generator().manual_seed(4)
    rows, f = 37, 1024
    gu, dout = (torch.randn(rows, 2 * f, generator=g) * 2).half(), torch.randn(rows, f, generator=g).half()
    x = gu.double().requires_grad_(True)
    (torch.nn.functional.silu(x[:, :f]) * x[:, f:]).backward(dout.double())
    got = tops.swiglu_bwd(dout.to(DEV), gu.to(DEV)).cpu()
    e = ref.rel_l2(got, x.grad)
    print(f"swiglu_bwd: rel L2 {e:.2e} (bound {4 * H16:.2e})")
    assert e <= 4 * H16                                # the fp16 result's rounding (2^-11 per element) dominates the fp32 arithmetic


@pytest.mark.parametrize("vocab", [512, 1000])
def test_xent_grad(tops, vocab):
    g = torch.Generator().manual_seed(vocab)
    rows, ld, scale = 45, vocab + 24, 1024.0 / 37
    logits = torch.randn(rows, ld, generator=g) * 8
    targets = torch.randint(0, vocab, (rows,), generator=g)
    targets[::5] = -1
    x = logits[:, :vocab].double().requires_grad_(True)
    (torch.nn.functional.cross_entropy(x, targets.masked_fill(targets < 0, -100), ignore_index=-100, reduction="sum") * scale).backward()
    buf = logits.to(DEV)
    lse = torch.logsumexp(logits[:, :vocab].double(), -1).float()
    tops.xent_grad_(buf[:, :vocab], lse.to(DEV), targets.to(DEV, torch.int32), scale)
    got = buf.cpu()
    assert torch.equal(got[:, vocab:], logits[:, vocab:]), "columns beyond the vocabulary are not touched"
    assert not got[::5, :vocab].any(), "rows with target -1 become zeros"
    e = ref.rel_l2(got[:, :vocab], x.grad)
    # exp(logit - lse): the fp32 difference of numbers up to ~40 errs by 40 * 2^-24 absolute = relative in exp; + exp's own 2 ulp
    bound = 4 * (40 * 2.0 ** -24 + 2.0 ** -22)
    print(f"xent_grad vocab={vocab}: rel L2 {e:.2e} (bound {bound:.2e})")
    assert e <= bound


def test_adamw_and_sumsq(tops):
    g = torch.Generator().manual_seed(5)
    n = 70001
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10 ** (i - 1) for i in range(3)]
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for i, gr in enumerate(grads):
        scale = 1024.0
        gd = (gr * scale).to(DEV)
        ss = float(tops.sumsq(gd))
        want_ss = float((gr.double() * scale).pow(2).sum())
        assert abs(ss - want_ss) <= 1e-6 * want_ss, (ss, want_ss)
        norm = ss ** 0.5 / scale
        mul = min(1.0, 0.3 / (norm + 1e-6))
        probe = gr.clone().requires_grad_(True)
        probe.grad = gr.clone()
        assert abs(float(torch.nn.utils.clip_grad_norm_([probe], 0.3)) - norm) <= 1e-6 * norm
        # torch gets the gradient clipped by the SAME factor (its own fp32 norm differs from the fp64 one in the 7th digit, and v
        # carries the factor squared): what is compared below is the optimizer arithmetic
        pt.grad = (gr.double() * mul).float()
        opt.step()
        tops.adamw_(p, gd, m, v, i + 1, 2e-4, weight_decay=0.01, grad_mul=mul / scale)
        st = opt.state[pt]
        for name, a, bb in (("p", p, pt.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            e = ref.rel_l2(a.cpu(), bb)
            print(f"adamw step {i + 1} {name}: rel L2 {e:.2e}")
            assert e <= 1e-6, (i, name, e)
    bad = grads[0].clone()
    bad[12345] = float("inf")
    assert not np.isfinite(float(tops.sumsq(bad.to(DEV))))
    bad[12345] = float("nan")
    assert not np.isfinite(float(tops.sumsq(bad.to(DEV))))


# ------------------------------------------------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def tiny_run(tiny, kats):
    """One accumulate (loss + gradients) and three steps on the fixture batch, shared by the tests below."""
    cfg, sd, lora, ids, lens = tiny
    tr = make_trainer(cfg, sd, lora, int(kats["r"]), float(kats["lora_alpha"]), lr=float(kats["lr"]))
    loss0 = tr.accumulate([(ids, lens)])
    grads = {k: v.detach().cpu().clone() for k, v in tr.named_grads().items()}
    params0 = tr.params.clone()
    reports = [tr.step([(ids, lens)]) for _ in range(3)]
    return tr, loss0, grads, params0, reports


def test_model_loss_and_gradients(tiny_run, kats):
    _, loss0, grads, _, _ = tiny_run
    want = float(kats["losses"][0])
    print(f"loss {loss0:.6f} vs {want:.6f}: rel {abs(loss0 - want) / want:.2e} (bound {TINY_LOSS_BOUND:.2e})")
    assert abs(loss0 - want) <= TINY_LOSS_BOUND * want
    worst = 0.0
    for (i, p, h), gr in grads.items():
        e = ref.rel_l2(gr, kats[f"grad.{i}.{p}.{h}"])
        worst = max(worst, e)
        assert e <= TINY_GRAD_BOUND + FIXTURE_GRAD_STORAGE, (i, p, h, e)
    print(f"worst LoRA gradient rel L2 {worst:.2e} (bound {TINY_GRAD_BOUND:.2e})")


def test_three_steps(tiny_run, tiny, kats):
    tr, _, _, _, reports = tiny_run
    cfg, sd, lora, ids, lens = tiny
    losses = [r.loss for r in reports] + [tr.loss(ids, lens)]
    for j, (a, w) in enumerate(zip(losses, kats["losses"])):
        print(f"step {j}: loss {a:.6f} vs {float(w):.6f} rel {abs(a - w) / w:.2e} (bound {TINY_TRAJ_BOUND:.2e})")
        assert abs(a - w) <= TINY_TRAJ_BOUND * w, (j, a, w)
    for r, w in zip(reports, kats["grad_norms"]):
        assert not r.skipped and abs(r.grad_norm - w) <= TINY_GRAD_BOUND * w, (r, w)
    ad = tr.adapter()
    worst = 0.0
    for (i, p), (a, b) in ad.pairs.items():
        for h, now, was in (("A", a, lora[(i, p)][0]), ("B", b, lora[(i, p)][1])):
            e = ref.rel_l2(now - was, kats[f"delta.{i}.{p}.{h}"].astype(np.float32))
            worst = max(worst, e)
            assert e <= TINY_DELTA_BOUND, (i, p, h, e)
    print(f"worst parameter change rel L2 {worst:.2e} (bound {TINY_DELTA_BOUND:.2e})")


def test_step_is_repeatable(tiny_run, tiny, kats):
    cfg, sd, lora, ids, lens = tiny
    runs = []
    for _ in range(2):
        tr = make_trainer(cfg, sd, lora, int(kats["r"]), float(kats["lora_alpha"]), lr=float(kats["lr"]))
        tr.step([(ids[:2], lens[:2]), (ids[2:], lens[2:])])            # two micro-batches: the accumulation path too
        runs.append((tr.grads.clone(), tr.params.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(runs[0][0].any())


def test_accumulation_equals_one_batch(tiny_run, tiny, kats):
    """Micro-batches normalised by the whole step's token count give the one-batch gradient (to fp16-path rounding)."""
    cfg, sd, lora, ids, lens = tiny
    _, loss0, grads, _, _ = tiny_run
    tr = make_trainer(cfg, sd, lora, int(kats["r"]), float(kats["lora_alpha"]))
    loss = tr.accumulate([(ids[:2], lens[:2]), (ids[2:], lens[2:])])
    assert abs(loss - loss0) <= TINY_LOSS_BOUND * loss0
    for k, gr in tr.named_grads().items():
        assert ref.rel_l2(gr.cpu(), grads[k]) <= TINY_GRAD_BOUND, k


def test_real_widths_one_layer():
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = dataclasses.replace(LlamaShape.wide(), layers=1)
    sd = make_llama_weights(cfg, 0)
    lora = ref.make_lora(cfg, 8, 11)
    ids, lens = ref.make_batch(cfg, (64,), 12)
    loss_w, want = ref.loss_and_grads(sd, cfg, lora, 4.0, ids, lens)
    tr = make_trainer(cfg, sd, lora, 8, 32.0)
    loss = tr.accumulate([(ids, lens)])
    assert abs(loss - loss_w) <= 4 * 1.3e-5 * loss_w, (loss, loss_w)       # emulated 1.3e-5
    worst = 0.0
    for k, gr in tr.named_grads().items():
        e = ref.rel_l2(gr.cpu(), want[k])
        worst = max(worst, e)
        assert e <= WIDE_GRAD_BOUND, (k, e)
    print(f"real widths: worst gradient rel L2 {worst:.2e} (bound {WIDE_GRAD_BOUND:.2e})")


def test_adapter_round_trip_through_inference(tiny_run, tiny, tmp_path):
    """Train, save_adapter, load through load_peft_model into the fp16 (merged) inference path: its mean -log p of the training batch
    is the trainer's own forward loss at those parameters.  Merging rounds W + scaling B A to fp16 once where the trainer rounds W, A,
    scaling B and the rank activations separately: a part of the roundings whose whole effect on this loss is 5.6e-6 (TINY_LOSS_BOUND)."""
    import llm_int8_ref as i8
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.peft import load_peft_model
    from astts.llm.weights import load_llama_weights
    cfg, sd, lora, ids, lens = tiny
    base = i8.write_base(str(tmp_path / "base"), cfg, sd)
    sd16 = load_llama_weights(base)
    tr = make_trainer(cfg, sd16, lora, 8, 32.0)
    for _ in range(3):
        tr.step([(ids, lens)])
    tr.save_adapter(str(tmp_path / "adapter"))
    own = tr.loss(ids, lens)
    state, cfg2, ad, _ = load_peft_model(str(tmp_path / "adapter"), base)
    emb = LlamaEmbedder(state, cfg2, DEV, lora=ad)
    lp = emb.token_logprobs(ids.to(DEV), lens.to(DEV, torch.int32))
    inf = -float(lp.sum()) / int((lens - 1).sum())
    print(f"round trip: trainer {own:.6f} inference {inf:.6f} rel {abs(own - inf) / own:.2e} (bound {TINY_LOSS_BOUND:.2e})")
    assert abs(own - inf) <= TINY_LOSS_BOUND * own
