"""GPU tests of the fine-tuning regularisers (LoRA dropout from a counter-based generator, NEFTune): the generator against its numpy
restatement bit for bit, every kernel against fp64 on fp16-valued inputs, the trainer against the fp32 autograd restatement
(tests/lora_reg_ref.py), and the ft_llm command line with the reference's recipe switched on.

Bounds.  Relative L2 per tensor.  The kernel bounds come from the number formats and are derived where they are set.  The model
bounds are 4x the error of the restatement run with fp16 rounding where the GPU path holds fp16 (``h16=True``) against its fp32 run,
computed on the CPU for this batch, seed 42, draw 0; the figures stand beside the constants and in DESIGN.md section 2."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import llm_train_ref as ref  # noqa: E402
import lora_reg_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H16 = 2.0 ** -11                       # fp16 rounding, relative
SEED = 42
NEFTUNE_ALPHA = 5.0

# emulated (h16 restatement vs fp32, lora_dropout p, NEFTune alpha 5) -> bound = 4x; measured on an MI355X: DESIGN.md section 2
REG_LOSS_BOUND = {0.05: 4 * 1.04e-5, 0.5: 4 * 1.68e-5}      # loss of the fixture batch: emulated 1.04e-5 / 1.68e-5 relative (GPU 6.6e-6 / 1.33e-5)
REG_GRAD_BOUND = {0.05: 4 * 1.76e-3, 0.5: 4 * 1.75e-3}      # worst LoRA gradient (layer 2 k_proj B / A): emulated 1.76e-3 / 1.75e-3 (GPU 1.77e-3 / 1.84e-3)


@pytest.fixture(scope="module")
def tops():
    import astts  # noqa: F401
    from astts import train_ops
    return train_ops


@pytest.fixture(scope="module")
def ops():
    import astts  # noqa: F401
    from astts import ops
    return ops


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


def make_trainer(cfg, sd, lora, r, alpha, **kw):
    from astts.llm.peft import PROJ, LoraAdapter
    from astts.llm.train import LoraTrainer
    ad = LoraAdapter(r=r, lora_alpha=alpha, use_rslora=False, targets=tuple(PROJ), base_model_name_or_path="", pairs=dict(lora))
    return LoraTrainer(sd, cfg, DEV, adapter=ad, lr=1e-3, total_steps=1, warmup_ratio=0.0, loss_scale=1.0, seed=SEED, **kw)


def masks(rows, cin, parts, p, stream, draw):
    """float64 [parts, rows, cin]: part j's keep mask (stream + j), from the numpy generator."""
    return torch.from_numpy(np.stack([rr.dropout_mask(rows, cin, p, SEED, stream + j, draw) for j in range(parts)])).double()


# ------------------------------------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("cin", [512, 3072, 8192])
@pytest.mark.parametrize("rows", [1, 77, 257])
def test_dropout_mask(tops, rows, cin, p):
    got = {}
    for stream, draw in ((3, 0), (3, 7), (2 * 8 + 6, 0), (2 * 8 + 6, 7)):           # two streams, two draws
        got[(stream, draw)] = m = tops.dropout_mask(rows, cin, p, SEED, stream, draw, DEV).cpu().numpy()
        assert np.array_equal(m, rr.dropout_mask(rows, cin, p, SEED, stream, draw)), (stream, draw)
    other_seed = tops.dropout_mask(rows, cin, p, SEED + (1 << 32), 3, 0, DEV).cpu().numpy()      # the seed's high word counts
    assert np.array_equal(other_seed, rr.dropout_mask(rows, cin, p, SEED + (1 << 32), 3, 0))
    base = got[(3, 0)]
    for name, m in (("draw", got[(3, 7)]), ("stream", got[(22, 0)]), ("seed", other_seed)):
        assert not np.array_equal(m, base), f"changing the {name} leaves the mask unchanged"
    if rows * cin >= 1 << 15:                                                        # the kept share is 1 - floor(p 65536) / 65536
        assert abs(base.mean() - (1 - p)) < 0.01


def test_neftune(tops):
    b, t, hidden = 2, 40, 512
    mag = float(np.float32(rr.neftune_mag(NEFTUNE_ALPHA, t, hidden)))
    g = torch.Generator().manual_seed(1)
    # |x| < mag / 2: the kernel's fma rounds x + noise once, by at most 2^-24 |x + noise| < 2^-24 * 1.5 mag -- inside the 2^-23 mag set
    # for it (the noise itself, an odd multiple of 2^-24 times mag, is exact before that rounding)
    x = ((torch.rand(b * t, hidden, generator=g) - 0.5) * mag).float()
    for draw in (0, 3):
        want = rr.neftune_noise(b * t, hidden, mag, SEED, draw)
        out = tops.neftune_(x.to(DEV).clone(), mag, SEED, draw).cpu()
        err = float((out.double() - x.double() - torch.from_numpy(want)).abs().max())
        print(f"neftune draw {draw}: max |error| {err:.3e} (bound {2.0 ** -23 * mag:.3e})")
        assert err <= 2.0 ** -23 * mag
        noise = tops.neftune_(torch.zeros(b * t, hidden, device=DEV), mag, SEED, draw).cpu()
        assert float(noise.abs().max()) < mag and float(noise.abs().min()) > 0.0     # strictly inside (-mag, mag)
        assert abs(float(noise.mean())) < 0.01 * mag and float(noise.abs().max()) > 0.99 * mag
    assert not torch.equal(tops.neftune_(torch.zeros(8, hidden, device=DEV), mag, SEED, 0), tops.neftune_(torch.zeros(8, hidden, device=DEV), mag, SEED, 1))


# ------------------------------------------------------------------------------------------------------------- kernels
def operands(ops, rows, cin, parts, r, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cin, generator=g).half()
    a = ((torch.rand(parts * r, cin, generator=g) * 2 - 1) / math.sqrt(cin)).half()
    dt = torch.randn(rows, parts * r, generator=g).half()
    return x, a, dt


@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("r", [8, 32])
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("cin", [512, 3072])
@pytest.mark.parametrize("rows", [1, 77, 257])
def test_lora_down(tops, ops, rows, cin, parts, r, p):
    x, a, _ = operands(ops, rows, cin, parts, r, rows + cin + parts + r)
    a_pack = ops.PackedWeight(a.float(), None, DEV)
    stream, draw = 8 + 4, 5
    m = masks(rows, cin, parts, p, stream, draw)
    want = torch.cat([(m[j] * x.double()) @ a[j * r:(j + 1) * r].double().t() for j in range(parts)], 1) / (1 - p)
    got = tops.lora_down(x.to(DEV), a_pack, parts, r, p, SEED, stream, draw)
    assert got.dtype == torch.float16 and got.shape == (rows, parts * r)
    e = ref.rel_l2(got.cpu(), want)
    print(f"lora_down rows={rows} cin={cin} parts={parts} r={r} p={p}: rel L2 {e:.2e} (bound {H16:.2e})")
    assert e <= H16                                    # one fp16 rounding of the output
    if p == 0.05:                                      # once per shape: no dropout is the plain product, bit for bit (the wrapper hands p = 0 to it)
        assert torch.equal(tops.lora_down(x.to(DEV), a_pack, parts, r, 0.0, SEED, stream, draw), ops.linear(x.to(DEV), a_pack, out_dtype=torch.float16))


@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("r", [8, 32])
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("cin", [512, 3072])
@pytest.mark.parametrize("rows", [1, 77, 257])
def test_lora_grad_dropout(tops, ops, rows, cin, parts, r, p):
    x, _, dt = operands(ops, rows, cin, parts, r, rows + cin + parts + r + 1)
    stream, draw = 2 * 8, 1
    m = masks(rows, cin, parts, p, stream, draw)
    want = torch.cat([dt[:, j * r:(j + 1) * r].double().t() @ (m[j] * x.double()) for j in range(parts)], 0) / (1 - p)
    # test_lora_grad's bound for the unmasked product: masking removes terms and adds none
    bound = max(4 * rows ** 1.5 * 2.0 ** -24, 2.0 ** -22)
    kw = dict(parts=parts, r=r, p=p, seed=SEED, rng_stream=stream, draw=draw)
    xd, dtd = x.to(DEV), dt.to(DEV)
    got = tops.lora_grad_dropout(dtd, xd, alpha=0.5, **kw)
    twice = tops.lora_grad_dropout(dtd.float(), xd, out=got.clone(), alpha=0.5, accumulate=True, **kw)     # fp32 U, accumulated on top
    e1, e2 = ref.rel_l2(got.cpu(), 0.5 * want), ref.rel_l2(twice.cpu(), want)
    print(f"lora_grad_dropout rows={rows} cin={cin} parts={parts} r={r} p={p}: rel L2 {e1:.2e} / {e2:.2e} (bound {bound:.2e})")
    assert e1 <= bound and e2 <= bound
    assert torch.equal(tops.lora_grad_dropout(dtd, xd, alpha=0.5, **kw), got)                               # repeatable bit for bit


@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("parts,r", [(1, 8), (2, 32), (3, 8), (3, 32), (1, 64)])
@pytest.mark.parametrize("cin", [512, 520, 3072])          # 520: a multiple of 8 that ends inside a 32-column tile
@pytest.mark.parametrize("rows", [1, 77, 257])
def test_lora_dx_dropout(tops, ops, rows, cin, parts, r, p):
    _, a, dt = operands(ops, rows, cin, parts, r, rows + cin + parts + r + 2)
    g = torch.Generator().manual_seed(rows)
    res = torch.randn(rows, cin, generator=g)
    at_pack = ops.PackedWeight(a.float().t().contiguous(), None, DEV)
    stream, draw = 8 + 3, 2
    m = masks(rows, cin, parts, p, stream, draw)
    want = res.double() + sum(m[j] * (dt[:, j * r:(j + 1) * r].double() @ a[j * r:(j + 1) * r].double()) for j in range(parts)) / (1 - p)
    kw = dict(parts=parts, r=r, p=p, seed=SEED, rng_stream=stream, draw=draw)
    b32 = parts * r * 2.0 ** -24                             # the worst case of the fp32 accumulation
    got32 = tops.lora_dx_dropout(dt.to(DEV), at_pack, res.to(DEV), **kw)
    got16 = tops.lora_dx_dropout(dt.to(DEV), at_pack, res.to(DEV), out_dtype=torch.float16, **kw)
    e32, e16 = ref.rel_l2(got32.cpu(), want), ref.rel_l2(got16.cpu(), want)
    print(f"lora_dx_dropout rows={rows} cin={cin} parts={parts} r={r} p={p}: fp32 {e32:.2e} (bound {b32:.2e}), fp16 {e16:.2e} (bound {b32 + H16:.2e})")
    assert got32.dtype == torch.float32 and got16.dtype == torch.float16
    assert e32 <= b32 and e16 <= b32 + H16
    same = tops.lora_dx_dropout(torch.zeros_like(dt).to(DEV), at_pack, res.to(DEV), **kw)
    assert torch.equal(same.cpu(), res), "dt = 0 carries the residual through exactly"


# ------------------------------------------------------------------------------------------------------------- whole model
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_model_loss_and_gradients(tiny, kats, p):
    """p = 0.5 too: a mask applied in forward but not in backward (or the reverse) changes half of every product."""
    cfg, sd, lora, ids, lens = tiny
    r, alpha = int(kats["r"]), float(kats["lora_alpha"])
    want_loss, want = rr.loss_and_grads(sd, cfg, lora, alpha / r, ids, lens, p, NEFTUNE_ALPHA, SEED, 0)
    tr = make_trainer(cfg, sd, lora, r, alpha, lora_dropout=p, neftune_alpha=NEFTUNE_ALPHA)
    loss = tr.accumulate([(ids, lens)])
    el = abs(loss - want_loss) / want_loss
    print(f"p={p}: loss {loss:.6f} vs {want_loss:.6f}: rel {el:.2e} (bound {REG_LOSS_BOUND[p]:.2e})")
    worst = max((ref.rel_l2(gr.cpu(), want[k]), k) for k, gr in tr.named_grads().items())
    print(f"p={p}: worst LoRA gradient rel L2 {worst[0]:.2e} at {worst[1]} (bound {REG_GRAD_BOUND[p]:.2e})")
    assert el <= REG_LOSS_BOUND[p]
    assert worst[0] <= REG_GRAD_BOUND[p], worst


def test_repeatable_and_draws_separate(tiny, kats):
    cfg, sd, lora, ids, lens = tiny
    r, alpha = int(kats["r"]), float(kats["lora_alpha"])
    runs = []
    for _ in range(2):
        tr = make_trainer(cfg, sd, lora, r, alpha, lora_dropout=0.05, neftune_alpha=NEFTUNE_ALPHA)
        assert tr.draw == 0 and tr.noise_seed == SEED
        tr.accumulate([(ids[:2], lens[:2]), (ids[2:], lens[2:])])
        assert tr.draw == 2                                   # one draw per micro-batch
        runs.append(tr.grads.clone())
    assert torch.equal(runs[0], runs[1]) and bool(runs[0].any())
    plain = make_trainer(cfg, sd, lora, r, alpha)
    before = tr.loss(ids, lens)
    assert tr.draw == 2, "an evaluation takes no draw"
    assert before == plain.loss(ids, lens), "loss() is an evaluation: no dropout, no noise"
    other = make_trainer(cfg, sd, lora, r, alpha, lora_dropout=0.05, neftune_alpha=NEFTUNE_ALPHA, noise_seed=SEED + 1)
    other.accumulate([(ids[:2], lens[:2]), (ids[2:], lens[2:])])
    assert not torch.equal(other.grads, runs[0])


def test_off_means_off(tiny, kats):
    cfg, sd, lora, ids, lens = tiny
    r, alpha = int(kats["r"]), float(kats["lora_alpha"])
    a = make_trainer(cfg, sd, lora, r, alpha)
    b = make_trainer(cfg, sd, lora, r, alpha, lora_dropout=0.0, neftune_alpha=0.0)
    la, lb = a.accumulate([(ids[:2], lens[:2]), (ids[2:], lens[2:])]), b.accumulate([(ids[:2], lens[:2]), (ids[2:], lens[2:])])
    assert la == lb and torch.equal(a.grads, b.grads) and bool(a.grads.any())


# ------------------------------------------------------------------------------------------------------------- command line
def test_cli_reference_recipe(tmp_path, monkeypatch):
    from astts.cli import ft_llm
    from astts.llm.peft import load_adapter
    from astts.llm.train import lr_at
    monkeypatch.setenv("ASTTS_TINY_MODEL", "1")
    words = [f"w{i}" for i in range(97)]
    with open(tmp_path / "toy.train.0shot_w5_spdescV2.jsonl", "w") as f:
        for i in range(40):
            said = " ".join(words[(7 * i + j) % 97] for j in range(20 + i % 9))
            f.write(json.dumps({"messages": [{"role": "user", "content": said}, {"role": "assistant", "content": words[i % 5]}]}) + "\n")
    args = ft_llm.build_parser().parse_args(
        ["--do_train", "--packing", "--max_seq_len", "64", "--lora_dropout", "0.05", "--neftune_noise_alpha", "5", "--lr_scheduler", "linear",
         "--max_steps", "3", "--allow_random_init", "--lora_r", "8", "--loss_scale", "1", "--data_name", "toy", "--data_folder", str(tmp_path),
         "--output_folder", str(tmp_path / "out"), "--ft_model_id", "ft", "--base_model_id", str(tmp_path / "no_such_base")])
    ft_llm.main(args)
    out = tmp_path / "out" / "ft"
    log = [json.loads(line) for line in open(out / "train_log.jsonl")]
    assert [rec["step"] for rec in log] == [1, 2, 3]
    for i, rec in enumerate(log):
        assert math.isfinite(rec["loss"]) and math.isfinite(rec["grad_norm"]) and not rec["skipped"], rec
        assert rec["lr"] == lr_at(i, args.lr, 3, schedule="linear"), rec
    assert [rec["lr"] for rec in log] == [0.0, args.lr, args.lr / 2]           # warm-up of ceil(0.09) = 1 step, then (3 - step) / 2
    assert json.load(open(out / "adapter_config.json"))["lora_dropout"] == 0.05
    ad = load_adapter(str(out))
    assert ad.r == 8 and len(ad.pairs) == 3 * 7 and any(bool(b.any()) for _, b in ad.pairs.values())
