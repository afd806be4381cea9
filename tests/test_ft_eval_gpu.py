"""GPU tests of evaluation while fine-tuning: the merge kernel (astts_train_lora_merge) against an fp64 restatement written here,
LoraTrainer.eval_model() against the host-merged LlamaEmbedder, save_state / load_state against an uninterrupted run (equality), and
the ft_llm command with --eval_steps / --save_steps / --load_best_model_at_end, resumed and uninterrupted."""
import dataclasses
import json
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
MAX_ULP = 1                 # no element of a merged image is further than this from the fp64 restatement's fp16 rounding
MAX_SHARE = 2e-3            # and at most this share differs at all (a plain fp32 evaluation of the formula: 1e-4 .. 3e-4)
GROUP_NAMES = ("wqkv", "wo", "wgu", "wd")


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


def ordered(h: torch.Tensor) -> torch.Tensor:
    """fp16 -> int32 whose differences count fp16 steps (+0 and -0 coincide)."""
    i = h.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_and_share(got: torch.Tensor, want: torch.Tensor):
    d = (ordered(got) - ordered(want)).abs()
    return int(d.max()), float((d != 0).float().mean())


def restatement(w16: torch.Tensor, a: torch.Tensor, b: torch.Tensor, outs, r: int, scaling: float) -> torch.Tensor:
    """(w.double() + scaling * b.double() @ a_part.double()).half(), part by part."""
    res, o = [], 0
    for j, n in enumerate(outs):
        res.append((w16[o:o + n].double() + scaling * b[o:o + n].double() @ a[j * r:(j + 1) * r].double()).half())
        o += n
    return torch.cat(res, 0)


# ------------------------------------------------------------------------------------------------------------- the merge kernel
@pytest.mark.parametrize("outs,cin,r", [
    ((130,), 70, 16),                    # ragged in both paddings
    ((256,), 192, 8),
    ((256, 64, 64), 320, 32),            # three unequal parts: g1, g2 = 256, 320 of n = 384
    ((128, 128), 128, 16),               # two parts
])
def test_lora_merge(tops, ops, outs, cin, r):
    n, scaling = sum(outs), 128.0 / r
    g = torch.Generator().manual_seed(n * 1000 + cin + r)
    w = (torch.randn(n, cin, generator=g) * 0.04).half().float()
    a = ((torch.rand(len(outs) * r, cin, generator=g) * 2 - 1) / cin ** 0.5).to(DEV)
    b = (torch.randn(n, r, generator=g) * 0.02).to(DEV)
    wp = ops.PackedWeight(w, None, DEV)
    before = wp.data.clone()
    assert torch.equal(wp.data[:n, 0, :cin].cpu().float(), w), "w is fp16-representable"
    out = ops.PackedWeight.zeros_like(wp)
    out.data.fill_(7.0)                                                      # the kernel writes every element, padding included
    g1 = outs[0]
    g2 = n if len(outs) < 3 else outs[0] + outs[1]
    tops.lora_merge(wp, a, b, out, r, g1, g2, scaling)
    first = out.data.clone()
    want = restatement(wp.data[:n, 0, :cin].cpu(), a.cpu(), b.cpu(), outs, r, scaling)
    ulp, share = ulp_and_share(first[:n, 0, :cin].cpu(), want)
    print(f"lora_merge {outs} x {cin} r {r}: max {ulp} ulp, {share:.2e} of the elements differ (bounds {MAX_ULP}, {MAX_SHARE:.0e})")
    assert ulp <= MAX_ULP and share <= MAX_SHARE
    assert bool((first[:n, 0, :cin] != wp.data[:n, 0, :cin]).any()), "the adapter changed the weights"
    assert not bool(first[n:].any()) and not bool(first[:, :, cin:].any()), "padding rows and columns are zero"
    assert torch.equal(wp.data, before), "w is unchanged"
    out.data.fill_(-3.0)
    tops.lora_merge(wp, a, b, out, r, g1, g2, scaling)
    assert torch.equal(out.data, first), "two runs are bit-equal"
    tops.lora_merge(wp, a, torch.zeros_like(b), out, r, g1, g2, scaling)
    assert torch.equal(out.data, wp.data), "b = 0: out is w, bit for bit"


# ------------------------------------------------------------------------------------------------------------- eval_model
def rounded_state(sd):
    """The projection weights rounded to fp16: what a stored checkpoint holds."""
    return {k: (v.half().float() if "_proj.weight" in k else v) for k, v in sd.items()}


def make_trainer(cfg, sd, lora, r, alpha, **kw):
    from astts.llm.peft import PROJ, LoraAdapter
    from astts.llm.train import LoraTrainer
    ad = LoraAdapter(r=r, lora_alpha=alpha, use_rslora=False, targets=tuple(PROJ), base_model_name_or_path="", pairs=dict(lora))
    kw.setdefault("warmup_ratio", 0.0)
    kw.setdefault("total_steps", 1)
    return LoraTrainer(sd, cfg, DEV, adapter=ad, lr=1e-3, seed=42, **kw)


def images(model):
    return [(i, nm, L[nm].data) for i, L in enumerate(model.L) for nm in GROUP_NAMES]


def compare_images(got, want, what):
    worst_ulp, worst_share = 0, 0.0
    for (i, nm, g), (_, _, w) in zip(images(got), images(want)):
        ulp, share = ulp_and_share(g, w)
        worst_ulp, worst_share = max(worst_ulp, ulp), max(worst_share, share)
        assert ulp <= MAX_ULP and share <= MAX_SHARE, (what, i, nm, ulp, share)
    print(f"{what}: worst image {worst_ulp} ulp, {worst_share:.2e} differ (bounds {MAX_ULP}, {MAX_SHARE:.0e})")


def restated_state(sd16, adapter):
    """The state whose projections are the fp64 restatement's fp16 images of W + scaling B A."""
    from astts.llm.peft import PROJ
    out = dict(sd16)
    for (i, p), (a, b) in adapter.pairs.items():
        k = f"model.layers.{i}.{PROJ[p]}.weight"
        out[k] = (sd16[k].double() + adapter.scaling * b.double() @ a.double()).half().float()
    return out


@pytest.fixture(scope="module")
def tiny_eval(kats):
    """Two optimizer steps on the fixture batch, then eval_model() beside the host-merged embedder of the same adapter."""
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.tiny()
    sd = rounded_state(make_llama_weights(cfg, int(kats["seed"])))
    lora = ref.make_lora(cfg, int(kats["r"]), int(kats["lora_seed"]))
    ids, lens = torch.from_numpy(kats["ids"]), torch.from_numpy(kats["lens"])
    tr = make_trainer(cfg, sd, lora, int(kats["r"]), float(kats["lora_alpha"]))
    for _ in range(2):
        assert not tr.step([(ids, lens)]).skipped
    emb = tr.eval_model()
    host = LlamaEmbedder(sd, cfg, DEV, lora=tr.adapter())
    return cfg, sd, tr, emb, host, ids, lens


def test_eval_model_images(tiny_eval):
    cfg, sd, tr, emb, host, ids, lens = tiny_eval
    compare_images(emb, host, "eval_model vs host merge (tiny)")
    for (i, nm, g), (_, _, base) in zip(images(emb), images(tr.dec)):
        assert g.data_ptr() != base.data_ptr() and not torch.equal(g, base), (i, nm)
    # everything else is the trainer's own tensor, not a copy
    assert emb.embed.data_ptr() == tr.dec.embed.data_ptr() and emb.head.data.data_ptr() == tr.dec.head.data.data_ptr()
    assert emb.norm.data_ptr() == tr.dec.norm.data_ptr() and all(E["n1"] is L["n1"] and E["n2"] is L["n2"] for E, L in zip(emb.L, tr.dec.L))
    assert emb.cos.data_ptr() == tr.dec.cos.data_ptr()


def test_eval_model_generates_and_scores_as_the_host_merge(tiny_eval):
    """The logits bound: 4 x what the host-merged embedder's own last-position logits move by when its images are replaced by the
    fp64 restatement's (they differ from the host's fp32 merge in the restatement's mismatches only).  Measured: DESIGN.md section 2."""
    from astts.llm.embedder import LlamaEmbedder
    cfg, sd, tr, emb, host, ids, lens = tiny_eval
    g = torch.Generator().manual_seed(5)
    prompts = [[cfg.bos_token_id] + torch.randint(3, cfg.vocab, (n,), generator=g).tolist() for n in (5, 9, 12)]
    assert emb.generate_greedy_batch(prompts, 10) == host.generate_greedy_batch(prompts, 10)
    restated = LlamaEmbedder(restated_state(sd, tr.adapter()), cfg, DEV)
    compare_images(host, restated, "host merge vs fp64 restatement")
    same = torch.tensor([[cfg.bos_token_id] + torch.randint(3, cfg.vocab, (11,), generator=g).tolist() for _ in range(3)], device=DEV)
    lh = host.logits_last(same)
    bound = 4.0 * float((restated.logits_last(same) - lh).abs().max())
    got = float((emb.logits_last(same) - lh).abs().max())
    print(f"last-position logits: eval_model vs host merge {got:.3e} (bound {bound:.3e}; logits up to {float(lh.abs().max()):.2f})")
    assert got <= bound


def test_eval_model_refreshes_in_place(tiny_eval):
    cfg, sd, tr, emb, host, ids, lens = tiny_eval
    ptrs = [g.data_ptr() for _, _, g in images(emb)]
    old = [g.clone() for _, _, g in images(emb)]
    assert not tr.step([(ids, lens)]).skipped
    again = tr.eval_model()
    assert again is emb and [g.data_ptr() for _, _, g in images(again)] == ptrs, "the images are refreshed, not reallocated"
    assert all(not torch.equal(g, o) for (_, _, g), o in zip(images(again), old)), "every image follows the new parameters"


def test_eval_model_images_qwen2():
    """Bias kept, a GQA group of 7, widths that are no multiple of 256."""
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.qwen2_tiny()
    sd = rounded_state(make_llama_weights(cfg, 3))
    tr = make_trainer(cfg, sd, ref.make_lora(cfg, 8, 11), 8, 32.0)
    ids, lens = ref.make_batch(cfg, [9, 14], 2)
    for _ in range(2):
        assert not tr.step([(ids, lens)]).skipped
    emb = tr.eval_model()
    host = LlamaEmbedder(sd, cfg, DEV, lora=tr.adapter())
    compare_images(emb, host, "eval_model vs host merge (qwen2_tiny)")
    for E, H in zip(emb.L, host.L):
        assert E["wqkv"].bias is not None and torch.equal(E["wqkv"].bias, H["wqkv"].bias)
    prompts = [[cfg.bos_token_id, 7, 9, 30], [cfg.bos_token_id, 100, 5]]
    assert emb.generate_greedy_batch(prompts, 4) == host.generate_greedy_batch(prompts, 4)


# ------------------------------------------------------------------------------------------------------------- resume
def test_resume_equals_uninterrupted(kats, tmp_path):
    from astts.llm.config import LlamaShape
    from astts.llm.train import LoraTrainer
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.tiny()
    sd = make_llama_weights(cfg, int(kats["seed"]))
    r, alpha = int(kats["r"]), float(kats["lora_alpha"])
    lora = ref.make_lora(cfg, r, int(kats["lora_seed"]))
    ids, lens = torch.from_numpy(kats["ids"]), torch.from_numpy(kats["lens"])
    micro = [(ids[:2], lens[:2]), (ids[2:], lens[2:])]
    recipe = dict(lora_dropout=0.05, neftune_alpha=5.0, schedule="linear", total_steps=6, warmup_ratio=0.03)
    a = make_trainer(cfg, sd, lora, r, alpha, **recipe)
    reps_a = [a.step(micro) for _ in range(6)]
    b = make_trainer(cfg, sd, lora, r, alpha, **recipe)
    reps_c = [b.step(micro) for _ in range(3)]
    b.save_state(str(tmp_path / "state"))
    assert sorted(os.listdir(tmp_path / "state")) == ["trainer_recipe.json", "trainer_state.safetensors"]
    del b
    c = make_trainer(cfg, sd, lora, r, alpha, **recipe)
    c.load_state(str(tmp_path / "state"))
    assert (c.sched_step, c.draw) == (3, 6)
    reps_c += [c.step(micro) for _ in range(3)]
    for name in ("params", "m", "v"):
        assert torch.equal(getattr(a, name), getattr(c, name)), name
    assert (a.draw, a.opt_step, a.sched_step, a.loss_scale) == (c.draw, c.opt_step, c.sched_step, c.loss_scale)
    assert [dataclasses.asdict(x) for x in reps_a] == [dataclasses.asdict(x) for x in reps_c]
    assert not any(x.skipped for x in reps_a) and reps_a[-1].lr < reps_a[1].lr
    # another recipe is refused, and the message names the key
    other = make_trainer(cfg, sd, lora, r, alpha, **dict(recipe, schedule="constant"))
    with pytest.raises(ValueError, match="'schedule'"):
        other.load_state(str(tmp_path / "state"))
    wider = LoraTrainer(sd, cfg, DEV, r=2 * r, lora_alpha=alpha, lr=1e-3, seed=42, **recipe)
    with pytest.raises(ValueError, match="'r'"):
        wider.load_state(str(tmp_path / "state"))


# ------------------------------------------------------------------------------------------------------------- command line
WORDS = [f"w{i}" for i in range(97)]
LABELS = ("happy", "sad", "neutral")


def write_split(folder, split, shift):
    with open(folder / f"toy.{split}.0shot_w5_spdescV2.jsonl", "w") as f:
        for i in range(8):
            said = " ".join(WORDS[(7 * (i + shift) + j) % 97] for j in range(12 + i % 5))
            f.write(json.dumps({"messages": [{"role": "user", "content": said}, {"role": "assistant", "content": LABELS[i % 3]}]}) + "\n")


def run_cli(folder, name, *extra):
    from astts.cli import ft_llm
    args = ft_llm.build_parser().parse_args(
        ["--do_train", "--eval_steps", "2", "--save_steps", "2", "--eval_delay", "2", "--save_total_limit", "1", "--load_best_model_at_end",
         "--lr_scheduler", "linear", "--lora_dropout", "0.05", "--neftune_noise_alpha", "5", "--allow_random_init", "--lora_r", "8",
         "--data_name", "toy", "--data_folder", str(folder), "--output_folder", str(folder / "out"), "--ft_model_id", name,
         "--base_model_id", str(folder / "no_such_base"), *extra])
    ft_llm.main(args)
    return folder / "out" / name


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    folder = tmp_path_factory.mktemp("ft_eval")
    mp = pytest.MonkeyPatch()
    mp.setenv("ASTTS_TINY_MODEL", "1")
    write_split(folder, "train", 0)
    write_split(folder, "valid", 3)
    try:
        yield folder, run_cli(folder, "whole", "--max_steps", "6")
    finally:
        mp.undo()


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_evaluates_saves_and_keeps_the_best(cli_run):
    from astts.cli import ft_llm
    folder, out = cli_run
    metrics = []
    for s in (2, 4, 6):
        res = json.load(open(out / f"result_eval_step-{s}.json"))
        assert sorted(res) == ["detail_pred", "metrics"] and list(res["metrics"]) == ["eval_weighted-f1"]
        assert len(res["detail_pred"]) == 8 and all(len(t) == 3 and all(isinstance(x, str) for x in t) for t in res["detail_pred"])
        assert len({t[1] for t in res["detail_pred"]}) == len(LABELS)             # [pred, label, raw]: the gold labels of the valid rows
        metrics.append(res["metrics"]["eval_weighted-f1"])
    assert not os.path.exists(out / "result_eval_step-1.json") and not os.path.exists(out / "result_eval_step-3.json")
    elog = [json.loads(ln) for ln in open(out / "eval_log.jsonl")]
    assert [(e["step"], e["eval_weighted-f1"]) for e in elog] == list(zip((2, 4, 6), metrics))
    assert [json.loads(ln)["step"] for ln in open(out / "train_log.jsonl")] == [1, 2, 3, 4, 5, 6]
    best = (2, 4, 6)[metrics.index(max(metrics))]                                 # index(): the first maximum
    state = json.load(open(out / "checkpoint-6" / ft_llm.TRAINER_STATE))
    assert state["global_step"] == 6 and state["best_model_checkpoint"] == f"checkpoint-{best}" and state["best_metric"] == max(metrics)
    assert sorted(d for d in os.listdir(out) if d.startswith("checkpoint-")) == sorted({f"checkpoint-{best}", "checkpoint-6"})
    for name in ft_llm.ADAPTER_FILES:
        assert read_bytes(out / name) == read_bytes(out / f"checkpoint-{best}" / name), name
    assert {"trainer_recipe.json", "trainer_state.safetensors", *ft_llm.ADAPTER_FILES, ft_llm.TRAINER_STATE} <= set(os.listdir(out / "checkpoint-6"))


def test_cli_resumes_to_the_same_run(cli_run, capsys):
    from astts.cli import ft_llm
    folder, whole = cli_run
    part = run_cli(folder, "resumed", "--max_steps", "4", "--total_steps", "6")
    assert [json.loads(ln)["step"] for ln in open(part / "train_log.jsonl")] == [1, 2, 3, 4]
    assert os.path.isdir(part / "checkpoint-4")
    capsys.readouterr()
    run_cli(folder, "resumed", "--max_steps", "6")
    said = capsys.readouterr().out
    assert "resuming from" in said and "checkpoint-4" in said
    assert read_bytes(part / "train_log.jsonl") == read_bytes(whole / "train_log.jsonl")
    assert read_bytes(part / "eval_log.jsonl") == read_bytes(whole / "eval_log.jsonl")
    for name in ft_llm.ADAPTER_FILES:
        assert read_bytes(part / name) == read_bytes(whole / name), name
    assert read_bytes(part / "checkpoint-6" / "trainer_state.safetensors") == read_bytes(whole / "checkpoint-6" / "trainer_state.safetensors")
    # other training data under the same output directory: an error, not a fresh start
    write_split(folder, "train", 1)
    with pytest.raises(SystemExit, match="other data"):
        run_cli(folder, "resumed", "--max_steps", "8", "--total_steps", "6")
    write_split(folder, "train", 0)
    # another recipe: refused by load_state, naming the key
    with pytest.raises(ValueError, match="'total_steps'"):
        run_cli(folder, "resumed", "--max_steps", "8")
