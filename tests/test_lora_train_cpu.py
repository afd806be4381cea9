"""CPU tests of LoRA fine-tuning: the pure-torch restatement (tests/llm_train_ref.py) reproduces the transformers fixture, the
adapter directory round-trips through astts.llm.peft, the ft_llm command line has the reference's flags, the second library's header,
exports and ctypes signatures agree (and the main library's ABI is untouched), the schedule and the accumulation arithmetic."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import llm_train_ref as ref  # noqa: E402

# fp32 against fp32 (transformers' eager attention vs this restatement: other summation orders).  Gradients: the fixture keeps 16
# mantissa bits (2^-16 = 1.5e-5) on top of ~1e-6 of fp32 noise through three layers; parameter changes: stored as fp16 (2^-11 per
# element, 2.9e-4 in relative L2 at most) on top of Adam's amplification of that noise where v is small.
GRAD_TOL, LOSS_TOL, DELTA_TOL = 4e-5, 1e-6, 2e-3


@pytest.fixture(scope="module")
def kats():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lora_train_kats.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny(kats):
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.tiny()
    return (cfg, make_llama_weights(cfg, int(kats["seed"])), ref.make_lora(cfg, int(kats["r"]), int(kats["lora_seed"])),
            torch.from_numpy(kats["ids"]), torch.from_numpy(kats["lens"]))


def test_restatement_reproduces_fixture(tiny, kats):
    cfg, sd, lora, ids, lens = tiny
    ids2, lens2 = ref.make_batch(cfg, tuple(int(n) for n in lens), int(kats["batch_seed"]))
    assert torch.equal(ids2, ids) and torch.equal(lens2, lens)
    scaling = float(kats["lora_alpha"]) / int(kats["r"])
    loss, grads = ref.loss_and_grads(sd, cfg, lora, scaling, ids, lens)
    assert abs(loss - kats["losses"][0]) <= LOSS_TOL * kats["losses"][0]
    for (i, p, h), g in grads.items():
        assert ref.rel_l2(g, kats[f"grad.{i}.{p}.{h}"]) <= GRAD_TOL, (i, p, h)
    _, g2 = ref.loss_and_grads(sd, cfg, lora, scaling, ids, lens, expand=True)          # the second attention formulation
    assert max(ref.rel_l2(g2[k], grads[k]) for k in grads) <= 1e-5
    losses, norms, params = ref.train(sd, cfg, lora, scaling, ids, lens, 3, float(kats["lr"]))
    assert np.allclose(losses, kats["losses"][:3], rtol=2e-6, atol=0) and np.allclose(norms, kats["grad_norms"], rtol=1e-5, atol=0)
    for (i, p), (a, b) in params.items():
        for h, now, was in (("A", a, lora[(i, p)][0]), ("B", b, lora[(i, p)][1])):
            assert ref.rel_l2(now - was, kats[f"delta.{i}.{p}.{h}"].astype(np.float32)) <= DELTA_TOL, (i, p, h)


def test_targets_and_padding():
    from astts.llm.train import next_token_targets
    ids = torch.tensor([[5, 6, 7, 8], [9, 10, 0, 0], [11, 0, 0, 0]])
    t = next_token_targets(ids, torch.tensor([4, 2, 1]))
    assert t.dtype == torch.int32 and t.tolist() == [[6, 7, 8, -1], [10, -1, -1, -1], [-1, -1, -1, -1]]


def test_save_adapter_round_trip(tmp_path):
    from astts.llm.config import LlamaShape
    from astts.llm.peft import PROJ, load_adapter
    from astts.llm.train import init_lora, save_adapter
    cfg = LlamaShape.tiny()
    ad = init_lora(cfg, 8, 128.0, seed=42, base_model_name_or_path="meta-llama/Llama-3.2-3B-Instruct")
    again = init_lora(cfg, 8, 128.0, seed=42)
    for k, (a, b) in ad.pairs.items():                                   # peft's init: B = 0, A uniform within 1 / sqrt(in), seeded
        assert not b.any() and torch.equal(a, again.pairs[k][0]) and float(a.abs().max()) <= 1 / math.sqrt(a.shape[1]) and a.std() > 0
        ad.pairs[k] = (a, torch.randn(b.shape, generator=torch.Generator().manual_seed(1)))
    d = str(tmp_path / "adapter")
    save_adapter(ad, d)
    back = load_adapter(d)
    assert back.r == 8 and back.lora_alpha == 128.0 and back.scaling == 16.0 and back.targets == tuple(PROJ)
    assert back.base_model_name_or_path == "meta-llama/Llama-3.2-3B-Instruct" and set(back.pairs) == set(ad.pairs)
    for k, (a, b) in ad.pairs.items():
        assert torch.equal(back.pairs[k][0], a) and torch.equal(back.pairs[k][1], b)
    conf = json.load(open(os.path.join(d, "adapter_config.json")))
    for key, val in (("peft_type", "LORA"), ("task_type", "CAUSAL_LM"), ("r", 8), ("lora_alpha", 128.0), ("bias", "none"),
                     ("use_rslora", False), ("use_dora", False), ("fan_in_fan_out", False), ("modules_to_save", None)):
        assert conf[key] == val, key
    assert sorted(conf["target_modules"]) == sorted(PROJ)
    from safetensors.torch import load_file
    keys = set(load_file(os.path.join(d, "adapter_model.safetensors")))
    assert keys == {f"base_model.model.model.layers.{i}.{full}.lora_{h}.weight" for i in range(cfg.layers) for full in PROJ.values() for h in "AB"}


def test_cli_parser_matches_reference():
    from astts.cli import ft_llm
    a = ft_llm.build_parser().parse_args([])
    want = dict(do_train=False, do_eval_test=False, do_eval_dev=False, ft_model_path=None, ft_model_id=None, prompting_type="spdescV2",
                base_model_id="meta-llama/Llama-2-7b-hf", epoch=None, max_steps=None, lr=2e-4, seed=42, kshot=0, lora_r=32, window=5,
                max_seq_len=None, data_name="iemocap", data_folder="./data/", output_folder="./finetuned_llm/", allow_random_init=False)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    assert (ft_llm.BATCH, ft_llm.ACCUM, ft_llm.LORA_ALPHA) == (4, 4, 128.0)
    a = ft_llm.build_parser().parse_args("--do_train --data_name meld --kshot 2 --window 3 --prompting_type fewshot".split())
    assert ft_llm.split_path(a, "valid") == "./data//meld.valid.2shot_w3_fewshot.jsonl"


def test_second_library_header_exports_ctypes():
    from astts import _lib, _lib_train
    text = re.sub(r"/\*.*?\*/", "", open(_lib_train.HEADER_PATH).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(astts_[a-z0-9_]+)\s*\(", text)))
    assert names and all(n.startswith("astts_train_") for n in names)
    assert set(_lib_train.declared_symbols()) == set(names), "a prototype escaped the parser"
    assert os.path.exists(_lib_train.LIB_PATH), "libastts_train.so not built: run __graft_entry__.build()"
    raw = ctypes.CDLL(_lib_train.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    lib = _lib_train.load()
    assert lib.astts_train_abi_version() == 1 and lib.astts_train_last_error_string() is not None
    assert lib.astts_train_lora_grad_row_split() == 256
    for need in ("attn_gqa_bwd", "rmsnorm_bwd", "swiglu_bwd", "xent_grad", "lora_grad", "sumsq", "adamw"):
        assert f"astts_train_{need}" in names
    sig = _lib_train.signatures()["astts_train_adamw"]
    assert sig[0] is ctypes.c_int32 and sig[1][:4] == [ctypes.c_void_p] * 4 and sig[1][4] is ctypes.c_int64 and sig[1][-1] is ctypes.c_void_p
    # host-side argument checks answer without a GPU, with the main ABI's codes and a message
    assert lib.astts_train_adamw(None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 1.0, None) == _lib.ERR_INVALID
    assert sig[1][5:13] == [ctypes.c_double] * 8
    assert b"adamw" in lib.astts_train_last_error_string()
    # the main library keeps its own names (89 since astts_knn_route), ABI 6, none of the new ones
    main = _lib.declared_symbols()
    assert len(main) == 89 and not [n for n in main if n.startswith("astts_train_")]
    assert _lib.load().astts_abi_version() == 6
    assert not any(fn.endswith(".h") and "train" in fn for fn in os.listdir(os.path.join(ROOT, "include")))


def test_lr_schedule_and_accumulation_arithmetic():
    from astts.cli.ft_llm import plan_steps
    from astts.llm.train import clip_multiplier, lr_at, warmup_steps
    assert warmup_steps(100) == 3 and warmup_steps(10) == 1 and warmup_steps(0) == 0
    assert [lr_at(s, 2e-4, 100) for s in range(5)] == [0.0, 2e-4 / 3, 2e-4 * 2 / 3, 2e-4, 2e-4]      # transformers: step 0 runs at 0
    assert lr_at(0, 2e-4, 100, ratio=0.0) == 2e-4
    sched = torch.optim.lr_scheduler.LambdaLR(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=2e-4),
                                              lambda s: 1.0 if s >= 3 else s / 3)                    # get_constant_schedule_with_warmup
    for s in range(6):
        assert abs(sched.get_last_lr()[0] - lr_at(s, 2e-4, 100)) < 1e-18
        sched.optimizer.step()
        sched.step()
    assert clip_multiplier(0.1) == 1.0 and abs(clip_multiplier(3.0) - 0.3 / (3.0 + 1e-6)) < 1e-15
    assert plan_steps(100, None, 7) == (7, 25) and plan_steps(100, 2, None) == (14, 25) and plan_steps(100, 2, -1) == (14, 25)
    assert plan_steps(3, 1, None) == (1, 1)


def test_accumulated_gradient_is_the_big_batch_gradient(tiny, kats):
    """What LoraTrainer.accumulate does, in the restatement: micro-batch token-loss SUMS over the whole step's target count."""
    cfg, sd, lora, ids, lens = tiny
    scaling = float(kats["lora_alpha"]) / int(kats["r"])
    _, whole = ref.loss_and_grads(sd, cfg, lora, scaling, ids, lens)
    total = int((lens - 1).sum())
    acc = None
    for sl in (slice(0, 2), slice(2, 3)):
        n = int((lens[sl] - 1).sum())
        _, g = ref.loss_and_grads(sd, cfg, lora, scaling, ids[sl], lens[sl], loss_scale=n / total)
        g = {k: v * (n / total) for k, v in g.items()}                     # loss_and_grads divides the scale out again
        acc = g if acc is None else {k: acc[k] + g[k] for k in g}
    assert max(ref.rel_l2(acc[k], whole[k]) for k in whole) <= 1e-5
