"""Generates tests/golden/llama_hd64.npz and llama_hd64_train.npz: inputs and expected outputs of the Llama decoder at head dimension 64
(Llama-3.2-1B's geometry in its smallest form: LlamaShape.tiny64(), 8 / 2 heads of 64, llama3 RoPE, tied head), produced on the CPU in
fp32 by transformers' LlamaForCausalLM with eager attention on the seeded weights of make_llama_weights(LlamaShape.tiny64()).  No real
checkpoint exists where this runs and peft is not installed: the LoRA branch of the training record is added by its explicit formula
``W x + (lora_alpha / r) * B (A x)`` (as tests/golden/make_qwen2_fixtures.py does).

Recorded: a right-padded batch of 130, 64 and 5 tokens; of every row the last-layer hidden states of its real positions, the mean-pooled
embedding, the last position's logits, an 8-token greedy continuation and the token log-probabilities; and, with a seeded LoRA (r = 8,
non-zero B) on all seven projections, the mean next-token loss and every dA, dB.  Only seeds travel: weights, batch and LoRA regenerate
from them (tests/llama_hd64_ref.py).  Two files, each under 1 MiB: the forward pass in full fp32, the loss and the gradients as fp32
with the low 8 mantissa bits cleared (16 mantissa bits, relative error 2^-16).

The batch seed is the one of llama_hd64_ref.BATCH_SEEDS whose greedy continuations have the largest smallest top-2 logit margin in this
fp32 run; the script asserts that this margin is at least 5 x the largest absolute logit error of the fp16-rounded restatement along
those continuations (widen BATCH_SEEDS if no seed meets that), so rounding cannot change a recorded token.

The script then runs the restatement of tests/llama_hd64_ref.py against what it wrote: in fp32 (must reproduce the file) and with fp16
rounding at the points where the GPU path holds fp16.  The printed errors of the second run are the "emulated" column of DESIGN.md
section 2 "Head dimension 64"; every GPU bound of tests/test_llm_hd64_gpu.py is 4 x its emulated error.

Run on the build machine only (python tests/golden/make_llama_hd64_fixtures.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.join(ROOT, "tests")]

from transformers import LlamaForCausalLM  # noqa: E402

import llama_hd64_ref as ref  # noqa: E402
from astts.llm.config import LlamaShape  # noqa: E402
from astts.llm.peft import PROJ  # noqa: E402
from astts.llm.weights import make_llama_weights  # noqa: E402


class LoraLinear(torch.nn.Module):
    def __init__(self, base: torch.nn.Linear, a: torch.Tensor, b: torch.Tensor, scaling: float):
        super().__init__()
        self.base, self.scaling = base, scaling
        self.lora_A, self.lora_B = torch.nn.Parameter(a.clone()), torch.nn.Parameter(b.clone())

    def forward(self, x):
        return self.base(x) + self.scaling * ((x @ self.lora_A.t()) @ self.lora_B.t())


def trunc24(x: torch.Tensor) -> np.ndarray:
    return (x.detach().float().contiguous().numpy().view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)


def continuations(model, cfg, ids, lens):
    """-> (tokens [B, GEN_LEN], top-1 minus top-2 logit of every generated token [B, GEN_LEN], the step logits [B, GEN_LEN, vocab])."""
    gen, margins, scores = [], [], []
    for i, n in enumerate(lens):                           # one prompt per call: no padding inside generate
        prompt = ids[i:i + 1, :int(n)]
        g = model.generate(prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=ref.GEN_LEN, do_sample=False,
                           eos_token_id=None, pad_token_id=cfg.eos_token_id, output_scores=True, return_dict_in_generate=True)
        gen.append(g.sequences[0, int(n):].numpy())
        margins.append([float(t[0] - t[1]) for t in (torch.topk(s[0], 2).values for s in g.scores)])
        scores.append(torch.stack([s[0] for s in g.scores]))
    return np.stack(gen), np.asarray(margins, np.float32), torch.stack(scores)


def main():
    torch.manual_seed(0)
    cfg = LlamaShape.tiny64()
    sd = make_llama_weights(cfg, ref.SEED)
    hf_cfg = cfg.hf_config()
    hf_cfg._attn_implementation = "eager"
    assert hf_cfg.head_dim == 64 and hf_cfg.num_attention_heads == 8 and hf_cfg.num_key_value_heads == 2
    model = LlamaForCausalLM(hf_cfg).eval().float()
    full = dict(sd)
    if cfg.tie_embeddings:
        full.setdefault("lm_head.weight", sd["model.embed_tokens.weight"])
    missing = model.load_state_dict(full, strict=True, assign=True)
    assert not missing.missing_keys and not missing.unexpected_keys, missing
    for p in model.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        best = None
        for seed in ref.BATCH_SEEDS:
            ids, lens = ref.make_batch(cfg, ref.LENS, seed)
            gen, margins, scores = continuations(model, cfg, ids, lens)
            if best is None or float(margins.min()) > float(best[2].min()):
                best = (seed, gen, margins, scores)
    batch_seed, gen, margins, scores = best
    ids, lens = ref.make_batch(cfg, ref.LENS, batch_seed)
    # the fp16-rounded restatement along the same continuations: its largest absolute logit error against this fp32 run
    worst = 0.0
    for i, n in enumerate(lens):
        toks, steps = ref.greedy(sd, cfg, ids[i, :int(n)].tolist(), ref.GEN_LEN, h16=True)
        assert toks == gen[i].tolist(), (i, toks, gen[i].tolist())
        worst = max(worst, float((steps - scores[i]).abs().max()))
    print(f"batch seed {batch_seed} of {ref.BATCH_SEEDS}: smallest top-2 margin {float(margins.min()):.4f}, largest |logit error| of the "
          f"fp16-rounded restatement {worst:.4f} (ratio {float(margins.min()) / worst:.1f})")
    assert float(margins.min()) >= 5 * worst, "no seed of BATCH_SEEDS is far enough from a tie: widen the range"
    mask = (torch.arange(ids.shape[1])[None, :] < lens[:, None]).long()
    out = {"seed": np.int64(ref.SEED), "batch_seed": np.int64(batch_seed), "lora_seed": np.int64(ref.LORA_SEED), "r": np.int64(ref.R),
           "lora_alpha": np.float64(ref.ALPHA), "ids": ids.numpy(), "lens": lens.numpy(), "greedy": gen, "greedy_margins": margins}
    with torch.no_grad():
        o = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        hs = o.hidden_states[-1]
        out["hidden"] = torch.cat([hs[i, :int(n)] for i, n in enumerate(lens)]).numpy()
        out["embedding"] = torch.stack([hs[i, :int(n)].mean(0) for i, n in enumerate(lens)]).numpy()
        out["logits_last"] = torch.stack([o.logits[i, int(n) - 1] for i, n in enumerate(lens)]).numpy()
        lp = torch.log_softmax(o.logits[:, :-1].double(), -1).gather(-1, ids[:, 1:, None])[..., 0]
        out["logprobs"] = torch.where(mask[:, 1:].bool(), lp, torch.zeros_like(lp)).float().numpy()
    # training: the LoRA branch by its formula on all seven projections, A and B the only trainable parameters
    lora = ref.make_lora(cfg, ref.R, ref.LORA_SEED)
    scaling = ref.ALPHA / ref.R
    mods = {}
    for i, layer in enumerate(model.model.layers):
        for p, full_name in PROJ.items():
            parent = getattr(layer, full_name.split(".")[0])
            m = LoraLinear(getattr(parent, p), *lora[(i, p)], scaling)
            setattr(parent, p, m)
            mods[(i, p)] = m
    labels = torch.where(mask.bool(), ids, torch.full_like(ids, -100))
    model.train()
    loss = model(input_ids=ids, attention_mask=mask, labels=labels).loss
    loss.backward()
    train = {"loss": np.float64(float(loss.detach()))}
    for (i, p), m in mods.items():
        train[f"grad.{i}.{p}.A"], train[f"grad.{i}.{p}.B"] = trunc24(m.lora_A.grad), trunc24(m.lora_B.grad)
    path = os.path.join(ROOT, "tests", "golden", "llama_hd64.npz")
    np.savez_compressed(path, **out)
    np.savez_compressed(path.replace(".npz", "_train.npz"), **train)
    sizes = (os.path.getsize(path), os.path.getsize(path.replace(".npz", "_train.npz")))
    assert max(sizes) < 1 << 20, sizes
    print("->", path, sizes[0] // 1024, "KB and", sizes[1] // 1024, "KB; loss", float(train["loss"]), "; greedy", out["greedy"].tolist())
    report(path)


def report(path):
    """The restatement against the file: fp32 (reproduces it) and fp16-rounded (the emulated error of every GPU bound)."""
    fx = {**np.load(path), **np.load(path.replace(".npz", "_train.npz"))}
    cfg = LlamaShape.tiny64()
    sd = make_llama_weights(cfg, int(fx["seed"]))
    ids, lens = torch.from_numpy(fx["ids"]), torch.from_numpy(fx["lens"])
    lora = ref.make_lora(cfg, int(fx["r"]), int(fx["lora_seed"]))
    scaling = float(fx["lora_alpha"]) / int(fx["r"])
    for h16 in (False, True):
        got = ref.outputs(sd, cfg, ids, lens, h16=h16)
        errs = {k: ref.rel_l2(got[k], fx[k]) for k in ("hidden", "embedding", "logits_last", "logprobs")}
        loss, grads = ref.loss_and_grads(sd, cfg, lora, scaling, ids, lens, h16=h16)
        errs["loss"] = abs(loss - float(fx["loss"])) / float(fx["loss"])
        worst = max(((ref.rel_l2(g, fx[f"grad.{i}.{p}.{h}"]), (i, p, h)) for (i, p, h), g in grads.items()))
        errs["grad (worst)"] = worst[0]
        toks = [ref.greedy(sd, cfg, ids[i, :int(n)].tolist(), ref.GEN_LEN, h16=h16)[0] for i, n in enumerate(lens)]
        print(("fp16-rounded" if h16 else "fp32") + " restatement vs the fixture (relative L2): " +
              ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" at {worst[1]}; greedy equal: {toks == fx['greedy'].tolist()}")


if __name__ == "__main__":
    main()
