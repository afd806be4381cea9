"""Generates tests/golden/qwen2_tiny.npz and qwen2_tiny_train.npz: inputs and expected outputs of the Qwen2 track of the LLM (the reference's src/ft_llm_cn.py,
src/evaluate_base_model_cn.py and src/llm_bio_extract_cn.py run Qwen2.5-7B-Instruct), produced on the CPU in fp32 by the third-party
implementation they call -- transformers' Qwen2ForCausalLM -- on the seeded weights of make_llama_weights(LlamaShape.qwen2_tiny()).
No real Qwen2.5 checkpoint exists where this runs, and neither peft nor bitsandbytes is installed: the LoRA branch of the training
record is added by its explicit formula ``W x + b + (lora_alpha / r) * B (A x)`` (as tests/golden/make_lora_train_fixtures.py does),
and nothing here is quantised.

Recorded: a right-padded batch of 130, 64 and 5 tokens; of every row the last-layer hidden states of its real positions, the mean-pooled
embedding, the last position's logits, an 8-token greedy continuation and the token log-probabilities; and, with a seeded LoRA (r = 8,
non-zero B) on all seven projections, the mean next-token loss and every dA, dB.  Only seeds travel: weights, batch and LoRA regenerate
from them (tests/qwen2_ref.py).  The repository's limit is 1 MiB per file, so the record is two files: the forward pass in full fp32 in
qwen2_tiny.npz, the loss and the gradients in qwen2_tiny_train.npz, the gradients as fp32 with the low 8 mantissa bits cleared (relative
error 2^-16, as lora_train_kats.npz stores them).  The batch seed is the one of 22 .. 39 whose greedy continuations have the largest
smallest top-2 logit margin in this fp32 run (0.077, against an fp16 error of ~0.007 per logit): a continuation that rounding cannot
change, chosen from the reference's own numbers.

The script then runs the restatement of tests/qwen2_ref.py against what it wrote: in fp32 (must reproduce the file) and with fp16
rounding at the points where the GPU path holds fp16.  The printed errors of the second run are the "emulated" column of DESIGN.md
section 2 "Qwen2"; every GPU bound of tests/test_qwen2_gpu.py is 4 x its emulated error.

Run in the BUILD container only (python tests/golden/make_qwen2_fixtures.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.join(ROOT, "tests")]

from transformers import Qwen2ForCausalLM  # noqa: E402

import qwen2_ref as ref  # noqa: E402
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


def main():
    torch.manual_seed(0)
    cfg = LlamaShape.qwen2_tiny()
    sd = make_llama_weights(cfg, ref.SEED)
    hf_cfg = cfg.hf_config()
    hf_cfg._attn_implementation = "eager"
    model = Qwen2ForCausalLM(hf_cfg).eval().float()
    missing = model.load_state_dict(sd, strict=True, assign=True)
    assert not missing.missing_keys and not missing.unexpected_keys, missing
    for p in model.parameters():
        p.requires_grad_(False)
    ids, lens = ref.make_batch(cfg, ref.LENS, ref.BATCH_SEED)
    mask = (torch.arange(ids.shape[1])[None, :] < lens[:, None]).long()
    out = {"seed": np.int64(ref.SEED), "batch_seed": np.int64(ref.BATCH_SEED), "lora_seed": np.int64(ref.LORA_SEED), "r": np.int64(ref.R),
           "lora_alpha": np.float64(ref.ALPHA), "ids": ids.numpy(), "lens": lens.numpy()}
    with torch.no_grad():
        o = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        hs = o.hidden_states[-1]
        out["hidden"] = torch.cat([hs[i, :int(n)] for i, n in enumerate(lens)]).numpy()
        out["embedding"] = torch.stack([hs[i, :int(n)].mean(0) for i, n in enumerate(lens)]).numpy()
        out["logits_last"] = torch.stack([o.logits[i, int(n) - 1] for i, n in enumerate(lens)]).numpy()
        lp = torch.log_softmax(o.logits[:, :-1].double(), -1).gather(-1, ids[:, 1:, None])[..., 0]
        out["logprobs"] = torch.where(mask[:, 1:].bool(), lp, torch.zeros_like(lp)).float().numpy()
        gen, margins = [], []
        for i, n in enumerate(lens):                       # one prompt per call: no padding inside generate
            prompt = ids[i:i + 1, :int(n)]
            g = model.generate(prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=ref.GEN_LEN, do_sample=False,
                               eos_token_id=None, pad_token_id=cfg.eos_token_id, output_scores=True, return_dict_in_generate=True)
            gen.append(g.sequences[0, int(n):].numpy())
            margins.append([float(t[0] - t[1]) for t in (torch.topk(s[0], 2).values for s in g.scores)])
        out["greedy"] = np.stack(gen)
        out["greedy_margins"] = np.asarray(margins, np.float32)       # top-1 minus top-2 logit of every generated token
    # training: the LoRA branch by its formula on all seven projections, A and B the only trainable parameters
    lora = ref.make_lora(cfg, ref.R, ref.LORA_SEED)
    scaling = ref.ALPHA / ref.R
    mods = {}
    for i, layer in enumerate(model.model.layers):
        for p, full in PROJ.items():
            parent = getattr(layer, full.split(".")[0])
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
    path = os.path.join(ROOT, "tests", "golden", "qwen2_tiny.npz")
    np.savez_compressed(path, **out)
    np.savez_compressed(path.replace(".npz", "_train.npz"), **train)
    print("->", path, os.path.getsize(path) // 1024, "KB and", os.path.getsize(path.replace(".npz", "_train.npz")) // 1024, "KB; loss",
          float(train["loss"]), "; greedy", out["greedy"].tolist(), "; smallest top-2 margin", float(out["greedy_margins"].min()))
    report(path)


def report(path):
    """The restatement against the file: fp32 (reproduces it) and fp16-rounded (the emulated error of every GPU bound)."""
    fx = {**np.load(path), **np.load(path.replace(".npz", "_train.npz"))}
    cfg = LlamaShape.qwen2_tiny()
    sd = make_llama_weights(cfg, int(fx["seed"]))
    ids, lens = torch.from_numpy(fx["ids"]), torch.from_numpy(fx["lens"])
    lora = ref.make_lora(cfg, int(fx["r"]), int(fx["lora_seed"]))
    scaling = float(fx["lora_alpha"]) / int(fx["r"])
    for h16 in (False, True):
        got = ref.outputs(sd, cfg, ref.fp_linear(sd, cfg, h16=h16), ids, lens, h16=h16)
        errs = {k: ref.rel_l2(got[k], fx[k]) for k in ("hidden", "embedding", "logits_last", "logprobs")}
        loss, grads = ref.loss_and_grads(sd, cfg, lora, scaling, ids, lens, h16=h16)
        errs["loss"] = abs(loss - float(fx["loss"])) / float(fx["loss"])
        worst = max(((ref.rel_l2(g, fx[f"grad.{i}.{p}.{h}"]), (i, p, h)) for (i, p, h), g in grads.items()))
        errs["grad (worst)"] = worst[0]
        toks = [ref.greedy(sd, cfg, ref.fp_linear(sd, cfg, h16=h16), ids[i, :int(n)].tolist(), ref.GEN_LEN, h16=h16)[0] for i, n in enumerate(lens)]
        print(("fp16-rounded" if h16 else "fp32") + " restatement vs the fixture (relative L2): " +
              ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" at {worst[1]}; greedy equal: {toks == fx['greedy'].tolist()}")


if __name__ == "__main__":
    main()
