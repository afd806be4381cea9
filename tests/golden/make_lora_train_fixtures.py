"""Generates tests/golden/lora_train_kats.npz: the loss, the LoRA gradients and three optimizer steps of LoRA fine-tuning, produced
by transformers' LlamaForCausalLM in fp32 on the seeded weights of make_llama_weights(LlamaShape.tiny()).  peft is not installed
where this runs, so the LoRA branch is added by its explicit formula: every one of the seven projections becomes
``W x + (lora_alpha / r) * B (A x)`` with A and B as the only trainable parameters (what peft's lora.Linear computes without dropout).
torch.optim.AdamW (0.9, 0.999, 1e-8, weight decay 0) with clip_grad_norm_(0.3), as src/ft_llm.py's TrainingArguments set.

Run in the BUILD container only (python tests/golden/make_lora_train_fixtures.py).  The file is data: a seed, token ids, numbers.
The weights, the LoRA and the batch regenerate from their seeds (tests/llm_train_ref.py).  To stay below the repository's 1 MiB limit
per file the gradients are stored as fp32 with the low 8 mantissa bits cleared (relative error 2^-16) and the parameters after the
third step as their fp16 difference from the initial ones; of the first two steps the file keeps the loss and the gradient norm."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.join(ROOT, "tests")]

from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

import llm_train_ref as ref  # noqa: E402
from astts.llm.config import LlamaShape  # noqa: E402
from astts.llm.peft import PROJ  # noqa: E402
from astts.llm.weights import make_llama_weights  # noqa: E402

SEED, LORA_SEED, BATCH_SEED, R, ALPHA, LENS, LR, STEPS = 0, 11, 12, 8, 32.0, (40, 17, 2), 1e-3, 3


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
    cfg = LlamaShape.tiny()
    sd = make_llama_weights(cfg, SEED)
    model = LlamaForCausalLM(LlamaConfig(**cfg.hf_kwargs(), attn_implementation="eager")).float()
    missing = model.load_state_dict(sd, strict=False, assign=True)
    model.tie_weights()
    assert set(missing.missing_keys) <= {"lm_head.weight"} and not missing.unexpected_keys, missing
    for p in model.parameters():
        p.requires_grad_(False)
    lora = ref.make_lora(cfg, R, LORA_SEED)
    scaling = ALPHA / R
    mods = {}
    for i, layer in enumerate(model.model.layers):
        for p, full in PROJ.items():
            parent = getattr(layer, full.split(".")[0])
            m = LoraLinear(getattr(parent, p), *lora[(i, p)], scaling)
            setattr(parent, p, m)
            mods[(i, p)] = m
    ids, lens = ref.make_batch(cfg, LENS, BATCH_SEED)
    mask = (torch.arange(ids.shape[1])[None, :] < lens[:, None]).long()
    labels = torch.where(mask.bool(), ids, torch.full_like(ids, -100))
    params = [t for m in mods.values() for t in (m.lora_A, m.lora_B)]
    opt = torch.optim.AdamW(params, lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    out = {"seed": np.int64(SEED), "lora_seed": np.int64(LORA_SEED), "batch_seed": np.int64(BATCH_SEED), "r": np.int64(R),
           "lora_alpha": np.float64(ALPHA), "lr": np.float64(LR), "ids": ids.numpy(), "lens": lens.numpy()}
    losses, norms = [], []
    model.train()
    for step in range(STEPS):
        opt.zero_grad()
        loss = model(input_ids=ids, attention_mask=mask, labels=labels).loss
        loss.backward()
        if step == 0:
            for (i, p), m in mods.items():
                out[f"grad.{i}.{p}.A"], out[f"grad.{i}.{p}.B"] = trunc24(m.lora_A.grad), trunc24(m.lora_B.grad)
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, 0.3)))
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(model(input_ids=ids, attention_mask=mask, labels=labels).loss))
    for (i, p), m in mods.items():
        out[f"delta.{i}.{p}.A"] = (m.lora_A.detach() - lora[(i, p)][0]).numpy().astype(np.float16)
        out[f"delta.{i}.{p}.B"] = (m.lora_B.detach() - lora[(i, p)][1]).numpy().astype(np.float16)
    out["losses"], out["grad_norms"] = np.asarray(losses, np.float64), np.asarray(norms, np.float64)   # losses: before each step + after the last
    path = os.path.join(ROOT, "tests", "golden", "lora_train_kats.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path) // 1024, "KB; losses", losses, "norms", norms)
    # the restatement the tests run, against the third-party numbers just written
    l0, g = ref.loss_and_grads(sd, cfg, lora, scaling, ids, lens)
    worst = max(ref.rel_l2(g[(i, p, h)], torch.from_numpy(out[f"grad.{i}.{p}.{h}"])) for (i, p) in mods for h in "AB")
    print("restatement: loss", l0, "vs", losses[0], "; worst gradient rel L2", worst)


if __name__ == "__main__":
    main()
