"""Restatement of the Llama decoder in plain torch for the head-dimension-64 models (LlamaShape.tiny64 / wide64; DESIGN.md section 2
"Head dimension 64"): tests/qwen2_ref.py's layer stack with the RoPE frequencies ``cfg.rope_type`` names (Llama-3 scaled or plain) and
a q | k | v bias only where ``cfg.qkv_bias`` says so.  Everything is written in ``cfg.head_dim``; the helpers are those of
tests/llm_train_ref.py (attention, rope, rmsnorm, the fp16 rounding with a rounded gradient) and tests/qwen2_ref.py (logits, pooling,
token log-probabilities).  ``h16=True`` rounds where the GPU path stores fp16, exactly as qwen2_ref does.  The fp32 run reproduces
tests/golden/llama_hd64.npz (tests/test_llm_hd64_cpu.py); the error of the fp16-rounded run against that fixture is what the GPU
bounds of tests/test_llm_hd64_gpu.py are made of (tests/golden/make_llama_hd64_fixtures.py prints it)."""
from __future__ import annotations

import os
import sys
from typing import Callable

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import qwen2_ref as q2  # noqa: E402
from llm_train_ref import _rnd, attention, leaves, make_batch, make_lora, rel_l2, rmsnorm, rope  # noqa: E402,F401
from astts.llm.decoder import inv_freq  # noqa: E402
from astts.llm.peft import PROJ  # noqa: E402

SEED, LORA_SEED, R, ALPHA, LENS, GEN_LEN = 31, 33, 8, 32.0, (130, 64, 5), 8
BATCH_SEEDS = range(40, 64)           # the generator keeps the one whose greedy continuations are least near a tie


def fp_linear(sd, cfg, lora=None, scaling: float = 1.0, h16: bool = False) -> Callable:
    """lin(i, module, x [B, T, K]) -> ``W x (+ b) + scaling * B (A x)``; ``lora``: (layer, module) -> (A, B), unmerged."""
    W = (lambda k: sd[k].half().float()) if h16 else (lambda k: sd[k])

    def lin(i, p, x):
        y = x @ W(f"model.layers.{i}.{PROJ[p]}.weight").t()
        if cfg.qkv_bias and p in q2.BIASED:
            y = y + sd[f"model.layers.{i}.{PROJ[p]}.bias"]
        ab = None if lora is None else lora.get((i, p))
        if ab is not None:
            t = _rnd(x @ _rnd(ab[0], h16).t(), h16)
            y = y + t @ _rnd(ab[1] * scaling, h16).t()
        return y

    return lin


def hidden(sd, cfg, lin: Callable, ids: torch.Tensor, lens: torch.Tensor, h16: bool = False) -> torch.Tensor:
    """ids [B, T] right-padded, lens [B] -> final-norm hidden states fp32 [B, T, hidden] (== hidden_states[-1] of LlamaModel on the
    real positions)."""
    b, t = ids.shape
    fr = torch.arange(t, dtype=torch.float32)[:, None] * inv_freq(cfg)[None, :]
    cos, sin = fr.cos(), fr.sin()
    x = sd["model.embed_tokens.weight"][ids]
    for i in range(cfg.layers):
        pre = f"model.layers.{i}."
        h1 = _rnd(rmsnorm(x, sd[pre + "input_layernorm.weight"], cfg.rms_eps), h16)
        q = _rnd(lin(i, "q_proj", h1), h16).view(b, t, cfg.heads, cfg.head_dim)
        k = _rnd(lin(i, "k_proj", h1), h16).view(b, t, cfg.kv_heads, cfg.head_dim)
        v = _rnd(lin(i, "v_proj", h1), h16).view(b, t, cfg.kv_heads, cfg.head_dim)
        q, k = _rnd(rope(q, cos, sin), h16), _rnd(rope(k, cos, sin), h16)
        ao = _rnd(attention(q, k, v, lens, cfg.heads, cfg.kv_heads, h16=h16), h16)
        x = x + lin(i, "o_proj", ao)
        h2 = _rnd(rmsnorm(x, sd[pre + "post_attention_layernorm.weight"], cfg.rms_eps), h16)
        gate, up = _rnd(lin(i, "gate_proj", h2), h16), _rnd(lin(i, "up_proj", h2), h16)
        x = x + lin(i, "down_proj", _rnd(torch.nn.functional.silu(gate) * up, h16))
    return rmsnorm(x, sd["model.norm.weight"], cfg.rms_eps)


def outputs(sd, cfg, ids, lens, h16: bool = False) -> dict:
    """What the fixture records of one forward pass: hidden states of the real positions (rows concatenated), the mean-pooled
    embedding, the last position's logits and the token log-probabilities."""
    with torch.no_grad():
        hf = hidden(sd, cfg, fp_linear(sd, cfg, h16=h16), ids, lens, h16)
        last = torch.stack([hf[i, int(n) - 1] for i, n in enumerate(lens)])
        return {"hidden": torch.cat([hf[i, :int(n)] for i, n in enumerate(lens)]), "embedding": q2.pooled(hf, lens),
                "logits_last": q2.logits(sd, cfg, last, h16), "logprobs": q2.token_logprobs(sd, cfg, hf, ids, lens, h16)}


def greedy(sd, cfg, prompt, n_new: int, h16: bool = False):
    """Greedy continuation with the prompt re-run for every token -> (new tokens, the logits of every step [n_new, vocab])."""
    out, steps = [int(i) for i in prompt], []
    lin = fp_linear(sd, cfg, h16=h16)
    with torch.no_grad():
        for _ in range(n_new):
            lg = q2.logits(sd, cfg, hidden(sd, cfg, lin, torch.tensor([out]), torch.tensor([len(out)]), h16)[0, -1], h16)
            steps.append(lg)
            out.append(int(torch.argmax(lg)))
    return out[len(prompt):], torch.stack(steps)


def model_loss(sd, cfg, lora, scaling: float, ids, lens, h16: bool = False):
    """Mean next-token cross-entropy over the real targets; ``lora``: leaf tensors for the gradients."""
    b, t = ids.shape
    lg = q2.logits(sd, cfg, hidden(sd, cfg, fp_linear(sd, cfg, lora, scaling, h16), ids, lens, h16), h16)
    pos = torch.arange(t)[None, :]
    tgt = torch.where(pos + 1 < lens[:, None], torch.cat([ids[:, 1:], ids[:, :1]], 1), torch.full_like(ids, -100))
    return torch.nn.functional.cross_entropy(lg.reshape(b * t, -1), tgt.reshape(-1), ignore_index=-100)


def loss_and_grads(sd, cfg, lora, scaling, ids, lens, h16=False):
    """-> (loss, {(layer, module, "A" | "B"): gradient})."""
    lv = leaves(lora)
    loss = model_loss(sd, cfg, lv, scaling, ids, lens, h16=h16)
    loss.backward()
    grads = {}
    for (i, p), (a, b) in lv.items():
        grads[(i, p, "A")], grads[(i, p, "B")] = a.grad, b.grad
    return float(loss.detach()), grads
