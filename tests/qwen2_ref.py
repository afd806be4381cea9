"""Restatement of the Qwen2 decoder (transformers' Qwen2ForCausalLM: Llama with a bias on the q / k / v projections, plain RoPE and an
untied head) in plain torch, for inference, LLM.int8 + LoRA and LoRA fine-tuning (DESIGN.md section 2 "Qwen2").  Uses only torch and
safetensors and the helpers of tests/llm_train_ref.py (attention, rope, rmsnorm, the fp16 rounding with a rounded gradient) and
tests/llm_int8_ref.py (the LLM.int8 linear, the adapter writer), so the GPU tests call it live.

One function, ``hidden``, runs a right-padded batch through the layer stack with a pluggable linear:

    fp_linear(...)        ``W x + b + scaling * B (A x)``; ``h16=True`` rounds the weights, the LoRA operands and the rank activations to
                          fp16 as the GPU path holds them (the bias stays fp32: it is added in the GEMM's fp32 epilogue)
    int8_linear(...)      LLM.int8 by segment (llm_int8_ref.make_linear) + the fp32 bias + the unmerged LoRA branch

``h16=True`` rounds (value and gradient) where the GPU path stores fp16: the norm outputs, q | k | v after the bias and again after RoPE,
q * scale * log2 e and P inside the attention, the attention output, gate | up, the SwiGLU product and the final hidden states where
they become the head GEMM's operand.  The fp32 run reproduces tests/golden/qwen2_tiny.npz (tests/test_qwen2_cpu.py); the error of the
fp16-rounded run against that fixture is what the GPU bounds are made of (tests/golden/make_qwen2_fixtures.py prints it)."""
from __future__ import annotations

import json
import os
import sys
from typing import Callable, Optional

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import llm_int8_ref as i8  # noqa: E402
from llm_train_ref import _rnd, attention, leaves, make_batch, make_lora, rel_l2, rmsnorm, rope  # noqa: E402,F401
from astts.llm.peft import PROJ  # noqa: E402

SEED, BATCH_SEED, LORA_SEED, R, ALPHA, LENS, GEN_LEN = 21, 38, 23, 8, 32.0, (130, 64, 5), 8
BIASED = ("q_proj", "k_proj", "v_proj")


def inv_freq(cfg) -> torch.Tensor:
    """Plain RoPE, float32 as transformers computes it."""
    assert cfg.rope_type == "default", cfg.rope_type
    return 1.0 / (cfg.rope_theta ** (torch.arange(0, cfg.head_dim, 2, dtype=torch.float) / cfg.head_dim))


def _bias(sd, i: int, p: str):
    return sd[f"model.layers.{i}.{PROJ[p]}.bias"] if p in BIASED else None


def fp_linear(sd, cfg, lora=None, scaling: float = 1.0, h16: bool = False) -> Callable:
    """lin(i, module, x [B, T, K], seg) -> y.  ``lora``: (layer, module) -> (A, B), unmerged."""
    W = (lambda k: sd[k].half().float()) if h16 else (lambda k: sd[k])

    def lin(i, p, x, seg):
        y = x @ W(f"model.layers.{i}.{PROJ[p]}.weight").t()
        b = _bias(sd, i, p)
        if b is not None:
            y = y + b
        ab = None if lora is None else lora.get((i, p))
        if ab is not None:
            t = _rnd(x @ _rnd(ab[0], h16).t(), h16)
            y = y + t @ _rnd(ab[1] * scaling, h16).t()
        return y

    return lin


def int8_linear(sd, cfg, lora=None, scaling: float = 1.0, tau: float = 6.0) -> Callable:
    """The LLM.int8 linear of llm_int8_ref (fp32 arithmetic) with Qwen2's bias on top.  ``lora`` keyed (layer, module)."""
    short = None if lora is None else {(i, p[:-5]): ab for (i, p), ab in lora.items()}
    base = i8.make_linear(sd, cfg, short, scaling, int8=True, tau=tau)

    def lin(i, p, x, seg):
        y = base(p[:-5], i, x.reshape(-1, x.shape[-1]), seg).view(*x.shape[:-1], -1)
        b = _bias(sd, i, p)
        return y if b is None else y + b

    return lin


def segments(lens, t: int) -> torch.Tensor:
    """The LLM.int8 segment of every row of a right-padded [B, T] batch, flat: the text's index, -1 on padding."""
    return torch.tensor([b if i < int(n) else -1 for b, n in enumerate(lens) for i in range(t)], dtype=torch.long)


def hidden(sd, cfg, lin: Callable, ids: torch.Tensor, lens: torch.Tensor, h16: bool = False) -> torch.Tensor:
    """ids [B, T] right-padded, lens [B] -> final-norm hidden states fp32 [B, T, hidden] (== hidden_states[-1] of Qwen2Model on the
    real positions; padding rows hold finite values that nothing reads)."""
    b, t = ids.shape
    fr = torch.arange(t, dtype=torch.float32)[:, None] * inv_freq(cfg)[None, :]
    cos, sin = fr.cos(), fr.sin()
    seg = segments(lens, t)
    x = sd["model.embed_tokens.weight"][ids]
    for i in range(cfg.layers):
        pre = f"model.layers.{i}."
        h1 = _rnd(rmsnorm(x, sd[pre + "input_layernorm.weight"], cfg.rms_eps), h16)
        q = _rnd(lin(i, "q_proj", h1, seg), h16).view(b, t, cfg.heads, cfg.head_dim)
        k = _rnd(lin(i, "k_proj", h1, seg), h16).view(b, t, cfg.kv_heads, cfg.head_dim)
        v = _rnd(lin(i, "v_proj", h1, seg), h16).view(b, t, cfg.kv_heads, cfg.head_dim)
        q, k = _rnd(rope(q, cos, sin), h16), _rnd(rope(k, cos, sin), h16)
        ao = _rnd(attention(q, k, v, lens, cfg.heads, cfg.kv_heads, h16=h16), h16)
        x = x + lin(i, "o_proj", ao, seg)
        h2 = _rnd(rmsnorm(x, sd[pre + "post_attention_layernorm.weight"], cfg.rms_eps), h16)
        gate, up = _rnd(lin(i, "gate_proj", h2, seg), h16), _rnd(lin(i, "up_proj", h2, seg), h16)
        x = x + lin(i, "down_proj", _rnd(torch.nn.functional.silu(gate) * up, h16), seg)
    return rmsnorm(x, sd["model.norm.weight"], cfg.rms_eps)


def logits(sd, cfg, hf: torch.Tensor, h16: bool = False) -> torch.Tensor:
    head = sd["model.embed_tokens.weight" if cfg.tie_embeddings else "lm_head.weight"]
    return _rnd(hf, h16) @ (head.half().float() if h16 else head).t()


def pooled(hf: torch.Tensor, lens) -> torch.Tensor:
    return torch.stack([hf[i, :int(n)].mean(0) for i, n in enumerate(lens)])


def token_logprobs(sd, cfg, hf, ids, lens, h16: bool = False) -> torch.Tensor:
    """[B, T - 1]: log p(token t + 1 | tokens <= t) on the real positions, 0 on padding (LlamaEmbedder.token_logprobs)."""
    lp = torch.log_softmax(logits(sd, cfg, hf[:, :-1], h16).double(), -1).gather(-1, ids[:, 1:, None])[..., 0]
    take = torch.arange(1, ids.shape[1])[None, :] < torch.as_tensor(lens)[:, None]
    return torch.where(take, lp, torch.zeros_like(lp)).float()


def outputs(sd, cfg, lin, ids, lens, h16: bool = False) -> dict:
    """What the fixture records of one forward pass: hidden states of the real positions (rows concatenated), the mean-pooled
    embedding, the last position's logits and the token log-probabilities."""
    with torch.no_grad():
        hf = hidden(sd, cfg, lin, ids, lens, h16)
        last = torch.stack([hf[i, int(n) - 1] for i, n in enumerate(lens)])
        return {"hidden": torch.cat([hf[i, :int(n)] for i, n in enumerate(lens)]), "embedding": pooled(hf, lens),
                "logits_last": logits(sd, cfg, last, h16), "logprobs": token_logprobs(sd, cfg, hf, ids, lens, h16)}


def greedy(sd, cfg, lin, prompt, n_new: int, h16: bool = False):
    """Greedy continuation with the prompt re-run for every token -> (new tokens, top-1 minus top-2 logit per step)."""
    out, margins = [int(i) for i in prompt], []
    with torch.no_grad():
        for _ in range(n_new):
            ids = torch.tensor([out])
            lg = logits(sd, cfg, hidden(sd, cfg, lin, ids, torch.tensor([len(out)]), h16)[0, -1], h16)
            top = torch.topk(lg, 2).values
            margins.append(float(top[0] - top[1]))
            out.append(int(torch.argmax(lg)))
    return out[len(prompt):], margins


def model_loss(sd, cfg, lora, scaling: float, ids, lens, h16: bool = False, loss_scale: float = 1.0):
    """Mean next-token cross-entropy over the real targets (times ``loss_scale``); ``lora``: leaf tensors for the gradients."""
    b, t = ids.shape
    hf = hidden(sd, cfg, fp_linear(sd, cfg, lora, scaling, h16), ids, lens, h16)
    lg = logits(sd, cfg, hf, h16)
    pos = torch.arange(t)[None, :]
    tgt = torch.where(pos + 1 < lens[:, None], torch.cat([ids[:, 1:], ids[:, :1]], 1), torch.full_like(ids, -100))
    return torch.nn.functional.cross_entropy(lg.reshape(b * t, -1), tgt.reshape(-1), ignore_index=-100) * loss_scale


def loss_and_grads(sd, cfg, lora, scaling, ids, lens, h16=False, loss_scale=1.0):
    """-> (loss, {(layer, module, "A" | "B"): gradient}) with the loss scale divided out again."""
    lv = leaves(lora)
    loss = model_loss(sd, cfg, lv, scaling, ids, lens, h16=h16, loss_scale=loss_scale)
    loss.backward()
    grads = {}
    for (i, p), (a, b) in lv.items():
        grads[(i, p, "A")], grads[(i, p, "B")] = a.grad / loss_scale, b.grad / loss_scale
    return float(loss.detach()) / loss_scale, grads


def merged(sd, lora, scaling: float) -> dict:
    """W + scaling * B A (fp32) for every projection with a LoRA pair (keys (layer, module))."""
    out = dict(sd)
    for (i, p), (a, b) in lora.items():
        k = f"model.layers.{i}.{PROJ[p]}.weight"
        out[k] = sd[k] + scaling * (b @ a)
    return out


def config_json(cfg) -> dict:
    """The keys of a Qwen2.5 checkpoint's config.json (as saved by transformers 4.x: rope_theta at the top, no rope_scaling)."""
    assert cfg.model_type == "qwen2"
    return {"architectures": ["Qwen2ForCausalLM"], "model_type": "qwen2", "vocab_size": cfg.vocab, "hidden_size": cfg.hidden,
            "intermediate_size": cfg.ffn, "num_hidden_layers": cfg.layers, "num_attention_heads": cfg.heads,
            "num_key_value_heads": cfg.kv_heads, "hidden_act": "silu", "max_position_embeddings": cfg.max_positions,
            "rms_norm_eps": cfg.rms_eps, "rope_theta": cfg.rope_theta, "rope_scaling": None, "use_sliding_window": False,
            "sliding_window": 131072, "max_window_layers": cfg.layers, "tie_word_embeddings": cfg.tie_embeddings,
            "attention_dropout": 0.0, "bos_token_id": cfg.bos_token_id, "eos_token_id": cfg.eos_token_id, "torch_dtype": "float16"}


def write_base(path: str, cfg, sd: dict, eos_ids=None, config: Optional[dict] = None) -> str:
    """A Qwen2 checkpoint directory: config.json, generation_config.json, model.safetensors (fp16 as saved, biases included)."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(config if config is not None else config_json(cfg), f)
    with open(os.path.join(path, "generation_config.json"), "w") as f:
        json.dump({"bos_token_id": cfg.bos_token_id, "eos_token_id": eos_ids if eos_ids is not None else cfg.eos_token_id}, f)
    save_file({k: v.to(torch.float16).contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    return path


def write_adapter(path: str, lora: dict, r: int, alpha: float, base: str = "Qwen/Qwen2.5-7B-Instruct") -> str:
    """A peft adapter directory (llm_int8_ref.write_adapter) from a LoRA keyed (layer, module)."""
    return i8.write_adapter(path, {(i, p[:-5]): ab for (i, p), ab in lora.items()}, r, alpha, base=base)
