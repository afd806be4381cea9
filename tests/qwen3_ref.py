"""Restatement of the Qwen3 decoder (transformers' Qwen3ForCausalLM: Qwen2 without the q / k / v bias, with an RMSNorm over head_dim on
every q and k head before RoPE, and a head_dim that is a config key of its own) in plain torch, for inference, LLM.int8 + LoRA and LoRA
fine-tuning (DESIGN.md section 2 "Qwen3").  Uses only torch and safetensors and the helpers of tests/qwen2_ref.py, tests/llm_train_ref.py
and tests/llm_int8_ref.py, so the GPU tests call it live.

``qknorm_rope`` is the operator astts_op_qknorm_rope computes (include/llm/astts_qknorm.h), in whatever dtype it is given: the operator
tests run it in fp64.  ``hidden`` runs a right-padded batch through the layer stack with a pluggable linear, as qwen2_ref.hidden does.

``h16=True`` rounds (value and gradient) where the GPU path stores fp16: the norm outputs, q | k | v after the GEMM, ONCE MORE after
norm + rotation (the fused kernel computes both in fp32 and rounds at its store; its transpose rounds d(pre-norm q | k) once), and the
rest as qwen2_ref: q * scale * log2 e and P inside the attention, the attention output, gate | up, the SwiGLU product and the final
hidden states where they become the head GEMM's operand.  The fp32 run reproduces tests/golden/qwen3_tiny.npz (tests/test_qwen3_cpu.py);
the error of the fp16-rounded run against that fixture is what the GPU bounds are made of (tests/golden/make_qwen3_fixtures.py prints it)."""
from __future__ import annotations

import os
import sys
from typing import Callable, Optional

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import llm_int8_ref as i8  # noqa: E402
import qwen2_ref as q2  # noqa: E402
from qwen2_ref import (_rnd, attention, inv_freq, leaves, logits, make_batch, make_lora, merged, pooled, rel_l2, rmsnorm, rope,  # noqa: E402,F401
                       segments, token_logprobs, write_adapter)
from astts.llm.peft import PROJ  # noqa: E402

# the batch seed: chosen by tests/golden/make_qwen3_fixtures.py (its docstring says how)
SEED, BATCH_SEED, LORA_SEED, R, ALPHA, LENS, GEN_LEN = 31, 36, 29, 8, 32.0, (130, 64, 5), 8
SHAPES = ("qwen3_tiny", "qwen3_tiny_untied")


def qknorm_rope(x: torch.Tensor, w: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, eps: float) -> torch.Tensor:
    """x [..., T, H, D], w [D], cos / sin [T, D / 2] (or [..., T, D / 2]: a table row per row of x) -> rope(w * x * rsqrt(mean x^2 + eps))."""
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    c, s = torch.cat([cos, cos], -1).unsqueeze(-2), torch.cat([sin, sin], -1).unsqueeze(-2)
    h = x.shape[-1] // 2
    return y * c + torch.cat([-y[..., h:], y[..., :h]], -1) * s


def fp_linear(sd, cfg, lora=None, scaling: float = 1.0, h16: bool = False) -> Callable:
    """qwen2_ref.fp_linear without a bias (``attention_bias`` is false in the released models and in the shapes here)."""
    assert not cfg.qkv_bias
    W = (lambda k: sd[k].half().float()) if h16 else (lambda k: sd[k])

    def lin(i, p, x, seg):
        y = x @ W(f"model.layers.{i}.{PROJ[p]}.weight").t()
        ab = None if lora is None else lora.get((i, p))
        if ab is not None:
            t = _rnd(x @ _rnd(ab[0], h16).t(), h16)
            y = y + t @ _rnd(ab[1] * scaling, h16).t()
        return y

    return lin


def int8_linear(sd, cfg, lora=None, scaling: float = 1.0, tau: float = 6.0) -> Callable:
    """The LLM.int8 linear of llm_int8_ref (fp32 arithmetic), no bias.  ``lora`` keyed (layer, module)."""
    assert not cfg.qkv_bias
    short = None if lora is None else {(i, p[:-5]): ab for (i, p), ab in lora.items()}
    base = i8.make_linear(sd, cfg, short, scaling, int8=True, tau=tau)
    return lambda i, p, x, seg: base(p[:-5], i, x.reshape(-1, x.shape[-1]), seg).view(*x.shape[:-1], -1)


def hidden(sd, cfg, lin: Callable, ids: torch.Tensor, lens: torch.Tensor, h16: bool = False, qk_norm: Optional[bool] = None) -> torch.Tensor:
    """ids [B, T] right-padded, lens [B] -> final-norm hidden states fp32 [B, T, hidden] (== hidden_states[-1] of Qwen3Model on the real
    positions).  ``qk_norm=False``: the model any earlier code would have computed from the same projections (no norm)."""
    qk_norm = cfg.qk_norm if qk_norm is None else qk_norm
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
        if qk_norm:
            q = _rnd(qknorm_rope(q, sd[pre + "self_attn.q_norm.weight"], cos, sin, cfg.rms_eps), h16)
            k = _rnd(qknorm_rope(k, sd[pre + "self_attn.k_norm.weight"], cos, sin, cfg.rms_eps), h16)
        else:
            q, k = _rnd(rope(q, cos, sin), h16), _rnd(rope(k, cos, sin), h16)
        ao = _rnd(attention(q, k, v, lens, cfg.heads, cfg.kv_heads, h16=h16), h16)
        x = x + lin(i, "o_proj", ao, seg)
        h2 = _rnd(rmsnorm(x, sd[pre + "post_attention_layernorm.weight"], cfg.rms_eps), h16)
        gate, up = _rnd(lin(i, "gate_proj", h2, seg), h16), _rnd(lin(i, "up_proj", h2, seg), h16)
        x = x + lin(i, "down_proj", _rnd(torch.nn.functional.silu(gate) * up, h16), seg)
    return rmsnorm(x, sd["model.norm.weight"], cfg.rms_eps)


def outputs(sd, cfg, lin, ids, lens, h16: bool = False, qk_norm: Optional[bool] = None) -> dict:
    """What the fixture records of one forward pass (as qwen2_ref.outputs)."""
    with torch.no_grad():
        hf = hidden(sd, cfg, lin, ids, lens, h16, qk_norm)
        last = torch.stack([hf[i, int(n) - 1] for i, n in enumerate(lens)])
        return {"hidden": torch.cat([hf[i, :int(n)] for i, n in enumerate(lens)]), "embedding": pooled(hf, lens),
                "logits_last": logits(sd, cfg, last, h16), "logprobs": token_logprobs(sd, cfg, hf, ids, lens, h16)}


def greedy(sd, cfg, lin, prompt, n_new: int, h16: bool = False):
    """Greedy continuation with the prompt re-run for every token -> (new tokens, top-1 minus top-2 logit per step)."""
    out, margins = [int(i) for i in prompt], []
    with torch.no_grad():
        for _ in range(n_new):
            lg = logits(sd, cfg, hidden(sd, cfg, lin, torch.tensor([out]), torch.tensor([len(out)]), h16)[0, -1], h16)
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


def config_json(cfg) -> dict:
    """The keys of a Qwen3 checkpoint's config.json (as the released models carry them: head_dim of its own, layer_types all full)."""
    assert cfg.model_type == "qwen3"
    return {"architectures": ["Qwen3ForCausalLM"], "model_type": "qwen3", "vocab_size": cfg.vocab, "hidden_size": cfg.hidden,
            "intermediate_size": cfg.ffn, "num_hidden_layers": cfg.layers, "num_attention_heads": cfg.heads,
            "num_key_value_heads": cfg.kv_heads, "head_dim": cfg.head_dim, "hidden_act": "silu", "max_position_embeddings": cfg.max_positions,
            "rms_norm_eps": cfg.rms_eps, "rope_theta": cfg.rope_theta, "rope_scaling": None, "attention_bias": False,
            "use_sliding_window": False, "sliding_window": None, "max_window_layers": cfg.layers,
            "layer_types": ["full_attention"] * cfg.layers, "tie_word_embeddings": cfg.tie_embeddings, "attention_dropout": 0.0,
            "bos_token_id": cfg.bos_token_id, "eos_token_id": cfg.eos_token_id, "torch_dtype": "float16"}


def write_base(path: str, cfg, sd: dict, eos_ids=None, config: Optional[dict] = None) -> str:
    """A Qwen3 checkpoint directory: config.json, generation_config.json, model.safetensors (fp16 as saved, norm weights included)."""
    return q2.write_base(path, cfg, sd, eos_ids, config if config is not None else config_json(cfg))
