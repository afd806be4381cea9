"""Restatement of LoRA fine-tuning of the Llama decoder in plain torch with autograd (DESIGN.md section 2 "Fine-tuning"): the model
of transformers' LlamaForCausalLM with peft's LoRA branch ``y = W x + scaling * B (A x)`` on the seven projections, the mean next-token
cross-entropy over the real tokens, torch.optim.AdamW with clip_grad_norm_.  Uses only torch, so the GPU tests call it live.

``h16=True`` rounds to fp16 (value and gradient) at exactly the points where the GPU path (astts.llm.train) holds fp16: the weights,
every MFMA operand (norm outputs, the LoRA rank activations, q | k | v before and after RoPE, q * scale * log2 e, P, the attention
output, gate | up, the SwiGLU output, the final hidden states).  Gradients are rounded after multiplication by ``loss_scale``.  The
error of that run against the fp32 one is what the GPU tests' bounds are made of."""
from __future__ import annotations

import math
import os
import sys
from typing import Dict, Tuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from astts.llm.decoder import llama3_inv_freq  # noqa: E402
from astts.llm.peft import PROJ  # noqa: E402

LOG2E = 1.44269504088896341


class _R16(torch.autograd.Function):
    """x -> fp16(x); gradient g -> fp16(g)."""

    @staticmethod
    def forward(ctx, x):
        return x.half().float()

    @staticmethod
    def backward(ctx, g):
        return g.half().float()


def _rnd(x, h16):
    return _R16.apply(x) if h16 else x


def make_lora(cfg, r: int, seed: int, zero_b: bool = False) -> Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]]:
    """A seeded LoRA with a NON-ZERO B (with B = 0 every dA is zero): A ~ U(-1/sqrt(in), 1/sqrt(in)), B ~ N(0, 0.02^2)."""
    from astts.llm.train import proj_shapes

    g = torch.Generator().manual_seed(seed)
    out = {}
    shapes = proj_shapes(cfg)
    for i in range(cfg.layers):
        for p in PROJ:
            o, n = shapes[p]
            a = (torch.rand(r, n, generator=g) * 2 - 1) / math.sqrt(n)
            b = torch.zeros(o, r) if zero_b else torch.randn(o, r, generator=g) * 0.02
            out[(i, p)] = (a, b)
    return out


def make_batch(cfg, lens, seed: int):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros((len(lens), max(lens)), dtype=torch.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = torch.randint(3, cfg.vocab, (n,), generator=g)
        ids[i, 0] = cfg.bos_token_id
    return ids, torch.tensor(lens, dtype=torch.int64)


def attention(q, k, v, lens, heads: int, kv_heads: int, expand: bool = False, h16: bool = False):
    """q [B, T, heads, 128], k / v [B, T, kv_heads, 128] -> [B, T, heads * 128].  Causal, keys at or beyond lens masked, queries at or
    beyond produce zeros.  ``expand``: the second formulation -- repeat the kv heads and run plain attention head by head."""
    b, t, _, d = q.shape
    pos = torch.arange(t)
    mask = (pos[None, :] <= pos[:, None])[None] & (pos[None, None, :] < lens[:, None, None])          # [B, Tq, Tk]
    qvalid = (pos[None, :] < lens[:, None]).float()                                                   # [B, T]
    scale = 1.0 / math.sqrt(d)
    if h16:                                  # the kernels round q * scale * log2(e) to fp16 and work in the log2 domain
        q = _rnd(q * (scale * LOG2E), True) / LOG2E
    else:
        q = q * scale
    if expand:
        g = heads // kv_heads
        k, v = k.repeat_interleave(g, 2), v.repeat_interleave(g, 2)
        outs = []
        for h in range(heads):
            s = q[:, :, h] @ k[:, :, h].transpose(1, 2)
            p = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
            outs.append(_rnd(p, h16) @ v[:, :, h])
        o = torch.stack(outs, 2)
    else:
        g = heads // kv_heads
        qg = q.view(b, t, kv_heads, g, d)
        s = torch.einsum("bikgd,bjkd->bkgij", qg, k)
        p = torch.softmax(s.masked_fill(~mask[:, None, None], float("-inf")), -1)
        o = torch.einsum("bkgij,bjkd->bikgd", _rnd(p, h16), v).reshape(b, t, heads, d)
    return (o * qvalid[:, :, None, None]).reshape(b, t, heads * d)


def rope(x, cos, sin):
    """transformers' apply_rotary_pos_emb on [B, T, H, 128] with cos / sin [T, 64]."""
    c, s = torch.cat([cos, cos], -1)[None, :, None, :], torch.cat([sin, sin], -1)[None, :, None, :]
    h = x.shape[-1] // 2
    return x * c + torch.cat([-x[..., h:], x[..., :h]], -1) * s


def rmsnorm(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def model_loss(sd, cfg, lora, scaling: float, ids, lens, h16: bool = False, loss_scale: float = 1.0, expand: bool = False):
    """Mean next-token cross-entropy over the real targets (times ``loss_scale``).  ``lora``: (layer, module) -> (A, B) (leaf tensors)."""
    b, t = ids.shape
    W = (lambda k: sd[k].half().float()) if h16 else (lambda k: sd[k])
    fr = torch.arange(t, dtype=torch.float32)[:, None] * llama3_inv_freq(cfg)[None, :]
    cos, sin = fr.cos(), fr.sin()
    hq, hk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim

    def lin(i, p, x):
        a, bm = lora[(i, p)]
        tt = _rnd(x @ _rnd(a, h16).t(), h16)
        return x @ W(f"model.layers.{i}.{PROJ[p]}.weight").t() + tt @ _rnd(bm * scaling, h16).t()

    x = sd["model.embed_tokens.weight"][ids]
    for i in range(cfg.layers):
        pre = f"model.layers.{i}."
        h1 = _rnd(rmsnorm(x, sd[pre + "input_layernorm.weight"], cfg.rms_eps), h16)
        q = _rnd(lin(i, "q_proj", h1), h16).view(b, t, cfg.heads, cfg.head_dim)
        k = _rnd(lin(i, "k_proj", h1), h16).view(b, t, cfg.kv_heads, cfg.head_dim)
        v = _rnd(lin(i, "v_proj", h1), h16).view(b, t, cfg.kv_heads, cfg.head_dim)
        q, k = _rnd(rope(q, cos, sin), h16), _rnd(rope(k, cos, sin), h16)
        ao = _rnd(attention(q, k, v, lens, cfg.heads, cfg.kv_heads, expand=expand, h16=h16), h16)
        x = x + lin(i, "o_proj", ao)
        h2 = _rnd(rmsnorm(x, sd[pre + "post_attention_layernorm.weight"], cfg.rms_eps), h16)
        gate, up = _rnd(lin(i, "gate_proj", h2), h16), _rnd(lin(i, "up_proj", h2), h16)
        act = _rnd(torch.nn.functional.silu(gate) * up, h16)
        x = x + lin(i, "down_proj", act)
    hf = _rnd(rmsnorm(x, sd["model.norm.weight"], cfg.rms_eps), h16)
    head = W("model.embed_tokens.weight" if cfg.tie_embeddings else "lm_head.weight")
    logits = hf @ head.t()
    pos = torch.arange(t)[None, :]
    tgt = torch.where(pos + 1 < lens[:, None], torch.cat([ids[:, 1:], ids[:, :1]], 1), torch.full_like(ids, -100))
    return torch.nn.functional.cross_entropy(logits.reshape(b * t, -1), tgt.reshape(-1), ignore_index=-100) * loss_scale


def leaves(lora):
    return {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}


def loss_and_grads(sd, cfg, lora, scaling, ids, lens, h16=False, loss_scale=1.0, expand=False):
    """-> (loss, {(layer, module, "A" | "B"): gradient}) with the loss scale divided out again."""
    lv = leaves(lora)
    loss = model_loss(sd, cfg, lv, scaling, ids, lens, h16=h16, loss_scale=loss_scale, expand=expand)
    loss.backward()
    grads = {}
    for (i, p), (a, b) in lv.items():
        grads[(i, p, "A")], grads[(i, p, "B")] = a.grad / loss_scale, b.grad / loss_scale
    return float(loss.detach()) / loss_scale, grads


def train(sd, cfg, lora, scaling, ids, lens, steps: int, lr: float, max_norm: float = 0.3, h16: bool = False, loss_scale: float = 1.0):
    """``steps`` AdamW steps (0.9, 0.999, 1e-8, weight decay 0) with clip_grad_norm_(max_norm) on one batch -> (the loss before each
    step, the global gradient norm of each step, the parameters after the last step)."""
    lv = leaves(lora)
    ps = [t for ab in lv.values() for t in ab]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    losses, norms = [], []
    for _ in range(steps):
        opt.zero_grad()
        loss = model_loss(sd, cfg, lv, scaling, ids, lens, h16=h16, loss_scale=loss_scale)
        loss.backward()
        if loss_scale != 1.0:
            for t in ps:
                t.grad.div_(loss_scale)
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
        losses.append(float(loss.detach()) / loss_scale)
    return losses, norms, {k: (a.detach(), b.detach()) for k, (a, b) in lv.items()}


def rel_l2(x, ref) -> float:
    x, ref = torch.as_tensor(x).double(), torch.as_tensor(ref).double()
    return float((x - ref).norm() / ref.norm().clamp_min(1e-300))
