"""Restatement of the fine-tuning regularisers (DESIGN.md section 2 "Fine-tuning", include/train/astts_train.h): Philox4x32-10 in
numpy, the LoRA-dropout keep mask and the NEFTune noise it defines, and the model of tests/llm_train_ref.py with both applied (fp32
torch autograd; ``attention``, ``rope`` and ``rmsnorm`` are that file's).  Uses numpy and torch only, so the GPU tests call it live.

Contract.  key = the 64-bit seed, low word then high word; counter = (group low, group high, stream, draw); stream = layer * 8 +
position in astts.llm.peft.PROJ for dropout, 0xFFFFFFFF for NEFTune; draw = the number of training forwards run before.  Dropout:
group = (row * cin + col) / 8, element e takes 16 bits of word e >> 1 (low half for even e), kept iff bits >= floor(p * 65536).
NEFTune: element i uses word i & 3 of group i >> 2, u = ((bits >> 8) + 0.5) 2^-24, noise = mag (2u - 1)."""
from __future__ import annotations

import math

import numpy as np
import torch

import llm_train_ref as ref
from llm_train_ref import PROJ, _rnd, attention, llama3_inv_freq, rmsnorm, rope

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
NEFTUNE_STREAM = 0xFFFFFFFF
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def _group_words(groups: int, seed: int, stream: int, draw: int) -> np.ndarray:
    """uint32 [groups, 4]: the generator's output for groups 0 .. groups - 1."""
    g = np.arange(groups, dtype=np.uint64)
    seed &= (1 << 64) - 1
    w = philox4x32_10((g & MASK32, g >> np.uint64(32), np.uint64(stream), np.uint64(draw)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, 1)


def dropout_threshold(p: float) -> int:
    return int(math.floor(p * 65536))


def dropout_mask(rows: int, cin: int, p: float, seed: int, stream: int, draw: int) -> np.ndarray:
    """uint8 [rows, cin], 1 = kept."""
    assert cin % 8 == 0
    w = _group_words(rows * cin // 8, seed, stream, draw)
    bits = np.stack([w & 0xFFFF, w >> 16], 2).reshape(-1, 8)            # element e: word e >> 1, low half first
    return (bits >= dropout_threshold(p)).astype(np.uint8).reshape(rows, cin)


def neftune_noise(rows: int, hidden: int, mag: float, seed: int, draw: int) -> np.ndarray:
    """float64 [rows, hidden]: mag (2u - 1), exactly."""
    assert hidden % 4 == 0
    w = _group_words(rows * hidden // 4, seed, NEFTUNE_STREAM, draw).reshape(rows, hidden)
    u = ((w >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    return float(mag) * (2.0 * u - 1.0)


def neftune_mag(alpha: float, t: int, hidden: int) -> float:
    return alpha / math.sqrt(t * hidden)


def model_loss(sd, cfg, lora, scaling: float, ids, lens, p: float, neftune_alpha: float, seed: int, draw: int, h16: bool = False,
               loss_scale: float = 1.0):
    """llm_train_ref.model_loss in training mode: every LoRA module drops its own input (mask of stream layer * 8 + position in
    PROJ), the embedding output takes NEFTune noise.  ``h16`` rounds where the GPU path holds fp16, as there."""
    b, t = ids.shape
    rows = b * t
    W = (lambda k: sd[k].half().float()) if h16 else (lambda k: sd[k])
    fr = torch.arange(t, dtype=torch.float32)[:, None] * llama3_inv_freq(cfg)[None, :]
    cos, sin = fr.cos(), fr.sin()
    names = list(PROJ)
    keep_scale = 1.0 / (1.0 - p)

    def lin(i, pn, x):
        a, bm = lora[(i, pn)]
        xm = x
        if p > 0.0:
            m = dropout_mask(rows, x.shape[-1], p, seed, i * 8 + names.index(pn), draw)
            xm = x * torch.from_numpy(m).float().view(x.shape)
        tt = _rnd((xm @ _rnd(a, h16).t()) * keep_scale, h16)               # the scale multiplies the fp32 accumulator
        return x @ W(f"model.layers.{i}.{PROJ[pn]}.weight").t() + tt @ _rnd(bm * scaling, h16).t()

    x = sd["model.embed_tokens.weight"][ids]
    if neftune_alpha > 0.0:
        mag = np.float32(neftune_mag(neftune_alpha, t, cfg.hidden))
        noise = neftune_noise(rows, cfg.hidden, float(mag), seed, draw)
        x = (x.double() + torch.from_numpy(noise).view(b, t, cfg.hidden)).float()
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
        act = _rnd(torch.nn.functional.silu(gate) * up, h16)
        x = x + lin(i, "down_proj", act)
    hf = _rnd(rmsnorm(x, sd["model.norm.weight"], cfg.rms_eps), h16)
    head = W("model.embed_tokens.weight" if cfg.tie_embeddings else "lm_head.weight")
    logits = hf @ head.t()
    pos = torch.arange(t)[None, :]
    tgt = torch.where(pos + 1 < lens[:, None], torch.cat([ids[:, 1:], ids[:, :1]], 1), torch.full_like(ids, -100))
    return torch.nn.functional.cross_entropy(logits.reshape(rows, -1), tgt.reshape(-1), ignore_index=-100) * loss_scale


def loss_and_grads(sd, cfg, lora, scaling, ids, lens, p, neftune_alpha, seed, draw, h16=False):
    """-> (loss, {(layer, module, "A" | "B"): gradient})."""
    lv = ref.leaves(lora)
    loss = model_loss(sd, cfg, lv, scaling, ids, lens, p, neftune_alpha, seed, draw, h16=h16)
    loss.backward()
    grads = {}
    for (i, pn), (a, b) in lv.items():
        grads[(i, pn, "A")], grads[(i, pn, "B")] = a.grad, b.grad
    return float(loss.detach()), grads
