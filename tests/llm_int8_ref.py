"""Restatement of the embedder's LLM.int8 + LoRA arithmetic in plain torch (DESIGN.md "LLM.int8 + LoRA"), and writers of synthetic
PEFT adapter / base checkpoint directories.  Uses only torch and safetensors, so GPU tests call it live.  Not bitsandbytes or peft:
their published behaviour restated (none of the libraries is needed to run it).

A *linear* here is ``lin(key, layer, x, seg) -> y fp32`` with key one of q k v o gate up down, x fp32 ``[M, K]``, seg int ``[M]``."""
from __future__ import annotations

import json
import math
import os
from typing import Callable, Dict, List, Optional

import torch

PROJ = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
        "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}


# ------------------------------------------------------------------------------------------------------------ quantisation
def quant_weight(w: torch.Tensor):
    """W [N, K] -> (CB int8 [N, K], SCB fp32 [N]): cast to fp16, per-row absmax, rint(W * (127 / SCB)) half to even."""
    w = w.to(torch.float16).float()
    scb = w.abs().amax(1)
    s = torch.where(scb > 0, torch.tensor(127.0) .to(scb.device) / scb, torch.zeros_like(scb))
    return torch.round(w * s[:, None]).to(torch.int8), scb


def quant_act(x16: torch.Tensor, seg: torch.Tensor, tau: float):
    """x fp16 [M, K], seg int [M] (-1 pad) -> (CA int8, SCA fp32 [M], zeroed bool [M, K], outlier bool [M, K]).
    ``zeroed``: the elements CA sets to 0 (the segment's outlier columns; a pad row: its own elements >= tau);
    ``outlier``: the elements that enter the outlier term (pad rows: none)."""
    x = x16.float()
    a = x.abs()
    m, k = x.shape
    dec = tau > 0
    own = a >= tau if dec else torch.zeros_like(a, dtype=torch.bool)
    outl = torch.zeros_like(own)
    seg = seg.to(x.device).long()
    if dec:
        for s in torch.unique(seg[seg >= 0]).tolist():
            rows = seg == s
            outl[rows] = own[rows].any(0)[None, :].expand(int(rows.sum()), k)
    zeroed = outl | (own & (seg < 0)[:, None])
    below = a < tau if dec else torch.ones_like(own)
    sca = torch.where(below, a, torch.zeros_like(a)).amax(1)
    s = torch.where(sca > 0, torch.tensor(127.0).to(sca.device) / sca, torch.zeros_like(sca))
    ca = torch.round(x * s[:, None])
    ca = torch.where(zeroed, torch.zeros_like(ca), ca).to(torch.int8)
    return ca, sca, zeroed, outl


def outlier_columns(outl: torch.Tensor, seg: torch.Tensor) -> Dict[int, List[int]]:
    """{segment: sorted outlier columns} from quant_act's outlier mask."""
    out = {}
    for s in torch.unique(seg[seg >= 0]).tolist():
        rows = (seg == s).to(outl.device)
        out[int(s)] = torch.nonzero(outl[rows].any(0)).flatten().tolist()
    return out


def int8_linear(x16: torch.Tensor, cb: torch.Tensor, scb: torch.Tensor, seg: torch.Tensor, tau: float, lora=None,
                dtype=torch.float64) -> torch.Tensor:
    """y = base + outlier + lora, in ``dtype`` (fp64: the GEMM tests' yardstick; the int32 accumulator is exact in fp64).
    lora = (A [r, K], B [N, r], scaling) or None."""
    ca, sca, _, outl = quant_act(x16, seg, tau)
    acc = ca.to(dtype) @ cb.to(dtype).T
    y = acc * (sca.to(dtype)[:, None] * scb.to(dtype)[None, :]) / 16129.0
    if outl.any():
        wdq = cb.to(dtype) * scb.to(dtype)[:, None] / 127.0
        y = y + torch.where(outl, x16.to(dtype), torch.zeros((), dtype=dtype, device=x16.device)) @ wdq.T
    if lora is not None:
        a, b, scaling = lora
        y = y + scaling * ((x16.to(dtype) @ a.to(dtype).T) @ b.to(dtype).T)
    return y


def lora_scaling(r: int, alpha: float, use_rslora: bool = False) -> float:
    return alpha / math.sqrt(r) if use_rslora else alpha / r


def make_linear(sd, cfg, lora: Optional[dict] = None, scaling: float = 1.0, int8: bool = True, tau: float = 6.0) -> Callable:
    """The pluggable linear: int8 (x cast to fp16, LLM.int8 by segment, fp32 result) or plain fp32 ``x @ W^T``; plus the unmerged
    LoRA branch ``scaling * (x A^T) B^T`` when ``lora`` = {(layer, key): (A, B)} has the projection."""
    cache = {}

    def lin(key, i, x, seg):
        w = sd[f"model.layers.{i}.{PROJ[key]}.weight"]
        ab = None if lora is None else lora.get((i, key))
        if not int8:
            y = x @ w.T
            if ab is not None:
                y = y + scaling * ((x @ ab[0].T) @ ab[1].T)
            return y
        if (i, key) not in cache:
            cache[(i, key)] = quant_weight(w)
        cb, scb = cache[(i, key)]
        lo = None if ab is None else (ab[0], ab[1], scaling)
        return int8_linear(x.to(torch.float16), cb, scb, seg, tau, lo, dtype=torch.float32)

    return lin


# ------------------------------------------------------------------------------------------------------------ the decoder
def _rope(cfg, positions: torch.Tensor):
    from astts.llm.embedder import llama3_inv_freq

    fr = positions.float()[:, None] * llama3_inv_freq(cfg)[None, :]
    emb = torch.cat([fr, fr], -1)
    return emb.cos(), emb.sin()


def _rot(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def _rms(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


class Decoder:
    """One sequence with a KV cache: ``step(ids)`` runs the next len(ids) positions as one segment (the prefill: the prompt; a decode
    step: one token) and returns the final-norm hidden states [len, hidden].  ``outliers[(layer, key)]`` records the outlier
    columns each linear saw (q/k/v/gate/up share their input: recorded under q and gate).  ``fp16_io``: round where the GPU path
    stores fp16 (q|k|v, the attention output, gate|up, the SwiGLU product), so that the comparison measures the int8 arithmetic rather
    than those roundings."""

    def __init__(self, sd, cfg, lin, tau: float = 6.0, fp16_io: bool = False):
        self.sd, self.cfg, self.lin, self.tau = sd, cfg, lin, tau
        self.r16 = (lambda v: v.to(torch.float16).float()) if fp16_io else (lambda v: v)
        self.k: List[torch.Tensor] = [None] * cfg.layers
        self.v: List[torch.Tensor] = [None] * cfg.layers
        self.pos = 0
        self.outliers: Dict[tuple, List[int]] = {}

    def step(self, ids) -> torch.Tensor:
        cfg, sd = self.cfg, self.sd
        ids = torch.as_tensor(ids, dtype=torch.long)
        t = ids.shape[0]
        seg = torch.zeros(t, dtype=torch.long)
        x = sd["model.embed_tokens.weight"][ids].float()
        cos, sin = _rope(cfg, torch.arange(self.pos, self.pos + t))
        hd, rep = cfg.head_dim, cfg.heads // cfg.kv_heads
        for i in range(cfg.layers):
            p = f"model.layers.{i}."
            h = _rms(x, sd[p + "input_layernorm.weight"], cfg.rms_eps)
            self._note(i, "q", h)
            q = self.r16(self.lin("q", i, h, seg)).view(t, cfg.heads, hd).transpose(0, 1)
            k = self.r16(self.lin("k", i, h, seg)).view(t, cfg.kv_heads, hd).transpose(0, 1)
            v = self.r16(self.lin("v", i, h, seg)).view(t, cfg.kv_heads, hd).transpose(0, 1)
            q = self.r16(q * cos + _rot(q) * sin)
            k = self.r16(k * cos + _rot(k) * sin)
            self.k[i] = k if self.k[i] is None else torch.cat([self.k[i], k], 1)
            self.v[i] = v if self.v[i] is None else torch.cat([self.v[i], v], 1)
            kk, vv = self.k[i].repeat_interleave(rep, 0), self.v[i].repeat_interleave(rep, 0)
            s = q @ kk.transpose(-1, -2) / math.sqrt(hd)
            tk = kk.shape[1]
            causal = torch.arange(tk)[None, :] > (torch.arange(t) + self.pos)[:, None]
            s = s.masked_fill(causal[None], float("-inf"))
            a = self.r16((torch.softmax(s, -1) @ vv).transpose(0, 1).reshape(t, cfg.heads * hd))
            x = x + self.lin("o", i, a, seg)
            h = _rms(x, sd[p + "post_attention_layernorm.weight"], cfg.rms_eps)
            self._note(i, "gate", h)
            g, u = self.r16(self.lin("gate", i, h, seg)), self.r16(self.lin("up", i, h, seg))
            x = x + self.lin("down", i, self.r16(torch.nn.functional.silu(g) * u), seg)
        self.pos += t
        return _rms(x, sd["model.norm.weight"], cfg.rms_eps)

    def _note(self, i, key, h):
        if self.tau > 0:
            cols = torch.nonzero((h.to(torch.float16).float().abs() >= self.tau).any(0)).flatten().tolist()
            self.outliers[(i, key)] = self.outliers.get((i, key), []) + [cols]

    def logits(self, h_last: torch.Tensor) -> torch.Tensor:
        head = self.sd.get("lm_head.weight", self.sd["model.embed_tokens.weight"])
        return h_last @ head.T


def embed(sd, cfg, lin, ids, tau: float = 6.0) -> torch.Tensor:
    """Mean-pooled final hidden state of one text (src/search_milvus.py:75-108)."""
    return Decoder(sd, cfg, lin, tau).step(ids).mean(0)


def generate(sd, cfg, lin, ids, n_new: int, tau: float = 6.0, fp16_io: bool = False):
    """Greedy continuation (prefill = one segment, then one-token segments) -> (new tokens, top-1 minus top-2 logit per step)."""
    d = Decoder(sd, cfg, lin, tau, fp16_io)
    h = d.step(ids)[-1]
    toks, margins = [], []
    for s in range(n_new):
        lg = d.logits(h)
        top = torch.topk(lg, 2).values
        toks.append(int(torch.argmax(lg)))
        margins.append(float(top[0] - top[1]))
        if s + 1 < n_new:
            h = d.step([toks[-1]])[-1]
    return toks, margins


# ------------------------------------------------------------------------------------------------------------ directories
def make_lora(cfg, r: int = 32, seed: int = 1, std_a: float = 0.02, std_b: float = 0.02, targets=tuple(PROJ)) -> dict:
    """{(layer, key): (A [r, in], B [out, r])} seeded (B non-zero: a trained adapter, not a fresh one)."""
    g = torch.Generator().manual_seed(seed)
    dims = {"q": (cfg.hidden, cfg.heads * cfg.head_dim), "k": (cfg.hidden, cfg.kv_heads * cfg.head_dim),
            "v": (cfg.hidden, cfg.kv_heads * cfg.head_dim), "o": (cfg.heads * cfg.head_dim, cfg.hidden),
            "gate": (cfg.hidden, cfg.ffn), "up": (cfg.hidden, cfg.ffn), "down": (cfg.ffn, cfg.hidden)}
    out = {}
    for i in range(cfg.layers):
        for key in targets:
            din, dout = dims[key]
            out[(i, key)] = (torch.randn(r, din, generator=g) * std_a, torch.randn(dout, r, generator=g) * std_b)
    return out


def merged(sd, lora: dict, scaling: float) -> dict:
    """W + scaling * B A (fp32) for every projection with a LoRA pair."""
    out = dict(sd)
    for (i, key), (a, b) in lora.items():
        k = f"model.layers.{i}.{PROJ[key]}.weight"
        out[k] = sd[k] + scaling * (b @ a)
    return out


def write_base(path: str, cfg, sd: dict, eos_ids=None) -> str:
    """A transformers-style checkpoint directory: config.json, generation_config.json, model.safetensors (fp16 as saved)."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    conf = dict(cfg.hf_kwargs(), architectures=["LlamaForCausalLM"], model_type="llama", torch_dtype="float16")
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(conf, f)
    with open(os.path.join(path, "generation_config.json"), "w") as f:
        json.dump({"bos_token_id": cfg.bos_token_id, "eos_token_id": eos_ids if eos_ids is not None else cfg.eos_token_id}, f)
    save_file({k: v.to(torch.float16).contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    return path


def write_adapter(path: str, lora: dict, r: int = 32, alpha: float = 128, use_rslora: bool = False, target_modules="all-linear",
                  base: str = "meta-llama/Llama-3.2-3B-Instruct", embed: Optional[torch.Tensor] = None,
                  lm_head: Optional[torch.Tensor] = None, extra_config: Optional[dict] = None, extra_keys: Optional[dict] = None) -> str:
    """A peft LoRA adapter directory as ``save_pretrained`` writes it: adapter_config.json + adapter_model.safetensors with keys
    ``base_model.model.model.layers.{i}.<proj>.lora_{A,B}.weight`` (no adapter name); ``embed`` / ``lm_head``: the resized tables that
    ``save_embedding_layers="auto"`` adds after a vocabulary resize."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    conf = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": r, "lora_alpha": alpha, "lora_dropout": 0.05, "bias": "none",
            "target_modules": target_modules, "use_rslora": use_rslora, "use_dora": False, "fan_in_fan_out": False,
            "modules_to_save": None, "base_model_name_or_path": base, "inference_mode": True}
    conf.update(extra_config or {})
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(conf, f)
    t = {}
    for (i, key), (a, b) in lora.items():
        p = f"base_model.model.model.layers.{i}.{PROJ[key]}."
        t[p + "lora_A.weight"] = a.contiguous()
        t[p + "lora_B.weight"] = b.contiguous()
    if embed is not None:
        t["base_model.model.model.embed_tokens.weight"] = embed.to(torch.float16).contiguous()
    if lm_head is not None:
        t["base_model.model.lm_head.weight"] = lm_head.to(torch.float16).contiguous()
    t.update(extra_keys or {})
    save_file(t, os.path.join(path, "adapter_model.safetensors"))
    return path
