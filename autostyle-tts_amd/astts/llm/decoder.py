"""The Llama-3.2 decoder on the GPU: weights, RoPE tables and the layer stack in its two layouts (batch-major over right-padded
texts; time-major over left-padded prompts with a KV cache).  astts.llm.embedder.LlamaEmbedder builds the reference's calls on it.
Every tensor operation is a HIP kernel of libastts.so (GEMMs: the MFMA family of csrc/ops_gemm.hip with fp16 activations;
RMSNorm / RoPE / causal GQA attention at head_dim 64 or 128 / SwiGLU / mean-pool: csrc/ops_llm.hip).  fp16 weights and MFMA
operands, fp32 residual stream, norms and softmax.  Parity: tests/test_llm_gpu.py against fixtures produced by transformers (fp32).

``int8=True`` runs the reference's own numerics instead (src/search_milvus.py:47-62: a PEFT LoRA adapter over LLM.int8 weights):
the seven projections of every layer become int8 weights with per-row scales, their inputs are quantised per row with the outlier
columns of each sequence (|x| >= ``int8_threshold``) kept in fp16 against the dequantised weight, and the adapter's LoRA branch
(``lora``: an astts.llm.peft.LoraAdapter) runs unmerged in fp32 -- all of it csrc/ops_int8.hip (DESIGN.md "LLM.int8 + LoRA").
No fp16 copy of those projections is kept.  A ``lora`` without ``int8`` is merged into the fp16 weights at load.

A Qwen2 shape (``cfg.qkv_bias``, ``cfg.rope_type == "default"``, untied head; DESIGN.md section 2 "Qwen2") runs through the same stack:
the q | k | v bias rides on the fused pack into the GEMM's fp32 epilogue, in both layouts and both precisions.

A Qwen3 shape (``cfg.qk_norm``; DESIGN.md section 2 "Qwen3") differs in one launch per layer: ops.qknorm_rope_ (csrc/ops_qknorm.hip)
normalises every q and k head over its head_dim values, scales it by ``self_attn.q_norm`` / ``k_norm`` and rotates it, in the launch
that is RoPE's for the other families.  Its head_dim is a config key of its own: hq = heads * head_dim is not hidden.
"""
from __future__ import annotations

import math
import os
import threading
from typing import Callable, List, Optional

import torch

from .. import ops
from .config import LlamaShape
from .peft import PROJ


def llama3_inv_freq(cfg: LlamaShape) -> torch.Tensor:
    """transformers' _compute_llama3_parameters, float32 as there."""
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, cfg.head_dim, 2, dtype=torch.int64).float() / cfg.head_dim))
    low_wl = cfg.rope_original_max_pos / cfg.rope_low_freq_factor
    high_wl = cfg.rope_original_max_pos / cfg.rope_high_freq_factor
    wl = 2 * math.pi / inv
    inv_l = torch.where(wl > low_wl, inv / cfg.rope_factor, inv)
    smooth = (cfg.rope_original_max_pos / wl - cfg.rope_low_freq_factor) / (cfg.rope_high_freq_factor - cfg.rope_low_freq_factor)
    smoothed = (1 - smooth) * inv_l / cfg.rope_factor + smooth * inv_l
    medium = ~(wl < high_wl) * ~(wl > low_wl)
    return torch.where(medium, smoothed, inv_l)


def default_inv_freq(cfg: LlamaShape) -> torch.Tensor:
    """transformers' compute_default_rope_parameters: 1 / theta^(2i/d), float32 as there."""
    return 1.0 / (cfg.rope_theta ** (torch.arange(0, cfg.head_dim, 2, dtype=torch.float) / cfg.head_dim))


def inv_freq(cfg: LlamaShape) -> torch.Tensor:
    """The RoPE inverse frequencies ``cfg.rope_type`` names."""
    if cfg.rope_type == "llama3":
        return llama3_inv_freq(cfg)
    if cfg.rope_type == "default":
        return default_inv_freq(cfg)
    raise ValueError(f"rope_type {cfg.rope_type!r}: 'llama3' or 'default'")


def _merge_lora(state: dict, lora) -> dict:
    """W + scaling * B A in fp32 for the fp16 path (the int8 path keeps the branch unmerged, as peft does)."""
    out = dict(state)
    for (i, p), (a, b) in lora.pairs.items():
        k = f"model.layers.{i}.{PROJ[p]}.weight"
        out[k] = state[k].float() + lora.scaling * (b.float() @ a.float())
    return out


class LlamaDecoder:
    def __init__(self, state: dict, cfg: LlamaShape, device=None, int8: bool = False, lora=None, int8_threshold: float = 6.0, rope_len: int = 576):
        if not torch.cuda.is_available():
            raise RuntimeError("astts.llm needs a ROCm GPU; there is no CPU fallback in the product path")
        if cfg.head_dim not in (64, 128):
            raise ValueError(f"LlamaDecoder: head_dim {cfg.head_dim}: the attention kernels are built for 64 and 128")
        self.cfg = cfg
        self.device = dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.mfma_attention = os.environ.get("ASTTS_LLM_ATTN", "mfma") != "valu"
        self.int8, self.int8_threshold = bool(int8), float(int8_threshold)
        # a bias this model would drop is an error: the checkpoint would run and compute another function
        ok = (".q_proj.bias", ".k_proj.bias", ".v_proj.bias") if cfg.qkv_bias else ()
        dropped = [k for k in state if k.endswith(".bias") and not (ok and k.endswith(ok))]
        if dropped:
            raise ValueError(f"the checkpoint has biases that this {cfg.model_type} shape (qkv_bias={cfg.qkv_bias}) does not apply: {dropped[:3]}")
        # the same rule for Qwen3's q / k norm: weights this shape would not apply are an error, and so are missing ones
        qkn = [k for k in state if k.endswith((".self_attn.q_norm.weight", ".self_attn.k_norm.weight"))]
        if qkn and not cfg.qk_norm:
            raise ValueError(f"the checkpoint has q / k norm weights that this {cfg.model_type} shape (qk_norm=False) does not apply: {sorted(qkn)[:3]}")
        if cfg.qk_norm:
            lost = [k for i in range(cfg.layers) for k in (f"model.layers.{i}.self_attn.q_norm.weight", f"model.layers.{i}.self_attn.k_norm.weight")
                    if k not in state or tuple(state[k].shape) != (cfg.head_dim,)]
            if lost:
                raise ValueError(f"this {cfg.model_type} shape has qk_norm=True but the checkpoint lacks [head_dim] norm weights: {lost[:3]}")
        if lora is not None and not self.int8:
            state = _merge_lora(state, lora)

        def weight(i: int, *names: str):
            """The projections ``names`` of layer i, fused along their output rows, in the format this model runs."""
            ws = [state[f"model.layers.{i}.{nm}.weight"] for nm in names]
            # Qwen2: q | k | v carry a bias, added in fp32 in the GEMM's epilogue (before the fp16 store, so before RoPE); a missing one is an error
            bias = torch.cat([state[f"model.layers.{i}.{nm}.bias"].float() for nm in names]) if cfg.qkv_bias and "q_proj" in names[0] else None
            if not self.int8:
                return ops.PackedWeight(ws[0] if len(ws) == 1 else torch.cat(ws, 0), bias, dev)
            ab = [None if lora is None else lora.pairs.get((i, nm.split(".")[-1])) for nm in names]
            r = next((p[0].shape[0] for p in ab if p is not None), None)
            if r is not None:                                 # a fused projection with LoRA on some parts: zero pairs on the others
                ab = [p if p is not None else (torch.zeros(r, w.shape[1]), torch.zeros(w.shape[0], r)) for w, p in zip(ws, ab)]
            return ops.Int8Weight([(w, None, None) if p is None else (w, p[0], p[1]) for w, p in zip(ws, ab)],
                                  1.0 if lora is None else lora.scaling, dev, bias=bias)

        with torch.cuda.device(dev):
            f = lambda k: state[k].to(device=dev, dtype=torch.float32).contiguous()
            self.embed = f("model.embed_tokens.weight")               # fp32 table: the lookup feeds the fp32 residual stream
            self.L = [{"n1": f(f"model.layers.{i}.input_layernorm.weight"), "n2": f(f"model.layers.{i}.post_attention_layernorm.weight"),
                       "wqkv": weight(i, "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "wo": weight(i, "self_attn.o_proj"),
                       "wgu": weight(i, "mlp.gate_proj", "mlp.up_proj"), "wd": weight(i, "mlp.down_proj")} for i in range(cfg.layers)]
            if cfg.qk_norm:
                for i, L in enumerate(self.L):
                    L["qn"], L["kn"] = f(f"model.layers.{i}.self_attn.q_norm.weight"), f(f"model.layers.{i}.self_attn.k_norm.weight")
            self.norm = f("model.norm.weight")
            head = state["model.embed_tokens.weight"] if cfg.tie_embeddings else state["lm_head.weight"]
            self.head = ops.PackedWeight(head, None, dev)
            self._rope_lock = threading.Lock()
            self._rope_tables(rope_len)

    @classmethod
    def adopt(cls, base: "LlamaDecoder", layers: List[dict], rope_len: int = 0, **kw):
        """A second fp16 decoder over prepared weights: ``layers`` (one dict per layer with the keys of ``base.L``) are taken as they
        are, the embedding table, final norm, head and RoPE tables are ``base``'s own tensors.  Nothing is read from a state dict,
        nothing is packed.  ``kw``: what a subclass adds (LlamaEmbedder: tokenizer, max_length)."""
        assert not base.int8 and len(layers) == len(base.L) and all(set(l) == set(b) for l, b in zip(layers, base.L))
        self = cls.__new__(cls)
        self.cfg, self.device, self.mfma_attention = base.cfg, base.device, base.mfma_attention
        self.int8, self.int8_threshold = False, base.int8_threshold
        self.embed, self.norm, self.head, self.L = base.embed, base.norm, base.head, layers
        self._rope_lock = threading.Lock()
        self._rope = base._rope
        self._rope_for(rope_len)                     # longer than the base's tables: this decoder grows a pair of its own
        self._adopted(**kw)
        return self

    def _adopted(self) -> None:
        pass

    def _lin(self, x: torch.Tensor, w, seg, residual=None, out_dtype=torch.float32) -> torch.Tensor:
        """One projection: the fp16 GEMM (ops.linear), or with int8 the LLM.int8 + LoRA GEMM on the segments ``seg`` = (ids, count)."""
        if self.int8:
            return w(x, seg[0], seg[1], self.int8_threshold, residual=residual, out_dtype=out_dtype)
        return ops.linear(x, w, residual=residual, out_dtype=out_dtype)

    def _segments(self, b: int, t: int = 1, lens: Optional[torch.Tensor] = None, start: Optional[torch.Tensor] = None):
        """The LLM.int8 segments (ids int32 flat, count) of ``b`` texts of ``t`` positions: one segment per text, a pad row (-1) in none.
        Rows ``[B, T]``, text j real below ``lens[j]`` (None: all of it; ``t`` = 1: a decode step), or with ``start`` ``[T, B]``, text j
        real from ``start[j]`` on.  None without ``int8``: the fp16 GEMM has no segments, and nothing is launched for them."""
        if not self.int8:
            return None
        bi = torch.arange(b, dtype=torch.int32, device=self.device)
        pos = torch.arange(t, dtype=torch.int32, device=self.device)
        if start is not None:
            ids = torch.where(pos[:, None] >= start[None, :], bi[None, :], -1)
        else:
            ids = bi[:, None].expand(b, t) if lens is None else torch.where(pos[None, :] < lens.to(self.device)[:, None], bi[:, None], -1)
        return ids.reshape(-1).to(torch.int32).contiguous(), b

    def _rope_tables(self, n: int) -> None:
        """(cos, sin) rows for positions < n, published as ONE tuple: a thread that sees the new cos also sees the new sin."""
        fr = torch.arange(n, dtype=torch.float32)[:, None] * inv_freq(self.cfg)[None, :]
        self._rope = (fr.cos().to(self.device).contiguous(), fr.sin().to(self.device).contiguous())

    def _rope_for(self, n: int):
        """One consistent (cos, sin) pair that covers positions < n, grown first if it has to be: the untruncated generation prompt
        (milvus/search_json.py:178) can exceed max_length."""
        if n > self._rope[0].shape[0]:
            with self._rope_lock:
                if n > self._rope[0].shape[0]:
                    self._rope_tables((n + 255) // 256 * 256)
        return self._rope

    cos = property(lambda self: self._rope[0])
    sin = property(lambda self: self._rope[1])

    def _layer(self, x: torch.Tensor, L: dict, seg, attend: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
        """One decoder layer on the fp32 residual stream ``x``.  ``attend(qkv, L)``: q|k|v fp16 ``[.., .., hq + 2 hk]`` (not yet rotated) ->
        the attention output; RoPE (with Qwen3's q / k norm in the same launch), cache and attention are all that the two layouts below differ in."""
        eps = self.cfg.rms_eps                                                    # the norms in fp16: their only consumer is an MFMA operand
        qkv = self._lin(ops.rmsnorm(x, L["n1"], eps), L["wqkv"], seg, out_dtype=torch.float16)
        x = self._lin(attend(qkv, L), L["wo"], seg, residual=x)
        gu = self._lin(ops.rmsnorm(x, L["n2"], eps), L["wgu"], seg, out_dtype=torch.float16)
        return self._lin(ops.swiglu(gu), L["wd"], seg, residual=x)

    def hidden(self, ids: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids int [B, T] (right-padded), lens int32 [B] or None -> final-norm hidden states fp32 [B, T, hidden]
        (== outputs.hidden_states[-1] of LlamaModel)."""
        cfg = self.cfg
        b, t = ids.shape
        cos, sin = self._rope_for(t)
        hq, hk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
        # v_mfma_f32_32x32x16_f16 (csrc/ops_llm.hip attn_gqa_mfma), or the VALU kernel: the second implementation (tests)
        attn = ops.attn_gqa if self.mfma_attention else ops.attn_causal_gqa

        def attend(qkv: torch.Tensor, L: dict) -> torch.Tensor:                   # [B, T, hq + 2 hk]
            if cfg.qk_norm:                                                       # Qwen3: norm and rotation in the one launch
                ops.qknorm_rope_(qkv, cos, sin, L["qn"], L["kn"], cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.rms_eps)
            else:
                ops.rope_llama_(qkv, cos, sin, cfg.heads + cfg.kv_heads, cfg.head_dim)         # q heads then k heads: contiguous
            return attn(qkv[..., :hq], qkv[..., hq:hq + hk], qkv[..., hq + hk:], cfg.heads, cfg.kv_heads, cfg.head_dim, lens)

        x = ops.embedding(self.embed, ids.to(self.device))
        seg = self._segments(b, t, lens=lens)
        for L in self.L:
            x = self._layer(x, L, seg, attend)
        return ops.rmsnorm(x, self.norm, cfg.rms_eps, out_dtype=torch.float32)

    def hidden_cached(self, x: torch.Tensor, cache: List[torch.Tensor], pos0: int, start: torch.Tensor, seg) -> torch.Tensor:
        """x fp32 [T', B, hidden] = the new positions pos0 .. pos0 + T' - 1 of LEFT-padded rows, time-major -> final-norm hidden of the
        LAST of them [B, hidden].  ``cache``: per layer fp16 ``[T_max, B, 2 * kv_heads * head_dim]``, K (rotated) | V; the rows of a step are
        contiguous in it.  ``start[b]`` (int32 [B]): the time step of row b's first token; it masks the row's pad keys and shifts its RoPE
        positions so that that token has position 0, as in the one-at-a-time reference run."""
        cfg = self.cfg
        tn = x.shape[0]
        cos, sin = self._rope_for(cache[0].shape[0])
        hq, hk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
        for L, kv in zip(self.L, cache):
            def attend(qkv: torch.Tensor, L: dict) -> torch.Tensor:               # [T', B, hq + 2 hk]
                if cfg.qk_norm:
                    ops.qknorm_rope_(qkv, cos, sin, L["qn"], L["kn"], cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.rms_eps, pos0=pos0, shift=start,
                                     time_major=True)
                else:
                    ops.rope_llama_ex_(qkv, cos, sin, cfg.heads + cfg.kv_heads, cfg.head_dim, pos0=pos0, shift=start, time_major=True)
                kv[pos0:pos0 + tn].copy_(qkv[..., hq:])                            # K (rotated) | V into the cache rows
                return ops.attn_gqa(qkv[..., :hq], kv[:pos0 + tn, :, :hk], kv[:pos0 + tn, :, hk:], cfg.heads, cfg.kv_heads, cfg.head_dim,
                                    key_start=start, pos0=pos0, time_major=True)

            x = self._layer(x, L, seg, attend)
        return ops.rmsnorm(x[-1].contiguous(), self.norm, cfg.rms_eps, out_dtype=torch.float32)
