"""The query embedder on the GPU: Llama-3.2 decoder forward -> mean-pooled last hidden state, and the greedy
continuation that names the emotion.

Replaces, in the reference's retrieval scripts (paths under /root/reference):
    get_embedding(text, model, tokenizer, device, layer=-1, pooling='mean')   src/search_milvus.py:75-108
                                                                              (same function: milvus/search_json.py:76-109)
    generate_emotion_label(text, ...)  -> model.generate(do_sample=False)     milvus/search_json.py:154-198
    create_combined_embedding(...)     -> concatenate(emotion, biography)     milvus/search_json.py:201-229,
                                                                              src/search_milvus.py:214-221
Every tensor operation is a HIP kernel of libastts.so (GEMMs: the MFMA family of csrc/ops_gemm.hip with fp16 activations;
RMSNorm / RoPE / causal GQA attention at head_dim 128 / SwiGLU / mean-pool: csrc/ops_llm.hip).  fp16 weights and MFMA
operands, fp32 residual stream, norms and softmax.  Parity: tests/test_llm_gpu.py against fixtures produced by transformers (fp32).

``int8=True`` runs the reference's own numerics instead (src/search_milvus.py:47-62: a PEFT LoRA adapter over LLM.int8 weights):
the seven projections of every layer become int8 weights with per-row scales, their inputs are quantised per row with the outlier
columns of each sequence (|x| >= ``int8_threshold``) kept in fp16 against the dequantised weight, and the adapter's LoRA branch
(``lora``: an astts.llm.peft.LoraAdapter) runs unmerged in fp32 -- all of it csrc/ops_int8.hip (DESIGN.md "LLM.int8 + LoRA").
No fp16 copy of those projections is kept.  A ``lora`` without ``int8`` is merged into the fp16 weights at load.

The tokenizer is the checkpoint's own (tokenizer.json: not available offline); anything with ``encode(text) -> list[int]``
plugs in (`transformers.AutoTokenizer` when the checkpoint directory is given).  ``HashTokenizer`` is a labelled
deterministic stand-in so that the CLIs run end to end without one.
"""
from __future__ import annotations

import threading

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..ops import PackedWeight
from .config import LlamaShape


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


class HashTokenizer:
    """STAND-IN (the Llama tokenizer files do not exist offline): bos + one id per whitespace-separated word by a fixed
    hash.  Deterministic, reversible in nothing; good for plumbing and benchmarks only."""

    def __init__(self, cfg: LlamaShape):
        self.cfg = cfg

    def encode(self, text: str, add_special_tokens: bool = True) -> List[int]:
        import zlib

        return ([self.cfg.bos_token_id] if add_special_tokens else []) + [3 + zlib.crc32(w.encode("utf-8")) % (self.cfg.vocab - 3)
                                                                          for w in text.split()]

    def decode(self, ids: Sequence[int]) -> str:
        return " ".join(f"<{int(i)}>" for i in ids)


class LlamaEmbedder:
    def __init__(self, state: dict, cfg: LlamaShape, device=None, tokenizer=None, max_length: int = 512, int8: bool = False, lora=None,
                 int8_threshold: float = 6.0):
        if not torch.cuda.is_available():
            raise RuntimeError("astts.llm needs a ROCm GPU; there is no CPU fallback in the product path")
        if cfg.head_dim != 128:
            raise ValueError("LlamaEmbedder: the attention kernel is built for head_dim 128 (Llama-3.2)")
        self.cfg = cfg
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.tokenizer = tokenizer or HashTokenizer(cfg)
        self.max_length = max_length                                  # truncation=True, max_length=512: src/search_milvus.py:92
        import os
        self.mfma_attention = os.environ.get("ASTTS_LLM_ATTN", "mfma") != "valu"
        self.int8, self.int8_threshold = bool(int8), float(int8_threshold)
        if lora is not None and not self.int8:
            state = _merge_lora(state, lora)
        dev = self.device
        with torch.cuda.device(dev):
            f = lambda k: state[k].to(device=dev, dtype=torch.float32).contiguous()
            self.embed = f("model.embed_tokens.weight")               # fp32 table: the lookup feeds the fp32 residual stream
            self.L = []
            for i in range(cfg.layers):
                p = f"model.layers.{i}."
                if self.int8:
                    self.L.append(self._int8_layer(state, i, lora, dev))
                    continue
                wqkv = torch.cat([state[p + "self_attn.q_proj.weight"], state[p + "self_attn.k_proj.weight"],
                                  state[p + "self_attn.v_proj.weight"]], 0)
                wgu = torch.cat([state[p + "mlp.gate_proj.weight"], state[p + "mlp.up_proj.weight"]], 0)
                self.L.append({"n1": f(p + "input_layernorm.weight"), "n2": f(p + "post_attention_layernorm.weight"),
                               "wqkv": PackedWeight(wqkv, None, dev), "wo": PackedWeight(state[p + "self_attn.o_proj.weight"], None, dev),
                               "wgu": PackedWeight(wgu, None, dev), "wd": PackedWeight(state[p + "mlp.down_proj.weight"], None, dev)})
            self.norm = f("model.norm.weight")
            head = state["model.embed_tokens.weight"] if cfg.tie_embeddings else state["lm_head.weight"]
            self.head = PackedWeight(head, None, dev)
            self._rope_lock = threading.Lock()
            self._rope_tables(max(max_length, 16) + 64)

    def _int8_layer(self, state: dict, i: int, lora, dev) -> dict:
        p = f"model.layers.{i}."
        pairs = {} if lora is None else lora.pairs
        scaling = 1.0 if lora is None else lora.scaling

        def w(*names):
            parts = []
            for nm in names:
                ab = pairs.get((i, nm.split(".")[-1]))
                parts.append((state[p + nm + ".weight"], None if ab is None else ab[0], None if ab is None else ab[1]))
            if any(q[1] is not None for q in parts):          # a fused projection with LoRA on some parts: zero pairs on the others
                r = next(q[1].shape[0] for q in parts if q[1] is not None)
                parts = [q if q[1] is not None else (q[0], torch.zeros(r, q[0].shape[1]), torch.zeros(q[0].shape[0], r)) for q in parts]
            return ops.Int8Weight(parts, scaling, dev)

        f = lambda k: state[k].to(device=dev, dtype=torch.float32).contiguous()
        return {"n1": f(p + "input_layernorm.weight"), "n2": f(p + "post_attention_layernorm.weight"),
                "wqkv": w("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "wo": w("self_attn.o_proj"),
                "wgu": w("mlp.gate_proj", "mlp.up_proj"), "wd": w("mlp.down_proj")}

    def _lin(self, x: torch.Tensor, w, seg, residual=None, out_dtype=torch.float32) -> torch.Tensor:
        """One projection: the fp16 GEMM (ops.linear), or with int8 the LLM.int8 + LoRA GEMM on the segments ``seg`` = (ids, count)."""
        if self.int8:
            return w(x, seg[0], seg[1], self.int8_threshold, residual=residual, out_dtype=out_dtype)
        return ops.linear(x, w, residual=residual, out_dtype=out_dtype)

    def _is_eos(self, tok: int) -> bool:
        return tok == self.cfg.eos_token_id or tok in self.cfg.eos_token_ids

    def _rope_tables(self, n: int) -> None:
        """(cos, sin) rows for positions < n, published as ONE tuple: a thread that sees the new cos also sees the new sin."""
        fr = torch.arange(n, dtype=torch.float32)[:, None] * llama3_inv_freq(self.cfg)[None, :]
        self._rope = (fr.cos().to(self.device).contiguous(), fr.sin().to(self.device).contiguous())

    @property
    def cos(self) -> torch.Tensor:
        return self._rope[0]

    @property
    def sin(self) -> torch.Tensor:
        return self._rope[1]

    # ------------------------------------------------------------------ the decoder stack
    def hidden(self, ids: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids int [B, T] (right-padded), lens int32 [B] or None -> final-norm hidden states fp32 [B, T, hidden]
        (== outputs.hidden_states[-1] of LlamaModel)."""
        cfg = self.cfg
        b, t = ids.shape
        if t > self._rope[0].shape[0]:  # the untruncated generation prompt (milvus/search_json.py:178) can exceed max_length
            with self._rope_lock:
                if t > self._rope[0].shape[0]:
                    self._rope_tables((t + 255) // 256 * 256)
        cos, sin = self._rope           # one consistent pair for the whole pass
        hq, hk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
        x = ops.embedding(self.embed, ids.to(self.device))
        seg = None
        if self.int8:                  # LLM.int8 segments: one per text; the right padding belongs to none
            sid = torch.arange(b, dtype=torch.int32, device=self.device)[:, None].expand(b, t)
            if lens is not None:
                sid = torch.where(torch.arange(t, device=self.device)[None, :] < lens.to(self.device)[:, None], sid, -1)
            seg = (sid.reshape(-1).to(torch.int32).contiguous(), b)
        for L in self.L:
            h = ops.rmsnorm(x, L["n1"], cfg.rms_eps)                              # fp16: its only consumer is an MFMA operand
            qkv = self._lin(h, L["wqkv"], seg, out_dtype=torch.float16)          # [B, T, hq + 2 hk]
            ops.rope_llama_(qkv, cos, sin, cfg.heads + cfg.kv_heads, cfg.head_dim)             # q heads then k heads: contiguous
            if self.mfma_attention:                                                # v_mfma_f32_32x32x16_f16 (csrc/ops_llm.hip attn_gqa_mfma)
                a = ops.attn_gqa(qkv[..., :hq], qkv[..., hq:hq + hk], qkv[..., hq + hk:], cfg.heads, cfg.kv_heads, cfg.head_dim, lens=lens)
            else:                                                                  # the VALU kernel: the second implementation (tests)
                a = ops.attn_causal_gqa(qkv[..., :hq], qkv[..., hq:hq + hk], qkv[..., hq + hk:], cfg.heads, cfg.kv_heads, cfg.head_dim, lens)
            x = self._lin(a, L["wo"], seg, residual=x)
            h = ops.rmsnorm(x, L["n2"], cfg.rms_eps)
            gu = self._lin(h, L["wgu"], seg, out_dtype=torch.float16)
            x = self._lin(ops.swiglu(gu), L["wd"], seg, residual=x)
        return ops.rmsnorm(x, self.norm, cfg.rms_eps, out_dtype=torch.float32)

    def embed_ids(self, ids: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Mean over each text's tokens of the last hidden state -> fp32 [B, hidden] on the GPU."""
        if lens is not None:
            lens = lens.to(device=self.device, dtype=torch.int32)
        return ops.mean_pool(self.hidden(ids, lens), lens)

    def logits_last(self, ids: torch.Tensor) -> torch.Tensor:
        h = self.hidden(ids)[:, -1]
        return ops.linear(h.contiguous(), self.head)

    def generate_greedy_recompute(self, ids: Sequence[int], max_new_tokens: int = 10) -> List[int]:
        """do_sample=False continuation with the prompt re-run for every new token (rounds 3-4; kept as the second implementation
        the tests hold the cached path to)."""
        out = list(int(i) for i in ids)
        for _ in range(max_new_tokens):
            lg = self.logits_last(torch.tensor([out], dtype=torch.int64, device=self.device))
            nxt = int(torch.argmax(lg[0]))                                        # one scalar back to the host per token
            out.append(nxt)
            if self._is_eos(nxt):
                break
        return out

    def generate_greedy_batch(self, prompts: Sequence[Sequence[int]], max_new_tokens: int = 10) -> List[List[int]]:
        """do_sample=False continuation (milvus/search_json.py:178-188: model.generate(max_new_tokens=10)) of several prompts at once,
        with a KV cache and no host synchronisation inside the loop: ONE pass over the prompts, then ``max_new_tokens - 1`` one-token
        steps; the argmax runs on the device (``astts_op_argmax_rows``) and feeds the next step's embedding lookup; the tokens come
        back in one copy at the end and are cut at each row's first EOS on the host (transformers stops a row there).
        Layout: prompts are LEFT-padded to a common length, time-major ``[T, B]`` (the rows of a step are contiguous in the cache
        ``[T_max, B, 2 * kv_heads * 128]`` per layer); ``key_start[b]`` masks a row's pad keys and shifts its RoPE positions so that its
        first token has position 0, as in the one-at-a-time reference run."""
        return self._generate_batch(prompts, max_new_tokens, lambda s, lg, out: ops.argmax_rows(lg, out=out))

    def _generate_batch(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, pick, keep_logits: bool = False, poll: int = 0):
        """The KV-cached decode both continuations share: ``pick(step, logits fp32 [B, vocab], out int32 [B])`` chooses each step's
        tokens on the device.  ``keep_logits``: also return every step's logits ``[max_new_tokens, B, vocab]`` (device).  ``poll`` > 0:
        every ``poll`` steps one scalar comes back to ask whether every row has produced an EOS (then the loop stops: what a row holds
        after its first EOS is cut off below either way, so no returned token changes)."""
        cfg, dev = self.cfg, self.device
        prompts = [[int(i) for i in p] for p in prompts]
        b, lens = len(prompts), [len(p) for p in prompts]
        t, n_new = max(lens), int(max_new_tokens)
        if n_new <= 0:
            return ([list(p) for p in prompts], torch.empty((0, b, cfg.vocab), device=dev)) if keep_logits else [list(p) for p in prompts]
        t_max = t + n_new
        if t_max > self._rope[0].shape[0]:
            with self._rope_lock:
                if t_max > self._rope[0].shape[0]:
                    self._rope_tables((t_max + 255) // 256 * 256)
        cos, sin = self._rope
        hq, hk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
        ids = torch.zeros((t, b), dtype=torch.int32)
        for j, p in enumerate(prompts):
            ids[t - lens[j]:, j] = torch.tensor(p, dtype=torch.int32)
        start = torch.tensor([t - n for n in lens], dtype=torch.int32, device=dev)
        cache = [torch.empty((t_max, b, 2 * hk), dtype=torch.float16, device=dev) for _ in self.L]
        toks = torch.zeros((n_new, b), dtype=torch.int32, device=dev)
        seg_prefill = seg_step = None
        if self.int8:                  # LLM.int8 segments: a prompt's tokens in the prefill (left padding: none), one row per decode step
            bi = torch.arange(b, dtype=torch.int32, device=dev)
            seg_prefill = (torch.where(torch.arange(t, dtype=torch.int32, device=dev)[:, None] >= start[None, :], bi[None, :], -1)
                           .reshape(-1).to(torch.int32).contiguous(), b)
            seg_step = (bi, b)

        def stack(x: torch.Tensor, pos0: int) -> torch.Tensor:
            """x fp32 [T', B, hidden] = the new positions pos0 .. pos0 + T' - 1 -> final-norm hidden of the LAST of them [B, hidden]."""
            tn = x.shape[0]
            seg = seg_prefill if pos0 == 0 else seg_step
            for L, kv in zip(self.L, cache):
                h = ops.rmsnorm(x, L["n1"], cfg.rms_eps)
                qkv = self._lin(h, L["wqkv"], seg, out_dtype=torch.float16)                   # [T', B, hq + 2 hk]
                ops.rope_llama_ex_(qkv, cos, sin, cfg.heads + cfg.kv_heads, cfg.head_dim, pos0=pos0, shift=start, time_major=True)
                kv[pos0:pos0 + tn].copy_(qkv[..., hq:])                                        # K (rotated) | V into the cache rows
                a = ops.attn_gqa(qkv[..., :hq], kv[:pos0 + tn, :, :hk], kv[:pos0 + tn, :, hk:], cfg.heads, cfg.kv_heads, cfg.head_dim,
                                 key_start=start, pos0=pos0, time_major=True)
                x = self._lin(a, L["wo"], seg, residual=x)
                h = ops.rmsnorm(x, L["n2"], cfg.rms_eps)
                gu = self._lin(h, L["wgu"], seg, out_dtype=torch.float16)
                x = self._lin(ops.swiglu(gu), L["wd"], seg, residual=x)
            return ops.rmsnorm(x[-1].contiguous(), self.norm, cfg.rms_eps, out_dtype=torch.float32)

        logits = torch.empty((n_new, b, cfg.vocab), dtype=torch.float32, device=dev) if keep_logits else None
        eos = torch.tensor(sorted({int(cfg.eos_token_id), *(int(e) for e in cfg.eos_token_ids)}), dtype=torch.int32, device=dev) if poll > 0 else None
        x = ops.embedding(self.embed, ids.to(dev))
        for s in range(n_new):
            h_last = stack(x, 0 if s == 0 else t + s - 1)
            lg = ops.linear(h_last, self.head)
            pick(s, lg, toks[s])
            if keep_logits:
                logits[s].copy_(lg)
            if s + 1 < n_new:
                if poll > 0 and (s + 1) % poll == 0 and bool(torch.isin(toks[:s + 1], eos).any(0).all()):
                    break
                x = ops.embedding(self.embed, toks[s])[None]
        got = toks.cpu().numpy()                                                               # the one synchronisation
        out = []
        for j, p in enumerate(prompts):
            row = list(p)
            for s in range(n_new):
                row.append(int(got[s, j]))
                if self._is_eos(row[-1]):
                    break
            out.append(row)
        return (out, logits) if keep_logits else out

    @staticmethod
    def row_uniforms(seed: int, index: int, n: int) -> torch.Tensor:
        """The ``n`` uniforms of the row that is number ``index`` in the caller's list: its own generator, so that a row's draws do
        not depend on which other rows share its batch."""
        g = torch.Generator().manual_seed((int(seed) & 0xffffffff) * 1000003 + int(index))
        return torch.rand(n, generator=g, dtype=torch.float32)

    def generate_sample_batch(self, prompts: Sequence[Sequence[int]], max_new_tokens: int = 250, temperature: float = 0.7, top_k: int = 50,
                              top_p: float = 0.9, uniforms: Optional[torch.Tensor] = None, seed: int = 0, return_logits: bool = False):
        """do_sample=True continuation (milvus/search_json.py:139-147: model.generate(do_sample=True, temperature=0.7, top_p=0.9,
        max_new_tokens=250); top_k=50 is GenerationConfig's default, which that call inherits) of several prompts at once: the decode of
        ``generate_greedy_batch`` with each step's token drawn on the device by ``astts_op_sample_topk_topp`` (temperature -> top-k ->
        top-p -> inverse-CDF draw on an injected uniform; definition: include/astts.h).  ``uniforms``: fp32 ``[max_new_tokens, B]`` in
        [0, 1); absent, row j's column is ``row_uniforms(seed, j, max_new_tokens)``.  One copy back at the end (plus one scalar every
        32 steps to stop once every row has ended); rows are cut at their first EOS.  ``return_logits`` (tests, small vocabularies):
        returns ``(rows, logits fp32 [max_new_tokens, B, vocab])`` and runs every step."""
        b, n_new = len(prompts), int(max_new_tokens)
        if uniforms is None:
            uniforms = torch.stack([self.row_uniforms(seed, j, max(n_new, 0)) for j in range(b)], 1) if b else torch.empty((max(n_new, 0), 0))
        uniforms = torch.as_tensor(uniforms, dtype=torch.float32)
        if tuple(uniforms.shape) != (max(n_new, 0), b):
            raise ValueError(f"uniforms {tuple(uniforms.shape)}: expected [max_new_tokens, B] = {(max(n_new, 0), b)}")
        u = uniforms.to(self.device).contiguous()
        pick = lambda s, lg, out: ops.sample_topk_topp(lg, u[s], temperature, top_k, top_p, out=out)
        return self._generate_batch(prompts, n_new, pick, keep_logits=return_logits, poll=0 if return_logits else 32)

    def generate_greedy(self, ids: Sequence[int], max_new_tokens: int = 10) -> List[int]:
        """do_sample=False continuation of one prompt (milvus/search_json.py:178-188): the cached path with one row."""
        return self.generate_greedy_batch([ids], max_new_tokens)[0]

    # ------------------------------------------------------------------ scoring: log-probabilities of given tokens
    def token_logprobs(self, ids: torch.Tensor, lens: Optional[torch.Tensor] = None, start: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids int ``[B, T]`` (right-padded), lens int ``[B]`` or None -> fp32 ``[B, T - 1]`` on the GPU: entry ``[b, t]`` is the
        log-probability of token ``t + 1`` given the tokens ``<= t`` of row b, for every real position (``t + 1 < lens[b]``); padding
        -- and, with ``start`` (int ``[B]``), every target position before ``start[b]`` -- is 0 and never reaches the head.
        One pass of the decoder stack (``hidden``: fp16, or int8 + LoRA, as constructed), then the rows that have a target are gathered
        and scored by ``ops.head_logprob``: the head GEMM with a log-sum-exp epilogue, no ``[rows, vocab]`` logits."""
        b, t = ids.shape
        out = torch.zeros((b, max(t - 1, 0)), dtype=torch.float32, device=self.device)
        if t < 2:
            return out
        ids = ids.to(self.device)
        if lens is not None:
            lens = lens.to(device=self.device, dtype=torch.int32)
        h = self.hidden(ids, lens)                                                # fp32 [B, T, hidden]
        pos = torch.arange(1, t, device=self.device)[None, :]                     # the target's position in the sequence
        take = torch.ones((b, t - 1), dtype=torch.bool, device=self.device) if lens is None else pos < lens[:, None]
        if start is not None:
            take = take & (pos >= start.to(self.device)[:, None])
        rb, rt = torch.nonzero(take, as_tuple=True)
        if rb.numel() == 0:
            return out
        rows = h[rb, rt].to(torch.float16)                                        # the GEMM's operand type (ops.linear converts the same way)
        targets = ids[rb, rt + 1].to(torch.int32)
        out[rb, rt] = ops.head_logprob(rows, self.head, targets)
        return out

    def _pad_batch(self, seqs: Sequence[Sequence[int]]):
        tmax = max(len(s) for s in seqs)
        ids = torch.zeros((len(seqs), tmax), dtype=torch.int64)
        for i, s in enumerate(seqs):
            ids[i, : len(s)] = torch.tensor(list(s), dtype=torch.int64)
        return ids, torch.tensor([len(s) for s in seqs], dtype=torch.int32)

    def _ids_of(self, x, continuation: bool = False) -> List[int]:
        """Token ids of a text (or the ids themselves).  Tokenizer protocol: ``encode(text) -> ids`` (with whatever special tokens
        the model expects in front) for prompts; a CONTINUATION carries no special tokens of its own, so a continuation given as
        text needs ``encode(text, add_special_tokens=False)`` (transformers' signature; HashTokenizer has it).  A tokenizer without
        that keyword cannot say what it adds: pass the continuation as token ids then."""
        if not isinstance(x, str):
            return [int(i) for i in x]
        if not continuation:
            return [int(i) for i in self.tokenizer.encode(x)]
        import inspect
        try:
            ps = inspect.signature(self.tokenizer.encode).parameters
            plain = "add_special_tokens" in ps or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in ps.values())
        except (TypeError, ValueError):
            plain = True
        if not plain:
            raise TypeError("score / classify: this tokenizer's encode() has no add_special_tokens keyword, so a continuation given as "
                            "text cannot be tokenised without its special tokens; pass token ids")
        return [int(i) for i in self.tokenizer.encode(x, add_special_tokens=False)]

    def score(self, prompts: Sequence, continuations: Sequence, batch: int = 32):
        """Per (prompt, continuation) pair: ``(logprobs, total)`` -- the log-probability of every continuation token given the prompt
        and the continuation before it (a list of floats), and their sum.  Texts go through the tokenizer (the continuation without
        special tokens), sequences of ints are taken as token ids.  ONE teacher-forced pass over prompt + continuation per pair,
        ``batch`` pairs at a time (right-padded); only the continuation's positions are scored."""
        if len(prompts) != len(continuations):
            raise ValueError("score: one continuation per prompt")
        pairs = [(self._ids_of(p), self._ids_of(c, continuation=True)) for p, c in zip(prompts, continuations)]
        for p, c in pairs:
            if not p or not c:
                raise ValueError("score: a pair needs at least one prompt token (the context of the first scored token) and one continuation token")
        res = []
        step = max(int(batch), 1)
        for c0 in range(0, len(pairs), step):
            chunk = pairs[c0:c0 + step]
            ids, lens = self._pad_batch([p + c for p, c in chunk])
            start = torch.tensor([len(p) for p, _ in chunk], dtype=torch.int32)
            lp = self.token_logprobs(ids, lens, start=start).cpu()
            for i, (p, c) in enumerate(chunk):
                row = lp[i, len(p) - 1: len(p) - 1 + len(c)]
                res.append(([float(v) for v in row], float(row.sum(dtype=torch.float64))))
        return res

    def perplexity(self, texts: Sequence, batch: int = 32) -> float:
        """exp(mean negative log-likelihood) over every scored token of ``texts`` (each token after a text's first)."""
        seqs = [self._ids_of(t) for t in texts]
        total, count = 0.0, 0
        step = max(int(batch), 1)
        for c0 in range(0, len(seqs), step):
            ids, lens = self._pad_batch(seqs[c0:c0 + step])
            total += float(self.token_logprobs(ids, lens).sum(dtype=torch.float64))
            count += int((lens - 1).clamp(min=0).sum())
        if count == 0:
            raise ValueError("perplexity: no text has a second token to score")
        return math.exp(-total / count)

    def classify(self, prompts: Sequence, labels: Sequence, batch: int = 32):
        """Closed-set choice: for each prompt the label whose tokens have the largest SUMMED log-probability after it -- the sum
        decides (it is the log-probability of the label as a whole; the per-token mean favours long labels and is returned for
        inspection only); ties go to the first label.  -> ``(choice, sums, means)``: a list of label indices and two float64 numpy
        arrays ``[prompts, labels]``.  The prompt is replayed once per label (``len(labels)`` rows per prompt in the batch)."""
        p_ids = [self._ids_of(p) for p in prompts]
        l_ids = [self._ids_of(l, continuation=True) for l in labels]
        flat = self.score([p for p in p_ids for _ in l_ids], [l for _ in p_ids for l in l_ids], batch=batch)
        sums = np.array([s for _, s in flat], dtype=np.float64).reshape(len(p_ids), len(l_ids))
        means = sums / np.array([len(l) for l in l_ids], dtype=np.float64)[None, :]
        return [int(i) for i in sums.argmax(axis=1)], sums, means

    # ------------------------------------------------------------------ the reference's call surface
    def _encode(self, text: str) -> List[int]:
        ids = list(self.tokenizer.encode(text))
        return ids[: self.max_length]

    def get_embedding(self, text: str) -> np.ndarray:
        """src/search_milvus.py:75-108 with layer=-1, pooling='mean' -> numpy float32 [hidden]."""
        ids = torch.tensor([self._encode(text)], dtype=torch.int64)
        return self.embed_ids(ids).cpu().numpy()[0]

    def get_embeddings(self, texts: Sequence[str]) -> np.ndarray:
        """Many texts in one right-padded batch; each row equals get_embedding(text) (padding is masked)."""
        enc = [self._encode(t) for t in texts]
        tmax = max(len(e) for e in enc)
        ids = torch.zeros((len(enc), tmax), dtype=torch.int64)
        for i, e in enumerate(enc):
            ids[i, : len(e)] = torch.tensor(e)
        return self.embed_ids(ids, torch.tensor([len(e) for e in enc])).cpu().numpy()

    EMOTION_PROMPT = """\n=======
Context: Given predefined emotional label set [happy, sad, neutral, angry, excited, frustrated], and below conversation:
"
{}
"

Question: What is the emotion of the speaker at the utterance "{}"?
Answer:"""

    def generate_emotion_label(self, text: str, max_new_tokens: int = 10) -> str:
        """milvus/search_json.py:154-198: greedy continuation of the few-shot prompt, decoded (prompt included, as there),
        stripped and lower-cased."""
        return self.generate_emotion_labels([text], max_new_tokens)[0]

    def generate_emotion_labels(self, texts: Sequence[str], max_new_tokens: int = 10) -> List[str]:
        """The labels of several utterances in one batched greedy decode (each equals generate_emotion_label of its text)."""
        prompts = [list(self.tokenizer.encode(self.EMOTION_PROMPT.format(t, t))) for t in texts]    # untruncated: only get_embedding truncates there
        outs = self.generate_greedy_batch(prompts, max_new_tokens)
        dec = (lambda o: self.tokenizer.decode(o, skip_special_tokens=True)) if self._decode_takes_skip else self.tokenizer.decode   # search_json.py:191
        return [dec(o).strip().lower() for o in outs]

    BIOGRAPHY_PROMPT = """
Given this conversation between speakers:
"
{}
"
In overall of above conversation, what do you think about the characteristics of speaker {}? (Note: provide an answer within 250 words)
"""

    def generate_biography(self, full_conversation: str, speaker_name: str, max_new_tokens: int = 250, seed: int = 0) -> str:
        """milvus/search_json.py:113-151: the sampled continuation of the biography prompt, decoded without special tokens, the prompt
        removed, stripped."""
        return self.generate_biographies([(full_conversation, speaker_name)], max_new_tokens, seed)[0]

    def generate_biographies(self, items: Sequence, max_new_tokens: int = 250, seed: int = 0, batch: int = 32, first_index: int = 0) -> List[str]:
        """The biographies of several (conversation, speaker) pairs, ``batch`` prompts per sampled decode.  Pair number i draws from
        ``row_uniforms(seed, first_index + i, ...)`` whatever batch it lands in (``first_index``: the pairs are a slice of a longer list)."""
        items = [(str(c), str(s)) for c, s in items]
        texts = [self.BIOGRAPHY_PROMPT.format(c, s) for c, s in items]
        prompts = [list(self.tokenizer.encode(t)) for t in texts]                                  # untruncated, as tokenizer(prompting) there
        dec = (lambda o: self.tokenizer.decode(o, skip_special_tokens=True)) if self._decode_takes_skip else self.tokenizer.decode
        out: List[str] = []
        n_new = int(max_new_tokens)
        for c0 in range(0, len(items), max(int(batch), 1)):
            idx = range(c0, min(c0 + max(int(batch), 1), len(items)))
            u = torch.stack([self.row_uniforms(seed, first_index + i, max(n_new, 0)) for i in idx], 1)
            rows = self.generate_sample_batch([prompts[i] for i in idx], n_new, uniforms=u)
            out.extend(dec(r).replace(texts[i], "").strip() for i, r in zip(idx, rows))       # :148-150
        return out

    @property
    def _decode_takes_skip(self) -> bool:
        """Decided from the tokenizer's signature, once: a TypeError raised INSIDE a real tokenizer's decode must not be mistaken for
        "this stand-in has no skip_special_tokens argument" (and silently decoded with the special tokens in)."""
        if not hasattr(self, "_decode_skip"):
            import inspect
            try:
                ps = inspect.signature(self.tokenizer.decode).parameters
                self._decode_skip = "skip_special_tokens" in ps or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in ps.values())
            except (TypeError, ValueError):
                self._decode_skip = True
        return self._decode_skip

    def combined_embedding(self, emotion_text: str, biography_text: str) -> np.ndarray:
        """milvus/search_json.py:201-229 / src/search_milvus.py:214-221: [emotion | biography] float32, un-normalised."""
        e = self.get_embeddings([emotion_text, biography_text])
        return np.concatenate((e[0], e[1])).astype(np.float32)


def _merge_lora(state: dict, lora) -> dict:
    """W + scaling * B A in fp32 for the fp16 path (the int8 path keeps the branch unmerged, as peft does)."""
    from .peft import PROJ

    out = dict(state)
    for (i, p), (a, b) in lora.pairs.items():
        k = f"model.layers.{i}.{PROJ[p]}.weight"
        out[k] = state[k].float() + lora.scaling * (b.float() @ a.float())
    return out
