"""The acoustic transformer (text encoder + causal LM body) and its C++ decode engine (libastts ``astts_lm_*``)."""
from __future__ import annotations

import ctypes
import math
import os
import threading
from typing import List, Optional

import torch

from .. import _lib, ops
from ..ops import PackedWeight
from .config import SynthConfig
from .decode import DecodeJob, LmSession, Prefill, _eos_min, decode_groups
from .encoder import SD, RelPosEncoder, _dev, fold_layernorm


class AcousticLM:
    """TransformerLM: text encoder + causal rel-pos transformer with a time-major KV cache
    ``[T_max, B, 2d]`` per layer (the K|V GEMM writes straight into the cache rows of the new positions)."""

    def __init__(self, sd: SD, cfg: SynthConfig, device):
        self.cfg, self.device = cfg, device
        self.text_emb = _dev(sd["text_embedding.weight"], device)
        self.text_enc = RelPosEncoder(sd, "text_encoder", cfg.lm_heads, cfg.lm_text_layers, "swish",
                                      ("norm_mha", "norm_ff"), False, True, cfg.ln_eps, cfg.max_positions, device)
        self.text_aff = PackedWeight(sd["text_encoder_affine_layer.weight"], sd["text_encoder_affine_layer.bias"], device)
        self.llm_emb = _dev(sd["llm_embedding.weight"], device)
        self.speech_emb = _dev(sd["speech_embedding.weight"], device)
        self.spk_aff = PackedWeight(sd["spk_embed_affine_layer.weight"], sd["spk_embed_affine_layer.bias"], device)
        # the LM body re-reads its position tables and KV cache every decode step: both live in HBM as fp16
        self.body = RelPosEncoder(sd, "llm", cfg.lm_heads, cfg.lm_layers, "relu", ("norm1", "norm2"), True, True,
                                  cfg.ln_eps, cfg.max_positions, device, pos_dtype=torch.float16, fold_ln=True)
        # after_norm is only ever followed by the output head: folded into it (the body's `after` is the identity affine)
        hw, hb = fold_layernorm(sd["llm_decoder.weight"].float().cpu(), sd["llm_decoder.bias"].float().cpu(),
                                sd["llm.after_norm.weight"].float().cpu(), sd["llm.after_norm.bias"].float().cpu())
        self.head = PackedWeight(hw, hb, device)
        self._eng_lock = threading.Lock()

    def prefix(self, text: torch.Tensor, text_lens: torch.Tensor, spk: torch.Tensor, prompt_tokens: torch.Tensor) -> torch.Tensor:
        """-> time-major [S0, B, d]: sos | spk | text_encoder(text) | task_id | speech_emb(prompt)."""
        b = text.shape[0]
        te = ops.embedding(self.text_emb, text)
        enc = ops.linear(self.text_enc.forward(te, text_lens), self.text_aff)
        spk_n = torch.nn.functional.normalize(spk, dim=1)  # 192-vector per utterance: host-side plumbing
        spk_e = ops.linear(spk_n, self.spk_aff)[:, None, :]
        sos = self.llm_emb[0].view(1, 1, -1).expand(b, 1, -1)
        task = self.llm_emb[1].view(1, 1, -1).expand(b, 1, -1)
        pe = ops.embedding(self.speech_emb, prompt_tokens)
        return torch.cat([sos, spk_e, enc, task, pe], dim=1).transpose(0, 1).contiguous()

    def new_cache(self, b: int, t_max: int) -> List[torch.Tensor]:
        if t_max > self.body.center:      # relative positions 0 .. t_max - 1 must be rows of the tables
            raise ValueError(f"AcousticLM: a context of {t_max} positions exceeds the relative-position tables "
                             f"(SynthConfig.max_positions = {self.body.center})")
        return [torch.empty((t_max, b, 2 * self.body.d), dtype=torch.float16, device=self.device) for _ in self.body.L]

    def prefix_ragged(self, texts: List[torch.Tensor], spk: torch.Tensor, prompts: List[torch.Tensor]):
        """Ragged batch: row i has its own text length and prompt length.  Rows are LEFT-padded to the longest
        prefix (relative-position attention is translation invariant, so masking the pad keys is exact):
        -> (prefix [S0, B, d] time-major, key_start int32 [B])."""
        b = len(texts)
        dev = self.device
        tl = [int(t.numel()) for t in texts]
        tmax = max(tl)
        text = torch.zeros((b, tmax), dtype=torch.int64, device=dev)
        for i, t in enumerate(texts):
            text[i, :tl[i]] = t.to(dev).view(-1)
        text_lens = torch.tensor(tl, dtype=torch.int32, device=dev)
        te = ops.embedding(self.text_emb, text)
        enc = ops.linear(self.text_enc.forward(te, text_lens), self.text_aff)      # suffix padding + causal: exact
        spk_e = ops.linear(torch.nn.functional.normalize(spk.to(dev), dim=1), self.spk_aff)
        s0 = [2 + tl[i] + 1 + int(prompts[i].numel()) for i in range(b)]
        smax = max(s0)
        pre = torch.zeros((b, smax, self.body.d), dtype=torch.float32, device=dev)
        for i in range(b):                                                          # host-side assembly (plumbing)
            o = smax - s0[i]
            pre[i, o] = self.llm_emb[0]
            pre[i, o + 1] = spk_e[i]
            pre[i, o + 2:o + 2 + tl[i]] = enc[i, :tl[i]]
            pre[i, o + 2 + tl[i]] = self.llm_emb[1]
            pre[i, o + 3 + tl[i]:] = ops.embedding(self.speech_emb, prompts[i].to(dev).view(1, -1))[0]
        key_start = torch.tensor([smax - s for s in s0], dtype=torch.int32, device=dev)
        return pre.transpose(0, 1).contiguous(), key_start

    def forward_new(self, x: torch.Tensor, cache: List[torch.Tensor], pos0: int, key_start: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: time-major [T, B, d] NEW positions pos0..pos0+T-1 -> hidden [T, B, d]; fills the cache."""
        body = self.body
        d = body.d
        t, b = x.shape[0], x.shape[1]
        h = body.embed_in(x)
        tk = pos0 + t
        lens = torch.full((b,), tk, dtype=torch.int32, device=self.device)
        for lay, kvc in zip(body.L, cache):
            n = ops.layernorm(h, *lay["n1"], body.eps)
            q = ops.linear(n, lay["wq"])
            ops.gemm(n.view(t * b, d), lay["wkv"], out=kvc[pos0:pos0 + t].view(t * b, 2 * d))
            kv = kvc[:tk]
            a = ops.attn_relpos(q, kv[..., :d], kv[..., d:], lay["pos"], lay["u"], lay["v"], body.heads, lens=lens,
                                q_pos0=pos0, pos_center=body.center, causal=True, time_major=True, key_start=key_start)
            h = ops.linear(a, lay["wo"], residual=h)
            n = ops.layernorm(h, *lay["n2"], body.eps)
            f = ops.linear(n, lay["w1"], act="relu")
            h = ops.linear(f, lay["w2"], residual=h)
        return ops.layernorm(h, *body.after, body.eps)

    def logits(self, hidden_last: torch.Tensor) -> torch.Tensor:
        return ops.linear(hidden_last, self.head)

    def step_logits(self, tok: torch.Tensor, cache: List[torch.Tensor], pos: int, key_start: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One decode step for B <= 32 utterances with the launch-saving fusions of astts_op_gemm_fused:
        embedding gather inside the embed GEMM, LayerNorm inside the QKV / FFN-in / head GEMMs, K|V written
        straight into the cache.  5 launches per layer.  tok int32 [B] -> logits [B, V+1]."""
        body = self.body
        d, b = body.d, tok.shape[0]
        h = ops.gemm_fused(self.speech_emb, body.embed, b, gather=tok)
        h = ops.layernorm(h, *body.embed_ln, body.eps, relu_scale=math.sqrt(d))
        lens = torch.full((b,), pos + 1, dtype=torch.int32, device=self.device)
        for lay, kvc in zip(body.L, cache):
            q = ops.gemm_fused(h, lay["wqkv"], b, ln=lay["n1"], ln_eps=body.eps, out2=kvc[pos], n_split=d)
            kv = kvc[:pos + 1]
            a = ops.attn_relpos(q[None], kv[..., :d], kv[..., d:], lay["pos"], lay["u"], lay["v"], body.heads, lens=lens,
                                q_pos0=pos, pos_center=body.center, causal=True, time_major=True, key_start=key_start)
            h = ops.gemm_fused(a[0], lay["wo"], b, residual=h)
            f = ops.gemm_fused(h, lay["w1"], b, ln=lay["n2"], ln_eps=body.eps, act="relu")
            h = ops.gemm_fused(f, lay["w2"], b, residual=h)
        return ops.gemm_fused(h, self.head, b, ln=body.after, ln_eps=body.eps)

    # ---- C++ decode engine (libastts astts_lm_*): same fused step, issued without Python in the loop
    def _engine(self):
        if getattr(self, "_eng", None) is not None:
            return self._eng
        with self._eng_lock:            # decode groups run on several host threads: ONE of them builds the handle and its table
            return self._engine_locked()

    def _engine_locked(self):
        if getattr(self, "_eng", None) is None:
            body, cfg = self.body, self.cfg
            c = ops.LmConfig(body.d, body.heads, cfg.lm_ffn, len(body.L), cfg.speech_vocab + 1, cfg.speech_vocab, body.center,
                             body.L[0]["pos"].stride(0), cfg.top_k, cfg.ras_win, cfg.top_p, cfg.ras_tau, body.eps, 1, 1,
                             1 if body.fold_ln else 0, 1 if cfg.eos_policy == "reject" else 0)
            # the decode step's input projection acts on a table lookup: speech_emb[tok] W^T + b is a row of the table
            # speech_emb W^T + b, formed once here (the same fp16 products on the GPU; the big-tile GEMM sums them in another fp32
            # order than the step's GEMV, so the two paths agree to rounding, not bit for bit: tests/test_lm_step_gpu.py) and
            # gathered by the step.  ASTTS_LM_EMBED_TABLE=0: no table, the projection runs every step (the engine's other branch).
            self.embed_table = ops.linear(self.speech_emb, body.embed).contiguous() if os.environ.get("ASTTS_LM_EMBED_TABLE", "1") != "0" else None
            torch.cuda.current_stream(self.device).synchronize()     # one-off: decode chains on OTHER streams read the table
            g = ops.LmGlobals(self.speech_emb.data_ptr(), body.embed.data.data_ptr(), body.embed.bias.data_ptr(),
                              body.embed_ln[0].data_ptr(), body.embed_ln[1].data_ptr(), body.after[0].data_ptr(),
                              body.after[1].data_ptr(), self.head.data.data_ptr(), self.head.bias.data_ptr(),
                              None if self.embed_table is None else self.embed_table.data_ptr())
            arr = (ops.LmLayer * len(body.L))()
            for i, L in enumerate(body.L):
                arr[i] = ops.LmLayer(L["n1"][0].data_ptr(), L["n1"][1].data_ptr(), L["wqkv"].data.data_ptr(), L["wqkv"].bias.data_ptr(),
                                     L["wo"].data.data_ptr(), L["wo"].bias.data_ptr(), L["n2"][0].data_ptr(), L["n2"][1].data_ptr(),
                                     L["w1"].data.data_ptr(), L["w1"].bias.data_ptr(), L["w2"].data.data_ptr(), L["w2"].bias.data_ptr(),
                                     L["pos"].data_ptr(), L["u"].data_ptr(), L["v"].data_ptr())
            h = ctypes.c_void_p()
            _lib.check(_lib.load().astts_lm_create(ctypes.byref(c), ctypes.byref(g), arr, ctypes.byref(h)))
            self._eng = h
        return self._eng

    def prefill(self, prefix: torch.Tensor, n_steps: int, key_start: Optional[torch.Tensor] = None) -> Prefill:
        """The part of a decode call that does not depend on the sampler: the KV cache of the prefix and the logits of its last
        position, on the CURRENT stream.  -> state for `decode_prefilled` (which may run on another stream: the pipeline enqueues
        this on its front stream so that a decode chain is nothing but its steps)."""
        s0, b = prefix.shape[0], prefix.shape[1]
        cache = self.new_cache(b, s0 + n_steps)
        hid = self.forward_new(prefix, cache, 0, key_start)
        logits0 = self.logits(hid[-1]).contiguous()
        return Prefill(cache, logits0, s0, b, n_steps, key_start)

    @staticmethod
    def prefill_tensors(state: Prefill) -> List[torch.Tensor]:
        return state.tensors()

    def decode_begin(self, state: Prefill, uniforms: torch.Tensor, ignore_eos=True, forced_tokens: Optional[torch.Tensor] = None,
                     return_logits: bool = False) -> DecodeJob:
        """The buffers of one decode of `prefill`'s state (b <= 32 rows): token history, workspace (it carries the logits from one
        range of steps to the next), uniforms.  -> job for `decode_range`."""
        need = int(_lib.load().astts_lm_workspace_bytes(self._engine(), state.b))
        ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        job = DecodeJob.begin(state, self.cfg.speech_vocab + 1, uniforms, ignore_eos, forced_tokens, return_logits)
        job.ws, job.ws_aligned, job.ws_bytes = ws, (ws.data_ptr() + 255) // 256 * 256, need
        return job

    def decode_range(self, job: DecodeJob, s_end: Optional[int] = None) -> None:
        """Enqueue decode steps [job.next, s_end) on the CURRENT stream (one C++ call, no host synchronisation).  The ranges of
        one decode must be issued in order on one stream (astts_lm_decode)."""
        job.decode(_lib.load(), self._engine(), s_end, _lib.stream_ptr())

    def decode_prefilled(self, state: Prefill, uniforms: torch.Tensor, ignore_eos: bool = True, forced_tokens: Optional[torch.Tensor] = None,
                         return_logits: bool = False):
        """The decode steps of `prefill`'s state (b <= 32 rows) on the current stream: one C++ call, no host synchronisation."""
        job = self.decode_begin(state, uniforms, ignore_eos, forced_tokens, return_logits)
        self.decode_range(job)
        self._keepalive = job            # buffers referenced by kernels still in flight
        return (job.toks, job.logits) if return_logits else job.toks

    def decode_engine(self, prefix: torch.Tensor, n_steps: int, uniforms: torch.Tensor, ignore_eos: bool = True,
                      forced_tokens: Optional[torch.Tensor] = None, return_logits: bool = False,
                      key_start: Optional[torch.Tensor] = None):
        return self.decode_prefilled(self.prefill(prefix, n_steps, key_start), uniforms, ignore_eos, forced_tokens, return_logits)

    def session(self, rows_max: int, t_arena: int, stream=None) -> LmSession:
        """A decode chain that a second batch can join while the first is decoding (LmSession)."""
        return LmSession(self, rows_max, t_arena, stream)

    WIDE_ROWS = 256      # ASTTS_LM_MAX_ROWS: rows of one wide-engine call

    def decode(self, prefix: torch.Tensor, n_steps: int, uniforms: torch.Tensor, ignore_eos: bool = True,
               forced_tokens: Optional[torch.Tensor] = None, return_logits: bool = False, use_engine: bool = True,
               key_start: Optional[torch.Tensor] = None, group_steps: Optional[List[int]] = None, wide: bool = False):
        """Fixed-length autoregressive decode, no host synchronisation inside the loop.
        prefix: [S0, B, d]; uniforms [n_steps, B, 2] -> tokens int32 [B, n_steps] (+ logits [B, n_steps, V+1]).
        ``wide`` (throughput runs): batches of 33 .. 256 rows go through ONE chain of plain GEMMs per projection (the engine's wide
        path: the weights are read once per token for all rows) instead of 32-row groups on two streams.  Same fp16 products with fp32
        accumulation, another summation order: a row's tokens then need not equal its <= 32-row run bit for bit (the default keeps the
        groups, whose rows do)."""
        b = prefix.shape[1]
        if not use_engine:
            return self.decode_ops(prefix, n_steps, uniforms, ignore_eos, forced_tokens, return_logits, key_start)
        if b <= 32 or (wide and b <= self.WIDE_ROWS):
            return self.decode_engine(prefix, n_steps, uniforms, ignore_eos, forced_tokens, return_logits, key_start)
        return decode_groups(self, prefix, n_steps, uniforms, ignore_eos, forced_tokens, return_logits, key_start, group_steps)

    def decode_ops(self, prefix: torch.Tensor, n_steps: int, uniforms: torch.Tensor, ignore_eos: bool = True,
                   forced_tokens: Optional[torch.Tensor] = None, return_logits: bool = False,
                   key_start: Optional[torch.Tensor] = None):
        """The same decode, one Python call per operator (the form the C++ engine is checked against)."""
        cfg = self.cfg
        s0, b = prefix.shape[0], prefix.shape[1]
        cache = self.new_cache(b, s0 + n_steps)
        hid = self.forward_new(prefix, cache, 0, key_start)
        cur = self.logits(hid[-1])
        toks = torch.zeros((b, n_steps), dtype=torch.int32, device=self.device)
        all_logits = [] if return_logits else None
        for s in range(n_steps):
            if return_logits:
                all_logits.append(cur)
            tok = ops.ras_sample(cur, toks, s, uniforms[s], cfg.top_k, cfg.top_p, cfg.ras_win, cfg.ras_tau,
                                 cfg.speech_vocab, s < _eos_min(ignore_eos, n_steps), eos_policy=cfg.eos_policy)
            if forced_tokens is not None:
                tok = forced_tokens[:, s].to(torch.int32).contiguous()
            toks[:, s] = tok
            if s + 1 < n_steps:
                if b <= 32:
                    cur = self.step_logits(tok.clamp(max=cfg.speech_vocab - 1), cache, s0 + s, key_start)
                else:
                    emb = ops.embedding(self.speech_emb, tok)[None]        # [1, B, d]
                    hid = self.forward_new(emb, cache, s0 + s, key_start)
                    cur = self.logits(hid[0])
        if return_logits:
            return toks, torch.stack(all_logits, dim=1)
        return toks
