"""The query embedder on the GPU: Llama-3.2 decoder forward -> mean-pooled last hidden state, the greedy continuation that names
the emotion, the sampled one that writes a biography, and the scoring of given continuations.

Replaces, in the reference's retrieval scripts (paths under /root/reference):
    get_embedding(text, model, tokenizer, device, layer=-1, pooling='mean')   src/search_milvus.py:75-108
                                                                              (same function: milvus/search_json.py:76-109)
    generate_emotion_label(text, ...)  -> model.generate(do_sample=False)     milvus/search_json.py:154-198
    create_combined_embedding(...)     -> concatenate(emotion, biography)     milvus/search_json.py:201-229,
                                                                              src/search_milvus.py:214-221
The model itself -- weights (fp16, or LLM.int8 + LoRA), RoPE tables, the layer stack -- is astts.llm.decoder.LlamaDecoder; the
tokenizer protocol and its stand-in are astts.llm.tokenizer.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from .config import LlamaShape
from .decoder import LlamaDecoder, llama3_inv_freq  # noqa: F401  (llama3_inv_freq: imported from here by its users)
from .tokenizer import HashTokenizer, decode_clean, encode_continuation


class LlamaEmbedder(LlamaDecoder):
    def __init__(self, state: dict, cfg: LlamaShape, device=None, tokenizer=None, max_length: int = 512, int8: bool = False, lora=None, int8_threshold: float = 6.0):
        super().__init__(state, cfg, device, int8=int8, lora=lora, int8_threshold=int8_threshold, rope_len=max(max_length, 16) + 64)
        self.tokenizer = tokenizer or HashTokenizer(cfg)
        self.max_length = max_length                                  # truncation=True, max_length=512: src/search_milvus.py:92

    def _adopted(self, tokenizer=None, max_length: int = 512) -> None:
        """LlamaDecoder.adopt's hook: ``LlamaEmbedder.adopt(base, layers, rope_len, tokenizer=..., max_length=...)``."""
        self.tokenizer = tokenizer or HashTokenizer(self.cfg)
        self.max_length = max_length

    def _is_eos(self, tok: int) -> bool:
        return tok == self.cfg.eos_token_id or tok in self.cfg.eos_token_ids

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
        Prompts are LEFT-padded to a common length, time-major ``[T, B]``: the layout of ``hidden_cached``."""
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
        ids = torch.zeros((t, b), dtype=torch.int32)
        for j, p in enumerate(prompts):
            ids[t - lens[j]:, j] = torch.tensor(p, dtype=torch.int32)
        start = torch.tensor([t - n for n in lens], dtype=torch.int32, device=dev)
        cache = [torch.empty((t + n_new, b, 2 * cfg.kv_heads * cfg.head_dim), dtype=torch.float16, device=dev) for _ in self.L]
        toks = torch.zeros((n_new, b), dtype=torch.int32, device=dev)
        seg_prefill, seg_step = self._segments(b, t, start=start), self._segments(b)          # LLM.int8: the prompts' tokens; one row per decode step
        logits = torch.empty((n_new, b, cfg.vocab), dtype=torch.float32, device=dev) if keep_logits else None
        eos = torch.tensor(sorted({int(cfg.eos_token_id), *(int(e) for e in cfg.eos_token_ids)}), dtype=torch.int32, device=dev) if poll > 0 else None
        x = ops.embedding(self.embed, ids.to(dev))
        for s in range(n_new):
            h_last = self.hidden_cached(x, cache, 0 if s == 0 else t + s - 1, start, seg_prefill if s == 0 else seg_step)
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
        """Token ids of a text (or the ids themselves); a continuation carries no special tokens of its own (``encode_continuation``)."""
        if not isinstance(x, str):
            return [int(i) for i in x]
        return encode_continuation(self.tokenizer, x) if continuation else [int(i) for i in self.tokenizer.encode(x)]

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
        return list(self.tokenizer.encode(text))[: self.max_length]

    def get_embedding(self, text: str) -> np.ndarray:
        """src/search_milvus.py:75-108 with layer=-1, pooling='mean' -> numpy float32 [hidden]."""
        ids = torch.tensor([self._encode(text)], dtype=torch.int64)
        return self.embed_ids(ids).cpu().numpy()[0]

    def get_embeddings(self, texts: Sequence[str]) -> np.ndarray:
        """Many texts in one right-padded batch; each row equals get_embedding(text) (padding is masked)."""
        ids, lens = self._pad_batch([self._encode(t) for t in texts])
        return self.embed_ids(ids, lens).cpu().numpy()

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
        return [decode_clean(self.tokenizer, o).strip().lower() for o in outs]                     # search_json.py:191

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
        out: List[str] = []
        n_new = int(max_new_tokens)
        for c0 in range(0, len(items), max(int(batch), 1)):
            idx = range(c0, min(c0 + max(int(batch), 1), len(items)))
            u = torch.stack([self.row_uniforms(seed, first_index + i, max(n_new, 0)) for i in idx], 1)
            rows = self.generate_sample_batch([prompts[i] for i in idx], n_new, uniforms=u)
            out.extend(decode_clean(self.tokenizer, r).replace(texts[i], "").strip() for i, r in zip(idx, rows))       # :148-150
        return out

    def combined_embedding(self, emotion_text: str, biography_text: str) -> np.ndarray:
        """milvus/search_json.py:201-229 / src/search_milvus.py:214-221: [emotion | biography] float32, un-normalised."""
        e = self.get_embeddings([emotion_text, biography_text])
        return np.concatenate((e[0], e[1])).astype(np.float32)
