"""BERT-family sentence encoders on the GPU (m3e, bge, multilingual-e5: transformers' BertModel / RobertaModel / XLMRobertaModel without
the pooler): the second kind of model that may sit in front of the style bank, next to the causal decoders of astts.llm.decoder.  The
reference names "Moka embeddings" (m3e-base, 768-d) beside its Llama embedder (README.md:16); ``BertEmbedder`` has the calls the retrieval
CLIs make on ``LlamaEmbedder`` (``get_embedding``, ``get_embeddings``, ``combined_embedding``, ``embed_ids``, ``cfg.hidden``) and none
of its generation methods.

Every tensor operation is a HIP kernel of libastts.so.  One post-LayerNorm layer (DESIGN.md section 2 "BERT-family encoders"):

    qkv  = x16 Wqkv^T + b            one fused GEMM, fp16 [rows, 3 hidden]                                   astts_op_gemm
    a    = softmax(q k^T / 8) v      bidirectional, keys at or beyond lens masked, fp16                      astts_op_attn_mha
    x32  = a Wo^T + b + x32          fp32                                                                    astts_op_gemm
    x32, x16 = LayerNorm(x32)        fp32 for the residual stream, the same value as fp16 for the next GEMM  astts_op_layernorm_dual
    f    = gelu(x16 Wi^T + b)        exact-erf GELU in the epilogue, fp16                                    astts_op_gemm
    x32  = f Wo2^T + b + x32         fp32                                                                    astts_op_gemm
    x32, x16 = LayerNorm(x32)                                                                                astts_op_layernorm_dual

behind ``LayerNorm(word[id] + pos[pos_offset + j] + type[type_id])`` in one launch (astts_op_bert_embed_ln).  The residual stream and
every LayerNorm are fp32; GEMM operands, q | k | v, the attention output and the GELU output are fp16.  Parity: tests/test_bert_gpu.py
against fixtures produced by transformers (fp32) on seeded weights.
"""
from __future__ import annotations

import zlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..frontend_nets import l2_normalize
from .bert_dir import SentenceSetup
from .config import BertShape
from .weights import bert_weight_shapes


class HashBertTokenizer:
    """STAND-IN for a directory without tokenizer files, as astts.llm.tokenizer.HashTokenizer is for the decoders: [CLS] + one id per
    whitespace-separated word by a fixed hash + [SEP].  Good for plumbing and benchmarks only."""

    def __init__(self, shape: BertShape):
        self.vocab = shape.vocab
        roberta = shape.model_type != "bert"
        self.cls_id, self.sep_id = (0, 2) if roberta else ((101, 102) if shape.vocab > 103 else (1, 2))
        self.first = 3 if roberta or shape.vocab <= 103 else 103
        if shape.vocab < self.first + 8:
            raise ValueError(f"HashBertTokenizer: a vocabulary of {shape.vocab} entries leaves fewer than 8 ids behind the special tokens "
                             f"(ids below {self.first}) for the words")

    def encode(self, text: str, add_special_tokens: bool = True) -> List[int]:
        words = [self.first + zlib.crc32(w.encode("utf-8")) % (self.vocab - self.first) for w in text.split()]
        return [self.cls_id] + words + [self.sep_id] if add_special_tokens else words


def embed_in_length_order(seqs: Sequence[Sequence[int]], embed, batch: int, pad_id: int, width: int) -> np.ndarray:
    """``embed(ids int64 [n, T], lens int32 [n]) -> [n, width]`` over token rows sorted by length, ``batch`` rows to a right-padded
    batch, so that a five-token label does not pay for a 250-token biography -> float32 [len(seqs), width] in the CALLER's order."""
    out = np.zeros((len(seqs), width), np.float32)
    order = sorted(range(len(seqs)), key=lambda i: len(seqs[i]))
    step = max(int(batch), 1)
    for c0 in range(0, len(order), step):
        chunk = order[c0:c0 + step]
        ids = torch.full((len(chunk), max(len(seqs[i]) for i in chunk)), int(pad_id), dtype=torch.int64)
        for r, i in enumerate(chunk):
            ids[r, :len(seqs[i])] = torch.tensor(list(seqs[i]), dtype=torch.int64)
        out[chunk] = np.asarray(embed(ids, torch.tensor([len(seqs[i]) for i in chunk], dtype=torch.int32)), np.float32)
    return out


class BertEncoder:
    """The layer stack: ``hidden(ids, lens, type_ids)`` -> the last layer's token states."""

    def __init__(self, state: dict, cfg: BertShape, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("astts.llm needs a ROCm GPU; there is no CPU fallback in the product path")
        if cfg.head_dim != 64 or cfg.heads * 64 != cfg.hidden:
            raise ValueError(f"BertEncoder: hidden {cfg.hidden} / heads {cfg.heads}: the attention kernel is built for a head dimension of 64")
        if cfg.hidden % 8 or cfg.hidden > 4096:
            raise ValueError(f"BertEncoder: hidden {cfg.hidden}: the LayerNorm kernel is built for multiples of 8 up to 4096")
        want = bert_weight_shapes(cfg)
        wrong = [k for k in want if k not in state or tuple(state[k].shape) != want[k]] + [k for k in state if k not in want]
        if wrong:
            raise ValueError(f"BertEncoder: the state dict does not fit this {cfg.model_type} shape (missing, extra or mis-shaped): {sorted(wrong)[:3]}")
        self.cfg = cfg
        self.device = dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            f = lambda k: state[k].to(device=dev, dtype=torch.float32).contiguous()
            e = "embeddings."
            self.word, self.pos, self.type = f(e + "word_embeddings.weight"), f(e + "position_embeddings.weight"), f(e + "token_type_embeddings.weight")
            self.emb_ln = (f(e + "LayerNorm.weight"), f(e + "LayerNorm.bias"))

            def pack(i: int, *names: str) -> ops.PackedWeight:
                p = f"encoder.layer.{i}."
                return ops.PackedWeight(torch.cat([state[p + nm + ".weight"].float() for nm in names], 0),
                                        torch.cat([state[p + nm + ".bias"].float() for nm in names]), dev)

            self.L = [{"wqkv": pack(i, "attention.self.query", "attention.self.key", "attention.self.value"),
                       "wo": pack(i, "attention.output.dense"), "wi": pack(i, "intermediate.dense"), "wo2": pack(i, "output.dense"),
                       "ln1": (f(f"encoder.layer.{i}.attention.output.LayerNorm.weight"), f(f"encoder.layer.{i}.attention.output.LayerNorm.bias")),
                       "ln2": (f(f"encoder.layer.{i}.output.LayerNorm.weight"), f(f"encoder.layer.{i}.output.LayerNorm.bias"))}
                      for i in range(cfg.layers)]

    def _layer(self, x32: torch.Tensor, x16: torch.Tensor, L: dict, lens: Optional[torch.Tensor]):
        """One encoder layer: the fp32 residual stream ``x32`` and its fp16 copy ``x16`` (both LayerNorm outputs) -> the next pair."""
        h, eps = self.cfg.hidden, self.cfg.ln_eps
        qkv = ops.linear(x16, L["wqkv"], out_dtype=torch.float16)
        a = ops.attn_mha(qkv[..., :h], qkv[..., h:2 * h], qkv[..., 2 * h:], self.cfg.heads, lens=lens, out_dtype=torch.float16)
        x32, x16 = ops.layernorm_dual(ops.linear(a, L["wo"], residual=x32), *L["ln1"], eps, inplace=True)
        f = ops.linear(x16, L["wi"], act="gelu", out_dtype=torch.float16)
        return ops.layernorm_dual(ops.linear(f, L["wo2"], residual=x32), *L["ln2"], eps, inplace=True)

    def _checked(self, ids, lens, type_ids):
        """The range checks the kernels do not make (they clamp): on the host, before anything is uploaded."""
        cfg = self.cfg
        ids = torch.as_tensor(ids).cpu()
        if ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
            raise ValueError(f"ids {tuple(ids.shape)}: expected [B, T] with B, T >= 1")
        b, t = ids.shape
        if t + cfg.pos_offset > cfg.max_positions:
            raise ValueError(f"{t} tokens (positions from {cfg.pos_offset}) exceed the {cfg.max_positions} rows of the position table")
        if int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab:
            raise ValueError(f"token ids outside [0, {cfg.vocab}): min {int(ids.min())}, max {int(ids.max())}")
        if lens is not None:
            lens = torch.as_tensor(lens).cpu()
            if tuple(lens.shape) != (b,) or int(lens.min()) < 1 or int(lens.max()) > t:
                raise ValueError(f"lens {lens.tolist()}: expected [B] = {b} values in [1, {t}]")
        if type_ids is not None:
            type_ids = torch.as_tensor(type_ids).cpu()
            if tuple(type_ids.shape) != (b, t) or int(type_ids.min()) < 0 or int(type_ids.max()) >= cfg.type_vocab:
                raise ValueError(f"type_ids {tuple(type_ids.shape)}: expected {(b, t)} values in [0, {cfg.type_vocab})")
        up = lambda x: None if x is None else x.to(device=self.device, dtype=torch.int32).contiguous()
        return up(ids), up(lens), up(type_ids)

    def hidden(self, ids, lens=None, type_ids=None) -> torch.Tensor:
        """ids int [B, T] (right-padded), lens int [B] or None, type_ids int [B, T] or None (all 0) -> the last layer's hidden states fp32
        [B, T, hidden] (== last_hidden_state of BertModel / XLMRobertaModel on the real positions; what padding rows hold is unspecified).
        Raises ValueError for ids, type ids or a length outside the tables."""
        return self._hidden(*self._checked(ids, lens, type_ids))

    def _hidden(self, ids: torch.Tensor, lens: Optional[torch.Tensor], type_ids: Optional[torch.Tensor]) -> torch.Tensor:
        """``hidden`` on what ``_checked`` returned: int32 tensors on the device."""
        with torch.cuda.device(self.device):
            x32, x16 = ops.bert_embed_ln(self.word, self.pos, self.type, ids, type_ids, lens, *self.emb_ln, self.cfg.pos_offset, self.cfg.ln_eps)
            for L in self.L:
                x32, x16 = self._layer(x32, x16, L, lens)
        return x32


class BertEmbedder(BertEncoder):
    def __init__(self, state: dict, cfg: BertShape, device=None, tokenizer=None, setup: Optional[SentenceSetup] = None, batch: int = 32):
        super().__init__(state, cfg, device)
        self.setup = setup or SentenceSetup("mean", False, min(512, cfg.max_tokens))
        if self.setup.pooling not in ("mean", "cls"):
            raise ValueError(f"pooling {self.setup.pooling!r}: 'mean' or 'cls'")
        if not 2 <= self.setup.max_seq_length <= cfg.max_tokens:
            raise ValueError(f"max_seq_length {self.setup.max_seq_length}: between 2 and the {cfg.max_tokens} positions of the table")
        self.tokenizer = tokenizer or HashBertTokenizer(cfg)
        self.batch = int(batch)

    max_length = property(lambda self: self.setup.max_seq_length)

    def embed_ids(self, ids, lens=None, type_ids=None) -> torch.Tensor:
        """The sentence vectors of token rows -> fp32 [B, hidden] on the GPU: mean over each row's real tokens, or its first token's
        state, L2-normalised when the directory says so."""
        ids, lens, type_ids = self._checked(ids, lens, type_ids)             # one upload: the pooling reads the same lens
        h = self._hidden(ids, lens, type_ids)
        with torch.cuda.device(self.device):
            e = h[:, 0].contiguous() if self.setup.pooling == "cls" else ops.mean_pool(h, lens)
            return l2_normalize(e) if self.setup.normalize else e

    def _encode(self, text: str) -> List[int]:
        """The tokenizer's ids ([CLS] ... [SEP]) cut to max_seq_length the way transformers truncates one sequence: the LAST token (the
        closing special token) stays.  An empty text is [CLS][SEP]."""
        ids = [int(i) for i in self.tokenizer.encode(text)]
        if len(ids) < 2:
            raise ValueError(f"the tokenizer returned {len(ids)} token(s) for {text[:40]!r}: it does not add [CLS] / [SEP]")
        n = self.max_length
        return ids if len(ids) <= n else ids[:n - 1] + ids[-1:]

    def get_embedding(self, text: str) -> np.ndarray:
        return self.get_embeddings([text])[0]

    def get_embeddings(self, texts: Sequence[str]) -> np.ndarray:
        """numpy float32 [len(texts), hidden], row i for texts[i] (``embed_in_length_order``; padding is masked, so a row does not
        depend on its batch)."""
        return embed_in_length_order([self._encode(t) for t in texts], lambda ids, lens: self.embed_ids(ids, lens).cpu().numpy(),
                                     self.batch, self.cfg.pad_token_id, self.cfg.hidden)

    def combined_embedding(self, emotion_text: str, biography_text: str) -> np.ndarray:
        """[emotion | biography] float32, 2 x hidden: the style-bank query of milvus/search_json.py:201-229 on this encoder."""
        e = self.get_embeddings([emotion_text, biography_text])
        return np.concatenate((e[0], e[1])).astype(np.float32)
