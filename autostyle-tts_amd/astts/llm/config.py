"""Shapes of the embedder LLM.  The reference loads "Llama 3.2" 3B (src/search_milvus.py:251-252, milvus/RAG.py:458:
hidden 3072 -> 2 x 3072 = the 6144-d bank); these are that checkpoint's config.json values.  The same dataclass describes a Qwen2
checkpoint (the reference's ``_cn`` scripts run Qwen2.5-7B-Instruct): ``model_type``, ``qkv_bias`` and ``rope_type`` carry the differences.
A Qwen3 checkpoint adds ``qk_norm`` (a per-head RMSNorm of q and k before RoPE) and a ``head_dim`` that is not hidden / heads.
``BertShape`` is the other family in front of the style bank: the BERT-type sentence encoders (m3e, bge, e5) of astts.llm.encoder_bert."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class LlamaShape:
    vocab: int = 128256
    hidden: int = 3072
    layers: int = 28
    heads: int = 24
    kv_heads: int = 8
    head_dim: int = 128
    ffn: int = 8192
    rms_eps: float = 1e-5
    rope_theta: float = 500000.0
    # rope_scaling {"rope_type": "llama3"}
    rope_factor: float = 32.0
    rope_low_freq_factor: float = 1.0
    rope_high_freq_factor: float = 4.0
    rope_original_max_pos: int = 8192
    max_positions: int = 131072
    tie_embeddings: bool = True
    eos_token_id: int = 128001
    bos_token_id: int = 128000
    eos_token_ids: tuple = ()   # further stop ids (generation_config.json's list; set by the adapter loader)
    model_type: str = "llama"   # "llama" | "qwen2" | "qwen3": the transformers class a checkpoint of this shape loads into
    qkv_bias: bool = False      # q / k / v projections carry a bias (Qwen2; Llama's attention_bias)
    rope_type: str = "llama3"   # "llama3": the scaling above; "default": plain 1 / theta^(2i/d), the four rope_* fields unused
    qk_norm: bool = False       # Qwen3: every q and k head is RMS-normalised over head_dim (self_attn.q_norm / k_norm) before RoPE

    @staticmethod
    def llama32_3b() -> "LlamaShape":
        return LlamaShape()

    @staticmethod
    def tiny() -> "LlamaShape":
        """Small everywhere except the head dimension (128, as the 3B model)."""
        return LlamaShape(vocab=512, hidden=512, layers=3, heads=4, kv_heads=2, ffn=1024, eos_token_id=2, bos_token_id=1)

    @staticmethod
    def wide() -> "LlamaShape":
        """The real widths (hidden 3072, 24 / 8 heads, FFN 8192) with few layers and a small vocabulary: the kernels at the
        shapes Llama-3.2-3B runs them at, in a model whose weights regenerate from a seed in seconds."""
        return LlamaShape(vocab=4096, layers=3, eos_token_id=2, bos_token_id=1)

    @staticmethod
    def qwen2_tiny() -> "LlamaShape":
        """Qwen2.5-7B's differences from Llama in their smallest form: q / k / v biases, plain RoPE at theta 1e6, an untied head and a
        GQA group of 7 (7 query heads on 1 KV head).  896 and 1152 are multiples of 128 and 64 but not of 256."""
        return LlamaShape(vocab=512, hidden=896, layers=3, heads=7, kv_heads=1, ffn=1152, rms_eps=1e-6, rope_theta=1e6,
                          max_positions=32768, tie_embeddings=False, eos_token_id=2, bos_token_id=1, model_type="qwen2", qkv_bias=True,
                          rope_type="default")

    @staticmethod
    def llama32_1b() -> "LlamaShape":
        """Llama-3.2-1B's config.json: head dimension 64 (the attention kernels are built for 64 and 128), a KV group of 4."""
        return LlamaShape(hidden=2048, layers=16, heads=32, kv_heads=8, head_dim=64)

    @staticmethod
    def tiny64() -> "LlamaShape":
        """``tiny()`` at head dimension 64: 8 / 2 heads (a KV group of 4) over the same widths."""
        return LlamaShape(vocab=512, hidden=512, layers=3, heads=8, kv_heads=2, head_dim=64, ffn=1024, eos_token_id=2, bos_token_id=1)

    @staticmethod
    def wide64() -> "LlamaShape":
        """Llama-3.2-1B's widths (hidden 2048, 32 / 8 heads of 64, FFN 8192) with two layers and a small vocabulary, as ``wide()`` is to the 3B."""
        return LlamaShape(vocab=4096, hidden=2048, layers=2, heads=32, kv_heads=8, head_dim=64, eos_token_id=2, bos_token_id=1)

    @staticmethod
    def qwen2_tiny64() -> "LlamaShape":
        """``qwen2_tiny()`` with 14 / 2 heads of 64 (Qwen2.5-0.5B's geometry): the same widths, a KV group of 7 at head dimension 64."""
        return LlamaShape(vocab=512, hidden=896, layers=3, heads=14, kv_heads=2, head_dim=64, ffn=1152, rms_eps=1e-6, rope_theta=1e6,
                          max_positions=32768, tie_embeddings=False, eos_token_id=2, bos_token_id=1, model_type="qwen2", qkv_bias=True,
                          rope_type="default")

    @staticmethod
    def qwen3_tiny() -> "LlamaShape":
        """Qwen3's differences in their smallest form: the q / k norm, no bias, and 8 / 4 heads of 128 over hidden 640, so that
        hq = 1024 and hk = 512 both differ from hidden (Qwen3-0.6B: hidden 1024, hq 2048).  Tied head, as 0.6B to 4B."""
        return LlamaShape(vocab=512, hidden=640, layers=3, heads=8, kv_heads=4, head_dim=128, ffn=1152, rms_eps=1e-6, rope_theta=1e6,
                          max_positions=32768, tie_embeddings=True, eos_token_id=2, bos_token_id=1, model_type="qwen3", qkv_bias=False,
                          rope_type="default", qk_norm=True)

    @staticmethod
    def qwen3_tiny_untied() -> "LlamaShape":
        """``qwen3_tiny()`` with a head of its own, as Qwen3-8B and up."""
        from dataclasses import replace
        return replace(LlamaShape.qwen3_tiny(), tie_embeddings=False)

    def hf_config(self):
        """The transformers config of this shape: Qwen3Config, Qwen2Config or LlamaConfig (used only by the fixture scripts of tests/golden)."""
        if self.model_type == "qwen3":
            from transformers import Qwen3Config

            assert self.qk_norm and self.rope_type == "default", self
            return Qwen3Config(vocab_size=self.vocab, hidden_size=self.hidden, intermediate_size=self.ffn, num_hidden_layers=self.layers,
                               num_attention_heads=self.heads, num_key_value_heads=self.kv_heads, head_dim=self.head_dim,
                               max_position_embeddings=self.max_positions, rms_norm_eps=self.rms_eps, rope_theta=self.rope_theta,
                               rope_scaling=None, use_sliding_window=False, attention_bias=self.qkv_bias,
                               tie_word_embeddings=self.tie_embeddings, hidden_act="silu", attention_dropout=0.0,
                               eos_token_id=self.eos_token_id, bos_token_id=self.bos_token_id, pad_token_id=None)
        if self.model_type == "qwen2":
            from transformers import Qwen2Config

            assert self.qkv_bias and self.rope_type == "default" and self.hidden == self.heads * self.head_dim, self
            return Qwen2Config(vocab_size=self.vocab, hidden_size=self.hidden, intermediate_size=self.ffn, num_hidden_layers=self.layers,
                               num_attention_heads=self.heads, num_key_value_heads=self.kv_heads, max_position_embeddings=self.max_positions,
                               rms_norm_eps=self.rms_eps, rope_theta=self.rope_theta, rope_scaling=None, use_sliding_window=False,
                               tie_word_embeddings=self.tie_embeddings, hidden_act="silu", attention_dropout=0.0,
                               eos_token_id=self.eos_token_id, bos_token_id=self.bos_token_id, pad_token_id=None)
        from transformers import LlamaConfig

        kw = self.hf_kwargs()
        kw["attention_bias"] = self.qkv_bias
        if self.rope_type == "default":
            kw["rope_scaling"] = None
        return LlamaConfig(**kw)

    def hf_kwargs(self) -> dict:
        """transformers.LlamaConfig arguments (used only by tests/golden/make_llama_fixtures.py)."""
        return dict(vocab_size=self.vocab, hidden_size=self.hidden, intermediate_size=self.ffn, num_hidden_layers=self.layers,
                    num_attention_heads=self.heads, num_key_value_heads=self.kv_heads, head_dim=self.head_dim,
                    max_position_embeddings=self.max_positions, rms_norm_eps=self.rms_eps, rope_theta=self.rope_theta,
                    rope_scaling={"factor": self.rope_factor, "high_freq_factor": self.rope_high_freq_factor,
                                  "low_freq_factor": self.rope_low_freq_factor,
                                  "original_max_position_embeddings": self.rope_original_max_pos, "rope_type": "llama3"},
                    tie_word_embeddings=self.tie_embeddings, attention_bias=False, mlp_bias=False, hidden_act="silu",
                    eos_token_id=self.eos_token_id, bos_token_id=self.bos_token_id, pad_token_id=None)


@dataclass(frozen=True)
class BertShape:
    """A BERT-family sentence encoder (transformers' BertModel / RobertaModel / XLMRobertaModel without the pooler: post-LayerNorm
    blocks, learned absolute positions, exact-erf GELU, head dimension 64).  The defaults are m3e-base's config.json ("Moka": bert-base
    over the 21 128-entry Chinese vocabulary), whose 768-d sentence vector is the style bank's D = 768."""
    model_type: str = "bert"        # "bert" | "roberta" | "xlm-roberta"
    vocab: int = 21128
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    ffn: int = 3072
    max_positions: int = 512
    type_vocab: int = 2
    ln_eps: float = 1e-12
    pad_token_id: int = 0

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads

    @property
    def pos_offset(self) -> int:
        """The position of a row's first token: RoBERTa numbers the real tokens from pad_token_id + 1 (transformers'
        create_position_ids_from_input_ids; on right-padded rows exactly that), BERT from 0."""
        return self.pad_token_id + 1 if self.model_type in ("roberta", "xlm-roberta") else 0

    @property
    def max_tokens(self) -> int:
        return self.max_positions - self.pos_offset

    @staticmethod
    def m3e_base() -> "BertShape":
        return BertShape()

    @staticmethod
    def bert_tiny() -> "BertShape":
        """Two heads of 64, two layers, two token types; 160 positions hold the 130-token row that crosses the attention's 128-query tile."""
        return BertShape(vocab=512, hidden=128, layers=2, heads=2, ffn=512, max_positions=160)

    @staticmethod
    def xlmr_tiny() -> "BertShape":
        """``bert_tiny()`` as an XLM-R: one token type, pad_token_id 1, so positions start at 2 and 162 of them hold 160 tokens."""
        return BertShape(model_type="xlm-roberta", vocab=512, hidden=128, layers=2, heads=2, ffn=512, max_positions=162, type_vocab=1,
                         ln_eps=1e-5, pad_token_id=1)

    def hf_config(self):
        """The transformers config of this shape (used only by tests/golden/make_bert_fixtures.py)."""
        kw = dict(vocab_size=self.vocab, hidden_size=self.hidden, num_hidden_layers=self.layers, num_attention_heads=self.heads,
                  intermediate_size=self.ffn, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                  max_position_embeddings=self.max_positions, type_vocab_size=self.type_vocab, layer_norm_eps=self.ln_eps,
                  pad_token_id=self.pad_token_id)
        if self.model_type == "bert":
            from transformers import BertConfig
            return BertConfig(**kw)
        if self.model_type == "xlm-roberta":
            from transformers import XLMRobertaConfig
            return XLMRobertaConfig(**kw)
        from transformers import RobertaConfig
        return RobertaConfig(**kw)
