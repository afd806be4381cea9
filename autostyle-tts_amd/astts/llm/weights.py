"""State dicts of the embedder LLM: seeded synthetic weights at a given shape (no Llama checkpoint exists offline) and the
loader for a real one.  Names follow transformers' LlamaForCausalLM so a real checkpoint loads through the same path."""
from __future__ import annotations

import glob
import os
from typing import Dict, Optional

import torch

from .config import BertShape, LlamaShape

StateDict = Dict[str, torch.Tensor]
BIAS_OUTLIERS = (3, 40, 77, 101, 126)    # the entries (mod the bias length) of every q / k bias that make_llama_weights sets to +-16
# Qwen3 q_norm / k_norm: (entry mod head_dim, value) that make_llama_weights sets in every norm weight.  Real ones have outliers both ways
QK_NORM_OUTLIERS = ((5, 8.0), (17, 0.02), (33, 0.0), (62, 8.0), (47, 0.02))


def make_llama_weights(cfg: LlamaShape, seed: int = 0, device=None) -> StateDict:
    """Deterministic (torch.Generator, CPU) fp32 weights: projections N(0, 0.02^2 * 4) so that activations stay O(1)
    through a few layers, norm scales 1 + 0.1 N(0,1).  The fixture generator, the oracle tests and the GPU tests all
    call this -- the weights never travel, only the seed does.  ``device``: draw on that device instead (its own generator, so
    OTHER values than the CPU stream's: for throughput runs of the full 3.2 B-parameter model, where no fixture is compared)."""
    g = torch.Generator(device=device).manual_seed(seed) if device is not None else torch.Generator().manual_seed(seed)
    r = lambda *s, std: torch.randn(*s, generator=g, device=device) * std
    sd: StateDict = {"model.embed_tokens.weight": r(cfg.vocab, cfg.hidden, std=0.5)}
    kv = cfg.kv_heads * cfg.head_dim
    q = cfg.heads * cfg.head_dim
    for i in range(cfg.layers):
        p = f"model.layers.{i}."
        sd[p + "self_attn.q_proj.weight"] = r(q, cfg.hidden, std=0.04)
        sd[p + "self_attn.k_proj.weight"] = r(kv, cfg.hidden, std=0.04)
        sd[p + "self_attn.v_proj.weight"] = r(kv, cfg.hidden, std=0.04)
        sd[p + "self_attn.o_proj.weight"] = r(cfg.hidden, q, std=0.02)
        sd[p + "mlp.gate_proj.weight"] = r(cfg.ffn, cfg.hidden, std=0.04)
        sd[p + "mlp.up_proj.weight"] = r(cfg.ffn, cfg.hidden, std=0.04)
        sd[p + "mlp.down_proj.weight"] = r(cfg.hidden, cfg.ffn, std=0.02)
        sd[p + "input_layernorm.weight"] = 1.0 + r(cfg.hidden, std=0.1)
        sd[p + "post_attention_layernorm.weight"] = 1.0 + r(cfg.hidden, std=0.1)
    sd["model.norm.weight"] = 1.0 + r(cfg.hidden, std=0.1)
    if not cfg.tie_embeddings:
        sd["lm_head.weight"] = r(cfg.vocab, cfg.hidden, std=0.05)
    if cfg.qkv_bias:
        # drawn after everything else, so a shape without biases consumes the generator exactly as before.  Real Qwen2.5 q / k biases
        # have large outliers: std 0.5 and a fixed handful of entries at +-16, values that matter after the fp16 store of q | k | v
        for i in range(cfg.layers):
            p = f"model.layers.{i}."
            for nm, n, std in (("q", q, 0.5), ("k", kv, 0.5), ("v", kv, 0.05)):
                b = r(n, std=std)
                if nm != "v":
                    for j, at in enumerate(BIAS_OUTLIERS):
                        b[at % n] = 16.0 if (i + j) % 2 == 0 else -16.0
                sd[p + f"self_attn.{nm}_proj.bias"] = b
    if cfg.qk_norm:
        # drawn after everything else, as the biases are: every shape without the norm consumes the generator exactly as before
        for i in range(cfg.layers):
            for nm in ("q_norm", "k_norm"):
                w = 1.0 + r(cfg.head_dim, std=0.1)
                for at, val in QK_NORM_OUTLIERS:
                    w[at % cfg.head_dim] = val
                sd[f"model.layers.{i}.self_attn.{nm}.weight"] = w
    return sd


def load_llama_weights(model_dir: str) -> StateDict:
    """A transformers checkpoint directory (``*.safetensors`` shards or ``pytorch_model*.bin``), e.g. the fine-tuned
    Llama-3.2-3B the reference points at (src/search_milvus.py:251).  PEFT adapters must be merged beforehand."""
    sd: StateDict = {}
    shards = sorted(glob.glob(os.path.join(model_dir, "*.safetensors")))
    if shards:
        from safetensors.torch import load_file

        for s in shards:
            sd.update(load_file(s, device="cpu"))
    else:
        bins = sorted(glob.glob(os.path.join(model_dir, "pytorch_model*.bin")))
        if not bins:
            raise FileNotFoundError(f"no *.safetensors / pytorch_model*.bin under {model_dir!r}")
        for b in bins:
            sd.update(torch.load(b, map_location="cpu", weights_only=True))
    return {k: v.float() for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------- BERT-family sentence encoders
# names follow transformers' BertModel / XLMRobertaModel (no prefix); a checkpoint saved from a *ForMaskedLM / *ForPreTraining class
# carries them behind "bert." / "roberta."
BERT_PREFIXES = ("bert.", "roberta.")
BERT_IGNORED = ("pooler.", "cls.", "lm_head.")                    # heads the sentence vector does not pass through
BERT_IGNORED_KEYS = ("embeddings.position_ids", "embeddings.token_type_ids")      # buffers older transformers versions saved


def bert_weight_shapes(shape: BertShape) -> Dict[str, tuple]:
    """Every tensor a BertShape needs, by its transformers name."""
    h, f = shape.hidden, shape.ffn
    out = {"embeddings.word_embeddings.weight": (shape.vocab, h), "embeddings.position_embeddings.weight": (shape.max_positions, h),
           "embeddings.token_type_embeddings.weight": (shape.type_vocab, h), "embeddings.LayerNorm.weight": (h,), "embeddings.LayerNorm.bias": (h,)}
    for i in range(shape.layers):
        p = f"encoder.layer.{i}."
        for nm in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            out[p + nm + ".weight"], out[p + nm + ".bias"] = (h, h), (h,)
        out[p + "intermediate.dense.weight"], out[p + "intermediate.dense.bias"] = (f, h), (f,)
        out[p + "output.dense.weight"], out[p + "output.dense.bias"] = (h, f), (h,)
        for nm in ("attention.output.LayerNorm", "output.LayerNorm"):
            out[p + nm + ".weight"], out[p + nm + ".bias"] = (h,), (h,)
    return out


def make_bert_weights(shape: BertShape, seed: int = 0) -> StateDict:
    """Deterministic (torch.Generator, CPU) fp32 weights of a BertShape, in the order of ``bert_weight_shapes``: tables N(0, 0.5^2) /
    N(0, 0.2^2) for positions and types, projections N(0, 0.04^2) into the attention and the FFN and N(0, 0.02^2) out of them, biases
    N(0, 0.1^2), LayerNorm 1 + 0.1 N / 0.1 N.  As for the Llama shapes only the seed travels."""
    g = torch.Generator().manual_seed(seed)
    sd: StateDict = {}
    for k, s in bert_weight_shapes(shape).items():
        if k.endswith("LayerNorm.weight"):
            sd[k] = 1.0 + torch.randn(*s, generator=g) * 0.1
        elif k.endswith(".bias"):
            sd[k] = torch.randn(*s, generator=g) * 0.1
        elif k.startswith("embeddings."):
            sd[k] = torch.randn(*s, generator=g) * (0.5 if "word" in k else 0.2)
        else:
            sd[k] = torch.randn(*s, generator=g) * (0.02 if k.endswith("output.dense.weight") else 0.04)
    return sd


def map_bert_keys(sd: StateDict, shape: BertShape) -> StateDict:
    """A checkpoint's tensors under the unprefixed names: a "bert." / "roberta." prefix is dropped, the pooler, the pre-training heads
    and the saved position_ids / token_type_ids buffers are ignored; any other unknown tensor, a missing one or a wrong shape is an error."""
    want = bert_weight_shapes(shape)
    out: StateDict = {}
    unknown = []
    for k, v in sd.items():
        if k.startswith(BERT_IGNORED):
            continue
        name = next((k[len(p):] for p in BERT_PREFIXES if k.startswith(p)), k)
        if name.startswith(BERT_IGNORED) or name in BERT_IGNORED_KEYS:
            continue
        if name not in want:
            unknown.append(k)
        else:
            out[name] = v.float()
    if unknown:
        raise ValueError(f"the checkpoint has tensors this {shape.model_type} encoder does not apply: {sorted(unknown)[:3]}")
    missing = sorted(set(want) - set(out))
    if missing:
        raise ValueError(f"the checkpoint lacks tensors of this {shape.model_type} encoder: {missing[:3]}")
    bad = [(k, tuple(out[k].shape), want[k]) for k in want if tuple(out[k].shape) != want[k]]
    if bad:
        raise ValueError(f"tensor shapes do not fit config.json: {bad[:3]}")
    return out


def load_bert_weights(model_dir: str, shape: Optional[BertShape] = None) -> StateDict:
    """A BERT / RoBERTa / XLM-R checkpoint directory (safetensors shards or pytorch_model*.bin) -> the tensors of its shape
    (``shape``, else the directory's config.json) under the unprefixed names (``map_bert_keys``)."""
    if shape is None:
        from .bert_dir import bert_shape_from_config
        shape = bert_shape_from_config(model_dir)
    return map_bert_keys(load_llama_weights(model_dir), shape)
