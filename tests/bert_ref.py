"""Restatement of the BERT-family encoder (transformers' BertModel / XLMRobertaModel with add_pooling_layer=False: post-LayerNorm blocks,
learned absolute positions, exact-erf GELU) and of its sentence vectors in plain torch (DESIGN.md section 2 "BERT-family encoders").
Uses only torch, so the GPU tests call it live.

``layernorm_dual`` and ``embed_ln`` are what astts_op_layernorm_dual / astts_op_bert_embed_ln compute (include/llm/astts_bert.h), in
whatever dtype they are given.  ``hidden`` runs a right-padded batch through the layer stack.

``h16=True`` rounds where the GPU path holds fp16: the GEMM operands (every LayerNorm output where it feeds a GEMM, every weight), q | k | v
after their GEMM, inside the attention q * (1/8) * log2 e and P (the MFMA operands of astts_op_attn_mha), the attention output and the
GELU output.  The residual stream, the biases and every LayerNorm stay fp32.  The fp32 run reproduces tests/golden/bert_tiny.npz
(tests/test_bert_cpu.py); the error of the fp16-rounded run against that fixture is what the GPU bounds are made of
(tests/golden/make_bert_fixtures.py prints it).

Three deliberately WRONG restatements show what the fixture tells apart: ``pos_shift=1`` (positions one too far), ``drop_types=True``
(the token-type table left out) and ``tanh_gelu=True``."""
from __future__ import annotations

import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from astts.llm.config import BertShape  # noqa: E402

SEED, BATCH_SEED, LENS = 47, 53, (130, 64, 5, 2)        # 130 crosses the attention's 128-query tile; 2 is [CLS][SEP]
SHAPES = ("bert_tiny", "xlmr_tiny", "m3e_base")
TINY = ("bert_tiny", "xlmr_tiny")                       # hidden states recorded; m3e_base: the embeddings only
POOLED = ("mean", "cls", "mean_norm", "cls_norm")
LOG2E = 1.4426950408889634


def rel_l2(x, ref) -> float:
    x, ref = torch.as_tensor(x).double(), torch.as_tensor(ref).double()
    return float((x - ref).norm() / ref.norm().clamp_min(1e-300))


def _rnd(x: torch.Tensor, h16: bool) -> torch.Tensor:
    return x.half().to(x.dtype) if h16 else x


def make_batch(shape: BertShape, lens=LENS, seed: int = BATCH_SEED):
    """Right-padded rows of random tokens from [3, vocab) (never the pad id), the padding filled with pad_token_id; token types: the
    second half of every row is type 1 where the shape has two types.  -> ids, lens, type_ids (int64)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), max(lens)), shape.pad_token_id, dtype=torch.int64)
    types = torch.zeros_like(ids)
    for i, n in enumerate(lens):
        ids[i, :n] = torch.randint(3, shape.vocab, (n,), generator=g)
        if shape.type_vocab > 1:
            types[i, n // 2:n] = 1
    ids[0, 1], ids[0, 2] = 0, shape.vocab - 1          # the word table's ends (0 is not XLM-R's pad id, and BERT's positions do not look at it)
    return ids, torch.tensor(lens, dtype=torch.int64), types


def layernorm_dual(x, gamma, beta, eps):
    """-> (y, y rounded once to fp16): mean, then the variance of the centred values."""
    d = x - x.mean(-1, keepdim=True)
    y = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps) * gamma + beta
    return y, y.half()


def embed_ln(word, pos, typ, ids, type_ids, lens, gamma, beta, pos_offset: int, eps: float):
    """LayerNorm(word[id] + pos[pos_offset + j] + typ[type_id]) on the real tokens, zeros behind them -> [B, T, c]."""
    b, t = ids.shape
    x = word[ids] + pos[pos_offset + torch.arange(t)][None] + (typ[type_ids] if type_ids is not None else typ[0])
    y = layernorm_dual(x, gamma, beta, eps)[0]
    return y * (torch.arange(t)[None, :] < torch.as_tensor(lens)[:, None]).to(y.dtype)[..., None]


def attention(q, k, v, lens, h16: bool = False):
    """q / k / v [B, T, heads, 64] -> [B, T, heads * 64]: bidirectional, keys at or beyond lens masked, scale 1/8."""
    b, t, heads, d = q.shape
    mask = torch.arange(t)[None, None, None, :] < torch.as_tensor(lens)[:, None, None, None]
    q = _rnd(q * (LOG2E / math.sqrt(d)), True) / LOG2E if h16 else q / math.sqrt(d)
    s = torch.einsum("bihd,bjhd->bhij", q, k).masked_fill(~mask, float("-inf"))
    return torch.einsum("bhij,bjhd->bihd", _rnd(torch.softmax(s, -1), h16), v).reshape(b, t, heads * d)


def hidden(sd, shape: BertShape, ids, lens, type_ids=None, h16: bool = False, pos_shift: int = 0, drop_types: bool = False,
           tanh_gelu: bool = False) -> torch.Tensor:
    """ids [B, T] right-padded, lens [B], type_ids [B, T] or None -> the last layer's hidden states fp32 [B, T, hidden]
    (== last_hidden_state on the real positions; padding rows hold finite values that nothing reads)."""
    b, t = ids.shape
    W = (lambda k: sd[k].half().float()) if h16 else (lambda k: sd[k])
    lin = lambda x, name: x @ W(name + ".weight").t() + sd[name + ".bias"]
    e = "embeddings."
    typ = sd[e + "token_type_embeddings.weight"]
    x = embed_ln(sd[e + "word_embeddings.weight"], sd[e + "position_embeddings.weight"], torch.zeros_like(typ) if drop_types else typ, ids,
                 type_ids, lens, sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], shape.pos_offset + pos_shift, shape.ln_eps)
    for i in range(shape.layers):
        p = f"encoder.layer.{i}."
        x16 = _rnd(x, h16)
        q, k, v = (_rnd(lin(x16, p + "attention.self." + nm), h16).view(b, t, shape.heads, 64) for nm in ("query", "key", "value"))
        a = _rnd(attention(q, k, v, lens, h16), h16)
        x = layernorm_dual(lin(a, p + "attention.output.dense") + x, sd[p + "attention.output.LayerNorm.weight"],
                           sd[p + "attention.output.LayerNorm.bias"], shape.ln_eps)[0]
        f = _rnd(F.gelu(lin(_rnd(x, h16), p + "intermediate.dense"), approximate="tanh" if tanh_gelu else "none"), h16)
        x = layernorm_dual(lin(f, p + "output.dense") + x, sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"], shape.ln_eps)[0]
    return x


def pooled(h: torch.Tensor, lens) -> dict:
    """The four sentence vectors of every row: mean over the real tokens and the first token's state, raw and L2-normalised."""
    mean = torch.stack([h[i, :int(n)].mean(0) for i, n in enumerate(lens)])
    return {"mean": mean, "cls": h[:, 0], "mean_norm": F.normalize(mean, dim=-1), "cls_norm": F.normalize(h[:, 0], dim=-1)}


def outputs(sd, shape, ids, lens, type_ids, **kw) -> dict:
    """What the fixture records of one forward pass: the hidden states of the real positions (rows concatenated) and the pooled vectors."""
    with torch.no_grad():
        h = hidden(sd, shape, ids, lens, type_ids, **kw)
        return {"hidden": torch.cat([h[i, :int(n)] for i, n in enumerate(lens)]), **pooled(h, lens)}


# ---------------------------------------------------------------------------------------------- checkpoint directories written by tests
def config_json(shape: BertShape) -> dict:
    arch = {"bert": "BertModel", "roberta": "RobertaModel", "xlm-roberta": "XLMRobertaModel"}[shape.model_type]
    return {"architectures": [arch], "model_type": shape.model_type, "vocab_size": shape.vocab, "hidden_size": shape.hidden,
            "num_hidden_layers": shape.layers, "num_attention_heads": shape.heads, "intermediate_size": shape.ffn, "hidden_act": "gelu",
            "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.1, "max_position_embeddings": shape.max_positions,
            "type_vocab_size": shape.type_vocab, "layer_norm_eps": shape.ln_eps, "pad_token_id": shape.pad_token_id,
            "position_embedding_type": "absolute", "initializer_range": 0.02, "torch_dtype": "float32"}


VOCAB_HEAD = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "<", ">"] + [str(i) for i in range(10)] + [f"##{i}" for i in range(10)]


def write_vocab(path: str, n: int) -> str:
    """A BERT vocab.txt of n entries: the special tokens, "<", ">" and the digit pieces (the stand-in LLM tokenizer decodes to "<123> <45>",
    which then splits into pieces of its own instead of [UNK]), then w27, w28, ... (the word w<i> has id i)."""
    with open(os.path.join(path, "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB_HEAD + [f"w{i}" for i in range(len(VOCAB_HEAD), n)]) + "\n")
    return path


def write_dir(path: str, shape: BertShape, sd: dict, prefix: str = "", config=None, sentence=None, extra=None) -> str:
    """A checkpoint directory: config.json, model.safetensors (fp32; keys behind ``prefix``; ``extra`` tensors added as they are),
    a vocab.txt, and with ``sentence`` = (pooling key, normalize, max_seq_length) the sentence-transformers files."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(config if config is not None else config_json(shape), f)
    save_file({**{prefix + k: v.contiguous() for k, v in sd.items()}, **(extra or {})}, os.path.join(path, "model.safetensors"))
    write_vocab(path, shape.vocab)
    if sentence is not None:
        write_sentence_files(path, *sentence)
    return path


def write_sentence_files(path: str, mode: str, normalize: bool, max_seq_length: int, dense: bool = False) -> None:
    """modules.json, 1_Pooling/config.json, sentence_bert_config.json as sentence-transformers saves them; ``mode``: the
    pooling_mode_* key that is true."""
    mods = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if dense:
        mods.append({"idx": len(mods), "name": str(len(mods)), "path": "2_Dense", "type": "sentence_transformers.models.Dense"})
    if normalize:
        mods.append({"idx": len(mods), "name": str(len(mods)), "path": f"{len(mods)}_Normalize", "type": "sentence_transformers.models.Normalize"})
    with open(os.path.join(path, "modules.json"), "w") as f:
        json.dump(mods, f)
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    keys = ("pooling_mode_cls_token", "pooling_mode_mean_tokens", "pooling_mode_max_tokens", "pooling_mode_mean_sqrt_len_tokens",
            "pooling_mode_weightedmean_tokens", "pooling_mode_lasttoken")
    with open(os.path.join(path, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": 768, **{k: k == mode for k in keys}, "include_prompt": True}, f)
    with open(os.path.join(path, "sentence_bert_config.json"), "w") as f:
        json.dump({"max_seq_length": max_seq_length, "do_lower_case": False}, f)
