"""What a BERT-family sentence-encoder directory says about itself: the shape (config.json) and, for a sentence-transformers directory,
how the token states become the sentence vector (modules.json, 1_Pooling/config.json, sentence_bert_config.json).

Anything that would load and compute another model is refused by key with a ConfigError, as astts.llm.peft.shape_from_config does for
the decoders.  Prompts (config_sentence_transformers.json: "query: " / "passage: " of e5, the bge instruction) are NOT applied: texts
are embedded as given, and a caller that wants a prefix puts it into the text."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass

from .config import BertShape
from .peft import ConfigError

BERT_MODEL_TYPES = ("bert", "roberta", "xlm-roberta")
# encoder families that are NOT built: a directory of one of them is an encoder all the same, and is refused as one (by model_type)
OTHER_ENCODER_TYPES = ("albert", "distilbert", "mpnet", "nomic_bert", "electra", "deberta", "deberta-v2", "roformer", "mobilebert",
                       "camembert", "xlm", "xlm-roberta-xl", "modernbert", "new", "t5", "mt5")


def is_bert_dir(path: str) -> bool:
    """A directory whose config.json names one of the BERT-family model types."""
    p = os.path.join(path or "", "config.json")
    if not os.path.isfile(p):
        return False
    with open(p) as f:
        return str(json.load(f).get("model_type", "")) in BERT_MODEL_TYPES


def is_encoder_dir(path: str) -> bool:
    """A directory whose config.json names a BERT-family model type or another encoder family: load_embedder sends both to
    ``bert_shape_from_config``, which builds the first and refuses the second by key, instead of reading them as a Llama."""
    p = os.path.join(path or "", "config.json")
    if not os.path.isfile(p):
        return False
    with open(p) as f:
        return str(json.load(f).get("model_type", "")) in BERT_MODEL_TYPES + OTHER_ENCODER_TYPES


def bert_shape_from_config(model_dir: str) -> BertShape:
    """BertShape from a transformers config.json of model_type bert, roberta or xlm-roberta."""
    with open(os.path.join(model_dir, "config.json")) as f:
        c = json.load(f)
    model_type = str(c.get("model_type", ""))
    if model_type not in BERT_MODEL_TYPES:
        raise ConfigError(f"config.json model_type={model_type!r}: the encoder runs {', '.join(BERT_MODEL_TYPES)} checkpoints only "
                          "(albert, distilbert, mpnet, nomic_bert and the rest are other layer stacks)")
    if c.get("is_decoder"):
        raise ConfigError("config.json is_decoder=true: a causal BERT is not built")
    if c.get("add_cross_attention"):
        raise ConfigError("config.json add_cross_attention=true: cross-attention layers are not built")
    act = c.get("hidden_act", "gelu")
    if act != "gelu":
        raise ConfigError(f"config.json hidden_act={act!r}: only 'gelu' (the exact erf form) is built")
    pet = c.get("position_embedding_type") or "absolute"
    if pet != "absolute":
        raise ConfigError(f"config.json position_embedding_type={pet!r}: only 'absolute' (learned) positions are built")
    hidden, heads = int(c["hidden_size"]), int(c["num_attention_heads"])
    if heads < 1 or hidden % heads or hidden // heads != 64:
        raise ConfigError(f"config.json hidden_size={hidden} / num_attention_heads={heads}: the attention kernel is built for a head "
                          "dimension of 64 (bert-base / -large, m3e, bge-base / -large, multilingual-e5; not MiniLM or bge-small)")
    d = BertShape()
    pad = c.get("pad_token_id")
    shape = BertShape(model_type=model_type, vocab=int(c["vocab_size"]), hidden=hidden, layers=int(c["num_hidden_layers"]), heads=heads,
                      ffn=int(c["intermediate_size"]), max_positions=int(c["max_position_embeddings"]),
                      type_vocab=int(c.get("type_vocab_size", d.type_vocab)), ln_eps=float(c.get("layer_norm_eps", d.ln_eps)),
                      pad_token_id=int(pad) if pad is not None else (1 if model_type != "bert" else 0))
    if shape.max_tokens < 2:
        raise ConfigError(f"config.json max_position_embeddings={shape.max_positions} with pad_token_id={shape.pad_token_id}: no room for [CLS][SEP]")
    return shape


@dataclass(frozen=True)
class SentenceSetup:
    pooling: str = "mean"             # "mean" over the real tokens | "cls": the first token's state
    normalize: bool = False           # an L2 Normalize module follows the pooling
    max_seq_length: int = 512


def _read_json(path: str) -> dict:
    with open(path) as f:
        return json.load(f)


def sentence_setup(model_dir: str, shape: BertShape) -> SentenceSetup:
    """A sentence-transformers directory (modules.json): pooling mode from the Pooling module's config.json (mean or cls; every other
    mode and a Dense module are refused by name), whether a Normalize module follows, max_seq_length from sentence_bert_config.json.
    A plain transformers directory: mean pooling, no normalisation, max_seq_length = min(512, the positions the table has)."""
    limit = shape.max_tokens
    mj = os.path.join(model_dir, "modules.json")
    if not os.path.isfile(mj):
        return SentenceSetup("mean", False, min(512, limit))
    pooling, normalize = None, False
    for m in _read_json(mj):
        kind = str(m.get("type", "")).rsplit(".", 1)[-1]
        if kind == "Transformer":
            continue
        if kind == "Pooling":
            pc = _read_json(os.path.join(model_dir, m.get("path", "1_Pooling"), "config.json"))
            on = sorted(k for k, v in pc.items() if k.startswith("pooling_mode_") and v is True)
            other = [k for k in on if k not in ("pooling_mode_mean_tokens", "pooling_mode_cls_token")]
            if other:
                raise ConfigError(f"{m.get('path', '1_Pooling')}/config.json {other[0]}=true: only mean and cls pooling are built")
            if len(on) != 1:
                raise ConfigError(f"{m.get('path', '1_Pooling')}/config.json enables {on or 'no pooling mode'}: exactly one of "
                                  "pooling_mode_mean_tokens / pooling_mode_cls_token is built (no concatenated poolings)")
            if pc.get("include_prompt") is False:
                raise ConfigError(f"{m.get('path', '1_Pooling')}/config.json include_prompt=false: prompts are not applied, so none can be left out")
            pooling = "mean" if on[0] == "pooling_mode_mean_tokens" else "cls"
        elif kind == "Normalize":
            if pooling is None:
                raise ConfigError("modules.json: Normalize comes before the Pooling module")
            normalize = True
        else:
            raise ConfigError(f"modules.json module {m.get('type')!r} ({m.get('path', '')}): only Transformer, Pooling and Normalize are built "
                              "(no Dense head)")
    if pooling is None:
        raise ConfigError("modules.json has no Pooling module")
    sb = os.path.join(model_dir, "sentence_bert_config.json")
    n = int(_read_json(sb).get("max_seq_length") or 512) if os.path.isfile(sb) else 512
    return SentenceSetup(pooling, normalize, max(2, min(n, limit)))
