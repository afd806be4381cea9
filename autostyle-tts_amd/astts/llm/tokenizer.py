"""The tokenizer side of the query embedder.  The tokenizer is the checkpoint's own (tokenizer.json: not available offline); anything
with ``encode(text) -> list[int]`` plugs in (`transformers.AutoTokenizer` when the checkpoint directory is given)."""
import inspect
import zlib
from typing import List, Sequence

from .config import LlamaShape


class HashTokenizer:
    """STAND-IN (the Llama tokenizer files do not exist offline), so that the CLIs run end to end without one: bos + one id per
    whitespace-separated word by a fixed hash.  Deterministic, reversible in nothing; good for plumbing and benchmarks only."""

    def __init__(self, cfg: LlamaShape):
        self.cfg = cfg

    def encode(self, text: str, add_special_tokens: bool = True) -> List[int]:
        return ([self.cfg.bos_token_id] if add_special_tokens else []) + [3 + zlib.crc32(w.encode("utf-8")) % (self.cfg.vocab - 3)
                                                                          for w in text.split()]

    def decode(self, ids: Sequence[int]) -> str:
        return " ".join(f"<{int(i)}>" for i in ids)


_TAKES = {}         # (tokenizer class, method, keyword) -> bool: decided once per tokenizer


def _takes(tok, method: str, keyword: str) -> bool:
    """Whether ``tok.method`` accepts ``keyword``, from its signature and never from a call: a TypeError raised INSIDE a real
    tokenizer must not be mistaken for "this stand-in has no such argument".  A signature that cannot be read counts as yes."""
    key = (type(tok), method, keyword)
    if key not in _TAKES:
        try:
            ps = inspect.signature(getattr(tok, method)).parameters
            _TAKES[key] = keyword in ps or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in ps.values())
        except (TypeError, ValueError):
            _TAKES[key] = True
    return _TAKES[key]


def encode_continuation(tok, text: str) -> List[int]:
    """Token ids of a CONTINUATION given as text.  ``encode(text)`` puts whatever special tokens the model expects in front; a
    continuation carries none of its own, so it needs ``encode(text, add_special_tokens=False)`` (transformers' signature;
    HashTokenizer has it).  A tokenizer without that keyword cannot say what it adds: pass the continuation as token ids then."""
    if not _takes(tok, "encode", "add_special_tokens"):
        raise TypeError("score / classify: this tokenizer's encode() has no add_special_tokens keyword, so a continuation given as "
                        "text cannot be tokenised without its special tokens; pass token ids")
    return [int(i) for i in tok.encode(text, add_special_tokens=False)]


def decode_clean(tok, ids: Sequence[int]) -> str:
    """``decode(ids, skip_special_tokens=True)`` (milvus/search_json.py:148,191) where the tokenizer has that argument: a stand-in may not."""
    return tok.decode(ids, skip_special_tokens=True) if _takes(tok, "decode", "skip_special_tokens") else tok.decode(ids)
