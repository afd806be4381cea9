"""ctypes binding of the two row operators of the BERT-family encoder in libastts.so (include/llm/astts_bert.h): LayerNorm with an
fp32 and an fp16 copy of its result, and the same behind the word + position + type embedding sum.

The calls live in libastts.so itself; their signatures are parsed from their own header and set on the library object astts/_lib.py
loads (astts._lib.bind_headers).
"""
from __future__ import annotations

import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "llm", "astts_bert.h"))

signatures, load = _lib.bind_headers(HEADER_PATH, what="the BERT encoder's LayerNorm and embedding operators")
