"""ctypes binding of the Qwen3 q / k norm + RoPE operator of libastts.so (include/llm/astts_qknorm.h).

The call lives in libastts.so itself; its signature is parsed from its own header and set on the library object astts/_lib.py
loads (astts._lib.bind_headers).
"""
from __future__ import annotations

import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "llm", "astts_qknorm.h"))

signatures, load = _lib.bind_headers(HEADER_PATH, what="the q / k norm + RoPE operator")
