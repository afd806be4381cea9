"""ctypes binding of the Qwen3 q / k norm + RoPE operator of libastts.so (include/llm/astts_qknorm.h).

The call lives in libastts.so itself; its signature is parsed from its own header exactly as astts/_lib_knn_grouped.py parses
include/knn/astts_knn_grouped.h, and set on the library object astts/_lib.py loads.
"""
from __future__ import annotations

import functools
import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "llm", "astts_qknorm.h"))


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    if not os.path.exists(HEADER_PATH):
        raise _lib.AsttsLibraryMissing(f"{HEADER_PATH} not found: the ctypes signature of astts_op_qknorm_rope is derived from this header")
    with open(HEADER_PATH) as f:
        return _lib.parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def load():
    """libastts.so with the prototype of the fused norm set (once)."""
    lib = _lib.load()
    for name, (res, args) in signatures().items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
