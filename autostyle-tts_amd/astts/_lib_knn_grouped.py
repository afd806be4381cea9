"""ctypes binding of the grouped / ranged style-bank search of libastts.so (include/knn/astts_knn_grouped.h).

The calls live in libastts.so itself; their signatures are parsed from their own header exactly as astts/_lib_knn.py parses
include/knn/astts_knn_mutable.h, and set on the library object astts/_lib.py loads.
"""
from __future__ import annotations

import functools
import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "knn",
                                            "astts_knn_grouped.h"))
DEFAULT_ROUNDS = 64      # ASTTS_KNN_GROUPED_DEFAULT_ROUNDS


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    if not os.path.exists(HEADER_PATH):
        raise _lib.AsttsLibraryMissing(f"{HEADER_PATH} not found: the ctypes signatures of the grouped search are derived from this header")
    with open(HEADER_PATH) as f:
        return _lib.parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def load():
    """libastts.so with the prototypes of the grouped search set (once)."""
    lib = _lib.load()
    for name, (res, args) in signatures().items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
