"""ctypes binding of the mutable style-bank entry points of libastts.so (include/knn/astts_knn_mutable.h).

The calls live in libastts.so itself; their signatures are parsed from their own header exactly as astts/_lib.py parses
include/astts.h, and set on the library object that module loads (astts._lib.bind_headers).
"""
from __future__ import annotations

import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "knn",
                                            "astts_knn_mutable.h"))

signatures, load = _lib.bind_headers(HEADER_PATH, what="the style-bank mutations")
