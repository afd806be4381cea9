"""ctypes binding of the grouped / ranged style-bank search of libastts.so (include/knn/astts_knn_grouped.h).

The calls live in libastts.so itself; their signatures are parsed from their own header and set on the library object
astts/_lib.py loads (astts._lib.bind_headers).
"""
from __future__ import annotations

import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "knn",
                                            "astts_knn_grouped.h"))
DEFAULT_ROUNDS = 64      # ASTTS_KNN_GROUPED_DEFAULT_ROUNDS

signatures, load = _lib.bind_headers(HEADER_PATH, what="the grouped search")
