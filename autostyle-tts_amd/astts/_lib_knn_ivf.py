"""ctypes binding of the IVF_FLAT index of libastts.so (include/knn/astts_knn_ivf.h).

The calls live in libastts.so itself; their signatures are parsed from their own header and set on the library object
astts/_lib.py loads (astts._lib.bind_headers).
"""
from __future__ import annotations

import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "knn",
                                            "astts_knn_ivf.h"))
DEFAULT_NITER = 20       # ASTTS_KNN_IVF_DEFAULT_NITER
DEFAULT_NPROBE = 8       # what a search without an nprobe probes (the host's default; the C call takes nprobe explicitly)
SLICE_ROWS = 64          # ASTTS_KNN_IVF_SLICE_ROWS
MAX_NLIST = 65535        # ASTTS_KNN_IVF_MAX_NLIST

signatures, load = _lib.bind_headers(HEADER_PATH, what="the IVF index")
