"""ctypes binding of the IVF_FLAT index of libastts.so (include/knn/astts_knn_ivf.h).

The calls live in libastts.so itself; their signatures are parsed from their own header exactly as astts/_lib_knn_grouped.py parses
include/knn/astts_knn_grouped.h, and set on the library object astts/_lib.py loads.
"""
from __future__ import annotations

import functools
import os

from . import _lib

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "knn",
                                            "astts_knn_ivf.h"))
DEFAULT_NITER = 20       # ASTTS_KNN_IVF_DEFAULT_NITER
DEFAULT_NPROBE = 8       # what a search without an nprobe probes (the host's default; the C call takes nprobe explicitly)
SLICE_ROWS = 64          # ASTTS_KNN_IVF_SLICE_ROWS
MAX_NLIST = 65535        # ASTTS_KNN_IVF_MAX_NLIST


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    if not os.path.exists(HEADER_PATH):
        raise _lib.AsttsLibraryMissing(f"{HEADER_PATH} not found: the ctypes signatures of the IVF index are derived from this header")
    with open(HEADER_PATH) as f:
        return _lib.parse_prototypes(f.read())


@functools.lru_cache(maxsize=None)
def load():
    """libastts.so with the prototypes of the IVF index set (once)."""
    lib = _lib.load()
    for name, (res, args) in signatures().items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
