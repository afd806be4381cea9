"""ctypes binding of the session entry points of libastts.so (include/session/astts_lm_session.h: decode sessions,
include/session/astts_flow_session.h: flow sessions, include/session/astts_flow_share.h: the launches a joined flow pass shares).

The session calls live in libastts.so itself; their signatures are parsed from their own headers exactly as astts/_lib.py parses
include/astts.h, and set on the library object that module loads.
"""
from __future__ import annotations

import functools
import os

from . import _lib

_DIR = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "session"))
HEADER_PATH = os.path.join(_DIR, "astts_lm_session.h")
FLOW_HEADER_PATH = os.path.join(_DIR, "astts_flow_session.h")
FLOW_SHARE_HEADER_PATH = os.path.join(_DIR, "astts_flow_share.h")


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    sigs = {}
    for path in (HEADER_PATH, FLOW_HEADER_PATH, FLOW_SHARE_HEADER_PATH):
        if not os.path.exists(path):
            raise _lib.AsttsLibraryMissing(f"{path} not found: the ctypes signatures of the session calls are derived from this header")
        with open(path) as f:
            sigs.update(_lib.parse_prototypes(f.read()))
    return sigs


@functools.lru_cache(maxsize=None)
def load():
    """libastts.so with the session prototypes set (once)."""
    lib = _lib.load()
    for name, (res, args) in signatures().items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
