"""ctypes binding of libastts_train.so (the fine-tuning kernels declared in include/train/astts_train.h).  The signatures come from
that header through astts._lib.parse_prototypes, as the main library's do; there is no fallback when the library is missing."""
from __future__ import annotations

import ctypes
import functools
import os

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libastts_train.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "train", "astts_train.h"))
ABI_VERSION = 1


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    if not os.path.exists(HEADER_PATH):
        raise _lib.AsttsLibraryMissing(f"{HEADER_PATH} not found: the ctypes signatures of libastts_train.so are derived from this header")
    with open(HEADER_PATH) as f:
        return parse(f.read())


def parse(text: str) -> dict:
    sigs = _lib.parse_prototypes(text)
    stray = [n for n in sigs if not n.startswith("astts_train_")]
    if stray:
        raise ValueError(f"include/train/astts_train.h declares names outside astts_train_*: {stray}")
    return sigs


def declared_symbols():
    return sorted(signatures())


_loaded = None


def load():
    """Load libastts_train.so (once).  Raises AsttsLibraryMissing when it has not been built."""
    global _loaded
    if _loaded is not None:
        return _loaded
    if not os.path.exists(LIB_PATH):
        raise _lib.AsttsLibraryMissing(f"{LIB_PATH} not found: build it with `make -C autostyle-tts_amd/csrc` (it builds both libraries).  "
                                       "There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in signatures().items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.astts_train_abi_version() != ABI_VERSION:
        raise _lib.AsttsLibraryMissing(f"{LIB_PATH} has ABI {lib.astts_train_abi_version()}, this package needs {ABI_VERSION}: rebuild it")
    _loaded = lib
    return lib


def check(code: int) -> None:
    if code != _lib.OK:
        msg = load().astts_train_last_error_string()
        raise _lib.AsttsError(code, msg.decode("utf-8", "replace") if msg else "")
