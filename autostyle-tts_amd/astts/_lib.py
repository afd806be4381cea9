"""ctypes binding of libastts.so (the C ABI declared in include/astts.h).

There is no fallback: if the shared library is missing, or a call returns an error status,
this module raises.  Nothing here computes anything on the CPU.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_void_p

# HIP multiplexes its streams onto GPU_MAX_HW_QUEUES hardware queues; streams that share a queue never overlap, and the chip's command
# processor has FOUR pipes: queues that share a pipe take turns at every kernel boundary (two launch chains on such a pair run 2.4x slower
# each, synth/model.py).  FOUR queues = one per pipe: the pipeline's render stream and its (up to three) decode chains then sit on pipes of
# their own by construction and the caller's front stream shares the render queue.  Rounds 1-3 asked for 8 (two queues per pipe): with
# that the three-chain pipeline lost to the two-chain one; with 4 it wins (batch-8 benchmark, same box, alternating: 428 -> 457x real
# time; 5: the same; 3 and 6: no gain; 2: 292x).  Read by the HIP runtime when it initialises (the first HIP call), so it has to be in
# the environment before that; an explicit setting wins.
def _hip_already_initialised() -> bool:
    import sys
    t = sys.modules.get("torch")
    try:
        return bool(t is not None and t.cuda.is_initialized())
    except Exception:      # noqa: BLE001
        return False


if "GPU_MAX_HW_QUEUES" not in os.environ and _hip_already_initialised():
    # too late: the runtime read its own default (8 queues = two per pipe) at its first call.  Everything still works; the stream
    # pipeline then calibrates to two decode chains instead of three.
    import warnings
    warnings.warn("astts: HIP was initialised before astts was imported, so GPU_MAX_HW_QUEUES=4 (one hardware queue per command-processor "
                  "pipe) cannot take effect any more; PipelinedSynth then runs two decode chains instead of three (measured: 428x instead "
                  "of 457x real time on the batch-8 benchmark).  Import astts -- or export GPU_MAX_HW_QUEUES=4 -- before the first "
                  "torch.cuda call.", RuntimeWarning, stacklevel=2)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libastts.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "astts.h"))

OK = 0
ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_RANGE = -1, -2, -3, -4, -5
DTYPE_F16, DTYPE_F32 = 1, 2
METRIC_COSINE, METRIC_IP, METRIC_L2 = 0, 1, 2
KNN_MAX_K = 1024
KNN_FORCE_EXACT = 1


class AsttsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libastts error {code}: {msg}")
        self.code = code


class AsttsLibraryMissing(ImportError):
    pass


_CTYPES = {"void": None, "int": c_int32, "int32_t": c_int32, "int64_t": c_int64, "uint32_t": c_uint32, "size_t": c_size_t,
           "float": c_float, "double": c_double, "astts_stream_t": c_void_p}
_PROTOTYPE = re.compile(r"(?:^|(?<=[;{}]))\s*([\w\s*]+?)\b(astts_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl: str, proto: str, returned: bool = False):
    """One return type or parameter: a pointer is a c_void_p (a returned ``const char*`` a c_char_p), a scalar must be in _CTYPES."""
    words = [w for w in decl.replace("*", " ").split() if w != "const"]
    if "*" in decl:
        return c_char_p if returned and words == ["char"] else c_void_p
    if not words or words[0] not in _CTYPES:
        raise ValueError(f"unknown type {' '.join(decl.split())!r} in `{proto}`: add it to astts/_lib.py:_CTYPES")
    return _CTYPES[words[0]]


def parse_prototypes(text: str) -> dict:
    """name -> (restype, argtypes) of every ``type astts_name(args);`` of a C header."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                              # comments
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)                                # preprocessor lines
    text = re.sub(r"typedef\s+struct\s*\{[^{}]*\}", "typedef struct", text)         # struct bodies
    sigs = {}
    for m in _PROTOTYPE.finditer(text):
        ret, name, args = m.groups()
        proto = " ".join(f"{ret}{name}({args});".split())
        params = [] if args.split() in ([], ["void"]) else args.split(",")
        sigs[name] = (_ctype(ret, proto, returned=True), [_ctype(a, proto) for a in params])
    return sigs


def _header_signatures(paths, what: str) -> dict:
    sigs = {}
    for path in paths:
        if not os.path.exists(path):
            raise AsttsLibraryMissing(f"{path} not found: the ctypes signatures of {what} are derived from this header")
        with open(path) as f:
            sigs.update(parse_prototypes(f.read()))
    return sigs


def _set_prototypes(lib, sigs: dict):
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    """The C ABI as include/astts.h declares it: the header is the one place where a signature is written.  Parsed once."""
    return _header_signatures((HEADER_PATH,), "libastts.so")


def declared_symbols():
    return sorted(signatures())


@functools.lru_cache(maxsize=None)
def load():
    """Load libastts.so (once).  Raises AsttsLibraryMissing when it has not been built."""
    if not os.path.exists(LIB_PATH):
        raise AsttsLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C autostyle-tts_amd/csrc`.  There is no CPU fallback.")
    return _set_prototypes(ctypes.CDLL(LIB_PATH), signatures())


def bind_headers(*paths: str, what: str):
    """The binding of headers beside include/astts.h whose calls libastts.so exports too (include/knn/, include/llm/,
    include/session/): -> (signatures, load).  ``signatures()``: name -> (restype, argtypes) of every prototype of ``paths``, parsed
    once; ``load()``: the library object of ``load`` above with those prototypes set, once.  ``what`` names the calls in the message
    of a missing header."""
    @functools.lru_cache(maxsize=None)
    def header_signatures() -> dict:
        return _header_signatures(paths, what)

    @functools.lru_cache(maxsize=None)
    def load_bound():
        return _set_prototypes(load(), header_signatures())

    return header_signatures, load_bound


def check(code: int) -> None:
    if code != OK:
        msg = load().astts_last_error_string()
        raise AsttsError(code, msg.decode("utf-8", "replace") if msg else "")


def stream_ptr(stream=None) -> int:
    """hipStream_t of a torch stream (current stream by default) as an integer."""
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)
