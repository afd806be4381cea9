"""ctypes binding of the session entry points of libastts.so (include/session/astts_lm_session.h: decode sessions,
include/session/astts_flow_session.h: flow sessions, include/session/astts_flow_share.h: the launches a joined flow pass shares).

The session calls live in libastts.so itself; their signatures are parsed from their own headers exactly as astts/_lib.py parses
include/astts.h, and set on the library object that module loads (astts._lib.bind_headers).
"""
from __future__ import annotations

import os

from . import _lib

_DIR = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "session"))
HEADER_PATH = os.path.join(_DIR, "astts_lm_session.h")
FLOW_HEADER_PATH = os.path.join(_DIR, "astts_flow_session.h")
FLOW_SHARE_HEADER_PATH = os.path.join(_DIR, "astts_flow_share.h")

signatures, load = _lib.bind_headers(HEADER_PATH, FLOW_HEADER_PATH, FLOW_SHARE_HEADER_PATH, what="the session calls")
