"""The flow session's bookkeeping (csrc/flow_session.h: slots, rows, Euler steps, the sequence ranges of a joined pass; no HIP) driven by
the stand-alone host program tests/host/flow_session_plan_main.cpp, compiled with -fsanitize=address,undefined and run directly; and
the session's ctypes signatures, parsed from its own header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flow_session_bookkeeping_program_under_host_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "flow_session_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "flow_session_plan_main.cpp"), "-o", str(exe)], check=True, timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "flow_session_plan: ok" in run.stdout


def test_flow_session_signatures_come_from_its_own_header():
    from astts import _lib, _lib_session

    sigs = _lib_session.signatures()
    want = {"astts_flow_session_" + n for n in ("bytes", "create", "destroy", "can_admit", "admit", "step", "state")}
    assert want <= set(sigs)
    assert not want & set(_lib.signatures()), "the flow session is declared in include/session/, not in include/astts.h"
    assert len(sigs["astts_flow_session_admit"][1]) == 13 and len(sigs["astts_flow_session_create"][1]) == 9
    lib = _lib_session.load()
    for name in want:
        assert hasattr(lib, name), f"{name} is declared but libastts.so does not export it"
