"""The decode session's bookkeeping (csrc/lm_session.h: slots, shifts, quantum sizing, rebase; no HIP) driven by the stand-alone host
program tests/host/lm_session_plan_main.cpp, compiled with -fsanitize=address,undefined and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_session_bookkeeping_program_under_host_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "lm_session_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "lm_session_plan_main.cpp"), "-o", str(exe)], check=True, timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "lm_session_plan: ok" in run.stdout
