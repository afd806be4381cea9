"""What a joined flow pass shares (csrc/flow_share.h: the segment table of the one tfm_ffn_fused launch, the grouping of the batches
whose astts_op_gemm runs as one launch; no HIP) driven by the stand-alone host program tests/host/flow_share_plan_main.cpp, compiled
with -fsanitize=address,undefined and run directly; and the ctypes signatures of the two entry points, parsed from their own header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flow_share_plan_program_under_host_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "flow_share_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "flow_share_plan_main.cpp"), "-o", str(exe)], check=True, timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "flow_share_plan: ok" in run.stdout


def test_flow_share_signatures_come_from_their_own_header():
    from astts import _lib, _lib_session

    sigs = _lib_session.signatures()
    want = {"astts_op_tfm_ffn_fused_seg", "astts_op_gemm_planned"}
    assert want <= set(sigs)
    assert not want & set(_lib.signatures()), "the shared launches are declared in include/session/, not in include/astts.h"
    # the arguments of the operators they extend, plus the segment table (n_seg, row0, rows for m) / plan_m
    assert len(sigs["astts_op_tfm_ffn_fused_seg"][1]) == len(_lib.signatures()["astts_op_tfm_ffn_fused"][1]) + 2
    assert len(sigs["astts_op_gemm_planned"][1]) == len(_lib.signatures()["astts_op_gemm"][1]) + 1
    lib = _lib_session.load()
    for name in want:
        assert hasattr(lib, name), f"{name} is declared but libastts.so does not export it"
