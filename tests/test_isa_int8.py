"""Build-time ISA checks of csrc/ops_int8.hip (cross-compiled, no GPU): the int8 GEMM runs on the i8 matrix cores and nothing
spills to scratch."""
import os
import re

from test_isa_checks import CSRC, _asm, _kernels


def test_int8_gemm_uses_i8_mfma_and_no_scratch(tmp_path):
    asm = _asm(os.path.join(CSRC, "ops_int8.hip"), tmp_path)
    ks = _kernels(asm, r"i8_gemm")
    assert len(ks) == 1, sorted(ks)
    body = next(iter(ks.values()))
    assert re.search(r"v_mfma_i32_(32x32x32|16x16x64)_i8", body), "no i8 MFMA in i8_gemm"
    assert "v_mfma_f32_32x32x2_f32" in body                       # the LoRA side loop
    for name, b in _kernels(asm, r"i8_").items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", b), f"{name} uses scratch"
        assert "scratch_" not in b and "buffer_store" not in b, name


def test_lora_down_runs_on_fp32_mfma(tmp_path):
    ks = _kernels(_asm(os.path.join(CSRC, "ops_int8.hip"), tmp_path), r"i8_lora_down")
    assert len(ks) == 2, sorted(ks)
    assert all("v_mfma_f32_32x32x2_f32" in b for b in ks.values())
