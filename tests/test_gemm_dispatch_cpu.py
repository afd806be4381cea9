"""Which kernel the GEMM launcher picks, asked of the library itself (astts_op_gemm_kernel_kind: a host query, no GPU): every shape of
tests/test_conv_tiles_gpu.py lands on the tile it is there for, and the table covers all five instantiations of gemm_tile."""
import pytest

import conv_tile_cases as ctc


@pytest.fixture(scope="module")
def ops():
    from astts import ops

    return ops


def test_case_table_covers_every_tile_kind(ops):
    kinds = {}
    for c in ctc.CASES + ctc.EPILOGUE_SHAPES + ctc.VIEW_SHAPES:
        kind = ctc.kernel_kind(c)
        assert kind == c["expected"], (c["id"], ctc.geometry(c), kind)
        assert kind not in ("ring", "skinny"), c["id"]
        kinds.setdefault(kind, set()).add("f16" if c["x16"] else "f32")
    table = {ctc.kernel_kind(c) for c in ctc.CASES}
    assert table == {"T32", "T128", "T128x64", "T64k128", "T64k64"}
    assert kinds["T128"] == {"f16", "f32"} and kinds["T128x64"] == {"f16", "f32"}
    # the geometry the issue's table states, so that a slip in geometry() shows here and not as a different launch on the GPU
    by_id = {c["id"].split("-")[0]: ctc.geometry(c)[:2] for c in ctc.CASES}
    assert by_id["1"] == (5520, 2048) and by_id["2"] == (11012, 1024) and by_id["3"] == (26250, 256) and by_id["4"] == (50006, 128)
    assert by_id["5"] == (3000, 1280) and by_id["6"] == (50000, 64) and by_id["7"] == (5504, 1280) and by_id["8"] == (6000, 1280)


def test_kernel_kind_rule_boundaries(ops):
    """The rule's thresholds, each from both sides (384 tiles = 1.5 per CU; n <= 32; n > 64 for the 128-wide tile; BK 128 needs
    cin_pad % 128 == 0 and K >= 256), and the families in front of the tile kernels."""
    k = ops.gemm_kernel_kind
    assert k(128 * 383 + 1, 128, 64) == "T128" and k(128 * 383, 128, 64) == "T128x64"      # 384 / 383 tiles of 128 x 128 (766 of 128 x 64)
    assert k(128 * 383 + 1, 64, 64) == "T128x64" and k(128 * 383, 64, 64) == "T64k64"
    assert k(128 * 400, 32, 64) == "T32" and k(128 * 400, 33, 64) == "T128x64"
    assert k(1000, 256, 128, taps=2, plain=False) == "T64k128" and k(1000, 256, 128, taps=1, plain=False) == "T64k64"
    assert k(1000, 256, 192, taps=3, plain=False) == "T64k64"
    assert k(32, 256, 128) == "skinny" and k(33, 256, 128) == "T64k64" and k(32, 256, 128, plain=False) == "T64k64"
    assert k(32, 256, 128, out_f16=True) == "T64k64"
    # the ring kernels take plain fp16 GEMMs on whole K tiles from an aligned x; everything else stays on the register-staged tiles
    assert k(5504, 1024, 256, x_f16=True) == "ring"
    assert k(5504, 1024, 256, x_f16=True, x_aligned=False) == "T128x64" and k(5504, 1024, 250, x_f16=True) == "T128x64"
    assert k(5504, 1024, 256, x_f16=True, plain=False) == "T128x64" and k(63, 1024, 256, x_f16=True) == "T64k128"
    ops.set_gemm_ring_mode(0)
    try:
        assert k(5504, 1024, 256, x_f16=True) == "T128x64"
    finally:
        ops.set_gemm_ring_mode(-1)
    assert k(5504, 1024, 256, x_f16=True) == "ring"
    from astts import _lib

    with pytest.raises(_lib.AsttsError):
        k(0, 128, 64)
