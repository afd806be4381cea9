"""The shapes of tests/test_conv_tiles_gpu.py, kept apart from it so that a CPU test (tests/test_gemm_dispatch_cpu.py) can ask the
library's own rule (astts_op_gemm_kernel_kind) which kernel each of them runs: a later change of the rule must not silently move a
row of this table off the tile it is here for.

A case is what one operator call needs: ``op`` is "convT" (ops.conv_transpose1d, kernel 2 * stride, padding stride / 2), "conv"
(ops.conv1d) or "linear" (ops.linear / a plain ops.gemm); x is ``[b, t, cin]`` (``[t, cin]`` rows for "linear", b = 1); ``lens`` are the
rows' own input lengths (None: every row is full).  Epilogue: act(acc + bias) * alpha * row_scale[m] + residual.

Every batch length is deliberately NOT a multiple of 128, so batch boundaries and the padded taps around them fall inside 128-row
tiles, and m / n leave ragged last tiles.  The ragged lengths hold a full row, rows a few steps short, rows shorter than the kernel's
reach (len < dil * (k - 1)) and len = 1.
"""


def _c(id, op, expected, b, t, cin, cout, k=1, stride=1, dil=1, pad=0, x16=False, out16=False, lens=None, act="none", slope=0.1,
       alpha=1.0, bias=True, residual=False, row_scale=False):
    return dict(id=id, op=op, expected=expected, b=b, t=t, cin=cin, cout=cout, k=k, stride=stride, dil=dil, pad=pad, x16=x16, out16=out16,
                lens=lens, act=act, slope=slope, alpha=alpha, bias=bias, residual=residual, row_scale=row_scale)


CASES = [
    # 1: the vocoder's first transposed convolution at 16 x 344 frames: m = 16 * 345 = 5520, n = 8 * 256 = 2048 -> 44 * 16 = 704 tiles
    _c("1-convT-512-lens", "convT", "T128", 16, 344, 512, 256, stride=8,
       lens=[344, 340, 1, 200, 129, 128, 127, 344, 3, 257, 343, 64, 300, 2, 344, 339]),
    # 2: m = 4 * 2753 = 11012, n = 8 * 128 = 1024 -> 87 * 8 = 696 tiles
    _c("2-convT-256", "convT", "T128", 4, 2752, 256, 128, stride=8),
    # 3: the NSF source down-convolution: 18 channels (not a multiple of 8: the slow staging path), t_out = 8750, m = 26250 -> 206 * 2 = 412
    _c("3-conv-cin18-s8-lens", "conv", "T128", 3, 70001, 18, 256, k=16, stride=8, pad=4, lens=[70001, 69990, 9], act="leaky", slope=0.1,
       alpha=0.5, residual=True),
    _c("3b-conv-cin18-s8-lens-rowscale", "conv", "T128", 3, 70001, 18, 256, k=16, stride=8, pad=4, lens=[1, 70001, 69997], act="elu",
       alpha=1.25, bias=False, row_scale=True),
    # 4: the 1-tap source convolution: a plain fp32 GEMM with K = 18 -> 391 tiles
    _c("4-linear-k18", "linear", "T128", 1, 50006, 18, 128, act="relu", alpha=0.5, residual=True),
    _c("4b-linear-k18-rowscale", "linear", "T128", 1, 50006, 18, 128, act="leaky", slope=0.2, alpha=2.0, residual=True, row_scale=True),
    # 5: m = 3000, n = 1280: 24 * 10 = 240 < 384 <= 24 * 20 = 480
    _c("5-conv-gelu-out16", "conv", "T128x64", 2, 1500, 128, 1280, k=3, pad=1, out16=True, act="gelu"),
    # 5n: 1281 columns (the scalar column tail, odd ldc): 24 * 11 = 264 < 384 <= 24 * 21 = 504
    _c("5n-conv-gelu-out16-n1281", "conv", "T128x64", 2, 1500, 128, 1281, k=3, pad=1, out16=True, act="gelu", alpha=0.75),
    # 6: n = 64 never takes the 128-wide tile: m = 50000 -> 391 tiles of 128 x 64
    _c("6-conv-x16-dil2", "conv", "T128x64", 2, 25000, 64, 64, k=5, dil=2, pad=4, x16=True, residual=True),
    # 7: m = 5504, n = 1280 -> 43 * 10 = 430
    _c("7-conv-x16-out16-dil2", "conv", "T128", 16, 344, 256, 1280, k=3, dil=2, pad=2, x16=True, out16=True),
    # 7n: 1281 columns -> 43 * 11 = 473
    _c("7n-conv-x16-n1281", "conv", "T128", 16, 344, 256, 1281, k=3, dil=2, pad=2, x16=True, act="relu", bias=False, row_scale=True),
    # 8: t_out = 1500, m = 6000 -> 47 * 10 = 470
    _c("8-conv-x16-s2-lens", "conv", "T128", 4, 3000, 256, 1280, k=3, stride=2, pad=1, x16=True, lens=[3000, 2995, 1, 2], act="leaky",
       slope=0.2, alpha=0.5),
    # 9: 18 output columns
    _c("9-conv-n18-lens", "conv", "T32", 2, 30000, 128, 18, k=7, pad=3, lens=[29996, 5], act="elu", residual=True),
    # 10: small shapes of test_conv1d (tests/test_ops_gpu.py) with row lengths added
    _c("10a-conv-small-dil5-lens", "conv", "T64k128", 2, 300, 128, 128, k=11, dil=5, pad=25, lens=[297, 49], act="leaky", slope=0.1),
    _c("10b-conv-small-cin18-s8-lens", "conv", "T64k64", 2, 513, 18, 256, k=16, stride=8, pad=4, lens=[509, 1], act="leaky", slope=0.1),
    _c("10c-conv-small-s2-lens", "conv", "T64k128", 3, 301, 256, 256, k=3, stride=2, pad=1, lens=[301, 1, 296], act="leaky", slope=0.1,
       row_scale=True),
]

# interior and edge tiles in one launch (m and n ragged, n a multiple of 4): each runs through the four tile_epilogue_fast
# specialisations (none / fp16, none / fp32, none + residual / fp32, gelu / fp16), whose edge tiles take the general epilogue
EPILOGUE_SHAPES = [
    _c("e-T128-x16", "conv", "T128", 16, 345, 256, 1284, k=3, pad=1, x16=True),         # m = 5520: 44 * 11 = 484
    _c("e-T128x64-x32", "conv", "T128x64", 2, 1501, 128, 1284, k=3, pad=1),             # m = 3002: 24 * 11 = 264 < 384 <= 24 * 21 = 504
]

# plain fp32 GEMMs (K = 18) written through views of a larger zero-filled tensor: 391 tiles of each kind
VIEW_SHAPES = [
    _c("v-T128", "linear", "T128", 1, 50006, 18, 128),
    _c("v-T128x64", "linear", "T128x64", 1, 50006, 18, 64),
]


def geometry(c):
    """-> (m, n, taps, t_out, plain) of the GEMM the operator launches for a case (astts/ops.py: conv1d, conv_transpose1d, linear)."""
    if c["op"] == "convT":      # phase decomposition: t + 1 steps of two taps (pad 1), stride output phases per step
        return c["b"] * (c["t"] + 1), c["stride"] * c["cout"], 2, c["t"] + 1, False
    t_out = (c["t"] + 2 * c["pad"] - c["dil"] * (c["k"] - 1) - 1) // c["stride"] + 1
    plain = c["k"] == 1 and c["stride"] == 1 and c["pad"] == 0 and c["lens"] is None
    return c["b"] * t_out, c["cout"], c["k"], t_out, plain


def kernel_kind(c):
    """What the library says it runs for a case."""
    from astts import ops

    m, n, taps, _, plain = geometry(c)
    return ops.gemm_kernel_kind(m, n, c["cin"], taps=taps, plain=plain, x_f16=c["x16"], out_f16=c["out16"])
