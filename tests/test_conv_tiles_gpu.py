"""gemm_tile (csrc/ops_gemm.hip: the implicit-GEMM kernel behind ops.conv1d, ops.conv_transpose1d and the fp32-activation ops.linear) at
the tiles the VOCODER runs: the launcher picks one of five instantiations by output size, and tests/test_ops_gpu.py's convolutions (at most
40 tiles of 128 x 128) reach only the 64 x 64 and 128 x 32 ones.  Here every case first asserts, through the launcher's own rule
(astts_op_gemm_kernel_kind), the tile it is meant for, then compares the WHOLE output with a plain PyTorch CPU definition of the same
operation on the fp16-rounded operands (fp64 where cheap, fp32 otherwise).  Shapes and lengths: tests/conv_tile_cases.py.

Bars (the project's own, from test_conv1d / test_gemm_rows_*): 2e-4 of the output's maximum for fp32 outputs (fp32 accumulation order
only), 1.5e-3 for fp16 outputs (2^-11 output rounding).

Row lengths (``lens``): input steps at or beyond a row's length read as zero.  The input handed to the kernel holds large finite garbage
there, the definition zeros, and the output steps below the row's own output length are compared (ops.conv1d leaves the rest unspecified).

Measured on an MI355X when the file was written (relative error | bar): 1 8.3e-7, 2 5.5e-7, 3 3.1e-7, 3b 7.0e-7, 4 7.6e-8, 4b 1.2e-7, 6 2.1e-7,
7n 4.6e-7, 8 3.2e-7, 9 3.1e-7, 10a-c 2.1e-7 .. 4.0e-7 | 2e-4;  5 2.9e-4, 5n 3.7e-4, 7 2.7e-4 | 1.5e-3 (fp16 outputs);  the epilogue shapes
1.9e-7 .. 3.4e-7 | 2e-4 and 2.5e-4 .. 3.7e-4 | 1.5e-3;  the views 7.6e-8 .. 1.1e-7 | 2e-4 and 2.3e-4 .. 4.2e-4 | 1.5e-3, bit-equal to the contiguous
launch with every guard cell zero.  The file takes 2.6 s of test time (4.8 s with start-up); the references are oneDNN convolutions of at
most 23 GFLOP.  Mutation check (by hand, not kept): with the row-length clamp of the fast staging path removed, cases 1, 8, 9, 10a, 10c
fail and tests/test_ops_gpu.py passes; with the stride applied to the tap offset, cases 3, 3b, 8, 10b, 10c fail.
"""
import math
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_tile_cases as ctc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL32, TOL16 = 2e-4, 1.5e-3

ACTS = {"none": lambda t: t, "relu": F.relu, "gelu": F.gelu, "elu": F.elu}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[conv tiles] wall time of tests/test_conv_tiles_gpu.py: {time.perf_counter() - t0:.1f} s")


def _act(v, name, slope):
    return F.leaky_relu(v, slope) if name == "leaky" else ACTS[name](v)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _inputs(c):
    """CPU tensors of a case: what the kernel is handed (x with garbage behind each row's length) and what the definition reads
    (x_def: fp16-rounded, zero behind each row's length)."""
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    b, t, cin, cout, k, s = c["b"], c["t"], c["cin"], c["cout"], c["k"], c["stride"]
    m, n, _, t_out, _ = ctc.geometry(c)
    x = torch.randn(b, t, cin, generator=g)
    x_def = x.half().float()
    if c["x16"]:
        x = x.half()
    if c["lens"] is not None:
        assert len(c["lens"]) == b
        x, x_def = x.clone(), x_def.clone()
        for i, ln in enumerate(c["lens"]):
            junk = (1000.0 + 1000.0 * torch.rand(t - ln, cin, generator=g)) * (torch.randint(0, 2, (t - ln, cin), generator=g) * 2 - 1)
            x[i, ln:] = junk.to(x.dtype)
            x_def[i, ln:] = 0.0
    if c["op"] == "convT":
        w = torch.randn(cin, cout, 2 * s, generator=g) / math.sqrt(cin * 2)
    elif c["op"] == "conv":
        w = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k)
    else:
        w = torch.randn(cout, cin, generator=g) / math.sqrt(cin)
    bias = torch.randn(cout, generator=g)
    res = torch.randn(m, n, generator=g) if c["residual"] else None
    rs = (0.5 + torch.rand(m, generator=g)) if c["row_scale"] else None
    return x, x_def, w, bias, res, rs


def _accumulate(c, x_def, w):
    """The contraction alone, channels-last [b, t_out, n] ([b, t * stride, cout] for the transposed form): F.conv1d / F.conv_transpose1d /
    F.linear on the fp16-rounded operands; fp64 below 2 GFLOP."""
    m, n, taps, _, _ = ctc.geometry(c)
    dt = torch.float64 if 2.0 * m * n * taps * c["cin"] < 2e9 else torch.float32
    xd, wd = x_def.to(dt), w.half().to(dt)
    if c["op"] == "convT":
        return F.conv_transpose1d(xd.transpose(1, 2), wd, None, stride=c["stride"], padding=c["stride"] // 2).transpose(1, 2)
    if c["op"] == "conv":
        return F.conv1d(xd.transpose(1, 2), wd, None, stride=c["stride"], dilation=c["dil"], padding=c["pad"]).transpose(1, 2)
    return F.linear(xd, wd)


def _epilogue(c, acc, bias, res, rs):
    """act(acc + bias) * alpha * row_scale[m] + residual[m, n] (include/astts.h)"""
    v = acc + bias.to(acc.dtype) if c["bias"] else acc
    v = _act(v, c["act"], c["slope"]) * c["alpha"]
    if rs is not None:
        v = v * rs.to(acc.dtype).view(v.shape[0], v.shape[1], 1)
    if res is not None:
        v = v + res.to(acc.dtype).view(v.shape)
    return v


def _valid_steps(c, steps):
    """[b, steps] mask of the output steps a row's own length defines"""
    if c["lens"] is None:
        return torch.ones(c["b"], steps, dtype=torch.bool)
    out_len = []
    for ln in c["lens"]:
        if c["op"] == "convT":
            out_len.append(ln * c["stride"])
        else:
            out_len.append(min(max((ln + 2 * c["pad"] - c["dil"] * (c["k"] - 1) - 1) // c["stride"] + 1, 0), steps))
    return torch.arange(steps)[None, :] < torch.tensor(out_len)[:, None]


def _launch(ops, c, xd, pw, res, rs, lens):
    """The operator call of a case: the public wrapper where it can express the epilogue, ops.gemm with the same geometry otherwise."""
    _, n, _, t_out, _ = ctc.geometry(c)
    odt = torch.float16 if c["out16"] else torch.float32
    if c["op"] == "convT":
        return ops.conv_transpose1d(xd, pw, padding=c["stride"] // 2, lens=lens)
    wrapper = c["bias"] and rs is None
    if c["op"] == "conv":
        if wrapper:
            return ops.conv1d(xd, pw, stride=c["stride"], dil=c["dil"], pad=c["pad"], act=c["act"], alpha=c["alpha"], slope=c["slope"],
                              residual=None if res is None else res.view(c["b"], t_out, n), out_dtype=odt, lens=lens)
        y = ops.gemm(xd, pw, act=c["act"], residual=res, row_scale=rs, alpha=c["alpha"], slope=c["slope"], t_in=c["t"], t_out=t_out,
                     stride=c["stride"], dil=c["dil"], pad=c["pad"], use_bias=c["bias"], out_dtype=odt, in_lens=lens)
        return y.view(c["b"], t_out, n)
    if wrapper and c["act"] != "leaky":
        return ops.linear(xd, pw, act=c["act"], residual=None if res is None else res.view(1, -1, n), alpha=c["alpha"], out_dtype=odt)
    y = ops.gemm(xd.reshape(-1, c["cin"]), pw, act=c["act"], residual=res, row_scale=rs, alpha=c["alpha"], slope=c["slope"],
                 use_bias=c["bias"], out_dtype=odt)
    return y.view(1, -1, n)


def _pack(ops, c, w, bias):
    if c["op"] == "convT":
        return ops.PackedWeight.from_conv_transpose1d(w, bias, c["stride"])
    if c["op"] == "conv":
        return ops.PackedWeight.from_conv1d(w, bias)
    return ops.PackedWeight(w, bias)


def _compare(c, y, ref, tag=""):
    """whole output, every step a row's length defines; -> relative error (of the compared output's maximum)"""
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert y.dtype == (torch.float16 if c["out16"] else torch.float32)
    valid = _valid_steps(c, ref.shape[1])
    yv, rv = y.cpu().to(ref.dtype)[valid], ref[valid]
    assert bool(torch.isfinite(yv).all())
    err = float((yv - rv).abs().max() / rv.abs().max())
    tol = TOL16 if c["out16"] else TOL32
    print(f"[conv tiles] {c['id']}{tag}: {c['expected']}, rel err {err:.2e} (bar {tol:.1e}), {int(valid.sum())} of {valid.numel()} output steps compared")
    if err >= tol:       # where: tells staging / tap addressing / length clamp / epilogue apart
        d = (y.cpu().to(ref.dtype) - ref).abs() * valid[:, :, None]
        bi, ti, ni = (int(v) for v in (d == d.max()).nonzero()[0])
        bad = (d > tol * float(rv.abs().max()))
        print(f"[conv tiles] {c['id']}{tag}: worst at batch {bi} step {ti} column {ni}; bad elements per batch row "
              f"{bad.sum((1, 2)).tolist()}, steps with a bad element per row {[int(r.any(1).sum()) for r in bad]}")
    return err, tol


def _check_kind(ops, c):
    kind = ctc.kernel_kind(c)
    assert kind == c["expected"], f"{c['id']}: the launcher runs {kind} for {ctc.geometry(c)}, the case is meant for {c['expected']}"


def _to_dev(c, x, res, rs):
    lens = None if c["lens"] is None else torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
    return x.to(DEV), None if res is None else res.to(DEV), None if rs is None else rs.to(DEV), lens


@pytest.mark.parametrize("c", ctc.CASES, ids=lambda c: c["id"])
def test_conv_tile_matches_definition(c):
    from astts import ops

    _check_kind(ops, c)
    x, x_def, w, bias, res, rs = _inputs(c)
    pw = _pack(ops, c, w, bias)
    xd, resd, rsd, lens = _to_dev(c, x, res, rs)
    y = _launch(ops, c, xd, pw, resd, rsd, lens)
    torch.cuda.synchronize()
    m, n, _, t_out, _ = ctc.geometry(c)
    if c["op"] != "convT":
        assert y.numel() == m * n        # the launch had the geometry the tile was asked for
    ref = _epilogue(c, _accumulate(c, x_def, w), bias, res, rs)
    err, tol = _compare(c, y, ref)
    assert err < tol


@pytest.mark.parametrize("c", ctc.EPILOGUE_SHAPES, ids=lambda c: c["id"])
def test_fast_epilogue_specialisations_with_interior_and_edge_tiles(c):
    """tile_epilogue_fast serves interior tiles when the activation / output type / residual combination is one of four and everything is
    16-byte aligned; the tiles on the ragged m and n edges of the same launch take the general epilogue.  Each of the four, then the same
    launch with a row scale (which switches the fast path off), alpha != 1 and no bias."""
    from astts import ops

    _check_kind(ops, c)
    x, x_def, w, bias, _, _ = _inputs(c)
    m, n, _, t_out, _ = ctc.geometry(c)
    g = torch.Generator().manual_seed(5)
    res, rs = torch.randn(m, n, generator=g), 0.5 + torch.rand(m, generator=g)
    pw = _pack(ops, c, w, bias)
    acc = _accumulate(c, x_def, w)
    worst = []
    for act, out16, use_res, use_rs, use_bias, alpha in [("none", True, False, False, True, 1.0), ("none", False, False, False, True, 1.0),
                                                         ("none", False, True, False, True, 1.0), ("gelu", True, False, False, True, 1.0),
                                                         ("none", False, True, True, True, 0.5), ("gelu", True, False, True, False, 1.5),
                                                         ("none", False, True, False, False, 0.75)]:
        cc = dict(c, act=act, out16=out16, residual=use_res, row_scale=use_rs, bias=use_bias, alpha=alpha)
        _check_kind(ops, cc)
        xd, resd, rsd, lens = _to_dev(cc, x, res if use_res else None, rs if use_rs else None)
        y = _launch(ops, cc, xd, pw, resd, rsd, lens)
        torch.cuda.synchronize()
        ref = _epilogue(cc, acc, bias, res if use_res else None, rs if use_rs else None)
        worst.append(_compare(cc, y, ref, tag=f" [{act}, {'fp16' if out16 else 'fp32'} out{', residual' if use_res else ''}"
                                              f"{', row scale' if use_rs else ''}{'' if use_bias else ', no bias'}, alpha {alpha}]"))
    assert all(err < tol for err, tol in worst), worst


@pytest.mark.parametrize("out16", [False, True], ids=["out32", "out16"])
@pytest.mark.parametrize("c", ctc.VIEW_SHAPES, ids=lambda c: c["id"])
def test_gemm_into_offset_and_odd_strided_views(c, out16):
    """ops.gemm(out=view) into a zero-filled larger tensor: a 16-byte aligned column offset (interior tiles may take the vectorised
    epilogue), offset 1 with ldc % 4 == 0 (the general epilogue's vector stores at an unaligned address), and an odd ldc (scalar
    stores).  Each equals the contiguous launch bit for bit, and every guard row and column is still exactly zero."""
    from astts import ops

    c = dict(c, out16=out16)
    _check_kind(ops, c)
    x, x_def, w, bias, _, _ = _inputs(c)
    m, n, _, _, _ = ctc.geometry(c)
    odt = torch.float16 if out16 else torch.float32
    vec = 8 if out16 else 4               # elements per 16 bytes
    pw = _pack(ops, c, w, bias)
    xd = x[0].to(DEV)
    for act in ("none", "leaky"):
        cc = dict(c, act=act, slope=0.2, alpha=1.0 if act == "none" else 0.5)
        y0 = ops.gemm(xd, pw, act=act, slope=cc["slope"], alpha=cc["alpha"], out_dtype=odt)
        torch.cuda.synchronize()
        ref = _epilogue(cc, _accumulate(cc, x_def, w), bias, None, None)
        err, tol = _compare(cc, y0.view(1, m, n), ref, tag=f" [{act}, contiguous]")
        assert err < tol
        for ld, off, aligned in [(n + 2 * vec, vec, True), (n + 2 * vec, 1, False), (n + 2 * vec + 1, 3, None)]:
            big = torch.zeros(m + 2, ld, dtype=odt, device=DEV)
            view = big[1:m + 1, off:off + n]
            assert view.stride(0) == ld and ld % 4 == (1 if aligned is None else 0)
            assert aligned is None or (view.data_ptr() % 16 == 0) == aligned      # (odd ld: the rows' alignment varies)
            out = ops.gemm(xd, pw, act=act, slope=cc["slope"], alpha=cc["alpha"], out=view)
            torch.cuda.synchronize()
            assert out.data_ptr() == view.data_ptr()
            diff = int((_bits(view) != _bits(y0)).sum())
            assert diff == 0, f"{c['id']} {act} ld={ld} off={off}: {diff} elements differ from the contiguous launch"
            big[1:m + 1, off:off + n] = 0
            stray = int((_bits(big) != 0).sum())
            assert stray == 0, f"{c['id']} {act} ld={ld} off={off}: {stray} guard elements were written"


@pytest.mark.parametrize("cid", ["3-conv-cin18-s8-lens", "7-conv-x16-out16-dil2", "5-conv-gelu-out16", "6-conv-x16-dil2", "9-conv-n18-lens",
                                 "10a-conv-small-dil5-lens", "10b-conv-small-cin18-s8-lens", "1-convT-512-lens"])
def test_conv_tile_launches_are_bit_reproducible(cid):
    """The kernel has no atomics and every output element one owner: two launches on the same inputs that differ in one bit are a race
    (a missing barrier between the staging buffers, the epilogue slab reusing live LDS).  One launch per tile kind, both staging paths."""
    from astts import ops

    c = next(k for k in ctc.CASES if k["id"] == cid)
    _check_kind(ops, c)
    x, _, w, bias, res, rs = _inputs(c)
    pw = _pack(ops, c, w, bias)
    xd, resd, rsd, lens = _to_dev(c, x, res, rs)
    first = _bits(_launch(ops, c, xd, pw, resd, rsd, lens))
    for rep in range(3):
        again = _bits(_launch(ops, c, xd, pw, resd, rsd, lens))
        torch.cuda.synchronize()
        assert torch.equal(first, again), f"{cid} ({c['expected']}) launch {rep + 2}: {int((first != again).sum())} elements differ"
