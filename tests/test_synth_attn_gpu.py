"""GPU side of the synthesis attention suite: attn_mha_flash, attn_relpos_mfma, attn_relpos, attn_relpos_decode and attn_relpos_rows of
csrc/ops_attention.hip through astts.ops against the float64 definition, the cases and the bounds of tests/synth_attn_ref.py (error per
(batch row, head, query); zero rows exactly zero; don't-care rows finite).  Every bound comes from the reference side
(tests/test_synth_attn_cpu.py checks them there): MFMA_TOL = 3.45e-3 for the matrix-core kernels, F32_TOL = 1.92e-5 for the fp32 ones.
Before a case runs, the launcher's own conditions (pointer alignment, strides modulo 8, batch size, dtypes) are evaluated on its
arguments, so that a case cannot silently move to another kernel.  Each test prints one [parity] line."""
import os

import pytest
import torch

import synth_attn_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = torch.float16, torch.float32
_OUT = {}          # (kernel, dtypes, case name) -> the kernel's output [B, H, Tq, 64] on the CPU, computed once


def _i32(x, sl=slice(None)):
    return None if x is None else torch.tensor(x[sl], dtype=torch.int32, device=DEV)


def _mha(case, in_dtype, out_dtype, row=None):
    from astts import ops

    sl = slice(None) if row is None else slice(row, row + 1)
    hd = case.h * 64
    d = ref.mha_buffer(ref.build(case), in_dtype).to(DEV)[sl]
    out = ops.attn_mha(d[..., :hd], d[..., hd:2 * hd], d[..., 2 * hd:], case.h, lens=_i32(case.lens, sl), out_dtype=out_dtype)
    assert out.dtype == out_dtype
    return ref.heads_first(out.cpu(), case)


def _relpos(case, kernel, kv_dtype, pos_dtype, rows=None):
    """Run a relpos case (or the batch rows ``rows`` of it, a slice) on ``kernel`` -> [B, H, Tq, 64] fp32 on the CPU."""
    from astts import ops

    for name in ("ASTTS_RELPOS_VALU", "ASTTS_ATTN_DECODE", "ASTTS_ATTN_ROWS_HG"):
        assert name not in os.environ, f"{name} is set: the launcher would not pick the kernels this suite means to run"
    sl = slice(None) if rows is None else rows
    x = ref.build(case)
    hd = case.h * 64
    bufs = {k: v.to(DEV) for k, v in ref.relpos_buffers(x, kv_dtype, pos_dtype, pad=ref.VALU_PAD if kernel == "attn_relpos" else 0).items()}
    tm = case.form == "tm"
    if tm:
        q, kv = bufs["q"][:, sl], bufs["kv"][:case.tk, sl]
        ldk, k_bs, q_bs = kv.stride(0), kv.stride(1), q.stride(1)
    else:
        q, kv = bufs["q"][sl], bufs["kv"][sl, :case.tk]
        ldk, k_bs, q_bs = kv.stride(1), kv.stride(0), q.stride(0)
    k, v = kv[..., :hd], kv[..., hd:2 * hd]
    b = q.shape[1] if tm else q.shape[0]
    picked = ref.expected_kernel(case.tq, b, case.h, kv_dtype == F16, pos_dtype == F16, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                 bufs["table"].data_ptr(), ldk, bufs["table"].stride(0), k_bs, q_bs)
    assert picked == kernel, (case.name, kernel, picked)
    out = ops.attn_relpos(q, k, v, bufs["table"], bufs["bias_u"], bufs["bias_v"], case.h, lens=_i32(case.lens, sl), q_pos0=case.pos0,
                          pos_center=x.center, causal=case.causal, time_major=tm, key_start=_i32(case.key_start, sl))
    return ref.heads_first(out.cpu(), case)


def _once(key, run):
    if key not in _OUT:
        _OUT[key] = run()
    return _OUT[key]


def _relpos_once(case, kernel, kv_dtype, pos_dtype):
    return _once((kernel, kv_dtype, pos_dtype, case.name), lambda: _relpos(case, kernel, kv_dtype, pos_dtype))


def _judge(runs, bound, label):
    """runs: (case, tag, output) triples -> asserts every judged row within ``bound``, zero rows exactly zero, everything finite."""
    worst, where, failed, n = 0.0, None, [], 0
    for case, tag, got in runs:
        n += 1
        want = ref.expected(case)
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), (label, case.name, tag)
        err, bad = ref.row_errors(got, want)
        err = torch.where(ref.judged(case), err, torch.zeros_like(err))
        e = float(err.max())
        if e > worst:
            worst, where = e, (case.name, tag)
        if bool(bad.any()) or not e <= bound:
            b, h, i = [int(t) for t in (err == err.max()).nonzero()[0]]
            failed.append((case.name, tag, f"{e:.2e} at row {b} head {h} query {i}", f"{int(bad.sum())} zero rows not zero"))
    print(f"[parity] {label}: worst per-row err {worst:.2e} (bound {bound:.2e}) at {where}, {n} runs")
    assert not failed, failed[:10]


_NAME = {F16: "f16", F32: "f32"}
_ALL_DTYPES = ((F32, F32), (F16, F16), (F32, F16), (F16, F32))


def test_attn_mha_flash_all_four_instantiations():
    """t on and around every prefetch edge (64, 128, 192, 256) and 32-key mask edge with lens (t, 1) and (t, t - 1), lens on the edges at
    t = 257, a row without keys, a clamped lens; fp32 / fp16 input x fp32 / fp16 output on thirds of a fused q | k | v buffer."""
    runs = [(c, f"in {_NAME[i]} out {_NAME[o]}", _once(("mha", i, o, c.name), lambda: _mha(c, i, o)))
            for (i, o) in _ALL_DTYPES for c in ref.MHA_CASES]
    _judge(runs, ref.MFMA_TOL, "attn_mha_flash")


def _prefill_runs(kernel):
    return [(c, f"kv {_NAME[kvd]} table {_NAME[pd]}", _relpos_once(c, kernel, kvd, pd))
            for (kvd, pd) in _ALL_DTYPES for c in (ref.PREFILL_CASES if kvd == pd else ref.PREFILL_MIXED)]


def test_attn_relpos_mfma_prefill():
    """Batch-major (non-causal and causal, right-padded) and the time-major generation form with key_start on and around the 64-key
    tiles, pad queries in live rows, lens with key_start at pos0 > 0; aligned views -> the matrix-core kernel."""
    _judge(_prefill_runs("attn_relpos_mfma"), ref.MFMA_TOL, "attn_relpos_mfma")


def test_attn_relpos_valu_prefill():
    """The same data in a K | V buffer whose rows are 2 H 64 + 4 wide (ldk or k_bs = 4 mod 8) -> the fp32 VALU kernel."""
    _judge(_prefill_runs("attn_relpos"), ref.F32_TOL, "attn_relpos (VALU)")


def test_attn_relpos_prefill_kernels_agree():
    worst, where = 0.0, None
    for (kvd, pd) in ((F32, F32), (F16, F16)):
        for case in ref.PREFILL_CASES:
            a, b = _relpos_once(case, "attn_relpos_mfma", kvd, pd).double(), _relpos_once(case, "attn_relpos", kvd, pd).double()
            scale = ref.expected(case).abs().amax(-1)
            d = (a - b).abs().amax(-1) / torch.where(scale == 0, torch.ones_like(scale), scale)
            e = float(d[ref.judged(case)].max())
            if e > worst:
                worst, where = e, (case.name, _NAME[kvd])
    print(f"[parity] attn_relpos_mfma vs attn_relpos: worst per-row difference {worst:.2e} (bound {ref.MFMA_TOL:.2e}) at {where}")
    assert worst <= ref.MFMA_TOL, (worst, where)


def test_attn_relpos_decode_all_four_instantiations():
    """tk and key_start on and around the 256-key pass, time-major and batch-major caches with poisoned rows past tk, with and without
    lens; and causal with 40 poisoned keys after the query and no lens (the launcher bounds the keys at q_pos0 + 1)."""
    runs = [(c, f"kv {_NAME[kvd]} table {_NAME[pd]}", _relpos_once(c, "attn_relpos_decode", kvd, pd))
            for (kvd, pd) in _ALL_DTYPES for c in ref.DECODE_CASES]
    _judge(runs, ref.F32_TOL, "attn_relpos_decode")


def test_attn_relpos_rows():
    """33 and 40 rows x 4 heads over an fp16 time-major cache and an fp16 table: tk on and around the 64-key pass of the 16 key slots."""
    runs = [(c, "kv f16 table f16", _relpos_once(c, "attn_relpos_rows", F16, F16)) for c in ref.ROWS_CASES]
    _judge(runs, ref.F32_TOL, "attn_relpos_rows")


def test_attn_relpos_decode_and_rows_agree_on_shared_rows():
    """The first 32 rows of the 33-row cases go to attn_relpos_decode<half, half>; all 33 go to attn_relpos_rows."""
    worst, where = 0.0, None
    for case in (c for c in ref.ROWS_CASES if c.b == 33):
        a = _relpos(case, "attn_relpos_decode", F16, F16, rows=slice(0, 32)).double()
        b = _relpos_once(case, "attn_relpos_rows", F16, F16)[:32].double()
        scale = ref.expected(case)[:32].abs().amax(-1)
        e = float(((a - b).abs().amax(-1) / torch.where(scale == 0, torch.ones_like(scale), scale)).max())
        if e > worst:
            worst, where = e, case.name
    print(f"[parity] attn_relpos_decode<half, half> vs attn_relpos_rows: worst per-row difference {worst:.2e} (bound {ref.F32_TOL:.2e}) at {where}")
    assert worst <= ref.F32_TOL, (worst, where)


def test_batch_rows_are_independent():
    """Every batch row run alone gives the bits it has inside the batch: each kernel on one multi-row case, both forms for relpos.
    attn_relpos_rows needs more than 32 rows: there the 40-row batch is compared with its first and its last 33 rows."""
    pick = lambda cases, **kw: next(c for c in cases if all(getattr(c, k) == v for k, v in kw.items()))
    case = pick(ref.MHA_CASES, lens=(257, 192, 128, 64))
    whole = _once(("mha", F16, F16, case.name), lambda: _mha(case, F16, F16))
    for i in range(case.b):
        assert torch.equal(_mha(case, F16, F16, row=i)[0], whole[i]), (case.name, i)
    pre = (pick(ref.PREFILL_CASES, form="bm", causal=False, lens=(129, 128)), pick(ref.PREFILL_CASES, form="tm", tq=130))
    dec = (pick(ref.DECODE_CASES, form="bm", tk=257, pos0=256, lens=None), pick(ref.DECODE_CASES, form="tm", tk=513, lens=None))
    for kernel, cases in (("attn_relpos_mfma", pre), ("attn_relpos", pre), ("attn_relpos_decode", dec)):
        for case in cases:
            whole = _relpos_once(case, kernel, F16, F16)
            for i in range(case.b):
                assert torch.equal(_relpos(case, kernel, F16, F16, rows=slice(i, i + 1))[0], whole[i]), (kernel, case.name, i)
    case = pick(ref.ROWS_CASES, b=40, tk=129)
    whole = _relpos_once(case, "attn_relpos_rows", F16, F16)
    assert torch.equal(_relpos(case, "attn_relpos_rows", F16, F16, rows=slice(0, 33)), whole[:33])
    assert torch.equal(_relpos(case, "attn_relpos_rows", F16, F16, rows=slice(7, 40)), whole[7:])


def test_tq1_rejects_views_its_vector_loads_cannot_take():
    """The tq = 1 path loads q and the biases as float4 and K, V and the table four values at a time: a view off by one element, or a
    stride that is no multiple of 4, is ASTTS_ERR_INVALID (checked on the host: no kernel is launched)."""
    from astts import _lib, ops

    b, h, tk, center = 2, 2, 8, 100
    hd = h * 64
    z = lambda *shape, dtype=F32: torch.zeros(*shape, dtype=dtype, device=DEV)
    off = lambda n, dtype=F32: z(n + 1, dtype=dtype)[1:]                          # the same extent, one element further on

    def call(q=None, kv=None, table=None, bu=None, bv=None, kv_dtype=F16):
        q = z(1, b, hd) if q is None else q
        kv = z(tk, b, 2 * hd, dtype=kv_dtype) if kv is None else kv
        table = z(2 * center + 1, hd, dtype=kv_dtype) if table is None else table
        bu, bv = z(hd) if bu is None else bu, z(hd) if bv is None else bv
        return ops.attn_relpos(q, kv[..., :hd], kv[..., hd:2 * hd], table, bu, bv, h, q_pos0=tk - 1, pos_center=center, causal=True,
                               time_major=True)

    bad = {
        "q": dict(q=off(b * hd).view(1, b, hd)),
        "bias_u": dict(bu=off(hd)),
        "bias_v": dict(bv=off(hd)),
        "kv f16": dict(kv=off(tk * b * 2 * hd, F16).view(tk, b, 2 * hd)),
        "kv f32": dict(kv=off(tk * b * 2 * hd).view(tk, b, 2 * hd), kv_dtype=F32),
        "table f16": dict(table=off((2 * center + 1) * hd, F16).view(-1, hd)),
        "table f32": dict(table=off((2 * center + 1) * hd).view(-1, hd), kv_dtype=F32),
        "ldk, k_bs": dict(kv=z(tk, b, 2 * hd + 2, dtype=F16)),
        "ldp": dict(table=z(2 * center + 1, hd + 2, dtype=F16)[:, :hd]),
        "q_bs": dict(q=z(1, b, hd + 2)[..., :hd]),
    }
    for what, kw in bad.items():
        with pytest.raises(_lib.AsttsError) as err:
            call(**kw)
        assert err.value.code == _lib.ERR_INVALID, (what, err.value)
