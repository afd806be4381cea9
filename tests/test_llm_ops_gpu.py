"""GPU side of the Llama operator suite: the kernels of csrc/ops_llm.hip through astts.ops against the float64 definitions, cases and
bounds of tests/llm_ops_ref.py -- attn_gqa_mfma and attn_causal_gqa at their tile, block and mask edges (error per query row), the
grid-stride loops of rope_llama / rope_llama_ex / swiglu_rows past their grids, rmsnorm_rows' scalar path and short rows, argmax_rows'
ties and strided rows, mean_pool's clamps.  Every bound comes from the reference side (tests/test_llm_ops_cpu.py checks them there);
each operator prints one [parity] line with the worst error it showed beside its bound.  Attention: ATTN_TOL = 2.49e-3 per query row,
3 x the 8.3e-4 floor of the float64 emulation of the matrix-core kernel's fp16 roundings over the case list."""
import pytest
import torch

import llm_ops_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = ref.HD

_OUT = {}          # (kernel, case name) -> the kernel's output [B, heads, Tq, 128] on the CPU, computed once


def _i32(x):
    return None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)


def _attn(case, kernel="mfma", row=None):
    """Run one case (or its batch row ``row`` alone) -> [B, heads, Tq, 128] fp16 on the CPU."""
    from astts import ops

    x = ref.build_attn(case)
    sl = slice(None) if row is None else slice(row, row + 1)
    hq, hk = case.heads * HD, case.kv_heads * HD
    lens = None if case.lens is None else _i32(case.lens[sl])
    if case.form == "bm":
        d = x.bufs["qkv"].to(DEV)[sl]
        q, k, v = d[..., :hq], d[..., hq:hq + hk], d[..., hq + hk:]
        if kernel == "valu":
            out = ops.attn_causal_gqa(q, k, v, case.heads, case.kv_heads, HD, lens)
        else:
            out = ops.attn_gqa(q, k, v, case.heads, case.kv_heads, HD, lens=lens)
        return out.cpu().reshape(out.shape[0], case.tq, case.heads, HD).permute(0, 2, 1, 3)
    assert kernel == "mfma"
    q, cache = x.bufs["q"].to(DEV)[:, sl], x.bufs["cache"].to(DEV)[:, sl]
    out = ops.attn_gqa(q, cache[:case.tk, :, :hk], cache[:case.tk, :, hk:], case.heads, case.kv_heads, HD, lens=lens,
                       key_start=_i32(case.key_start[sl]), pos0=case.pos0, time_major=True)
    return out.cpu().reshape(case.tq, out.shape[1], case.heads, HD).permute(1, 2, 0, 3)


def _attn_once(case, kernel):
    if (kernel, case.name) not in _OUT:
        _OUT[(kernel, case.name)] = _attn(case, kernel)
    return _OUT[(kernel, case.name)]


def _check_attn(cases, kernel, label):
    worst, where, failed = 0.0, None, []
    for case in cases:
        got, want = _attn_once(case, kernel), ref.attn_expected(case)
        assert bool(torch.isfinite(got).all()), (label, case.name)
        err, bad = ref.row_errors(got, want)
        e = float(err.max())
        if e > worst:
            worst, where = e, case.name
        if bool(bad.any()) or not e <= ref.ATTN_TOL:
            b, h, i = [int(t) for t in (err == err.max()).nonzero()[0]]
            failed.append((case.name, f"{e:.2e} at row {b} head {h} query {i}", f"{int(bad.sum())} zero rows not zero"))
    print(f"[parity] {label}: worst per-row err {worst:.2e} (bound {ref.ATTN_TOL:.2e}) at {where}, {len(cases)} cases")
    assert not failed, failed


def test_attn_gqa_mfma_right_padded():
    """t in {1, 31 .. 385} with lens (t, 1), (t, t - 1), len on the tile and block edges, two query blocks beyond len; heads 6/2, 4/2, 2/2."""
    _check_attn(ref.ATTN_CASES_BM, "mfma", "attn_gqa (matrix cores), right-padded")


def test_attn_gqa_mfma_generation_form():
    """Time-major cache views with poisoned rows past tk, key_start on and around the 64-key tiles, decode steps, three query blocks
    at pos0 = 131, and lens with key_start at pos0 > 0."""
    _check_attn(ref.ATTN_CASES_TM, "mfma", "attn_gqa (matrix cores), generation form")


def test_attn_causal_gqa_valu_right_padded():
    _check_attn(ref.ATTN_CASES_BM, "valu", "attn_causal_gqa (VALU), right-padded")


def test_attn_kernels_agree_on_the_right_padded_list():
    worst, where = 0.0, None
    for case in ref.ATTN_CASES_BM:
        a, b, want = _attn_once(case, "mfma").double(), _attn_once(case, "valu").double(), ref.attn_expected(case)
        scale = want.abs().amax(-1)
        e = float(((a - b).abs().amax(-1) / torch.where(scale == 0, torch.ones_like(scale), scale)).max())
        if e > worst:
            worst, where = e, case.name
    print(f"[parity] attn_gqa vs attn_causal_gqa: worst per-row difference {worst:.2e} (bound {ref.ATTN_TOL:.2e}) at {where}")
    assert worst <= ref.ATTN_TOL, (worst, where)


def test_attn_batch_rows_are_independent():
    """Every batch row run alone gives the bits it has inside the batch (both kernels, both forms)."""
    pick = lambda cases, **kw: next(c for c in cases if all(getattr(c, k) == v for k, v in kw.items()))
    runs = [(pick(ref.ATTN_CASES_BM, heads=6, lens=(257, 129, 128, 64)), "mfma"), (pick(ref.ATTN_CASES_BM, heads=6, lens=(257, 129, 128, 64)), "valu"),
            (pick(ref.ATTN_CASES_TM, heads=6, tq=1, tk=513), "mfma"), (pick(ref.ATTN_CASES_TM, heads=4, tq=260), "mfma"),
            (pick(ref.ATTN_CASES_TM, heads=6, tq=70), "mfma")]
    for case, kernel in runs:
        whole = _attn_once(case, kernel)
        for i in range(case.b):
            assert torch.equal(_attn(case, kernel, row=i)[0], whole[i]), (case.name, kernel, i)


# ------------------------------------------------------------------------------------------------------------ the other kernels
def test_rmsnorm_rows():
    """c in {3, 63, 64, 66, 512, 3072, 3074} (scalar and float4 paths, less than a wave), 1 and 5 rows (a part-filled 4-row block), inputs
    scaled by 1e4 and 1e-4, fp32 and fp16 output."""
    from astts import ops

    worst32, worst16 = 0.0, 0.0
    for c in ref.RMS_C:
        for rows in ref.RMS_ROWS:
            for scale in ref.RMS_SCALES:
                x, w = ref.rms_inputs(c, rows, scale)
                want = ref.rmsnorm_ref(x, w, ref.RMS_EPS)
                y32 = ops.rmsnorm(x.to(DEV), w.to(DEV), ref.RMS_EPS, out_dtype=torch.float32).cpu().double()
                y16 = ops.rmsnorm(x.to(DEV), w.to(DEV), ref.RMS_EPS, out_dtype=torch.float16).cpu().double()
                assert y32.shape == want.shape and y16.shape == want.shape
                e32 = float(((y32 - want).abs().amax(-1) / want.abs().amax(-1)).max())
                e16 = float(((y16 - want).abs() / want.abs()).max())
                worst32, worst16 = max(worst32, e32), max(worst16, e16)
                assert e32 <= ref.RMS_TOL_F32 and e16 <= ref.RMS_TOL_F16, (c, rows, scale, e32, e16)
    print(f"[parity] rmsnorm: fp32 worst per-row err {worst32:.2e} (bound {ref.RMS_TOL_F32:.0e}), fp16 worst per-element err {worst16:.2e} "
          f"(bound {ref.RMS_TOL_F16:.2e})")


def _rope_check(got, x, want, bound, cols, what):
    assert torch.equal(got[..., cols:], x[..., cols:]), what                      # the v columns: not a bit changed
    err = (got.double() - want).abs()
    over = err > bound
    assert not bool(over.any()), (what, int(over.sum()), float((err - bound).max()))
    live = bound > 0
    return float((err[live] / bound[live]).max())


def test_rope_llama():
    """32 rotated heads of a 40-head q|k|v row, pos0 in {0, 200}; b = 2, t = 300 is 1 228 800 pairs, past the grid of 4096 x 256."""
    from astts import ops

    cos, sin = ref.rope_tables(520)
    dc, ds = cos.to(DEV), sin.to(DEV)
    ld, cols, worst = (ref.ROPE_HEADS + ref.ROPE_V_HEADS) * HD, ref.ROPE_HEADS * HD, 0.0
    for ci, (b, t, pos0) in enumerate(ref.ROPE_CASES):
        x = torch.randn(b, t, ld, generator=torch.Generator().manual_seed(40 + ci)).half()
        want, bound = ref.rope_ref(x, cos, sin, ref.ROPE_HEADS, HD, ref.rope_positions(b, t, pos0, False, None))
        got = ops.rope_llama_(x.to(DEV), dc, ds, ref.ROPE_HEADS, HD, pos0=pos0).cpu()
        worst = max(worst, _rope_check(got, x, want, bound, cols, (b, t, pos0)))
    print(f"[parity] rope_llama: worst err / bound {worst:.3f} (bound 2^-11 (|a| + |b|) (1 + 2^-10) per element)")


def test_rope_llama_ex():
    """Batch-major and time-major, per-row shifts, pos0 in {0, 200}, the decode step with a shift beyond its position (clamped to 0),
    and the grid-stride case."""
    from astts import ops

    cos, sin = ref.rope_tables(520)
    dc, ds = cos.to(DEV), sin.to(DEV)
    ld, cols, worst = (ref.ROPE_HEADS + ref.ROPE_V_HEADS) * HD, ref.ROPE_HEADS * HD, 0.0
    for ci, (b, t, pos0, tmaj, shift) in enumerate(ref.ROPE_EX_CASES):
        shape = (t, b, ld) if tmaj else (b, t, ld)
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(60 + ci)).half()
        want, bound = ref.rope_ref(x, cos, sin, ref.ROPE_HEADS, HD, ref.rope_positions(b, t, pos0, tmaj, shift))
        got = ops.rope_llama_ex_(x.to(DEV), dc, ds, ref.ROPE_HEADS, HD, pos0=pos0, shift=_i32(shift), time_major=tmaj).cpu()
        worst = max(worst, _rope_check(got, x, want, bound, cols, (b, t, pos0, tmaj, shift)))
    print(f"[parity] rope_llama_ex: worst err / bound {worst:.3f} (bound 2^-11 (|a| + |b|) (1 + 2^-10) per element)")


def test_swiglu_rows():
    """2100 x 8192 is 2 150 400 vectors of 8, past the grid of 8192 x 256; gates where exp(-x) overflows or vanishes stay finite."""
    from astts import ops

    rows, f = ref.SWIGLU_BIG
    gu = torch.randn(rows, 2 * f, generator=torch.Generator().manual_seed(7)).half()
    got = ops.swiglu(gu.to(DEV)).cpu().double()
    want, bound = ref.swiglu_ref(gu)
    err = (got - want).abs()
    worst = float((err / bound).max())
    assert got.shape == want.shape and not bool((err > bound).any()), (int((err > bound).sum()), worst)
    gates = torch.tensor(ref.SWIGLU_GATES, dtype=torch.float16)
    sp = torch.cat([torch.stack([gates, gates]), torch.tensor([[1.0] * 8, [-1.0] * 8], dtype=torch.float16)], 1)     # [2, 8 | 8]
    got = ops.swiglu(sp.to(DEV)).cpu().double()
    want, bound = ref.swiglu_ref(sp)
    assert bool(torch.isfinite(got).all()), got
    err = (got - want).abs()
    assert not bool((err > bound).any()), (got, want)
    worst = max(worst, float((err / bound).max()))
    print(f"[parity] swiglu: worst err / bound {worst:.3f} (bound 2^-10 |ref| + 2^-24 per element)")


def _argmax_rows(n, g):
    rows = [torch.randn(n, generator=g) for _ in range(3)]
    for a, b in ((255, 256), (3, 259), (70, 200)):          # neighbours in two waves / inside one thread's stride / across waves
        if b < n:
            r = torch.randn(n, generator=g)
            r[a] = r[b] = 9.0
            rows.append(r)
    r = torch.randn(n, generator=g)
    r[n // 2] = 50.0
    r[n - 1] = float("inf")
    rows.append(r)
    rows.append(torch.full((n,), float("-inf")))
    return torch.stack(rows)


def test_argmax_rows():
    from astts import ops

    g = torch.Generator().manual_seed(11)
    checked = 0
    for n in ref.ARGMAX_N:
        x = _argmax_rows(n, g)
        want = torch.argmax(x, 1)
        assert int(want[-1]) == 0 and int(want[-2]) == n - 1
        got = ops.argmax_rows(x.to(DEV)).cpu()
        assert got.dtype == torch.int32 and got.tolist() == want.tolist(), (n, got.tolist(), want.tolist())
        wide = torch.full((x.shape[0], n + 13), 99.0)        # larger than everything but +inf: a read outside the slice shows
        wide[:, 5:5 + n] = x
        view = wide.to(DEV)[:, 5:5 + n]
        assert view.stride(0) == n + 13
        assert ops.argmax_rows(view).cpu().tolist() == want.tolist(), ("strided", n)
        checked += 2 * x.shape[0]
    print(f"[parity] argmax_rows: {checked} rows equal torch.argmax (0 differ; n in {ref.ARGMAX_N}, ties, +inf, all -inf, strided rows)")


def test_mean_pool():
    from astts import ops

    worst = 0.0
    lens = torch.tensor(ref.MEAN_POOL_LENS, dtype=torch.int32)
    for c in ref.MEAN_POOL_C:
        x = torch.randn(len(lens), ref.MEAN_POOL_T, c, generator=torch.Generator().manual_seed(c))
        want, bound = ref.mean_pool_ref(x, ref.MEAN_POOL_LENS)
        got = ops.mean_pool(x.to(DEV), lens.to(DEV)).cpu().double()
        assert float(got[0].abs().max()) == 0.0                                   # lens = 0
        err = (got - want).abs()
        assert not bool((err > bound).any()), (c, float((err - bound).max()))
        live = bound > 0
        worst = max(worst, float((err[live] / bound[live]).max()))
        whole = ops.mean_pool(x.to(DEV)).cpu().double()                           # lens = None: every row over all t tokens
        at_t = [i for i, n in enumerate(ref.MEAN_POOL_LENS) if n >= ref.MEAN_POOL_T]
        assert len(at_t) == 2 and torch.equal(whole[at_t], got[at_t])              # lens = t and lens = t + 7 (clamped): the same bits
    print(f"[parity] mean_pool: worst err / bound {worst:.3f} (bound n 2^-24 mean|x| per element)")
