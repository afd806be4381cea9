"""CPU side of the Llama operator suite (tests/llm_ops_ref.py): the float64 attention reference against torch's scaled_dot_product_attention,
the case lists against what the kernels' tiles need, the sensitivity of every case's inputs to every wrong mask (a mistake the size of one
key changes every query row it touches by >= 10 x ATTN_TOL), the cap on zero rows, and ATTN_TOL against the measured fp16-emulation floor.
Measured here: floor 8.30e-4 (ATTN_EMU_FLOOR 8.3e-4), ATTN_TOL 2.49e-3.  Nothing here needs a GPU or the native library."""
import pytest
import torch

import llm_ops_ref as ref

ALL_ATTN = ref.ATTN_CASES_BM + ref.ATTN_CASES_TM
IDS = [c.name for c in ALL_ATTN]


def test_case_lists_cover_the_tile_and_block_edges():
    bm, tm = ref.ATTN_CASES_BM, ref.ATTN_CASES_TM
    assert len({c.name for c in ALL_ATTN}) == len(ALL_ATTN)
    for geom in ref.GEOMS:
        mine = [c for c in bm if (c.heads, c.kv_heads) == geom]
        for t in ref.BM_T:
            assert {c.lens for c in mine if c.tq == t} >= {(t, 1), (t, t - 1)}, (geom, t)
        assert {(257, 129, 128, 64), (257, 100)} <= {c.lens for c in mine}
        mine = [c for c in tm if (c.heads, c.kv_heads) == geom]
        assert {(c.tq, c.tk) for c in mine} >= {(1, 1), (1, 64), (1, 65), (1, 129), (1, 513), (3, 77), (33, 200), (130, 333), (260, 391)}
        assert all(c.b == 4 for c in mine)
        seen = {s for c in mine for s in c.key_start}
        assert seen >= set(ref.KEY_START_SET), sorted(seen)
        for c in mine:
            assert all(0 <= s <= c.tk - 1 for s in c.key_start) and c.pos0 + c.tq <= c.tk
            if c.lens is None:
                assert c.pos0 + c.tq == c.tk and c.pos0 + c.tq - 1 in c.key_start, c.name          # one visible key for the last query
                assert c.tq == 1 or any(c.pos0 < s < c.pos0 + c.tq - 1 for s in c.key_start), c.name   # pad queries in a live row
        assert any(c.lens is not None and c.pos0 > 0 and any(c.key_start) for c in mine)
        assert any(c.tq == 260 and c.pos0 % 32 != 0 for c in mine)
        # tile skipping: jfirst = 64, 128 and 192 with more than one query, and in a decode step
        assert {s // 64 * 64 for c in mine if c.tq > 1 for s in c.key_start} >= {0, 64, 128, 192}
        assert {s // 64 * 64 for c in mine if c.tq == 1 for s in c.key_start} >= {0, 64, 128, 192}
    assert sum((c.heads, c.kv_heads) == (2, 2) for c in ALL_ATTN) == 1


def _unpadded_rows(case):
    return [i for i in range(case.b) if (case.lens is None or case.lens[i] >= case.tk) and (case.key_start is None or case.key_start[i] == 0)]


@pytest.mark.parametrize("case", [c for c in ALL_ATTN if _unpadded_rows(c)], ids=[c.name for c in ALL_ATTN if _unpadded_rows(c)])
def test_reference_equals_torch_sdpa_on_unpadded_rows(case):
    """Batch rows without padding (lens = tk, key_start = 0): the reference is torch.nn.functional.scaled_dot_product_attention in float64
    with the KV heads repeated and the causal mask shifted by pos0."""
    x = ref.build_attn(case)
    full = _unpadded_rows(case)
    rep = case.heads // case.kv_heads
    mask = torch.arange(case.tk)[None, :] <= (case.pos0 + torch.arange(case.tq))[:, None]
    for i in full:
        want = torch.nn.functional.scaled_dot_product_attention(x.q[i:i + 1], x.k[i:i + 1].repeat_interleave(rep, 1),
                                                                x.v[i:i + 1].repeat_interleave(rep, 1), attn_mask=mask)
        err, bad = ref.row_errors(ref.attn_expected(case)[i:i + 1], want)
        assert float(err.max()) < 1e-12 and not bool(bad.any()), (case.name, i, float(err.max()))


def test_reference_on_rows_done_by_hand():
    """Two keys, one query head per KV head, identical scores: the output is the mean of the visible values; the masks remove exactly
    the keys they name, and a query with no key, or at or beyond lens, gives zeros."""
    q = torch.zeros(1, 1, 3, 128, dtype=torch.float64)
    k = torch.zeros(1, 1, 3, 128, dtype=torch.float64)
    v = torch.arange(3, dtype=torch.float64)[None, None, :, None].expand(1, 1, 3, 128) + 1.0         # values 1, 2, 3
    got = ref.attn_ref(q, k, v)[0, 0, :, 0].tolist()
    assert got == [1.0, 1.5, 2.0]
    assert ref.attn_ref(q, k, v, key_start=[1])[0, 0, :, 0].tolist() == [0.0, 2.0, 2.5]
    assert ref.attn_ref(q, k, v, lens=[2])[0, 0, :, 0].tolist() == [1.0, 1.5, 0.0]
    assert ref.attn_ref(q[:, :, :1], k, v, pos0=2)[0, 0, :, 0].tolist() == [2.0]
    assert ref.attn_ref(q[:, :, :1], k, v, pos0=1, lens=[1])[0, 0, :, 0].tolist() == [0.0]           # the query's position is a pad
    assert ref.attn_ref(q, k, v, mutate="drop_diag")[0, 0, :, 0].tolist() == [0.0, 1.0, 1.5]
    assert ref.attn_ref(q, k, v, mutate="leak_future")[0, 0, :, 0].tolist() == [1.5, 2.0, 2.0]
    # KV head = head // (heads // kv_heads)
    q6 = torch.zeros(1, 6, 1, 128, dtype=torch.float64)
    v2 = torch.tensor([10.0, 20.0], dtype=torch.float64)[None, :, None, None].expand(1, 2, 1, 128)
    assert ref.attn_ref(q6, torch.zeros_like(v2), v2)[0, :, 0, 0].tolist() == [10.0, 10.0, 10.0, 20.0, 20.0, 20.0]
    assert ref.attn_ref(q6, torch.zeros_like(v2), v2, mutate="kv_mod")[0, :, 0, 0].tolist() == [10.0, 20.0, 10.0, 20.0, 10.0, 20.0]


def test_row_errors_is_per_row_and_wants_exact_zeros():
    r = torch.zeros(3, 128, dtype=torch.float64)
    r[0, 5], r[1, 7] = 100.0, 0.01
    g = r.clone()
    g[1, 9] = 0.001                                  # 10 % of its own row, 1e-5 of the tensor's largest value
    g[2, 0] = 1e-30
    err, bad = ref.row_errors(g, r)
    assert err.tolist() == [0.0, pytest.approx(0.1), 0.0] and bad.tolist() == [False, False, True]


@pytest.mark.parametrize("case", ALL_ATTN, ids=IDS)
def test_every_wrong_mask_moves_every_row_it_touches(case):
    """For each mutation that changes this case's mask (or head map, or zero rows) at all, every query row it changes differs from the
    true reference by >= 10 x ATTN_TOL of the row's scale (a zero row must become non-zero).  The poisoned K / V are finite."""
    x = ref.build_attn(case)
    for buf in x.bufs.values():
        assert bool(torch.isfinite(buf).all())
    true, vis, zero, hmap = ref.attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens, return_mask=True)
    assert torch.equal(true, ref.attn_expected(case))
    if case.form == "bm":
        assert int(zero[:, 0].sum()) * 2 <= zero[:, 0].numel(), case.name                           # at most half of the rows are zero rows
    changed = 0
    for mut in ref.MUTATIONS:
        out, mvis, mzero, mmap = ref.attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens, mutate=mut, return_mask=True)
        live, mlive = vis & ~zero[..., None], mvis & ~mzero[..., None]                              # what a row attends, nothing for zero rows
        touched = (live != mlive).any(-1) | ((hmap != mmap)[None, :, None] & ~zero)
        if not bool(touched.any()):
            assert torch.equal(out, true), (case.name, mut)
            continue
        changed += 1
        assert torch.equal(out[~touched], true[~touched]), (case.name, mut)
        diff, _ = ref.row_errors(out, true)
        was_zero = zero & touched
        assert bool((out[was_zero].abs().amax(-1) > 10 * ref.ATTN_TOL).all()), (case.name, mut)
        moved = diff[touched & ~zero]
        if moved.numel():
            assert float(moved.min()) >= 10 * ref.ATTN_TOL, (case.name, mut, float(moved.min()))
    assert changed >= (1 if case.tk == 1 else 3), (case.name, changed)


def test_attn_tol_is_three_times_the_emulation_floor():
    """The float64 emulation of the matrix-core kernel's three fp16 roundings, over the whole case list: ATTN_EMU_FLOOR is its worst
    per-row error (to 10 %), and ATTN_TOL lies between 2 x and 4 x the value measured here."""
    worst, where = 0.0, None
    for case in ALL_ATTN:
        x = ref.build_attn(case)
        err, bad = ref.row_errors(ref.attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens, emulate=True), ref.attn_expected(case))
        assert not bool(bad.any()), case.name
        if float(err.max()) > worst:
            worst, where = float(err.max()), case.name
    print(f"[llm-ops] fp16-emulation floor {worst:.3e} at {where}; ATTN_EMU_FLOOR {ref.ATTN_EMU_FLOOR:.3e}, ATTN_TOL {ref.ATTN_TOL:.3e}")
    assert abs(ref.ATTN_EMU_FLOOR - worst) <= 0.1 * worst
    assert 2 * worst <= ref.ATTN_TOL <= 4 * worst


def test_other_operators_references_and_case_sizes():
    """The grid-stride cases exceed their grids, the references agree with torch's own float64 operators, and the bounds are what the
    docstrings derive."""
    b, t, _ = ref.ROPE_CASES[0]
    assert b * t * ref.ROPE_HEADS * 64 > 4096 * 256 and ref.ROPE_EX_CASES[0][0] * ref.ROPE_EX_CASES[0][1] * ref.ROPE_HEADS * 64 > 4096 * 256
    assert ref.SWIGLU_BIG[0] * (ref.SWIGLU_BIG[1] // 8) > 8192 * 256
    g = torch.Generator().manual_seed(0)
    x, w = ref.rms_inputs(66, 5, 1e-4)
    want = torch.nn.functional.rms_norm(x.double(), (66,), w.double(), ref.RMS_EPS)
    assert float((ref.rmsnorm_ref(x, w, ref.RMS_EPS) - want).abs().max()) < 1e-13
    assert float(ref.rmsnorm_ref(x, w, ref.RMS_EPS).abs().min()) > 2.0 ** -14                         # no fp16 subnormal among the outputs
    # rope: rotate-half with emb = cat(freqs, freqs), positions shifted per row and clamped at 0
    cos, sin = ref.rope_tables(16)
    xr = torch.randn(2, 3, 3 * 128, generator=g).half()
    pos = ref.rope_positions(2, 3, 5, False, (0, 7))
    assert pos.tolist() == [[5, 6, 7], [0, 0, 0]] and ref.rope_positions(2, 3, 5, True, (0, 7)).tolist() == [[5, 0], [6, 0], [7, 0]]
    got, bound = ref.rope_ref(xr, cos, sin, 2, 128, pos)
    xh = xr.double()[..., :256].reshape(2, 3, 2, 128)
    c2, s2 = torch.cat([cos, cos], -1).double()[pos][:, :, None], torch.cat([sin, sin], -1).double()[pos][:, :, None]
    want = xh * c2 + torch.cat([-xh[..., 64:], xh[..., :64]], -1) * s2
    assert float((got[..., :256].reshape(2, 3, 2, 128) - want).abs().max()) < 1e-15 and torch.equal(got[..., 256:], xr.double()[..., 256:])
    assert float(bound[..., 256:].abs().max()) == 0.0 and bool((bound[..., :256] >= 2.0 ** -11 * want.reshape(2, 3, 256).abs()).all())
    gu = torch.randn(4, 64, generator=g).half()
    sref, sb = ref.swiglu_ref(gu)
    assert float((sref - torch.nn.functional.silu(gu[:, :32].double()) * gu[:, 32:].double()).abs().max()) < 1e-15
    special, _ = ref.swiglu_ref(torch.tensor([list(ref.SWIGLU_GATES) + [1.0] * 8], dtype=torch.float16))
    assert bool(torch.isfinite(special).all()) and float(special[0, 0]) == 0.0 and float(special[0, 6]) == 65504.0
    xm = torch.randn(2, 9, 5, generator=g)
    mref, mb = ref.mean_pool_ref(xm, (0, 12))
    assert float(mref[0].abs().max()) == 0.0 and float((mref[1] - xm[1].double().mean(0)).abs().max()) < 1e-15
    assert torch.allclose(mb[1], 9 * 2.0 ** -24 * xm[1].double().abs().mean(0)) and {0, 1, ref.MEAN_POOL_T, ref.MEAN_POOL_T + 7} <= set(ref.MEAN_POOL_LENS)
