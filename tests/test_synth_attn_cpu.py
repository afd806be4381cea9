"""CPU side of the synthesis attention suite (tests/synth_attn_ref.py): the float64 reference against torch's
scaled_dot_product_attention, a three-loop statement of the relative-position definition and rows done by hand; the case lists against
the kernels' tile, pass and mask edges; the sensitivity of every case's inputs to every wrong variant (a touched row moves by
>= MUTATION_FACTOR x the bound of the kernels that run the case, an untouched row keeps its bits); the cap on rows that are not judged;
and both bounds against the floors measured here.  Nothing here needs a GPU or the native library."""
import functools

import pytest
import torch

import synth_attn_ref as ref

LISTS = {"mha": ref.MHA_CASES, "prefill": ref.PREFILL_CASES, "decode": ref.DECODE_CASES, "rows": ref.ROWS_CASES}


def test_case_lists_cover_the_tile_pass_and_mask_edges():
    names = [c.name for c in ref.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in ref.ALL_CASES:
        assert ref.center_of(c) >= c.tk + 80 and ref.center_of(c) >= c.pos0 + c.tq + 16, c.name
        assert c.h == (4 if c in ref.ROWS_CASES else 2)
    # attn_mha_flash: the prefetch edges (64, 128, 192, ...), the 32-key mask edges, a row without keys, a clamped lens
    assert ref.MHA_T == (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385)
    mha = ref.MHA_CASES
    for t in ref.MHA_T:
        assert {c.lens for c in mha if c.tq == t} >= {(t, 1), (t, t - 1)}, t
    lens257 = [c.lens for c in mha if c.tq == 257]
    assert (257, 192, 128, 64) in lens257 and any(ln[-4:] == (257, 129, 65, 33) for ln in lens257)
    assert any(0 in c.lens and c.tq > 1 for c in mha) and any(c.tq + 5 in c.lens for c in mha)
    assert all(c.b <= 5 and not c.causal and c.form == "bm" for c in mha)
    # prefill: one list for both kernels
    pre = ref.PREFILL_CASES
    assert all(c.tq >= 2 and c.b <= 4 for c in pre)
    for causal in (False, True):
        for t in (2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257):
            assert {c.lens for c in pre if c.form == "bm" and c.causal == causal and c.tq == t} >= {(t, 1), (t, t - 1)}, (causal, t)
    gen = [c for c in pre if c.form == "tm"]
    assert {(c.tq, c.tk) for c in gen} >= {(3, 65), (3, 77), (17, 80), (33, 200), (40, 73), (130, 333), (260, 391)}
    assert {s for c in gen for s in c.key_start} >= set(ref.KEY_START_SET)
    for c in gen:
        assert c.causal and all(0 <= s <= c.tk - 1 for s in c.key_start) and c.pos0 + c.tq <= c.tk
        if c.lens is None:
            assert c.pos0 == c.tk - c.tq and c.pos0 + c.tq - 1 in c.key_start, c.name                 # one visible key for the last query
            assert any(c.pos0 < s < c.pos0 + c.tq - 1 for s in c.key_start), c.name                   # pad queries in a live row
    assert any(c.lens is not None and c.pos0 > 0 and any(c.key_start) and c.pos0 + c.tq < c.tk for c in gen)
    assert {s // 64 * 64 for c in gen for s in c.key_start} >= {0, 64, 128, 192}                       # tile skipping (jstart)
    assert any((c.tq, c.tk) == (130, 333) for c in ref.PREFILL_MIXED) and set(ref.PREFILL_MIXED) <= set(pre)
    # decode: the 256-key pass (DG * DK), both forms, with and without lens
    dec = ref.DECODE_CASES
    assert all(c.tq == 1 and c.b <= 32 and c.causal for c in dec)
    for form in ("tm", "bm"):
        for with_lens in (False, True):
            mine = [c for c in dec if c.form == form and (c.lens is not None) == with_lens and c.tk == c.pos0 + 1]
            assert {c.tk for c in mine} >= {1, 2, 64, 255, 256, 257, 511, 512, 513}, (form, with_lens)
            for c in mine:
                assert set(c.key_start) == {min(s, c.tk - 1) for s in (0, 1, 31, 32, 33, 255, 256, c.tk - 1)}, c.name
    # rows: 16 key slots, 64 keys per pass
    rows = ref.ROWS_CASES
    for b in (33, 40):
        assert {c.tk for c in rows if c.b == b and c.tk == c.pos0 + 1} >= {1, 5, 63, 64, 65, 127, 128, 129, 333}
    for c in rows:
        assert c.tq == 1 and c.b > 32 and c.key_start[0] == 0
        if c.tk == c.pos0 + 1:
            assert c.key_start[-1] == c.tk - 1
    # the tq = 1 kernels clamp key_start to len - 1: this suite keeps below that
    for c in dec + rows:
        ln = c.lens if c.lens is not None else (min(c.tk, c.pos0 + 1),) * c.b
        assert all(s <= n - 1 and s <= c.pos0 for s, n in zip(c.key_start, ln)), c.name
    # causal at tq = 1 with keys after the query, on both kernels
    for cases in (dec, rows):
        assert any(c.lens is None and c.tk == c.pos0 + ref.DECODE_CAUSAL_GAP for c in cases)


def _full_rows(case):
    return [i for i in range(case.b) if case.lens[i] >= case.tk]


@pytest.mark.parametrize("case", ref.MHA_CASES, ids=[c.name for c in ref.MHA_CASES])
def test_reference_equals_torch_sdpa_on_unpadded_mha_rows(case):
    x = ref.build(case)
    for i in _full_rows(case):
        want = torch.nn.functional.scaled_dot_product_attention(x.q[i:i + 1], x.k[i:i + 1], x.v[i:i + 1])
        err, bad = ref.row_errors(ref.expected(case)[i:i + 1], want)
        assert float(err.max()) < 1e-12 and not bool(bad.any()), (case.name, i, float(err.max()))


def _three_loops(x, i_b):
    """The definition, one (head, query, key) at a time, for an unpadded batch row."""
    c = x.case
    out = torch.zeros(c.h, c.tq, ref.DH, dtype=torch.float64)
    for h in range(c.h):
        u, v = x.bias_u[h * 64:(h + 1) * 64], x.bias_v[h * 64:(h + 1) * 64]
        for i in range(c.tq):
            s = []
            for j in range(c.tk):
                p = x.table[c.pos0 + i - j + x.center, h * 64:(h + 1) * 64]
                s.append(float(((x.q[i_b, h, i] + u) @ x.k[i_b, h, j] + (x.q[i_b, h, i] + v) @ p) / 8.0))
            s = torch.tensor(s, dtype=torch.float64)
            if c.causal:
                s[torch.arange(c.tk) > c.pos0 + i] = float("-inf")
            out[h, i] = torch.softmax(s, 0) @ x.v[i_b, h, :c.tk]
    return out


def test_relpos_reference_equals_the_three_loop_definition_on_unpadded_rows():
    tiny = [c for c in ref.PREFILL_CASES if c.form == "bm" and c.tq in (2, 15, 17)] + [
        c for c in ref.PREFILL_CASES if (c.tq, c.tk) == (3, 65)] + [c for c in ref.DECODE_CASES if c.tk in (2, 64) and c.lens is None]
    checked = 0
    for c in tiny:
        x = ref.build(c)
        for i in range(c.b):
            if (c.lens is None or c.lens[i] >= c.tk) and (c.key_start is None or c.key_start[i] == 0):
                err, bad = ref.row_errors(ref.expected(c)[i], _three_loops(x, i))
                assert float(err.max()) < 1e-12 and not bool(bad.any()), (c.name, i, float(err.max()))
                checked += 1
    assert checked >= 12


def test_reference_on_rows_done_by_hand():
    """Identical scores: the output is the mean of the visible values, so the masks show as the keys they name.  Then a table that adds
    ln 3 to the score at relative position +1 only: the previous key weighs three times the others."""
    z = torch.zeros(1, 1, 3, 64, dtype=torch.float64)
    v = torch.arange(3, dtype=torch.float64)[None, None, :, None].expand(1, 1, 3, 64) + 1.0          # values 1, 2, 3
    col = lambda o: o[0, 0, :, 0].tolist()
    assert col(ref.attn_ref(z, z, v)) == [2.0, 2.0, 2.0]
    assert col(ref.attn_ref(z, z, v, lens=[2])) == [1.5, 1.5, 1.5]
    assert col(ref.attn_ref(z, z, v, lens=[0])) == [0.0, 0.0, 0.0]
    assert col(ref.attn_ref(z, z, v, lens=[2], mutate="lens_plus")) == [2.0, 2.0, 2.0]
    center = 100
    table, bias = torch.zeros(2 * center + 1, 64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    kw = dict(table=table, bias_u=bias, bias_v=bias, center=center)
    assert col(ref.attn_ref(z, z, v, causal=True, **kw)) == [1.0, 1.5, 2.0]
    assert col(ref.attn_ref(z, z, v, causal=True, key_start=[1], **kw)) == [0.0, 2.0, 2.5]
    assert col(ref.attn_ref(z, z, v, causal=True, lens=[2], **kw)) == [1.0, 1.5, 1.5]                 # a query past lens sees the valid keys
    assert col(ref.attn_ref(z[:, :, :1], z, v, causal=True, pos0=1, **kw)) == [1.5]
    assert col(ref.attn_ref(z[:, :, :1], z, v, causal=True, pos0=1, mutate="decode_not_causal", **kw)) == [2.0]
    assert col(ref.attn_ref(z, z, v, causal=True, mutate="drop_diag", **kw)) == [0.0, 1.0, 1.5]
    assert col(ref.attn_ref(z, z, v, causal=True, mutate="leak_future", **kw)) == [1.5, 2.0, 2.0]
    assert col(ref.attn_ref(z, z, v, causal=True, key_start=[1], mutate="kstart_minus", **kw)) == [1.0, 1.5, 2.0]
    assert col(ref.attn_ref(z, z, v, causal=True, key_start=[1], mutate="pad_nonzero", **kw)) == [1.0, 2.0, 2.5]
    # (q + v) . p: v = 8 ln 3 on dim 0, the table row of relative position +1 is e_0 -> score ln 3 for the previous key
    bias_v = torch.zeros(64, dtype=torch.float64)
    bias_v[0] = 8.0 * torch.log(torch.tensor(3.0, dtype=torch.float64))
    table[center + 1, 0] = 1.0
    kw = dict(table=table, bias_u=bias, bias_v=bias_v, center=center)
    got = col(ref.attn_ref(z, z, v, **kw))
    want = [2.0, (3 * 1 + 2 + 3) / 5.0, (1 + 3 * 2 + 3) / 5.0]
    assert max(abs(a - b) for a, b in zip(got, want)) < 1e-14
    got = col(ref.attn_ref(z, z, v, mutate="rel_plus", **kw))                                          # now rel 0 reads the row: the diagonal
    want = [(3 * 1 + 2 + 3) / 5.0, (1 + 3 * 2 + 3) / 5.0, (1 + 2 + 3 * 3) / 5.0]
    assert max(abs(a - b) for a, b in zip(got, want)) < 1e-14
    assert col(ref.attn_ref(z, z, v, mutate="no_pos", **kw)) == [2.0, 2.0, 2.0]
    assert col(ref.attn_ref(z, z, v, mutate="swap_uv", **kw)) == [2.0, 2.0, 2.0]                       # u = 0 meets the table, v meets k = 0


def test_row_errors_is_per_row_and_wants_exact_zeros():
    r = torch.zeros(3, 64, dtype=torch.float64)
    r[0, 5], r[1, 7] = 100.0, 0.01
    g = r.clone()
    g[1, 9] = 0.001                                  # 10 % of its own row, 1e-5 of the tensor's largest value
    g[2, 0] = 1e-30
    err, bad = ref.row_errors(g, r)
    assert err.tolist() == [0.0, pytest.approx(0.1), 0.0] and bad.tolist() == [False, False, True]


def test_the_valu_layout_and_the_dont_care_rows():
    x = ref.build(ref.PREFILL_BM[3])
    hd = x.case.h * 64
    for form_case in (ref.PREFILL_BM[3], ref.PREFILL_TM[0]):
        x = ref.build(form_case)
        bufs = ref.relpos_buffers(x, torch.float16, torch.float32, pad=ref.VALU_PAD)
        kv = bufs["kv"]
        k = kv[..., :hd]
        ldk, k_bs = (k.stride(1), k.stride(0)) if form_case.form == "bm" else (k.stride(0), k.stride(1))
        assert ldk % 8 == 4 or k_bs % 8 == 4
        assert ref.expected_kernel(form_case.tq, form_case.b, 2, True, False, 0, 0, 0, 0, ldk, hd, k_bs, hd) == "attn_relpos"
        assert ref.expected_kernel(form_case.tq, form_case.b, 2, True, False, 0, 0, 0, 0, 2 * hd, hd, 2 * hd, hd) == "attn_relpos_mfma"
        back = k.transpose(0, 1) if form_case.form == "tm" else k
        assert torch.equal(back.double(), ref.heads_last(x.k))                                         # fp16 holds the values exactly
    assert ref.expected_kernel(1, 33, 4, True, True, 0, 0, 0, 0, 512, 256, 512, 256) == "attn_relpos_rows"
    assert ref.expected_kernel(1, 32, 4, True, True, 0, 0, 0, 0, 512, 256, 512, 256) == "attn_relpos_decode"
    assert ref.expected_kernel(1, 33, 4, True, False, 0, 0, 0, 0, 512, 256, 512, 256) == "attn_relpos_decode"
    c = next(c for c in ref.PREFILL_BM if not c.causal and c.lens == (33, 1))
    dc = ref.dont_care(c)
    assert int(dc[0].sum()) == 0 and dc[1].tolist() == [False] + [True] * 32
    assert not bool(ref.dont_care(next(c for c in ref.PREFILL_BM if c.causal and c.lens == (33, 1))).any())
    zc = next(c for c in ref.MHA_CASES if 0 in c.lens and c.tq > 1)                                     # a row without keys: zero rows, judged
    assert not bool(ref.dont_care(zc)[1].any()) and float(ref.expected(zc)[1].abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def _sweep(which):
    """Every case of a list against every mutation -> (mutations that changed a case, failures)."""
    changed, failed = set(), []
    for case in LISTS[which]:
        x = ref.build(case)
        for t in x[1:7]:
            assert t is None or bool(torch.isfinite(t).all()), case.name
        true = ref.ref_of(x, return_mask=True)
        assert torch.equal(true.out, ref.expected(case))
        idle = int(true.zero.sum()) + int(ref.dont_care(case).sum())
        assert 2 * idle <= case.b * case.tq, (case.name, idle)                                          # at most half of the rows are not judged
        shape = (case.b, case.h, case.tq)
        nvis = (true.att > 0).sum(-1) if case.op == "relpos" else true.att.sum(-1)
        zero = true.zero[:, None, :].expand(shape)
        for mut in ref.MUTATIONS:
            if case.op == "mha" and mut in ref.SCORE_MUTATIONS:
                continue
            r = ref.ref_of(x, mutate=mut, return_mask=True)
            if mut in ref.SCORE_MUTATIONS:
                touched = nvis >= 2
            else:
                touched = (r.att != true.att).any(-1) | (r.zero != true.zero)
            touched = touched[:, None, :].expand(shape)
            if not bool(touched.any()):
                if not torch.equal(r.out, true.out):
                    failed.append((case.name, mut, "changed without touching a row"))
                continue
            changed.add(mut)
            if not torch.equal(r.out[~touched], true.out[~touched]):
                failed.append((case.name, mut, "an untouched row changed"))
            need = ref.MUTATION_FACTOR[mut] * ref.bound_of(case)
            diff, _ = ref.row_errors(r.out, true.out)
            was_zero = zero & touched
            if bool(was_zero.any()) and not bool((r.out[was_zero].abs().amax(-1) > need).all()):
                failed.append((case.name, mut, "a zero row stayed (nearly) zero"))
            moved = diff[touched & ~zero]
            if moved.numel() and not float(moved.min()) >= need:
                failed.append((case.name, mut, f"a touched row moved by {float(moved.min()):.2e} < {need:.2e}"))
    return frozenset(changed), tuple(failed)


@pytest.mark.parametrize("which", sorted(LISTS))
def test_every_wrong_variant_moves_every_row_it_touches(which):
    """For each mutation that changes a case at all: untouched rows keep their bits (a score mutation touches the rows with at least two
    visible keys: a row with one key cannot change), and every touched row differs from the true reference by
    >= MUTATION_FACTOR x the bound of the kernels that run the case (a zero row must become that large).  Every buffer is finite, and
    zero rows plus don't-care rows are at most half of a case's rows."""
    changed, failed = _sweep(which)
    assert not failed, failed[:20]


def test_every_mutation_changes_some_case_and_no_factor_is_below_four():
    changed = set().union(*(_sweep(which)[0] for which in LISTS))
    assert changed == set(ref.MUTATIONS), set(ref.MUTATIONS) - changed
    assert set(ref.MUTATION_FACTOR) == set(ref.MUTATIONS) and all(4.0 <= f <= 10.0 for f in ref.MUTATION_FACTOR.values())


def test_bounds_follow_the_measured_floors():
    """MFMA_EMU_FLOOR is the worst per-row error of the fp16 emulation over MHA_CASES (fp16 output) and PREFILL_CASES (to 10 %), and
    MFMA_TOL lies between 2 x and 4 x the value measured here; F32_FLOOR is the worst per-row error of the two float32 evaluations over
    PREFILL_CASES, DECODE_CASES and ROWS_CASES (to 10 %), F32_TOL = 8 x it and at most 1e-4."""
    worst, where = 0.0, None
    for case in ref.MHA_CASES + ref.PREFILL_CASES:
        err, bad = ref.row_errors(ref.ref_of(ref.build(case), emulate=True, out_f16=case.op == "mha"), ref.expected(case))
        assert not bool(bad.any()), case.name
        e = float(err[ref.judged(case)].max())
        if e > worst:
            worst, where = e, case.name
    worst32, where32 = 0.0, None
    for case in ref.PREFILL_CASES + ref.DECODE_CASES + ref.ROWS_CASES:
        for way in ("forward", "slots"):
            err, bad = ref.row_errors(ref.attn_f32(ref.build(case), way), ref.expected(case))
            assert not bool(bad.any()), (case.name, way)
            e = float(err[ref.judged(case)].max())
            if e > worst32:
                worst32, where32 = e, (case.name, way)
    print(f"[synth-attn] fp16-emulation floor {worst:.3e} at {where}; MFMA_EMU_FLOOR {ref.MFMA_EMU_FLOOR:.3e}, MFMA_TOL {ref.MFMA_TOL:.3e}")
    print(f"[synth-attn] float32 floor {worst32:.3e} at {where32}; F32_FLOOR {ref.F32_FLOOR:.3e}, F32_TOL {ref.F32_TOL:.3e}")
    assert abs(ref.MFMA_EMU_FLOOR - worst) <= 0.1 * worst and 2 * worst <= ref.MFMA_TOL <= 4 * worst
    assert ref.MFMA_TOL == 3 * ref.MFMA_EMU_FLOOR
    assert abs(ref.F32_FLOOR - worst32) <= 0.1 * worst32 and ref.F32_TOL == 8 * ref.F32_FLOOR and ref.F32_TOL <= 1e-4
