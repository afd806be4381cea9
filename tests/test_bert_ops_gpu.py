"""The two row operators of the BERT-family encoder on the GPU (include/llm/astts_bert.h, csrc/ops_bert.hip): astts_op_layernorm_dual
against torch.nn.functional.layer_norm in fp32 on the CPU, astts_op_bert_embed_ln against the same computation in torch
(tests/bert_ref.py).

Bounds.  The fp32 output: LN_TOL of tests/synth_elem_ref.py (2e-5 of the largest expected value), the bar astts_op_layernorm is held
to.  The fp16 output: equal, bit for bit, to the fp32 output rounded once.  Offset rows (x = 100 + 0.01 noise, eps = 1e-12) are held to
the same LN_TOL, against layer_norm evaluated in fp64 on the same fp32 inputs: on such rows the fp32 CPU evaluation is itself 1e-4 to
6e-4 away from the exact value (half an ulp of the mean, 4e-6, against a standard deviation of 0.01), which no kernel can follow to
2e-5; its distance to the fp64 evaluation is printed beside the kernel's."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bert_ref as ref  # noqa: E402
from synth_elem_ref import LN_TOL, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12                      # BERT's layer_norm_eps
SENTINEL = -77.0
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
ROWS, WIDTHS = (1, 5, 257), (8, 128, 768, 1024, 1544)       # 1544 = 24 * 64 + 8: no multiple of 64; 257 rows: more than one workgroup


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _case(rows, c, seed, pad=8):
    """x as the first c columns of a [rows, c + pad] buffer (ldx > c), gamma, beta."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, c + pad), SENTINEL)
    buf[:, :c] = torch.randn(rows, c, generator=g) * 3 + 1
    return buf, torch.randn(c, generator=g), torch.randn(c, generator=g)


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_dual_against_torch(rows, c):
    from astts import ops

    buf, ga, be = _case(rows, c, 1000 * c + rows)
    want = F.layer_norm(buf[:, :c], (c,), ga, be, EPS)
    gd, bd = ga.to(DEV), be.to(DEV)
    xb = buf.to(DEV)
    y32, y16 = ops.layernorm_dual(xb[:, :c], gd, bd, EPS)
    err = rel_err(y32, want)
    print(f"layernorm_dual rows={rows} c={c}: fp32 output rel err {err:.3e} (bound {LN_TOL:.1e})")
    assert y32.shape == y16.shape == (rows, c) and y32.dtype == torch.float32 and y16.dtype == torch.float16
    assert err < LN_TOL
    assert torch.equal(_bits(y16), _bits(y32.half())), "the fp16 output is not the fp32 output rounded once"
    assert torch.equal(xb.cpu(), buf), "the input was written to"
    # each output alone: the same bits
    only32, none16 = ops.layernorm_dual(xb[:, :c], gd, bd, EPS, want16=False)
    none32, only16 = ops.layernorm_dual(xb[:, :c], gd, bd, EPS, want32=False)
    assert none16 is None and none32 is None
    assert torch.equal(_bits(only32), _bits(y32)) and torch.equal(_bits(only16), _bits(y16))
    # a second launch: the same bits
    again32, again16 = ops.layernorm_dual(xb[:, :c], gd, bd, EPS)
    assert torch.equal(_bits(again32), _bits(y32)) and torch.equal(_bits(again16), _bits(y16))
    # in place (y32 = x, ldy32 = ldx > c), with and without the fp16 copy: the same bits, the columns beyond c untouched
    for want16 in (True, False):
        xi = buf.to(DEV)
        in32, in16 = ops.layernorm_dual(xi[:, :c], gd, bd, EPS, want16=want16, inplace=True)
        assert in32.data_ptr() == xi.data_ptr()
        assert torch.equal(_bits(xi[:, :c]), _bits(y32)) and bool((xi[:, c:] == SENTINEL).all())
        assert (in16 is None) if not want16 else torch.equal(_bits(in16), _bits(y16))


def test_layernorm_dual_strided_outputs_through_the_c_entry_point():
    """ldy32 = c + 4 and ldy16 = c + 8: rows land at their strides and nothing is written between them."""
    from astts import _lib, _lib_bert

    rows, c = 5, 776
    buf, ga, be = _case(rows, c, 7)
    xd, gd, bd = buf.to(DEV), ga.to(DEV), be.to(DEV)
    o32 = torch.full((rows, c + 4), SENTINEL, device=DEV)
    o16 = torch.full((rows, c + 8), SENTINEL, device=DEV, dtype=torch.float16)
    _lib.check(_lib_bert.load().astts_op_layernorm_dual(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), o32.data_ptr(), o16.data_ptr(), rows, c,
                                                       c + 8, c + 4, c + 8, EPS, _lib.stream_ptr()))
    want = F.layer_norm(buf[:, :c], (c,), ga, be, EPS)
    assert rel_err(o32[:, :c], want) < LN_TOL and torch.equal(_bits(o16[:, :c]), _bits(o32[:, :c].half()))
    assert bool((o32[:, c:] == SENTINEL).all()) and bool((o16[:, c:] == SENTINEL).all())


@pytest.mark.parametrize("c", WIDTHS)
def test_layernorm_dual_offset_rows(c):
    """x = 100 + 0.01 noise with eps = 1e-12: what a one-pass E[x^2] - mean^2 variance fails (and a mean rounded to fp32 misses by 1e-4)."""
    from astts import ops

    g = torch.Generator().manual_seed(c)
    x = 100.0 + 1e-2 * torch.randn(5, c, generator=g)
    ga, be = torch.randn(c, generator=g), torch.randn(c, generator=g)
    want64 = F.layer_norm(x.double(), (c,), ga.double(), be.double(), EPS)
    y32, y16 = ops.layernorm_dual(x.to(DEV), ga.to(DEV), be.to(DEV), EPS)
    err, cpu32 = rel_err(y32, want64), rel_err(F.layer_norm(x, (c,), ga, be, EPS), want64)
    print(f"layernorm_dual offset rows c={c}: rel err vs the fp64 evaluation {err:.3e} (bound {LN_TOL:.1e}); torch's fp32 CPU evaluation: {cpu32:.3e}")
    assert err < LN_TOL
    assert torch.equal(_bits(y16), _bits(y32.half())) and bool(torch.isfinite(y32).all())


@pytest.mark.parametrize("c", WIDTHS)
def test_layernorm_dual_constant_rows_return_beta(c):
    from astts import ops

    g = torch.Generator().manual_seed(c + 1)
    x = torch.tensor([0.1, -7.3, 100.0, 0.0, 3e4])[:, None].expand(5, c).contiguous()
    ga, be = torch.randn(c, generator=g), torch.randn(c, generator=g)
    y32, y16 = ops.layernorm_dual(x.to(DEV), ga.to(DEV), be.to(DEV), EPS)
    assert bool(torch.isfinite(y32).all()) and bool(torch.isfinite(y16).all())
    assert torch.equal(y32.cpu(), be[None, :].expand(5, c)) and torch.equal(_bits(y16), _bits(be.half()[None, :].expand(5, c)))


def test_layernorm_dual_refuses_what_it_is_not_built_for():
    """c = 12 and c = 4104: UNSUPPORTED; a pointer or a stride off 16 bytes, both outputs NULL: INVALID; nothing is launched."""
    from astts import _lib, _lib_bert

    fn = _lib_bert.load().astts_op_layernorm_dual
    x = torch.randn(4, 4112, device=DEV)
    ga, be = torch.ones(4112, device=DEV), torch.zeros(4112, device=DEV)
    o32 = torch.full((4, 4112), SENTINEL, device=DEV)
    o16 = torch.full((4, 4112), SENTINEL, device=DEV, dtype=torch.float16)
    st = _lib.stream_ptr()
    call = lambda c, xp=x.data_ptr(), y32=o32.data_ptr(), y16=o16.data_ptr(), ldx=4112, ld32=4112, ld16=4112: fn(
        xp, ga.data_ptr(), be.data_ptr(), y32, y16, 4, c, ldx, ld32, ld16, EPS, st)
    assert call(12) == ERR_UNSUPPORTED and call(4104) == ERR_UNSUPPORTED and call(0) == ERR_UNSUPPORTED
    assert call(768, xp=x.data_ptr() + 4) == ERR_INVALID                  # x one float into its buffer
    assert call(768, y16=o16.data_ptr() + 2) == ERR_INVALID               # y16 one half into its buffer
    assert call(768, ldx=4110) == ERR_INVALID and call(768, ld16=4116) == ERR_INVALID and call(768, ld32=760) == ERR_INVALID
    assert call(768, y32=None, y16=None) == ERR_INVALID
    torch.cuda.synchronize()
    assert bool((o32 == SENTINEL).all()) and bool((o16 == SENTINEL).all())
    assert call(768) == 0                                                 # and the aligned call goes through
    torch.cuda.synchronize()
    assert bool((o32[:, :768] != SENTINEL).any())


# ------------------------------------------------------------------------------------------------------------ the embedding sum
B, T, LENS, VOCAB, MAX_POS, N_TYPES = 3, 130, (130, 64, 5), 50, 140, 2


def _embed_case(c, seed):
    g = torch.Generator().manual_seed(seed)
    word, pos, typ = torch.randn(VOCAB, c, generator=g), torch.randn(MAX_POS, c, generator=g) * 0.5, torch.randn(N_TYPES, c, generator=g) * 0.5
    ids = torch.randint(0, VOCAB, (B, T), generator=g)
    ids[0, 0], ids[0, 1], ids[2, 4] = 0, VOCAB - 1, VOCAB - 1
    types = torch.randint(0, N_TYPES, (B, T), generator=g)
    return word, pos, typ, ids, types, torch.tensor(LENS), torch.randn(c, generator=g), torch.randn(c, generator=g)


@pytest.mark.parametrize("pos_offset", [0, 2])
@pytest.mark.parametrize("with_types", [True, False])
@pytest.mark.parametrize("c", [128, 776])           # the 16-lane kernel; the wave kernel with a half-filled second chunk
def test_bert_embed_ln_against_torch(c, with_types, pos_offset):
    from astts import ops

    word, pos, typ, ids, types, lens, ga, be = _embed_case(c, 10 * c + pos_offset)
    want = ref.embed_ln(word, pos, typ, ids, types if with_types else None, lens, ga, be, pos_offset, EPS)
    d = lambda t, dt=None: t.to(DEV) if dt is None else t.to(DEV, dt)
    args = (d(word), d(pos), d(typ), d(ids, torch.int32), d(types, torch.int32) if with_types else None, d(lens, torch.int32), d(ga), d(be), pos_offset, EPS)
    o32, o16 = ops.bert_embed_ln(*args)
    assert o32.shape == o16.shape == (B, T, c)
    for i, n in enumerate(LENS):
        err = rel_err(o32[i, :n], want[i, :n])
        print(f"bert_embed_ln c={c} types={with_types} pos_offset={pos_offset} row {i}: rel err {err:.3e} (bound {LN_TOL:.1e})")
        assert err < LN_TOL
        assert float(o32[i, n:].abs().sum()) == 0.0 and float(o16[i, n:].float().abs().sum()) == 0.0        # padding rows are zeros
    assert torch.equal(_bits(o16), _bits(o32.half()))
    a32, a16 = ops.bert_embed_ln(*args)
    assert torch.equal(_bits(a32), _bits(o32)) and torch.equal(_bits(a16), _bits(o16))
    only32, _ = ops.bert_embed_ln(*args, want16=False)
    _, only16 = ops.bert_embed_ln(*args, want32=False)
    assert torch.equal(_bits(only32), _bits(o32)) and torch.equal(_bits(only16), _bits(o16))
    no_lens32, _ = ops.bert_embed_ln(*args[:5], None, *args[6:])                                         # lens NULL: every row is full
    full = ref.embed_ln(word, pos, typ, ids, types if with_types else None, torch.tensor([T] * B), ga, be, pos_offset, EPS)
    assert rel_err(no_lens32, full) < LN_TOL


def test_bert_embed_ln_clamps_indices_into_the_tables():
    """An id or a type id one outside its table reads the table's nearest row, never beyond it."""
    from astts import ops

    c = 128
    word, pos, typ, ids, types, lens, ga, be = _embed_case(c, 3)
    bad_ids, bad_types = ids.clone(), types.clone()
    bad_ids[1, 3], bad_ids[1, 4], bad_types[1, 5], bad_types[1, 6] = -1, VOCAB, -1, N_TYPES
    ids[1, 3], ids[1, 4], types[1, 5], types[1, 6] = 0, VOCAB - 1, 0, N_TYPES - 1
    d = lambda t, dt=None: t.to(DEV) if dt is None else t.to(DEV, dt)
    run = lambda i, ty: ops.bert_embed_ln(d(word), d(pos), d(typ), d(i, torch.int32), d(ty, torch.int32), d(lens, torch.int32), d(ga), d(be), 0, EPS)[0]
    assert torch.equal(_bits(run(bad_ids, bad_types)), _bits(run(ids, types)))


def test_bert_embed_ln_refuses_what_it_is_not_built_for():
    from astts import _lib, _lib_bert

    fn = _lib_bert.load().astts_op_bert_embed_ln
    c = 16
    tab = torch.randn(8, c + 4, device=DEV)
    ids = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    ga, be = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    out = torch.full((4, c), SENTINEL, device=DEV)
    call = lambda cc, wp: fn(wp, tab.data_ptr(), tab.data_ptr(), ids.data_ptr(), None, None, ga.data_ptr(), be.data_ptr(), out.data_ptr(), None,
                             1, 4, cc, 8, 8, 8, 0, EPS, _lib.stream_ptr())
    assert call(12, tab.data_ptr()) == ERR_UNSUPPORTED and call(4104, tab.data_ptr()) == ERR_UNSUPPORTED
    assert call(c, tab.data_ptr() + 4) == ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
