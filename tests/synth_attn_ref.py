"""Float64 statement of the synthesis path's attention operators (csrc/ops_attention.hip, head dim 64): attn_mha_flash, and the
relative-position attention run by attn_relpos_mfma, attn_relpos, attn_relpos_decode and attn_relpos_rows; with the wrong variants
(`mutate=`), the case lists at the kernels' tile, mask and position edges, the input builders and the bounds.
tests/test_synth_attn_cpu.py proves the reference and the sensitivity of the cases without a GPU; tests/test_synth_attn_gpu.py runs the
kernels.  Nothing here is taken from a kernel's output.

Definition.  q [B, H, Tq, 64], k / v [B, H, Tk, 64]; relpos adds a table [2 center + 1, H 64], bias_u, bias_v [H 64], pos0, causal,
lens, key_start:
    score(i, j) = ((q_i + u) . k_j + (q_i + v) . table[pos0 + i - j + center]) / 8            (MHA: q_i . k_j / 8)
    key j is visible to query i of batch row b  iff  key_start[b] <= j < min(lens[b], Tk)  and, when causal,  j <= pos0 + i
A query with no visible key gives an exact zero row.  Query rows i >= lens[b] of the non-causal batch-major forms are computed by the
kernels and consumed by nobody (`dont_care`): they must be finite and are left out of the error.  The error is taken per (batch row,
head, query): max |got - ref| over the 64 dims / max |ref| of that row (`row_errors`).

Inputs (`build`).  One poison direction w per case; head h uses (-1)^h w, and 63 orthonormal directions orthogonal to it (rows 1 .. 63
of the 64 x 64 Hadamard matrix reflected by the Householder map that takes row 0 to w).  Key j carries ALPHA x one of 61 of them in
turn, the sign changing with every turn (a boost along a key's direction also reaches the key's aliases 61 k positions away; with the
sign every second alias is pushed down instead); a row's first and last valid key carry the two remaining directions and so have no
alias.  A query gets BOOST_DIAG (score + 5) along the keys before, on and after its diagonal (causal forms; a query past lens: the last
two valid keys), or along key first + 7 i mod n_valid and its neighbour (non-causal forms), and BOOST_EDGE (score + 6) along the row's
first and last valid key.  So every query has two adjacent keys of equal weight, and one key of a mask edge carries a share of the
softmax that the bound cannot hide.  Every key no query may see (left pads, right pads, cache rows past tk) is poisoned:
K = POISON_K w, which every query has a component BETA along (score ~ +190 and more), V = +-POISON_V; both finite.
The position table is N(0, SIGMA^2) plus (-1)^r TABLE_ALT w in row r, the biases are +-BIAS_W w plus N(0, BIAS_STD^2): the position
term of a key is then +-(BETA - BIAS_W) TABLE_ALT / 8 = +-0.375 by the parity of i - j, plus noise.  A table row off by one, a missing
position term, swapped biases (BETA + BIAS_W instead of BETA - BIAS_W) or another head's columns (the opposite sign) each move the
score between the two adjacent keys of a query by >= 0.75, which a random table alone does not promise for every row: with a purely
random table (std 0.3) and random biases, rows of two or three keys moved by less than 1e-3 under rel_plus, no_pos and swap_uv.
The noise (NOISE, SIGMA, BIAS_STD) is small for the same reason: at NOISE 0.25 the product of k's noise with q's boosts alone
scattered the scores by 0.3 and hid a dropped diagonal key (1.6e-2 of the row against a need of 3.5e-2).
Every value is fp16-representable, so the reference reads what the kernels read.

Bounds (measured by tests/test_synth_attn_cpu.py, which holds the constants to the measurement):
  matrix-core kernels (attn_mha_flash, attn_relpos_mfma): `attn_ref(..., emulate=True)` rounds q * scale * log2(e) (relpos:
    (q + u) sc and (q + v) sc), p (relative to the row's maximum) and an fp16 output to fp16.  Worst per-row error of that emulation
    over MHA_CASES (fp16 output) and PREFILL_CASES: MFMA_EMU_FLOOR; MFMA_TOL = 3 x the floor.  The margin is for the fp32 accumulation
    order and the hardware exp2, both below the roundings emulated.
  fp32 kernels (attn_relpos, attn_relpos_decode, attn_relpos_rows): the definition evaluated in float32 with the keys summed forward,
    and in 16 interleaved key slots merged flash-style (`attn_f32`).  Worst per-row error of either against float64 over PREFILL_CASES,
    DECODE_CASES and ROWS_CASES: F32_FLOOR; F32_TOL = 8 x the floor (the factor covers __expf, whose error grows with |argument|).
    F32_TOL is below 1e-4, the bar of tests/test_ops_gpu.py::test_attn_relpos_decode_matches_prefill_row.
Measured (CPU): fp16-emulation floor 1.152e-3 -> MFMA_EMU_FLOOR 1.15e-3, MFMA_TOL 3.45e-3; float32 floor 2.37e-6 -> F32_FLOOR 2.4e-6,
F32_TOL 1.92e-5.  Worst per-row error the kernels showed on one MI355X: attn_mha_flash 9.15e-4, attn_relpos_mfma 1.05e-3 (bound
3.45e-3); attn_relpos 2.91e-6, attn_relpos_decode 7.93e-7, attn_relpos_rows 7.86e-7 (bound 1.92e-5).  See EXPERIMENTS.md, section T."""
import functools
import math
import zlib
from collections import namedtuple

import torch

DH = 64
NCYC = DH - 3                         # key directions used in turn (63 are orthogonal to the poison direction; two are kept apart)
SCALE = 1.0 / math.sqrt(DH)
LOG2E = 1.44269504088896341
ALPHA = math.sqrt(4.0 / SCALE)        # |direction| of a key: a query with c ALPHA along it scores 4 c above the rest
BOOST_DIAG = 5.0                      # score boost of the keys around the diagonal (or of the key assigned to a non-causal query)
BOOST_EDGE = 6.0                      # score boost of a row's first and last valid key
BETA = 3.0                            # every query's component along its head's poison direction
POISON_K = 512.0                      # a leaked pad key scores BETA * POISON_K * SCALE = 192 above everything else
POISON_V = 30000.0
NOISE = 0.05                          # std of the random part of q and k
SIGMA = 0.05                          # std of the position table
TABLE_ALT = 2.0                       # table row r also carries (-1)^r TABLE_ALT w
BIAS_W = 1.5                          # bias_u = +BIAS_W w + noise, bias_v = -BIAS_W w + noise
BIAS_STD = 0.15                       # std of that noise
EXTRA_ROWS = 70                       # poisoned cache rows past tk (time-major and decode buffers)
VALU_PAD = 4                          # extra columns of the K|V buffer that sends a prefill case to attn_relpos

MFMA_EMU_FLOOR = 1.15e-3              # measured by test_synth_attn_cpu.py::test_bounds_follow_the_measured_floors: 1.152e-3
MFMA_TOL = 3 * MFMA_EMU_FLOOR         # 3.45e-3
F32_FLOOR = 2.4e-6                    # measured there too: 2.37e-6
F32_TOL = 8 * F32_FLOOR               # 1.92e-5

MASK_MUTATIONS = ("drop_diag", "leak_future", "kstart_minus", "kstart_plus", "lens_minus", "lens_plus", "drop_first32", "drop_last_sub",
                  "tile_swap", "pad_nonzero", "decode_not_causal")
SCORE_MUTATIONS = ("rel_plus", "rel_minus", "swap_uv", "no_pos", "pos_head_shift")
MUTATIONS = MASK_MUTATIONS + SCORE_MUTATIONS
# least distance of a touched row from the true reference, in units of the bound of the kernels that run the case
MUTATION_FACTOR = {m: 10.0 for m in MUTATIONS}

Case = namedtuple("Case", "name op form h b tq tk pos0 causal lens key_start")


def _j(x):
    return "_".join(map(str, x))


def _mha(t, lens, h=2):
    return Case(f"mha-t{t}-l{_j(lens)}", "mha", "bm", h, len(lens), t, t, 0, False, tuple(lens), None)


def _bm(t, lens, causal, h=2):
    return Case(f"bm-{'c' if causal else 'n'}-t{t}-l{_j(lens)}", "relpos", "bm", h, len(lens), t, t, 0, causal, tuple(lens), None)


def _tm(tq, tk, ks, lens=None, pos0=None, h=2, causal=True, tag="tm"):
    pos0 = tk - tq if pos0 is None else pos0
    many = len(ks) > 4                           # decode batches: the limits are a fixed function of (b, tk), not spelt out in the name
    name = f"{tag}-h{h}-q{tq}-k{tk}-p{pos0}-" + (f"b{len(ks)}" if many else f"s{_j(ks)}") + (
        "" if lens is None else "-lens" if many else f"-l{_j(lens)}")
    return Case(name, "relpos", "tm", h, len(ks), tq, tk, pos0, causal, None if lens is None else tuple(lens), tuple(ks))


MHA_T = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385)
MHA_LENS_257 = ((257, 192, 128, 64), (257, 129, 65, 33))
# the second list of lens leaves 544 of its 1028 query rows beyond lens; a fifth, full row in front keeps the case under the cap on
# rows that are not judged (zero + don't-care rows <= half) without dropping one of the lens
MHA_CASES = tuple(_mha(t, ln) for t in MHA_T for ln in ((t, 1), (t, t - 1))) + (
    _mha(257, MHA_LENS_257[0]), _mha(257, (257,) + MHA_LENS_257[1]),
    _mha(130, (130, 0, 97)),                      # a row without keys: no prefetch, no loop, zeros
    _mha(70, (75, 70, 69)),                       # lens = t + 5 is clamped to t
)

PREFILL_T = (2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
PREFILL_BM = tuple(dict.fromkeys(_bm(t, ln, causal) for causal in (False, True) for t in PREFILL_T for ln in ((t, 1), (t, t - 1))))
KEY_START_SET = (0, 1, 63, 64, 65, 127, 128, 200)
# generation form: causal, time-major, pos0 = tk - tq; key_start per batch row from KEY_START_SET, pos0 + tq - 1 (one visible key for
# the last query) and one value above pos0 (pad queries in a live row: zero rows)
_GEN = (
    (3, 65, (0, 32, 64, 63)),                     # pos0 = 62: the second query sits on the last key of a sub-tile
    (3, 77, (0, 63, 76, 75)),
    (17, 80, (0, 1, 79, 65)),                     # pos0 = 63: two 16-query blocks of the VALU kernel, the second one query long
    (33, 200, (1, 128, 199, 180)),
    (40, 73, (0, 1, 72, 50)),                     # pos0 = 33: a wave's last query sits on the first key of a 32-key sub-tile
    (130, 333, (64, 200, 332, 270)),
    (260, 391, (65, 127, 390, 200)),              # three query blocks of the matrix-core kernel, pos0 = 131
)
PREFILL_TM = tuple(_tm(tq, tk, ks) for (tq, tk, ks) in _GEN) + (
    # lens and key_start together at pos0 > 0 with pos0 + tq < tk: the cache holds more than the block attends
    _tm(70, 300, (0, 64, 130, 200), lens=(300, 256, 230, 201), pos0=200),)
PREFILL_CASES = PREFILL_BM + PREFILL_TM
# all four K/V x table dtype instantiations run on these; fp32/fp32 and fp16/fp16 on everything
PREFILL_MIXED = tuple(c for c in PREFILL_CASES if (c.tq, c.tk) in ((130, 333), (3, 65), (70, 300)) or (c.form == "bm" and c.tq in (33, 129)))

DECODE_TK = (1, 2, 64, 255, 256, 257, 511, 512, 513)
DECODE_KEY_START = (0, 1, 31, 32, 33, 255, 256)   # and tk - 1; all clipped to <= tk - 1
_DECODE_SHORT = (0, 1, 0, 2, 0, 1, 3, 0)          # lens = tk - this (never below key_start + 1)


def _decode(tk, form, with_lens, h=2):
    ks = tuple(min(s, tk - 1) for s in DECODE_KEY_START + (tk - 1,))
    lens = tuple(max(s + 1, tk - d) for s, d in zip(ks, _DECODE_SHORT)) if with_lens else None
    c = _tm(1, tk, ks, lens=lens, h=h, tag="dec-" + form)
    return c._replace(form=form)


DECODE_CAUSAL_GAP = 40                            # tq = 1, causal, no lens, tk = pos0 + 40: keys after the query must stay unseen
DECODE_CASES = tuple(_decode(tk, form, wl) for tk in DECODE_TK for form in ("tm", "bm") for wl in (False, True)) + tuple(
    _tm(1, 260 + DECODE_CAUSAL_GAP, (0, 1, 33, 255, 256, 260, 64, 200), pos0=260, tag="dec-" + form + "-gap")._replace(form=form)
    for form in ("tm", "bm"))

ROWS_TK = (1, 5, 63, 64, 65, 127, 128, 129, 333)
ROWS_B = (33, 40)


def _rows(b, tk, with_lens):
    pool = DECODE_KEY_START + KEY_START_SET
    ks = tuple(0 if r == 0 else tk - 1 if r == b - 1 else min(pool[r % len(pool)], tk - 1) for r in range(b))
    lens = tuple(max(s + 1, tk - _DECODE_SHORT[r % 8]) for r, s in enumerate(ks)) if with_lens else None
    return _tm(1, tk, ks, lens=lens, h=4, tag=f"rows{b}")


# 33 rows without lens, 40 rows with; and the causal gap case
ROWS_CASES = tuple(_rows(b, tk, b == 40) for b in ROWS_B for tk in ROWS_TK) + (
    _tm(1, 130 + DECODE_CAUSAL_GAP, tuple([0, 1, 63, 64, 65, 127, 128, 130] * 4 + [0]), pos0=130, h=4, tag="rows33-gap"),)

ALL_CASES = MHA_CASES + PREFILL_CASES + DECODE_CASES + ROWS_CASES


def center_of(case):
    """The table centre of a case: the smallest the host checks of the prefill path accept for it."""
    return max(case.tk + 80, case.pos0 + case.tq + 16)


def bound_of(case):
    """The widest bound of the kernels that run the case (the sensitivity of a case is judged against it)."""
    return F32_TOL if case.tq == 1 else MFMA_TOL


# ------------------------------------------------------------------------------------------------------------ reference
def _limits(b, tk, lens, key_start):
    ln = torch.full((b,), tk, dtype=torch.int64) if lens is None else torch.as_tensor(lens, dtype=torch.int64).clamp(min=0, max=tk)
    ks = torch.zeros((b,), dtype=torch.int64) if key_start is None else torch.as_tensor(key_start, dtype=torch.int64).clamp(min=0)
    return ln, ks


def assigned_key(i, first, n_valid):
    """The key a non-causal query is boosted along (and the one `drop_diag` takes from it): first + 7 i mod n_valid."""
    return first + (7 * i) % n_valid


RefOut = namedtuple("RefOut", "out att zero")


def attn_ref(q, k, v, table=None, bias_u=None, bias_v=None, tk=None, pos0=0, center=0, causal=False, lens=None, key_start=None,
             mutate=None, emulate=False, out_f16=False, return_mask=False):
    """q [B, H, Tq, 64], k / v [B, H, rows >= tk, 64] (rows past ``tk`` are cache rows no query may see) -> float64 [B, H, Tq, 64].
    ``table`` None: plain MHA.  ``mutate`` names one wrong variant (MUTATIONS).  ``emulate`` rounds what the matrix-core kernels round.
    ``return_mask`` gives RefOut(out, att, zero): att [B, Tq, rows] says what a query attends (for relpos: 1 + the K/V row read at each
    visible position, 0 elsewhere; for MHA, where the order of the keys means nothing: how often each K/V row is attended), zero
    [B, Tq] the zero rows."""
    assert mutate is None or mutate in MUTATIONS, mutate
    q, k, v = q.double(), k.double(), v.double()
    b, h, tq, _ = q.shape
    rows = k.shape[2]
    tk = rows if tk is None else tk
    relpos = table is not None
    ln, ks = _limits(b, tk, lens, key_start)
    first, nvalid = ks, (ln - ks).clamp(min=1)                                    # of the true mask: what drop_diag's key is named by
    jfirst = (ks // 64) * 64
    if mutate == "kstart_minus":
        ks = (ks - 1).clamp(min=0)
    elif mutate == "kstart_plus":
        ks = ks + 1
    elif mutate == "lens_minus":
        ln = (ln - 1).clamp(min=0)
    elif mutate == "lens_plus":
        ln = (ln + 1).clamp(max=rows)
    i = torch.arange(tq)
    qpos = pos0 + i
    j = torch.arange(rows)
    vis = ((j[None, :] >= ks[:, None]) & (j[None, :] < ln[:, None]))[:, None, :].expand(b, tq, rows)
    if causal and not (mutate == "decode_not_causal" and tq == 1):
        vis = vis & (j[None, :] <= (qpos[:, None] + (1 if mutate == "leak_future" else 0)))[None]
    if mutate == "drop_diag":
        if causal:
            vis = vis & (j[None, :] != qpos[:, None])[None]
        else:
            vis = vis & (j[None, None, :] != assigned_key(i[None, :], first[:, None], nvalid[:, None])[:, :, None])
    elif mutate == "drop_first32":
        vis = vis & ~((j[None, :] >= jfirst[:, None]) & (j[None, :] < jfirst[:, None] + 32))[:, None, :]
    elif mutate == "drop_last_sub":
        vis = vis & ~((ln % 32 != 0)[:, None] & (j[None, :] >= (ln // 32 * 32)[:, None]))[:, None, :]
    zero = ~vis.any(-1)                                                             # [B, Tq]
    if mutate == "pad_nonzero":                   # what a kernel without the zero-row guard leaves: attention over the whole buffer
        free = (j[None, :] <= qpos[:, None]) if causal else torch.ones(tq, rows, dtype=torch.bool)
        vis = torch.where(zero[:, :, None], free[None].expand(b, tq, rows), vis)
        zero = torch.zeros_like(zero)
    src = j[None, :].expand(b, rows).clone()                                        # the K/V row read at each key position
    if mutate == "tile_swap" and not relpos:      # the two register sets are attn_mha_flash's
        ntiles = (ln + 63) // 64                                                    # staged tiles of the row
        part = j ^ 64
        ok = ((j[None, :] // 64) < ntiles[:, None]) & ((part[None, :] // 64) < ntiles[:, None])
        swapped = torch.where(ok, torch.minimum(part[None, :], (ln - 1)[:, None]), src)      # the prefetch clamps to the last valid row
        for r in range(b):                        # without positions a swap that only permutes a row's visible keys is no mistake
            seen = vis[r].any(0)
            if sorted(swapped[r][seen].tolist()) != sorted(j[seen].tolist()):
                src[r] = swapped[r]
        k = torch.gather(k, 2, src[:, None, :, None].expand(b, h, rows, DH))
        v = torch.gather(v, 2, src[:, None, :, None].expand(b, h, rows, DH))
    sc = SCALE * LOG2E
    rnd = (lambda x: x.half().double()) if emulate else (lambda x: x)
    if relpos:
        bu, bv = bias_u.double().view(1, h, 1, DH), bias_v.double().view(1, h, 1, DH)
        if mutate == "swap_uv":
            bu, bv = bv, bu
        s = torch.einsum("bhid,bhjd->bhij", rnd((q + bu) * sc), k)
        if mutate != "no_pos":
            tbl = table.double().view(-1, h, DH)
            if mutate == "pos_head_shift":
                tbl = torch.roll(tbl, -1, 1)                                        # head h reads head h + 1's columns
            idx = qpos[:, None] - j[None, :] + center + {"rel_plus": 1, "rel_minus": -1}.get(mutate, 0)      # [Tq, rows]
            idx = idx.clamp(min=0, max=tbl.shape[0] - 1)                            # only rows past tk can leave the table
            lo, hi = int(idx.min()), int(idx.max())
            g = torch.einsum("bhid,rhd->bhir", rnd((q + bv) * sc), tbl[lo:hi + 1])
            s = s + torch.gather(g, 3, (idx - lo)[None, None].expand(b, h, tq, rows))
    else:
        s = torch.einsum("bhid,bhjd->bhij", rnd(q * sc), k)
    s = s.masked_fill(~vis[:, None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhij,bhjd->bhid", rnd(p), v) / torch.where(l > 0, l, torch.ones_like(l))
    o = o.masked_fill(zero[:, None, :, None], 0.0)
    if emulate and out_f16:
        o = o.half().double()
    if not return_mask:
        return o
    live = vis & ~zero[:, :, None]
    if relpos:
        att = torch.where(live, src[:, None, :].expand(b, tq, rows) + 1, torch.zeros((), dtype=torch.int64))
    else:
        att = torch.zeros(b, tq, rows, dtype=torch.int64).scatter_add_(2, src[:, None, :].expand(b, tq, rows).contiguous(), live.long())
    return RefOut(o, att, zero)


def row_errors(got, ref):
    """got, ref [..., 64] -> (errors [...] = max |got - ref| / max |ref| per row, with 0 where the reference row is zero;
    flags [...] of reference zero rows where ``got`` is not exactly zero)."""
    got, ref = got.double(), ref.double()
    scale = ref.abs().amax(-1)
    zero = scale == 0
    err = (got - ref).abs().amax(-1) / torch.where(zero, torch.ones_like(scale), scale)
    return torch.where(zero, torch.zeros_like(err), err), zero & (got.abs().amax(-1) != 0)


def dont_care(case):
    """[B, Tq] bool: query rows at or beyond lens of the non-causal batch-major forms that still see a key (rows without a key are
    zero rows and are judged)."""
    ln, _ = _limits(case.b, case.tk, case.lens, case.key_start)
    if case.causal or case.form != "bm" or case.tq == 1:
        return torch.zeros(case.b, case.tq, dtype=torch.bool)
    return (torch.arange(case.tq)[None, :] >= ln[:, None]) & (ln[:, None] > 0)


# ------------------------------------------------------------------------------------------------------------ inputs
def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _orth(x, w):
    return x - (x * w).sum(-1, keepdim=True) * w


def _basis(w):
    """w [..., 1, 64] unit -> [..., 63, 64]: orthonormal rows, all orthogonal to w (rows 1 .. 63 of the 64 x 64 Hadamard matrix,
    reflected by the Householder map that takes row 0 to w: plain arithmetic, the same on every machine)."""
    n = torch.arange(DH)
    bits = sum(((n[:, None] >> s) & (n[None, :] >> s) & 1) for s in range(6))
    had = (1.0 - 2.0 * (bits % 2).double()) / math.sqrt(DH)
    x = had[0] - w
    return had[1:] - 2.0 * (had[1:] * x).sum(-1, keepdim=True) * x / (x * x).sum(-1, keepdim=True)


Inputs = namedtuple("Inputs", "case q k v table bias_u bias_v center")


def _f16(x):
    return x.half().double()


@functools.lru_cache(maxsize=None)
def build(case):
    """-> Inputs: q [B, H, Tq, 64], k / v [B, H, rows, 64] (rows = tk, + EXTRA_ROWS poisoned ones for the time-major and decode forms),
    table [2 center + 1, H 64] and biases [H 64] (None for MHA): float64 copies of fp16-representable values."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    b, h, tq, tk, pos0 = case.b, case.h, case.tq, case.tk, case.pos0
    rows = tk + (EXTRA_ROWS if case.op == "relpos" and (case.form == "tm" or case.tq == 1) else 0)
    ln, ks = _limits(b, tk, case.lens, case.key_start)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    w = _unit(rnd(1, 1, 1, DH)) * (1.0 - 2.0 * (torch.arange(h) % 2).double()).view(1, h, 1, 1)      # w of head h is (-1)^h w of head 0
    # the direction of each key: NCYC directions in turn, the sign changing with every turn (a boost along a key's direction also
    # reaches the key's aliases NCYC k positions away: with the sign every second one is pushed down instead), and two directions of
    # their own for a row's first and last valid key, which so have no alias at all
    basis = _basis(w)                                                               # [1, H, 63, 64]
    gen = 1.0 - 2.0 * ((torch.arange(rows) // NCYC) % 2).double()
    u = (basis[:, :, torch.arange(rows) % NCYC] * gen[:, None]).repeat(b, 1, 1, 1)  # [B, H, rows, 64]
    for bi in range(b):
        first, last = int(ks[bi]), int(ln[bi]) - 1
        if last >= first:
            u[bi, :, last] = basis[0, :, NCYC + 1]
            u[bi, :, first] = basis[0, :, NCYC]
    k = NOISE * _orth(rnd(b, h, rows, DH), w) + ALPHA * u
    v = rnd(b, h, rows, DH)
    j = torch.arange(rows)
    dead = (j[None, :] < ks[:, None]) | (j[None, :] >= ln[:, None])                 # [B, rows]: no query may see these keys
    sign = torch.where(torch.rand(b, h, rows, DH, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    k = torch.where(dead[:, None, :, None], POISON_K * w, k)
    v = torch.where(dead[:, None, :, None], POISON_V * sign, v)
    q = NOISE * _orth(rnd(b, h, tq, DH), w) + BETA * w
    for bi in range(b):
        first, last = int(ks[bi]), int(ln[bi]) - 1
        if last < first:
            continue                                                                # a row without keys
        n = last - first + 1
        for i in range(tq):
            pos = pos0 + i
            if case.causal:
                if pos < first:
                    continue                                                        # a pad query: no boost
                near = (max(pos - 1, first), pos, min(pos + 1, last)) if pos <= last else (max(last - 1, first), last)
            else:
                a = assigned_key(i, first, n)
                near = (a, a + 1) if a < last else (max(a - 1, first), a)
            boost = {}
            for key in near:
                boost[key] = BOOST_DIAG
            for key in (first, last):
                boost[key] = BOOST_EDGE                                             # each key once, the edge boost where both apply
            for key, c in boost.items():
                q[bi, :, i] += (c / 4.0) * ALPHA * u[bi, :, key]
    q, k, v = _f16(q), _f16(k), _f16(v)
    if case.op == "mha":
        return Inputs(case, q, k, v, None, None, None, 0)
    center = center_of(case)
    wf = w.reshape(h * DH)
    sign = 1.0 - 2.0 * (torch.arange(2 * center + 1) % 2).double()
    table = _f16(SIGMA * rnd(2 * center + 1, h * DH) + TABLE_ALT * sign[:, None] * wf[None, :])
    bias_u = _f16(BIAS_W * wf + BIAS_STD * rnd(h * DH))
    bias_v = _f16(-BIAS_W * wf + BIAS_STD * rnd(h * DH))
    return Inputs(case, q, k, v, table, bias_u, bias_v, center)


def ref_of(x, **kw):
    c = x.case
    return attn_ref(x.q, x.k, x.v, x.table, x.bias_u, x.bias_v, tk=c.tk, pos0=c.pos0, center=x.center, causal=c.causal, lens=c.lens,
                    key_start=c.key_start, **kw)


@functools.lru_cache(maxsize=None)
def expected(case):
    """The float64 reference of a case, [B, H, Tq, 64]; computed once and shared (do not write to it)."""
    return ref_of(build(case))


def judged(case):
    """[B, H, Tq] bool: the rows whose error counts (everything but the don't-care rows)."""
    return (~dont_care(case))[:, None, :].expand(case.b, case.h, case.tq)


# ------------------------------------------------------------------------------------------------------------ float32 evaluations
def attn_f32(x, way):
    """The relpos definition of a case evaluated in float32: way "forward" adds the keys one after the other, way "slots" keeps 16
    interleaved key slots with their own running maximum and sum and merges them flash-style at the end."""
    c = x.case
    f = lambda t: t.float()
    q, k, v = f(x.q), f(x.k[:, :, :c.tk]), f(x.v[:, :, :c.tk])
    b, h, tq, tk = c.b, c.h, c.tq, c.tk
    ln, ks = _limits(b, tk, c.lens, c.key_start)
    j = torch.arange(tk)
    qpos = c.pos0 + torch.arange(tq)
    vis = ((j[None, :] >= ks[:, None]) & (j[None, :] < ln[:, None]))[:, None, :].expand(b, tq, tk)
    if c.causal:
        vis = vis & (j[None, :] <= qpos[:, None])[None]
    scale = torch.tensor(SCALE, dtype=torch.float32)
    qu = (q + f(x.bias_u).view(1, h, 1, DH)) * scale
    qv = (q + f(x.bias_v).view(1, h, 1, DH)) * scale
    tbl = f(x.table).view(-1, h, DH)
    idx = qpos[:, None] - j[None, :] + x.center
    lo, hi = int(idx.min()), int(idx.max())
    g = torch.einsum("bhid,rhd->bhir", qv, tbl[lo:hi + 1])
    s = torch.einsum("bhid,bhjd->bhij", qu, k) + torch.gather(g, 3, (idx - lo)[None, None].expand(b, h, tq, tk))
    s = s.masked_fill(~vis[:, None], float("-inf"))

    def run(keys):
        """Keys ``keys`` in order -> (m, l, o) of the flash recurrence's end, the keys' weights taken against their own maximum."""
        ss = s[..., keys]
        m = ss.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = torch.exp(ss - m)
        l = torch.zeros(b, h, tq, 1)
        o = torch.zeros(b, h, tq, DH)
        for n, key in enumerate(keys.tolist()):
            l = l + p[..., n:n + 1]
            o = o + p[..., n:n + 1] * v[:, :, key:key + 1, :]
        return m, l, o

    if way == "forward":
        m, l, o = run(j)
    else:
        assert way == "slots"
        parts = [run(j[slot::16]) for slot in range(16) if slot < tk]
        m = torch.stack([pm for pm, _, _ in parts]).amax(0)
        l, o = torch.zeros(b, h, tq, 1), torch.zeros(b, h, tq, DH)
        for pm, pl, po in parts:
            wgt = torch.exp(pm - m)
            l, o = l + pl * wgt, o + po * wgt
    out = o / torch.where(l > 0, l, torch.ones_like(l))
    return out.masked_fill(~vis.any(-1)[:, None, :, None], 0.0)


# ------------------------------------------------------------------------------------------------------------ kernel-side layouts
def heads_last(x):
    """[B, H, T, 64] -> [B, T, H 64]."""
    return x.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[2], -1)


def heads_first(out, case):
    """A kernel's output in the layout of its q (bm: [B, Tq, H 64], tm: [Tq, B, H 64]) -> [B, H, Tq, 64]."""
    if case.form == "bm":
        return out.reshape(out.shape[0], case.tq, case.h, DH).permute(0, 2, 1, 3)
    return out.reshape(case.tq, out.shape[1], case.h, DH).permute(1, 2, 0, 3)


def expected_kernel(tq, b, h, kv_f16, pos_f16, q_ptr, k_ptr, v_ptr, pos_ptr, ldk, ldp, k_bs, q_bs):
    """The kernel astts_op_attn_relpos launches for these arguments, by the launcher's own conditions (no environment switch set)."""
    al = (k_ptr % 16 == 0 and v_ptr % 16 == 0 and pos_ptr % 16 == 0 and ldk % 8 == 0 and ldp % 8 == 0 and k_bs % 8 == 0)
    if tq == 1:
        rows = b > 32 and kv_f16 and pos_f16 and h % 4 == 0 and al and q_ptr % 16 == 0 and q_bs % 4 == 0
        return "attn_relpos_rows" if rows else "attn_relpos_decode"
    return "attn_relpos_mfma" if al else "attn_relpos"


def mha_buffer(x, dtype):
    """The fused [B, T, 3 H 64] q | k | v buffer of an MHA case; the operator takes its thirds as views."""
    return torch.cat([heads_last(x.q), heads_last(x.k), heads_last(x.v)], -1).to(dtype).contiguous()


def relpos_buffers(x, kv_dtype, pos_dtype, pad=0):
    """-> dict: q fp32 (bm [B, Tq, H 64], tm [Tq, B, H 64]), kv: the K | V buffer in ``kv_dtype`` (bm [B, rows, 2 H 64 + pad], tm
    [rows, B, 2 H 64 + pad]; the pad columns are poisoned like V), table in ``pos_dtype``, bias_u, bias_v fp32.  pad = VALU_PAD makes the
    row stride (bm) or the batch stride (tm) of the K and V views 4 mod 8, which the matrix-core kernel's loads do not take."""
    c = x.case
    kv = torch.cat([heads_last(x.k), heads_last(x.v)] + ([torch.full((c.b, x.k.shape[2], pad), POISON_V, dtype=torch.float64)] if pad else []), -1)
    q = heads_last(x.q)
    if c.form == "tm":
        kv, q = kv.transpose(0, 1), q.transpose(0, 1)
    return {"q": q.float().contiguous(), "kv": kv.to(kv_dtype).contiguous(), "table": x.table.to(pos_dtype).contiguous(),
            "bias_u": x.bias_u.float().contiguous(), "bias_v": x.bias_v.float().contiguous()}
