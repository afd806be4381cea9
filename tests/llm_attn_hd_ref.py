"""The attention part of tests/llm_ops_ref.py with the head dimension as a parameter: the float64 statement of attn_causal_gqa and
attn_gqa_mfma (csrc/ops_llm.hip), the input builder, the head-dimension-64 case lists and their tolerance.  At ``hd = 128`` every
function here gives llm_ops_ref's bits (tests/test_llm_hd64_cpu.py holds that), which ties this module to the proven one; the GPU tests
of head dimension 64 (tests/test_llm_hd64_gpu.py) use it at ``hd = 64``.

The rules are llm_ops_ref's.  Key j is visible to query i of batch row b iff j <= pos0 + i and j >= key_start[b] and j < lens[b]; a
query at or beyond lens[b], or that sees no key, gives zeros.  Errors are per (batch row, head, query): the largest absolute error over
the hd dims divided by the largest absolute value of the reference row.  Each valid key position has a unit direction (rows 1 .. hd - 1
of the hd x hd Hadamard matrix, reflected to be orthogonal to the group's poison direction: 63 directions at 64, so they repeat every
63 keys), added x ALPHA (a score boost of 4) to the key and to the queries that must notice it; every key that no query may see is
poisoned (score ~ BETA POISON_K scale above everything else: +192 at 64).

Cases at 64 (the smallest shapes that cross the 32-query wave, the 128-query block, the 32-key sub-tile, the 64-key tile and the
skipped-tile boundary), for the geometries (8, 2), (14, 2) and (2, 2) = KV groups of 4, 7 and 1:
  batch-major   t in {1, 33, 65, 129} with lens (t, 1) and (t, t - 1); 257 with lens (257, 129, 128, 64)
  time-major    (tq, tk) = (1, 1), (1, 65), (1, 129) with key_start (64, 65, 127, 128), (3, 65), (40, 73), (130, 333) with key_start
                (64, 200, 332, 270), and (70, 300) at pos0 = 200 with lens and key_start; cache rows past tk are poisoned

Tolerance.  ``attn_ref(..., emulate=True)`` is the float64 computation with the matrix-core kernel's three fp16 roundings (q * scale *
log2(e), p, the output).  Its worst per-row error against the exact reference over CASES_64 is ATTN64_EMU_FLOOR = 1.06e-3 (measured:
1.062e-3, at tm-h2x2-q130-k333-s64_200_332_270), and ATTN64_TOL is 3 x that = 3.18e-3, the project's rule (tests/test_llm_hd64_cpu.py measures the floor again
and holds the tolerance between 2 x and 4 x of it).  Nothing here is taken from a kernel's output."""
import functools
import math
import zlib
from collections import namedtuple

import torch

LOG2E = 1.44269504088896341
BETA = 3.0                            # every query's component along its group's poison direction
POISON_K = 512.0
POISON_V = 30000.0
NOISE = 0.25                          # std of the random part of q and k

ATTN64_EMU_FLOOR = 1.06e-3            # measured by test_llm_hd64_cpu.py::test_tolerance_is_three_times_the_emulation_floor_at_64
ATTN64_TOL = 3 * ATTN64_EMU_FLOOR

MUTATIONS = ("drop_diag", "leak_future", "kstart_minus", "kstart_plus", "lens_minus", "lens_plus", "kv_mod", "drop_first32", "pad_nonzero")

AttnCase = namedtuple("AttnCase", "name form heads kv_heads b tq tk pos0 lens key_start")


def scale_of(hd):
    return 1.0 / math.sqrt(hd)


def alpha_of(hd):
    """|direction| added to a key and to its queries: score boost alpha^2 * scale = 4"""
    return math.sqrt(4.0 / scale_of(hd))


def _bm(heads, kvh, t, lens):
    return AttnCase(f"bm-h{heads}x{kvh}-t{t}-l" + "_".join(map(str, lens)), "bm", heads, kvh, len(lens), t, t, 0, tuple(lens), None)


def _tm(heads, kvh, tq, tk, ks, lens=None, pos0=None):
    pos0 = tk - tq if pos0 is None else pos0
    name = f"tm-h{heads}x{kvh}-q{tq}-k{tk}-s" + "_".join(map(str, ks)) + ("" if lens is None else "-l" + "_".join(map(str, lens)))
    return AttnCase(name, "tm", heads, kvh, len(ks), tq, tk, pos0, None if lens is None else tuple(lens), tuple(ks))


GEOMS_64 = ((8, 2), (14, 2), (2, 2))
BM_T_64 = (1, 33, 65, 129)
CASES_BM_64 = tuple(_bm(h, kv, t, ln) for (h, kv) in GEOMS_64 for t in BM_T_64 for ln in ((t, 1), (t, t - 1))) + tuple(
    _bm(h, kv, 257, (257, 129, 128, 64)) for (h, kv) in GEOMS_64)
_TM_64 = (
    (1, 1, (0, 0, 0, 0)),
    (1, 65, (0, 1, 63, 64)),
    (1, 129, (64, 65, 127, 128)),
    (3, 65, (0, 32, 64, 63)),                   # pos0 = 62: the second query sits on the last key of a sub-tile
    (40, 73, (0, 1, 72, 50)),                   # pos0 = 33: a wave's last query sits on the first key of a 32-key sub-tile
    (130, 333, (64, 200, 332, 270)),
)
CASES_TM_64 = tuple(_tm(h, kv, tq, tk, ks) for (h, kv) in GEOMS_64 for (tq, tk, ks) in _TM_64) + tuple(
    _tm(h, kv, 70, 300, (0, 64, 130, 200), lens=(300, 256, 230, 201), pos0=200) for (h, kv) in GEOMS_64)
CASES_64 = CASES_BM_64 + CASES_TM_64
TM_EXTRA_ROWS = 70                                # poisoned cache rows past tk


# ------------------------------------------------------------------------------------------------------------ reference
def _limits(b, tk, lens, key_start):
    ln = torch.full((b,), tk, dtype=torch.int64) if lens is None else torch.as_tensor(lens, dtype=torch.int64).clamp(max=tk)
    ks = torch.zeros((b,), dtype=torch.int64) if key_start is None else torch.as_tensor(key_start, dtype=torch.int64).clamp(min=0)
    return ln, ks


def attn_ref(q, k, v, pos0=0, key_start=None, lens=None, mutate=None, emulate=False, return_mask=False):
    """q [B, heads, Tq, hd], k / v [B, kv_heads, Tk, hd] -> float64 [B, heads, Tq, hd]; the head dimension is q's last axis.

    ``mutate`` names one wrong variant, see MUTATIONS.  ``emulate`` rounds q * scale * log2(e), p and the output to fp16 as attn_gqa_mfma
    does (p relative to the row's final maximum).  ``return_mask`` also gives the visibility [B, heads, Tq, Tk], the zero-row flags
    [B, heads, Tq] and the head -> KV head map."""
    assert mutate is None or mutate in MUTATIONS, mutate
    q, k, v = q.double(), k.double(), v.double()
    b, heads, tq, hd = q.shape
    scale = scale_of(hd)
    kvh, tk = k.shape[1], k.shape[2]
    rep = heads // kvh
    hmap = torch.arange(heads) % kvh if mutate == "kv_mod" else torch.arange(heads) // rep
    ln, ks = _limits(b, tk, lens, key_start)
    jfirst = (ks // 64) * 64
    if mutate == "kstart_minus":
        ks = (ks - 1).clamp(min=0)
    elif mutate == "kstart_plus":
        ks = ks + 1
    elif mutate == "lens_minus":
        ln = (ln - 1).clamp(min=0)
    elif mutate == "lens_plus":
        ln = (ln + 1).clamp(max=tk)
    qpos = pos0 + torch.arange(tq)
    j = torch.arange(tk)
    causal = j[None, :] <= (qpos[:, None] + (1 if mutate == "leak_future" else 0))                 # [Tq, Tk]
    vis = causal[None] & (j[None, None, :] >= ks[:, None, None]) & (j[None, None, :] < ln[:, None, None])
    if mutate == "drop_diag":
        vis = vis & (j[None, :] != qpos[:, None])[None]
    elif mutate == "drop_first32":
        vis = vis & ~((j[None, :] >= jfirst[:, None]) & (j[None, :] < jfirst[:, None] + 32))[:, None, :]
    qvalid = qpos[None, :] < ln[:, None]                                                            # [B, Tq]
    zero = ~(qvalid & vis.any(-1))
    if mutate == "pad_nonzero":                    # what a kernel without the zeroing would leave: plain causal attention over the buffer
        vis = torch.where(zero[:, :, None], (j[None, :] <= qpos[:, None])[None].expand(b, tq, tk), vis)
        zero = torch.zeros_like(zero)
    kk, vv = k[:, hmap], v[:, hmap]
    if emulate:
        s = torch.einsum("bhid,bhjd->bhij", (q * (scale * LOG2E)).half().double(), kk)
    else:
        s = torch.einsum("bhid,bhjd->bhij", q, kk) * (scale * LOG2E)
    s = s.masked_fill(~vis[:, None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    if emulate:
        p = p.half().double()
    o = torch.einsum("bhij,bhjd->bhid", p, vv) / torch.where(l > 0, l, torch.ones_like(l))
    o = o.masked_fill(zero[:, None, :, None], 0.0)
    if emulate:
        o = o.half().double()
    if return_mask:
        return o, vis[:, None].expand(b, heads, tq, tk), zero[:, None].expand(b, heads, tq), hmap
    return o


def row_errors(got, ref):
    """got, ref [..., hd] -> (errors [...] = max |got - ref| / max |ref| per row, with 0 where the reference row is zero;
    flags [...] of reference zero rows where ``got`` is not exactly zero)."""
    got, ref = got.double(), ref.double()
    scale = ref.abs().amax(-1)
    zero = scale == 0
    err = (got - ref).abs().amax(-1) / torch.where(zero, torch.ones_like(scale), scale)
    return torch.where(zero, torch.zeros_like(err), err), zero & (got.abs().amax(-1) != 0)


# ------------------------------------------------------------------------------------------------------------ inputs
def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _orth(x, w):
    return x - (x * w).sum(-1, keepdim=True) * w


def _basis(w):
    """w [..., 1, hd] unit -> [..., hd - 1, hd]: orthonormal rows, all orthogonal to w (rows 1 .. hd - 1 of the hd x hd Hadamard matrix,
    reflected by the Householder map that takes row 0 to w: plain arithmetic, the same on every machine)."""
    hd = w.shape[-1]
    n = torch.arange(hd)
    bits = sum(((n[:, None] >> s) & (n[None, :] >> s) & 1) for s in range(hd.bit_length() - 1))
    had = (1.0 - 2.0 * (bits % 2).double()) / math.sqrt(hd)
    v = had[0] - w
    return had[1:] - 2.0 * (had[1:] * v).sum(-1, keepdim=True) * v / (v * v).sum(-1, keepdim=True)


AttnInputs = namedtuple("AttnInputs", "case q k v bufs")


@functools.lru_cache(maxsize=None)
def build_attn(case, hd=64):
    """-> AttnInputs: q [B, heads, Tq, hd], k / v [B, kv_heads, Tk, hd] as float64 copies of the fp16 values the kernels read, and
    ``bufs``: the fp16 buffers in the kernel's layout -- form "bm": {"qkv": [B, T, (heads + 2 kv_heads) hd]}; form "tm":
    {"q": [Tq, B, heads hd], "cache": [Tk + TM_EXTRA_ROWS, B, 2 kv_heads hd]} (K | V, rows past tk poisoned)."""
    assert hd >= 2 and hd & (hd - 1) == 0, hd
    alpha = alpha_of(hd)
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    b, heads, kvh, tq, tk, pos0 = case.b, case.heads, case.kv_heads, case.tq, case.tk, case.pos0
    rep = heads // kvh
    rows = tk + (TM_EXTRA_ROWS if case.form == "tm" else 0)
    ln, ks = _limits(b, tk, case.lens, case.key_start)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    w = _unit(rnd(b, kvh, 1, hd))                                                  # poison direction of a (batch row, KV group)
    u = _basis(w)[:, :, torch.arange(rows) % (hd - 1)]                              # the direction of each key position
    k = NOISE * _orth(rnd(b, kvh, rows, hd), w) + alpha * u
    v = rnd(b, kvh, rows, hd)
    j = torch.arange(rows)
    dead = (j[None, :] < ks[:, None]) | (j[None, :] >= ln[:, None])                 # [B, rows]: no query may see these keys
    sign = torch.where(torch.rand(b, kvh, rows, hd, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    k = torch.where(dead[:, None, :, None], POISON_K * w, k)
    v = torch.where(dead[:, None, :, None], POISON_V * sign, v)
    q = NOISE * _orth(rnd(b, heads, tq, hd), w.repeat_interleave(rep, 1)) + BETA * w.repeat_interleave(rep, 1)
    for bi in range(b):
        first, last = int(ks[bi]), int(ln[bi]) - 1
        for i in range(tq):
            pos = pos0 + i
            if not first <= pos <= last:
                continue                                                            # a pad query: no boost
            for key in sorted({key % (hd - 1) for key in (pos, min(pos + 1, last), first, last)}):      # each direction once
                q[bi, :, i] += alpha * u[bi, :, key].repeat_interleave(rep, 0)
    q16, k16, v16 = q.half(), k.half(), v.half()
    if case.form == "bm":
        flat = lambda x: x.permute(0, 2, 1, 3).reshape(b, x.shape[2], -1)
        bufs = {"qkv": torch.cat([flat(q16), flat(k16), flat(v16)], -1).contiguous()}
    else:
        flat = lambda x: x.permute(2, 0, 1, 3).reshape(x.shape[2], b, -1)
        bufs = {"q": flat(q16).contiguous(), "cache": torch.cat([flat(k16), flat(v16)], -1).contiguous()}
    return AttnInputs(case, q16.double(), k16[:, :, :tk].double(), v16[:, :, :tk].double(), bufs)


@functools.lru_cache(maxsize=None)
def attn_expected(case, hd=64):
    """The float64 reference of a case, [B, heads, Tq, hd]; computed once and shared (do not write to it)."""
    x = build_attn(case, hd)
    return attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens)


def heads_first(out, case, hd=64):
    """A kernel's output in the layout of its q (bm: [B, Tq, heads hd], tm: [Tq, B, heads hd]) -> [B, heads, Tq, hd]."""
    if case.form == "bm":
        return out.reshape(case.b, case.tq, case.heads, hd).permute(0, 2, 1, 3)
    return out.reshape(case.tq, case.b, case.heads, hd).permute(1, 2, 0, 3)
