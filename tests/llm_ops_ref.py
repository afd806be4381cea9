"""Float64 statements of the Llama operators of csrc/ops_llm.hip (rmsnorm_rows, rope_llama, rope_llama_ex, swiglu_rows, mean_pool,
argmax_rows, attn_causal_gqa, attn_gqa_mfma), the case lists at the kernels' tile and grid edges, the input builders and the tolerances.
tests/test_llm_ops_cpu.py proves the references and the sensitivity of the cases without a GPU; tests/test_llm_ops_gpu.py runs the kernels.

Attention.  Key j is visible to query i of batch row b iff j <= pos0 + i and j >= key_start[b] and j < lens[b]; a query whose position
pos0 + i is at or beyond lens[b], or that sees no key, gives zeros.  The error of a result is taken per (batch row, head, query): the
largest absolute error over the 128 dims divided by the largest absolute value of that reference row (`row_errors`), so that a short-context
row with a large output does not set the scale of a long-context one.

Inputs (`build_attn`) are made so that every mask boundary carries weight: each valid key position has a unit direction (orthonormal,
repeating every 127 keys), added x ALPHA (a score boost of 4) to the key and to the queries that must notice it -- the query on its
diagonal, the query just before it (a future-key leak), and, for a row's first and last valid key, every query of the row.  Every key
that no query may see (left pads, right pads, cache rows past tk) is poisoned: K = POISON_K x a direction that every query of the group
has a component of (score ~ +136, so a leak takes the whole softmax), V = +-POISON_V.  The poison is finite: the kernels multiply masked
V by p = 0.

Tolerance.  The matrix-core kernel rounds q * scale * log2(e), p and the output to fp16; `attn_ref(..., emulate=True)` is the float64
computation with exactly those three roundings.  Its worst per-row error against the exact reference over the whole case list
(ATTN_CASES_BM + ATTN_CASES_TM) is ATTN_EMU_FLOOR = 8.3e-4 (measured: 8.30e-4, at bm-h6x2-t63-l63_62), and ATTN_TOL is
3 x that = 2.49e-3: the margin is for the fp32 accumulation order and the hardware exp2, both below the roundings emulated
(tests/test_llm_ops_cpu.py measures the floor again and holds ATTN_TOL between 2 x and 4 x of it).  The VALU kernel rounds less (p
stays fp32) and is held to the same bound.  Nothing here is taken from a kernel's output."""
import functools
import math
import zlib
from collections import namedtuple

import torch

HD = 128
SCALE = 1.0 / math.sqrt(HD)
LOG2E = 1.44269504088896341
ALPHA = math.sqrt(4.0 / SCALE)        # |direction| added to a key and to its queries: score boost ALPHA^2 * SCALE = 4
BETA = 3.0                            # every query's component along its group's poison direction
POISON_K = 512.0                      # a leaked pad key scores BETA * POISON_K * SCALE ~ 136 above everything else
POISON_V = 30000.0
NOISE = 0.25                          # std of the random part of q and k

ATTN_EMU_FLOOR = 8.3e-4               # measured by test_llm_ops_cpu.py::test_attn_tol_is_three_times_the_emulation_floor
ATTN_TOL = 3 * ATTN_EMU_FLOOR

MUTATIONS = ("drop_diag", "leak_future", "kstart_minus", "kstart_plus", "lens_minus", "lens_plus", "kv_mod", "drop_first32", "pad_nonzero")

AttnCase = namedtuple("AttnCase", "name form heads kv_heads b tq tk pos0 lens key_start")


def _bm(heads, kvh, t, lens):
    return AttnCase(f"bm-h{heads}x{kvh}-t{t}-l" + "_".join(map(str, lens)), "bm", heads, kvh, len(lens), t, t, 0, tuple(lens), None)


def _tm(heads, kvh, tq, tk, ks, lens=None, pos0=None):
    pos0 = tk - tq if pos0 is None else pos0
    name = f"tm-h{heads}x{kvh}-q{tq}-k{tk}-s" + "_".join(map(str, ks)) + ("" if lens is None else "-l" + "_".join(map(str, lens)))
    return AttnCase(name, "tm", heads, kvh, len(ks), tq, tk, pos0, None if lens is None else tuple(lens), tuple(ks))


GEOMS = ((6, 2), (4, 2))
BM_T = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 385)
# right-padded, batch-major views into a fused q|k|v buffer (ops.attn_gqa(..., lens) and ops.attn_causal_gqa)
ATTN_CASES_BM = tuple(_bm(h, kv, t, ln) for (h, kv) in GEOMS for t in BM_T for ln in ((t, 1), (t, t - 1))) + tuple(
    _bm(h, kv, 257, ln) for (h, kv) in GEOMS for ln in ((257, 129, 128, 64), (257, 100))) + (_bm(2, 2, 129, (129, 77)),)

# generation form, time-major; key_start per batch row drawn from {0, 1, 63, 64, 65, 127, 128, 200}, pos0 + tq - 1 (one visible key for
# the last query) and one value above pos0 (pad queries: zero rows), clipped to the case
_TM = (
    (1, 1, (0, 0, 0, 0)),
    (1, 64, (0, 1, 63, 63)),
    (1, 65, (0, 1, 63, 64)),
    (1, 129, (64, 65, 127, 128)),
    (1, 513, (0, 128, 200, 512)),
    (3, 65, (0, 32, 64, 63)),                   # pos0 = 62: the second query sits on the last key of a sub-tile, the first must not see it
    (3, 77, (0, 63, 76, 75)),
    (33, 200, (1, 128, 199, 180)),
    (40, 73, (0, 1, 72, 50)),                   # pos0 = 33: a wave's last query sits on the first key of a 32-key sub-tile
    (130, 333, (64, 200, 332, 270)),
    (260, 391, (65, 127, 390, 200)),            # three query blocks, pos0 = 131
)
ATTN_CASES_TM = tuple(_tm(h, kv, tq, tk, ks) for (h, kv) in GEOMS for (tq, tk, ks) in _TM) + tuple(
    # lens and key_start together, pos0 > 0 (and pos0 + tq < tk: the cache holds more than the block attends)
    _tm(h, kv, 70, 300, (0, 64, 130, 200), lens=(300, 256, 230, 201), pos0=200) for (h, kv) in GEOMS)
TM_EXTRA_ROWS = 70                                # poisoned cache rows past tk

KEY_START_SET = (0, 1, 63, 64, 65, 127, 128, 200)


# ------------------------------------------------------------------------------------------------------------ attention: reference
def _limits(b, tk, lens, key_start):
    ln = torch.full((b,), tk, dtype=torch.int64) if lens is None else torch.as_tensor(lens, dtype=torch.int64).clamp(max=tk)
    ks = torch.zeros((b,), dtype=torch.int64) if key_start is None else torch.as_tensor(key_start, dtype=torch.int64).clamp(min=0)
    return ln, ks


def attn_ref(q, k, v, pos0=0, key_start=None, lens=None, mutate=None, emulate=False, return_mask=False):
    """q [B, heads, Tq, 128], k / v [B, kv_heads, Tk, 128] -> float64 [B, heads, Tq, 128].

    ``mutate`` (only tests/test_llm_ops_cpu.py uses it) names one wrong variant, see MUTATIONS.  ``emulate`` rounds q * scale * log2(e),
    p and the output to fp16 as attn_gqa_mfma does (p relative to the row's final maximum).  ``return_mask`` also gives what decides a
    row: the visibility [B, heads, Tq, Tk] (the KV head folded in as a head-dependent copy) and the zero-row flags [B, heads, Tq]."""
    assert mutate is None or mutate in MUTATIONS, mutate
    q, k, v = q.double(), k.double(), v.double()
    b, heads, tq, _ = q.shape
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
        s = torch.einsum("bhid,bhjd->bhij", (q * (SCALE * LOG2E)).half().double(), kk)
    else:
        s = torch.einsum("bhid,bhjd->bhij", q, kk) * (SCALE * LOG2E)
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
    """got, ref [..., 128] -> (errors [...] = max |got - ref| / max |ref| per row, with 0 where the reference row is zero;
    flags [...] of reference zero rows where ``got`` is not exactly zero)."""
    got, ref = got.double(), ref.double()
    scale = ref.abs().amax(-1)
    zero = scale == 0
    err = (got - ref).abs().amax(-1) / torch.where(zero, torch.ones_like(scale), scale)
    return torch.where(zero, torch.zeros_like(err), err), zero & (got.abs().amax(-1) != 0)


# ------------------------------------------------------------------------------------------------------------ attention: inputs
def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _orth(x, w):
    return x - (x * w).sum(-1, keepdim=True) * w


def _basis(w):
    """w [..., 1, 128] unit -> [..., 127, 128]: orthonormal rows, all orthogonal to w (rows 1 .. 127 of the 128 x 128 Hadamard matrix,
    reflected by the Householder map that takes row 0 to w: plain arithmetic, the same on every machine)."""
    n = torch.arange(HD)
    bits = sum(((n[:, None] >> s) & (n[None, :] >> s) & 1) for s in range(7))
    had = (1.0 - 2.0 * (bits % 2).double()) / math.sqrt(HD)
    v = had[0] - w
    return had[1:] - 2.0 * (had[1:] * v).sum(-1, keepdim=True) * v / (v * v).sum(-1, keepdim=True)


AttnInputs = namedtuple("AttnInputs", "case q k v bufs")


@functools.lru_cache(maxsize=None)
def build_attn(case):
    """-> AttnInputs: q [B, heads, Tq, 128], k / v [B, kv_heads, Tk, 128] as float64 copies of the fp16 values the kernels read, and
    ``bufs``: the fp16 buffers in the kernel's layout -- form "bm": {"qkv": [B, T, (heads + 2 kv_heads) 128]}; form "tm":
    {"q": [Tq, B, heads 128], "cache": [Tk + TM_EXTRA_ROWS, B, 2 kv_heads 128]} (K | V, rows past tk poisoned)."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    b, heads, kvh, tq, tk, pos0 = case.b, case.heads, case.kv_heads, case.tq, case.tk, case.pos0
    rep = heads // kvh
    rows = tk + (TM_EXTRA_ROWS if case.form == "tm" else 0)
    ln, ks = _limits(b, tk, case.lens, case.key_start)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    w = _unit(rnd(b, kvh, 1, HD))                                                  # poison direction of a (batch row, KV group)
    # the direction of each key position: orthonormal, orthogonal to w, repeating every 127 keys (so a query also meets its boosted
    # keys' aliases 127 k positions away; no cross-talk otherwise)
    u = _basis(w)[:, :, torch.arange(rows) % (HD - 1)]
    k = NOISE * _orth(rnd(b, kvh, rows, HD), w) + ALPHA * u
    v = rnd(b, kvh, rows, HD)
    j = torch.arange(rows)
    dead = (j[None, :] < ks[:, None]) | (j[None, :] >= ln[:, None])                 # [B, rows]: no query may see these keys
    sign = torch.where(torch.rand(b, kvh, rows, HD, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    k = torch.where(dead[:, None, :, None], POISON_K * w, k)
    v = torch.where(dead[:, None, :, None], POISON_V * sign, v)
    q = NOISE * _orth(rnd(b, heads, tq, HD), w.repeat_interleave(rep, 1)) + BETA * w.repeat_interleave(rep, 1)
    for bi in range(b):
        first, last = int(ks[bi]), int(ln[bi]) - 1
        for i in range(tq):
            pos = pos0 + i
            if not first <= pos <= last:
                continue                                                            # a pad query: no boost
            for key in sorted({key % (HD - 1) for key in (pos, min(pos + 1, last), first, last)}):      # each direction once
                q[bi, :, i] += ALPHA * u[bi, :, key].repeat_interleave(rep, 0)
    q16, k16, v16 = q.half(), k.half(), v.half()
    if case.form == "bm":
        flat = lambda x: x.permute(0, 2, 1, 3).reshape(b, x.shape[2], -1)
        bufs = {"qkv": torch.cat([flat(q16), flat(k16), flat(v16)], -1).contiguous()}
    else:
        flat = lambda x: x.permute(2, 0, 1, 3).reshape(x.shape[2], b, -1)
        bufs = {"q": flat(q16).contiguous(), "cache": torch.cat([flat(k16), flat(v16)], -1).contiguous()}
    return AttnInputs(case, q16.double(), k16[:, :, :tk].double(), v16[:, :, :tk].double(), bufs)


@functools.lru_cache(maxsize=None)
def attn_expected(case):
    """The float64 reference of a case, [B, heads, Tq, 128]; computed once and shared (do not write to it)."""
    x = build_attn(case)
    return attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens)


def heads_first(out, case):
    """A kernel's output in the layout of its q (bm: [B, Tq, heads 128], tm: [Tq, B, heads 128]) -> [B, heads, Tq, 128]."""
    if case.form == "bm":
        return out.reshape(case.b, case.tq, case.heads, HD).permute(0, 2, 1, 3)
    return out.reshape(case.tq, case.b, case.heads, HD).permute(1, 2, 0, 3)


# ------------------------------------------------------------------------------------------------------------ the other kernels
RMS_C = (3, 63, 64, 66, 512, 3072, 3074)
RMS_ROWS = (1, 5)
RMS_SCALES = (1e4, 1e-4)
RMS_EPS = 1e-5
RMS_TOL_F32 = 1e-5                    # per row, of the row's largest value (the bound of test_llm_operators_against_definitions)
RMS_TOL_F16 = 2.0 ** -10              # per element, relative: the fp16 rounding (2^-11) with room for the fp32 arithmetic before it


def rms_inputs(c, rows, scale):
    """x fp32 [rows, c] with every |x| in [0.75, ~10] x scale (no output small enough to be an fp16 subnormal), w fp32 [c]."""
    g = torch.Generator().manual_seed(1000 * c + rows)
    z = torch.randn(rows, c, generator=g)
    x = (torch.sign(z) + (z == 0)) * (0.25 + z.abs()) * 3.0 * scale
    return x.float(), (1 + 0.1 * torch.randn(c, generator=g)).float()


def rmsnorm_ref(x, w, eps):
    x, w = x.double(), w.double()
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def rope_tables(n, head_dim=HD, theta=500000.0):
    """cos / sin fp32 [n, head_dim / 2] (the kernels take the table's first half: emb = cat(freqs, freqs))."""
    inv = theta ** (-torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim)
    f = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]
    return f.cos().float().contiguous(), f.sin().float().contiguous()


ROPE_HEADS, ROPE_V_HEADS = 32, 8      # 24 query + 8 key heads are rotated; 8 value heads follow them in the row
# (b, t, pos0): the large one has 2 * 300 * 32 * 64 = 1 228 800 pairs > 4096 blocks x 256 threads
ROPE_CASES = ((2, 300, 0), (2, 300, 200), (3, 7, 0), (1, 1, 200))
# (b, t, pos0, time_major, shift)
ROPE_EX_CASES = (
    (2, 300, 0, False, (0, 9)),
    (2, 300, 200, True, (0, 250)),
    (3, 7, 0, False, None),
    (3, 7, 200, True, (0, 9, 205)),
    (4, 1, 200, False, (0, 9, 200, 250)),        # a decode step; 250 > 200 clamps to position 0
    (4, 1, 200, True, (0, 9, 200, 250)),
)


def rope_ref(x, cos, sin, heads, head_dim, pos):
    """x [..., ld] (any float type), pos int64 broadcastable to x.shape[:-1] -> (float64 result with the first heads * head_dim columns
    rotated, per-element bound 2^-11 (|a| + |b|) (1 + 2^-10): the fp16 rounding of a value no larger than |a| + |b|; 0 elsewhere)."""
    x = x.double()
    h = head_dim // 2
    c, s = cos.double()[pos][..., None, :], sin.double()[pos][..., None, :]
    xr = x[..., :heads * head_dim].reshape(*x.shape[:-1], heads, head_dim)
    a, b = xr[..., :h], xr[..., h:]
    out, bound = x.clone(), torch.zeros_like(x)
    out[..., :heads * head_dim] = torch.cat([a * c - b * s, b * c + a * s], -1).reshape(*x.shape[:-1], heads * head_dim)
    mag = (a.abs() + b.abs()) * (2.0 ** -11 * (1 + 2.0 ** -10))
    bound[..., :heads * head_dim] = torch.cat([mag, mag], -1).reshape(*x.shape[:-1], heads * head_dim)
    return out, bound


def rope_positions(b, t, pos0, time_major, shift):
    ti = torch.arange(t)[:, None] if time_major else torch.arange(t)[None, :]
    sh = torch.zeros(b, dtype=torch.int64) if shift is None else torch.as_tensor(shift, dtype=torch.int64)
    return (pos0 + ti - (sh[None, :] if time_major else sh[:, None])).clamp(min=0)


SWIGLU_BIG = (2100, 8192)             # 2100 * 1024 = 2 150 400 vectors of 8 > 8192 blocks x 256 threads
SWIGLU_GATES = (-65504.0, -100.0, -20.0, -0.0, 0.0, 20.0, 65504.0, 1.0)
F16_SUBNORMAL = 2.0 ** -24


def swiglu_ref(gu):
    """fp16 [..., 2f] -> (float64 silu(gate) * up, per-element bound 2^-10 |ref| + one fp16 subnormal step)."""
    f = gu.shape[-1] // 2
    g, u = gu[..., :f].double(), gu[..., f:].double()
    ref = g * torch.sigmoid(g) * u
    return ref, ref.abs() * 2.0 ** -10 + F16_SUBNORMAL


ARGMAX_N = (1, 5, 255, 256, 257, 128256)
MEAN_POOL_C = (96, 257, 3072)
MEAN_POOL_T = 512
MEAN_POOL_LENS = (0, 1, 300, MEAN_POOL_T, MEAN_POOL_T + 7)


def mean_pool_ref(x, lens):
    """fp32 [B, T, C], lens -> (float64 [B, C], per-element bound n 2^-24 mean|x|: n - 1 roundings of the sequential fp32 sum, each at
    most 2^-24 of sum|x|, and one of the division)."""
    x = x.double()
    out, bound = torch.zeros(x.shape[0], x.shape[2], dtype=torch.float64), torch.zeros(x.shape[0], x.shape[2], dtype=torch.float64)
    for i, n in enumerate(lens):
        n = min(int(n), x.shape[1])
        if n > 0:
            out[i] = x[i, :n].mean(0)
            bound[i] = n * 2.0 ** -24 * x[i, :n].abs().mean(0)
    return out, bound
