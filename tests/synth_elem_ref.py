"""Float64 statement of the operators of csrc/ops_norm_elem.hip (LayerNorm, GroupNorm, the element-wise family, embedding gather, linear
interpolation) and of the signal operators at the head of csrc/ops_audio.hip (f0_prefix / nsf_source, stft16, istft16); with the wrong
variants (`mutate=`), the case lists at the kernels' path, chunk and grid-stride edges, the input builders and the bounds.
tests/test_synth_elem_cpu.py proves the definitions and the sensitivity of the cases without a GPU; tests/test_synth_elem_gpu.py runs
the kernels.  Nothing here is taken from a kernel's output.

Every input is float32 (the kernels read exactly what the reference reads) and every definition is evaluated in float64.  The error of
a run is max |got - ref| / max |ref| over the whole output (`rel_err`, as tests/test_ops_gpu.py), or max |got - ref| (`abs_err`) for
iSTFT and the NSF source, whose outputs are bounded by 1.  Every output element is judged.

Inputs.  GroupNorm rows hold N(-0.5, 2^2) (the project's usual inputs) on their valid frames, or N(mean, std^2) in the offset cases
(GN_OFFSETS); the frames behind a row's length hold N(25, 2^2), which a correct kernel never reads; the last batch row of every case
is N(0, 0.01^2) at full length, so that eps inside or outside the root differ by 5 % there.  Ragged STFT rows carry 50.0 behind their
length and the frames behind a ragged iSTFT row's length are as loud as the rest, for the same reason.  Element-wise ops run on N(0, 1.5^2) and, where an op
has a branch, on EDGE_VALUES (Mish across 20, SiLU / ELU at -90, leaky / ELU / ReLU at 0 and +-1e-30, clamp at +-CLAMP_S and the
floats next to it).  Snake runs with alpha in [0.1, 1.1] and x ~ N(0, 2^2), |alpha x| up to about 10: the vocoder's alpha is 1 at
initialisation and its activations are a few units, so the range of the fast sine the kernel uses is covered with margin.

Bounds.  Where tests/test_ops_gpu.py has a bar it is kept: LayerNorm 2e-5, GroupNorm 5e-5, Snake / Mish / ELU 1e-5, the other
element-wise ops 1e-6 (masking and clamping exact), interpolation 1e-5, STFT 1e-5, iSTFT and NSF 2e-5 absolute, embedding exact at
scale 1 (one float32 rounding, 2^-23, with a scale).  Where it has none, the floor is the error of the float32 torch op against the
float64 reference on the cases' own inputs (measured by tests/test_synth_elem_cpu.py, which holds the constants below to the
measurement), plus 2^-11 for a float16 result, and the bound is four times that:
    LayerNorm  float32 floor 1.518e-7 -> LN_F16_TOL 1.9538e-3      GroupNorm float32 floor 1.659e-7 -> GN_F16_TOL 1.9538e-3
    EL_SILU    floor 7.824e-8         -> SILU_TOL 3.2e-7           EL_TANH   floor 3.198e-8        -> TANH_TOL 1.32e-7
Mutation distances are held against the float32 bound of the operator (ten times it): the float16 runs repeat the same cases through
the other store path, every case also runs with float32 output, and it is that run which tells the variants apart.
The offset GroupNorm cases at mean 100, std 0.1 (GN_REPORTED) are printed, not judged.  Errors the kernels showed on one MI355X are in
EXPERIMENTS.md, section Y."""
import functools
import math
import zlib
from collections import namedtuple

import torch

# ---------------------------------------------------------------- the kernels' constants (csrc/ops_norm_elem.hip, csrc/ops_audio.hip)
BLOCK = 256                         # threads per block of every grid-stride kernel
ELEM_GRID_CAP = 2048                # grid_for(): elementwise, interp_linear_rows
AUDIO_GRID_CAP = 4096               # grid_for_a(): nsf_source, stft16, istft16
ELEM_STRIDE = ELEM_GRID_CAP * BLOCK     # 524 288: an element past it is a thread's second trip
AUDIO_STRIDE = AUDIO_GRID_CAP * BLOCK   # 1 048 576
LN_MAX_VEC_C = 2048                 # layernorm_rows: float4 path for c % 4 == 0, c <= 2048, aligned
LN_ROUND = 256                      # 64 lanes x 4 channels per round of the float4 path
LN_ROWS_PER_BLOCK = 4
GN_ROWS = 64                        # rows per chunk of groupnorm_stats / groupnorm_apply
GN_FUSED_TILE_BYTES = 150 * 1024    # groupnorm_fused when t * cpg * 4 <= this
GNF_NT = 512                        # threads of groupnorm_fused; fixed column when GNF_NT % (cpg / 4) == 0
GN_FUSED_Z2_BLOCKS = 256            # gridDim.z = 2 when b * groups * 2 <= this
GN_APPLY_NT = 256                   # groupnorm_apply: float4 columns walk in steps of this
F0_SCAN = 256                       # frames per round of f0_prefix
N_FFT, HOP = 16, 4
MAG_CLIP, AUDIO_LIMIT = 100.0, 0.99

EL_SNAKE, EL_LEAKY, EL_ADD, EL_MUL_ROWMASK, EL_ADD_BC, EL_SCALE, EL_CFG_EULER, EL_MISH, EL_SILU, EL_CLAMP, EL_TANH, EL_ELU, EL_RELU_SCALE = range(13)
EL_NAMES = ("snake", "leaky", "add", "mul_rowmask", "add_bc", "scale", "cfg_euler", "mish", "silu", "clamp", "tanh", "elu", "relu_scale")

# ---------------------------------------------------------------- bounds
F16_EPS = 2.0 ** -11
LN_TOL, GN_TOL = 2e-5, 5e-5
LN_F32_FLOOR = 1.6e-7               # measured: 1.518e-7 (test_synth_elem_cpu.py::test_bounds_follow_the_measured_floors)
GN_F32_FLOOR = 1.75e-7              # measured: 1.659e-7
LN_F16_TOL = 4 * (LN_F32_FLOOR + F16_EPS)
GN_F16_TOL = 4 * (GN_F32_FLOOR + F16_EPS)
SILU_FLOOR, TANH_FLOOR = 8.0e-8, 3.3e-8      # measured: 7.824e-8, 3.198e-8
SILU_TOL, TANH_TOL = 4 * SILU_FLOOR, 4 * TANH_FLOOR
EL_TOL = {EL_SNAKE: 1e-5, EL_MISH: 1e-5, EL_ELU: 1e-5, EL_SILU: SILU_TOL, EL_TANH: TANH_TOL, EL_MUL_ROWMASK: 0.0, EL_CLAMP: 0.0}
EL_TOL.update({op: 1e-6 for op in range(13) if op not in EL_TOL})
EMB_SCALED_TOL = 2.0 ** -23         # one float32 rounding of table * scale
INTERP_TOL, STFT_TOL = 1e-5, 1e-5
ISTFT_ATOL, NSF_ATOL = 2e-5, 2e-5
MUTATION_FACTOR = 10.0


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def abs_err(got, want):
    return float((got.detach().cpu().double() - want.detach().cpu().double()).abs().max())


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


# ================================================================ LayerNorm
LN_C = (1, 4, 63, 80, 252, 256, 260, 513, 1024, 2048, 2052)
LN_ROWS = (1, 4, 5, 37)
LnCase = namedtuple("LnCase", "name rows c")
LN_CASES = tuple(LnCase(f"ln-r{r}-c{c}", r, c) for c in LN_C for r in LN_ROWS)
# through the C entry point: (name, c, ldx - c, ldy - c, which pointer is a view one element into its buffer)
LnRaw = namedtuple("LnRaw", "name rows c dx dy off")
LN_RAW_CASES = (
    LnRaw("ln-raw-ld-vec", 5, 256, 4, 8, None), LnRaw("ln-raw-ld-vec-260", 5, 260, 4, 8, None),
    LnRaw("ln-raw-ldx1", 5, 256, 1, 0, None), LnRaw("ln-raw-x-off", 5, 256, 0, 0, "x"),
    LnRaw("ln-raw-y-off", 5, 256, 0, 0, "y"), LnRaw("ln-raw-gamma-off", 5, 256, 0, 0, "gamma"),
    LnRaw("ln-raw-beta-off", 5, 256, 0, 0, "beta"),
)


def ln_takes_vector_path(c, ldx, ldy, x_al=True, y_al=True, g_al=True, b_al=True):
    return c % 4 == 0 and c <= LN_MAX_VEC_C and ldx % 4 == 0 and ldy % 4 == 0 and x_al and y_al and g_al and b_al


def ln_inputs(case):
    g = _gen(case.name)
    return dict(x=_randn(g, case.rows, case.c) * 3 + 1, gamma=_randn(g, case.c), beta=_randn(g, case.c))


def layernorm(x, gamma, beta, eps=1e-5, relu_scale=0.0):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    return relu_scale * y.clamp_min(0) if relu_scale > 0 else y


# ================================================================ GroupNorm
GnCase = namedtuple("GnCase", "name t c groups lens path offset")
GN_OFFSETS = ((30.0, 0.3), (8.0, 0.5))
GN_REPORTED = ((100.0, 0.1),)
GN_MUTATIONS = ("unbiased", "eps_outside", "stats_t", "group_shift", "add_first", "pad_keep")


def gn_path(b, t, c, groups, aligned=True):
    """The kernel the launcher picks (astts_op_groupnorm) and, inside it, the form of the loop."""
    cpg = c // groups
    if cpg % 4 == 0 and c % 4 == 0 and t * cpg * 4 <= GN_FUSED_TILE_BYTES and aligned:
        walk = "fixed" if GNF_NT % (cpg // 4) == 0 else "walk"
        return f"fused-{walk}-z{2 if b * groups * 2 <= GN_FUSED_Z2_BLOCKS else 1}"
    return "two-vec" if (c % 4 == 0 and cpg % 4 == 0 and aligned) else "two-scalar"


def gn_lens(t, b=None):
    """t, t - 1, 1, 0, t + 5 (clamped), one length inside the first chunk, the chunk edges below t, and t again (the low-variance row)."""
    lens = [t, t - 1, 1, 0, t + 5] + [n for n in (37, GN_ROWS, 2 * GN_ROWS) if n < t] + [t]
    if b is not None:
        lens = [lens[i % (len(lens) - 1)] for i in range(b - 1)] + [t]
    return tuple(lens)


def _gn(t, c, groups, path, b=None, offset=None):
    lens = gn_lens(t, b)
    tag = "" if offset is None else f"-m{offset[0]:g}s{offset[1]:g}"
    case = GnCase(f"gn-t{t}-c{c}-g{groups}-b{len(lens)}{tag}", t, c, groups, lens, path, offset)
    assert gn_path(len(lens), t, c, groups) == path, (case.name, gn_path(len(lens), t, c, groups))
    return case


GN_TWO_LAUNCH_SHAPES = ((481, 80, 1, "two-vec"), (1201, 256, 8, "two-vec"), (131, 12, 2, "two-scalar"), (131, 6, 2, "two-scalar"),
                        (151, 2048, 8, "two-vec"))
GN_PAIR = ((480, 80, 1, "fused-walk-z2"), (481, 80, 1, "two-vec"))
GN_CASES = (
    _gn(37, 8, 2, "fused-fixed-z2"), _gn(70, 256, 8, "fused-fixed-z2"), _gn(131, 128, 2, "fused-fixed-z2"),      # cpg 4, 32, 64
    _gn(131, 80, 1, "fused-walk-z2"), _gn(131, 24, 2, "fused-walk-z2"), _gn(480, 80, 1, "fused-walk-z2"),
    _gn(1, 256, 8, "fused-fixed-z2"), _gn(1, 80, 1, "fused-walk-z2"),
    _gn(37, 32, 8, "fused-fixed-z1", b=17), _gn(131, 96, 8, "fused-walk-z1", b=17),
    _gn(1200, 256, 8, "fused-fixed-z2"),
) + tuple(_gn(*s) for s in GN_TWO_LAUNCH_SHAPES)
GN_OFFSET_CASES = tuple(_gn(t, c, g, p, offset=o) for o in GN_OFFSETS for (t, c, g, p) in GN_TWO_LAUNCH_SHAPES + GN_PAIR[:1])
GN_REPORTED_CASES = tuple(_gn(t, c, g, p, offset=o) for o in GN_REPORTED for (t, c, g, p) in GN_TWO_LAUNCH_SHAPES + GN_PAIR[:1])
GN_MISALIGNED = _gn(131, 256, 8, "fused-fixed-z2")      # run through the C entry point with one pointer a view one element in
GN_VARIANTS = ((False, False), (True, True))            # (mish, add_bc)


@functools.lru_cache(maxsize=4)
def gn_inputs(case):
    g = _gen(case.name)
    b, t, c = len(case.lens), case.t, case.c
    mean, std = (-0.5, 2.0) if case.offset is None else case.offset
    x = _randn(g, b, t, c) * std + mean
    if case.offset is None:
        x[b - 1] = _randn(g, t, c) * 0.01
    for i, n in enumerate(case.lens):
        n = max(0, min(n, t))
        x[i, n:] = _randn(g, t - n, c) * 2 + 25
    return dict(x=x, gamma=_randn(g, c), beta=_randn(g, c), add=_randn(g, b, c), lens=case.lens)


def mish(x):
    return x * torch.tanh(torch.nn.functional.softplus(x, threshold=1e9))


def groupnorm(x, gamma, beta, groups, eps=1e-5, lens=None, use_mish=False, add_bc=None, mutate=None):
    """x [B, T, C] -> float64 [B, T, C]: each row normalised per group over its first clamp(lens[b], 0, T) frames; Mish, then add_bc[b];
    zero behind the length."""
    b, t, c = x.shape
    cpg = c // groups
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    gidx = torch.arange(c) // cpg
    if mutate == "group_shift":
        gidx = ((torch.arange(c) + 1) // cpg).clamp_max(groups - 1)
    out = torch.zeros_like(x)
    for i in range(b):
        n = t if lens is None else max(0, min(int(lens[i]), t))
        n_stat = t if mutate == "stats_t" else n
        n_out = t if mutate == "pad_keep" else n
        if n_out == 0:
            continue
        y = torch.zeros(n_out, c, dtype=torch.float64)
        for gi in range(groups):
            sel = gidx == gi
            v = x[i, :n_stat][:, sel]
            cnt = v.numel()
            mean = v.mean() if cnt else torch.tensor(0.0, dtype=torch.float64)
            var = ((v - mean) ** 2).sum() / (cnt - 1 if mutate == "unbiased" and cnt > 1 else max(cnt, 1))
            rstd = 1.0 / (torch.sqrt(var) + eps) if mutate == "eps_outside" else 1.0 / torch.sqrt(var + eps)
            y[:, sel] = (x[i, :n_out][:, sel] - mean) * rstd
        y = y * gamma + beta
        if mutate == "add_first" and add_bc is not None:
            y = y + add_bc[i].double()
        if use_mish:
            y = mish(y)
        if mutate != "add_first" and add_bc is not None:
            y = y + add_bc[i].double()
        out[i, :n_out] = y
    return out


def gn_bears(case, mutation, use_mish, add):
    t, cl = case.t, [max(0, min(n, case.t)) for n in case.lens]
    return {"unbiased": any(0 < n * (case.c // case.groups) <= 256 for n in cl), "eps_outside": case.offset is None,
            "stats_t": any(0 < n < t for n in cl), "group_shift": case.groups > 1, "add_first": use_mish and add,
            "pad_keep": any(n < t for n in cl)}[mutation]


@functools.lru_cache(maxsize=8)
def gn_expected(case, use_mish, add):
    d = gn_inputs(case)
    return groupnorm(d["x"], d["gamma"], d["beta"], case.groups, 1e-5, d["lens"], use_mish, d["add"] if add else None)


# ================================================================ element-wise family
CLAMP_S, LEAKY_S, ADD_S, SCALE_S, RELU_S, CFG_DT, CFG_R = 0.99, 0.1, 1.0 / 3.0, 22.6, 32.0, 0.07, 0.7
TINY = 1e-30
_F = lambda v: float(torch.tensor(v, dtype=torch.float32))
EDGE_VALUES = (-90.0, -20.0, -1.0, -TINY, -0.0, 0.0, TINY, 1.0, 19.5, _F(19.999), 20.0, _F(20.001), 20.5,
               _F(CLAMP_S), -_F(CLAMP_S), float(torch.nextafter(torch.tensor(CLAMP_S, dtype=torch.float32), torch.tensor(2.0))),
               float(torch.nextafter(torch.tensor(CLAMP_S, dtype=torch.float32), torch.tensor(0.0))),
               -float(torch.nextafter(torch.tensor(CLAMP_S, dtype=torch.float32), torch.tensor(2.0))))
EL_EDGE_OPS = (EL_LEAKY, EL_SCALE, EL_MISH, EL_SILU, EL_CLAMP, EL_TANH, EL_ELU, EL_RELU_SCALE)
ElCase = namedtuple("ElCase", "name b t c")
EL_CASES = tuple(ElCase(f"el-c{c}", 2, 33, c) for c in (1, 80, 128)) + (ElCase("el-stride", 2, 1030, 256),)
EL_EDGE_CASE = ElCase("el-edges", 1, len(EDGE_VALUES), 1)
assert EL_CASES[-1].b * EL_CASES[-1].t * EL_CASES[-1].c == 527360 > ELEM_STRIDE


@functools.lru_cache(maxsize=2)
def el_inputs(case):
    g = _gen(case.name)
    b, t, c = case.b, case.t, case.c
    if case.name == "el-edges":
        x = torch.tensor(EDGE_VALUES, dtype=torch.float32).view(1, -1, 1)
    else:
        x = _randn(g, b, t, c) * 1.5
    lens = tuple([t - 13, t] + [max(t // 2, 1)] * (b - 2))[:b]
    return dict(x=x, z=_randn(g, 2 * b, t, c), alpha=torch.rand(c, generator=g) + 0.1, bc=_randn(g, b, c), lens=lens)


def el_args(op, d):
    """Keyword arguments of astts.ops.elementwise / `elementwise` below for ``op`` on the inputs ``d`` (tensors still on the CPU)."""
    b = d["x"].shape[0]
    return {EL_SNAKE: dict(p0=d["alpha"]), EL_LEAKY: dict(s=LEAKY_S), EL_ADD: dict(z=d["z"][:b].contiguous(), s=ADD_S),
            EL_MUL_ROWMASK: dict(lens=d["lens"]), EL_ADD_BC: dict(p0=d["bc"]), EL_SCALE: dict(s=SCALE_S),
            EL_CFG_EULER: dict(z=d["z"], s=CFG_DT, s2=CFG_R), EL_CLAMP: dict(s=CLAMP_S), EL_RELU_SCALE: dict(s=RELU_S)}.get(op, {})


def elementwise(op, x, z=None, p0=None, lens=None, s=0.0, s2=0.0, mutate=None):
    b, t, c = x.shape
    x = x.double()
    s, s2 = _F(s), _F(s2)                 # the kernel receives float32 scalars
    if op == EL_SNAKE:
        al = p0.double()
        return x + torch.sin(al * x) ** 2 / (al + 1e-9)
    if op == EL_LEAKY:
        return torch.where(x > 0, x, x * s)
    if op == EL_ADD:
        return x + s * z.double()
    if op == EL_MUL_ROWMASK:
        keep = torch.arange(t)[None, :] < torch.tensor(lens)[:, None]
        return x * keep[..., None]
    if op == EL_ADD_BC:
        return x + p0.double()[:, None, :]
    if op == EL_SCALE:
        return s * x
    if op == EL_CFG_EULER:
        zc, zu = z[:b].double(), z[b:].double()
        return x + s * ((1 - s2) * zc + s2 * zu) if mutate == "cfg_sign" else x + s * ((1 + s2) * zc - s2 * zu)
    if op == EL_MISH:
        return mish(x)
    if op == EL_SILU:
        return x * torch.sigmoid(x)
    if op == EL_CLAMP:
        return x.clamp(-s, s)
    if op == EL_TANH:
        return torch.tanh(x)
    if op == EL_ELU:
        return torch.where(x > 0, x, torch.expm1(x))
    if op == EL_RELU_SCALE:
        return s * x.clamp_min(0)
    raise ValueError(op)


# ================================================================ embedding
EMB_VOCAB = 37
EMB_ROWS, EMB_C, EMB_SCALES = (1, 5, 150), (1, 80, 512), (1.0, 22.6)
EMB_EDGE_IDS = (-1, EMB_VOCAB, 0, EMB_VOCAB - 1)


def emb_inputs(rows, c):
    g = _gen(f"emb-{rows}-{c}")
    ids = torch.randint(0, EMB_VOCAB, (rows,), generator=g, dtype=torch.int32)
    edge = torch.tensor(EMB_EDGE_IDS, dtype=torch.int32)
    ids[:min(rows, 4)] = edge[(torch.arange(min(rows, 4)) + EMB_C.index(c)) % 4]      # a single row takes another edge id for every c
    return dict(table=_randn(g, EMB_VOCAB, c), ids=ids)


def embedding(table, ids, scale=1.0):
    return table.double()[ids.long().clamp(0, table.shape[0] - 1)] * _F(scale)


# ================================================================ linear interpolation
InterpCase = namedtuple("InterpCase", "name b t_in t_out c in_lens out_lens")
INTERP_CASES = tuple(InterpCase(f"interp-{ti}-{to}", 2, ti, to, 80, None, None)
                     for ti, outs in ((1, (1, 5)), (2, (1, 2, 7)), (150, (75, 150, 258, 430))) for to in outs) + (
    InterpCase("interp-ragged", 5, 150, 430, 80, (150, 1, 97, 40, 150), (430, 200, 0, 113, 1)),
    InterpCase("interp-stride", 2, 150, 3300, 80, None, None),
)
assert 2 * 3300 * 80 == 528000 > ELEM_STRIDE


def interp_inputs(case):
    return _randn(_gen(case.name), case.b, case.t_in, case.c)


def interp_linear(x, t_out, in_lens=None, out_lens=None, mutate=None):
    """Half-pixel linear resampling (F.interpolate, align_corners=False) of each row from its own length to its own length."""
    b, t_in_max, c = x.shape
    x = x.double()
    out = torch.zeros(b, t_out, c, dtype=torch.float64)
    for i in range(b):
        ti = t_in_max if in_lens is None else min(in_lens[i], t_in_max)
        to = t_out if out_lens is None else min(out_lens[i], t_out)
        if mutate == "from_t_max":
            ti = t_in_max
        if to < 1 or ti < 1:
            continue
        o = torch.arange(to, dtype=torch.float64)
        if mutate == "align_corners":
            src = o * ((ti - 1) / (to - 1)) if to > 1 else torch.zeros(1, dtype=torch.float64)
        else:
            src = ((o + 0.5) * ti / to - 0.5).clamp_min(0)
        i0 = src.floor().long().clamp_max(ti - 1)
        i1 = (i0 + 1).clamp_max(ti - 1)
        w = (src - i0)[:, None]
        out[i, :to] = x[i, i0] * (1 - w) + x[i, i1] * w
    return out


# ================================================================ STFT(16, 4, periodic Hann, reflect) / the HiFT iSTFT head
StftCase = namedtuple("StftCase", "name b n lens")
STFT_BIG_N = 2097168
STFT_CASES = (StftCase("stft-16", 2, 16, None), StftCase("stft-20", 2, 20, None), StftCase("stft-2560", 2, 2560, None),
              StftCase("stft-ragged", 6, 2560, (2560, 16, 20, 1284, 2556, 1024)), StftCase("stft-stride", 2, STFT_BIG_N, None))
assert 2 * (STFT_BIG_N // HOP + 1) > AUDIO_STRIDE
STFT_PAD_VALUE = 50.0


def stft_inputs(case):
    x = _randn(_gen(case.name), case.b, case.n)
    for i, n in enumerate(case.lens or ()):
        x[i, n:] = STFT_PAD_VALUE
    return x


def _hann():
    return 0.5 - 0.5 * torch.cos(2 * math.pi * torch.arange(N_FFT, dtype=torch.float64) / N_FFT)


def _dft_basis():
    k = torch.arange(N_FFT // 2 + 1, dtype=torch.float64)[None, :]
    n = torch.arange(N_FFT, dtype=torch.float64)[:, None]
    ang = 2 * math.pi * k * n / N_FFT
    return torch.cat([torch.cos(ang), -torch.sin(ang)], dim=1)          # [16, 18]: re[0..8], im[0..8]


def stft16(x, lens=None, mutate=None):
    """x [B, L] -> float64 [B, L / 4 + 1, 18]; row b is a signal of lens[b] samples: its first lens[b] / 4 + 1 frames, zeros behind."""
    b, lmax = x.shape
    out = torch.zeros(b, lmax // HOP + 1, 18, dtype=torch.float64)
    basis = _dft_basis() * _hann()[:, None]
    for i in range(b):
        n = lmax if lens is None else min(lens[i], lmax)
        nf = n // HOP + 1
        sig = x[i].double()
        pos = torch.arange(-N_FFT // 2, n + N_FFT // 2)
        refl = lmax if mutate == "reflect_padded" else n
        pos = pos.abs()
        pos = torch.where(pos >= refl, 2 * (refl - 1) - pos, pos)
        frames = sig[pos].unfold(0, N_FFT, HOP)[:nf]
        out[i, :nf] = frames @ basis
    return out


IstftCase = namedtuple("IstftCase", "name b frames frame_lens")
ISTFT_BIG_FRAMES = 131074
ISTFT_CASES = (IstftCase("istft-2", 16, 2, None), IstftCase("istft-3", 16, 3, None), IstftCase("istft-641", 2, 641, None),
               IstftCase("istft-ragged", 6, 641, (641, 1, 2, 3, 320, 640)), IstftCase("istft-stride", 2, ISTFT_BIG_FRAMES, None))
assert 2 * HOP * (ISTFT_BIG_FRAMES - 1) > AUDIO_STRIDE


def istft_inputs(case):
    """Pre-activations N(0, 0.5^2) as the existing test; one frame in 16 is quiet (N(-3, 0.3^2)), so that its samples stay inside the
    clamp, and every 7th of all log-magnitudes is raised: to 4.7 .. 6.2 (past log(100) = 4.6, the clip) or to 1.5 .. 2.5 (loud)."""
    g = _gen(case.name)
    y = _randn(g, case.b, case.frames, 18) * 0.5
    quiet = (torch.arange(case.frames) % 16) == 5
    y[:, quiet, :9] = _randn(g, case.b, int(quiet.sum()), 9) * 0.3 - 3.0
    flat = y[..., :9].reshape(-1)
    idx = torch.arange(0, flat.numel(), 7)
    hot = torch.rand(idx.numel(), generator=g)
    y[..., :9] = flat.index_copy(0, idx, torch.where(hot < 0.5, 4.7 + 3.0 * hot, 1.0 + hot)).view(case.b, case.frames, 9)
    return y


def istft16(y, mag_clip=MAG_CLIP, audio_limit=AUDIO_LIMIT, frame_lens=None, mutate=None):
    """y [B, F, 18] -> float64 [B, 4 (F - 1)]: magnitude min(exp(y[..., :9]), mag_clip), phase sin(y[..., 9:]), inverse real DFT, Hann
    window, overlap-add over the row's own frames / the overlapped squared window, centre trimmed, clamp; zeros behind the row."""
    b, fmax, _ = y.shape
    y = y.double()
    out = torch.zeros(b, HOP * (fmax - 1), dtype=torch.float64)
    win = _hann()
    for i in range(b):
        nf = fmax if frame_lens is None else min(frame_lens[i], fmax)
        if nf < 2:
            continue
        n_ola = fmax if mutate == "ola_sees_padding" else nf
        mag = torch.exp(y[i, :n_ola, :9])
        if mutate != "unclipped":
            mag = mag.clamp_max(mag_clip)
        ph = torch.sin(y[i, :n_ola, 9:])
        spec = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))
        fr = torch.fft.irfft(spec, n=N_FFT, dim=-1) * win                  # [F, 16]
        total = N_FFT + HOP * (n_ola - 1)
        num, den = torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
        idx = (torch.arange(n_ola)[:, None] * HOP + torch.arange(N_FFT)[None, :]).reshape(-1)
        num.index_add_(0, idx, fr.reshape(-1))
        den.index_add_(0, idx, (win * win).repeat(n_ola))
        n = HOP * (nf - 1)
        wav = num[N_FFT // 2:N_FFT // 2 + n] / den[N_FFT // 2:N_FFT // 2 + n]
        out[i, :n] = wav.clamp(-audio_limit, audio_limit)
    return out


# ================================================================ NSF source
NsfCase = namedtuple("NsfCase", "name b tm up")
NSF_SR, NSF_AMP, NSF_SIGMA, NSF_THR, NSF_NH = 22050.0, 0.1, 0.003, 10.0, 9
NSF_CASES = tuple(NsfCase(f"nsf-tm{tm}", 2, tm, 256) for tm in (1, 255, 256, 257)) + (
    NsfCase("nsf-stride", 8, 513, 256), NsfCase("nsf-up480", 2, 257, 480))
assert 8 * 513 * 256 == 1050624 > AUDIO_STRIDE
NSF_THR_FRAME = 13
NSF_MUTATIONS = ("inclusive_prefix", "prefix_restart", "voiced_ge", "harmonic_zero_based")


def nsf_inputs(case):
    """f0 in 80 .. 380 Hz; unvoiced stretches (f0 = 0) across each 256-frame edge in odd rows and voiced across it in even rows; frames
    NSF_THR_FRAME + 32 k sit exactly on the voiced threshold."""
    g = _gen(case.name)
    b, tm, up = case.b, case.tm, case.up
    f0 = torch.rand(b, tm, generator=g) * 300 + 80
    f = torch.arange(tm)
    f0[:, (f % 32) == NSF_THR_FRAME] = NSF_THR
    for i in range(b):
        if i % 2 == 1:
            f0[i, ((f % F0_SCAN) >= F0_SCAN - 6) | ((f % F0_SCAN) < 4) & (f >= F0_SCAN)] = 0.0
        else:
            f0[i, (f % 64) == 20 + i] = 0.0
    phase0 = (torch.rand(b, NSF_NH, generator=g) * 2 - 1) * math.pi
    phase0[:, 0] = 0
    return dict(f0=f0, phase0=phase0, noise=_randn(g, b, tm * up, NSF_NH), lin_w=_randn(g, NSF_NH) * 0.3, lin_b=_randn(g, 1) * 0.1)


def nsf_source(f0, phase0, noise, lin_w, lin_b, up, sr=NSF_SR, amp=NSF_AMP, sigma=NSF_SIGMA, thr=NSF_THR, mutate=None):
    """-> float64 [B, Tm up]: tanh(sum_h w_h (amp sin(2 pi frac(h cumsum(f0 / sr)) + phase0_h) uv + namp noise_h) + bias)."""
    b, tm = f0.shape
    nh = phase0.shape[1]
    f0d = f0.double()
    pre = torch.cumsum(f0d, 1) - f0d                                       # exclusive prefix over frames
    if mutate == "inclusive_prefix":
        pre = torch.cumsum(f0d, 1)
    if mutate == "prefix_restart":
        pre = torch.cat([torch.cumsum(ch, 1) - ch for ch in f0d.split(F0_SCAN, dim=1)], dim=1)
    r = torch.arange(1, up + 1, dtype=torch.float64)
    cum = ((pre * up)[..., None] + f0d[..., None] * r).reshape(b, tm * up) / sr
    harm = torch.arange(0 if mutate == "harmonic_zero_based" else 1, nh + (0 if mutate == "harmonic_zero_based" else 1), dtype=torch.float64)
    f0u = f0d.repeat_interleave(up, dim=1)
    uv = ((f0u >= thr) if mutate == "voiced_ge" else (f0u > thr)).double()[..., None]
    src = torch.sin(2 * math.pi * torch.remainder(cum[..., None] * harm, 1.0) + phase0.double()[:, None, :])
    src = src.mul_(amp).mul_(uv).add_((uv * sigma + (1 - uv) * amp / 3) * noise.double())
    return torch.tanh(src @ lin_w.double() + lin_b.double())
