"""GPU side of the norm / element-wise / vocoder-signal suite: layernorm_rows, groupnorm_fused, groupnorm_stats + groupnorm_apply,
elementwise, embedding_rows and interp_linear_rows of csrc/ops_norm_elem.hip and f0_prefix / nsf_source, stft16 and istft16 of
csrc/ops_audio.hip against the float64 definitions, the cases and the bounds of tests/synth_elem_ref.py.  Every output element is
judged, padding must be exactly zero, the gap columns of a strided output must keep their sentinel.  The bounds come from the reference
side (tests/test_synth_elem_cpu.py): the bars of tests/test_ops_gpu.py where it has one (LayerNorm 2e-5, GroupNorm 5e-5, Snake / Mish /
ELU 1e-5, other element-wise ops 1e-6 or exact, interpolation and STFT 1e-5, iSTFT and NSF 2e-5 absolute), four times the measured
float32 floor (+ 2^-11 for float16 results) where it has none: LayerNorm fp16 and GroupNorm fp16 1.954e-3, EL_SILU 3.2e-7, EL_TANH
1.32e-7.  Each test prints one [parity] line.  Worst errors one MI355X showed (EXPERIMENTS.md, section Y): LayerNorm 1.7e-7 (fp16 out
4.4e-4), GroupNorm 1.3e-6 (fp16 out 4.2e-4; offset inputs 3.5e-6; t = 480 against t = 481 2.1e-6), Snake 1.2e-7, Mish 9.4e-8, ELU
1.6e-8, SiLU 7.8e-8, tanh 8.0e-8, the other element-wise ops <= 5.7e-8, embedding with a scale 5.6e-8, interpolation 1.3e-7, STFT
2.0e-7, iSTFT 4.8e-6 absolute, NSF source 6.6e-8 absolute; masking, clamping and the unscaled embedding exact."""
import math

import pytest
import torch

import synth_elem_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = torch.float16, torch.float32
SENTINEL = 777.0


def _i32(x):
    return None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)


def _off(t):
    """The same values in a view one element into its buffer (4 bytes off for float32, 2 for float16)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


class _Worst:
    def __init__(self, label, bound):
        self.label, self.bound, self.worst, self.where, self.failed, self.n = label, bound, 0.0, None, [], 0

    def add(self, err, where, bound=None):
        bound = self.bound if bound is None else bound
        self.n += 1
        if err > self.worst or self.where is None:
            self.worst, self.where = err, where
        if not err <= bound:
            self.failed.append((where, f"{err:.3e} > {bound:.3e}"))

    def done(self):
        print(f"[parity] {self.label}: worst err {self.worst:.3e} (bound {self.bound:.3e}) at {self.where}, {self.n} runs")
        assert not self.failed, self.failed[:10]


def _zero_behind(got, valid, name):
    for i, n in enumerate(valid):
        if n < got.shape[1]:
            assert float(got[i, n:].abs().max()) == 0.0, (name, i, "padding is not zero")


# ================================================================ LayerNorm
def test_layernorm_every_path_and_both_outputs():
    """c on both sides of the float4 conditions (c % 4, c <= 2048) and of a 256-channel round, rows around the four of a block, float32
    and float16 output, plain and relu_scale = sqrt(c)."""
    from astts import ops

    w32, w16 = _Worst("layernorm fp32 out", ref.LN_TOL), _Worst("layernorm fp16 out", ref.LN_F16_TOL)
    for case in ref.LN_CASES:
        d = ref.ln_inputs(case)
        x, ga, be = (d[k].to(DEV) for k in ("x", "gamma", "beta"))
        for rs in (0.0, math.sqrt(case.c)):
            want = ref.layernorm(d["x"], d["gamma"], d["beta"], 1e-5, rs)
            for dt, w in ((F32, w32), (F16, w16)):
                got = ops.layernorm(x, ga, be, 1e-5, out_dtype=dt, relu_scale=rs)
                assert got.dtype == dt and got.shape == x.shape
                w.add(ref.rel_err(got, want), (case.name, rs))
    w32.done()
    w16.done()


def _ln_raw(case, out_dtype, data):
    from astts import _lib

    ldx, ldy = case.c + case.dx, case.c + case.dy
    xb = torch.full((case.rows, ldx), SENTINEL, device=DEV)
    xb[:, :case.c] = data["x"].to(DEV)
    x = _off(xb) if case.off == "x" else xb
    ga = _off(data["gamma"].to(DEV)) if case.off == "gamma" else data["gamma"].to(DEV)
    be = _off(data["beta"].to(DEV)) if case.off == "beta" else data["beta"].to(DEV)
    yb = torch.full((case.rows, ldy), SENTINEL, dtype=out_dtype, device=DEV)
    y = _off(yb) if case.off == "y" else yb
    al = lambda t, n=16: t.data_ptr() % n == 0
    vec = ref.ln_takes_vector_path(case.c, ldx, ldy, al(x), al(y, 8 if out_dtype == F16 else 16), al(ga), al(be))
    assert vec == (case.off is None and case.dx % 4 == 0), (case.name, vec)
    _lib.check(_lib.load().astts_op_layernorm(x.data_ptr(), ga.data_ptr(), be.data_ptr(), y.data_ptr(), 1 if out_dtype == F16 else 0,
                                              case.rows, case.c, ldx, ldy, 1e-5, 0.0, _lib.stream_ptr()))
    y = y.cpu()
    assert bool((y[:, case.c:] == SENTINEL).all()), (case.name, "gap columns were written")
    return y[:, :case.c]


def test_layernorm_strides_and_views_through_the_c_entry_point():
    """ldx = c + 4 with ldy = c + 8 (float4 path; c = 260 ends in a partial round), ldx = c + 1 and x a view one float into its buffer
    (scalar path); then y, gamma and beta one element into theirs, which the float4 path must refuse: same result as the aligned run
    (two float32 results inside the bar of each other; two float16 results at most one float16 step, 2^-10 of the value, apart)."""
    from astts import ops

    w32, w16 = _Worst("layernorm (C entry) fp32 out", ref.LN_TOL), _Worst("layernorm (C entry) fp16 out", ref.LN_F16_TOL)
    for case in ref.LN_RAW_CASES:
        d = ref.ln_inputs(case)
        want = ref.layernorm(d["x"], d["gamma"], d["beta"], 1e-5)
        for dt, w in ((F32, w32), (F16, w16)):
            got = _ln_raw(case, dt, d)
            w.add(ref.rel_err(got, want), case.name)
            if case.off:
                aligned = ops.layernorm(d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV), 1e-5, out_dtype=dt).cpu()
                w.add(ref.rel_err(got, aligned.double()), (case.name, "vs aligned"), ref.LN_TOL if dt == F32 else 2 * ref.F16_EPS)
    w32.done()
    w16.done()


# ================================================================ GroupNorm
def _gn_run(case, use_mish, add, out_dtype, d=None):
    from astts import ops

    d = ref.gn_inputs(case) if d is None else d
    got = ops.groupnorm(d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV), case.groups, 1e-5, lens=_i32(d["lens"]), mish=use_mish,
                        add_bc=d["add"].to(DEV) if add else None, out_dtype=out_dtype)
    assert got.dtype == out_dtype and got.shape == d["x"].shape
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), case.name
    _zero_behind(got, [max(0, min(n, case.t)) for n in d["lens"]], case.name)
    return got


def test_groupnorm_every_path_of_the_launcher():
    """Fused kernel (fixed and walking column, gridDim.z 2 and 1, t = 1, t odd, the last t that fits) and the two-launch path (tile
    size, cpg % 4 != 0, c = 2048) with lens t, t - 1, 1, 0, t + 5, inside the first chunk and on the chunk edges; plain and with Mish
    and add_bc; float32 and float16 output."""
    w32, w16 = _Worst("groupnorm fp32 out", ref.GN_TOL), _Worst("groupnorm fp16 out", ref.GN_F16_TOL)
    for case in ref.GN_CASES:
        for use_mish, add in ref.GN_VARIANTS:
            want = ref.gn_expected(case, use_mish, add)
            for dt, w in ((F32, w32), (F16, w16)):
                w.add(ref.rel_err(_gn_run(case, use_mish, add, dt), want), (case.name, case.path, use_mish))
    w32.done()
    w16.done()


def test_groupnorm_two_launch_path_on_offset_inputs():
    """mean 30 / std 0.3 and mean 8 / std 0.5 at every two-launch shape and at t = 480 (fused): the statistics must not be formed as
    E[x^2] - mean^2 from float32 sums (1e-3 of the output at mean 30).  mean 100 / std 0.1 is printed, not judged."""
    w = _Worst("groupnorm offset inputs", ref.GN_TOL)
    for case in ref.GN_OFFSET_CASES:
        for use_mish, add in ref.GN_VARIANTS:
            w.add(ref.rel_err(_gn_run(case, use_mish, add, F32), ref.gn_expected(case, use_mish, add)), (case.name, case.path, use_mish))
    for case in ref.GN_REPORTED_CASES:
        err = ref.rel_err(_gn_run(case, False, False, F32), ref.gn_expected(case, False, False))
        print(f"[reported] groupnorm {case.name} ({case.path}): err {err:.3e} (not judged)")
    w.done()


def test_groupnorm_fused_and_two_launch_agree_across_the_tile_limit():
    """The same 480 frames normalised inside a t = 480 batch (fused) and inside a t = 481 batch with lens = 480 (two launches)."""
    assert ref.gn_path(4, *ref.GN_PAIR[0][:3]) == "fused-walk-z2" and ref.gn_path(4, *ref.GN_PAIR[1][:3]) == "two-vec"
    w = _Worst("groupnorm t = 480 vs t = 481", ref.GN_TOL)
    for offset in (None,) + ref.GN_OFFSETS:
        g = ref._gen(f"gn-pair-{offset}")
        mean, std = (-0.5, 2.0) if offset is None else offset
        x481 = ref._randn(g, 4, 481, 80) * std + mean
        small = ref.GnCase("gn-pair-480", 480, 80, 1, (480,) * 4, "fused-walk-z2", offset)
        large = ref.GnCase("gn-pair-481", 481, 80, 1, (480,) * 4, "two-vec", offset)
        d = dict(gamma=ref._randn(g, 80), beta=ref._randn(g, 80), add=ref._randn(g, 4, 80), lens=(480,) * 4)
        a = _gn_run(small, True, True, F32, dict(d, x=x481[:, :480].contiguous()))
        b = _gn_run(large, True, True, F32, dict(d, x=x481))
        want = ref.groupnorm(x481[:, :480], d["gamma"], d["beta"], 1, 1e-5, None, True, d["add"])
        w.add(ref.rel_err(a, want), ("fused", offset))
        w.add(ref.rel_err(b[:, :480], want), ("two-launch", offset))
        w.add(float((a.double() - b[:, :480].double()).abs().max() / want.abs().max()), ("difference", offset))
    w.done()


def test_groupnorm_views_through_the_c_entry_point():
    """x, y, gamma, beta or add_bc a view one element into its buffer: the launcher leaves the fused kernel and groupnorm_apply its
    float4 form; the result is the aligned one."""
    from astts import _lib

    case = ref.GN_MISALIGNED
    d = ref.gn_inputs(case)
    b, t, c = d["x"].shape
    lib = _lib.load()
    want = ref.gn_expected(case, True, True)
    w32, w16 = _Worst("groupnorm (C entry) fp32 out", ref.GN_TOL), _Worst("groupnorm (C entry) fp16 out", ref.GN_F16_TOL)
    lens = _i32(d["lens"])
    for dt, w in ((F32, w32), (F16, w16)):
        aligned = _gn_run(case, True, True, dt)
        for which in ("x", "y", "gamma", "beta", "add"):
            t_ = {k: (_off(d[k].to(DEV)) if k == which else d[k].to(DEV)) for k in ("x", "gamma", "beta", "add")}
            ybuf = torch.full((b * t * c + 2,), SENTINEL, dtype=dt, device=DEV)
            y = ybuf[1:-1] if which == "y" else ybuf[:-2]
            al = all(v.data_ptr() % 16 == 0 for v in t_.values()) and y.data_ptr() % (8 if dt == F16 else 16) == 0
            assert ref.gn_path(b, t, c, case.groups, aligned=al) == "two-scalar", which
            need = int(lib.astts_op_groupnorm_workspace_bytes(b, t, case.groups))
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            _lib.check(lib.astts_op_groupnorm(t_["x"].data_ptr(), lens.data_ptr(), t_["gamma"].data_ptr(), t_["beta"].data_ptr(),
                                              t_["add"].data_ptr(), y.data_ptr(), 1 if dt == F16 else 0, b, t, c, case.groups, 1e-5, 1,
                                              ws.data_ptr(), need, _lib.stream_ptr()))
            got = y.view(b, t, c).cpu()
            edge = ybuf.cpu()
            assert float(edge[-1]) == SENTINEL and float(edge[0 if which == "y" else -2]) == SENTINEL, (which, "wrote outside y")
            _zero_behind(got, [max(0, min(n, t)) for n in d["lens"]], which)
            w.add(ref.rel_err(got, want), which)
            w.add(ref.rel_err(got, aligned.double()), (which, "vs aligned"), ref.GN_TOL if dt == F32 else 2 * ref.F16_EPS)
    w32.done()
    w16.done()


# ================================================================ element-wise family
def test_elementwise_all_ops_branch_points_and_the_second_grid_trip():
    """All thirteen ops at c = 1, 80, 128 and on (2, 1030, 256) = 527 360 elements (past the 2048 x 256 threads of the launch);
    the ops with a branch also on the values around it."""
    from astts import ops

    w = {op: _Worst(f"elementwise {ref.EL_NAMES[op]}", ref.EL_TOL[op]) for op in range(13)}
    for case in ref.EL_CASES + (ref.EL_EDGE_CASE,):
        d = ref.el_inputs(case)
        x = d["x"].to(DEV)
        for op in (ref.EL_EDGE_OPS if case is ref.EL_EDGE_CASE else range(13)):
            kw = ref.el_args(op, d)
            want = ref.elementwise(op, d["x"], **kw)
            dev_kw = {k: (_i32(v) if k == "lens" else v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
            got = ops.elementwise(op, x, **dev_kw).cpu()
            assert got.shape == want.shape and bool(torch.isfinite(got).all()), (case.name, op)
            w[op].add(ref.rel_err(got, want), case.name)
            if op == ref.EL_MUL_ROWMASK:
                _zero_behind(got, d["lens"], case.name)
    for op in range(13):
        w[op].done()


# ================================================================ embedding, interpolation
def test_embedding_clamps_ids_scales_and_keeps_the_row_stride():
    from astts import _lib, ops

    exact, scaled = _Worst("embedding scale 1", 0.0), _Worst("embedding scale 22.6", ref.EMB_SCALED_TOL)
    for rows in ref.EMB_ROWS:
        for c in ref.EMB_C:
            d = ref.emb_inputs(rows, c)
            tab, ids = d["table"].to(DEV), d["ids"].to(DEV)
            for scale, w in zip(ref.EMB_SCALES, (exact, scaled)):
                want = ref.embedding(d["table"], d["ids"], scale)
                w.add(ref.rel_err(ops.embedding(tab, ids, scale), want), (rows, c))
                y = torch.full((rows, c + 3), SENTINEL, device=DEV)
                _lib.check(_lib.load().astts_op_embedding(tab.data_ptr(), ids.data_ptr(), y.data_ptr(), rows, c, c + 3, ref.EMB_VOCAB, scale,
                                                          _lib.stream_ptr()))
                y = y.cpu()
                assert bool((y[:, c:] == SENTINEL).all()), (rows, c, "gap columns were written")
                w.add(ref.rel_err(y[:, :c], want), (rows, c, "ldy = c + 3"))
    exact.done()
    scaled.done()


def test_interp_linear_uniform_ragged_and_the_second_grid_trip():
    from astts import ops

    w = _Worst("interp_linear", ref.INTERP_TOL)
    for case in ref.INTERP_CASES:
        x = ref.interp_inputs(case)
        want = ref.interp_linear(x, case.t_out, case.in_lens, case.out_lens)
        got = ops.interp_linear(x.to(DEV), case.t_out, _i32(case.in_lens), _i32(case.out_lens)).cpu()
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), case.name
        if case.out_lens:
            _zero_behind(got, case.out_lens, case.name)
        w.add(ref.rel_err(got, want), case.name)
    w.done()


# ================================================================ STFT, iSTFT, NSF source
def test_stft16_shortest_signals_ragged_rows_and_the_second_grid_trip():
    from astts import ops

    w = _Worst("stft16", ref.STFT_TOL)
    for case in ref.STFT_CASES:
        x = ref.stft_inputs(case)
        want = ref.stft16(x, case.lens)
        got = ops.stft16(x.to(DEV), _i32(case.lens)).cpu()
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), case.name
        if case.lens:
            _zero_behind(got, [n // 4 + 1 for n in case.lens], case.name)
        w.add(ref.rel_err(got, want), case.name)
    w.done()


def test_istft16_clip_clamp_ragged_rows_and_the_second_grid_trip():
    from astts import ops

    w = _Worst("istft16 (absolute)", ref.ISTFT_ATOL)
    for case in ref.ISTFT_CASES:
        y = ref.istft_inputs(case)
        want = ref.istft16(y, frame_lens=case.frame_lens)
        got = ops.istft16(y.to(DEV), ref.MAG_CLIP, ref.AUDIO_LIMIT, _i32(case.frame_lens)).cpu()
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), case.name
        if case.frame_lens:
            _zero_behind(got, [4 * (n - 1) for n in case.frame_lens], case.name)
        w.add(ref.abs_err(got, want), case.name)
    w.done()


def test_nsf_source_prefix_carry_threshold_and_the_second_grid_trip():
    from astts import ops

    w = _Worst("nsf_source (absolute)", ref.NSF_ATOL)
    for case in ref.NSF_CASES:
        d = ref.nsf_inputs(case)
        want = ref.nsf_source(up=case.up, **d)
        got = ops.nsf_source(d["f0"].to(DEV), d["phase0"].to(DEV), d["noise"].to(DEV), d["lin_w"].to(DEV), d["lin_b"].to(DEV), case.up,
                             ref.NSF_SR, ref.NSF_AMP, ref.NSF_SIGMA, ref.NSF_THR).cpu()
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), case.name
        w.add(ref.abs_err(got, want), case.name)
    w.done()
