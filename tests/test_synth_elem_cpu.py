"""CPU side of the norm / element-wise / vocoder-signal suite (tests/synth_elem_ref.py): the float64 definitions against torch's own
operators (F.layer_norm, F.group_norm, F.mish, F.interpolate, torch.stft, torch.istft), oracle.synth.hift_source and rows done by hand;
the case lists against the kernels' constants; the sensitivity of every case's inputs to the wrong variants that bear on it (a judged
output moves by >= MUTATION_FACTOR x the operator's bound); and the bounds that have no earlier bar against the floors measured here.
Nothing here needs a GPU or the native library."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

import synth_elem_ref as ref

F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------- the definitions
def test_layernorm_matches_torch_and_a_hand_row():
    for case in ref.LN_CASES:
        d = ref.ln_inputs(case)
        want = F.layer_norm(d["x"].double(), (case.c,), d["gamma"].double(), d["beta"].double(), 1e-5)
        got = ref.layernorm(d["x"], d["gamma"], d["beta"], 1e-5)
        assert ref.rel_err(got, want) < 1e-12, case.name
        rs = math.sqrt(case.c)
        assert ref.rel_err(ref.layernorm(d["x"], d["gamma"], d["beta"], 1e-5, rs), rs * want.clamp_min(0)) < 1e-12, case.name
    x = torch.tensor([[1.0, 2.0, 3.0, 4.0]])                                   # mean 2.5, var 1.25
    got = ref.layernorm(x, torch.tensor([1.0, 1.0, 2.0, 2.0]), torch.tensor([0.0, 1.0, 0.0, -1.0]), 0.0, 2.0)
    r = 1.0 / math.sqrt(1.25)
    assert torch.allclose(got, torch.tensor([[0.0, 2 * (1 - 0.5 * r), 2 * r, 2 * (3 * r - 1)]], dtype=F64), atol=1e-14)


def test_groupnorm_matches_torch_row_by_row_and_a_hand_row():
    for case in ref.GN_CASES + ref.GN_OFFSET_CASES:
        if case.t * case.c > 200000:
            continue                                                            # the same code on more data
        d = ref.gn_inputs(case)
        for use_mish, add in ref.GN_VARIANTS:
            got = ref.gn_expected(case, use_mish, add)
            for i, n in enumerate(case.lens):
                n = max(0, min(n, case.t))
                assert float(got[i, n:].abs().max()) == 0.0 if n < case.t else True
                if n == 0:
                    continue
                want = F.group_norm(d["x"][i:i + 1, :n].double().transpose(1, 2), case.groups, d["gamma"].double(), d["beta"].double(), 1e-5)
                want = want.transpose(1, 2)[0]
                if use_mish:
                    want = F.mish(want)
                if add:
                    want = want + d["add"][i].double()
                assert ref.rel_err(got[i, :n], want) < 1e-9, (case.name, i)
    # two frames, two groups of one channel each: group 0 sees (1, 3) -> -1, +1; group 1 sees (5, 7) -> -1, +1; the third frame is padding
    x = torch.tensor([[[1.0, 5.0], [3.0, 7.0], [9.0, 9.0]]])
    got = ref.groupnorm(x, torch.tensor([2.0, 1.0]), torch.tensor([0.5, -1.0]), 2, 0.0, lens=(2,), add_bc=torch.tensor([[10.0, 20.0]]))
    assert torch.allclose(got, torch.tensor([[[8.5, 18.0], [12.5, 20.0], [0.0, 0.0]]], dtype=F64), atol=1e-12)
    assert torch.allclose(ref.mish(torch.tensor([-2.0, 0.0, 25.0], dtype=F64)), F.mish(torch.tensor([-2.0, 0.0, 25.0], dtype=F64)), atol=1e-15)


def test_elementwise_definitions_match_torch():
    d = ref.el_inputs(ref.EL_CASES[1])
    x, xd = d["x"], d["x"].double()
    run = lambda op: ref.elementwise(op, x, **ref.el_args(op, d))
    s32 = lambda v: float(torch.tensor(v, dtype=F32))
    assert ref.rel_err(run(ref.EL_MISH), F.mish(xd)) < 1e-14
    assert ref.rel_err(run(ref.EL_SILU), F.silu(xd)) < 1e-14
    assert ref.rel_err(run(ref.EL_ELU), F.elu(xd)) < 1e-14
    assert ref.rel_err(run(ref.EL_LEAKY), F.leaky_relu(xd, s32(ref.LEAKY_S))) < 1e-14
    assert ref.rel_err(run(ref.EL_TANH), xd.tanh()) == 0.0
    assert torch.equal(run(ref.EL_CLAMP), xd.clamp(-s32(ref.CLAMP_S), s32(ref.CLAMP_S)))
    assert torch.equal(run(ref.EL_RELU_SCALE), s32(ref.RELU_S) * F.relu(xd)) and torch.equal(run(ref.EL_SCALE), s32(ref.SCALE_S) * xd)
    al = d["alpha"].double()
    assert ref.rel_err(run(ref.EL_SNAKE), xd + (1.0 / (al + 1e-9)) * torch.sin(xd * al) ** 2) < 1e-14
    assert float((al[None, None, :] * xd).abs().max()) < 12.0                                          # the stated Snake range
    assert torch.equal(run(ref.EL_ADD), xd + s32(ref.ADD_S) * d["z"][:2].double())
    assert torch.equal(run(ref.EL_ADD_BC)[1, 7], xd[1, 7] + d["bc"][1].double())
    masked = run(ref.EL_MUL_ROWMASK)
    assert torch.equal(masked[0, :20], xd[0, :20]) and float(masked[0, 20:].abs().max()) == 0.0 and torch.equal(masked[1], xd[1])
    dt, r = s32(ref.CFG_DT), s32(ref.CFG_R)
    assert torch.equal(run(ref.EL_CFG_EULER), xd + dt * ((1 + r) * d["z"][:2].double() - r * d["z"][2:].double()))
    # the edge values sit on both sides of every branch
    e = torch.tensor(ref.EDGE_VALUES, dtype=F32)
    s = torch.tensor(ref.CLAMP_S, dtype=F32)
    assert (e > 20).any() and (e < 20).any() and (e == 20).any() and (e == -90).any()
    assert (e == 0).sum() == 2 and ((e > 0) & (e < 1e-20)).any() and ((e < 0) & (e > -1e-20)).any()
    assert (e == s).any() and (e == -s).any() and ((e > s) & (e < 1)).any() and ((e < s) & (e > 0.98)).any() and ((e < -s) & (e > -1)).any()


def test_embedding_and_interpolation_match_torch_and_hand_rows():
    for rows in ref.EMB_ROWS:
        for c in ref.EMB_C:
            d = ref.emb_inputs(rows, c)
            ids = d["ids"].long().clamp(0, ref.EMB_VOCAB - 1)
            assert torch.equal(ref.embedding(d["table"], d["ids"]), F.embedding(ids, d["table"]).double())
    tab = torch.tensor([[1.0], [2.0], [3.0]])
    assert ref.embedding(tab, torch.tensor([-1, 0, 2, 3]), 2.0).flatten().tolist() == [2.0, 2.0, 6.0, 6.0]
    for case in ref.INTERP_CASES:
        x = ref.interp_inputs(case)
        if case.in_lens is None:
            want = F.interpolate(x.double().transpose(1, 2), size=case.t_out, mode="linear").transpose(1, 2)
            assert ref.rel_err(ref.interp_linear(x, case.t_out), want) < 1e-12, case.name
        else:
            got = ref.interp_linear(x, case.t_out, case.in_lens, case.out_lens)
            for i, (ti, to) in enumerate(zip(case.in_lens, case.out_lens)):
                assert float(got[i, to:].abs().max()) == 0.0 if to < case.t_out else True
                if to:
                    want = F.interpolate(x[i:i + 1, :ti].double().transpose(1, 2), size=to, mode="linear").transpose(1, 2)[0]
                    assert ref.rel_err(got[i, :to], want) < 1e-12, (case.name, i)
    got = ref.interp_linear(torch.tensor([[[0.0], [4.0]]]), 4)                 # 2 -> 4: x0, 3/4 x0 + 1/4 x1, 1/4 x0 + 3/4 x1, x1
    assert got.flatten().tolist() == [0.0, 1.0, 3.0, 4.0]


def _torch_stft(sig):
    spec = torch.stft(sig, 16, 4, 16, window=torch.hann_window(16, periodic=True, dtype=sig.dtype), return_complex=True)
    return torch.cat([spec.real, spec.imag], dim=1).transpose(1, 2)


def _torch_istft(y, dtype):
    y = y.to(dtype)
    mag, ph = torch.exp(y[..., :9]).clamp_max(ref.MAG_CLIP), torch.sin(y[..., 9:])
    spec = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)).transpose(1, 2)
    return torch.istft(spec, 16, 4, 16, window=torch.hann_window(16, periodic=True, dtype=dtype)).clamp(-ref.AUDIO_LIMIT, ref.AUDIO_LIMIT)


def test_stft_and_istft_match_torch_row_by_row():
    for case in ref.STFT_CASES[:-1]:
        x = ref.stft_inputs(case)
        got = ref.stft16(x, case.lens)
        for i in range(case.b):
            n = case.n if case.lens is None else case.lens[i]
            assert ref.rel_err(got[i, :n // 4 + 1], _torch_stft(x[i:i + 1, :n].double())[0]) < 1e-12, (case.name, i)
            assert float(got[i, n // 4 + 1:].abs().max()) == 0.0 if n < case.n else True
    got = ref.stft16(torch.ones(1, 32))                                        # a constant: the window's sum in the DC bin, -sum / 2 beside it
    assert torch.allclose(got[0, :, 0], torch.full((9,), 8.0, dtype=F64), atol=1e-12)
    assert torch.allclose(got[0, :, 1], torch.full((9,), -4.0, dtype=F64), atol=1e-12) and float(got[0, :, 2:].abs().max()) < 1e-12
    for case in ref.ISTFT_CASES[:-1]:
        y = ref.istft_inputs(case)
        got = ref.istft16(y, frame_lens=case.frame_lens)
        for i in range(case.b):
            nf = case.frames if case.frame_lens is None else case.frame_lens[i]
            n = 4 * (nf - 1)
            assert float(got[i, n:].abs().max()) == 0.0 if n < got.shape[1] else True
            if nf >= 2:
                assert ref.abs_err(got[i, :n], _torch_istft(y[i:i + 1, :nf], F64)[0]) < 1e-12, (case.name, i)


def test_nsf_source_matches_the_oracle_and_a_hand_prefix():
    from oracle import synth as osyn

    for case in ref.NSF_CASES:
        if case.b > 2:
            continue                                                            # the same code on more data
        d = ref.nsf_inputs(case)
        cfg = types.SimpleNamespace(upsample_total=case.up, nb_harmonics=ref.NSF_NH - 1, sample_rate=ref.NSF_SR, nsf_alpha=ref.NSF_AMP,
                                    nsf_voiced_threshold=ref.NSF_THR, nsf_sigma=ref.NSF_SIGMA)
        sd = {"m_source.l_linear.weight": d["lin_w"][None, :], "m_source.l_linear.bias": d["lin_b"]}
        want = osyn.hift_source(sd, cfg, d["f0"], d["phase0"], d["noise"])
        got = ref.nsf_source(d["f0"], d["phase0"], d["noise"], d["lin_w"], d["lin_b"], case.up)
        assert got.shape == want.shape and ref.abs_err(got, want) < 2e-6, case.name      # the oracle takes sin and tanh in float32
    # one harmonic, sr 4, f0 = (1, 2), two samples per frame: cumulative phase 1/4, 2/4, 4/4, 6/4 cycles -> sin = 1, 0, 0, 0
    got = ref.nsf_source(torch.tensor([[1.0, 2.0]]), torch.zeros(1, 1), torch.zeros(1, 4, 1), torch.ones(1), torch.zeros(1), 2, sr=4.0,
                         amp=1.0, sigma=0.0, thr=0.5)
    assert torch.allclose(got, torch.tanh(torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=F64)), atol=1e-12)


# ---------------------------------------------------------------- the case lists
def test_case_lists_cover_the_path_chunk_and_stride_edges():
    assert (ref.BLOCK, ref.ELEM_GRID_CAP, ref.AUDIO_GRID_CAP) == (256, 2048, 4096)
    assert (ref.LN_MAX_VEC_C, ref.LN_ROUND, ref.GN_ROWS, ref.GNF_NT, ref.GN_FUSED_TILE_BYTES, ref.GN_FUSED_Z2_BLOCKS, ref.F0_SCAN) == (
        2048, 256, 64, 512, 150 * 1024, 256, 256)
    # LayerNorm: scalar path by c % 4 and by c > LN_MAX_VEC_C, a partial last round on both sides of LN_ROUND, rows around the block
    cs, rows = {c.c for c in ref.LN_CASES}, {c.rows for c in ref.LN_CASES}
    assert cs >= {1, 4, 63, 80, ref.LN_ROUND - 4, ref.LN_ROUND, ref.LN_ROUND + 4, 513, 1024, ref.LN_MAX_VEC_C, ref.LN_MAX_VEC_C + 4}
    assert rows >= {1, ref.LN_ROWS_PER_BLOCK, ref.LN_ROWS_PER_BLOCK + 1, 37} and len(ref.LN_CASES) == len(cs) * len(rows)
    raw = {c.name: c for c in ref.LN_RAW_CASES}
    vec = lambda c: ref.ln_takes_vector_path(c.c, c.c + c.dx, c.c + c.dy, c.off != "x", c.off != "y", c.off != "gamma", c.off != "beta")
    assert vec(raw["ln-raw-ld-vec"]) and (raw["ln-raw-ld-vec"].dx, raw["ln-raw-ld-vec"].dy) == (4, 8)
    assert not any(vec(c) for c in ref.LN_RAW_CASES if c.dx == 1 or c.off) and {c.off for c in ref.LN_RAW_CASES} >= {"x", "y", "gamma", "beta"}
    # GroupNorm: every path of the launcher and of the fused kernel's write loop
    by_path = {}
    for c in ref.GN_CASES:
        assert ref.gn_path(len(c.lens), c.t, c.c, c.groups) == c.path, c.name
        by_path.setdefault(c.path, []).append(c)
    assert set(by_path) == {"fused-fixed-z2", "fused-fixed-z1", "fused-walk-z2", "fused-walk-z1", "two-vec", "two-scalar"}
    assert {c.c // c.groups for c in by_path["fused-fixed-z2"]} >= {4, 32, 64}
    assert {(c.c, c.groups) for c in by_path["fused-walk-z2"]} >= {(80, 1), (24, 2)}
    z2 = by_path["fused-fixed-z2"] + by_path["fused-walk-z2"]
    assert any(c.t == 1 for c in z2) and any(c.t % 2 == 1 and c.t > 1 for c in z2)
    assert any(len(c.lens) == 17 and c.groups == 8 for c in by_path["fused-fixed-z1"])
    shape = lambda c: (c.t, c.c, c.groups)
    assert {shape(c) for c in by_path["two-vec"]} >= {(481, 80, 1), (1201, 256, 8), (151, 2048, 8)} and (480, 80, 1) in map(shape, z2)
    assert 480 * 80 * 4 == ref.GN_FUSED_TILE_BYTES == 1200 * 32 * 4 and (1200, 256, 8) in map(shape, z2)   # the last fused t beside the first two-launch t
    assert {(c.c, c.groups) for c in by_path["two-scalar"]} >= {(12, 2), (6, 2)}
    assert 2048 // 4 == 2 * ref.GN_APPLY_NT and 2048 == 8 * 256                 # (151, 2048, 8): two trips of the column loop, eight of the stats loop
    assert ref.gn_path(len(ref.GN_MISALIGNED.lens), 131, 256, 8, aligned=False) == "two-scalar"
    for c in ref.GN_CASES + ref.GN_OFFSET_CASES + ref.GN_REPORTED_CASES:
        want = {c.t, c.t - 1, 1, 0, c.t + 5} | {n for n in (37, ref.GN_ROWS, 2 * ref.GN_ROWS) if n < c.t}
        assert set(c.lens) == want and c.lens[-1] == c.t, c.name
    assert {(shape(c), c.offset) for c in ref.GN_OFFSET_CASES} == {(s[:3], o) for o in ((30.0, 0.3), (8.0, 0.5))
                                                                   for s in ref.GN_TWO_LAUNCH_SHAPES + ref.GN_PAIR[:1]}
    assert ref.GN_VARIANTS == ((False, False), (True, True))
    # element-wise, interpolation, signal operators: every grid-stride loop takes a second trip
    big = ref.EL_CASES[-1]
    assert {c.c for c in ref.EL_CASES} >= {1, 80, 128} and (big.b, big.t, big.c) == (2, 1030, 256) and big.b * big.t * big.c > ref.ELEM_STRIDE
    it = ref.INTERP_CASES
    assert {(c.t_in, c.t_out) for c in it} >= {(1, 1), (1, 5), (2, 1), (2, 2), (2, 7), (150, 75), (150, 150), (150, 430)}
    assert any(c.out_lens and 0 in c.out_lens and 1 in c.in_lens for c in it) and any(c.b * c.t_out * c.c == 528000 > ref.ELEM_STRIDE for c in it)
    assert {c.n for c in ref.STFT_CASES} >= {16, 20, 2560} and any(c.b * (c.n // 4 + 1) > ref.AUDIO_STRIDE for c in ref.STFT_CASES)
    assert any(c.lens and min(c.lens) == 16 and max(c.lens) == c.n and all(n % 4 == 0 for n in c.lens) for c in ref.STFT_CASES)
    assert {c.frames for c in ref.ISTFT_CASES} >= {2, 3, 641} and any(c.b * 4 * (c.frames - 1) > ref.AUDIO_STRIDE for c in ref.ISTFT_CASES)
    assert any(c.frame_lens and {1, 2} <= set(c.frame_lens) for c in ref.ISTFT_CASES)
    y = ref.istft_inputs(ref.ISTFT_CASES[2])
    assert float((y[..., :9] > math.log(ref.MAG_CLIP)).float().mean()) > 0.03
    wav = ref.istft16(y)
    clamped = float((wav.abs() == ref.AUDIO_LIMIT).float().mean())
    assert 0.05 < clamped < 0.95, clamped                                       # outputs reach the clamp, and many stay inside it
    nsf = ref.NSF_CASES
    assert {c.tm for c in nsf} >= {1, ref.F0_SCAN - 1, ref.F0_SCAN, ref.F0_SCAN + 1, 2 * ref.F0_SCAN + 1} and {c.up for c in nsf} == {256, 480}
    assert any(c.b == 8 and c.tm == 513 and c.b * c.tm * c.up == 1050624 > ref.AUDIO_STRIDE for c in nsf)
    f0 = ref.nsf_inputs(next(c for c in nsf if c.b == 8))["f0"]
    assert bool((f0 == ref.NSF_THR).any())
    for edge in (ref.F0_SCAN, 2 * ref.F0_SCAN):
        assert bool((f0[1, edge - 3:edge + 3] == 0).all()) and bool((f0[0, edge - 3:edge + 3] > ref.NSF_THR).all())   # unvoiced / voiced across the edge
    assert set(ref.EMB_EDGE_IDS) == {-1, 0, ref.EMB_VOCAB - 1, ref.EMB_VOCAB}
    for rows in ref.EMB_ROWS:
        seen = {int(i) for c in ref.EMB_C for i in ref.emb_inputs(rows, c)["ids"]}
        assert seen >= ({-1, ref.EMB_VOCAB} if rows == 1 else set(ref.EMB_EDGE_IDS)), rows


# ---------------------------------------------------------------- sensitivity
def _moved(want, wrong):
    return ref.rel_err(wrong, want)


def test_groupnorm_cases_tell_the_wrong_variants_apart():
    least = {}
    for case in ref.GN_CASES:
        d = ref.gn_inputs(case)
        for use_mish, add in ref.GN_VARIANTS:
            want = ref.gn_expected(case, use_mish, add)
            for m in ref.GN_MUTATIONS:
                if not ref.gn_bears(case, m, use_mish, add):
                    continue
                wrong = ref.groupnorm(d["x"], d["gamma"], d["beta"], case.groups, 1e-5, d["lens"], use_mish, d["add"] if add else None, mutate=m)
                dist = _moved(want, wrong)
                least[m] = min(least.get(m, 1e9), dist)
                assert dist >= ref.MUTATION_FACTOR * ref.GN_TOL, (case.name, use_mish, add, m, dist)
    print("[sensitivity] GroupNorm, least distance per variant:", {m: f"{v:.1e}" for m, v in least.items()})
    assert set(least) == set(ref.GN_MUTATIONS)


def test_offset_inputs_are_what_the_issue_measured():
    """A statement of the defect: E[x^2] - mean^2 from float32 sums of the offset inputs is off by far more than the bar, the two-pass
    form in float32 is not (so the bar is within float32's reach at mean 30, std 0.3)."""
    case = next(c for c in ref.GN_OFFSET_CASES if (c.t, c.c, c.offset) == (481, 80, (30.0, 0.3)))
    x = ref.gn_inputs(case)["x"][0]
    want = ref.groupnorm(x[None], torch.ones(80), torch.zeros(80), 1)[0]
    s1, s2 = x.sum(0).sum().double(), (x * x).sum(0).sum().double()              # float32 per-channel sums, as the kernel took them
    mean = s1 / x.numel()
    one_pass = (x.double() - mean) / torch.sqrt(s2 / x.numel() - mean * mean + 1e-5)
    two_pass = F.group_norm(x.t()[None], 1, eps=1e-5)[0].t()
    assert ref.rel_err(one_pass, want) > ref.GN_TOL and ref.rel_err(two_pass, want) < ref.GN_TOL / 10


def test_other_cases_tell_their_wrong_variants_apart():
    case = ref.EL_CASES[-1]
    d = ref.el_inputs(case)
    kw = ref.el_args(ref.EL_CFG_EULER, d)
    want = ref.elementwise(ref.EL_CFG_EULER, d["x"], **kw)
    assert _moved(want, ref.elementwise(ref.EL_CFG_EULER, d["x"], mutate="cfg_sign", **kw)) >= ref.MUTATION_FACTOR * ref.EL_TOL[ref.EL_CFG_EULER]
    for case in ref.INTERP_CASES:
        x = ref.interp_inputs(case)
        want = ref.interp_linear(x, case.t_out, case.in_lens, case.out_lens)
        variants = (["align_corners"] if case.t_in != case.t_out and case.t_in > 1 else []) + (["from_t_max"] if case.in_lens else [])
        for m in variants:
            dist = _moved(want, ref.interp_linear(x, case.t_out, case.in_lens, case.out_lens, mutate=m))
            assert dist >= ref.MUTATION_FACTOR * ref.INTERP_TOL, (case.name, m, dist)
    for case in ref.STFT_CASES:
        if case.lens:
            x = ref.stft_inputs(case)
            dist = _moved(ref.stft16(x, case.lens), ref.stft16(x, case.lens, mutate="reflect_padded"))
            assert dist >= ref.MUTATION_FACTOR * ref.STFT_TOL, (case.name, dist)
    for case in ref.ISTFT_CASES[:-1]:
        y = ref.istft_inputs(case)
        want = ref.istft16(y, frame_lens=case.frame_lens)
        for m in ("unclipped",) + (("ola_sees_padding",) if case.frame_lens else ()):
            dist = ref.abs_err(ref.istft16(y, frame_lens=case.frame_lens, mutate=m), want)
            assert dist >= ref.MUTATION_FACTOR * ref.ISTFT_ATOL, (case.name, m, dist)
    for case in ref.NSF_CASES:
        if case.b > 2:
            continue
        d = ref.nsf_inputs(case)
        want = ref.nsf_source(up=case.up, **d)
        for m in ref.NSF_MUTATIONS:
            if (m == "prefix_restart" and case.tm <= ref.F0_SCAN) or (m == "voiced_ge" and case.tm <= ref.NSF_THR_FRAME):
                continue
            dist = ref.abs_err(ref.nsf_source(up=case.up, mutate=m, **d), want)
            assert dist >= ref.MUTATION_FACTOR * ref.NSF_ATOL, (case.name, m, dist)


# ---------------------------------------------------------------- the bounds that have no earlier bar
def test_bounds_follow_the_measured_floors():
    """float32 torch against the float64 definition on the cases' own inputs; each constant sits at most 10 % above what is measured."""
    ln = 0.0
    for case in ref.LN_CASES:
        d = ref.ln_inputs(case)
        ln = max(ln, ref.rel_err(F.layer_norm(d["x"], (case.c,), d["gamma"], d["beta"], 1e-5), ref.layernorm(d["x"], d["gamma"], d["beta"])))
    gn = 0.0
    for case in ref.GN_CASES:
        d = ref.gn_inputs(case)
        for use_mish, add in ref.GN_VARIANTS:
            want = ref.gn_expected(case, use_mish, add)
            got = torch.zeros(want.shape, dtype=F32)
            for i, n in enumerate(case.lens):
                n = max(0, min(n, case.t))
                if n:
                    y = F.group_norm(d["x"][i:i + 1, :n].transpose(1, 2), case.groups, d["gamma"], d["beta"], 1e-5).transpose(1, 2)[0]
                    y = F.mish(y) if use_mish else y
                    got[i, :n] = y + d["add"][i] if add else y
            gn = max(gn, ref.rel_err(got, want))
    silu = tanh = 0.0
    for case in ref.EL_CASES + (ref.EL_EDGE_CASE,):
        x = ref.el_inputs(case)["x"]
        silu = max(silu, ref.rel_err(F.silu(x), ref.elementwise(ref.EL_SILU, x)))
        tanh = max(tanh, ref.rel_err(torch.tanh(x), ref.elementwise(ref.EL_TANH, x)))
    print(f"[floor] float32 torch vs float64: LayerNorm {ln:.3e}, GroupNorm {gn:.3e}, SiLU {silu:.3e}, tanh {tanh:.3e}")
    for measured, const in ((ln, ref.LN_F32_FLOOR), (gn, ref.GN_F32_FLOOR), (silu, ref.SILU_FLOOR), (tanh, ref.TANH_FLOOR)):
        assert measured <= const <= 1.1 * measured, (measured, const)
    assert ref.LN_F16_TOL == 4 * (ref.LN_F32_FLOOR + 2.0 ** -11) and ref.GN_F16_TOL == 4 * (ref.GN_F32_FLOOR + 2.0 ** -11)
    assert ref.SILU_TOL == 4 * ref.SILU_FLOOR and ref.TANH_TOL == 4 * ref.TANH_FLOOR
