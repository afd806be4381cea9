"""What a joined pass of a flow session shares among its batches (include/session/astts_flow_share.h): ONE tfm_ffn_fused launch over
a segment table, and ONE astts_op_gemm launch per group of batches whose plans for their own row counts are equal.  Every row must
carry the bits of its batch's own launch (torch.equal), at the operators and through the engine, with ``ASTTS_FLOW_SHARE`` unset and
``=0``; and the launch counts must show that sharing happens.  CosyVoice widths throughout (C = 256, hidden 1024, 8 heads): the tiny
widths take the unfused path."""
import dataclasses

import pytest
import torch

import gemm_plan_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, HIDDEN = 256, 1024


# ---------------------------------------------------------------------------------------------------------------- feed-forward operator

@pytest.fixture(scope="module")
def ffn_weights():
    from astts import ops
    from astts.synth.model import fold_layernorm

    g = torch.Generator().manual_seed(7)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w1, b1 = torch.randn(HIDDEN, C, generator=g) / 16, 0.1 * torch.randn(HIDDEN, generator=g)
    w2, b2 = torch.randn(C, HIDDEN, generator=g) / 32, 0.1 * torch.randn(C, generator=g)
    w1f, b1f = fold_layernorm(w1, b1, gamma, beta)
    p1, p2 = ops.PackedWeight(w1f, b1f), ops.PackedWeight(w2, b2)
    wo = {}
    for k0 in (256, 512):
        po = ops.PackedWeight(torch.randn(C, k0, generator=g) / 24, 0.1 * torch.randn(C, generator=g))
        wo[k0] = (po, ops.tfm_pack_frag(po))
    return p1, ops.tfm_pack_frag(p1), p2, ops.tfm_pack_frag(p2), wo


def _segments(rows, gap=0):
    out, r = [], 0
    for n in rows:
        out.append((r, n))
        r += n + gap
    return out, r


# tile counts 9, 33 and 1 (no multiple of 8; the chunk rotations 0..3 all occur and wrap: 33 tiles reach seed 4 = rotation 0 again),
# partial last tiles, segments that start at rows 283 and 1332 (not divisible by 32); two whole-tile segments; one segment
SEGMENTS = [(283, 1049, 1), (512, 640), (970,)]


@pytest.mark.parametrize("k0", [0, 256, 512])
@pytest.mark.parametrize("rows", SEGMENTS)
def test_segmented_ffn_launch_equals_one_launch_per_segment(ffn_weights, rows, k0):
    from astts import ops

    p1, f1, p2, f2, wo = ffn_weights
    segs, m = _segments(rows)
    g = torch.Generator().manual_seed(sum(rows) + k0)
    x = (torch.randn(m, C, generator=g) * 2 + 0.3).to(DEV)
    kw = {}
    attn = None
    if k0:
        attn = torch.randn(m, k0, generator=g).to(DEV, torch.float16)
        kw = dict(wo=wo[k0][0], wo_frag=wo[k0][1])
    ref = torch.cat([ops.tfm_ffn_fused(x[r0:r0 + n], p1, f1, p2, f2, attn=None if attn is None else attn[r0:r0 + n], **kw) for r0, n in segs])
    out = ops.tfm_ffn_fused(x, p1, f1, p2, f2, attn=attn, segments=segs, **kw)
    assert torch.equal(out, ref)
    if len(segs) == 1:       # one segment: astts_op_tfm_ffn_fused itself
        assert torch.equal(out, ops.tfm_ffn_fused(x, p1, f1, p2, f2, attn=attn, **kw))
    inplace = x.clone()
    assert ops.tfm_ffn_fused(inplace, p1, f1, p2, f2, attn=attn, segments=segs, out=inplace, **kw) is inplace
    assert torch.equal(inplace, ref)
    assert bool(torch.isfinite(out).all())


def test_segmented_ffn_launch_leaves_rows_between_segments_alone(ffn_weights):
    from astts import ops

    p1, f1, p2, f2, wo = ffn_weights
    segs, m = _segments((283, 1049, 1), gap=5)
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(m, C, generator=g) * 2 + 0.3).to(DEV)
    attn = torch.randn(m, 512, generator=g).to(DEV, torch.float16)
    out = torch.full_like(x, -7.0)
    ops.tfm_ffn_fused(x, p1, f1, p2, f2, attn=attn, wo=wo[512][0], wo_frag=wo[512][1], segments=segs, out=out)
    keep = torch.ones(m, dtype=torch.bool, device=DEV)
    for r0, n in segs:
        keep[r0:r0 + n] = False
        assert torch.equal(out[r0:r0 + n], ops.tfm_ffn_fused(x[r0:r0 + n], p1, f1, p2, f2, attn=attn[r0:r0 + n], wo=wo[512][0], wo_frag=wo[512][1]))
    assert bool((out[keep] == -7.0).all())


def test_segmented_ffn_launch_refuses_bad_tables(ffn_weights):
    from astts import _lib, ops

    p1, f1, p2, f2, _ = ffn_weights
    x = torch.zeros(128, C, device=DEV)
    for segs in ([(0, 64), (32, 64)], [(64, 32), (0, 32)], [(0, 0)], [(0, 16)] * 5, []):
        with pytest.raises(_lib.AsttsError) as e:
            ops.tfm_ffn_fused(x, p1, f1, p2, f2, segments=segs)
        assert e.value.code == _lib.ERR_INVALID


# ------------------------------------------------------------------------------------------------------------------------ GEMM operator

def _conv_case(name):
    """(x [seqs, t_in, cin], weight, conv arguments, t_out, sequences per segment, segments)"""
    from astts import ops

    g = torch.Generator().manual_seed(len(name))
    if name == "fp32 k=3":            # the ResNet / resampling convolution: n = 256, K = 3 x 256
        t_in = t_out = 384
        w = ops.PackedWeight(torch.randn(256, 3, 256, generator=g) / 28, 0.1 * torch.randn(256, generator=g))
        kw = dict(stride=1, pad=1)
    elif name == "fp32 k=3 stride 2":   # the down block's resampling convolution
        t_in, t_out = 767, 384
        w = ops.PackedWeight(torch.randn(256, 3, 256, generator=g) / 28, 0.1 * torch.randn(256, generator=g))
        kw = dict(stride=2, pad=1)
    else:                             # "fp32 transposed": the up block's phase-decomposed ConvTranspose1d, [b, tt, C] -> [b, tt + 1, 2 C]
        t_in, t_out = 383, 384
        w = ops.PackedWeight(torch.randn(512, 2, 256, generator=g) / 23, 0.1 * torch.randn(512, generator=g))
        kw = dict(stride=1, pad=1)
    return g, w, kw, t_in, t_out


# seqs per segment x 384 output rows: 16 -> 6 144 rows, 32 -> 12 288 rows
GEMM_CASES = [
    ("fp32 k=3", 16, 2, "T64k128", "T128x64"),
    ("fp32 k=3", 16, 3, "T64k128", "T128x64"),
    ("fp32 k=3", 32, 2, "T128x64", "T128"),
    ("fp32 k=3 stride 2", 16, 2, "T64k128", "T128x64"),
    ("fp32 transposed", 16, 2, "T128x64", "T128"),
]


@pytest.mark.parametrize("name,seqs,n_seg,alone,together", GEMM_CASES)
def test_planned_gemm_over_several_batches_equals_per_batch_gemm(name, seqs, n_seg, alone, together):
    from astts import ops

    g, w, kw, t_in, t_out = _conv_case(name)
    m1 = seqs * t_out
    # the case is one only while the batch's own row count and the total lie on opposite sides of a rule of gemm_plan.h
    assert ops.gemm_kernel_kind(m1, w.n, w.cin, taps=w.taps, plain=False) == alone
    assert ops.gemm_kernel_kind(n_seg * m1, w.n, w.cin, taps=w.taps, plain=False) == together
    x = torch.randn(n_seg * seqs, t_in, w.cin, generator=g).to(DEV)
    res = torch.randn(n_seg * m1, w.n, generator=g).to(DEV)
    ref = torch.cat([ops.gemm(x[i * seqs:(i + 1) * seqs], w, t_in=t_in, t_out=t_out, residual=res[i * m1:(i + 1) * m1], **kw) for i in range(n_seg)])
    out = ops.gemm(x, w, t_in=t_in, t_out=t_out, residual=res, plan_m=m1, **kw)
    assert torch.equal(out, ref)
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("n_seg", [2, 3])
def test_planned_ring_gemm_over_several_batches_equals_per_batch_gemm(n_seg):
    """fp16 rows, n = 512, K = 256 (the q|k|v projection's family): 1 280 rows alone run the 64 x 64 ring (10 x 8 = 80 tiles of
    128 x 64 < 160), 2 560 and 3 840 rows together the 128 x 64 ring (ring_tile_by_rule in gemm_plan.h; the recorded plan of 2 560)."""
    from astts import ops

    m1, n, k = 1280, 512, 256
    assert gemm_plan_golden.ring_tile(2 * m1, n, k) == "128x64"
    assert ops.gemm_kernel_kind(m1, n, k, x_f16=True) == "ring"
    g = torch.Generator().manual_seed(n_seg)
    w = ops.PackedWeight(torch.randn(n, k, generator=g) / 16, 0.1 * torch.randn(n, generator=g))
    x = torch.randn(n_seg * m1, k, generator=g).to(DEV, torch.float16)
    for dt in (torch.float16, torch.float32):
        ref = torch.cat([ops.gemm(x[i * m1:(i + 1) * m1], w, out_dtype=dt) for i in range(n_seg)])
        out = ops.gemm(x, w, out_dtype=dt, plan_m=m1)
        assert torch.equal(out, ref)
    ops.set_gemm_ring_mode(3)          # the 64 x 64 tile forced over all rows: what plan_m = 1 280 must have launched
    try:
        forced = ops.gemm(x, w, out_dtype=torch.float32)
    finally:
        ops.set_gemm_ring_mode(-1)
    assert torch.equal(out, forced)


def test_planned_gemm_refuses_the_skinny_family_for_more_rows():
    from astts import _lib, ops

    g = torch.Generator().manual_seed(3)
    w = ops.PackedWeight(torch.randn(256, 256, generator=g) / 16)
    x = torch.randn(64, 256, generator=g).to(DEV)
    assert ops.gemm_kernel_kind(32, 256, 256) == "skinny"
    with pytest.raises(_lib.AsttsError) as e:
        ops.gemm(x, w, plan_m=32)                     # the m <= 32 family keeps its rows in LDS: it does not serve 64
    assert e.value.code == _lib.ERR_UNSUPPORTED
    assert torch.equal(ops.gemm(x[:32], w, plan_m=32), ops.gemm(x[:32], w))     # the same rows: the ordinary call
    for bad in (0, 65):
        with pytest.raises(_lib.AsttsError) as e:
            ops.gemm(x, w, plan_m=bad)
        assert e.value.code == _lib.ERR_INVALID


# ------------------------------------------------------------------------------------------------------------------------------ engine

def _batch(cfg, b, t, seed):
    g = torch.Generator().manual_seed(seed)
    z, mu, cond = (torch.randn(b, t, cfg.mel, generator=g).to(DEV) for _ in range(3))
    return z, mu, torch.randn(b, cfg.mel, generator=g).to(DEV), cond, None


def _joined(fd, t, batches, joins, slots=4, rows_max=32):
    """Batch i is admitted when ``joins[i]`` passes have been enqueued -> every batch's mel."""
    sess = fd.session(t, slots, rows_max)
    jobs = [None] * len(batches)
    passes = 0
    while any(j is None for j in jobs) or sess.active():
        for i, (z, mu, spk, cond, lens) in enumerate(batches):
            if jobs[i] is None and joins[i] <= passes:
                assert sess.can_admit(z.shape[0], t), (i, passes, sess.state())
                jobs[i] = sess.admit(z.clone(), mu, spk, cond, lens)
        assert sess.active(), "a batch is waiting for a pass nobody runs"
        sess.step(1)
        passes += 1
    sess.close()
    torch.cuda.synchronize()
    return [j.x for j in jobs]


@pytest.fixture(scope="module")
def full_flow():
    from astts.synth.config import SynthConfig
    from astts.synth.model import FlowDecoder
    from astts.synth.weights import make_flow_weights

    cfg = dataclasses.replace(SynthConfig(), cfm_steps=3)      # CosyVoice-300M estimator widths: C = 256, 8 heads
    return cfg, FlowDecoder(make_flow_weights(cfg, 3), cfg, torch.device(DEV))


ENGINE_CASES = [
    (64, (5, 4), (0, 1)),                   # 20 and 16 feed-forward tiles
    (97, (5, 3, 8), (0, 1, 1)),             # odd length, partial tiles, unequal batches whose GEMM plans may differ
    (96, (8, 8, 8, 8), (0, 0, 1, 2)),
    (385, (2, 1), (0, 1)),                  # past the fused attention's 384 frames: the q|k|v GEMM of the unfused branch is grouped by plan
]


@pytest.fixture(scope="module")
def lone_solves(full_flow):
    """every case's batches and their lone solves, computed once and shared by both settings of the switch"""
    cfg, fd = full_flow
    out = {}
    for t, rows, _ in ENGINE_CASES:
        batches = [_batch(cfg, b, t, 1000 * i + t) for i, b in enumerate(rows)]
        out[t] = (batches, [fd.solve(z.clone(), mu, spk, cond, lens) for z, mu, spk, cond, lens in batches])
    return out


@pytest.mark.parametrize("share", [None, "0"])
@pytest.mark.parametrize("t,rows,joins", ENGINE_CASES)
def test_batches_sharing_feed_forward_and_gemm_launches_equal_their_lone_solves(full_flow, lone_solves, monkeypatch, t, rows, joins, share):
    cfg, fd = full_flow
    if share is None:
        monkeypatch.delenv("ASTTS_FLOW_SHARE", raising=False)
    else:
        monkeypatch.setenv("ASTTS_FLOW_SHARE", share)
    batches, ref = lone_solves[t]
    got = _joined(fd, t, batches, joins)
    for i, (r, o) in enumerate(zip(ref, got)):
        assert torch.isfinite(o).all()
        assert torch.equal(o, r), (i, joins, float((o - r).abs().max()))


def test_a_joined_pass_of_equal_batches_records_the_launches_of_one_lone_pass(full_flow, monkeypatch):
    """Sharing happens, rather than a silent fall-back to per-batch launches: the launch profiler (PROF_GEMM_TILE brackets every
    astts_op_gemm tile / ring launch and every tfm_ffn_fused launch) counts, for the passes of n equal batches joined from step 0, the
    launches of ONE lone batch's passes -- and, with ASTTS_FLOW_SHARE=0, every batch's own feed-forward and GEMM launches on top."""
    from astts import ops

    cfg, fd = full_flow
    t, b, n = 64, 4, 3

    def launches(n_batches):
        sess = fd.session(t, 4, 32)
        for i in range(n_batches):
            sess.admit(*_batch(cfg, b, t, 50 + i)[:4])
        torch.cuda.synchronize()
        ops.prof_enable(ops.PROF_GEMM_TILE, True)         # after the admissions: their time paths are per batch by nature
        try:
            sess.run()
            _, count, _, dropped = ops.prof_read(ops.PROF_GEMM_TILE)
        finally:
            ops.prof_enable(ops.PROF_GEMM_TILE, False)
        sess.close()
        assert dropped == 0
        return count

    monkeypatch.delenv("ASTTS_FLOW_SHARE", raising=False)
    lone = launches(1)
    assert lone >= cfg.cfm_steps * 8          # every transformer block of every pass has one feed-forward launch
    assert launches(n) == lone
    monkeypatch.setenv("ASTTS_FLOW_SHARE", "0")
    apart = launches(n)        # the feed-forward and GEMM launches once per batch again (the ResNet convolutions, bracketed too, stay shared)
    assert apart > lone and (apart - lone) % (n - 1) == 0
    assert cfg.cfm_steps * 8 <= (apart - lone) // (n - 1) <= lone
