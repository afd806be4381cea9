"""Flow sessions on the GPU (include/session/astts_flow_session.h, FlowSession, PipelinedSynth(render_join=True)): a batch that joins a
running Euler solve shares every launch of an estimator pass with the batches already there, each at its own step, and its mel must
equal ``FlowDecoder.solve`` (astts_flow_solve) of that batch ALONE bit for bit (torch.equal) -- whatever it shared its launches
with."""
import dataclasses
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _batch(cfg, b, t, seed, short=False):
    """(z, mu, spk, cond, lens) of one batch; ``short``: rows shorter than t (lens), zero beyond their length."""
    g = torch.Generator().manual_seed(seed)
    z, mu, cond = (torch.randn(b, t, cfg.mel, generator=g).to(DEV) for _ in range(3))
    spk = torch.randn(b, cfg.mel, generator=g).to(DEV)
    lens = None
    if short:
        lens = torch.tensor([max(t // 2 - 1, 2), t - 3, t, 5][:b], dtype=torch.int32, device=DEV)
        keep = (torch.arange(t, device=DEV)[None, :] < lens[:, None])[..., None]
        z, mu, cond = z * keep, mu * keep, cond * keep
    return z, mu, spk, cond, lens


def _alone(fd, batches):
    return [fd.solve(z.clone(), mu, spk, cond, lens) for z, mu, spk, cond, lens in batches]


def _joined(fd, t, batches, joins, slots=4, rows_max=32):
    """Batch i is admitted when ``joins[i]`` passes have been enqueued -> (every batch's mel, the session's final state)."""
    sess = fd.session(t, slots, rows_max)
    jobs = [None] * len(batches)
    done = []
    passes = 0
    while any(j is None for j in jobs) or sess.active():
        for i, (z, mu, spk, cond, lens) in enumerate(batches):
            if jobs[i] is None and joins[i] <= passes:
                assert sess.can_admit(z.shape[0], t), (i, passes, sess.state())
                jobs[i] = sess.admit(z.clone(), mu, spk, cond, lens)
        assert sess.active(), "a batch is waiting for a pass nobody runs"
        done += sess.step(1)
        passes += 1
    state = sess.state()
    sess.close()
    torch.cuda.synchronize()
    assert sorted(id(j) for j in done) == sorted(id(j) for j in jobs)       # every batch handed over exactly once
    assert state[0] == 0 and state[1] == 0 and state[2] == passes
    return [j.x for j in jobs], state


def _check(fd, t, batches, joins, **kw):
    ref = _alone(fd, batches)
    got, state = _joined(fd, t, batches, joins, **kw)
    for i, (r, o) in enumerate(zip(ref, got)):
        assert torch.isfinite(o).all()
        assert torch.equal(o, r), (i, joins, float((o - r).abs().max()))
    return state


@pytest.fixture(scope="module")
def tiny_flow():
    from astts.synth.config import SynthConfig
    from astts.synth.model import FlowDecoder
    from astts.synth.weights import make_flow_weights

    cfg = dataclasses.replace(SynthConfig.tiny(), cfm_steps=4)
    return cfg, FlowDecoder(make_flow_weights(cfg, 0), cfg, torch.device(DEV))


# (rows of every batch, the pass count at which it is admitted, which batches have rows shorter than t, slots)
TINY_CASES = {
    "second batch at step 0": ((2, 2), (0, 0), (), 4),
    "second batch after step 2": ((2, 2), (0, 2), (), 4),
    "second batch at the first one's last step": ((2, 2), (0, 3), (), 4),
    "third batch in the slot a finished one freed": ((2, 3, 2), (0, 1, 4), (), 2),
    "batches of 1 and 3 rows": ((1, 3), (0, 1), (), 4),
    "short rows beside a full batch": ((3, 2), (0, 1), (0,), 4),
    "full batch joined by short rows": ((2, 4), (0, 2), (1,), 4),
    "lone batch": ((3,), (0,), (), 4),
}


@pytest.mark.parametrize("t", [33, 40])         # odd and even: the half resolution rounds
@pytest.mark.parametrize("case", list(TINY_CASES))
def test_tiny_batches_join_a_running_solve_bit_identical(tiny_flow, case, t):
    cfg, fd = tiny_flow
    rows, joins, short, slots = TINY_CASES[case]
    batches = [_batch(cfg, b, t, 100 * i + b + t, short=i in short) for i, b in enumerate(rows)]
    state = _check(fd, t, batches, joins, slots=slots)
    alone_passes = cfg.cfm_steps * len(rows)
    assert state[3] == alone_passes                      # every batch was carried through all its steps ...
    if len(rows) > 1:
        assert state[2] < alone_passes                   # ... in fewer passes than one solve each


def test_tiny_session_refuses_what_it_cannot_hold(tiny_flow):
    cfg, fd = tiny_flow
    sess = fd.session(40, 2, 6)
    assert not sess.can_admit(2, 33)                     # another frame count
    assert not sess.can_admit(7, 40)                     # more rows than the session has
    sess.admit(*_batch(cfg, 4, 40, 1)[:4])
    assert not sess.can_admit(3, 40) and sess.can_admit(2, 40)
    sess.admit(*_batch(cfg, 1, 40, 2)[:4])
    assert not sess.can_admit(1, 40)                     # both slots taken
    sess.run()
    assert sess.active() == 0 and sess.can_admit(6, 40)
    sess.close()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def full_flow():
    from astts.synth.config import SynthConfig
    from astts.synth.model import FlowDecoder
    from astts.synth.weights import make_flow_weights

    cfg = dataclasses.replace(SynthConfig(), cfm_steps=3)      # CosyVoice-300M estimator widths: C = 256, 8 heads
    return cfg, FlowDecoder(make_flow_weights(cfg, 3), cfg, torch.device(DEV))


@pytest.mark.parametrize("t,rows,joins", [
    (64, (5, 4), (0, 1)),                   # 18 sequences against 10 and 8 alone: crosses tfm_attn_fused's switch at 2 * heads * b > 256
    (96, (8, 8, 8, 8), (0, 0, 1, 2)),       # 64 sequences x 3 tiles = 192 tiles against 48 alone: the ordinary rconv_lds form both ways
    (225, (8, 8, 8, 8), (0, 1, 1, 2)),      # 64 sequences x 8 tiles = 512 tiles: rconv_lds's SHARE form joined, the ordinary one alone
    (385, (1, 2), (0, 2)),                  # unfused attention (t > 384); the batch joins at the first one's last step
])
def test_fullsize_batches_join_a_running_solve_bit_identical(full_flow, t, rows, joins):
    cfg, fd = full_flow
    batches = [_batch(cfg, b, t, 1000 * i + t) for i, b in enumerate(rows)]
    _check(fd, t, batches, joins)


def test_tiny_pipeline_with_joined_render_is_bit_identical_to_sequential():
    """PipelinedSynth(render_join=True) over six tiny batches: tokens, mel and waveform of every batch equal SynthEngine.tts of that
    batch, and drain() returns all six.  The render worker is held until every batch's tokens are ready, so that four batches of the
    same frame count share one solve whatever the timing; the fifth of that frame count finds the session's four slots taken and the
    sixth has another frame count: both are rendered alone.  A second round runs ungated."""
    from astts.synth.config import SynthConfig
    from astts.synth.model import PipelinedSynth, SynthEngine
    from astts.synth.weights import make_all

    cfg = SynthConfig.tiny()
    eng = SynthEngine(make_all(cfg, 0), cfg, DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    nh = cfg.nb_harmonics + 1
    batches = []
    for B, Tt, Tp, Ts in ((4, 9, 14, 24), (8, 6, 14, 24), (2, 12, 14, 24), (5, 7, 14, 24), (3, 9, 14, 24), (4, 9, 10, 33)):
        tmp, tm = cfg.mel_frames_for_tokens(Tp), cfg.mel_frames_for_tokens(Ts)
        phase0 = (torch.rand(B, nh, device=DEV, generator=g) * 2 - 1) * math.pi
        phase0[:, 0] = 0
        batches.append((torch.randint(0, cfg.text_vocab, (B, Tt), device=DEV, generator=g), torch.full((B,), Tt, dtype=torch.int32, device=DEV),
                        torch.randn(B, cfg.spk_dim, device=DEV, generator=g), torch.randint(0, cfg.speech_vocab, (B, Tp), device=DEV, generator=g),
                        Ts, torch.rand(Ts, B, 2, device=DEV, generator=g), torch.randint(0, cfg.speech_vocab, (B, Tp), device=DEV, generator=g),
                        torch.randn(B, tmp, cfg.mel, device=DEV, generator=g), torch.randn(B, cfg.spk_dim, device=DEV, generator=g),
                        torch.randn(B, tmp + tm, cfg.mel, device=DEV, generator=g), phase0,
                        torch.randn(B, tm * cfg.upsample_total, nh, device=DEV, generator=g)))
    refs = [eng.tts(*a) for a in batches]
    torch.cuda.synchronize()
    pipe = PipelinedSynth(eng, lm_depth=3, lm_priority=0, render_priority=0, join=True, render_join=True)
    assert pipe.join and pipe.render_join
    try:
        for gated in (True, False):
            outs = []
            if gated:
                pipe._renderer.gate.clear()
            with torch.cuda.stream(pipe.front_stream):
                for a in batches:
                    r = pipe.submit(*a)           # six slots (three chains x two): nothing is rendered by submit
                    if r is not None:
                        outs.append(r)
                if gated:
                    assert not outs
                    for it in list(pipe._fifo):
                        it["fut"].result()        # every batch's last decode step is enqueued
                    torch.cuda.synchronize()      # ... and has run: a busy session admits a batch only once its tokens are there
                    pipe._renderer.gate.set()
                outs += pipe.drain()
            torch.cuda.synchronize()
            assert len(outs) == 6
            for o, r in zip(outs, refs):
                assert torch.equal(o[0], r[0]) and torch.equal(o[1], r[1]) and torch.equal(o[2], r[2]), gated
            if gated:
                passes, carried = pipe._renderer.stats()
                assert passes == cfg.cfm_steps and carried == 4 * cfg.cfm_steps      # four batches, one solve
    finally:
        pipe.close()
