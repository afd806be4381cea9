"""Decode sessions (csrc/lm_engine.hip: astts_lm_session_*, astts.synth.decode.LmSession): a batch that JOINS a running decode chain
gets, bit for bit, the logits (teacher forced) and the tokens (free running) of the same batch decoded alone by astts_lm_decode --
torch.equal, no tolerance: every decode kernel is row-independent and the attention only sees positions relative to the query."""
import dataclasses
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def tiny_lm():
    from astts.synth.config import SynthConfig
    from astts.synth.model import AcousticLM
    from astts.synth.weights import make_all

    cfg = dataclasses.replace(SynthConfig.tiny(), max_positions=1024)      # tiny widths; tables long enough for 520-key windows
    sd = make_all(cfg, 0)["llm"]
    return cfg, sd, AcousticLM(sd, cfg, torch.device(DEV))


def _batch(lm, cfg, b, tt, tp, steps, seed, ragged=None):
    """One batch: prefix, uniforms, forced tokens.  ragged: per-row (text, prompt) lengths -> left-padded prefix with key_start."""
    g = torch.Generator().manual_seed(seed)
    spk = torch.randn(b, cfg.spk_dim, generator=g)
    if ragged is None:
        text = torch.randint(0, cfg.text_vocab, (b, tt), generator=g)
        prompt = torch.randint(0, cfg.speech_vocab, (b, tp), generator=g)
        pre, ks = lm.prefix(text.to(DEV), torch.full((b,), tt, dtype=torch.int32, device=DEV), spk.to(DEV), prompt.to(DEV)), None
    else:
        texts = [torch.randint(0, cfg.text_vocab, (a,), generator=g) for a, _ in ragged]
        prompts = [torch.randint(0, cfg.speech_vocab, (p,), generator=g) for _, p in ragged]
        pre, ks = lm.prefix_ragged(texts, spk, prompts)
    return {"pre": pre, "ks": ks, "b": b, "steps": steps, "u": torch.rand(steps, b, 2, generator=g).to(DEV),
            "forced": torch.randint(0, cfg.speech_vocab, (b, steps), generator=g).to(DEV), "ignore_eos": True}


def _solo(lm, B, forced):
    """The reference: the batch alone through astts_lm_decode."""
    st = lm.prefill(B["pre"], B["steps"], B["ks"])
    toks, logits = lm.decode_prefilled(st, B["u"], B["ignore_eos"], B["forced"] if forced else None, return_logits=True)
    return toks.clone(), logits.clone()


def _joined(lm, batches, joins, forced, rows_max, t_arena):
    """Batch i is admitted when the chain has issued joins[i] steps (at once if the chain is idle).  forced: bool or one per batch.
    -> [(toks, logits)] and the session's final state (active mask, position, left 0, left 1, rebases, longest window)."""
    import ctypes

    flags = forced if isinstance(forced, (list, tuple)) else [forced] * len(batches)
    sess = lm.session(rows_max, t_arena)
    pending = sorted(range(len(batches)), key=lambda i: joins[i])
    ctx = [None] * len(batches)
    t = 0
    while pending or sess.active():
        while pending and (joins[pending[0]] <= t or not sess.active()):
            i = pending.pop(0)
            B = batches[i]
            st = lm.prefill(B["pre"], B["steps"], B["ks"])
            assert sess.can_admit(B["b"], st.s0, B["steps"]), (i, t)
            ctx[i] = sess.admit(st, B["u"], B["ignore_eos"], B["forced"] if flags[i] else None, return_logits=True)
            t = max(t, joins[i])
        k = min(sess.steps_left())
        if pending:
            k = min(k, joins[pending[0]] - t)
        done = sess.step(k)
        assert all(c.next == c.n_steps for c in done)
        t += k
    state = (ctypes.c_int32 * 6)()
    assert sess._lib.astts_lm_session_state(sess._h, state) == 0
    torch.cuda.synchronize()
    sess.close()
    return [(c.toks, c.logits) for c in ctx], list(state)


def _assert_joined_equals_solo(lm, batches, joins, rows_max, t_arena=None):
    if t_arena is None:
        t_arena = 2 * max(B["pre"].shape[0] + B["steps"] - 1 for B in batches)
    state = None
    for forced in (True, False):
        got, state = _joined(lm, batches, joins, forced, rows_max, t_arena)
        for i, B in enumerate(batches):
            toks, logits = _solo(lm, B, forced)
            assert torch.equal(got[i][0], toks), (i, forced)
            assert torch.equal(got[i][1], logits), (i, forced)
            if forced:
                assert torch.equal(toks, B["forced"].to(torch.int32))
    assert state[0] == 0
    return state


# (rows A, steps A, rows B, steps B, step of A at which B joins)
@pytest.mark.parametrize("ba,na,bb,nb,join", [(3, 20, 5, 30, 1),      # more rows, longer: A ends first
                                               (6, 30, 2, 12, 15),     # fewer rows, shorter: B ends first, in the middle of A
                                               (4, 16, 8, 24, 15),     # joins at A's last step (A only samples there)
                                               (8, 24, 8, 12, 12)])    # both end on the same step
def test_tiny_group_joins_a_running_chain_bit_identical(tiny_lm, ba, na, bb, nb, join):
    cfg, _, lm = tiny_lm
    A = _batch(lm, cfg, ba, 7, 11, na, 10 * ba + na)
    B = _batch(lm, cfg, bb, 5, 17, nb, 10 * bb + nb + 1)
    _assert_joined_equals_solo(lm, [A, B], [0, join], rows_max=16)


def test_tiny_third_group_takes_a_freed_slot_over_stale_keys(tiny_lm):
    """C lands in the rows A left, with a SHORTER prefix: the arena positions in front of its first key still hold A's keys."""
    cfg, _, lm = tiny_lm
    A = _batch(lm, cfg, 4, 9, 30, 14, 1)
    B = _batch(lm, cfg, 4, 6, 12, 40, 2)
    C = _batch(lm, cfg, 3, 3, 4, 20, 3)
    _assert_joined_equals_solo(lm, [A, B, C], [0, 5, 14], rows_max=8)


def test_tiny_ragged_group_with_row_eos_windows_joins_a_plain_one(tiny_lm):
    cfg, _, lm = tiny_lm
    A = _batch(lm, cfg, 3, 8, 9, 24, 21)
    R = _batch(lm, cfg, 5, 0, 0, 16, 22, ragged=[(5, 9), (17, 30), (11, 3), (1, 22), (8, 8)])
    R["ignore_eos"] = torch.tensor([0, 3, 16, 7, 1], dtype=torch.int32, device=DEV)
    _assert_joined_equals_solo(lm, [A, R], [0, 6], rows_max=8)
    _assert_joined_equals_solo(lm, [R, A], [0, 3], rows_max=8)


def _boundary_batches(lm, cfg, rows):
    """Valid keys pass 128 -> 129, 256 -> 257 and 512 -> 513 during the run: 64, 128 and 256 keys per key half (lm_attn: the halves'
    size steps there, and 256 keys are one chunk)."""
    out = []
    for i, n_keys in enumerate((129, 257, 513)):
        B = _batch(lm, cfg, rows, 8, 8, 14, 40 + i)
        s0 = B["pre"].shape[0]
        B = _batch(lm, cfg, rows, 8, 8 + (n_keys - 7) - s0, 14, 40 + i)        # the prefix ends 7 keys short of the boundary
        assert B["pre"].shape[0] == n_keys - 7
        out.append(B)
    return out


def test_tiny_shifted_windows_cross_the_attention_boundaries(tiny_lm):
    cfg, _, lm = tiny_lm
    _assert_joined_equals_solo(lm, _boundary_batches(lm, cfg, 3), [0, 4, 14], rows_max=8)


def test_tiny_rebase_at_the_smallest_arena_with_two_groups_active(tiny_lm):
    cfg, _, lm = tiny_lm
    batches = [_batch(lm, cfg, 2 + i, 5, 4 + i, 40, 60 + i) for i in range(3)]
    w = max(B["pre"].shape[0] + 39 for B in batches)
    assert 40 < w < 60                    # the chain starts at w and is rebased after w steps: B (20..60) and C (40..80) are active
    state = _assert_joined_equals_solo(lm, batches, [0, 20, 40], rows_max=16, t_arena=2 * w)
    assert state[4] >= 1 and state[5] == w


def test_tiny_two_group_sampler_matches_the_oracle_sampler(tiny_lm):
    """One launch samples both groups: different step indices, forced tokens in one group only, EOS may be produced in one group and
    not in the other.  The free group's tokens are the oracle sampler's on the engine's own logits."""
    from oracle import synth as osyn

    cfg, _, lm = tiny_lm
    A = _batch(lm, cfg, 3, 6, 9, 18, 71)
    B = _batch(lm, cfg, 5, 4, 13, 14, 72)
    for free, other in ((A, B), (B, A)):
        free["ignore_eos"], other["ignore_eos"] = False, True
        got, _ = _joined(lm, [A, B], [0, 7], [free is not A, free is not B], 8, 128)
        toks, logits = (x.cpu() for x in got[0 if free is A else 1])
        oth = got[1 if free is A else 0]
        assert torch.equal(oth[0], other["forced"].to(torch.int32))
        u = free["u"].cpu()
        for s in range(free["steps"]):
            ref = osyn.ras_sample(logits[:, s], toks[:, :s].long(), u[s], cfg.top_k, cfg.top_p, cfg.ras_win, cfg.ras_tau, cfg.speech_vocab,
                                  False, cfg.eos_policy)
            assert ref.tolist() == toks[:, s].tolist(), s
        st, sl = _solo(lm, free, False)
        assert torch.equal(st.cpu(), toks) and torch.equal(sl.cpu(), logits)


@pytest.fixture(scope="module")
def full_lm():
    from astts.synth.config import SynthConfig
    from astts.synth.model import AcousticLM
    from astts.synth.weights import make_lm_weights

    cfg = SynthConfig()
    sd = make_lm_weights(cfg, 0)
    return cfg, sd, AcousticLM(sd, cfg, torch.device(DEV))


def test_fullsize_two_eight_row_groups_join_at_step_11(full_lm):
    """CosyVoice-300M widths, the benchmark's rows: bit-identical to the solo runs and within 3e-3 of the oracle's logits."""
    from oracle import synth as osyn

    cfg, sd, lm = full_lm
    steps = 30
    batches, refs = [], []
    for seed in (5, 6):
        g = torch.Generator().manual_seed(seed)
        b, tt, tp = 8, 12, 20
        text = torch.randint(0, cfg.text_vocab, (b, tt), generator=g)
        spk = torch.randn(b, cfg.spk_dim, generator=g)
        prompt = torch.randint(0, cfg.speech_vocab, (b, tp), generator=g)
        forced = torch.randint(0, cfg.speech_vocab, (b, steps), generator=g)
        u = torch.rand(steps, b, 2, generator=g)
        pre_ref = osyn.lm_prefix(sd, cfg, text, torch.full((b,), tt), spk, prompt)
        refs.append(osyn.lm_decode(sd, cfg, pre_ref, steps, u, True, forced)[1])
        pre = lm.prefix(text.to(DEV), torch.full((b,), tt, dtype=torch.int32, device=DEV), spk.to(DEV), prompt.to(DEV))
        batches.append({"pre": pre, "ks": None, "b": b, "steps": steps, "u": u.to(DEV), "forced": forced.to(DEV), "ignore_eos": True})
    _assert_joined_equals_solo(lm, batches, [0, 11], rows_max=16)
    got, _ = _joined(lm, batches, [0, 11], True, 16, 256)
    for i in range(2):
        err = float((got[i][1].cpu() - refs[i]).abs().max()) / float(refs[i].abs().max())
        print(f"full size joined group {i}: logits rel err vs oracle {err:.2e}")
        assert err < 3e-3


def test_fullsize_shifted_windows_cross_the_attention_boundaries(full_lm):
    cfg, _, lm = full_lm
    _assert_joined_equals_solo(lm, _boundary_batches(lm, cfg, 2), [0, 4, 14], rows_max=4)


def test_tiny_pipeline_with_join_is_bit_identical_to_sequential():
    """PipelinedSynth(join=True) over five small batches of different shapes: tokens, mel and waveform of every batch equal
    SynthEngine.tts of that batch (the twin of test_fullsize_pipeline_and_cobatching_are_bit_identical_to_sequential).  The chains'
    threads are held until the first two batches are queued, so that the second is admitted beside the first whatever the timing (a
    tiny decode is enqueued in less time than a submit takes); the third batch's window (about 180 keys) is longer than the 128
    positions the first batch sized its chain for: with one chain the arena is replaced once the chain is empty, with two the idle
    chain is sized for it."""
    from astts.synth.config import SynthConfig
    from astts.synth.model import PipelinedSynth, SynthEngine
    from astts.synth.weights import make_all

    cfg = SynthConfig.tiny()
    eng = SynthEngine(make_all(cfg, 0), cfg, DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    nh = cfg.nb_harmonics + 1
    batches = []
    for B, Tt, Tp, Ts in ((4, 9, 14, 40), (8, 6, 10, 24), (2, 12, 130, 33), (5, 7, 9, 12), (8, 9, 14, 40)):
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
    for depth in (1, 2):
        pipe = PipelinedSynth(eng, lm_depth=depth, lm_priority=0, render_priority=0, join=True)
        assert pipe.join
        outs = []
        for ch in pipe._chains:
            ch.gate.clear()
        with torch.cuda.stream(pipe.front_stream):
            for i, a in enumerate(batches):
                if i == 2:
                    for ch in pipe._chains:
                        ch.gate.set()
                r = pipe.submit(*a)
                if r is not None:
                    outs.append(r)
            outs += pipe.drain()
        torch.cuda.synchronize()
        joins = sum(ch.joins for ch in pipe._chains)
        windows = [ch.session.max_window for ch in pipe._chains if ch.session is not None]
        pipe.close()
        assert joins >= 1, "no batch was admitted beside a running one"
        assert max(windows) >= 256 and (depth > 1 or windows == [256]), windows
        assert len(outs) == len(batches)
        for o, ref in zip(outs, refs):
            assert torch.equal(o[0], ref[0]) and torch.equal(o[1], ref[1]) and torch.equal(o[2], ref[2]), depth
