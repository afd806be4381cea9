"""The synthesis host's pure parts (astts/synth/pipeline.py, astts/synth/decode.py), without a GPU: which probed stream plays which
part, what a decode chain accepts, which batches may share a chain, and the C arguments of one decode."""
import ctypes
import itertools
from types import SimpleNamespace

import pytest
import torch

SIZES = [[1], [3], [1, 1], [2, 1], [1, 1, 1], [1, 1, 1, 1], [2, 2, 2, 2]]


@pytest.mark.parametrize("sizes,depth", list(itertools.product(SIZES, (1, 2, 3))))
def test_plan_streams_properties(sizes, depth):
    from astts.synth.pipeline import plan_streams

    render, lm, front = plan_streams(sizes, depth)
    n = len(sizes)
    assert render == (0, 0) and len(lm) == depth
    if n > 1:
        assert all(s is None or s[0] != 0 for s in lm)                   # a decode chain never shares render's pipe
    if n >= depth + 2:                                                   # a pipe each
        classes = [render[0]] + [s[0] for s in lm] + [front[0]]
        assert len(set(classes)) == depth + 2 and all(s[1] == 0 for s in [render, front] + lm)
    else:
        assert front == ((0, 1) if sizes[0] > 1 else None)
    given = [s for s in [render, front] + lm if s is not None]
    assert len(set(given)) == len(given)                                 # no stream handed out twice
    assert all(0 <= c < n and 0 <= j < sizes[c] for c, j in given)       # past a class's end: None (a fresh stream), never an index


def test_plan_streams_pinned():
    """Worked by hand from the assignment as it stood inside PipelinedSynth.__init__ before plan_streams existed."""
    from astts.synth.pipeline import plan_streams

    # two pipes, three roles + front: render first of pipe 0, front its second stream; both chains want pipe 1, which has one stream
    assert plan_streams([2, 1], 2) == ((0, 0), [(1, 0), None], (0, 1))
    # four pipes for render + two chains + front: the first stream of each, in that order
    assert plan_streams([1, 1, 1, 1], 2) == ((0, 0), [(1, 0), (2, 0)], (3, 0))
    # one pipe: its streams 0 and 1 are render's and front's, chains take what follows
    assert plan_streams([3], 2) == ((0, 0), [(0, 2), None], (0, 1))


def _chain(max_window=1024):
    from astts.synth.pipeline import _JoinChain

    return _JoinChain(lm=object(), device=None, stream=None, index=0, quantum=16, ahead=2, max_window=max_window)


def test_join_chain_reserve():
    ch = _chain()
    assert not ch.reserve(1025)                       # past the position tables
    assert ch.occupied() == 0
    assert ch.reserve(300) and ch._half == 384        # idle: accepted, the half rounded up to 128
    assert not ch.reserve(385)                        # longer than the held half while a batch is running
    assert ch.reserve(384) and ch._half == 384
    assert not ch.reserve(10)                         # two are held: a third is refused
    assert ch.occupied() == 2
    ch._occupied = 0                                  # both handed over
    assert ch.reserve(385) and ch._half == 512        # idle again: the longer window is taken
    ch._occupied = 0
    assert ch.reserve(1000) and ch._half == 1024      # 1024 is a multiple of 128 and the cap
    capped = _chain(max_window=1000)
    assert capped.reserve(999) and capped._half == 1000      # rounded to 1024, capped at max_window
    assert not capped.reserve(1001)


def test_join_chain_reserve_dead_chain_raises():
    ch = _chain()
    ch._dead = ValueError("boom")
    with pytest.raises(RuntimeError, match="decode chain 0 stopped"):
        ch.reserve(10)


def _lm_args(rows=8, text_len=5, prompt_len=7, n_tokens=6, u_steps=6):
    from astts.synth.pipeline import LmArgs

    return LmArgs(torch.zeros(rows, text_len, dtype=torch.int64), torch.full((rows,), text_len, dtype=torch.int32),
                  torch.randn(rows, 4), torch.zeros(rows, prompt_len, dtype=torch.int64), n_tokens, torch.rand(u_steps, rows, 2))


def test_lm_args_concat_and_compatible():
    from astts.synth.pipeline import LmArgs, PipelinedSynth

    compatible = lambda a, b, rows_max=32: PipelinedSynth._compatible(SimpleNamespace(lm_rows_max=rows_max), a, b)      # noqa: E731
    a, b = _lm_args(rows=8), _lm_args(rows=24)
    assert compatible(a, b)                                              # same lengths, 32 rows together
    assert not compatible(a, _lm_args(text_len=6))
    assert not compatible(a, _lm_args(prompt_len=8))
    assert not compatible(a, _lm_args(n_tokens=7))
    assert not compatible(a, _lm_args(u_steps=7))
    assert not compatible(a, _lm_args(rows=25)) and compatible(a, _lm_args(rows=25), 256)      # 33 rows
    c = LmArgs.concat([a, b])
    assert isinstance(c, LmArgs) and c.n_tokens == a.n_tokens
    for name in ("text", "text_lens", "lm_spk", "lm_prompt_tokens"):
        assert torch.equal(getattr(c, name), torch.cat([getattr(a, name), getattr(b, name)], 0)), name
    assert torch.equal(c.uniforms, torch.cat([a.uniforms, b.uniforms], 1))      # uniforms are [steps, rows, 2]
    assert len(tuple(c)) == 6 and c[4] == a.n_tokens                     # still the positional arguments of tts_tokens


class _Recorder:
    """In place of the library handle: records the arguments of whichever entry point is called and reports success."""

    def __init__(self):
        self.calls = {}

    def __getattr__(self, name):
        def call(*args):
            self.calls[name] = args
            if name == "astts_lm_session_admit":
                args[-1]._obj.value = 1                                  # slot_out (ctypes.byref keeps its object)
            return 0
        return call


@pytest.mark.parametrize("ignore_eos", [True, 3, "rows"])
def test_decode_job_argument_block_is_shared(ignore_eos):
    from astts.synth.decode import DecodeJob, Prefill

    b, s0, n, vocab = 3, 5, 4, 11
    ks = torch.zeros(b, dtype=torch.int32)
    state = Prefill([torch.zeros(s0 + n, b, 8, dtype=torch.float16) for _ in range(2)], torch.zeros(b, vocab), s0, b, n, ks)
    ie = torch.tensor([0, 1, 2], dtype=torch.int32) if ignore_eos == "rows" else ignore_eos
    job = DecodeJob.begin(state, vocab, torch.rand(n, b, 2), ie, torch.zeros(b, n, dtype=torch.int64), return_logits=True)
    assert job.toks.shape == (b, n) and job.toks.dtype == torch.int32 and job.logits.shape == (b, n, vocab)
    assert job.forced.dtype == torch.int32 and job.u.dtype == torch.float32 and job.next == 0
    job.ws_aligned, job.ws_bytes = 4096, 512
    lib = _Recorder()
    job.decode(lib, "ENGINE", 3, 77)
    assert job.next == 3
    assert job.admit(lib, "SESSION") == 1 and job.slot == 1
    dec, adm = lib.calls["astts_lm_decode"], lib.calls["astts_lm_session_admit"]
    assert len(dec) == 19 and len(adm) == 15                             # the two C signatures
    norm = lambda v: list(v) if isinstance(v, ctypes.Array) else v       # noqa: E731
    # handle | logits0 kv_cache key_start t_max b pos0 n_steps | (s_begin s_end) | uniforms forced eos_min eos_rows tokens logits | rest
    assert [norm(v) for v in dec[1:8]] == [norm(v) for v in adm[1:8]]
    assert list(dec[10:16]) == list(adm[8:14])
    assert dec[0] == "ENGINE" and adm[0] == "SESSION" and dec[8:10] == (0, 3) and dec[16:] == (4096, 512, 77)
    assert dec[1] == state.logits0.data_ptr() and norm(dec[2]) == [c.data_ptr() for c in state.cache] and dec[3] == ks.data_ptr()
    assert dec[4:8] == (s0 + n, b, s0, n)
    assert dec[10] == job.u.data_ptr() and dec[11] == job.forced.data_ptr()
    assert dec[12:14] == {True: (n, None), 3: (3, None)}.get(ignore_eos, (0, ie.data_ptr() if torch.is_tensor(ie) else None))
    assert dec[14] == job.toks.data_ptr() and dec[15] == job.logits.data_ptr()
    lib.calls.clear()
    job.decode(lib, "ENGINE", 3, 77)                                     # nothing left before step 3: no call
    assert job.next == 3 and not lib.calls


def test_eos_min():
    from astts.synth.decode import _eos_min

    assert _eos_min(True, 9) == 9
    assert _eos_min(False, 9) == 0
    assert _eos_min(4, 9) == 4
    assert _eos_min(torch.tensor([1, 2], dtype=torch.int32), 9) == 0
