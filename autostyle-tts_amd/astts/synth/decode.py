"""Decode state of the acoustic LM on the host: what a prefill leaves behind (``Prefill``), the buffers and C arguments of one decode
(``DecodeJob``), decode sessions that a second batch can join (``LmSession``) and the runner for batches of more than 32 rows."""
from __future__ import annotations

import ctypes
import sys
import threading
from dataclasses import dataclass
from typing import List, Optional

import torch

from .. import _lib, _lib_session, ops


def record_streams(tensors, stream) -> None:
    """Tell the caching allocator that these tensors (non-tensors are skipped) are read on ``stream``, not only on the stream they were
    allocated on: otherwise their blocks are recycled under kernels still in flight there."""
    for t in tensors:
        if isinstance(t, torch.Tensor):
            t.record_stream(stream)


def _eos_min(ignore_eos, n_steps: int) -> int:
    """True -> EOS masked for the whole fixed-length decode; False -> never; int -> masked for that many steps;
    int32 device tensor [B] -> per-row step counts (handled by the engine; scalar fallback 0)."""
    if torch.is_tensor(ignore_eos):
        return 0
    if ignore_eos is True:
        return n_steps
    if ignore_eos is False:
        return 0
    return int(ignore_eos)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


@dataclass(eq=False)
class Prefill:
    """``AcousticLM.prefill``: the KV cache of a prefix of ``s0`` positions (room for ``n_steps`` more) and the logits of its last one."""
    cache: List[torch.Tensor]
    logits0: torch.Tensor
    s0: int
    b: int
    n_steps: int
    key_start: Optional[torch.Tensor] = None

    def tensors(self) -> List[torch.Tensor]:
        return list(self.cache) + [self.logits0] + ([self.key_start] if self.key_start is not None else [])


@dataclass(eq=False)
class DecodeJob:
    """One decode of a prefilled batch (b <= 32 rows, or the wide engine's): token history, optional logits plane, sampler inputs and
    ``next``, the first step not enqueued yet.  ``ws*``: the engine workspace of a decode issued by ``AcousticLM.decode_range`` (it
    carries the logits from one range of steps to the next); ``slot``: the session slot of one admitted by ``LmSession.admit``, which
    also lets go of ``prefill`` (the session has copied its cache and logits)."""
    prefill: Optional[Prefill]
    n_steps: int
    toks: torch.Tensor
    logits: Optional[torch.Tensor]
    forced: Optional[torch.Tensor]
    u: torch.Tensor
    ignore_eos: object
    next: int = 0
    ws: Optional[torch.Tensor] = None
    ws_aligned: int = 0
    ws_bytes: int = 0
    slot: Optional[int] = None

    @classmethod
    def begin(cls, state: Prefill, vocab: int, uniforms: torch.Tensor, ignore_eos=True, forced_tokens: Optional[torch.Tensor] = None,
              return_logits: bool = False) -> "DecodeJob":
        """Allocate the buffers of one decode of ``state`` on its device (current stream); ``vocab``: width of a logits row."""
        b, n_steps, dev = state.b, state.n_steps, state.logits0.device
        return cls(state, n_steps, toks=torch.zeros((b, n_steps), dtype=torch.int32, device=dev),
                   logits=torch.empty((b, n_steps, vocab), dtype=torch.float32, device=dev) if return_logits else None,
                   forced=None if forced_tokens is None else forced_tokens.to(torch.int32).contiguous(),
                   u=uniforms.to(torch.float32).contiguous(), ignore_eos=ignore_eos)

    def c_args(self):
        """The arguments ``astts_lm_decode`` and ``astts_lm_session_admit`` share, as the two runs in which both signatures list them:
        (logits0, kv_cache, key_start, t_max, b, pos0, n_steps) and (uniforms, forced_tokens, eos_min_steps, eos_min_rows, tokens_out,
        logits_out)."""
        p, n, ie = self.prefill, self.n_steps, self.ignore_eos
        ptrs = (ctypes.c_void_p * len(p.cache))(*[c.data_ptr() for c in p.cache])
        return ((p.logits0.data_ptr(), ptrs, _ptr(p.key_start), p.s0 + n, p.b, p.s0, n),
                (self.u.data_ptr(), _ptr(self.forced), _eos_min(ie, n), ie.data_ptr() if torch.is_tensor(ie) else None,
                 self.toks.data_ptr(), _ptr(self.logits)))

    def decode(self, lib, eng, s_end: Optional[int], stream_ptr: int) -> None:
        """Enqueue steps [next, s_end) with ``astts_lm_decode`` on the stream ``stream_ptr`` names."""
        s_end = self.n_steps if s_end is None else min(int(s_end), self.n_steps)
        if s_end <= self.next:
            return
        head, tail = self.c_args()
        _lib.check(lib.astts_lm_decode(eng, *head, self.next, s_end, *tail, self.ws_aligned, self.ws_bytes, stream_ptr))
        self.next = s_end

    def admit(self, lib, session) -> int:
        """``astts_lm_session_admit`` on the current stream -> the slot the batch was given."""
        head, tail = self.c_args()
        slot = ctypes.c_int32(-1)
        _lib.check(lib.astts_lm_session_admit(session, *head, *tail, ctypes.byref(slot)))
        self.slot = int(slot.value)
        return self.slot


class LmSession:
    """One decode chain of the C++ engine that up to two prefilled batches share (include/session/astts_lm_session.h): a batch
    admitted while another is decoding JOINS it, and the chain's launches (72 per token, each a latency link) carry the rows of both.
    Every row's tokens and logits are bit-identical to ``AcousticLM.decode_prefilled`` of its batch alone (tested).

    ``rows_max`` <= 32 rows in all; ``t_arena`` >= twice the longest window (prefix + steps - 1) that will be admitted.  The session
    allocates layers * t_arena * rows_max * 4 d bytes of cache arena (0.94 GB at CosyVoice-300M widths, 1024 positions, 16 rows).
    All calls enqueue on ``stream`` (the stream current at construction by default) and none waits for the GPU; they are not
    thread-safe: one thread drives a session."""

    def __init__(self, lm, rows_max: int, t_arena: int, stream=None):
        self.lm, self.rows_max, self.t_arena = lm, int(rows_max), int(t_arena)
        self.stream = stream if stream is not None else torch.cuda.current_stream(lm.device)
        self._lib = _lib_session.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.astts_lm_session_create(lm._engine(), self.rows_max, self.t_arena, _lib.stream_ptr(self.stream), ctypes.byref(h)))
        self._h = h
        self._ctx = [None, None]          # per slot: the job of the batch that holds it (its buffers are read by kernels until its last step)

    def close(self) -> None:
        if self._h is not None:
            h, self._h = self._h, None
            _lib.check(self._lib.astts_lm_session_destroy(h))

    def __del__(self):
        if sys is None or sys.is_finalizing():      # at interpreter exit the process gives the memory back
            return
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass

    @property
    def max_window(self) -> int:
        return self.t_arena // 2

    def active(self) -> int:
        return sum(c is not None for c in self._ctx)

    def steps_left(self) -> List[int]:
        """Steps still to be enqueued, per admitted batch."""
        return [c.n_steps - c.next for c in self._ctx if c is not None]

    def can_admit(self, b: int, s0: int, n_steps: int) -> bool:
        return int(self._lib.astts_lm_session_can_admit(self._h, int(b), int(s0), int(n_steps))) >= 0

    def admit(self, state: Prefill, uniforms: torch.Tensor, ignore_eos=True, forced_tokens: Optional[torch.Tensor] = None,
              return_logits: bool = False) -> DecodeJob:
        """``state``: what ``AcousticLM.prefill`` returned.  -> the batch's job: ``job.toks`` (and ``job.logits``) are complete
        once ``step`` has returned it.  The prefill's cache is copied into the session's arena (stream order)."""
        with torch.cuda.stream(self.stream):
            job = DecodeJob.begin(state, self.lm.cfg.speech_vocab + 1, uniforms, ignore_eos, forced_tokens, return_logits)
            job.admit(self._lib, self._h)
        # the prefill's cache and first logits are read by the admission on this session's stream only: tell the allocator, then let go
        record_streams(state.tensors(), self.stream)
        job.prefill = None
        self._ctx[job.slot] = job
        return job

    def step(self, k: int) -> List[DecodeJob]:
        """Enqueue up to ``k`` token steps of every admitted batch as one chain.  -> the jobs of the batches that ended."""
        mask = ctypes.c_uint32(0)
        live = [c for c in self._ctx if c is not None]
        k = int(k)
        with torch.cuda.stream(self.stream):
            _lib.check(self._lib.astts_lm_session_step(self._h, k, ctypes.byref(mask)))
        done = []
        for c in live:
            c.next = min(c.n_steps, c.next + k)
        for slot in (0, 1):
            if mask.value >> slot & 1:
                done.append(self._ctx[slot])
                self._ctx[slot] = None
        return done

    def run(self) -> None:
        """Enqueue every remaining step of the admitted batches."""
        while self.active():
            self.step(max(self.steps_left()))


def decode_groups(lm, prefix: torch.Tensor, n_steps: int, uniforms: torch.Tensor, ignore_eos=True,
                  forced_tokens: Optional[torch.Tensor] = None, return_logits: bool = False,
                  key_start: Optional[torch.Tensor] = None, group_steps: Optional[List[int]] = None):
    """``AcousticLM.decode`` of more than 32 rows (BASELINE config 3: 64 long-form utterances): independent rows, decoded in groups
    of 32.  The groups are separate launch chains, latency-bound like any decode, so two of them run concurrently on their own streams
    (each enqueued by its own host thread: the engine call drops the GIL); results do not depend on the grouping or on what runs beside
    them.
    ``group_steps``: group g decodes only group_steps[g] <= n_steps steps (ragged batches sorted by length: the rows of a later group
    need fewer); its tokens come back zero-padded to n_steps."""
    b = prefix.shape[1]
    groups = [slice(b0, min(b0 + 32, b)) for b0 in range(0, b, 32)]
    if group_steps is not None and (len(group_steps) != len(groups) or return_logits or max(group_steps) > n_steps):
        raise ValueError("AcousticLM.decode: group_steps needs one step count <= n_steps per 32-row group (and no return_logits)")
    if getattr(lm, "_group_streams", None) is None:
        lm._group_streams = ops.concurrent_streams(2, device=lm.device)
    cur = torch.cuda.current_stream(lm.device)
    outs, errs = [None] * len(groups), []

    def run(gi, st):
        try:
            sl = groups[gi]
            with torch.cuda.device(lm.device), torch.cuda.stream(st):
                n_g = n_steps if group_steps is None else int(group_steps[gi])
                o = lm.decode_engine(prefix[:, sl].contiguous(), n_g, uniforms[:n_g, sl].contiguous(),
                                     ignore_eos[sl].contiguous() if torch.is_tensor(ignore_eos) else ignore_eos,
                                     None if forced_tokens is None else forced_tokens[sl, :n_g].contiguous(), return_logits,
                                     None if key_start is None else key_start[sl].contiguous())
                if n_g < n_steps:
                    o = torch.nn.functional.pad(o, (0, n_steps - n_g))
                outs[gi] = o
        except BaseException as e:      # noqa: BLE001  (re-raised on the calling thread)
            errs.append(e)

    for w0 in range(0, len(groups), 2):
        wave = []
        for k, gi in enumerate(range(w0, min(w0 + 2, len(groups)))):
            st = lm._group_streams[k]
            st.wait_stream(cur)
            th = threading.Thread(target=run, args=(gi, st))
            th.start()
            wave.append((th, st))
        for th, st in wave:
            th.join()
            cur.wait_stream(st)
    if errs:
        raise errs[0]
    for o in outs:
        record_streams(o if isinstance(o, tuple) else (o,), cur)
    if return_logits:
        return torch.cat([o[0] for o in outs], 0), torch.cat([o[1] for o in outs], 0)
    return torch.cat(outs, 0)
