"""The stream pipeline over consecutive batches: decode chains beside the render stage (``PipelinedSynth``)."""
from __future__ import annotations

import os
import threading
import time
from collections import deque
from concurrent.futures import Future, ThreadPoolExecutor
from typing import List, NamedTuple, Optional, Tuple

import torch

from .. import _lib, ops
from .decode import Prefill, record_streams
from .lm import AcousticLM

Slot = Optional[Tuple[int, int]]      # (pipe class, stream within the class); None: a fresh stream


def plan_streams(class_sizes: List[int], depth: int) -> Tuple[Slot, List[Slot], Slot]:
    """Which probed stream plays which part, given the number of streams in each command-processor pipe class
    (ops.stream_pipe_classes: launch chains whose queues share a pipe take turns at every kernel boundary and run 2.4x slower each)
    -> (render, decode chains, front).  One pipe each in order of importance: the render stream, the ``depth`` decode chains, then
    the front stream for the caller's own per-batch work.  With fewer pipes than that the front stream (a few launches per batch)
    doubles up with the render stream's pipe, then decode chains double up among themselves -- never with the render stream, unless
    there is one pipe only."""
    n = len(class_sizes)
    if n >= depth + 2:
        return (0, 0), [(c, 0) for c in range(1, depth + 1)], (depth + 1, 0)
    front = (0, 1) if class_sizes[0] > 1 else None
    lm_classes = list(range(1, n)) if n > 1 else [0]
    lm = []
    for i in range(depth):
        c = lm_classes[i % len(lm_classes)]
        j = i // len(lm_classes) + (0 if n > 1 else 2)      # one pipe: its first two streams are render's and front's
        lm.append((c, j) if j < class_sizes[c] else None)
    return (0, 0), lm, front


class LmArgs(NamedTuple):
    """The LM stage's share of ``PipelinedSynth.submit``'s arguments, in the order ``SynthEngine.tts_tokens`` takes them."""
    text: torch.Tensor
    text_lens: torch.Tensor
    lm_spk: torch.Tensor
    lm_prompt_tokens: torch.Tensor
    n_tokens: int
    uniforms: torch.Tensor

    @property
    def rows(self) -> int:
        return int(self.text.shape[0])

    @classmethod
    def concat(cls, parts: List["LmArgs"]) -> "LmArgs":
        """Compatible batches side by side (rows are independent in every LM kernel: a row's tokens do not depend on its neighbours)."""
        a = parts
        return cls(torch.cat([x.text for x in a], 0), torch.cat([x.text_lens for x in a], 0), torch.cat([x.lm_spk for x in a], 0),
                   torch.cat([x.lm_prompt_tokens for x in a], 0), a[0].n_tokens, torch.cat([x.uniforms for x in a], 1))


def _lib_check_spin(us: int, stream) -> None:
    _lib.check(_lib.load().astts_stream_spin(int(us), int(stream.cuda_stream)))


class _JoinChain:
    """One decode chain of ``PipelinedSynth(join=True)``: a stream, an LmSession on it and the host thread that drives it -- admit
    what is waiting, enqueue a range of ``quantum`` steps, hand over every batch that ended, stay at most ``ahead`` ranges ahead of
    the GPU.

    The session's arena is sized by the SUBMITTING thread, under the chain's lock (``reserve``): the longest window it has accepted,
    rounded up to 128 positions and never past ``max_window`` (the position tables).  A longer batch is accepted only while the chain
    holds no batch (its session is then replaced by a larger one before the batch is admitted); otherwise the chain answers "not
    now"."""

    ROWS_MAX = 16            # two batches of up to 8 rows side by side (a wider arena spreads a row's keys further apart: lm_step.h)

    def __init__(self, lm, device, stream, index: int, quantum: int, ahead: int, max_window: int):
        self.lm, self.device, self.stream, self.index = lm, device, stream, index
        self.quantum, self.ahead, self.max_window = quantum, ahead, max_window
        self.session = None                 # created / replaced by the chain's thread only, at the size `_half` asks for
        self._cv = threading.Condition()
        self._waiting = deque()             # (state, uniforms, event, future) of batches not admitted yet
        self._occupied = 0                  # batches accepted and not handed over
        self._half = 0                      # longest window the chain has promised to take (arena = 2 * _half positions)
        self._stop = False
        self._dead = None                   # the exception that ended the chain's thread
        self._thread = None
        self.gate = threading.Event()       # cleared: the thread admits nothing and enqueues nothing (tests: queue two batches, then open)
        self.gate.set()
        self.joins = 0                      # batches admitted while another was decoding on this chain

    def occupied(self) -> int:
        with self._cv:
            return self._occupied

    def reserve(self, window: int) -> bool:
        """Take a slot for a batch with this window (prefix + steps - 1 keys) if the chain can hold it now.  Called by the submitting
        thread; on True the batch must be handed to ``submit``."""
        with self._cv:
            if self._dead is not None:
                raise RuntimeError(f"decode chain {self.index} stopped: {self._dead!r}") from self._dead
            if self._occupied >= 2 or window > self.max_window:
                return False
            if window > self._half:
                if self._occupied:
                    return False            # a running batch lives in the smaller arena
                self._half = min((window + 127) // 128 * 128, self.max_window)
            self._occupied += 1
            return True

    def submit(self, state: Prefill, lm_args: LmArgs) -> Future:
        cur = torch.cuda.current_stream(self.device)
        record_streams(lm_args, self.stream)           # read on the chain's stream for the whole decode (see PipelinedSynth._launch_group)
        record_streams(state.tensors(), self.stream)
        ready = torch.cuda.Event()
        ready.record(cur)                   # the prefill (and whatever built the inputs) on the caller's stream
        fut = Future()
        with self._cv:
            if self._dead is not None:
                self._occupied -= 1
                raise RuntimeError(f"decode chain {self.index} stopped: {self._dead!r}") from self._dead
            self._waiting.append((state, lm_args.uniforms, ready, fut))
            if self._thread is None:
                self._thread = threading.Thread(target=self._run, name=f"astts-join-chain-{self.index}", daemon=True)
                self._thread.start()
            self._cv.notify()
        return fut

    def close(self) -> None:
        with self._cv:
            self._stop = True
            self._cv.notify()
        self.gate.set()
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self.session is not None:
            self.session.close()
            self.session = None

    def _admit_waiting(self, futs) -> None:
        while True:
            with self._cv:
                if not self._waiting:
                    return
                state, u, ready, fut = self._waiting[0]
                half = self._half
            idle = self.session is None or not self.session.active()
            if idle and (self.session is None or self.session.max_window < half):
                if self.session is not None:          # the chain has promised a longer window than its arena holds: a larger one
                    self.session.close()
                    self.session = None
                self.session = self.lm.session(self.ROWS_MAX, 2 * half, self.stream)
            if not self.session.can_admit(state.b, state.s0, state.n_steps):
                if not idle:
                    return                            # no free rows beside the running batch: it goes in when that one has ended
                with self._cv:                        # an idle session that cannot take it never will: this batch fails, the chain goes on
                    self._waiting.popleft()
                    self._occupied -= 1
                fut.set_exception(RuntimeError(f"decode chain {self.index}: a batch of {state.b} rows with a window of "
                                               f"{state.s0 + state.n_steps - 1} keys does not fit a session of {self.ROWS_MAX} rows "
                                               f"and {self.session.max_window} keys"))
                continue
            self.joins += 0 if idle else 1
            self.stream.wait_event(ready)
            futs[id(self.session.admit(state, u, ignore_eos=True))] = fut
            with self._cv:
                self._waiting.popleft()

    def _run(self):
        ahead = deque()
        futs = {}
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                while True:
                    self.gate.wait()
                    with self._cv:
                        while not self._stop and not self._waiting and not (self.session is not None and self.session.active()):
                            self._cv.wait()
                        if self._stop:
                            return
                    self._admit_waiting(futs)
                    if not self.session.active():
                        continue
                    done = self.session.step(min(self.quantum, min(self.session.steps_left())))
                    mark = torch.cuda.Event()
                    mark.record(self.stream)
                    for job in done:
                        with self._cv:
                            self._occupied -= 1
                        futs.pop(id(job)).set_result(([job.toks], mark))
                    ahead.append(mark)
                    if len(ahead) > self.ahead:
                        ahead.popleft().synchronize()
        except BaseException as e:      # noqa: BLE001  (handed to whoever waits for a batch of this chain; later submits raise)
            with self._cv:
                self._dead = e
                pending = [w[3] for w in self._waiting]
                self._waiting.clear()
                self._occupied = 0
            for f in list(futs.values()) + pending:
                if not f.done():
                    f.set_exception(e)


class _JoinRender:
    """The render stage of ``PipelinedSynth(render_join=True)``: the render stream, a FlowSession on it and the host thread that drives
    it.  When a batch's tokens are ready the thread runs that batch's encoder (mu, speaker affine, prompt condition), admits it and
    enqueues ONE Euler step at a time for everything admitted -- a batch joins between two steps, and every launch of an estimator pass
    then carries the sequences of all admitted batches -- staying at most ``AHEAD`` steps ahead of the GPU (it waits for the event of
    the step before last on the host, here, never in the C call); the vocoder runs per batch when its solve ends.  A batch whose frame
    count differs from a busy session's, or that does not fit its rows, is rendered alone as without the session."""

    SLOTS, ROWS_MAX, AHEAD = 4, 32, 2

    def __init__(self, engine, stream):
        self.eng, self.device, self.stream = engine, engine.device, stream
        self.session = None                 # created / replaced by the worker's thread only
        self._cv = threading.Condition()
        self._waiting = []                  # items handed over and not admitted yet, oldest first
        self._stop = False
        self._dead = None
        self._thread = None
        self.passes = self.carried = 0      # estimator passes enqueued by sessions this worker has closed, and the batches they carried
        self.gate = threading.Event()       # cleared: the thread admits nothing and enqueues nothing (tests: queue the batches, then open)
        self.gate.set()

    def submit(self, item, ready) -> None:
        """``item["fut"]`` is set (its LM stage is launched); ``ready``: the event on the caller's stream behind which the item's render
        inputs exist.  ``item["rfut"]`` resolves to (toks, mel, wav) once the batch's vocoder is enqueued."""
        item["rfut"], item["ready"] = Future(), ready
        with self._cv:
            if self._dead is not None:
                raise RuntimeError(f"render worker stopped: {self._dead!r}") from self._dead
            self._waiting.append(item)
            if self._thread is None:
                self._thread = threading.Thread(target=self._run, name="astts-join-render", daemon=True)
                self._thread.start()
        item["fut"].add_done_callback(self._wake)

    def _wake(self, _fut=None) -> None:
        with self._cv:
            self._cv.notify()

    def stats(self):
        """(estimator passes enqueued, batches they carried summed): carried / passes = batches per shared pass"""
        s = self.session.state() if self.session is not None else [0] * 8
        return self.passes + s[2], self.carried + s[3]

    def close(self) -> None:
        with self._cv:
            self._stop = True
            self._cv.notify()
        self.gate.set()
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        self._drop_session()

    def _drop_session(self) -> None:
        if self.session is not None:
            self.passes, self.carried = self.stats()
            self.session.close()
            self.session = None

    def _take_ready(self):
        """The oldest waiting batch whose decode is enqueued to its end -- and, while the session is solving other batches, whose tokens
        are there already: the render stream has to wait for the tokens' event, and everything admitted would wait with it."""
        busy = self.session is not None and self.session.active() > 0
        with self._cv:
            for i, item in enumerate(self._waiting):
                fut = item["fut"]
                if fut.done() and (not busy or fut.exception() is not None or fut.result()[1].query()):
                    return self._waiting.pop(i)
        return None

    def _begin(self, item, jobs) -> None:
        """The batch's tokens are ready: encoder + admission (or the whole render, alone, when the session cannot take it)."""
        eng, sr = self.eng, self.stream
        try:
            parts, ev = item["fut"].result()
        except Exception as e:      # noqa: BLE001  (the batch's decode failed: that is this batch's result)
            item["rfut"].set_exception(e)
            return
        toks = parts[item["k"]]
        sr.wait_event(ev)
        sr.wait_event(item["ready"])
        toks.record_stream(sr)
        record_streams(item["render"], sr)      # the caller's tensors, read on the render stream
        ptok, pmel, spk, z, phase0, noise = item["render"]
        b = int(toks.shape[0])
        mel_total = int(pmel.shape[1]) + eng.cfg.mel_frames_for_tokens(toks.shape[1])
        idle = self.session is None or not self.session.active()
        if idle and b <= self.ROWS_MAX and (self.session is None or self.session.t != mel_total):
            self._drop_session()
            self.session = eng.flow.session(mel_total, self.SLOTS, self.ROWS_MAX, sr)
        if not eng.flow.use_engine or self.session is None or not self.session.can_admit(b, mel_total):
            mel, wav = eng.tts_render(toks, *item["render"])
            item["rfut"].set_result((toks, mel, wav))
            return
        all_tok = torch.cat([ptok.to(torch.int32), toks], dim=1)
        tok_lens = torch.full((b,), all_tok.shape[1], dtype=torch.int32, device=self.device)
        x, mu, spk_e, cond, tmp = eng.flow.prepare(all_tok, tok_lens, pmel, spk, z, mel_total)
        jobs[id(self.session.admit(x, mu, spk_e, cond))] = (item, toks, tmp)

    def _run(self):
        ahead = deque()
        jobs = {}
        item = None
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                while True:
                    self.gate.wait()
                    with self._cv:
                        while not self._stop and not (self.session is not None and self.session.active()) and \
                                not any(w["fut"].done() for w in self._waiting):
                            self._cv.wait()
                        if self._stop:
                            return
                    while True:
                        item = self._take_ready()
                        if item is None:
                            break
                        self._begin(item, jobs)
                        item = None
                    if self.session is None or not self.session.active():
                        continue
                    for job in self.session.step(1):
                        it, toks, tmp = jobs.pop(id(job))
                        mel = job.x[:, tmp:].contiguous()
                        wav = self.eng.hift.forward(mel, it["render"][4], it["render"][5])
                        it["rfut"].set_result((toks, mel, wav))
                    mark = torch.cuda.Event()
                    mark.record(self.stream)
                    ahead.append(mark)
                    if len(ahead) > self.AHEAD:
                        ahead.popleft().synchronize()
        except BaseException as e:      # noqa: BLE001  (handed to whoever waits for a batch this worker holds; later submits raise)
            with self._cv:
                self._dead = e
                held = [w for w in self._waiting] + [j[0] for j in jobs.values()] + ([item] if item is not None else [])
                self._waiting.clear()
            for it in held:
                if not it["rfut"].done():
                    it["rfut"].set_exception(e)


class PipelinedSynth:
    """Software pipeline over consecutive (independent) batches on several HIP streams of one GPU.

    The LM decode is a chain of ~19k small dependent launches (latency-bound: it leaves most CUs idle), the
    flow + vocoder stage is throughput-bound.  ``lm_depth`` decode chains run concurrently on their own high-priority
    streams, each enqueued by its own host thread (the decode loop is C++: ctypes drops the GIL), while the render
    stage of an earlier batch runs on a further stream; an event hands each batch's tokens over.
    ``submit`` enqueues batch i and returns the (toks, mel, wav) of the batch whose render stage it enqueued
    (None while the pipeline fills); ``drain`` enqueues what is left and returns those results.  Nothing here
    synchronises the host with the GPU.

    ``cobatch`` > 1: the LM stages of that many consecutive compatible batches (same prefix / decode lengths, <= 32 rows
    together) run as ONE decode chain with their rows side by side -- the chain's ~19k launches are latency-bound and cost
    about the same for 16 rows as for 8 -- and each batch is then rendered on its own.  Rows are independent in every LM
    kernel (GEMM rows, per-(row, head) attention, per-row sampler with per-row uniforms), so every batch's tokens, mel and
    waveform are bit-identical to running it alone (tested).

    ``join``: each of the ``lm_depth`` chains is a decode SESSION (LmSession) with two slots and a host thread of its own.  A submitted
    batch joins a chain that is already decoding -- its launches then carry the rows of both batches -- or starts an idle one; no batch
    waits for a partner.  Only when all ``2 * lm_depth`` slots are taken does ``submit`` render the oldest batch first, as it does
    without ``join`` when every chain is busy.  Same bits as running each batch alone (tested).  Batches a session cannot take (more
    than 8 rows, the wide engine, windows past the position tables) get a chain call of their own as without ``join``; batches
    need not have equal prefix or decode lengths.
    Footprint: every chain keeps a daemon host thread and its session's cache arena -- layers * 2 * window * 16 rows * 4 d bytes,
    0.94 GB per chain at CosyVoice-300M widths and windows of up to 512 keys, 2.8 GB at three chains -- until ``close()`` is called
    (``autotune`` closes the pipelines it does not return; the one it returns is the caller's to close).  A chain whose arena is too
    short for a batch is given a longer one when it holds no batch.

    ``render_join`` (with one render stream): the render stage is a flow SESSION (FlowSession) driven by a host thread of its own
    (_JoinRender).  A batch whose tokens are ready joins the Euler solve that is running -- the launches of an estimator pass then
    carry the sequences of up to four batches, each at its own step -- instead of queueing behind it; same bits as rendering each
    batch alone (tested).  ``submit`` then returns a batch once the worker is through with it, which may be later than without
    ``render_join`` (more ``None`` returns, more results from ``drain``); every batch is still returned exactly once.  Footprint: one
    more daemon thread and the session's workspace (that of a 64-sequence solve) until ``close()``."""

    JOIN_QUANTUM = 16        # token steps a chain's thread enqueues between two looks at its queue of batches that want to join
    JOIN_AHEAD = 2           # ... and the ranges it keeps enqueued ahead of the GPU: a batch can only join what is not enqueued yet
    # whether ``autotune`` also tries the joined render (``render_join``) beside the joining chains; ASTTS_PIPE_RENDER_JOIN=0 / 1 overrides
    AUTOTUNE_RENDER_JOIN = os.environ.get("ASTTS_PIPE_RENDER_JOIN", "1") != "0"

    def __init__(self, engine, lm_depth: int = 2, lm_priority: int = -1, render_priority: int = 0, streams=None,
                 cobatch: int = 1, render_depth: int = 1, pipe_classes=None, front_prefill: Optional[bool] = None,
                 stagger_ms: Optional[float] = None, wide_lm: bool = False, join: bool = False, render_join: bool = False):
        self.eng = engine
        self.depth = max(1, int(lm_depth))
        # ``render_depth`` > 1: the flow + vocoder stages of consecutive batches alternate between that many streams.  One
        # render chain is ~6000 dependent launches of ~10 us that each fill the chip for a few microseconds and leave it
        # to latency (tails, boundaries) in between; a second chain runs in those gaps.
        self.render_depth = rd = max(1, int(render_depth))
        dev = engine.device
        with torch.cuda.device(dev):
            self.front_stream = None
            extra_render = []
            if streams is not None:
                self.s_lm, self.s_render = list(streams[:self.depth]), streams[self.depth]
                extra_render = list(streams[self.depth + 1:self.depth + rd])
            elif lm_priority != render_priority:
                self.s_lm = [torch.cuda.Stream(device=dev, priority=lm_priority) for _ in range(self.depth)]
                self.s_render = torch.cuda.Stream(device=dev, priority=render_priority)
            elif rd > 1:
                st = ops.concurrent_streams(self.depth + 1 + rd, priority=lm_priority, device=dev)
                self.s_render, extra_render, self.front_stream, self.s_lm = st[0], st[1:rd], st[rd], st[rd + 1:]
            else:
                # one stream per command-processor pipe as far as they go (plan_streams); run the caller's own per-batch work
                # (retrieval, input preparation) and `submit` under `torch.cuda.stream(pipe.front_stream)`
                classes = pipe_classes if pipe_classes is not None else ops.stream_pipe_classes(priority=lm_priority, device=dev)
                render, lm, front = plan_streams([len(c) for c in classes], self.depth)
                self.s_render = classes[render[0]][render[1]]
                self.s_lm = [torch.cuda.Stream(device=dev, priority=lm_priority) if s is None else classes[s[0]][s[1]] for s in lm]
                self.front_stream = None if front is None else classes[front[0]][front[1]]
            if self.front_stream is None:
                self.front_stream = torch.cuda.Stream(device=dev)
            while len(extra_render) < rd - 1:
                extra_render.append(torch.cuda.Stream(device=dev, priority=render_priority))
            self.s_renders = [self.s_render] + list(extra_render)
            self._r = 0
        self._pool = ThreadPoolExecutor(max_workers=self.depth)
        self._fifo = deque()
        self._pending = []                  # batches waiting for their (co-batched) LM stage to be launched
        self.cobatch = max(1, int(cobatch))
        # ``wide_lm`` (throughput runs): LM stages of more than 32 rows decode as ONE chain on the engine's wide path (plain GEMMs, the
        # weights read once per token for all rows) instead of 32-row groups; see AcousticLM.decode
        self.wide_lm = bool(wide_lm)
        self.lm_rows_max = AcousticLM.WIDE_ROWS if self.wide_lm else 32
        self.front_prefill = (os.environ.get("ASTTS_PIPE_FRONT_PREFILL", "1") != "0") if front_prefill is None else bool(front_prefill)
        self.stagger_ms = float(os.environ.get("ASTTS_PIPE_STAGGER_MS", "0")) if stagger_ms is None else float(stagger_ms)
        self._staggered = set()
        self._i = 0
        self.join = bool(join) and self.cobatch == 1 and not self.wide_lm
        lm_ = engine.lm
        self._chains = [_JoinChain(lm_, dev, self.s_lm[c], c, self.JOIN_QUANTUM, self.JOIN_AHEAD, lm_.body.center)
                        for c in range(self.depth)] if self.join else []
        # ``render_join``: the render stage is a flow SESSION driven by a thread of its own (_JoinRender): batches whose tokens are ready
        # join the Euler solve that is running instead of queueing behind it
        self.render_join = bool(render_join) and rd == 1
        self._renderer = _JoinRender(engine, self.s_render) if self.render_join else None

    def close(self) -> None:
        """Stop the chains' threads and free their sessions (``join``); the pipeline must be drained."""
        for ch in self._chains:
            ch.close()
        self._chains = []
        if self._renderer is not None:
            self._renderer.close()
        self._pool.shutdown(wait=True)

    @classmethod
    def autotune(cls, engine, sample_args, depths=(3, 2), trials: int = 3, steps: int = 4, verbose: bool = False,
                 front=None, dist=None, wide_lm: bool = False):
        """Build the pipeline by measurement.  How well the chains overlap depends on which hardware queues HIP hands the
        streams (it multiplexes streams onto a few queues in an order the caller cannot see; a chain that shares a queue
        with another busy stream, or with the stream the caller enqueues its own work on, stalls the hand-over events).
        Each trial draws a fresh set of mutually concurrent streams (ops.concurrent_streams), runs ``steps`` batches of
        ``sample_args`` (the positional arguments of ``submit``) and the fastest configuration is kept.  ``front``: the
        caller's own per-batch GPU work (a callable, e.g. the style retrieval), enqueued on ``pipe.front_stream`` before
        each submit exactly as the caller will.  ``dist`` (an initialised torch.distributed module): every rank runs the same
        trials and ALL ranks keep the configuration whose slowest rank is fastest (one all-reduce MAX of the per-configuration
        times) -- ranks that picked different chain counts would straggle at the per-step all-gather of the style ids."""
        best, best_dt = None, float("inf")
        per_cfg = []                        # (best pipe, best time) per configuration, in the order of `depths`
        with torch.cuda.device(engine.device):
            classes = ops.stream_pipe_classes(device=engine.device, verbose=verbose)      # one probe for all trials
        # every depth both ways: separate chains, and chains that a second batch joins (``join``)
        tried = []
        for cfg_ in depths:
            cfg_ = cfg_ if isinstance(cfg_, tuple) else (cfg_, 1)
            for join in (False, True):
                if join and (cfg_[1] != 1 or wide_lm):
                    continue
                tried.append(tuple(cfg_) + ("join",) if join else cfg_)
                # ... and the joining chains with the joined render (one render stream: the session is that stream's)
                if join and cls.AUTOTUNE_RENDER_JOIN and len(cfg_) < 3:
                    tried.append(tuple(cfg_) + ("join", "render_join"))
        for cfg_ in tried:
            join, rjoin = "join" in cfg_, "render_join" in cfg_
            depth, cob, rdep = (tuple(c for c in cfg_ if not isinstance(c, str)) + (1,))[:3]
            for _ in range(trials):
                lm_prio = int(os.environ.get("ASTTS_PIPE_LM_PRIORITY", "0"))      # experiments: -1 = high-priority decode streams
                pipe = cls(engine, lm_depth=depth, lm_priority=lm_prio, render_priority=0, cobatch=cob, render_depth=rdep,
                           pipe_classes=classes if rdep == 1 and lm_prio == 0 else None, wide_lm=wide_lm, join=join, render_join=rjoin)
                with torch.cuda.stream(pipe.front_stream):
                    for _ in range((depth + 1) * cob):
                        if front is not None:
                            front()
                        pipe.submit(*sample_args)
                    pipe.drain()
                    torch.cuda.synchronize(engine.device)
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        if front is not None:
                            front()
                        pipe.submit(*sample_args)
                    pipe.drain()
                    torch.cuda.synchronize(engine.device)
                dt = (time.perf_counter() - t0) / steps
                if verbose:
                    print(f"PipelinedSynth.autotune: depth {depth} cobatch {cob} render streams {rdep} join {join} render join {rjoin}: {dt * 1e3:.1f} ms/batch", flush=True)
                if dt < best_dt:
                    best, best_dt = pipe, dt
                if not per_cfg or per_cfg[-1][2] != cfg_:
                    per_cfg.append([pipe, dt, cfg_])
                elif dt < per_cfg[-1][1]:
                    if per_cfg[-1][0] is not best:
                        per_cfg[-1][0].close()
                    per_cfg[-1][0], per_cfg[-1][1] = pipe, dt
                else:
                    pipe.close()
        if dist is not None and len(per_cfg) > 1:
            t = torch.tensor([c[1] for c in per_cfg], dtype=torch.float64, device=engine.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            k = int(torch.argmin(t).item())
            best, best_dt = per_cfg[k][0], per_cfg[k][1]
            best.tuned_agreed_over_ranks = True
        for c in per_cfg:                   # the chains' threads and sessions of every configuration that lost
            if c[0] is not best:
                c[0].close()
        best.tuned_ms_per_batch = best_dt * 1e3
        best.tuned_table_ms = {str(c[2]): round(c[1] * 1e3, 2) for c in per_cfg}
        return best

    # ---- stages
    def _launch_group(self):
        """Start the LM stage of the pending batches as ONE decode chain (rows of all of them side by side)."""
        group, self._pending = self._pending, []
        chain = self._i % self.depth
        stream = self.s_lm[chain]
        self._i += 1
        cur = torch.cuda.current_stream(self.eng.device)
        # ``stagger_ms``: after an idle pipeline (construction, drain) chain c starts its first decode c * stagger_ms late (a one-wave
        # busy-wait kernel at the head of its stream).  Chains that start together stay in phase: their batches finish together, the
        # render stage gets them in bursts and the drain ends with `depth` renders in a row; offset by a third of a chain's period they
        # hand the render stage one batch at a time and the drain ends with ONE render.
        if self.stagger_ms > 0 and chain > 0 and chain not in self._staggered:
            self._staggered.add(chain)
            us = int(self.stagger_ms * 1000.0 * chain)
            while us > 0:
                _lib_check_spin(min(us, 100000), stream)
                us -= 100000
        lm_args = group[0]["lm"] if len(group) == 1 else LmArgs.concat([g["lm"] for g in group])
        # every input -- the caller's own tensors too -- was allocated on the caller's stream and is read on the chain's for
        # the whole decode (~100 ms behind the host): tell the caching allocator, or a caller that builds fresh inputs per
        # batch gets these blocks recycled under the running chain
        record_streams(lm_args, stream)
        sizes = [g["lm"].rows for g in group]
        # ``front_prefill`` (default; ASTTS_PIPE_FRONT_PREFILL=0 or front_prefill=False: the whole LM stage on the chain): prefix
        # assembly + prefill (text encoder, 14 layers over the prefix, first logits: ~4.7 ms of a chain's ~106 ms per batch, big-tile
        # GEMM launches) are enqueued HERE, on the caller's stream, and the chain is its decode steps only.  The chains are what
        # bounds the pipelined step: 95.5 -> 93.9 ms per batch (scripts/front_prefill_probe.py, alternating in one process, 4 of 4)
        state = None
        if self.front_prefill and sum(sizes) <= self.lm_rows_max:
            state = self.eng.tts_prefill(*lm_args[:5])
            record_streams(state.tensors(), stream)
        stream.wait_stream(cur)             # after the concatenations (and the prefill) above were enqueued

        def lm_stage():
            with torch.cuda.device(self.eng.device), torch.cuda.stream(stream):
                toks = self.eng.tts_tokens(*lm_args, wide=self.wide_lm) if state is None else self.eng.tts_decode(state, lm_args.uniforms)
                parts = list(torch.split(toks, sizes, 0)) if len(sizes) > 1 else [toks]
                ev = torch.cuda.Event()
                ev.record(stream)
            return parts, ev

        fut = self._pool.submit(lm_stage)
        for k, g in enumerate(group):
            g["fut"], g["k"] = fut, k
            self._to_renderer(g)

    def _to_renderer(self, item) -> None:
        """``render_join``: the batch's LM stage is launched -- the render worker takes it from here."""
        if self._renderer is not None:
            self._renderer.submit(item, item["ready"])

    def _render(self, item):
        if self._renderer is not None:      # enqueued by the render worker: wait (on the host) until it has enqueued this batch's vocoder
            out = item["rfut"].result()
            record_streams(out, torch.cuda.current_stream(self.eng.device))
            return out
        parts, ev = item["fut"].result()
        toks = parts[item["k"]]
        cur = torch.cuda.current_stream(self.eng.device)
        sr = self.s_renders[self._r % self.render_depth]
        self._r += 1
        with torch.cuda.stream(sr):
            sr.wait_event(ev)
            toks.record_stream(sr)
            record_streams(item["render"], sr)      # the caller's tensors, read on the render stream (see _launch_group)
            mel, wav = self.eng.tts_render(toks, *item["render"])
        # results are produced on the pipeline's streams and handed to the caller's: the caller still has to order its
        # stream behind them (drain() does; a caller that consumes results earlier waits on `pipe.s_render` itself), but
        # the allocator must not recycle them while the caller's stream may be using them
        record_streams((toks, mel, wav), cur)
        return toks, mel, wav

    def submit(self, text, text_lens, lm_spk, lm_prompt_tokens, n_tokens, uniforms, flow_prompt_tokens, flow_prompt_mel,
               flow_spk, z, phase0, noise):
        cur = torch.cuda.current_stream(self.eng.device)
        item = {"lm": LmArgs(text, text_lens, lm_spk, lm_prompt_tokens, n_tokens, uniforms),
                "render": (flow_prompt_tokens, flow_prompt_mel, flow_spk, z, phase0, noise), "fut": None, "k": 0}
        if self._renderer is None:
            for sr in self.s_renders:
                sr.wait_stream(cur)
        else:       # the worker enqueues on the render stream from its own thread: it orders the stream behind this event itself
            item["ready"] = torch.cuda.Event()
            item["ready"].record(cur)
        if self.join and self._join_submit(item):
            if self._renderer is not None:
                # the render worker takes batches as their tokens become ready: submit hands over the oldest batch only once the worker
                # is through with it, and waits for it only when more batches are in flight than chains and session hold together
                rfut = self._fifo[0].get("rfut")
                done = rfut is not None and (rfut.done() or len(self._fifo) > 2 * self.depth + _JoinRender.SLOTS)
                return self._render(self._fifo.popleft()) if done else None
            return self._render(self._fifo.popleft()) if len(self._fifo) > 2 * self.depth else None
        if self._pending and not self._compatible(self._pending[0]["lm"], item["lm"]):
            self._launch_group()
        self._pending.append(item)
        self._fifo.append(item)
        if len(self._pending) >= self.cobatch:
            self._launch_group()
        # keep `depth` decode chains in flight behind the batch being rendered
        if len(self._fifo) > self.depth * self.cobatch and self._fifo[0]["fut"] is not None:
            return self._render(self._fifo.popleft())
        return None

    def _join_submit(self, item) -> bool:
        """``join``: prefix and prefill on the caller's stream, then the batch goes to a chain that can hold it -- one that is already
        decoding if there is one (that is the join), else an idle one.  While no chain can (every slot taken, or a window longer than
        the arenas of the chains that are busy) the batches before it are waited for, oldest first: a chain hands a batch over when its
        last step is enqueued, and a chain without batches takes any window the position tables allow.
        -> False: not a batch a session takes (nothing is enqueued then)."""
        lm, lm_args = self.eng.lm, item["lm"]
        if lm_args.rows > _JoinChain.ROWS_MAX // 2:
            return False
        pre = lm.prefix(lm_args.text, lm_args.text_lens, lm_args.lm_spk, lm_args.lm_prompt_tokens)
        window = int(pre.shape[0]) + int(lm_args.n_tokens) - 1
        if window > lm.body.center:
            return False
        state = lm.prefill(pre, lm_args.n_tokens)
        order = lambda: sorted(self._chains, key=lambda ch: (ch.occupied() != 1, ch.index))     # noqa: E731
        chain = next((ch for ch in order() if ch.reserve(window)), None)
        for older in list(self._fifo):
            if chain is not None:
                break
            if older["fut"] is not None:
                try:
                    older["fut"].result()
                except Exception:      # noqa: BLE001  (raised again where that batch is rendered)
                    pass
                chain = next((ch for ch in order() if ch.reserve(window)), None)
        if chain is None:
            raise RuntimeError("PipelinedSynth: no decode chain can take the batch although none holds one")
        self._fifo.append(item)
        item["fut"] = chain.submit(state, lm_args)
        self._to_renderer(item)
        return True

    def _compatible(self, a: LmArgs, b: LmArgs) -> bool:
        """Batches can share a decode chain when their prefix and decode lengths agree (fixed-length batches of one job)."""
        return (a.n_tokens == b.n_tokens and a.text.shape[1] == b.text.shape[1]
                and a.lm_prompt_tokens.shape[1] == b.lm_prompt_tokens.shape[1] and a.uniforms.shape[0] == b.uniforms.shape[0]
                and a.rows + b.rows <= self.lm_rows_max)

    def drain(self):
        if self._pending:
            self._launch_group()
        self._staggered = set()          # the pipeline runs empty: the next first batches are staggered again
        self._i = 0
        out = []
        while self._fifo:
            out.append(self._render(self._fifo.popleft()))
        cur = torch.cuda.current_stream(self.eng.device)
        for st in self.s_lm:
            cur.wait_stream(st)
        for sr in self.s_renders:
            cur.wait_stream(sr)
        return out
