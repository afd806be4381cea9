"""LoRA fine-tuning of the Llama decoder on the GPU: what the reference's src/ft_llm.py does with peft + trl + bitsandbytes
(LoRA r = 32, alpha = 128 on all seven projections, AdamW, max_grad_norm 0.3, constant or linear learning rate with 3 % warm-up, LoRA
dropout and NEFTune noise from a counter-based generator), on this project's HIP kernels.  DESIGN.md section 2 "Fine-tuning" has the path, the numerics, the memory kept per token and what is not built.

Forward: LlamaDecoder's layer on batch-major right-padded rows, with the LoRA branch unmerged on the frozen fp16 base
(``y = W x + (scaling B)(A x)``: two more GEMMs per fused projection, A stacked and B block-diagonal over the projections that share
an input).  Backward: dX of every frozen projection is ``ops.linear`` on the transposed weight packed once at load; attention, the
norms, SwiGLU, the softmax gradient, the LoRA weight gradients and the optimizer are csrc/train/*.hip (astts.train_ops); RoPE's
transpose is the RoPE kernel with a negated sine table.  fp16 where a tensor is an MFMA operand, fp32 for the residual stream, its
gradient, the LoRA masters, their gradients and the Adam moments; a static power-of-two loss scale keeps the fp16 gradients in
range.  No atomics: a step is bit-for-bit repeatable.  A Qwen2 base (``cfg.qkv_bias``): the q | k | v bias is frozen; the forward picks
it up with the decoder's packs (the base GEMM's epilogue), the transposed packs of the backward carry none, so dX, dA and dB do not see it.

Regularisers (``lora_dropout``, ``neftune_alpha``; both 0 = the path above, bit for bit).  peft gives every LoRA module its own
dropout on its input, so q, k and v mask the same ``h1`` independently; the masks are never stored: each is a function of
(``noise_seed``, layer * 8 + position in PROJ, the forward's ``draw``) that ``lora_down`` regenerates in its operand load,
``lora_grad_dropout`` (dA) in its operand load and ``lora_dx_dropout`` in its epilogue.  dB needs nothing: ``t`` carries the mask.
NEFTune adds ``alpha / sqrt(T * hidden) * U(-1, 1)`` to the embedding output of a training forward.

Evaluation while training: ``eval_model()`` is a LlamaEmbedder on the CURRENT adapter -- ``train_ops.lora_merge`` writes
``fp16(W + scaling B A)`` from the fp32 masters into a second image of every fused projection, on the device.  ``save_state`` /
``load_state`` carry the masters, Adam's moments, the counters and the recipe; a resumed run equals an uninterrupted one bit for bit.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .config import LlamaShape
from .peft import PROJ, LoraAdapter

# the fused projections of LlamaDecoder's layer and the peft modules each is made of
GROUPS = (("wqkv", ("q_proj", "k_proj", "v_proj")), ("wo", ("o_proj",)), ("wgu", ("gate_proj", "up_proj")), ("wd", ("down_proj",)))
MAX_GRAD_NORM = 0.3
WARMUP_RATIO = 0.03


def proj_shapes(cfg: LlamaShape) -> Dict[str, Tuple[int, int]]:
    """peft module -> (out features, in features)."""
    hq, hk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    return {"q_proj": (hq, cfg.hidden), "k_proj": (hk, cfg.hidden), "v_proj": (hk, cfg.hidden), "o_proj": (cfg.hidden, hq),
            "gate_proj": (cfg.ffn, cfg.hidden), "up_proj": (cfg.ffn, cfg.hidden), "down_proj": (cfg.hidden, cfg.ffn)}


def init_lora(cfg: LlamaShape, r: int, lora_alpha: float, seed: int = 42, base_model_name_or_path: str = "") -> LoraAdapter:
    """peft's initial adapter: B = 0, A = kaiming_uniform(a = sqrt(5)), i.e. U(-1 / sqrt(in), 1 / sqrt(in)), drawn layer by layer in
    PROJ's order from ``torch.Generator().manual_seed(seed)`` on the CPU."""
    g = torch.Generator().manual_seed(seed)
    ad = LoraAdapter(r=r, lora_alpha=float(lora_alpha), use_rslora=False, targets=tuple(PROJ), base_model_name_or_path=base_model_name_or_path)
    shapes = proj_shapes(cfg)
    for i in range(cfg.layers):
        for p in PROJ:
            out_f, in_f = shapes[p]
            bound = 1.0 / math.sqrt(in_f)
            ad.pairs[(i, p)] = ((torch.rand(r, in_f, generator=g) * 2.0 - 1.0) * bound, torch.zeros(out_f, r))
    return ad


def save_adapter(adapter: LoraAdapter, path: str, lora_dropout: float = 0.0) -> None:
    """adapter_config.json + adapter_model.safetensors as peft's save_pretrained writes them (astts.llm.peft.load_adapter reads them)."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    conf = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "base_model_name_or_path": adapter.base_model_name_or_path, "r": adapter.r,
            "lora_alpha": adapter.lora_alpha, "lora_dropout": float(lora_dropout), "bias": "none", "target_modules": list(adapter.targets),
            "use_rslora": adapter.use_rslora, "use_dora": False, "fan_in_fan_out": False, "modules_to_save": None, "inference_mode": True,
            "init_lora_weights": True}
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(conf, f, indent=2, sort_keys=True)
    sd = {}
    for (i, p), (a, b) in sorted(adapter.pairs.items()):
        sd[f"base_model.model.model.layers.{i}.{PROJ[p]}.lora_A.weight"] = a.detach().to("cpu", torch.float32).contiguous()
        sd[f"base_model.model.model.layers.{i}.{PROJ[p]}.lora_B.weight"] = b.detach().to("cpu", torch.float32).contiguous()
    save_file(sd, os.path.join(path, "adapter_model.safetensors"), metadata={"format": "pt"})


def warmup_steps(total_steps: int, ratio: float = WARMUP_RATIO) -> int:
    """transformers' TrainingArguments.get_warmup_steps: ceil(total * ratio)."""
    return int(math.ceil(total_steps * ratio))


SCHEDULES = ("constant", "linear")


def lr_at(step: int, base_lr: float, total_steps: int, ratio: float = WARMUP_RATIO, schedule: str = "constant") -> float:
    """Learning rate of optimizer step ``step`` (0-based).  ``"constant"``: transformers' constant schedule with warm-up,
    ``base_lr * min(1, step / max(1, warmup))`` -- with a warm-up, the very first step runs at 0, as there.  ``"linear"``: its
    get_linear_schedule_with_warmup, the same warm-up and then ``max(0, (total - step) / max(1, total - warmup))``."""
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule {schedule!r}: one of {SCHEDULES}")
    w = warmup_steps(total_steps, ratio)
    if step < w:
        return base_lr * step / max(1, w)
    if schedule == "linear":
        return base_lr * max(0.0, (total_steps - step) / max(1, total_steps - w))
    return base_lr


def next_token_targets(ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """ids ``[B, T]`` right-padded, lens ``[B]`` -> int32 ``[B, T]``: the token at position i + 1 while that is a real token, else -1
    (transformers' shifted labels with the padding ignored)."""
    b, t = ids.shape
    nxt = torch.cat([ids[:, 1:], ids.new_zeros(b, 1)], 1)
    pos = torch.arange(t, device=ids.device)[None, :]
    return torch.where(pos + 1 < lens.to(ids.device)[:, None].long(), nxt, nxt.new_full((), -1)).to(torch.int32)


def clip_multiplier(grad_norm: float, max_norm: float = MAX_GRAD_NORM) -> float:
    """torch.nn.utils.clip_grad_norm_'s factor: min(1, max_norm / (norm + 1e-6))."""
    return min(1.0, max_norm / (grad_norm + 1e-6))


@dataclass
class StepReport:
    step: int
    loss: float
    grad_norm: float
    lr: float
    loss_scale: float
    skipped: bool


class _Group:
    """One fused projection's LoRA: masters (views into the trainer's flat buffers) and the packed fp16 operands made from them."""
    __slots__ = ("name", "parts", "outs", "cin", "a", "ga", "b", "gb", "a_pack", "b_pack", "at_pack", "bt_pack", "bblk", "stream", "bcat")


class LoraTrainer:
    def __init__(self, state: dict, cfg: LlamaShape, device=None, r: int = 32, lora_alpha: float = 128.0, seed: int = 42,
                 adapter: Optional[LoraAdapter] = None, lr: float = 2e-4, total_steps: int = 1, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: float = MAX_GRAD_NORM, warmup_ratio: float = WARMUP_RATIO,
                 loss_scale: float = 1024.0, head_chunk: int = 1024, base_model_name_or_path: str = "", rope_len: int = 576,
                 lora_dropout: float = 0.0, neftune_alpha: float = 0.0, noise_seed: Optional[int] = None, schedule: str = "constant"):
        from .. import ops, train_ops
        from .decoder import LlamaDecoder

        assert loss_scale > 0 and math.log2(loss_scale).is_integer(), "the loss scale is a power of two"
        assert 0.0 <= lora_dropout < 1.0 and neftune_alpha >= 0.0 and schedule in SCHEDULES, (lora_dropout, neftune_alpha, schedule)
        self.ops, self.tops = ops, train_ops
        self.cfg = cfg
        self.dec = LlamaDecoder(state, cfg, device, rope_len=rope_len)
        self.device = dev = self.dec.device
        self.adapter0 = adapter if adapter is not None else init_lora(cfg, r, lora_alpha, seed, base_model_name_or_path)
        self.r, self.lora_alpha, self.scaling = self.adapter0.r, self.adapter0.lora_alpha, self.adapter0.scaling
        self.base_name = self.adapter0.base_model_name_or_path or base_model_name_or_path
        self.lr, self.total_steps, self.betas, self.eps, self.weight_decay = lr, total_steps, betas, eps, weight_decay
        self.max_grad_norm, self.warmup_ratio, self.loss_scale, self.head_chunk = max_grad_norm, warmup_ratio, float(loss_scale), int(head_chunk)
        self.lora_dropout, self.neftune_alpha, self.schedule = float(lora_dropout), float(neftune_alpha), schedule
        self.noise_seed = int(seed if noise_seed is None else noise_seed)
        self.draw = 0               # training forwards run so far: the generator's draw of the next one
        self.opt_step = 0           # optimizer steps taken (skipped ones do not count)
        self.sched_step = 0         # scheduler position: every call of step()
        shapes = proj_shapes(cfg)
        rr = self.r
        n = sum(rr * (shapes[p][0] + shapes[p][1]) for p in PROJ) * cfg.layers
        with torch.cuda.device(dev):
            self.params = torch.zeros(n, dtype=torch.float32, device=dev)
            self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
            self.m = torch.zeros(n, dtype=torch.float32, device=dev)
            self.v = torch.zeros(n, dtype=torch.float32, device=dev)
            self.G: List[Dict[str, _Group]] = []
            # the frozen weights transposed, for dX = dY W: packed once
            self.WT: List[Dict[str, object]] = []
            off = 0
            for i in range(cfg.layers):
                gl, wt = {}, {}
                for name, parts in GROUPS:
                    g = _Group()
                    g.name, g.parts = name, parts
                    g.outs = [shapes[p][0] for p in parts]
                    g.cin = shapes[parts[0]][1]
                    g.stream = i * 8 + list(PROJ).index(parts[0])                 # part j draws from stream + j
                    R, nout = rr * len(parts), sum(g.outs)
                    g.a = self.params[off:off + R * g.cin].view(R, g.cin)
                    g.ga = self.grads[off:off + R * g.cin].view(R, g.cin)
                    off += R * g.cin
                    g.b, g.gb, b0 = [], [], off
                    for j, p in enumerate(parts):
                        g.a[j * rr:(j + 1) * rr].copy_(self.adapter0.pairs[(i, p)][0])
                        g.b.append(self.params[off:off + g.outs[j] * rr].view(g.outs[j], rr))
                        g.gb.append(self.grads[off:off + g.outs[j] * rr].view(g.outs[j], rr))
                        g.b[-1].copy_(self.adapter0.pairs[(i, p)][1])
                        off += g.outs[j] * rr
                    g.bcat = self.params[b0:off].view(nout, rr)                        # the parts' B back to back: one [out, r] master
                    g.bblk = torch.zeros(nout, R, dtype=torch.float32, device=dev)
                    g.a_pack = ops.PackedWeight(g.a, None, dev)                       # [R, in]:    t = x A^T
                    g.b_pack = ops.PackedWeight(g.bblk, None, dev)                    # [out, R]:   y += t (scaling B)^T
                    g.at_pack = ops.PackedWeight(g.a.t().contiguous(), None, dev)     # [in, R]:    dx += dt A
                    g.bt_pack = ops.PackedWeight(g.bblk.t().contiguous(), None, dev)  # [R, out]:   dt = dy (scaling B)
                    gl[name] = g
                    w = torch.cat([state[f"model.layers.{i}.{PROJ[p]}.weight"] for p in parts], 0)
                    wt[name] = ops.PackedWeight(w.to(dev).t().contiguous(), None, dev)
                self.G.append(gl)
                self.WT.append(wt)
            assert off == n
            head = state["model.embed_tokens.weight"] if cfg.tie_embeddings else state["lm_head.weight"]
            self.headT = ops.PackedWeight(head.to(dev).t().contiguous(), None, dev)
            self.nsq = torch.zeros(1, dtype=torch.float32, device=dev)
            self._eval = None           # eval_model()'s embedder: built on first use
            self.repack()

    # ------------------------------------------------------------------------------------------------ parameters
    def _pack_into(self, pw, src: torch.Tensor) -> None:
        """astts_op_pack_weight of fp32 ``src`` [n, cin] into the existing image of ``pw`` (a device kernel; the padding stays zero)."""
        from .. import _lib
        src = src.contiguous()
        assert src.shape == (pw.n, pw.cin) and src.dtype == torch.float32
        _lib.check(_lib.load().astts_op_pack_weight(src.data_ptr(), pw.data.data_ptr(), pw.n, 1, pw.cin, pw.n_pad, pw.cin_pad, _lib.stream_ptr()))

    def repack(self) -> None:
        """The fp16 GEMM operands of every LoRA pair from the fp32 masters: after load and after every optimizer step."""
        rr = self.r
        for gl in self.G:
            for g in gl.values():
                o = 0
                for j, b in enumerate(g.b):                      # block-diagonal scaling * B: projection j's rank columns feed its rows only
                    torch.mul(b, self.scaling, out=g.bblk[o:o + g.outs[j], j * rr:(j + 1) * rr])
                    o += g.outs[j]
                self._pack_into(g.a_pack, g.a)
                self._pack_into(g.b_pack, g.bblk)
                self._pack_into(g.at_pack, g.a.t())
                self._pack_into(g.bt_pack, g.bblk.t())

    def adapter(self) -> LoraAdapter:
        """The current masters as a LoraAdapter (CPU, fp32)."""
        ad = LoraAdapter(r=self.r, lora_alpha=self.lora_alpha, use_rslora=self.adapter0.use_rslora, targets=tuple(PROJ),
                         base_model_name_or_path=self.base_name)
        rr = self.r
        for i, gl in enumerate(self.G):
            for g in gl.values():
                for j, p in enumerate(g.parts):
                    ad.pairs[(i, p)] = (g.a[j * rr:(j + 1) * rr].detach().cpu().clone(), g.b[j].detach().cpu().clone())
        return ad

    def named_grads(self) -> Dict[Tuple[int, str, str], torch.Tensor]:
        """(layer, module, "A" | "B") -> the accumulated gradient (a view; it carries the loss scale)."""
        out, rr = {}, self.r
        for i, gl in enumerate(self.G):
            for g in gl.values():
                for j, p in enumerate(g.parts):
                    out[(i, p, "A")] = g.ga[j * rr:(j + 1) * rr]
                    out[(i, p, "B")] = g.gb[j]
        return out

    def save_adapter(self, path: str) -> None:
        save_adapter(self.adapter(), path, self.lora_dropout)

    def set_adapter(self, adapter: LoraAdapter) -> None:
        """The masters <- ``adapter``'s pairs (same r, every projection); the optimizer state stays.  Repacks."""
        rr = self.r
        if adapter.r != rr:
            raise ValueError(f"set_adapter: r {adapter.r} where the trainer has {rr}")
        for i, gl in enumerate(self.G):
            for g in gl.values():
                for j, p in enumerate(g.parts):
                    a, b = adapter.pairs[(i, p)]
                    g.a[j * rr:(j + 1) * rr].copy_(a)
                    g.b[j].copy_(b)
        self.repack()

    # ------------------------------------------------------------------------------------------------ evaluation while training
    def eval_model(self, tokenizer=None, max_length: int = 512):
        """A LlamaEmbedder that computes with the CURRENT adapter merged into the base: the inference path (generation, scoring) at
        plain fp16 speed.  Built on first use from ``self.dec`` -- it shares the embedding table, norms, head, biases and RoPE tables
        and owns a second fp16 image of the four fused projections per layer; EVERY call refreshes those images from the fp32 masters
        with ``train_ops.lora_merge`` (a device kernel; nothing goes through the host, the images are not reallocated).  The frozen
        base and the training state are not touched: no draw is taken."""
        from ..ops import PackedWeight
        from .embedder import LlamaEmbedder
        if self._eval is None:
            with torch.cuda.device(self.device):
                layers = [{k: (PackedWeight.zeros_like(v) if k in dict(GROUPS) else v) for k, v in L.items()} for L in self.dec.L]
                self._eval = LlamaEmbedder.adopt(self.dec, layers, rope_len=max(max_length, 16) + 64, tokenizer=tokenizer, max_length=max_length)
        emb = self._eval
        if tokenizer is not None:
            emb.tokenizer = tokenizer
        emb.max_length = max_length
        with torch.cuda.device(self.device):
            for L, E, gl in zip(self.dec.L, emb.L, self.G):
                for name, g in gl.items():
                    n = sum(g.outs)
                    g1 = g.outs[0]
                    g2 = n if len(g.outs) < 3 else g.outs[0] + g.outs[1]
                    self.tops.lora_merge(L[name], g.a, g.bcat, E[name], self.r, g1, g2, self.scaling)
        return emb

    # ------------------------------------------------------------------------------------------------ state: save / resume
    STATE_TENSORS, STATE_JSON = "trainer_state.safetensors", "trainer_recipe.json"

    def recipe(self) -> dict:
        """What a saved state belongs to: the adapter's and the optimizer's hyper-parameters, the schedule, the noise, the model shape."""
        import dataclasses
        return {"r": self.r, "lora_alpha": self.lora_alpha, "lr": self.lr, "schedule": self.schedule, "total_steps": self.total_steps,
                "warmup_ratio": self.warmup_ratio, "lora_dropout": self.lora_dropout, "neftune_alpha": self.neftune_alpha,
                "noise_seed": self.noise_seed, "betas": list(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm, "shape": json.loads(json.dumps(dataclasses.asdict(self.cfg)))}

    def save_state(self, path: str) -> None:
        """Everything the next step depends on besides the frozen base and the data: the fp32 masters, Adam's m and v (safetensors),
        and the counters ``draw``, ``opt_step``, ``sched_step``, ``loss_scale`` with ``recipe()`` (JSON).  No pickle."""
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        save_file({"params": self.params.detach().cpu(), "m": self.m.detach().cpu(), "v": self.v.detach().cpu()},
                  os.path.join(path, self.STATE_TENSORS), metadata={"format": "pt"})
        with open(os.path.join(path, self.STATE_JSON), "w") as f:
            json.dump({"recipe": self.recipe(), "draw": self.draw, "opt_step": self.opt_step, "sched_step": self.sched_step,
                       "loss_scale": self.loss_scale}, f, indent=2, sort_keys=True)

    def load_state(self, path: str) -> None:
        """``save_state``'s directory into this trainer.  A recipe that differs from this trainer's in any key is refused (ValueError
        naming the key): the continued run would not be the run that was saved.  Repacks the fp16 operands."""
        from safetensors.torch import load_file
        with open(os.path.join(path, self.STATE_JSON)) as f:
            st = json.load(f)
        mine, theirs = self.recipe(), st["recipe"]
        for k in sorted(set(mine) | set(theirs)):
            if k not in mine or k not in theirs or mine[k] != theirs[k]:
                raise ValueError(f"load_state: {path} was saved under another recipe: {k!r} is {theirs.get(k)!r} there and {mine.get(k)!r} here")
        t = load_file(os.path.join(path, self.STATE_TENSORS))
        for name, dst in (("params", self.params), ("m", self.m), ("v", self.v)):
            if t[name].shape != dst.shape or t[name].dtype != torch.float32:
                raise ValueError(f"load_state: {name} is {tuple(t[name].shape)} {t[name].dtype}, expected {tuple(dst.shape)} float32")
        for name, dst in (("params", self.params), ("m", self.m), ("v", self.v)):
            dst.copy_(t[name])
        self.draw, self.opt_step, self.sched_step = int(st["draw"]), int(st["opt_step"]), int(st["sched_step"])
        self.loss_scale = float(st["loss_scale"])
        self.repack()

    # ------------------------------------------------------------------------------------------------ forward / backward
    def _drop(self, g: _Group, draw: Optional[int]):
        """The dropout arguments of one fused projection in the forward numbered ``draw`` (None: evaluation, or dropout off)."""
        if draw is None or self.lora_dropout == 0.0:
            return None
        return dict(parts=len(g.parts), r=self.r, p=self.lora_dropout, seed=self.noise_seed, rng_stream=g.stream, draw=draw)

    def _fwd(self, x16: torch.Tensor, w, g: _Group, residual=None, out_dtype=torch.float32, draw: Optional[int] = None):
        """base GEMM in fp32 (+ residual), then the LoRA branch on top of it -> (y, t = x A^T fp16; under dropout each part of t sees
        x under its own mask)."""
        ops = self.ops
        base = ops.linear(x16, w, residual=residual)
        drop = self._drop(g, draw)
        t = ops.linear(x16, g.a_pack, out_dtype=torch.float16) if drop is None else self.tops.lora_down(x16, g.a_pack, **drop)
        return ops.linear(t, g.b_pack, residual=base, out_dtype=out_dtype), t

    def _bwd(self, dy: torch.Tensor, x16: torch.Tensor, t: torch.Tensor, wt, g: _Group, first: bool, out_dtype=torch.float32,
             draw: Optional[int] = None) -> torch.Tensor:
        """dy [rows, out] (fp16, or fp32: rounded where it becomes an operand) -> dx [rows, in]; adds this micro-batch's dA, dB.
        ``draw``: the forward's, whose masks dA and the LoRA part of dx regenerate."""
        ops, tops = self.ops, self.tops
        dt = ops.linear(dy, g.bt_pack, out_dtype=torch.float16)                     # [rows, R] = dy (scaling B)
        drop = self._drop(g, draw)
        if drop is None:
            dx = ops.linear(dt, g.at_pack, residual=ops.linear(dy, wt), out_dtype=out_dtype)
            tops.lora_grad(dt, x16, out=g.ga, accumulate=not first)                 # dA (all parts at once) = dt^T x
        else:
            dx = tops.lora_dx_dropout(dt, g.at_pack, ops.linear(dy, wt), out_dtype=out_dtype, **drop)
            tops.lora_grad_dropout(dt, x16, out=g.ga, accumulate=not first, **drop)  # dA_j = dt_j^T (mask_j o x) / (1 - p)
        o, rr = 0, self.r
        for j in range(len(g.parts)):                                               # dB_j = scaling dy_j^T t_j
            tops.lora_grad(dy[:, o:o + g.outs[j]], t[:, j * rr:(j + 1) * rr], out=g.gb[j], alpha=self.scaling, accumulate=not first)
            o += g.outs[j]
        return dx

    def forward(self, ids: torch.Tensor, lens: torch.Tensor, keep: bool = False, train: bool = False):
        """ids [B, T] right-padded, lens [B] -> (sum of next-token log-likelihoods over the real targets [1] fp32 on the device, number
        of targets, saved state for backward when ``keep``).  ``train``: dropout and NEFTune act, and the forward takes the next draw
        of the generator (kept with the state: backward regenerates its masks)."""
        ops, cfg, dec = self.ops, self.cfg, self.dec
        b, t = ids.shape
        ids = ids.to(self.device)
        lens32 = lens.to(self.device, torch.int32).contiguous()
        cos, sin = dec._rope_for(t)
        hq, hk, eps = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim, cfg.rms_eps
        rows = b * t
        x = ops.embedding(dec.embed, ids).view(rows, cfg.hidden)
        draw = None
        if train:
            draw, self.draw = self.draw, self.draw + 1
            if self.neftune_alpha > 0.0:                 # trl's neftune_post_forward_hook: padding positions get noise too
                self.tops.neftune_(x, self.neftune_alpha / math.sqrt(t * cfg.hidden), self.noise_seed, draw)
        saved = []
        for L, G in zip(dec.L, self.G):
            h1 = ops.rmsnorm(x, L["n1"], eps)
            qkv, t_qkv = self._fwd(h1, L["wqkv"], G["wqkv"], out_dtype=torch.float16, draw=draw)
            qkv3 = qkv.view(b, t, hq + 2 * hk)
            qk_pre = None
            if cfg.qk_norm:                                  # Qwen3: backward recomputes the norm from the q | k the op read
                qk_pre = qkv3[..., :hq + hk].contiguous() if keep else None
                ops.qknorm_rope_(qkv3, cos, sin, L["qn"], L["kn"], cfg.heads, cfg.kv_heads, cfg.head_dim, eps)
            else:
                ops.rope_llama_(qkv3, cos, sin, cfg.heads + cfg.kv_heads, cfg.head_dim)
            ao = ops.attn_gqa(qkv3[..., :hq], qkv3[..., hq:hq + hk], qkv3[..., hq + hk:], cfg.heads, cfg.kv_heads, cfg.head_dim, lens32).view(rows, hq)
            x1, t_o = self._fwd(ao, L["wo"], G["wo"], residual=x, draw=draw)
            h2 = ops.rmsnorm(x1, L["n2"], eps)
            gu, t_gu = self._fwd(h2, L["wgu"], G["wgu"], out_dtype=torch.float16, draw=draw)
            act = ops.swiglu(gu)
            x2, t_d = self._fwd(act, L["wd"], G["wd"], residual=x1, draw=draw)
            if keep:
                saved.append((x, h1, qkv3, t_qkv, ao, t_o, x1, h2, gu, t_gu, act, t_d, qk_pre))
            x = x2
        hf = ops.rmsnorm(x, dec.norm, eps)
        targets = next_token_targets(ids, lens32).reshape(rows).contiguous()
        lp, lse = ops.head_logprob(hf, dec.head, targets, want_lse=True, vocab=cfg.vocab)
        count = int((lens.clamp(min=1) - 1).sum())
        return lp.sum(dtype=torch.float32), count, ((saved, x, hf, targets, lse, lens32, b, t, draw) if keep else None)

    def backward(self, kept, denom: int, first: bool) -> None:
        """Accumulates d(loss_scale / denom * sum of token losses) / d(every A and B) into ``self.grads`` (``first``: overwrites)."""
        ops, tops, cfg, dec = self.ops, self.tops, self.cfg, self.dec
        saved, xf, hf, targets, lse, lens32, b, t, draw = kept
        rows, eps = b * t, cfg.rms_eps
        hq, hk = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
        cos, sin = dec._rope_for(t)
        nsin = -sin
        dh = torch.empty((rows, cfg.hidden), dtype=torch.float32, device=self.device)
        for r0 in range(0, rows, self.head_chunk):                       # the logits plane: head_chunk rows at a time
            r1 = min(rows, r0 + self.head_chunk)
            logits = ops.linear(hf[r0:r1], dec.head)
            tops.xent_grad_(logits, lse[r0:r1], targets[r0:r1], self.loss_scale / denom)
            ops.gemm(logits, self.headT, out=dh[r0:r1])
        dx = torch.zeros((rows, cfg.hidden), dtype=torch.float32, device=self.device)
        tops.rmsnorm_bwd_(dx, dh, xf, dec.norm, eps)
        for L, G, WT, s in zip(reversed(dec.L), reversed(self.G), reversed(self.WT), reversed(saved)):
            x0, h1, qkv3, t_qkv, ao, t_o, x1, h2, gu, t_gu, act, t_d, qk_pre = s
            dact = self._bwd(dx, act, t_d, WT["wd"], G["wd"], first, out_dtype=torch.float16, draw=draw)
            dgu = tops.swiglu_bwd(dact, gu)
            dh2 = self._bwd(dgu, h2, t_gu, WT["wgu"], G["wgu"], first, draw=draw)
            tops.rmsnorm_bwd_(dx, dh2, x1, L["n2"], eps)
            dao = self._bwd(dx, ao, t_o, WT["wo"], G["wo"], first, out_dtype=torch.float16, draw=draw)
            dqkv = tops.attn_gqa_bwd(qkv3, dao.view(b, t, hq), cfg.heads, cfg.kv_heads, cfg.head_dim, lens32)
            if cfg.qk_norm:                                                                   # rotation and norm transposed in one launch
                tops.qknorm_rope_bwd_(dqkv, qk_pre, cos, sin, L["qn"], L["kn"], cfg.heads, cfg.kv_heads, cfg.head_dim, eps)
            else:
                ops.rope_llama_(dqkv, cos, nsin, cfg.heads + cfg.kv_heads, cfg.head_dim)      # the rotation's transpose
            dh1 = self._bwd(dqkv.view(rows, hq + 2 * hk), h1, t_qkv, WT["wqkv"], G["wqkv"], first, draw=draw)
            tops.rmsnorm_bwd_(dx, dh1, x0, L["n1"], eps)

    def loss(self, ids: torch.Tensor, lens: torch.Tensor) -> float:
        """Mean next-token cross-entropy over the real targets at the current parameters (forward only)."""
        s, count, _ = self.forward(ids, lens)
        return -float(s) / max(count, 1)

    # ------------------------------------------------------------------------------------------------ optimizer
    def accumulate(self, batches: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> float:
        """Forward + backward of the micro-batches of one optimizer step -> the mean loss over ALL their targets (what transformers'
        Trainer optimises under gradient accumulation: the token count of the whole accumulated batch normalises every micro-batch)."""
        denom = max(1, sum(int((lens.clamp(min=1) - 1).sum()) for _, lens in batches))
        total = 0.0
        for j, (ids, lens) in enumerate(batches):
            s, _, kept = self.forward(ids, lens, keep=True, train=True)
            self.backward(kept, denom, first=j == 0)
            total += float(s)
        return -total / denom

    def step(self, batches: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> StepReport:
        """One optimizer step over ``batches`` (gradient accumulation).  A non-finite gradient norm skips the update and halves the scale."""
        loss = self.accumulate(batches)
        scale = self.loss_scale
        self.tops.sumsq(self.grads, out=self.nsq)
        norm = math.sqrt(float(self.nsq)) / scale if math.isfinite(float(self.nsq)) else float("nan")
        lr = lr_at(self.sched_step, self.lr, self.total_steps, self.warmup_ratio, self.schedule)
        self.sched_step += 1
        if not math.isfinite(norm):
            self.loss_scale = scale / 2.0
            return StepReport(self.sched_step, loss, float("nan"), lr, scale, True)
        self.opt_step += 1
        self.tops.adamw_(self.params, self.grads, self.m, self.v, self.opt_step, lr, self.betas[0], self.betas[1], self.eps,
                         self.weight_decay, grad_mul=clip_multiplier(norm, self.max_grad_norm) / scale)
        self.repack()
        return StepReport(self.sched_step, loss, norm, lr, scale, False)
