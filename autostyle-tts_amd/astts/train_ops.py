"""Python wrappers of libastts_train.so: the backward and optimizer kernels of LoRA fine-tuning (csrc/train/*.hip).  Tensors are
torch CUDA tensors, the launch goes to the current stream, nothing synchronises and nothing falls back to PyTorch."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib, _lib_train

check = _lib_train.check


def _L():
    return _lib_train.load()


def _st():
    return _lib.stream_ptr()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)


def attn_gqa_bwd(qkv: torch.Tensor, dout: torch.Tensor, heads: int, kv_heads: int, head_dim: int,
                 lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal GQA attention backward.  ``qkv`` fp16 ``[B, T, (heads + 2 kv_heads) * hd]`` = rotated q | rotated k | v; ``dout`` fp16
    ``[B, T, heads * hd]``; ``lens`` int32 ``[B]`` (right padding) -> dq | dk | dv fp16, laid out as ``qkv`` (still in the rotated basis)."""
    assert qkv.is_cuda and qkv.dtype == dout.dtype == torch.float16 and qkv.dim() == dout.dim() == 3
    assert qkv.is_contiguous() and dout.is_contiguous(), "attn_gqa_bwd takes whole planes"
    b, t, w = qkv.shape
    assert w == (heads + 2 * kv_heads) * head_dim and dout.shape == (b, t, heads * head_dim), (qkv.shape, dout.shape)
    if lens is not None:
        assert lens.is_cuda and lens.dtype == torch.int32 and lens.shape == (b,) and lens.is_contiguous()
    out = torch.empty_like(qkv)
    ws = _ws(_L().astts_train_attn_gqa_bwd_workspace_bytes(b, t, heads), qkv.device)
    check(_L().astts_train_attn_gqa_bwd(qkv.data_ptr(), dout.data_ptr(), None if lens is None else lens.data_ptr(), out.data_ptr(), b, t,
                                        heads, kv_heads, head_dim, w, heads * head_dim, w, 1.0 / math.sqrt(head_dim), ws.data_ptr(),
                                        ws.numel(), _st()))
    return out


def qknorm_rope_bwd_(dqkv: torch.Tensor, x_pre: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, q_norm_w: torch.Tensor,
                     k_norm_w: torch.Tensor, heads: int, kv_heads: int, head_dim: int, eps: float, pos0: int = 0) -> torch.Tensor:
    """The transpose of ops.qknorm_rope_ (Qwen3), in place on the q | k columns of ``dqkv`` fp16 ``[B, T, ld]`` (d(rotated q | k) as
    attn_gqa_bwd leaves it -> d(pre-norm q | k)); ``x_pre`` fp16 ``[B, T, >= (heads + kv_heads) * hd]``: the q | k the forward op read.
    The norm weights are frozen (no weight gradient); dv and the padding are not touched."""
    wqk = (heads + kv_heads) * head_dim
    for a in (dqkv, x_pre):
        assert a.is_cuda and a.dtype == torch.float16 and a.dim() == 3 and a.stride(2) == 1 and a.stride(0) == a.shape[1] * a.stride(1)
        assert a.shape[2] >= wqk, (a.shape, wqk)
    b, t = dqkv.shape[0], dqkv.shape[1]
    assert x_pre.shape[:2] == (b, t)
    assert cos.shape[0] >= pos0 + t and cos.shape == sin.shape and cos.shape[1] == head_dim // 2 and cos.is_contiguous() and sin.is_contiguous()
    assert cos.dtype == sin.dtype == torch.float32
    for w in (q_norm_w, k_norm_w):
        assert w.is_cuda and w.dtype == torch.float32 and w.shape == (head_dim,) and w.is_contiguous(), (w.dtype, w.shape)
    check(_L().astts_train_qknorm_rope_bwd(dqkv.data_ptr(), dqkv.stride(1), x_pre.data_ptr(), x_pre.stride(1), cos.data_ptr(), sin.data_ptr(),
                                           q_norm_w.data_ptr(), k_norm_w.data_ptr(), b, t, heads, kv_heads, head_dim, pos0, float(eps), _st()))
    return dqkv


def rmsnorm_bwd_(dres: torch.Tensor, dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """``dres += d rmsnorm(x, w) / dx applied to dy``: all fp32, ``[..., c]`` contiguous; the weight is frozen (no dw)."""
    for t in (dres, dy, x, w):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.shape)
    c = x.shape[-1]
    assert dres.shape == dy.shape == x.shape and w.shape == (c,)
    check(_L().astts_train_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), dres.data_ptr(), x.numel() // c, c, float(eps), _st()))
    return dres


def swiglu_bwd(dout: torch.Tensor, gate_up: torch.Tensor) -> torch.Tensor:
    """``dout`` fp16 ``[..., f]``, ``gate_up`` fp16 ``[..., 2f]`` -> d(gate | up) fp16 ``[..., 2f]``."""
    assert dout.is_cuda and dout.dtype == gate_up.dtype == torch.float16 and dout.is_contiguous() and gate_up.is_contiguous()
    f = dout.shape[-1]
    assert gate_up.shape == (*dout.shape[:-1], 2 * f), (dout.shape, gate_up.shape)
    out = torch.empty_like(gate_up)
    check(_L().astts_train_swiglu_bwd(dout.data_ptr(), gate_up.data_ptr(), out.data_ptr(), dout.numel() // f, f, _st()))
    return out


def xent_grad_(logits: torch.Tensor, lse: torch.Tensor, targets: torch.Tensor, scale: float) -> torch.Tensor:
    """In place: fp32 logits ``[rows, vocab]`` -> ``(softmax - onehot(target)) * scale``; rows with target -1 -> zeros."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows, vocab = logits.shape
    assert lse.dtype == torch.float32 and lse.shape == (rows,) and lse.is_contiguous()
    assert targets.dtype == torch.int32 and targets.shape == (rows,) and targets.is_contiguous()
    check(_L().astts_train_xent_grad(logits.data_ptr(), logits.stride(0), lse.data_ptr(), targets.data_ptr(), rows, vocab, float(scale), _st()))
    return logits


def lora_grad_row_split() -> int:
    return int(_L().astts_train_lora_grad_row_split())


def lora_grad(u: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None, alpha: float = 1.0,
              accumulate: bool = False) -> torch.Tensor:
    """``G[n, k] = (accumulate ? G : 0) + alpha * sum_rows u[row, n] * x[row, k]``: ``u`` ``[rows, n]`` fp16 or fp32 (rounded to fp16),
    ``x`` ``[rows, k]`` fp16, both possibly column slices of wider planes (unit column stride); ``out`` fp32 ``[n, k]``."""
    assert u.is_cuda and u.dim() == 2 and x.dim() == 2 and u.shape[0] == x.shape[0] and u.stride(1) == 1 and x.stride(1) == 1
    assert u.dtype in (torch.float16, torch.float32) and x.dtype == torch.float16, (u.dtype, x.dtype)
    rows, n = u.shape
    k = x.shape[1]
    if out is None:
        assert not accumulate
        out = torch.empty((n, k), dtype=torch.float32, device=u.device)
    assert out.dtype == torch.float32 and out.shape == (n, k) and out.stride(1) == 1
    ws = _ws(_L().astts_train_lora_grad_workspace_bytes(rows, n, k), u.device)
    check(_L().astts_train_lora_grad(u.data_ptr(), 1 if u.dtype == torch.float32 else 0, u.stride(0), x.data_ptr(), x.stride(0),
                                     out.data_ptr(), out.stride(0), rows, n, k, float(alpha), 1 if accumulate else 0, ws.data_ptr(),
                                     ws.numel(), _st()))
    return out


def sumsq(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum of squares of a flat fp32 buffer -> fp32 ``[1]`` on the device (not finite exactly when an element is not)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=x.device)
    ws = _ws(_L().astts_train_sumsq_workspace_bytes(x.numel()), x.device)
    check(_L().astts_train_sumsq(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
    return out


def adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float, beta1: float = 0.9,
           beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, grad_mul: float = 1.0) -> None:
    """One AdamW step (``step`` >= 1) in place on flat fp32 buffers; the gradient counts as ``grad_mul * g``."""
    for t in (p, g, m, v):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous() and t.numel() == p.numel()
    assert step >= 1
    check(_L().astts_train_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(beta1), float(beta2),
                                 float(eps), float(weight_decay), 1.0 - beta1 ** step, 1.0 - beta2 ** step, float(grad_mul), _st()))


def lora_merge(w_pack, a: torch.Tensor, b: torch.Tensor, out_pack, r: int, g1: int, g2: int, scaling: float):
    """``out_pack`` <- fp16(``w_pack`` + scaling * B A), part by part: ``w_pack`` / ``out_pack`` are PackedWeights of one geometry
    (distinct images), ``a`` the fp32 master ``[parts * r, cin]``, ``b`` the fp32 master ``[n, r]`` (the parts' B back to back), rows
    below ``g1`` part 0, below ``g2`` part 1, the rest part 2 (``g1 = g2 = n``: a single projection).  fp32 accumulation in a fixed
    order: repeatable bit for bit.  ``w_pack`` is left as it is."""
    n, cin = w_pack.n, w_pack.cin
    assert w_pack.taps == 1 and out_pack.taps == 1 and (out_pack.n, out_pack.cin, out_pack.n_pad, out_pack.cin_pad) == (n, cin, w_pack.n_pad, w_pack.cin_pad)
    assert w_pack.data.dtype == out_pack.data.dtype == torch.float16 and w_pack.data.is_contiguous() and out_pack.data.is_contiguous()
    parts = 1 + (1 if g1 < n else 0) + (1 if g2 < n else 0)
    for t in (a, b):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == w_pack.data.device, (t.dtype, t.shape, t.device)
    assert a.shape == (parts * r, cin) and b.shape == (n, r), (a.shape, b.shape, parts, r, n, cin)
    check(_L().astts_train_lora_merge(w_pack.data.data_ptr(), a.data_ptr(), b.data_ptr(), out_pack.data.data_ptr(), n, cin, w_pack.n_pad,
                                      w_pack.cin_pad, int(r), int(g1), int(g2), float(scaling), _st()))
    return out_pack


# ---- the regularisers: LoRA dropout from a counter-based generator (no stored masks) and NEFTune.  The contract of (seed, rng_stream,
# draw) is in include/train/astts_train.h; part j of a fused projection uses rng_stream + j
NEFTUNE_STREAM = 0xFFFFFFFF


def dropout_threshold(p: float) -> int:
    """An element is kept iff its 16 random bits are >= this."""
    return int(math.floor(p * 65536))


def dropout_mask(rows: int, cin: int, p: float, seed: int, rng_stream: int, draw: int, device=None) -> torch.Tensor:
    """The keep mask of one (seed, rng_stream, draw, p): uint8 ``[rows, cin]``.  The training path never stores one; this pins the generator."""
    out = torch.empty((rows, cin), dtype=torch.uint8, device=device or torch.device("cuda", torch.cuda.current_device()))
    check(_L().astts_train_dropout_mask(out.data_ptr(), rows, cin, float(p), int(seed), int(rng_stream), int(draw), _st()))
    return out


def neftune_(x: torch.Tensor, mag: float, seed: int, draw: int) -> torch.Tensor:
    """In place on fp32 ``[..., hidden]``: ``x += mag * (2u - 1)``, u uniform in (0, 1) from the generator's NEFTune stream."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    hidden = x.shape[-1]
    check(_L().astts_train_neftune(x.data_ptr(), x.numel() // hidden, hidden, float(mag), int(seed), int(draw), _st()))
    return x


def lora_down(x: torch.Tensor, a_pack, parts: int, r: int, p: float, seed: int, rng_stream: int, draw: int) -> torch.Tensor:
    """``t[rows, parts * r]`` fp16, column block j = ``(mask_j * x) @ A_j.T / (1 - p)``: ``x`` fp16 ``[rows, cin]``, ``a_pack`` the
    PackedWeight of the stacked ``[parts * r, cin]`` A.  ``p == 0`` has no mask to draw: it is ``ops.linear`` itself."""
    assert x.is_cuda and x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1
    rows, cin = x.shape
    assert a_pack.n == parts * r and a_pack.cin == cin and a_pack.taps == 1, (a_pack.n, a_pack.cin, parts, r, cin)
    if p == 0.0:
        from . import ops
        return ops.linear(x, a_pack, out_dtype=torch.float16)
    t = torch.empty((rows, parts * r), dtype=torch.float16, device=x.device)
    check(_L().astts_train_lora_down(x.data_ptr(), x.stride(0), a_pack.data.data_ptr(), a_pack.cin_pad, t.data_ptr(), t.stride(0), rows, cin,
                                     parts, r, float(p), int(seed), int(rng_stream), int(draw), _st()))
    return t


def lora_grad_dropout(u: torch.Tensor, x: torch.Tensor, parts: int, r: int, p: float, seed: int, rng_stream: int, draw: int,
                      out: Optional[torch.Tensor] = None, alpha: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    """``lora_grad`` with ``u`` ``[rows, parts * r]`` and the dropout masks applied to ``x`` ``[rows, cin]`` as it is read: rows
    ``j * r .. (j + 1) * r`` of the result see mask j, and ``alpha / (1 - p)`` scales it."""
    assert u.is_cuda and u.dim() == 2 and x.dim() == 2 and u.shape[0] == x.shape[0] and u.stride(1) == 1 and x.stride(1) == 1
    assert u.dtype in (torch.float16, torch.float32) and x.dtype == torch.float16, (u.dtype, x.dtype)
    rows, n = u.shape
    cin = x.shape[1]
    assert n == parts * r, (n, parts, r)
    if out is None:
        assert not accumulate
        out = torch.empty((n, cin), dtype=torch.float32, device=u.device)
    assert out.dtype == torch.float32 and out.shape == (n, cin) and out.stride(1) == 1
    ws = _ws(_L().astts_train_lora_grad_workspace_bytes(rows, n, cin), u.device)
    check(_L().astts_train_lora_grad_dropout(u.data_ptr(), 1 if u.dtype == torch.float32 else 0, u.stride(0), x.data_ptr(), x.stride(0),
                                             out.data_ptr(), out.stride(0), rows, parts, r, cin, float(alpha), 1 if accumulate else 0,
                                             float(p), int(seed), int(rng_stream), int(draw), ws.data_ptr(), ws.numel(), _st()))
    return out


def lora_dx_dropout(dt: torch.Tensor, at_pack, residual: torch.Tensor, parts: int, r: int, p: float, seed: int, rng_stream: int,
                    draw: int, out_dtype=torch.float32) -> torch.Tensor:
    """``dx = residual + sum_j mask_j * (dt_j @ A_j) / (1 - p)``: ``dt`` fp16 ``[rows, parts * r]``, ``at_pack`` the PackedWeight of the
    transposed stack ``[cin, parts * r]``, ``residual`` fp32 ``[rows, cin]``.  fp32 output overwrites ``residual``; fp16 is a new tensor."""
    assert dt.is_cuda and dt.dtype == torch.float16 and dt.dim() == 2 and dt.stride(1) == 1
    rows, n = dt.shape
    cin = at_pack.n
    assert n == parts * r and at_pack.cin == n and at_pack.taps == 1, (n, parts, r, at_pack.cin)
    assert residual.dtype == torch.float32 and residual.shape == (rows, cin) and residual.is_contiguous()
    assert out_dtype in (torch.float32, torch.float16)
    out = residual if out_dtype == torch.float32 else torch.empty((rows, cin), dtype=torch.float16, device=dt.device)
    check(_L().astts_train_lora_dx_dropout(dt.data_ptr(), dt.stride(0), at_pack.data.data_ptr(), at_pack.cin_pad, residual.data_ptr(),
                                           out.data_ptr(), 1 if out_dtype == torch.float16 else 0, rows, cin, parts, r, float(p), int(seed),
                                           int(rng_stream), int(draw), _st()))
    return out
