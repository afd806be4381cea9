"""Definition of astts_op_head_logprob (csrc/ops_score.hip, include/astts.h), restated in float64 on the operands the kernel sees.

    logit[m][c] = sum_k h16[m][k] * w16[c][k] (+ bias[c])        h16, w16: the fp16-rounded operands, every product and sum in float64
    logprob[m]  = logit[m][t] - logsumexp(logit[m][0 .. vocab))   t = targets[m]
    targets[m] outside [0, vocab) (-1 by convention): ignored -- logprob[m] = 0, ignored[m] = True
    columns at or beyond ``vocab`` (the head's padding, or a head wider than the vocabulary) take no part in the maximum, the sum
    or the argmax; argmax ties go to the lowest column (torch.argmax / astts_op_argmax_rows).

tests/test_llm_scoring_cpu.py holds this to torch.nn.functional.cross_entropy / log_softmax; tests/test_llm_scoring_gpu.py holds the
kernel to this.  Works on any device (the GPU test runs the large cases in float64 on the GPU, in row chunks).
"""
import torch


def head_logits(h, w, bias=None, vocab=None):
    """float64 logits ``[rows, vocab]`` of fp16-rounded ``h`` ``[rows, k]`` and ``w`` ``[n >= vocab, k]``."""
    vocab = w.shape[0] if vocab is None else vocab
    lg = h.to(torch.float16).to(torch.float64) @ w[:vocab].to(torch.float16).to(torch.float64).T
    if bias is not None:
        lg = lg + bias[:vocab].to(torch.float64)
    return lg


def logprob_from_logits(lg, targets):
    """``lg`` float64 ``[rows, vocab]`` (tail already cut), ``targets`` int ``[rows]`` -> dict(logprob, lse, argmax, ignored, top2_gap)."""
    rows, vocab = lg.shape
    t = targets.to(torch.int64)
    ignored = (t < 0) | (t >= vocab)
    mx = lg.max(dim=1).values
    lse = mx + torch.log(torch.exp(lg - mx[:, None]).sum(dim=1))
    picked = lg.gather(1, t.clamp(0, vocab - 1)[:, None])[:, 0]
    logprob = torch.where(ignored, torch.zeros_like(lse), picked - lse)
    # lowest column among the maxima (torch.argmax does not promise which of several equal entries it returns)
    cols = torch.arange(vocab, device=lg.device)[None, :].expand(rows, vocab)
    argmax = torch.where(lg == mx[:, None], cols, torch.full_like(cols, vocab)).min(dim=1).values
    if vocab > 1:
        top2 = lg.topk(2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
    else:
        gap = torch.full_like(mx, float("inf"))
    return {"logprob": logprob, "lse": lse, "argmax": argmax.to(torch.int32), "ignored": ignored, "top2_gap": gap}


def head_logprob(h, w, targets, bias=None, vocab=None, chunk=1024):
    """The whole definition; rows are taken ``chunk`` at a time so that the float64 logits of a wide vocabulary fit.  Also returns
    ``logit_absmax``: the largest |logit| met (the scale the GEMM tolerance is relative to)."""
    out = {k: [] for k in ("logprob", "lse", "argmax", "ignored", "top2_gap")}
    amax = 0.0
    for r0 in range(0, h.shape[0], chunk):
        lg = head_logits(h[r0:r0 + chunk], w, bias, vocab)
        amax = max(amax, float(lg.abs().max()))
        part = logprob_from_logits(lg, targets[r0:r0 + chunk])
        for k in out:
            out[k].append(part[k])
    res = {k: torch.cat(v) for k, v in out.items()}
    res["logit_absmax"] = amax
    return res
