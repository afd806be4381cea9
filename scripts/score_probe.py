"""Fused head log-probabilities (ops.head_logprob) against the path a user had before it: ops.linear into fp32 logits, then
torch.log_softmax and a gather.  hidden 3072, vocab 128 256, rows in {32, 576, 4096, 16 384}; both paths on the same N(0, 1) data,
alternating in one process; per path the median / min of the rounds (device events around `inner` calls) and the peak device memory
above the resident operands.  --only fused|plain runs one path (for a kernel trace in a run of its own).

    python scripts/score_probe.py [--rows 32 576 4096 16384] [--rounds 7] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[32, 576, 4096, 16384])
    ap.add_argument("--hidden", type=int, default=3072)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["fused", "plain"], default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import astts  # noqa: F401
    import torch
    from astts import ops

    assert torch.cuda.is_available(), "score_probe needs the GPU"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(args.vocab, args.hidden, generator=g, device=dev) / args.hidden ** 0.5
    head = ops.PackedWeight(w, None, dev)
    del w
    out = []
    for rows in args.rows:
        h32 = torch.randn(rows, args.hidden, generator=g, device=dev)
        h16 = h32.to(torch.float16)
        t = torch.randint(0, args.vocab, (rows,), generator=g, device=dev, dtype=torch.int32)
        t64 = t.to(torch.int64)

        def fused():
            return ops.head_logprob(h16, head, t)

        def plain():     # what the parent commit offers: the logits plane, then torch
            lg = ops.linear(h32, head)
            return torch.log_softmax(lg, dim=-1).gather(1, t64[:, None])[:, 0]

        paths = {"fused": fused, "plain": plain}
        if args.only:
            paths = {args.only: paths[args.only]}
        inner = max(1, min(20, 4096 // rows))
        times = {k: [] for k in paths}
        peak = {}
        for k, fn in paths.items():           # warm-up + peak memory of one call
            fn()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            r = fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
            del r
        if len(paths) == 2:
            d = float((fused().double() - plain().double()).abs().max())
        else:
            d = None
        for _ in range(args.rounds):
            for k, fn in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / inner)
        rec = {"rows": rows, "hidden": args.hidden, "vocab": args.vocab, "inner": inner, "rounds": args.rounds, "max_abs_diff": d}
        flop = 2.0 * rows * args.hidden * args.vocab
        for k in paths:
            ts = sorted(times[k])
            rec[k] = {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "peak_bytes": int(peak[k]),
                      "tflops_at_median": flop / (ts[len(ts) // 2] * 1e-3) / 1e12}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del h32, h16, t, t64
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
