"""Times astts_op_qknorm_rope (Qwen3: q / k norm + RoPE in one launch) against the RoPE launch it replaces, astts_op_rope_llama /
astts_op_rope_llama_ex, at Qwen3-8B's shapes (32 + 8 heads of 128): one decode step of 1 row and of 256 rows (time-major, per-row shift)
and a prefill of 32 x 512 tokens (batch-major).  Device events around ``--calls`` back-to-back launches, ``--reps`` windows per
operator, the two operators alternating; prints the median and the range of the per-call time of each and one JSON line.
``--shape i --calls 200 --reps 2`` under ``rocprofv3 --kernel-trace --stats`` gives the kernels' own durations at one shape.

    python scripts/qknorm_probe.py [--calls 400] [--reps 15] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "autostyle-tts_amd")]

import astts  # noqa: E402,F401  (before torch.cuda: astts/_lib.py sets the hardware queue count)
import torch  # noqa: E402
from astts import ops  # noqa: E402

HEADS, KV, HD, EPS = 32, 8, 128, 1e-6
SHAPES = (("decode b=1", 1, 1, True), ("decode b=256", 256, 1, True), ("prefill 32x512", 32, 512, False))


def window(fn, calls: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", type=int, default=-1, help="run only SHAPES[i] (under a kernel trace: one shape per kernel name)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.float) / HD))
    fr = torch.arange(1024, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = fr.cos().to(dev).contiguous(), fr.sin().to(dev).contiguous()
    qw, kw = (1.0 + 0.1 * torch.randn(HD, generator=g)).to(dev), (1.0 + 0.1 * torch.randn(HD, generator=g)).to(dev)
    result = {}
    for name, b, t, tm in (SHAPES if args.shape < 0 else SHAPES[args.shape:args.shape + 1]):
        shape = (t, b, (HEADS + 2 * KV) * HD) if tm else (b, t, (HEADS + 2 * KV) * HD)
        x0 = torch.randn(*shape, generator=g).half().to(dev)
        shift = (torch.arange(b, dtype=torch.int32) % 7).to(dev) if tm else None
        pos0 = 300 if tm else 0
        xa, xb = x0.clone(), x0.clone()
        if tm:
            rope = lambda: ops.rope_llama_ex_(xa, cos, sin, HEADS + KV, HD, pos0=pos0, shift=shift, time_major=True)
        else:
            rope = lambda: ops.rope_llama_(xa, cos, sin, HEADS + KV, HD)
        fused = lambda: ops.qknorm_rope_(xb, cos, sin, qw, kw, HEADS, KV, HD, EPS, pos0=pos0, shift=shift, time_major=tm)
        for fn in (rope, fused):                     # warm-up: code objects, clocks
            window(fn, 50)
        times = {"rope": [], "qknorm_rope": []}
        for _ in range(args.reps):                   # alternate: both see the same neighbours
            times["rope"].append(window(rope, args.calls))
            times["qknorm_rope"].append(window(fused, args.calls))
        row = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
        row["bytes_qk"] = b * t * (HEADS + KV) * HD * 2
        result[name] = row
        print(f"{name}: rope {row['rope']['median_us']:.2f} us ({row['rope']['min_us']:.2f} .. {row['rope']['max_us']:.2f}), "
              f"qknorm_rope {row['qknorm_rope']['median_us']:.2f} us ({row['qknorm_rope']['min_us']:.2f} .. {row['qknorm_rope']['max_us']:.2f}) "
              f"per call over {args.calls} back-to-back calls x {args.reps} windows; q | k is {row['bytes_qk']} bytes", flush=True)
    line = json.dumps({"probe": "qknorm_rope", "calls": args.calls, "reps": args.reps, "shapes": result})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
