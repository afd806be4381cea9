"""Time one LoRA training step at Llama-3.2-3B shapes ("One timing for the record"): seeded weights drawn on
the device, all 28 layers, vocabulary 128 256, r = 32, one micro-batch of 4 x 512 tokens; a warm-up step, then the mean of
``--steps`` steps (forward, backward, norm, AdamW, re-pack), each ended by a device synchronise.  Prints one JSON line.

    python tools/time_lora_step.py                                          # regularisers off
    python tools/time_lora_step.py --lora_dropout 0.05 --neftune_noise_alpha 5

With both at 0 no regulariser argument is passed, so the same file times a tree from before they existed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--layers", type=int, default=None, help="fewer than the model's 28 (a rehearsal)")
    ap.add_argument("--lora_r", type=int, default=32)
    ap.add_argument("--lora_dropout", type=float, default=0.0)
    ap.add_argument("--neftune_noise_alpha", type=float, default=0.0)
    ap.add_argument("--tag", type=str, default="")
    args = ap.parse_args()

    import dataclasses

    import astts  # noqa: F401  before the first torch.cuda call
    import torch
    from astts.llm.config import LlamaShape
    from astts.llm.train import LoraTrainer
    from astts.llm.weights import make_llama_weights

    assert torch.cuda.is_available(), "this measures a GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    cfg = LlamaShape.llama32_3b()
    if args.layers:
        cfg = dataclasses.replace(cfg, layers=args.layers)
    sd = make_llama_weights(cfg, 0, device=dev)
    kw = {}
    if args.lora_dropout or args.neftune_noise_alpha:
        kw = dict(lora_dropout=args.lora_dropout, neftune_alpha=args.neftune_noise_alpha)
    tr = LoraTrainer(sd, cfg, dev, r=args.lora_r, lora_alpha=128.0, total_steps=args.steps + args.warmup, warmup_ratio=0.0,
                     rope_len=args.seq + 64, **kw)
    del sd
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(3, cfg.vocab, (args.batch, args.seq), generator=g)
    lens = torch.full((args.batch,), args.seq, dtype=torch.int64)
    for _ in range(args.warmup):
        tr.step([(ids, lens)])
    torch.cuda.synchronize()
    times, reports = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        reports.append(tr.step([(ids, lens)]))
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    mean = sum(times) / len(times)
    print(json.dumps({"tag": args.tag, "ms_per_step": round(mean, 3), "ms_steps": [round(t, 3) for t in times],
                      "tokens_per_s": round(args.batch * args.seq / mean * 1e3, 1), "layers": cfg.layers, "batch": args.batch, "seq": args.seq,
                      "r": args.lora_r, "lora_dropout": args.lora_dropout, "neftune_noise_alpha": args.neftune_noise_alpha,
                      "losses": [round(r.loss, 4) for r in reports], "skipped": [r.skipped for r in reports],
                      "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


if __name__ == "__main__":
    main()
