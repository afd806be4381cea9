"""Throughput of the LLM.int8 + LoRA embedder against the fp16 one at the bench's shape (256 texts x 60 tokens, the full 28-layer
Llama-3.2-3B, seeded weights drawn on the GPU), and per-shape TOPS of the int8 GEMM (astts_op_i8_gemm, no side terms) as a fraction
of the i8 MFMA peak.  Prints one JSON line.

    python scripts/llm_int8_probe.py [--batch 256] [--tokens 60] [--iters 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd")):
    sys.path.insert(0, p)

import astts  # noqa: E402,F401  (before the first torch.cuda call: astts/_lib.py sets the queue count)
from astts import _lib  # noqa: E402,F401
import torch  # noqa: E402

I8_PEAK_TOPS = 5033.0     # MI355X dense int8 MFMA peak (2x the fp16 peak)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=60)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    from astts import ops
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights

    dev = "cuda"
    m = a.batch * a.tokens
    out = {"batch": a.batch, "tokens": a.tokens, "gemm": {}}
    for n, k in [(5120, 3072), (3072, 3072), (16384, 3072), (3072, 8192)]:
        w = torch.randn(n, k, device=dev) * 0.04
        cb, scb = ops.i8_quantize_weight(w)
        x = torch.randn(m, k, device=dev).to(torch.float16)
        seg = (torch.arange(m, dtype=torch.int32, device=dev) // a.tokens).contiguous()
        act = ops.i8_quantize_act(x, seg, a.batch, 6.0)
        t_i8 = timed(lambda: ops.i8_gemm(act, cb, scb, n, outliers=False), a.iters)
        t_q = timed(lambda: ops.i8_quantize_act(x, seg, a.batch, 6.0), a.iters)
        pw = ops.PackedWeight(w, None, dev)
        t_f16 = timed(lambda: ops.linear(x, pw, out_dtype=torch.float16), a.iters)
        tops = 2.0 * m * n * k / t_i8 / 1e12
        out["gemm"][f"{n}x{k}"] = {"i8_us": round(t_i8 * 1e6, 1), "i8_tops": round(tops, 1), "frac_peak": round(tops / I8_PEAK_TOPS, 3),
                                   "quant_act_us": round(t_q * 1e6, 1), "f16_ring_us": round(t_f16 * 1e6, 1)}
        del w, cb, scb, x, act, pw
    cfg = LlamaShape.llama32_3b()
    sd = make_llama_weights(cfg, 0, device=dev)
    ids = torch.randint(3, 5000, (a.batch, a.tokens), generator=torch.Generator().manual_seed(0))
    lens = torch.full((a.batch,), a.tokens, dtype=torch.int32)
    from types import SimpleNamespace

    g = torch.Generator(device=dev).manual_seed(1)
    dims = {"q_proj": (cfg.hidden, cfg.heads * 128), "k_proj": (cfg.hidden, cfg.kv_heads * 128), "v_proj": (cfg.hidden, cfg.kv_heads * 128),
            "o_proj": (cfg.heads * 128, cfg.hidden), "gate_proj": (cfg.hidden, cfg.ffn), "up_proj": (cfg.hidden, cfg.ffn),
            "down_proj": (cfg.ffn, cfg.hidden)}
    pairs = {(i, p): (torch.randn(32, di, generator=g, device=dev) * 0.02, torch.randn(do, 32, generator=g, device=dev) * 0.02)
             for i in range(cfg.layers) for p, (di, do) in dims.items()}
    lora = SimpleNamespace(pairs=pairs, scaling=128 / 32)
    res = {}
    for name, kw in [("fp16", {}), ("int8_lora", {"int8": True, "lora": lora})]:
        emb = LlamaEmbedder(sd, cfg, dev, **kw)
        t = timed(lambda: emb.embed_ids(ids, lens), max(1, a.iters // 2))
        res[name] = {"s_per_batch": round(t, 4), "texts_per_s": round(a.batch / t, 1)}
        del emb
        torch.cuda.empty_cache()
    out["embedder"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
