"""Texts per second of the BERT-family sentence encoder (astts.llm.encoder_bert.BertEmbedder) at the m3e-base shape: 256 texts of 60
tokens in one batch, seeded weights and token ids.  One process; warm-up passes, then the median over device events of ``--iters`` timed
passes of ``embed_ids`` (tokens on the host -> sentence vectors on the device).  Also prints the share of the fp16 MFMA peak that rate
is, from the layer stack's flop count (projections, attention products and FFN; LayerNorm, GELU and softmax not counted), and with
``--cpu`` the time transformers' BertModel takes for the same batch in fp32 on the host, as context.

    python scripts/bert_embed_probe.py [--texts 256] [--tokens 60] [--iters 20] [--warmup 5] [--cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd")]

MFMA_FP16_PEAK = 2.5e15          # dense fp16 MFMA, FLOP/s (MI355X specification)


def encoder_flops(shape, texts: int, tokens: int) -> float:
    """Multiply-adds x 2 of one pass: q | k | v, QK^T and PV over ``tokens`` keys, the output projection and the two FFN GEMMs."""
    h, f = shape.hidden, shape.ffn
    per_token = 2 * h * 3 * h + 2 * 2 * tokens * h + 2 * h * h + 2 * 2 * h * f
    return float(shape.layers * per_token * texts * tokens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=60)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="also time transformers' BertModel (fp32, host) on the same batch")
    args = ap.parse_args()

    import astts  # noqa: F401  before torch.cuda: astts/_lib.py sets GPU_MAX_HW_QUEUES
    import torch

    from astts.llm.config import BertShape
    from astts.llm.encoder_bert import BertEmbedder
    from astts.llm.weights import make_bert_weights

    if not torch.cuda.is_available():
        raise SystemExit("bert_embed_probe needs the GPU: a timing taken anywhere else says nothing about it")
    shape = BertShape.m3e_base()
    sd = make_bert_weights(shape, 0)
    emb = BertEmbedder(sd, shape, "cuda")
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, shape.vocab, (args.texts, args.tokens), generator=g)
    lens = torch.full((args.texts,), args.tokens, dtype=torch.int32)
    for _ in range(args.warmup):
        out = emb.embed_ids(ids, lens)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = emb.embed_ids(ids, lens)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e-3)
    assert bool(torch.isfinite(out).all())
    med = statistics.median(times)
    flops = encoder_flops(shape, args.texts, args.tokens)
    res = {"probe": "bert_embed", "shape": "m3e_base", "texts": args.texts, "tokens": args.tokens, "iters": args.iters,
           "seconds_median": med, "seconds_min": min(times), "seconds_max": max(times), "texts_per_second": args.texts / med,
           "gflop_per_pass": flops / 1e9, "tflops": flops / med / 1e12, "share_of_fp16_mfma_peak": flops / med / MFMA_FP16_PEAK}
    if args.cpu:
        from transformers import BertModel

        cfg = shape.hf_config()
        cfg._attn_implementation = "eager"
        model = BertModel(cfg, add_pooling_layer=False).eval().float()
        model.load_state_dict(sd, strict=False, assign=True)
        with torch.no_grad():
            model(input_ids=ids[:8])                                                     # warm-up
            c0 = time.perf_counter()
            model(input_ids=ids)
            res["host_fp32_transformers_seconds"] = time.perf_counter() - c0
        res["host_threads"] = torch.get_num_threads()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
