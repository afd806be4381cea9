"""IVF_FLAT index against the brute-force search on one GPU: time per search, recall, build time ("IVF_FLAT").

    python scripts/knn_ivf_probe.py [--out FILE.json] [--quick]

One process.  Every timing is a median over ``--repeats`` searches after ``--warmup`` of them, each between a pair of HIP events on the
search stream (``search_ivf_device`` / ``search_device`` on the same handle, the same queries, in the same run; the brute-force search is
the code the index does not touch).  ``scan GB/s`` divides the bytes of the rows the chunk's probed lists hold -- every list once, the
list-major scan's ideal traffic -- by the IVF search time minus the time of its coarse search (the centroid bank searched alone): the
list scan and the selection together, so a lower bound for the scan kernel.
Recall@k: the share of the brute-force top-k ids an IVF search returns.  Banks: a clustered synthetic one (256 Gaussian blobs), an
unclustered Gaussian one (the stress leg's: the brute-force search certifies its fp16 scan there, which it cannot inside a tight blob --
``brute_fallbacks`` counts the queries that took its exact fp64 path), and the shipped 130 x 6144 bank at nlist 128 / nprobe 10 with its
own rows as queries (the known-answer file's self-retrieval hits).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd")]

import numpy as np  # noqa: E402
import astts  # noqa: E402,F401  (before the first torch.cuda call: GPU_MAX_HW_QUEUES)
import torch  # noqa: E402
from astts.knn import StyleBank  # noqa: E402

HBM_GBS = 8000.0


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)      # us


def make_bank(kind, n, d, seed, blobs=256):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bank = torch.randn((n, d), generator=g, device="cuda")
    if kind == "clustered":
        centres = 4.0 * torch.randn((blobs, d), generator=g, device="cuda")
        bank += centres[torch.randint(0, blobs, (n,), generator=g, device="cuda")]
    bank = bank.to(torch.float16)
    qrow = torch.randint(0, n, (256,), generator=g, device="cuda")
    q = bank[qrow].float() + 0.5 * torch.randn((256, d), generator=g, device="cuda")
    return bank, q.contiguous()


def recall(ivf_idx, brute_idx):
    hit = (ivf_idx[:, :, None] == brute_idx[:, None, :]).any(1)
    return float(hit.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one shape, one nlist: a smoke run of the script itself")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--niter", type=int, default=20)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "warmup": args.warmup, "repeats": args.repeats,
           "niter": args.niter, "build": [], "search": [], "recall": []}
    shapes = [(20000, 768)] if args.quick else [(100000, 6144), (100000, 768)]
    nlists = [128] if args.quick else [128, 1024]
    k = 10
    for kind, (n, d) in [(kind, shape) for shape in shapes for kind in ("gaussian", "clustered")]:
        bank, q = make_bank(kind, n, d, 7)
        sb = StyleBank(bank)
        del bank
        brute, fallbacks = {}, {}
        for nq in (1, 8, 64, 256):
            brute[nq] = timed(lambda: sb.search_device(q[:nq], k), args.warmup, args.repeats)
            fallbacks[nq] = sb.last_fallbacks()
        bidx = {kk: sb.search_device(q, kk)[0] for kk in (3, 10)}
        for nlist in nlists:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = sb.build_index(nlist, niter=args.niter)
            build_s = time.perf_counter() - t0
            cent, list_of = sb.index_export()
            lens = np.bincount(list_of, minlength=info["nlist"])
            res["build"].append({"bank": kind, "n": n, "d": d, "nlist": nlist, "niter": args.niter, "seconds": round(build_s, 3),
                                 "max_list_len": info["max_list_len"], "mean_list_len": float(lens.mean())})
            print(f"build {kind} {n} x {d} nlist {nlist} niter {args.niter}: {build_s:.2f} s, lists of {lens.min()}..{lens.max()} rows", flush=True)
            cb = StyleBank(torch.from_numpy(cent).cuda())
            for nprobe in (1, 10, 32):
                res["recall"].append({"bank": f"{kind} {n} x {d}", "nlist": nlist, "nprobe": nprobe,
                                      "recall@3": recall(sb.search_ivf_device(q, 3, nprobe)[0], bidx[3]),
                                      "recall@10": recall(sb.search_ivf_device(q, 10, nprobe)[0], bidx[10])})
                for nq in (1, 8, 64, 256):
                    t_ivf = timed(lambda: sb.search_ivf_device(q[:nq], k, nprobe), args.warmup, args.repeats)
                    t_coarse = timed(lambda: cb.search_device(q[:nq], nprobe), args.warmup, args.repeats)
                    probed = cb.search_device(q[:nq], nprobe)[0].unique().cpu().numpy()
                    gbytes = float(lens[probed].sum()) * sb.d * 2 / 1e9
                    row = {"bank": kind, "n": n, "d": d, "nlist": nlist, "nprobe": nprobe, "Q": nq, "ivf_us": round(t_ivf, 1),
                           "brute_us": round(brute[nq], 1), "brute_fallbacks": fallbacks[nq],
                           "coarse_us": round(t_coarse, 1), "speedup": round(brute[nq] / t_ivf, 2), "lists_read": int(probed.size),
                           "scan_GBps": round(gbytes / max(t_ivf - t_coarse, 1e-3) * 1e6, 1)}
                    row["scan_of_hbm"] = round(row["scan_GBps"] / HBM_GBS, 3)
                    res["search"].append(row)
                    print(json.dumps(row), flush=True)
            cb.close()
        sb.close()
        del sb
        torch.cuda.empty_cache()
    # the shipped bank: nlist 128, nprobe 10, its rows as queries
    golden = os.path.join(ROOT, "tests", "golden")
    real = np.load(os.path.join(golden, "style_bank_130x6144.f16.npy"))
    kats = json.load(open(os.path.join(golden, "knn_kats.json")))
    sb = StyleBank(real)
    sb.build_index(128, niter=args.niter)
    qs = torch.from_numpy(real.astype(np.float32)).cuda()
    got = sb.search_ivf_device(qs, 5, 10)[0].cpu().numpy()
    want = np.asarray(kats["self_top5_idx"])
    kept = int(sum(len(set(g.tolist()) & set(w.tolist())) for g, w in zip(got, want)))
    rng = np.random.default_rng(0)
    qn = torch.from_numpy((real.astype(np.float32) + 0.5 * rng.standard_normal(real.shape)).astype(np.float32)).cuda()
    res["recall"].append({"bank": "shipped 130 x 6144", "nlist": 128, "nprobe": 10,
                          "recall@3": recall(sb.search_ivf_device(qn, 3, 10)[0], sb.search_device(qn, 3)[0]),
                          "recall@10": recall(sb.search_ivf_device(qn, 10, 10)[0], sb.search_device(qn, 10)[0]),
                          "kat_self_top5_hits_kept": kept, "kat_self_top5_hits": int(want.size),
                          "kat_self_top1_kept": int((got[:, 0] == want[:, 0]).sum())})
    sb.close()
    for r in res["recall"]:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
