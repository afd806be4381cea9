"""Host cost of a style-bank search on one GPU: what the Python side of ``StyleBank.search_device`` adds to a launch-bound search
(21.7 us per search at the benchmark's shape, 9.4 us of it the host side of the call).

    python scripts/knn_host_probe.py [--out FILE.json] [--calls 500] [--warmup 50] [--repeats 7]

One process; the public API only, so the same file measures any commit that has it.  Bank 1000 x 6144 fp16, 8 queries, k = 3,
preallocated outputs.  Two figures, each the median of ``--repeats`` repetitions after ``--warmup`` calls:
  host_us    wall time of ``--calls`` calls enqueued with no synchronisation inside the loop, per call: the host side alone (the clock
             stops before the GPU has finished, which is the point);
  search_us  the same loop with the final ``torch.cuda.synchronize()`` inside the clock, per call: the time per search, as bench.py
             computes ``knn_qps``.
The same two figures for one grouped search (limit 3 x group_size 2 over 10 groups; it synchronises once per round by design) and
one IVF search (nlist 16, nprobe 4) are printed for the record.  Compare commits in fresh processes, alternating, in one visit.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd")]

import astts  # noqa: E402,F401  (before the first torch.cuda call: GPU_MAX_HW_QUEUES)
import torch  # noqa: E402
from astts.knn import StyleBank  # noqa: E402


def measure(fn, calls, warmup, repeats):
    """-> (host us per call, us per search): medians over ``repeats`` loops of ``calls`` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    host, total = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((t1 - t0) / calls * 1e6)
        total.append((t2 - t0) / calls * 1e6)
    return round(statistics.median(host), 3), round(statistics.median(total), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    n, d, nq, k = 1000, 6144, 8, 3
    g = torch.Generator(device="cuda").manual_seed(11)
    bank = torch.randn((n, d), generator=g, device="cuda").to(torch.float16)
    q = (bank[:nq].float() + 0.5 * torch.randn((nq, d), generator=g, device="cuda")).contiguous()
    groups = (torch.arange(n, device="cuda") % 10).to(torch.int32)
    sb = StyleBank(bank)
    out_idx = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    out_score = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "bank": [n, d], "Q": nq, "k": k,
           "calls": args.calls, "warmup": args.warmup, "repeats": args.repeats}
    res["plain_host_us"], res["plain_search_us"] = measure(lambda: sb.search_device(q, k, out_idx=out_idx, out_score=out_score),
                                                           args.calls, args.warmup, args.repeats)
    res["grouped_host_us"], res["grouped_search_us"] = measure(lambda: sb.search_grouped_device(q, 3, 2, groups, 10),
                                                               args.calls, args.warmup, args.repeats)
    sb.build_index(16)
    res["ivf_host_us"], res["ivf_search_us"] = measure(lambda: sb.search_ivf_device(q, k, 4), args.calls, args.warmup, args.repeats)
    sb.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
