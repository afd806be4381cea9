"""Cost of keeping a searched collection up to date: "insert one row, then one search" through MilvusClient on a 100k x 768 COSINE
bank, warm, median of nine runs ("A bank that changes").  It uses only insert / search, so it also runs on a
commit where insert still drops the resident bank: point it at that checkout's package to compare.

usage: python scripts/knn_insert_search.py [dir that holds the astts package] [label]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "autostyle-tts_amd"))
import astts  # noqa: E402,F401  (first: sets the hardware-queue count before HIP initialises)
import torch  # noqa: E402
from astts.compat.pymilvus import MilvusClient  # noqa: E402

N, D, RUNS, WARM = 100_000, 768, 9, 3
rng = np.random.default_rng(0)
vecs = rng.standard_normal((N + RUNS + WARM, D)).astype(np.float16).astype(np.float32)      # fp16-exact, as the shipped bank
c = MilvusClient("unused.db", persist=False)
c.create_collection("bank", dimension=D, metric_type="COSINE")
c.insert("bank", [{"id": i, "vector": vecs[i]} for i in range(N)])
c.search("bank", data=[vecs[123] + 0.1], limit=3)               # the bank goes to HBM here
torch.cuda.synchronize()
times = []
for r in range(WARM + RUNS):
    row = {"id": N + r, "vector": vecs[N + r]}
    t0 = time.perf_counter()
    c.insert("bank", [row])
    hits = c.search("bank", data=[vecs[N + r]], limit=3)        # (returns host lists: the search has finished)
    dt = time.perf_counter() - t0
    assert hits[0][0]["id"] == N + r, hits[0][:2]               # the row just inserted is its own nearest neighbour
    if r >= WARM:
        times.append(dt * 1e3)
print(json.dumps({"label": sys.argv[2] if len(sys.argv) > 2 else "this tree", "n": N, "d": D, "runs": RUNS,
                  "median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}))
