"""The definition of astts_op_sample_topk_topp (include/astts.h) in numpy float64: temperature -> top-k -> top-p -> inverse-CDF draw
on an injected uniform.  TEST INFRASTRUCTURE ONLY; tests/test_llm_sampling_cpu.py holds it to transformers' TemperatureLogitsWarper ->
TopKLogitsWarper -> TopPLogitsWarper (kept set equal, probabilities within 1e-6).

Per row: candidates = the top_k largest logits under (logit descending, id ascending) on the raw fp32 logits; s = logit / temperature
in fp32; p = softmax(s) over the candidates (float64 from here on); nucleus = the candidates whose exclusive prefix sum of p is
< top_p; q = p / sum(p over the nucleus); token = first nucleus entry whose inclusive prefix sum of q exceeds u (else the last).

Three margins say how far the inputs are from a decision an fp32 implementation could take the other way:
    kth      logit gap between the last candidate and the best entry left out (inf when every entry is a candidate);
    nucleus  min over the candidates of |exclusive prefix - top_p|;
    draw     min over the nucleus entries but the last of |cdf - u| (the last entry's cdf is 1 and decides nothing: it is taken when
             no earlier entry is).
The GPU tests assert every margin >= MARGIN = 1e-5: about 10x the fp32 error of a 50-term sum and of one division."""
from typing import NamedTuple

import numpy as np

MARGIN = 1e-5


class Sampled(NamedTuple):
    ids: np.ndarray       # nucleus token ids, in candidate order
    q: np.ndarray         # float64 renormalised probabilities of the nucleus
    token: int
    kth: float
    nucleus: float
    draw: float

    @property
    def margin(self) -> float:
        return min(self.kth, self.nucleus, self.draw)


def sample_row(logits, u: float, temperature: float, top_k: int, top_p: float) -> Sampled:
    x = np.ascontiguousarray(logits, dtype=np.float32)
    assert x.ndim == 1 and temperature > 0 and 0 < top_p <= 1 and 1 <= top_k <= 1024 and 0 <= u < 1
    kk = min(int(top_k), x.shape[0])
    order = np.lexsort((np.arange(x.shape[0]), -x.astype(np.float64)))        # logit descending, id ascending
    cand = order[:kk]
    kth = float(x[cand[-1]]) - float(x[order[kk]]) if kk < x.shape[0] else float("inf")
    s = (x[cand] / np.float32(temperature)).astype(np.float64)                # the division in fp32, as the definition says
    e = np.exp(s - s[0])
    p = e / e.sum()
    incl = np.cumsum(p)
    excl = incl - p
    excl[0] = 0.0
    n = int(np.argmax(excl >= top_p)) if bool((excl >= top_p).any()) else kk   # first candidate outside the nucleus
    n = max(n, 1)
    q = p[:n] / p[:n].sum()
    cdf = np.cumsum(q)
    over = np.nonzero(cdf > u)[0]
    pick = int(over[0]) if len(over) else n - 1
    draw = float(np.abs(cdf[:-1] - u).min()) if n > 1 else float("inf")
    return Sampled(cand[:n].astype(np.int64), q, int(cand[pick]), kth, float(np.abs(excl - top_p).min()), draw)


def sample_rows(logits, uniforms, temperature: float, top_k: int, top_p: float):
    """[rows, vocab], [rows] -> (tokens int64 [rows], smallest margin over the rows, list of Sampled)."""
    rows = [sample_row(r, float(u), temperature, top_k, top_p) for r, u in zip(np.asarray(logits), np.asarray(uniforms))]
    return np.array([r.token for r in rows], np.int64), min(r.margin for r in rows), rows


def uniform_for(logits, token: int, temperature: float, top_k: int, top_p: float) -> float:
    """A uniform that makes the definition draw ``token`` (the middle of its cdf interval) -- to force a continuation."""
    r = sample_row(logits, 0.0, temperature, top_k, top_p)
    where = np.nonzero(r.ids == token)[0]
    assert len(where), f"token {token} is outside the nucleus {r.ids.tolist()}"
    cdf = np.concatenate([[0.0], np.cumsum(r.q)])
    return float(np.float32(0.5 * (cdf[where[0]] + cdf[where[0] + 1])))


def normal_rows(seed: int, rows: int, vocab: int, scale: float = 1.0, ld=None) -> np.ndarray:
    """The test logits: numpy's default_rng(seed) standard normals times ``scale``, fp32 [rows, ld or vocab]."""
    return (np.random.default_rng(seed).standard_normal((rows, ld or vocab)) * scale).astype(np.float32)


# The shared test inputs: (name, seed, rows, vocab, ld, scales cycled over the rows, temperature, top_k, top_p).  Seeds are chosen so that
# every margin of every row is >= MARGIN (tests/golden/make_sampling_fixtures.py refuses to write a fixture otherwise).
CASES = [
    ("wide64", 211, 64, 128256, 128256, (1.0, 2.0, 4.0, 8.0), 0.7, 50, 0.9),
    ("wide_k1", 12, 4, 128256, 128256, (1.0, 4.0), 0.7, 1, 0.9),
    ("wide_k1024_p1", 13, 2, 128256, 128260, (1.0, 2.0), 1.0, 1024, 1.0),
    ("wide_k1024_odd_ld", 814, 2, 128256, 128257, (1.0,), 0.7, 1024, 0.9),
    ("wide_p05", 15, 4, 128256, 128259, (1.0, 2.0), 1.0, 50, 0.5),
    ("v7", 16, 8, 7, 9, (1.0, 3.0), 0.7, 50, 0.9),
    ("v7_k1", 17, 8, 7, 7, (1.0,), 1.0, 1, 0.5),
    ("v1000_p1", 18, 8, 1000, 1000, (1.0, 2.0), 1.0, 50, 1.0),
    ("v1000_k1024", 119, 2, 1000, 1003, (1.0,), 0.7, 1024, 0.9),
    ("v4097", 20, 8, 4097, 4100, (1.0, 2.0), 0.7, 50, 0.5),
    ("v4097_k1024_p1", 5521, 2, 4097, 4097, (1.0,), 1.0, 1024, 1.0),
]


def case_inputs(case):
    """-> (logits fp32 [rows, ld] (columns >= vocab are filler the operator must not read into its answer), uniforms fp32 [rows])."""
    name, seed, rows, vocab, ld, scales, temperature, top_k, top_p = case
    x = normal_rows(seed, rows, vocab, 1.0, ld)
    x *= np.array([scales[r % len(scales)] for r in range(rows)], np.float32)[:, None]
    x[:, vocab:] = 1.0e4                                       # larger than any logit: reading past vocab would show
    u = np.random.default_rng(seed + 1000).random(rows).astype(np.float32)
    return x, np.minimum(u, np.float32(1.0 - 2.0 ** -24))


def case_answers(case):
    x, u = case_inputs(case)
    return sample_rows(x[:, :case[3]], u, case[6], case[7], case[8])
