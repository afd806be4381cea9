"""Generates tests/golden/scoring_kats.npz: teacher-forced log-probabilities of the embedder's LLM as transformers'
LlamaForCausalLM computes them in fp32 on the CPU, on the seeded weights of astts.llm.weights.make_llama_weights at
LlamaShape.tiny() (seed 7) and LlamaShape.wide() (seed 8) -- the models tests/golden/make_llama_fixtures.py uses.
Run in the build container only (python tests/golden/make_scoring_fixtures.py); the .npz is data.  Per model <m>:

  <m>/ids, <m>/lens          a right-padded batch of random sequences
  <m>/token_logprobs         float64 [B, T - 1]: log P(token t + 1 | tokens <= t) at every real position, 0 on the padding
  <m>/logit_absmax           the largest |logit| at a real position of that batch: the scale of the tests' tolerance
  <m>/labels, <m>/label_lens six multi-token "labels" (random ids, 2-3 tokens)
  <m>/prompts, <m>/prompt_lens   N_PROMPTS prompts
  <m>/label_sums             float64 [N_PROMPTS, 6]: summed log-probability of each label's tokens after each prompt
  <m>/label_token_logprobs   float64 [N_PROMPTS, 6, 3]: the same per token (0 beyond a label's length)

MARGIN RULE.  The GPU test holds a token's log-probability to TOL = 2 * 1e-2 * logit_absmax (twice the bound tests/test_llm_gpu.py
puts on these models' logits), so a label's sum may move by len(label) * TOL and the comparison of two labels by the sum of both.  A
prompt is CLEAR when its best label beats every other label by more than (len(best) + len(other)) * TOL.  Prompts are drawn from one
seeded stream and taken in order; an unclear one is kept only while fewer than MAX_UNCLEAR (= 10 % of N_PROMPTS) are in, so at least
90 % of the stored prompts are clear.  The script asserts it, and prints how many candidates it drew.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd")]

from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

from astts.llm.config import LlamaShape  # noqa: E402
from astts.llm.weights import make_llama_weights  # noqa: E402

N_PROMPTS = 40
MAX_UNCLEAR = N_PROMPTS // 10
MODEL_REL = 2 * 1e-2
LABEL_LENS = (2, 3, 2, 3, 2, 2)


def _model(cfg, seed):
    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig(**cfg.hf_kwargs())).eval().float()
    missing = model.load_state_dict(make_llama_weights(cfg, seed), strict=False, assign=True)
    model.tie_weights()
    assert set(missing.missing_keys) <= {"lm_head.weight"} and not missing.unexpected_keys, missing
    return model


def _logprobs(model, ids, lens):
    """float64 [B, T - 1] and the largest |logit| at a real position."""
    mask = (torch.arange(ids.shape[1])[None, :] < lens[:, None]).to(torch.int64)
    with torch.no_grad():
        lg = model(input_ids=ids, attention_mask=mask).logits.double()
    lp = torch.log_softmax(lg[:, :-1], dim=-1).gather(2, ids[:, 1:, None])[..., 0]
    real = torch.arange(1, ids.shape[1])[None, :] < lens[:, None]
    return torch.where(real, lp, torch.zeros_like(lp)), float(lg[mask.bool()].abs().max())


def run(name, cfg, seed, seq_lens, out):
    model = _model(cfg, seed)
    g = torch.Generator().manual_seed(seed + 100)

    def draw(n, bos=True):
        row = torch.randint(3, cfg.vocab, (n,), generator=g)
        if bos:
            row[0] = cfg.bos_token_id
        return row

    ids = torch.zeros((len(seq_lens), max(seq_lens)), dtype=torch.int64)
    for i, n in enumerate(seq_lens):
        ids[i, :n] = draw(n)
    lens = torch.tensor(seq_lens)
    lp, amax = _logprobs(model, ids, lens)
    labels = torch.zeros((6, max(LABEL_LENS)), dtype=torch.int64)
    for i, n in enumerate(LABEL_LENS):
        labels[i, :n] = draw(n, bos=False)
    tol = MODEL_REL * amax                 # the scale is fixed by the sequences above, before any prompt is looked at
    keep, unclear, drawn = [], 0, 0
    while len(keep) < N_PROMPTS and drawn < 20 * N_PROMPTS:
        drawn += 1
        p = draw(int(torch.randint(4, 13, (1,), generator=g)))
        b = torch.zeros((6, len(p) + labels.shape[1]), dtype=torch.int64)
        bl = torch.tensor([len(p) + n for n in LABEL_LENS])
        for i, n in enumerate(LABEL_LENS):
            b[i, :len(p)] = p
            b[i, len(p):len(p) + n] = labels[i, :n]
        l6, _ = _logprobs(model, b, bl)
        tok = torch.zeros((6, labels.shape[1]), dtype=torch.float64)
        for i, n in enumerate(LABEL_LENS):
            tok[i, :n] = l6[i, len(p) - 1:len(p) - 1 + n]
        s = tok.sum(1)
        best = int(s.argmax())
        clear = all(s[best] - s[j] > (LABEL_LENS[best] + LABEL_LENS[j]) * tol for j in range(6) if j != best)
        if not clear:
            if unclear >= MAX_UNCLEAR:
                continue
            unclear += 1
        keep.append((p, tok))
    assert len(keep) == N_PROMPTS and unclear <= MAX_UNCLEAR, (len(keep), unclear)
    pl = [len(p) for p, _ in keep]
    prompts = torch.zeros((N_PROMPTS, max(pl)), dtype=torch.int64)
    for i, (p, _) in enumerate(keep):
        prompts[i, :len(p)] = p
    toks = torch.stack([t for _, t in keep])
    out.update({f"{name}/seed": np.int64(seed), f"{name}/ids": ids.numpy(), f"{name}/lens": lens.numpy(),
                f"{name}/token_logprobs": lp.numpy(), f"{name}/logit_absmax": np.float64(amax),
                f"{name}/labels": labels.numpy(), f"{name}/label_lens": np.asarray(LABEL_LENS, np.int64),
                f"{name}/prompts": prompts.numpy(), f"{name}/prompt_lens": np.asarray(pl, np.int64),
                f"{name}/label_sums": toks.sum(2).numpy(), f"{name}/label_token_logprobs": toks.numpy()})
    print(f"{name}: max|logit| {amax:.3f}, token tolerance {tol:.3f}; {N_PROMPTS} prompts kept of {drawn} drawn, {unclear} unclear; "
          f"label choices {np.bincount(toks.sum(2).argmax(1).numpy(), minlength=6).tolist()}")


if __name__ == "__main__":
    out = {}
    run("tiny", LlamaShape.tiny(), 7, [23, 5, 64, 130], out)
    run("wide", LlamaShape.wide(), 8, [40, 17, 9], out)
    path = os.path.join(ROOT, "tests", "golden", "scoring_kats.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path) // 1024, "KB")
