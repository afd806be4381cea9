"""Generates tests/golden/qwen3_tiny.npz and qwen3_tiny_train.npz: inputs and expected outputs of the Qwen3 track of the LLM, produced on
the CPU in fp32 by transformers' Qwen3ForCausalLM on the seeded weights of make_llama_weights(LlamaShape.qwen3_tiny()) and of
qwen3_tiny_untied() (the head of Qwen3-8B and up).  No real Qwen3 checkpoint exists where this runs, and neither peft nor bitsandbytes
is installed: the LoRA branch of the training record is added by its explicit formula ``W x + (lora_alpha / r) * B (A x)`` (as
tests/golden/make_qwen2_fixtures.py does), and nothing here is quantised.

Recorded: a right-padded batch of 130, 64 and 5 tokens; of every row the last-layer hidden states of its real positions, the mean-pooled
embedding, the last position's logits, an 8-token greedy continuation and the token log-probabilities; and, with a seeded LoRA (r = 8,
non-zero B) on all seven projections, the mean next-token loss and every dA, dB (tied shape).  The untied shape draws lm_head before the
norm weights, so all its weights behind the head differ: its record is stored under the prefix ``untied.`` with the hidden states of the
5-token row only (the embedding, a mean over every position, stands for the rest), which keeps the file below the Qwen2 one.  Only seeds
travel: weights, batch and LoRA regenerate from them (tests/qwen3_ref.py).  Forward pass in full fp32 in qwen3_tiny.npz; loss and
gradients in qwen3_tiny_train.npz, the gradients as fp32 with the low 8 mantissa bits cleared (relative error 2^-16).

The batch seed (qwen3_ref.BATCH_SEED) is the one of 22 .. 39 whose greedy continuations have the largest smallest top-2 logit margin over
BOTH shapes in the fp32 restatement (``--scan`` prints the table): a continuation that fp16 rounding cannot change.

The script then runs the restatement of tests/qwen3_ref.py against what it wrote: in fp32 (must reproduce the file) and with fp16
rounding at the points where the GPU path holds fp16.  The printed errors of the second run are the "emulated" column of DESIGN.md
section 2 "Qwen3"; every GPU bound of tests/test_qwen3_gpu.py is 4 x its emulated error.

Run in the BUILD container only (python tests/golden/make_qwen3_fixtures.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.join(ROOT, "tests")]

import qwen3_ref as ref  # noqa: E402
from astts.llm.config import LlamaShape  # noqa: E402
from astts.llm.peft import PROJ  # noqa: E402
from astts.llm.weights import make_llama_weights  # noqa: E402
from make_qwen2_fixtures import LoraLinear, trunc24  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "qwen3_tiny.npz")
FWD = ("hidden", "embedding", "logits_last", "logprobs")


def scan():
    for seed in range(22, 40):
        worst = []
        for name in ref.SHAPES:
            cfg = getattr(LlamaShape, name)()
            sd = make_llama_weights(cfg, ref.SEED)
            ids, lens = ref.make_batch(cfg, ref.LENS, seed)
            lin = ref.fp_linear(sd, cfg)
            worst.append(min(min(ref.greedy(sd, cfg, lin, ids[i, :int(n)].tolist(), ref.GEN_LEN)[1]) for i, n in enumerate(lens)))
        print(f"batch seed {seed}: smallest top-2 margin {min(worst):.4f} (tied {worst[0]:.4f}, untied {worst[1]:.4f})", flush=True)


def forward_record(model, cfg, ids, lens, mask) -> dict:
    out = {}
    with torch.no_grad():
        o = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        hs = o.hidden_states[-1]
        out["hidden"] = torch.cat([hs[i, :int(n)] for i, n in enumerate(lens)]).numpy()
        out["embedding"] = torch.stack([hs[i, :int(n)].mean(0) for i, n in enumerate(lens)]).numpy()
        out["logits_last"] = torch.stack([o.logits[i, int(n) - 1] for i, n in enumerate(lens)]).numpy()
        lp = torch.log_softmax(o.logits[:, :-1].double(), -1).gather(-1, ids[:, 1:, None])[..., 0]
        out["logprobs"] = torch.where(mask[:, 1:].bool(), lp, torch.zeros_like(lp)).float().numpy()
        gen, margins = [], []
        for i, n in enumerate(lens):                       # one prompt per call: no padding inside generate
            prompt = ids[i:i + 1, :int(n)]
            g = model.generate(prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=ref.GEN_LEN, do_sample=False,
                               eos_token_id=None, pad_token_id=cfg.eos_token_id, output_scores=True, return_dict_in_generate=True)
            gen.append(g.sequences[0, int(n):].numpy())
            margins.append([float(t[0] - t[1]) for t in (torch.topk(s[0], 2).values for s in g.scores)])
        out["greedy"] = np.stack(gen)
        out["greedy_margins"] = np.asarray(margins, np.float32)       # top-1 minus top-2 logit of every generated token
    return out


def load_model(cfg, sd):
    from transformers import Qwen3ForCausalLM

    hf_cfg = cfg.hf_config()
    hf_cfg._attn_implementation = "eager"
    model = Qwen3ForCausalLM(hf_cfg).eval().float()
    res = model.load_state_dict(sd if not cfg.tie_embeddings else {**sd, "lm_head.weight": sd["model.embed_tokens.weight"]}, strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def main():
    torch.manual_seed(0)
    out = {"seed": np.int64(ref.SEED), "batch_seed": np.int64(ref.BATCH_SEED), "lora_seed": np.int64(ref.LORA_SEED), "r": np.int64(ref.R),
           "lora_alpha": np.float64(ref.ALPHA)}
    train = {}
    for name in ref.SHAPES:
        cfg = getattr(LlamaShape, name)()
        sd = make_llama_weights(cfg, ref.SEED)
        model = load_model(cfg, sd)
        ids, lens = ref.make_batch(cfg, ref.LENS, ref.BATCH_SEED)
        mask = (torch.arange(ids.shape[1])[None, :] < lens[:, None]).long()
        rec = forward_record(model, cfg, ids, lens, mask)
        if cfg.tie_embeddings:
            out.update(ids=ids.numpy(), lens=lens.numpy(), **rec)
        else:
            rec["hidden"] = rec["hidden"][-int(lens[-1]):]                # the last (5-token) row only
            out.update({f"untied.{k}": v for k, v in rec.items()})
            continue
        # training: the LoRA branch by its formula on all seven projections, A and B the only trainable parameters
        lora = ref.make_lora(cfg, ref.R, ref.LORA_SEED)
        mods = {}
        for i, layer in enumerate(model.model.layers):
            for p, full in PROJ.items():
                parent = getattr(layer, full.split(".")[0])
                m = LoraLinear(getattr(parent, p), *lora[(i, p)], ref.ALPHA / ref.R)
                setattr(parent, p, m)
                mods[(i, p)] = m
        labels = torch.where(mask.bool(), ids, torch.full_like(ids, -100))
        model.train()
        loss = model(input_ids=ids, attention_mask=mask, labels=labels).loss
        loss.backward()
        train["loss"] = np.float64(float(loss.detach()))
        for (i, p), m in mods.items():
            train[f"grad.{i}.{p}.A"], train[f"grad.{i}.{p}.B"] = trunc24(m.lora_A.grad), trunc24(m.lora_B.grad)
    np.savez_compressed(PATH, **out)
    np.savez_compressed(PATH.replace(".npz", "_train.npz"), **train)
    print("->", PATH, os.path.getsize(PATH) // 1024, "KB and", os.path.getsize(PATH.replace(".npz", "_train.npz")) // 1024, "KB; loss",
          float(train["loss"]), "; greedy", out["greedy"].tolist(), out["untied.greedy"].tolist(), "; smallest top-2 margins",
          float(out["greedy_margins"].min()), float(out["untied.greedy_margins"].min()))
    report()


def record_of(fx, cfg) -> dict:
    """The forward record of one shape out of the loaded file."""
    pre = "" if cfg.tie_embeddings else "untied."
    return {k: fx[pre + k] for k in FWD + ("greedy",)}


def hidden_rows(got_hidden: torch.Tensor, cfg, lens) -> torch.Tensor:
    """The rows of ``outputs(...)["hidden"]`` that the file holds for this shape."""
    return got_hidden if cfg.tie_embeddings else got_hidden[-int(lens[-1]):]


def report():
    """The restatement against the file: fp32 (reproduces it) and fp16-rounded (the emulated error of every GPU bound)."""
    fx = {**np.load(PATH), **np.load(PATH.replace(".npz", "_train.npz"))}
    ids, lens = torch.from_numpy(fx["ids"]), torch.from_numpy(fx["lens"])
    for name in ref.SHAPES:
        cfg = getattr(LlamaShape, name)()
        sd = make_llama_weights(cfg, int(fx["seed"]))
        want = record_of(fx, cfg)
        for h16 in (False, True):
            lin = ref.fp_linear(sd, cfg, h16=h16)
            got = ref.outputs(sd, cfg, lin, ids, lens, h16=h16)
            got["hidden"] = hidden_rows(got["hidden"], cfg, lens)
            errs = {k: ref.rel_l2(got[k], want[k]) for k in FWD}
            at = ""
            if cfg.tie_embeddings:
                lora = ref.make_lora(cfg, int(fx["r"]), int(fx["lora_seed"]))
                loss, grads = ref.loss_and_grads(sd, cfg, lora, float(fx["lora_alpha"]) / int(fx["r"]), ids, lens, h16=h16)
                errs["loss"] = abs(loss - float(fx["loss"])) / float(fx["loss"])
                worst = max(((ref.rel_l2(g, fx[f"grad.{i}.{p}.{h}"]), (i, p, h)) for (i, p, h), g in grads.items()))
                errs["grad (worst)"], at = worst[0], f" at {worst[1]}"
            toks = [ref.greedy(sd, cfg, lin, ids[i, :int(n)].tolist(), ref.GEN_LEN, h16=h16)[0] for i, n in enumerate(lens)]
            off = ref.outputs(sd, cfg, lin, ids, lens, h16=h16, qk_norm=False)
            off["hidden"] = hidden_rows(off["hidden"], cfg, lens)
            print(f"{name}: " + ("fp16-rounded" if h16 else "fp32") + " restatement vs the fixture (relative L2): " +
                  ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + at + f"; greedy equal: {toks == want['greedy'].tolist()}; "
                  "without the norm: " + ", ".join(f"{k} {ref.rel_l2(off[k], want[k]):.3e}" for k in FWD), flush=True)


if __name__ == "__main__":
    scan() if "--scan" in sys.argv[1:] else report() if "--report" in sys.argv[1:] else main()
