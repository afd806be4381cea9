"""Generates tests/golden/bert_tiny.npz: inputs and expected outputs of the BERT-family encoder track, produced on the CPU in fp32 by
transformers' BertModel and XLMRobertaModel (add_pooling_layer=False, eager attention) on the seeded weights of
make_bert_weights(BertShape.bert_tiny() / xlmr_tiny() / m3e_base()).  No real m3e / bge / e5 checkpoint exists where this runs.

Recorded: a right-padded batch of 130, 64, 5 and 2 tokens (token types mixed on the BERT shapes); of the tiny shapes the last hidden
states of the real positions and the mean-pooled and CLS sentence vectors, each raw and L2-normalised; of m3e_base (BERT-base depth) the
four sentence vectors only.  Only seeds travel: weights and batch regenerate from them (tests/bert_ref.py).

The script then runs the restatement of tests/bert_ref.py against what it wrote: in fp32 (must reproduce the file) and with fp16
rounding at the points where the GPU path holds fp16.  The printed errors of the second run are the "emulated" column of DESIGN.md
section 2 "BERT-family encoders"; every GPU bound of tests/test_bert_gpu.py is 4 x its emulated error.  It also prints the error of three
deliberately wrong restatements (positions shifted by one, the token-type table dropped, tanh-GELU): what the fixture can tell apart.

Run in the BUILD container only (python tests/golden/make_bert_fixtures.py; ``--report`` prints the comparison alone)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.join(ROOT, "tests")]

import bert_ref as ref  # noqa: E402
from astts.llm.config import BertShape  # noqa: E402
from astts.llm.weights import make_bert_weights  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "bert_tiny.npz")


def load_model(shape, sd):
    from transformers import BertModel, XLMRobertaModel

    hf_cfg = shape.hf_config()
    hf_cfg._attn_implementation = "eager"
    model = (BertModel if shape.model_type == "bert" else XLMRobertaModel)(hf_cfg, add_pooling_layer=False).eval().float()
    res = model.load_state_dict(sd, strict=False, assign=True)
    assert not res.unexpected_keys and all(k.endswith(("position_ids", "token_type_ids")) for k in res.missing_keys), res
    return model


def record(model, shape, ids, lens, types) -> dict:
    mask = (torch.arange(ids.shape[1])[None, :] < lens[:, None]).long()
    with torch.no_grad():
        h = model(input_ids=ids, attention_mask=mask, token_type_ids=types).last_hidden_state
    return {"hidden": torch.cat([h[i, :int(n)] for i, n in enumerate(lens)]).numpy(), **{k: v.numpy() for k, v in ref.pooled(h, lens).items()}}


def main():
    torch.manual_seed(0)
    out = {"seed": np.int64(ref.SEED), "batch_seed": np.int64(ref.BATCH_SEED), "lens": np.asarray(ref.LENS, np.int64)}
    for name in ref.SHAPES:
        shape = getattr(BertShape, name)()
        ids, lens, types = ref.make_batch(shape)
        rec = record(load_model(shape, make_bert_weights(shape, ref.SEED)), shape, ids, lens, types)
        if name not in ref.TINY:
            del rec["hidden"]
        out.update({f"{name}.{k}": v for k, v in rec.items()}, **{f"{name}.ids": ids.numpy().astype(np.int32), f"{name}.types": types.numpy().astype(np.int8)})
    np.savez_compressed(PATH, **out)
    print("->", PATH, os.path.getsize(PATH) // 1024, "KB")
    report()


def report():
    """The restatement against the file: fp32 (reproduces it), fp16-rounded (the emulated error of every GPU bound) and the three wrong ones."""
    fx = np.load(PATH)
    for name in ref.SHAPES:
        shape = getattr(BertShape, name)()
        sd = make_bert_weights(shape, int(fx["seed"]))
        ids, lens, types = ref.make_batch(shape, tuple(int(n) for n in fx["lens"]), int(fx["batch_seed"]))
        assert np.array_equal(ids.numpy(), fx[f"{name}.ids"]) and np.array_equal(types.numpy(), fx[f"{name}.types"])
        keys = [k for k in ("hidden",) + ref.POOLED if f"{name}.{k}" in fx]
        runs = (("fp32", {}), ("fp16-rounded", {"h16": True}), ("WRONG positions + 1", {"pos_shift": 1}), ("WRONG no token types", {"drop_types": True}),
                ("WRONG tanh-GELU", {"tanh_gelu": True}))
        for label, kw in runs:
            if label.startswith("WRONG") and name not in ref.TINY and "GELU" not in label:
                continue
            got = ref.outputs(sd, shape, ids, lens, types, **kw)
            line = ", ".join(f"{k} {ref.rel_l2(got[k], fx[f'{name}.{k}']):.3e}" for k in keys)
            cos = min(float(torch.nn.functional.cosine_similarity(got["mean"], torch.from_numpy(fx[f"{name}.mean"]), dim=-1).min()), 1.0)
            print(f"{name}: {label} restatement vs the fixture (relative L2): {line}; smallest mean-embedding cosine {cos:.6f}", flush=True)


if __name__ == "__main__":
    report() if "--report" in sys.argv[1:] else main()
