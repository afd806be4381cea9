"""Weighted-F1 evaluation of the emotion label the LLM gives, on the GPU engine: what the reference's src/evaluate_base_model.py does
(and the evaluation loop of src/ft_llm.py:88-157 when ``--model_path`` is a PEFT adapter directory), as one command.

    python -m astts.cli.evaluate_erc --model_path <llama dir or adapter dir> --data_folder ./data/ [--method generate|score|both]
                                     [--save_details --details_output_path out.json] [--limit N]
    python -m torch.distributed.run --nproc-per-node 8 -m astts.cli.evaluate_erc ...     (rows sharded by rank, gathered on rank 0)

Data: ``{data_folder}/{data_name}.{split}.{kshot}shot_w{window}_{prompting_type}.jsonl`` (evaluate_base_model.py:95-98; the script
evaluates the third, "test", entry of its list: ``--split`` defaults to it), or ``--data_file``.  Each row is ``{"messages": [system, user, ..., assistant]}``;
the last message's content is the gold label.

Prompt: ``messages[:-1]`` through the chat template with the generation prompt added -- ``tokenizer.apply_chat_template`` when the
loaded tokenizer carries a template, otherwise ``chatml_prompt``: a RESTATEMENT of the ChatML template that trl's
``setup_chat_format`` installs in the reference (trl is not a dependency here, so it is restated, not called):
``<|im_start|>{role}\\n{content}<|im_end|>\\n`` per message, then ``<|im_start|>assistant\\n``.  The prompt is tokenised and truncated
to ``--max_length`` (512) tokens from the RIGHT, as the reference's ``tokenizer(..., truncation=True, max_length=512)`` does: that cuts
the TAIL of a long prompt -- the shipped rows average ~3 500 characters, so most lose the question and the generation prompt.  It is
the reference's behaviour and stays the default; ``--truncation_side left`` keeps the end of the prompt instead.  Nothing is padded to
``max_length``: the engine masks.

Methods.  ``generate`` (default, the reference's): ``generate_greedy_batch(max_new_tokens=10)``, decoded with special tokens kept,
``post_process`` = ``split("assistant\\n")[-1].split("<|im_end|>")[0]``.  ``score``: ``LlamaEmbedder.classify`` over the label set
met in the data (the label with the largest summed log-probability after the prompt), plus the mean negative log-likelihood of the
gold label.  ``both``: both, and the share of rows on which they agree.  The gold label goes through encode (at most 10 tokens) ->
decode without special tokens, as ``split_label`` + ``batch_decode`` do.

``--re_gen_data`` (data preparation, reformat_data_ft_llm.py) is not part of this package and is refused.
"""
import argparse
import json
import sys

from astts import parallel
from astts.metrics import weighted_f1


def chatml_prompt(messages, add_generation_prompt: bool = True) -> str:
    """RESTATEMENT of the ChatML chat template (trl ``setup_chat_format``, format "chatml")."""
    text = "".join(f"<|im_start|>{m['role']}\n{m['content']}<|im_end|>\n" for m in messages)
    return text + "<|im_start|>assistant\n" if add_generation_prompt else text


def build_prompt(tokenizer, messages) -> str:
    if getattr(tokenizer, "chat_template", None) and hasattr(tokenizer, "apply_chat_template"):
        return tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    return chatml_prompt(messages)


def post_process(str_out: str) -> str:
    """evaluate_base_model.py:38-44."""
    try:
        return str_out.split("assistant\n")[-1].split("<|im_end|>")[0]
    except Exception:  # noqa: BLE001
        return "error"


def _takes(fn, name: str) -> bool:
    import inspect
    try:
        ps = inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return True
    return name in ps or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in ps.values())


def _decode(tokenizer, ids, skip_special: bool) -> str:
    if _takes(tokenizer.decode, "skip_special_tokens"):
        return tokenizer.decode(list(ids), skip_special_tokens=skip_special)
    return tokenizer.decode(list(ids))


def gold_label(tokenizer, content: str) -> str:
    """split_label (encode, at most 10 tokens) then batch_decode(skip_special_tokens=True): the string the F1 compares with."""
    return _decode(tokenizer, list(tokenizer.encode(content))[:10], True)


def encode_prompt(tokenizer, text: str, max_length: int, side: str = "right"):
    ids = [int(i) for i in tokenizer.encode(text)]
    if len(ids) > max_length:
        ids = ids[:max_length] if side == "right" else ids[-max_length:]
    return ids


def data_path(args) -> str:
    if getattr(args, "data_file", None):
        return args.data_file
    return f"{args.data_folder}/{args.data_name}.{args.split}.{args.kshot}shot_w{args.window}_{args.prompting_type}.jsonl"


def read_rows(path: str, limit=None):
    rows = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            if line.strip():
                rows.append(json.loads(line))
    return rows[:limit] if limit else rows


def evaluate_rows(rows, embedder, label_set, method: str, batch: int, max_length: int, side: str):
    """This rank's rows -> a list of per-row records (plain Python: they cross ranks)."""
    tok = embedder.tokenizer
    prompts = [encode_prompt(tok, build_prompt(tok, r["messages"][:-1]), max_length, side) for r in rows]
    gold_raw = [r["messages"][-1]["content"] for r in rows]
    recs = [{"label": gold_label(tok, g)} for g in gold_raw]
    step = max(int(batch), 1)
    if method in ("generate", "both"):
        for c0 in range(0, len(rows), step):
            outs = embedder.generate_greedy_batch(prompts[c0:c0 + step], max_new_tokens=10)
            for rec, o in zip(recs[c0:c0 + step], outs):
                rec["raw"] = _decode(tok, o, False)
                rec["pred"] = post_process(rec["raw"])
    if method in ("score", "both") and rows:
        kw = {"add_special_tokens": False} if _takes(tok.encode, "add_special_tokens") else {}
        lab_ids = [[int(i) for i in tok.encode(l, **kw)] for l in label_set]
        choice, sums, _ = embedder.classify(prompts, lab_ids, batch=step * max(len(label_set), 1))
        for rec, g, c, s in zip(recs, gold_raw, choice, sums):
            rec["pred_score"] = label_set[int(c)]
            rec["sums"] = [float(v) for v in s]
            rec["gold_nll"] = -float(s[label_set.index(g)])
    return recs


def main(args, embedder=None):
    if getattr(args, "re_gen_data", False):
        raise SystemExit("evaluate_erc: --re_gen_data is not supported: regenerating the prompt files (reformat_data_ft_llm.py) is data "
                         "preparation outside this package; produce the .jsonl with the reference and pass --data_folder or --data_file")
    import random

    import numpy as np
    import torch

    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dist, rank, world, local = parallel.init_from_env()
    if dist is not None and dist.get_backend() == "nccl":
        torch.cuda.set_device(local)
    rows = read_rows(data_path(args), args.limit)
    label_set = sorted({r["messages"][-1]["content"] for r in rows})      # from the data, not a constant
    b0, b1, _ = parallel.shard_bounds(len(rows), world, rank)
    with parallel.rank_work(dist, "evaluate_erc: load the model"):
        if embedder is None:
            from astts.cli.search_milvus import load_embedder
            embedder = load_embedder(args.model_path, args.allow_random_init, args.seed, args.base_model_path, args.llm_precision)
    with parallel.rank_work(dist, "evaluate_erc: this rank's rows"):
        recs = evaluate_rows(rows[b0:b1], embedder, label_set, args.method, args.per_device_eval_batch_size, args.max_length,
                             args.truncation_side)
    if dist is not None:
        box = [None] * world
        dist.all_gather_object(box, recs)
        recs = [r for part in box for r in part]
    result = None
    if rank == 0:
        labels = [r["label"] for r in recs]
        result = {}
        if args.method in ("generate", "both"):
            result["f1_weighted"] = weighted_f1(labels, [r["pred"] for r in recs])
            result["detail_pred"] = [[r["pred"], r["label"], r["raw"]] for r in recs]
        if args.method in ("score", "both"):
            f1s = weighted_f1(labels, [r["pred_score"] for r in recs])
            nll = sum(r["gold_nll"] for r in recs) / max(len(recs), 1)
            if args.method == "score":
                result["f1_weighted"] = f1s
                result["detail_pred"] = [[r["pred_score"], r["label"], r["pred_score"]] for r in recs]
            else:
                result["f1_weighted_score"] = f1s
                result["agreement"] = sum(1 for r in recs if r["pred"] == r["pred_score"]) / max(len(recs), 1)
            result["gold_label_nll"] = nll
            result["label_set"] = label_set
            result["detail_score"] = [[r["pred_score"], r["label"], r["sums"]] for r in recs]
        print(f"Base Model Test Weighted F1 Score: {result['f1_weighted']}")
        for k in ("f1_weighted_score", "gold_label_nll", "agreement"):
            if k in result:
                print(f"{k}: {result[k]}")
        if args.save_details:
            with open(args.details_output_path, "w") as f:
                json.dump(result, f, indent=2)
            print(f"Detailed predictions saved to {args.details_output_path}")
    if dist is not None:
        dist.barrier()
    return result


def build_parser():
    p = argparse.ArgumentParser(description="Weighted F1 of the LLM's emotion label (src/evaluate_base_model.py) on the GPU engine")
    p.add_argument("--base_model_id", "--model_path", dest="model_path", default="", help="Llama checkpoint directory, or a PEFT LoRA "
                   "adapter directory (then the evaluation of ft_llm.py)")
    p.add_argument("--base_model_path", default=None, help="base checkpoint directory of a LoRA adapter (local only; nothing is fetched)")
    p.add_argument("--llm_precision", choices=("int8", "fp16"), default=None)
    p.add_argument("--allow_random_init", action="store_true", help="run on seeded random Llama weights when model_path does not exist")
    p.add_argument("--data_name", default="iemocap")
    p.add_argument("--data_folder", default="./data/")
    p.add_argument("--data_file", default=None, help="explicit .jsonl path (instead of the composed name)")
    p.add_argument("--output_folder", default="./finetuned_llm/", help="accepted for the reference's command lines; unused (no dataset cache)")
    p.add_argument("--per_device_eval_batch_size", type=int, default=1)
    p.add_argument("--prompting_type", default="spdescV2")
    p.add_argument("--kshot", type=int, default=0)
    p.add_argument("--window", type=int, default=5)
    p.add_argument("--re_gen_data", action="store_true", help="NOT SUPPORTED (refused)")
    p.add_argument("--save_details", action="store_true")
    p.add_argument("--details_output_path", default="base_model_evaluation_details.json")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--method", choices=("generate", "score", "both"), default="generate")
    p.add_argument("--max_length", type=int, default=512)
    p.add_argument("--truncation_side", choices=("right", "left"), default="right", help="right = the reference's (cuts the prompt's "
                   "tail); left keeps the question and the generation prompt")
    p.add_argument("--split", choices=("train", "valid", "test"), default="test", help="which of the three prepared files (the reference "
                   "evaluates test)")
    p.add_argument("--limit", type=int, default=None, help="evaluate the first N rows only")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
    parallel.shutdown()
    sys.exit(0)
