"""python -m astts.cli.ft_llm -- the reference's src/ft_llm.py: LoRA fine-tuning of the emotion-recognition LLM on the prepared
``{data_name}.{split}.{k}shot_w{w}_{type}.jsonl`` files, then (``--do_eval_dev`` / ``--do_eval_test``) its weighted-F1 evaluation.

Flags and defaults are the reference's (src/ft_llm.py:163-184), plus this project's ``--allow_random_init`` and ``--base_model_path``.
Training is astts.llm.train.LoraTrainer: LoRA r = ``--lora_r``, alpha 128 on all seven projections, AdamW, max_grad_norm 0.3,
3 % warm-up, batch 4 x gradient accumulation 4, every row = the chat-formatted conversation including the assistant's answer, loss
on all of its tokens (SFTTrainer's default).

Four parts of the reference's recipe are flags that default to OFF (the defaults train what this command trained before they
existed); the reference's own values are ``--lr_scheduler linear`` (scripts/train_llm.sh and train_llm_cn.sh pass it),
``--lora_dropout 0.05`` (its LoraConfig), ``--neftune_noise_alpha 5`` and ``--packing`` at ``--max_seq_len 1024`` (its SFTTrainer:
trl's ConstantLengthDataset -- conversations concatenated in file order and cut into chunks of exactly max_seq_len tokens that attend
across conversation boundaries).  An ``--lr_scheduler`` this command does not know is an error, not a silently constant rate.
What the reference does and this does not (NF4 base, bf16, gradient checkpointing, embedding resize, multi-GPU): DESIGN.md
section 2.  The base may be a Llama, a Qwen2 (src/ft_llm_cn.py's Qwen2.5: q / k / v biases, plain RoPE) or a Qwen3 checkpoint directory (q / k
norm; no thinking-mode template is applied, prompts go through as text); its
config.json decides.

Evaluation while training, checkpoints, the best adapter and resume (the reference's TrainingArguments, src/ft_llm.py:263-291) are
flags that default to OFF as well; the reference's run is ``--eval_steps 50 --save_steps 50 --eval_delay 200 --save_total_limit 1
--load_best_model_at_end``.  A step s counts every call of the trainer's step(), skipped ones included.  After step s with
``s % eval_steps == 0 and s >= eval_delay`` the ``valid`` file is evaluated as LLMErcTrainer.evaluation_loop does (10 greedy tokens,
weighted F1, batch 32) on ``LoraTrainer.eval_model()``: the live adapter merged on the device into a second fp16 weight image.  After
step s with ``s % save_steps == 0``, ``checkpoint-{s}/`` is written (adapter files, the trainer's state, ``trainer_state.json``) and
the older ones are rotated by transformers' rule (the best is never deleted; a limit of 1 keeps the best and the newest).  The best
checkpoint is the first with a strictly greater ``eval_weighted-f1``.  ``--load_best_model_at_end`` (needs save_steps to be a multiple
of eval_steps) writes that checkpoint's adapter to the output directory and hands it to ``--do_eval_dev`` / ``--do_eval_test``.
With ``--save_steps``, a run whose output directory holds ``checkpoint-*`` CONTINUES from the newest one, bit for bit as if it had
not stopped; another recipe or other training data there is an error, not a fresh start.  ``--total_steps`` pins the schedule's
length when an invocation stops before it (``--max_steps``).

Writes ``{output_folder}/{ft_model_id}``: the peft adapter directory (adapter_config.json, adapter_model.safetensors),
``train_log.jsonl`` (one line per optimizer step: step, loss, grad_norm, lr, loss_scale, skipped) and, when evaluating,
``result_eval_step-{s}.json`` (``{"metrics": {"eval_weighted-f1": f}, "detail_pred": [[pred, label, raw], ...]}``) and
``eval_log.jsonl`` (step, eval_weighted-f1)."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

from astts.cli import evaluate_erc

BATCH, ACCUM, LORA_ALPHA = 4, 4, 128.0


def build_parser():
    p = argparse.ArgumentParser(description="LoRA fine-tuning of the ERC LLM (src/ft_llm.py)")
    p.add_argument("--do_train", action="store_true", default=False, help="fine tuning a LLM model with LoRA")
    p.add_argument("--do_eval_test", action="store_true", default=False, help="eval on test set")
    p.add_argument("--do_eval_dev", action="store_true", default=False, help="eval on dev set")
    p.add_argument("--ft_model_path", type=str, default=None, help="fine-tuned adapter directory (evaluation without training)")
    p.add_argument("--ft_model_id", type=str, default=None, help="name of the adapter directory under --output_folder")
    p.add_argument("--prompting_type", type=str, default="spdescV2")
    p.add_argument("--base_model_id", type=str, default="meta-llama/Llama-2-7b-hf", help="base checkpoint directory (local only)")
    p.add_argument("--base_model_path", type=str, default=None, help="base checkpoint directory when --base_model_id is a hub name")
    p.add_argument("--epoch", type=int, default=None)
    p.add_argument("--max_steps", type=int, default=None)
    p.add_argument("--lr", type=float, default=2e-4)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--kshot", type=int, default=0)
    p.add_argument("--lora_r", type=int, default=32)
    p.add_argument("--window", type=int, default=5)
    p.add_argument("--max_seq_len", type=int, default=None)
    p.add_argument("--data_name", type=str, default="iemocap")
    p.add_argument("--data_folder", type=str, default="./data/")
    p.add_argument("--output_folder", type=str, default="./finetuned_llm/")
    p.add_argument("--allow_random_init", action="store_true", help="train seeded random Llama weights when the base checkpoint does not exist")
    p.add_argument("--loss_scale", type=float, default=1024.0, help="static power-of-two loss scale of the fp16 backward")
    p.add_argument("--limit", type=int, default=None, help="use the first N rows of each file only")
    p.add_argument("--lr_scheduler", type=str, default="constant", choices=["constant", "linear"],
                   help="learning-rate schedule after the 3 %% warm-up (the reference's scripts pass linear)")
    p.add_argument("--lora_dropout", type=float, default=0.0, help="dropout on the input of every LoRA module (the reference: 0.05)")
    p.add_argument("--neftune_noise_alpha", type=float, default=0.0, help="NEFTune noise on the embedding output (the reference: 5)")
    p.add_argument("--packing", action="store_true", default=False,
                   help="concatenate the conversations and train on chunks of exactly --max_seq_len (default 1024) tokens, as the reference does")
    p.add_argument("--eval_steps", type=int, default=0, help="evaluate on the valid file every N steps (0 = never; the reference: 50)")
    p.add_argument("--save_steps", type=int, default=0, help="write checkpoint-{step}/ every N steps and resume from the newest one (0 = never; the reference: 50)")
    p.add_argument("--eval_delay", type=int, default=200, help="no evaluation before this step (the reference: 200)")
    p.add_argument("--save_total_limit", type=int, default=None, help="keep at most N checkpoints, the best always among them (the reference: 1)")
    p.add_argument("--load_best_model_at_end", action="store_true", default=False,
                   help="write the adapter of the checkpoint with the best eval_weighted-f1 instead of the last weights (the reference does)")
    p.add_argument("--total_steps", type=int, default=None,
                   help="length of the learning-rate schedule when it is not the number of steps this invocation trains to (a run cut short "
                        "by --max_steps that a later invocation continues)")
    return p


def split_path(args, split: str) -> str:
    return f"{args.data_folder}/{args.data_name}.{split}.{args.kshot}shot_w{args.window}_{args.prompting_type}.jsonl"


def plan_steps(n_rows: int, epoch, max_steps, batch: int = BATCH, accum: int = ACCUM):
    """-> (optimizer steps, micro-batches per epoch).  ``max_steps`` wins over ``epoch`` when positive, as in TrainingArguments; an
    epoch's last optimizer step may hold fewer micro-batches."""
    micro = max(1, -(-n_rows // batch))
    per_epoch = max(1, -(-micro // accum))
    if max_steps is not None and max_steps > 0:
        return int(max_steps), micro
    return per_epoch * int(epoch if epoch else 3), micro          # TrainingArguments' num_train_epochs default: 3


def encode_rows(rows, tokenizer, max_seq_len):
    """The whole conversation, assistant answer included, chat-formatted (no generation prompt), truncated on the right."""
    out = []
    for r in rows:
        ids = [int(i) for i in tokenizer.encode(evaluate_erc.chatml_prompt(r["messages"], add_generation_prompt=False))]
        out.append(ids[:max_seq_len] if max_seq_len else ids)
    return [ids for ids in out if len(ids) >= 2]


def encode_packed(rows, tokenizer, seq_len: int):
    """``--packing``: every conversation encoded whole (no truncation), then pack_rows."""
    texts = [evaluate_erc.chatml_prompt(r["messages"], add_generation_prompt=False) for r in rows]
    return pack_rows([[int(i) for i in tokenizer.encode(t)] for t in texts], seq_len, [len(t) for t in texts])


PACK_SEQ_LEN, PACK_CHARS_PER_TOKEN, PACK_NUM_SEQUENCES = 1024, 3.6, 1024


def pack_rows(seqs, seq_len: int, texts_chars):
    """trl's ConstantLengthDataset (append_concat_token=False, infinite=False): the encoded rows, in file order and with nothing
    between them, fill buffers of ``seq_len * 3.6 * 1024`` characters of formatted text (``texts_chars[i]`` = the characters of row
    i; a buffer takes rows until it holds that many); each buffer's tokens are cut into chunks of exactly ``seq_len``, and the
    buffer's incomplete tail is dropped."""
    assert len(seqs) == len(texts_chars) and seq_len >= 1
    max_chars = seq_len * PACK_CHARS_PER_TOKEN * PACK_NUM_SEQUENCES
    out, i = [], 0
    while i < len(seqs):
        tokens, chars = [], 0
        while i < len(seqs) and chars < max_chars:
            tokens.extend(seqs[i])
            chars += texts_chars[i]
            i += 1
        out.extend(tokens[o:o + seq_len] for o in range(0, len(tokens) - seq_len + 1, seq_len))
    return out


def collate(seqs):
    import torch
    t = max(len(s) for s in seqs)
    ids = torch.zeros((len(seqs), t), dtype=torch.int64)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s)
    return ids, torch.tensor([len(s) for s in seqs], dtype=torch.int64)


def load_base(args):
    """-> (state dict, shape, tokenizer or None, base directory or None)."""
    from astts.llm.config import LlamaShape
    from astts.llm.peft import shape_from_config
    from astts.llm.weights import load_llama_weights, make_llama_weights
    base = args.base_model_path or args.base_model_id
    if base and os.path.isdir(base):
        from astts.cli.search_milvus import load_tokenizer
        tok = load_tokenizer(base)
        state = load_llama_weights(base)
        return state, shape_from_config(base, int(state["model.embed_tokens.weight"].shape[0])), tok, base
    if not (args.allow_random_init or os.environ.get("ASTTS_ALLOW_RANDOM_INIT") == "1"):
        raise FileNotFoundError(f"no base checkpoint directory at {base!r} (pass --allow_random_init to train seeded random weights)")
    cfg = LlamaShape.tiny() if os.environ.get("ASTTS_TINY_MODEL") == "1" else LlamaShape.llama32_3b()
    print(f"Warning: '{base}' not found; seeded RANDOM-INIT Llama weights at {cfg.hidden}-d (explicitly allowed)")
    return make_llama_weights(cfg, args.seed), cfg, None, None


# ---- evaluation while training, checkpoints, best model, resume: transformers' Trainer rules as the reference's TrainingArguments
# (src/ft_llm.py:263-291) use them.  A step s is the trainer's sched_step after the step: every call of step(), skipped ones included.
EVAL_BATCH, EVAL_MAX_LENGTH = 32, 512
ADAPTER_FILES = ("adapter_config.json", "adapter_model.safetensors")
TRAINER_STATE = "trainer_state.json"


def should_eval(step: int, eval_steps: int, eval_delay: int) -> bool:
    return eval_steps > 0 and step % eval_steps == 0 and step >= eval_delay


def should_save(step: int, save_steps: int) -> bool:
    return save_steps > 0 and step % save_steps == 0


def is_better(metric: float, best) -> bool:
    """Strictly greater (weighted F1: greater is better); a tie keeps the earlier checkpoint."""
    return best is None or metric > best


def checkpoints_to_delete(steps, best_step, limit):
    """transformers' Trainer._rotate_checkpoints on the saved steps: sorted by step, the best moved to just before the newest; a
    limit of 1 becomes 2 while the best is not the newest; what exceeds the limit goes, from the front."""
    order = sorted(int(s) for s in steps)
    if limit is None or limit <= 0 or len(order) <= limit:
        return []
    if best_step is not None and best_step in order:
        i = order.index(best_step)
        for j in range(i, len(order) - 2):
            order[j], order[j + 1] = order[j + 1], order[j]
    if best_step is not None and limit == 1 and order[-1] != best_step:
        limit = 2
    return order[:max(0, len(order) - limit)]


def check_flags(args) -> None:
    for name in ("eval_steps", "save_steps", "eval_delay"):
        if getattr(args, name) < 0:
            raise SystemExit(f"ft_llm: --{name} {getattr(args, name)} is negative")
    if args.load_best_model_at_end:
        if args.eval_steps <= 0 or args.save_steps <= 0 or args.save_steps % args.eval_steps != 0:
            raise SystemExit(f"ft_llm: --load_best_model_at_end needs --save_steps ({args.save_steps}) to be a positive multiple of "
                             f"--eval_steps ({args.eval_steps}): the best evaluation must have a checkpoint")


def data_fingerprint(seqs) -> dict:
    """The number of training sequences and a SHA-256 of their token ids (each sequence: its length, then its ids, as little-endian int64)."""
    import hashlib
    import struct
    h = hashlib.sha256()
    for s in seqs:
        h.update(struct.pack(f"<{len(s) + 1}q", len(s), *s))
    return {"sequences": len(seqs), "sha256": h.hexdigest()}


def data_position_to_json(order, pos: int, rng: random.Random) -> dict:
    v, internal, gauss = rng.getstate()
    return {"order": [int(i) for i in order], "pos": int(pos), "random_state": [v, list(internal), gauss]}


def data_position_from_json(d: dict):
    """-> (order, pos, a random.Random that draws what the saved one would have drawn next)."""
    v, internal, gauss = d["random_state"]
    rng = random.Random()
    rng.setstate((v, tuple(int(i) for i in internal), gauss))
    return [int(i) for i in d["order"]], int(d["pos"]), rng


def checkpoint_steps(out_dir: str):
    out = []
    for name in os.listdir(out_dir) if os.path.isdir(out_dir) else ():
        head, _, num = name.partition("-")
        if head == "checkpoint" and num.isdigit() and os.path.isfile(os.path.join(out_dir, name, TRAINER_STATE)):
            out.append(int(num))
    return sorted(out)


def _trim_log(path: str, last_step: int) -> None:
    """Keep the lines of steps <= last_step: a run killed after its last checkpoint logged steps that the resumed run takes again."""
    if not os.path.exists(path):
        return
    with open(path) as f:
        lines = [ln for ln in f if ln.strip()]
    keep = [ln for ln in lines if int(json.loads(ln)["step"]) <= last_step]
    if len(keep) != len(lines):
        with open(path, "w") as f:
            f.writelines(keep)


def evaluate_in_training(trainer, tokenizer, valid_rows, out_dir: str, step: int) -> float:
    """The reference's LLMErcTrainer.evaluation_loop on the dev rows at the trainer's CURRENT adapter: 10 greedy tokens per row
    through ``trainer.eval_model()``, weighted F1, ``result_eval_step-{step}.json`` in its format."""
    from astts.metrics import weighted_f1
    emb = trainer.eval_model(tokenizer, EVAL_MAX_LENGTH)
    label_set = sorted({r["messages"][-1]["content"] for r in valid_rows})
    recs = evaluate_erc.evaluate_rows(valid_rows, emb, label_set, "generate", EVAL_BATCH, EVAL_MAX_LENGTH, "right")
    f1 = float(weighted_f1([r["label"] for r in recs], [r["pred"] for r in recs]))
    with open(os.path.join(out_dir, f"result_eval_step-{step}.json"), "w") as f:
        json.dump({"metrics": {"eval_weighted-f1": f1}, "detail_pred": [[r["pred"], r["label"], r["raw"]] for r in recs]}, f, indent=1)
    return f1


def train(args, state, cfg, tok, base):
    import shutil

    import torch

    from astts.llm.tokenizer import HashTokenizer
    from astts.llm.train import LoraTrainer
    check_flags(args)
    tokenizer = tok or HashTokenizer(cfg)
    rows = evaluate_erc.read_rows(split_path(args, "train"), args.limit)
    if args.packing:
        seqs = encode_packed(rows, tokenizer, args.max_seq_len or PACK_SEQ_LEN)
    else:
        seqs = encode_rows(rows, tokenizer, args.max_seq_len)
    if not seqs:
        raise SystemExit(f"ft_llm: no usable rows in {split_path(args, 'train')}")
    valid_rows = evaluate_erc.read_rows(split_path(args, "valid"), args.limit) if args.eval_steps > 0 else []
    steps, _ = plan_steps(len(seqs), args.epoch, args.max_steps)
    total_steps = int(args.total_steps) if args.total_steps else steps
    out_dir = os.path.join(args.output_folder, args.ft_model_id or "ft_model")
    os.makedirs(out_dir, exist_ok=True)
    adapter = None
    if args.ft_model_path:
        from astts.llm.peft import load_adapter
        adapter = load_adapter(args.ft_model_path)
    trainer = LoraTrainer(state, cfg, r=args.lora_r, lora_alpha=LORA_ALPHA, seed=args.seed, adapter=adapter, lr=args.lr, total_steps=total_steps,
                          loss_scale=args.loss_scale, base_model_name_or_path=base or args.base_model_id,
                          rope_len=max(len(s) for s in seqs) + 64, lora_dropout=args.lora_dropout, neftune_alpha=args.neftune_noise_alpha,
                          schedule=args.lr_scheduler)
    rng = random.Random(args.seed)
    order, pos = [], 0
    fingerprint = data_fingerprint(seqs)
    best_metric, best_ckpt = None, None
    ckpt_dir = lambda s: os.path.join(out_dir, f"checkpoint-{s}")
    saved = checkpoint_steps(out_dir) if args.save_steps > 0 else []
    train_log, eval_log = os.path.join(out_dir, "train_log.jsonl"), os.path.join(out_dir, "eval_log.jsonl")
    if saved:                                               # resume from the newest checkpoint, as the reference does (src/ft_llm.py:315)
        with open(os.path.join(ckpt_dir(saved[-1]), TRAINER_STATE)) as f:
            ts = json.load(f)
        if ts["data"] != fingerprint:
            raise SystemExit(f"ft_llm: {ckpt_dir(saved[-1])} was trained on other data ({ts['data']} there, {fingerprint} here); "
                             "resume needs the same sequences -- use another --ft_model_id for a fresh run")
        trainer.load_state(ckpt_dir(saved[-1]))             # a recipe that differs: ValueError naming the key
        if trainer.sched_step != ts["global_step"]:
            raise SystemExit(f"ft_llm: {ckpt_dir(saved[-1])} is inconsistent: global_step {ts['global_step']}, trainer at {trainer.sched_step}")
        order, pos, rng = data_position_from_json(ts["data_position"])
        best_metric, best_ckpt = ts["best_metric"], ts["best_model_checkpoint"]
        for path in (train_log, eval_log):
            _trim_log(path, trainer.sched_step)
        print(f"resuming from {ckpt_dir(saved[-1])} (step {trainer.sched_step} of {steps})")
    else:
        for path in (train_log, eval_log) if args.eval_steps > 0 else (train_log,):
            open(path, "w").close()                         # a fresh run starts its logs; a resumed one appends to them
    with open(train_log, "a") as log:
        while trainer.sched_step < steps:
            batches = []
            for _ in range(ACCUM):
                if pos >= len(order):                       # a new epoch: reshuffle
                    order, pos = list(range(len(seqs))), 0
                    rng.shuffle(order)
                    if batches:
                        break                               # the epoch's last optimizer step holds what was left
                batches.append(collate([seqs[i] for i in order[pos:pos + BATCH]]))
                pos += BATCH
            rep = trainer.step(batches)
            rec = {"step": rep.step, "loss": rep.loss, "grad_norm": rep.grad_norm, "lr": rep.lr, "loss_scale": rep.loss_scale, "skipped": rep.skipped}
            log.write(json.dumps(rec) + "\n")
            log.flush()
            print(rec)
            s = trainer.sched_step
            if should_eval(s, args.eval_steps, args.eval_delay):
                f1 = evaluate_in_training(trainer, tokenizer, valid_rows, out_dir, s)
                with open(eval_log, "a") as f:
                    f.write(json.dumps({"step": s, "eval_weighted-f1": f1}) + "\n")
                print({"step": s, "eval_weighted-f1": f1})
                if is_better(f1, best_metric) and should_save(s, args.save_steps):
                    best_metric, best_ckpt = f1, f"checkpoint-{s}"
            if should_save(s, args.save_steps):
                trainer.save_adapter(ckpt_dir(s))
                trainer.save_state(ckpt_dir(s))
                with open(os.path.join(ckpt_dir(s), TRAINER_STATE), "w") as f:
                    json.dump({"global_step": s, "best_metric": best_metric, "best_model_checkpoint": best_ckpt, "data": fingerprint,
                               "data_position": data_position_to_json(order, pos, rng)}, f)
                best_step = int(best_ckpt.split("-")[1]) if best_ckpt else None
                for old in checkpoints_to_delete(checkpoint_steps(out_dir), best_step, args.save_total_limit):
                    shutil.rmtree(ckpt_dir(old))
    if args.load_best_model_at_end and best_ckpt is not None:
        from astts.llm.peft import load_adapter
        best_dir = os.path.join(out_dir, best_ckpt)
        trainer.set_adapter(load_adapter(best_dir))         # --do_eval_dev / --do_eval_test see the best adapter
        for name in ADAPTER_FILES:
            shutil.copyfile(os.path.join(best_dir, name), os.path.join(out_dir, name))
        print(f"best adapter ({best_ckpt}, eval_weighted-f1 {best_metric}) saved to {out_dir}")
    else:
        trainer.save_adapter(out_dir)
        print(f"adapter saved to {out_dir}")
    torch.cuda.synchronize()
    return trainer, out_dir


def evaluate(args, split: str, adapter_dir: str, state, cfg, tok, base):
    """evaluate_erc's evaluation on ``split`` with the adapter: through the adapter directory when there is a base checkpoint
    directory to load it over, else (random-init runs) on the in-memory base with the adapter read back from the directory."""
    ev = evaluate_erc.build_parser().parse_args([])
    ev.data_file, ev.split, ev.seed, ev.limit = split_path(args, split), split, args.seed, args.limit
    ev.output_folder = args.output_folder
    if base is not None:
        ev.model_path, ev.base_model_path = adapter_dir, base
        return evaluate_erc.main(ev)
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.peft import load_adapter
    return evaluate_erc.main(ev, embedder=LlamaEmbedder(state, cfg, tokenizer=tok, lora=load_adapter(adapter_dir)))


def main(args):
    if args.prompting_type == "zeroshot":
        args.kshot = 0
    print(args)
    state, cfg, tok, base = load_base(args)
    adapter_dir = args.ft_model_path or os.path.join(args.output_folder, args.ft_model_id or "ft_model")
    if args.do_train:
        _, adapter_dir = train(args, state, cfg, tok, base)
    results = {}
    if args.do_eval_test:
        results["test"] = evaluate(args, "test", adapter_dir, state, cfg, tok, base)
        print(f"Test result = {results['test'] and results['test'].get('f1_weighted')}")
    if args.do_eval_dev:
        results["valid"] = evaluate(args, "valid", adapter_dir, state, cfg, tok, base)
        print(f"Valid result = {results['valid'] and results['valid'].get('f1_weighted')}")
    return results


if __name__ == "__main__":
    main(build_parser().parse_known_args(sys.argv[1:])[0])        # unknown FLAGS pass, as before; an unknown value of a known flag exits
