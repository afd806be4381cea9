"""CPU side of LLM scoring: the package's weighted F1 against sklearn, the evaluation command's host logic (prompt, post-processing,
gold labels, arguments, the two-rank run with a stand-in engine), the committed transformers fixture against its own margin rule --
and two SELF-CHECKS OF THE REFERENCE, marked as such below: they hold tests/llm_scoring_ref.py (the float64 statement the GPU tests
compare the kernel with) to torch's cross_entropy / log_softmax and touch nothing of the product."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

import llm_scoring_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("vocab", [512, 515, 4096])
def test_reference_statement_equals_torch(vocab):
    """Self-check of the reference (no product symbol involved)."""
    g = torch.Generator().manual_seed(vocab)
    rows, k, n = 37, 64, vocab + 5                      # a head wider than the vocabulary: the tail must not count
    h = torch.randn(rows, k, generator=g)
    w = torch.randn(n, k, generator=g) * 0.3
    w[vocab:] = 10.0
    t = torch.randint(0, vocab, (rows,), generator=g)
    t[0], t[1], t[2], t[3], t[7] = 0, vocab - 1, -1, vocab - 1, -1
    got = ref.head_logprob(h, w, t, vocab=vocab, chunk=16)
    lg = h.half().double() @ w[:vocab].half().double().T
    ce = torch.nn.functional.cross_entropy(lg, t.clamp(min=0), reduction="none")
    ign = t < 0
    assert torch.equal(got["ignored"], ign) and bool((got["logprob"][ign] == 0).all())
    assert torch.allclose(got["logprob"][~ign], -ce[~ign], rtol=0, atol=1e-12)
    lsm = torch.log_softmax(lg, dim=-1)
    assert torch.allclose(got["logprob"][~ign], lsm[~ign].gather(1, t[~ign, None])[:, 0], rtol=0, atol=1e-12)
    assert torch.allclose(got["lse"], torch.logsumexp(lg, dim=-1), rtol=0, atol=1e-12)
    assert torch.equal(got["argmax"].long(), lg.argmax(1))
    assert got["logit_absmax"] == float(lg.abs().max())


def test_reference_argmax_ties_take_the_lowest_column():
    """Self-check of the reference (no product symbol involved)."""
    lg = torch.zeros(3, 9, dtype=torch.float64)
    lg[0, [4, 7]] = 2.0
    lg[1, [8, 0]] = 1.0
    out = ref.logprob_from_logits(lg, torch.tensor([4, 0, -1]))
    assert out["argmax"].tolist() == [4, 0, 0] and out["top2_gap"].tolist() == [0.0, 0.0, 0.0]


def test_weighted_f1_equals_sklearn():
    from sklearn.metrics import f1_score

    from astts.metrics import weighted_f1

    names = ["happy", "sad", "neutral", "angry", "excited", "frustrated"]
    rng = np.random.default_rng(0)
    labels = [names[i] for i in rng.integers(0, 6, 200)]
    for case in range(4):
        preds = list(labels)
        flip = rng.random(200) < 0.4
        preds = [names[rng.integers(0, 6)] if f else p for f, p in zip(flip, preds)]
        if case == 1:                                         # predictions outside the label set
            preds = ["neutral\n" if i % 7 == 0 else ("error" if i % 11 == 0 else p) for i, p in enumerate(preds)]
        if case == 2:                                         # a class of the label set that is never predicted
            preds = ["sad" if p == "angry" else p for p in preds]
        if case == 3:                                         # a class absent from the labels
            keep = [i for i, l in enumerate(labels) if l != "excited"]
            assert weighted_f1([labels[i] for i in keep], [preds[i] for i in keep]) == pytest.approx(
                f1_score([labels[i] for i in keep], [preds[i] for i in keep], average="weighted"), abs=1e-12)
            continue
        assert weighted_f1(labels, preds) == pytest.approx(f1_score(labels, preds, average="weighted"), abs=1e-12)
    assert weighted_f1(labels, labels) == 1.0
    with pytest.raises(ValueError):
        weighted_f1(["a"], [])


def test_scoring_fixture_keeps_its_margin_rule():
    """tests/golden/scoring_kats.npz: at least 90 % of the stored prompts are clear under the rule its script states."""
    fx = np.load(os.path.join(GOLD, "scoring_kats.npz"))
    for name in ("tiny", "wide"):
        tol = 2 * 1e-2 * float(fx[f"{name}/logit_absmax"])
        s, ll = fx[f"{name}/label_sums"], fx[f"{name}/label_lens"]
        assert s.shape == (40, 6) and np.allclose(s, fx[f"{name}/label_token_logprobs"].sum(2))
        best = s.argmax(1)
        clear = [all(s[i, best[i]] - s[i, j] > (ll[best[i]] + ll[j]) * tol for j in range(6) if j != best[i]) for i in range(40)]
        assert sum(clear) >= 36, (name, sum(clear))
        lp, lens = fx[f"{name}/token_logprobs"], fx[f"{name}/lens"]
        assert lp.shape == (len(lens), fx[f"{name}/ids"].shape[1] - 1) and (lp <= 0).all()
        assert all((lp[i, int(n) - 1:] == 0).all() for i, n in enumerate(lens))


# ---------------------------------------------------------------------------------------------- the evaluation command, host side
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSET = os.path.join(GOLD, "erc_valid_subset.jsonl")
CHATML = ("{% for message in messages %}{{'<|im_start|>' + message['role'] + '\n' + message['content'] + '<|im_end|>' + '\n'}}{% endfor %}"
          "{% if add_generation_prompt %}{{ '<|im_start|>assistant\n' }}{% endif %}")


def _subset():
    from astts.cli.evaluate_erc import read_rows

    rows = read_rows(SUBSET)
    assert len(rows) == 48 and os.path.getsize(SUBSET) < 300 * 1024
    return rows


def test_weighted_f1_on_the_subset_labels_equals_sklearn():
    from sklearn.metrics import f1_score

    from astts.metrics import weighted_f1

    labels = [r["messages"][-1]["content"] for r in _subset()]
    assert sorted(set(labels)) == ["angry", "excited", "frustrated", "happy", "neutral", "sad"]
    rng = np.random.default_rng(1)
    preds = [labels[i] for i in rng.permutation(len(labels))]
    assert weighted_f1(labels, preds) == pytest.approx(f1_score(labels, preds, average="weighted"), abs=1e-12)
    preds[3], preds[10] = "error", "Neutral"
    assert weighted_f1(labels, preds) == pytest.approx(f1_score(labels, preds, average="weighted"), abs=1e-12)


def test_chatml_restatement_equals_apply_chat_template():
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from transformers import PreTrainedTokenizerFast

    from astts.cli.evaluate_erc import build_prompt, chatml_prompt

    tok = PreTrainedTokenizerFast(tokenizer_object=Tokenizer(WordLevel({"a": 0, "[UNK]": 1}, unk_token="[UNK]")))
    tok.chat_template = CHATML
    for r in _subset():
        msgs = r["messages"][:-1]
        want = tok.apply_chat_template(msgs, tokenize=False, add_generation_prompt=True)
        assert chatml_prompt(msgs) == want and build_prompt(tok, msgs) == want
        assert chatml_prompt(r["messages"], add_generation_prompt=False) == tok.apply_chat_template(r["messages"], tokenize=False)


def test_post_process_gold_labels_and_truncation_on_the_subset():
    from llm_scoring_tok import ByteTokenizer

    from astts.cli.evaluate_erc import build_prompt, encode_prompt, gold_label, post_process

    tok = ByteTokenizer()
    lens = []
    for r in _subset():
        label = r["messages"][-1]["content"]
        prompt = build_prompt(tok, r["messages"][:-1])                      # no template on this tokenizer: the restatement
        assert prompt.endswith("<|im_start|>assistant\n")
        raw = "<|begin_of_text|>" + prompt + label + "<|im_end|>\n<|im_start|>"
        assert post_process(raw) == label
        assert post_process(prompt + label) == label and post_process("no marker at all") == "no marker at all"
        assert gold_label(tok, label) == label[:9]                          # bos + 9 bytes: split_label's max_length=10
        ids = encode_prompt(tok, prompt, 1 << 20)
        assert tok.decode(ids, skip_special_tokens=False) == "<|begin_of_text|>" + prompt
        lens.append(len(ids))
        right, left = encode_prompt(tok, prompt, 512, "right"), encode_prompt(tok, prompt, 512, "left")
        assert right == ids[:512] and left == ids[-512:] and len(right) == 512
        assert tok.decode(left).endswith("<|im_start|>assistant\n") and not tok.decode(right).endswith("assistant\n")
    assert min(lens) < 2000 and max(lens) > 7000                             # both short and long prompts, all over 512 tokens


def test_cli_arguments_file_name_and_refusal():
    from astts.cli import evaluate_erc as ev

    a = ev.build_parser().parse_args([])
    assert ev.data_path(a) == "./data//iemocap.test.0shot_w5_spdescV2.jsonl"      # the reference's f-string on its default folder
    assert (a.method, a.max_length, a.truncation_side, a.per_device_eval_batch_size, a.seed, a.limit) == ("generate", 512, "right", 1, 42, None)
    a = ev.build_parser().parse_args(["--model_path", "m", "--data_folder", "d", "--data_name", "meld", "--kshot", "2", "--window", "7",
                                      "--prompting_type", "cot", "--split", "valid"])
    assert a.model_path == "m" and ev.data_path(a) == "d/meld.valid.2shot_w7_cot.jsonl"
    a = ev.build_parser().parse_args(["--base_model_id", "b", "--data_file", "x.jsonl", "--method", "both", "--llm_precision", "int8",
                                      "--base_model_path", "bb", "--truncation_side", "left", "--limit", "5", "--save_details"])
    assert a.model_path == "b" and ev.data_path(a) == "x.jsonl" and a.method == "both" and a.llm_precision == "int8" and a.limit == 5
    with pytest.raises(SystemExit, match="re_gen_data is not supported"):
        ev.main(ev.build_parser().parse_args(["--re_gen_data", "--data_file", SUBSET]))


class _StubEmbedder:
    """Stand-in engine (the pattern of tests/test_drivers_dist_cpu.py): generation and label scores are pure functions of the prompt."""

    def __init__(self):
        from llm_scoring_tok import ByteTokenizer

        self.tokenizer = ByteTokenizer()
        self.names = ["angry", "excited", "frustrated", "happy", "neutral", "sad"]

    def generate_greedy_batch(self, prompts, max_new_tokens=10):
        out = []
        for p in prompts:
            word = self.names[sum(p) % 6] if sum(p) % 5 else "dunno"
            out.append(list(p) + self.tokenizer.encode("assistant\n" + word, add_special_tokens=False)[:max_new_tokens + 10] + [301])
        return out

    def classify(self, prompts, labels, batch=32):
        sums = np.array([[-float((sum(p) * (j + 3) + len(l)) % 17) - 0.5 * j for j, l in enumerate(labels)] for p in prompts])
        return [int(i) for i in sums.argmax(1)], sums, sums / np.array([len(l) for l in labels])[None, :]


def _erc_worker(rank, world, port, out):
    for p in (ROOT, os.path.join(ROOT, "autostyle-tts_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port), "ASTTS_DIST_BACKEND": "gloo"})
    torch.set_num_threads(1)
    from astts import parallel
    from astts.cli import evaluate_erc as ev

    args = ev.build_parser().parse_args(["--data_file", SUBSET, "--method", "both", "--save_details", "--details_output_path", out,
                                         "--per_device_eval_batch_size", "5"])
    res = ev.main(args, embedder=_StubEmbedder())
    assert (res is not None) == (rank == 0)
    parallel.shutdown()


def test_two_rank_run_writes_the_one_rank_details_file(tmp_path, capsys):
    import torch.multiprocessing as mp

    from astts.cli import evaluate_erc as ev

    one = str(tmp_path / "one.json")
    args = ev.build_parser().parse_args(["--data_file", SUBSET, "--method", "both", "--save_details", "--details_output_path", one,
                                         "--per_device_eval_batch_size", "5"])
    res = ev.main(args, embedder=_StubEmbedder())
    assert f"Base Model Test Weighted F1 Score: {res['f1_weighted']}" in capsys.readouterr().out
    assert len(res["detail_pred"]) == 48 and 0.0 <= res["agreement"] <= 1.0 and 0.0 < res["f1_weighted"] < 1.0
    assert all(len(d) == 3 for d in res["detail_pred"]) and res["label_set"] == _StubEmbedder().names
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    two = str(tmp_path / "two.json")
    mp.spawn(_erc_worker, args=(2, port, two), nprocs=2, join=True)
    assert open(one, "rb").read() == open(two, "rb").read()
    assert json.load(open(two))["f1_weighted"] == res["f1_weighted"]
