"""CPU tests of the fine-tuning recipe's host side: the numpy restatement of Philox4x32-10 (tests/lora_reg_ref.py) against the
Random123 known answers, the dropout threshold, the linear learning-rate schedule against torch's LambdaLR with transformers' lambda,
trl's packing on hand-made token lists, the new ft_llm flags, and the header's new entry points."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_reg_ref as rr  # noqa: E402


def _words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter,key,out", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, out):
    got = rr.philox4x32_10(_words(counter), _words(key))
    assert [int(w) for w in got] == _words(out)
    both = rr.philox4x32_10([np.array([c, 0], dtype=np.uint64) for c in _words(counter)], _words(key))     # vectorised = element-wise
    assert [int(w[0]) for w in both] == _words(out)


def test_dropout_threshold_and_mask_layout():
    from astts.train_ops import dropout_threshold
    assert rr.dropout_threshold(0.05) == 3276 == dropout_threshold(0.05)
    assert rr.dropout_threshold(0.5) == 32768 and rr.dropout_threshold(0.0) == 0
    seed, stream, draw = 42 + (7 << 32), 2 * 8 + 5, 9
    m = rr.dropout_mask(3, 16, 0.5, seed, stream, draw)
    assert m.shape == (3, 16) and m.dtype == np.uint8
    # element e of group g: 16 bits of word e >> 1 of philox((g, 0, stream, draw), (seed low, seed high)), low half when e is even
    g, e = 4, 5                                                 # row 2, column 5 of a [3, 16] input
    w = rr.philox4x32_10((g, 0, stream, draw), (42, 7))
    bits = (int(w[e >> 1]) >> 16) & 0xFFFF
    assert m[2, 5] == (bits >= 32768)
    assert rr.dropout_mask(3, 16, 0.0, seed, stream, draw).all()
    noise = rr.neftune_noise(2, 8, 0.25, seed, draw)
    w = rr.philox4x32_10((3, 0, rr.NEFTUNE_STREAM, draw), (42, 7))                                          # element 13: word 1 of group 3
    assert noise[1, 5] == 0.25 * (2 * ((int(w[1]) >> 8) + 0.5) * 2.0 ** -24 - 1)
    assert (np.abs(noise) < 0.25).all()


def test_linear_schedule():
    from astts.llm.train import lr_at, warmup_steps
    total, base = 100, 2e-4
    w = warmup_steps(total)
    assert w == 3

    def lr_lambda(step):                                        # transformers' _get_linear_schedule_with_warmup_lr_lambda
        if step < w:
            return float(step) / float(max(1, w))
        return max(0.0, float(total - step) / float(max(1, total - w)))

    sched = torch.optim.lr_scheduler.LambdaLR(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=base), lr_lambda)
    for s in range(total + 1):
        assert abs(sched.get_last_lr()[0] - lr_at(s, base, total, schedule="linear")) < 1e-18, s
        sched.optimizer.step()
        sched.step()
    assert lr_at(total, base, total, schedule="linear") == 0.0 and lr_at(total + 5, base, total, schedule="linear") == 0.0
    assert lr_at(0, base, total, schedule="linear") == 0.0 and lr_at(w, base, total, schedule="linear") == base
    assert [lr_at(s, base, total) for s in (0, 3, 99)] == [0.0, base, base]           # the default is still the constant schedule
    assert lr_at(50, base, total, 0.03, "constant") == base
    with pytest.raises(ValueError):
        lr_at(1, base, total, schedule="cosine")


def test_pack_rows():
    from astts.cli.ft_llm import PACK_CHARS_PER_TOKEN, PACK_NUM_SEQUENCES, pack_rows
    seqs = [[1, 10, 11], [1, 20], [1, 30, 31, 32, 33], [1, 40]]
    flat = [t for s in seqs for t in s]                          # 12 tokens, nothing between the rows
    out = pack_rows(seqs, 5, [9, 6, 15, 6])
    assert out == [flat[0:5], flat[5:10]]                        # exactly the concatenation cut at 5; the tail of 2 is dropped
    assert pack_rows(seqs, 4, [9, 6, 15, 6]) == [flat[0:4], flat[4:8], flat[8:12]]
    assert pack_rows(seqs, 13, [9, 6, 15, 6]) == [] and pack_rows([], 4, []) == []
    # a buffer takes rows until it holds seq_len * 3.6 * 1024 characters: with seq_len 2 that is 7372.8, so two rows of 4000 characters
    # fill one buffer, and each buffer drops its own tail instead of handing it to the next
    assert 2 * PACK_CHARS_PER_TOKEN * PACK_NUM_SEQUENCES == 7372.8
    rows = [[1, 2, 3], [4, 5], [6, 7, 8], [9, 10, 11, 12]]
    assert pack_rows(rows, 2, [4000, 4000, 4000, 4000]) == [[1, 2], [3, 4], [6, 7], [8, 9], [10, 11]]      # 5 and 12 are the tails
    assert pack_rows(rows, 2, [4000, 3000, 4000, 4000]) == [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12]]   # 7000 < 7372.8: a third row joins


def test_parser_new_flags(capsys):
    from astts.cli import ft_llm
    a = ft_llm.build_parser().parse_args([])
    assert (a.lr_scheduler, a.lora_dropout, a.neftune_noise_alpha, a.packing) == ("constant", 0.0, 0.0, False)
    a = ft_llm.build_parser().parse_args("--lr_scheduler linear --lora_dropout 0.05 --neftune_noise_alpha 5 --packing --max_seq_len 1024".split())
    assert (a.lr_scheduler, a.lora_dropout, a.neftune_noise_alpha, a.packing, a.max_seq_len) == ("linear", 0.05, 5.0, True, 1024)
    for parse in (ft_llm.build_parser().parse_args, ft_llm.build_parser().parse_known_args):            # main() parses with the second
        with pytest.raises(SystemExit) as e:
            parse(["--lr_scheduler", "cosine"])
        assert e.value.code == 2
    assert "--lr_scheduler" in capsys.readouterr().err
    for word in ("linear", "0.05", "neftune_noise_alpha 5", "1024"):                                       # the reference's own values
        assert word in ft_llm.__doc__, word


def test_adapter_config_carries_the_dropout(tmp_path):
    import json

    from astts.llm.config import LlamaShape
    from astts.llm.peft import load_adapter
    from astts.llm.train import init_lora, save_adapter
    ad = init_lora(LlamaShape.tiny(), 8, 128.0)
    save_adapter(ad, str(tmp_path / "a"), lora_dropout=0.05)
    save_adapter(ad, str(tmp_path / "b"))
    assert json.load(open(tmp_path / "a" / "adapter_config.json"))["lora_dropout"] == 0.05
    assert json.load(open(tmp_path / "b" / "adapter_config.json"))["lora_dropout"] == 0.0
    assert load_adapter(str(tmp_path / "a")).r == 8


def test_new_entry_points_under_abi_1():
    from astts import _lib, _lib_train
    names = _lib_train.declared_symbols()
    for need in ("dropout_mask", "neftune", "lora_down", "lora_grad_dropout", "lora_dx_dropout"):
        assert f"astts_train_{need}" in names
    lib = _lib_train.load()
    assert lib.astts_train_abi_version() == 1 and _lib_train.ABI_VERSION == 1
    # host-side argument checks answer without a GPU
    assert lib.astts_train_lora_down(None, 0, None, 0, None, 0, 1, 8, 1, 8, 0.1, 0, 0, 0, None) == _lib.ERR_INVALID
    assert b"lora_down" in lib.astts_train_last_error_string()
    assert lib.astts_train_dropout_mask(None, 4, 12, 0.1, 0, 0, 0, None) == _lib.ERR_INVALID              # cin not a multiple of 8
    assert lib.astts_train_neftune(None, 4, 8, 0.1, 0, 0, None) == _lib.ERR_INVALID
    assert lib.astts_train_lora_dx_dropout(None, 0, None, 0, None, None, 0, 1, 8, 4, 8, 0.1, 0, 0, 0, None) == _lib.ERR_INVALID   # parts > 3
    assert lib.astts_train_lora_grad_dropout(None, 0, 0, None, 0, None, 0, 1, 1, 12, 8, 1.0, 0, 0.1, 0, 0, 0, None, 0, None) == _lib.ERR_INVALID
