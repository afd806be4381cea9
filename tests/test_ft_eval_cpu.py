"""CPU tests of evaluation while fine-tuning: the merge entry point's declaration and host-side refusals, the step / best / rotation
rules of ft_llm on literal sequences, the new flags' defaults, and the data position's round trip through trainer_state.json."""
import json
import random

import pytest


def test_merge_entry_point_declared_under_abi_1():
    from astts import _lib_train
    assert "astts_train_lora_merge" in _lib_train.declared_symbols()
    assert _lib_train.load().astts_train_abi_version() == 1 and _lib_train.ABI_VERSION == 1


# (w, a, b, out, n, cin, n_pad, cin_pad, r, g1, g2): fake non-NULL pointers are never dereferenced, every case is refused on the host
P, Q = 0x10000, 0x900000
GOOD = dict(w=P, a=P, b=P, out=Q, n=256, cin=64, n_pad=256, cin_pad=64, r=8, g1=256, g2=256)


@pytest.mark.parametrize("change", [
    dict(w=None), dict(a=None), dict(b=None), dict(out=None),                       # NULL pointers
    dict(r=12), dict(r=0),                                                          # r % 8
    dict(g1=100), dict(g1=128, g2=200), dict(g1=192, g2=128), dict(g1=0), dict(g2=288), dict(g1=128, g2=128),   # part boundaries
    dict(n_pad=192), dict(n=130, n_pad=128),                                        # n_pad % 128, n_pad < n
    dict(cin_pad=96), dict(cin=70, cin_pad=64),                                     # cin_pad % 64, cin_pad < cin
    dict(out=P), dict(out=P + 64),                                                  # out aliases / overlaps w
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_merge_refuses_on_the_host(change):
    from astts import _lib, _lib_train
    lib = _lib_train.load()
    k = dict(GOOD, **change)
    code = lib.astts_train_lora_merge(k["w"], k["a"], k["b"], k["out"], k["n"], k["cin"], k["n_pad"], k["cin_pad"], k["r"], k["g1"], k["g2"], 4.0, None)
    assert code == _lib.ERR_INVALID
    assert b"lora_merge" in lib.astts_train_last_error_string()


def test_eval_steps():
    from astts.cli.ft_llm import should_eval, should_save
    assert [s for s in range(1, 401) if should_eval(s, 50, 200)] == [200, 250, 300, 350, 400]
    assert [s for s in range(1, 401) if should_eval(s, 0, 200)] == []                      # off
    assert [s for s in range(1, 13) if should_eval(s, 4, 6)] == [8, 12]                    # the delay is no multiple of eval_steps
    assert [s for s in range(1, 8) if should_save(s, 2)] == [2, 4, 6] and not any(should_save(s, 0) for s in range(1, 8))


def test_best_is_the_first_maximum():
    from astts.cli.ft_llm import is_better
    best, at = None, None
    for i, m in enumerate([0.3, 0.5, 0.5, 0.4]):
        if is_better(m, best):
            best, at = m, i
    assert (best, at) == (0.5, 1)
    assert is_better(0.0, None) and not is_better(0.5, 0.5)


@pytest.mark.parametrize("limit,saves,best,keep", [
    (1, [2, 4, 6], 2, {2, 6}),
    (1, [2, 4, 6], 6, {6}),
    (2, [2, 4, 6, 8], 2, {2, 8}),
    (None, [2, 4, 6], 2, {2, 4, 6}),
    (1, [2, 4], None, {4}),              # no evaluation yet: the limit becomes 2 only for a best that exists
    (3, [2, 4, 6], 4, {2, 4, 6}),
])
def test_rotation(limit, saves, best, keep):
    from astts.cli.ft_llm import checkpoints_to_delete
    gone = checkpoints_to_delete(saves, best, limit)
    assert set(saves) - set(gone) == keep and sorted(gone) == gone


def test_rotation_step_by_step_keeps_best_and_newest():
    """As the command calls it: after every save, on what is on disk."""
    from astts.cli.ft_llm import checkpoints_to_delete
    disk, best, metrics = [], None, {2: 0.3, 4: 0.5, 6: 0.5, 8: 0.4}
    for s in (2, 4, 6, 8):
        if best is None or metrics[s] > metrics[best]:
            best = s
        disk.append(s)
        for g in checkpoints_to_delete(disk, best, 1):
            disk.remove(g)
        assert set(disk) == {best, s}
    assert disk == [4, 8]


def test_load_best_needs_save_steps_multiple_of_eval_steps():
    from astts.cli import ft_llm
    ok = ft_llm.build_parser().parse_args("--eval_steps 2 --save_steps 4 --load_best_model_at_end".split())
    ft_llm.check_flags(ok)
    for bad in ("--eval_steps 4 --save_steps 6 --load_best_model_at_end", "--eval_steps 2 --load_best_model_at_end",
                "--save_steps 2 --load_best_model_at_end"):
        with pytest.raises(SystemExit) as e:
            ft_llm.check_flags(ft_llm.build_parser().parse_args(bad.split()))
        assert e.value.code not in (0, None) and "load_best_model_at_end" in str(e.value.code)
    ft_llm.check_flags(ft_llm.build_parser().parse_args("--eval_steps 4 --save_steps 6".split()))     # without the flag: any pair


def test_parser_leaves_the_feature_off():
    from astts.cli import ft_llm
    a = ft_llm.build_parser().parse_args([])
    assert (a.eval_steps, a.save_steps, a.eval_delay, a.save_total_limit, a.load_best_model_at_end, a.total_steps) == (0, 0, 200, None, False, None)
    assert not any(ft_llm.should_eval(s, a.eval_steps, a.eval_delay) or ft_llm.should_save(s, a.save_steps) for s in range(1, 1000))
    a = ft_llm.build_parser().parse_args("--eval_steps 50 --save_steps 50 --eval_delay 200 --save_total_limit 1 --load_best_model_at_end".split())
    assert (a.eval_steps, a.save_steps, a.eval_delay, a.save_total_limit, a.load_best_model_at_end) == (50, 50, 200, 1, True)
    for word in ("--eval_steps 50", "--save_total_limit 1", "--load_best_model_at_end", "--total_steps", "eval_log.jsonl"):
        assert word in ft_llm.__doc__, word


def test_data_position_round_trip(tmp_path):
    from astts.cli.ft_llm import data_position_from_json, data_position_to_json
    rng = random.Random(42)
    order = list(range(37))
    rng.shuffle(order)
    path = tmp_path / "trainer_state.json"
    with open(path, "w") as f:
        json.dump({"global_step": 4, "data_position": data_position_to_json(order, 16, rng)}, f)
    with open(path) as f:
        order2, pos2, rng2 = data_position_from_json(json.load(f)["data_position"])
    assert order2 == order and pos2 == 16
    nxt, nxt2 = list(range(37)), list(range(37))
    rng.shuffle(nxt)
    rng2.shuffle(nxt2)
    assert nxt == nxt2 and rng.random() == rng2.random()


def test_data_fingerprint():
    from astts.cli.ft_llm import data_fingerprint
    a = data_fingerprint([[1, 2, 3], [4, 5]])
    assert a["sequences"] == 2 and a == data_fingerprint([[1, 2, 3], [4, 5]])
    assert a != data_fingerprint([[1, 2], [3, 4, 5]]) and a != data_fingerprint([[1, 2, 3], [4, 6]])


def test_checkpoint_steps_and_log_trim(tmp_path):
    from astts.cli import ft_llm
    for s in (2, 10):
        (tmp_path / f"checkpoint-{s}").mkdir()
        (tmp_path / f"checkpoint-{s}" / ft_llm.TRAINER_STATE).write_text("{}")
    (tmp_path / "checkpoint-12").mkdir()                                   # no trainer_state.json: a save that did not finish
    (tmp_path / "checkpoint-x").mkdir()
    assert ft_llm.checkpoint_steps(str(tmp_path)) == [2, 10]
    log = tmp_path / "train_log.jsonl"
    log.write_text("".join(json.dumps({"step": s}) + "\n" for s in (1, 2, 3, 4, 5)))
    ft_llm._trim_log(str(log), 4)
    assert [json.loads(ln)["step"] for ln in open(log)] == [1, 2, 3, 4]
