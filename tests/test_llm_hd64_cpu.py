"""CPU side of head dimension 64 (DESIGN.md section 2 "Head dimension 64"): tests/llm_attn_hd_ref.py against the proven
tests/llm_ops_ref.py at 128 (bit for bit), its tolerance against the measured fp16-emulation floor at 64, the sensitivity of the 64 case
list to every wrong mask, what a Llama-3.2-1B-shaped config.json becomes, the new presets, and the fp32 restatement of
tests/llama_hd64_ref.py against the transformers fixture (tests/golden/llama_hd64.npz, llama_hd64_train.npz).
Measured here: floor 1.062e-3 (ATTN64_EMU_FLOOR 1.06e-3), ATTN64_TOL 3.18e-3.  Nothing here needs a GPU; the last test asks the native
library's host-side GEMM dispatch about Qwen2.5-0.5B's widths."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import llama_hd64_ref as lref  # noqa: E402
import llm_attn_hd_ref as ref  # noqa: E402
import llm_ops_ref as opsref  # noqa: E402
from astts.llm.config import LlamaShape  # noqa: E402
from astts.llm.peft import shape_from_config  # noqa: E402
from astts.llm.weights import make_llama_weights  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# every fourth case of the proven lists: all forms, both geometries, one to three query blocks
TIE_CASES = (opsref.ATTN_CASES_BM + opsref.ATTN_CASES_TM)[::4]


@pytest.mark.parametrize("case", TIE_CASES, ids=[c.name for c in TIE_CASES])
def test_at_128_the_module_is_llm_ops_ref_bit_for_bit(case):
    mine, theirs = ref.build_attn(ref.AttnCase(*case), 128), opsref.build_attn(case)
    assert set(mine.bufs) == set(theirs.bufs) and all(torch.equal(mine.bufs[k], theirs.bufs[k]) for k in theirs.bufs)
    assert torch.equal(mine.q, theirs.q) and torch.equal(mine.k, theirs.k) and torch.equal(mine.v, theirs.v)
    assert torch.equal(ref.attn_expected(ref.AttnCase(*case), 128), opsref.attn_expected(case))
    a = (case.pos0, case.key_start, case.lens)
    assert torch.equal(ref.attn_ref(mine.q, mine.k, mine.v, *a, emulate=True), opsref.attn_ref(theirs.q, theirs.k, theirs.v, *a, emulate=True))


def test_at_128_the_constants_and_mutations_are_llm_ops_ref_s():
    assert ref.MUTATIONS == opsref.MUTATIONS and ref.TM_EXTRA_ROWS == opsref.TM_EXTRA_ROWS
    assert (ref.scale_of(128), ref.alpha_of(128)) == (opsref.SCALE, opsref.ALPHA)
    assert (ref.BETA, ref.POISON_K, ref.POISON_V, ref.NOISE, ref.LOG2E) == (opsref.BETA, opsref.POISON_K, opsref.POISON_V, opsref.NOISE, opsref.LOG2E)
    case = opsref.ATTN_CASES_TM[9]
    x = opsref.build_attn(case)
    for mut in ref.MUTATIONS:
        a = (case.pos0, case.key_start, case.lens)
        assert torch.equal(ref.attn_ref(x.q, x.k, x.v, *a, mutate=mut), opsref.attn_ref(x.q, x.k, x.v, *a, mutate=mut)), mut
    r = torch.zeros(3, 64, dtype=torch.float64)
    r[0, 5], r[1, 7] = 100.0, 0.01
    g = r.clone()
    g[1, 9], g[2, 0] = 0.001, 1e-30
    for mod in (ref, opsref):
        err, bad = mod.row_errors(g, r)
        assert err.tolist() == [0.0, pytest.approx(0.1), 0.0] and bad.tolist() == [False, False, True]


def test_the_64_case_list_is_the_one_the_kernels_need():
    assert len({c.name for c in ref.CASES_64}) == len(ref.CASES_64)
    assert ref.GEOMS_64 == ((8, 2), (14, 2), (2, 2))
    for geom in ref.GEOMS_64:
        bm = [c for c in ref.CASES_BM_64 if (c.heads, c.kv_heads) == geom]
        for t in (1, 33, 65, 129):
            assert {c.lens for c in bm if c.tq == t} == {(t, 1), (t, t - 1)}
        assert {c.lens for c in bm if c.tq == 257} == {(257, 129, 128, 64)}
        tm = [c for c in ref.CASES_TM_64 if (c.heads, c.kv_heads) == geom]
        assert {(c.tq, c.tk) for c in tm} == {(1, 1), (1, 65), (1, 129), (3, 65), (40, 73), (130, 333), (70, 300)}
        by = {(c.tq, c.tk): c for c in tm}
        assert by[(1, 129)].key_start == (64, 65, 127, 128) and by[(130, 333)].key_start == (64, 200, 332, 270)
        assert by[(70, 300)].pos0 == 200 and by[(70, 300)].lens is not None and any(by[(70, 300)].key_start)
        for c in tm:
            assert c.pos0 + c.tq <= c.tk and ref.build_attn(c).bufs["cache"].shape[0] == c.tk + ref.TM_EXTRA_ROWS
            x = ref.build_attn(c)
            hk = c.kv_heads * 64
            assert bool((x.bufs["cache"][c.tk:, :, hk:].abs() == ref.POISON_V).all())              # rows past tk are poisoned
    x = ref.build_attn(ref.CASES_BM_64[0])
    assert x.q.shape[-1] == 64 and x.bufs["qkv"].shape[-1] == (8 + 4) * 64


def test_tolerance_is_three_times_the_emulation_floor_at_64():
    """The float64 emulation of the matrix-core kernel's three fp16 roundings over CASES_64: ATTN64_EMU_FLOOR is its worst per-row error
    (to 10 %), and ATTN64_TOL lies between 2 x and 4 x the value measured here."""
    worst, where = 0.0, None
    for case in ref.CASES_64:
        x = ref.build_attn(case)
        err, bad = ref.row_errors(ref.attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens, emulate=True), ref.attn_expected(case))
        assert not bool(bad.any()), case.name
        if float(err.max()) > worst:
            worst, where = float(err.max()), case.name
    print(f"[llm-hd64] fp16-emulation floor {worst:.3e} at {where}; ATTN64_EMU_FLOOR {ref.ATTN64_EMU_FLOOR:.3e}, ATTN64_TOL {ref.ATTN64_TOL:.3e}")
    assert abs(ref.ATTN64_EMU_FLOOR - worst) <= 0.1 * worst
    assert ref.ATTN64_TOL == 3 * ref.ATTN64_EMU_FLOOR and 2 * worst <= ref.ATTN64_TOL <= 4 * worst


@pytest.mark.parametrize("mut", ref.MUTATIONS)
def test_every_wrong_mask_moves_a_64_case_by_100_tolerances(mut):
    """A case list that cannot see a mask bug is no test: each mutation moves some row of some 64 case by more than 100 x ATTN64_TOL of
    the row's scale (a row that must be zero: by that much in absolute value)."""
    best, where = 0.0, None
    for case in ref.CASES_64:
        x = ref.build_attn(case)
        out = ref.attn_ref(x.q, x.k, x.v, case.pos0, case.key_start, case.lens, mutate=mut)
        err, bad = ref.row_errors(out, ref.attn_expected(case))
        moved = max(float(err.max()), float(out[bad].abs().max()) if bool(bad.any()) else 0.0)
        if moved > best:
            best, where = moved, case.name
    print(f"[llm-hd64] {mut}: moves {where} by {best / ref.ATTN64_TOL:.0f} x ATTN64_TOL")
    assert best > 100 * ref.ATTN64_TOL, (mut, best)


def _llama_1b_config():
    """Llama-3.2-1B's published config.json."""
    return {"architectures": ["LlamaForCausalLM"], "attention_bias": False, "attention_dropout": 0.0, "bos_token_id": 128000,
            "eos_token_id": 128001, "head_dim": 64, "hidden_act": "silu", "hidden_size": 2048, "initializer_range": 0.02,
            "intermediate_size": 8192, "max_position_embeddings": 131072, "mlp_bias": False, "model_type": "llama",
            "num_attention_heads": 32, "num_hidden_layers": 16, "num_key_value_heads": 8, "pretraining_tp": 1, "rms_norm_eps": 1e-05,
            "rope_scaling": {"factor": 32.0, "high_freq_factor": 4.0, "low_freq_factor": 1.0, "original_max_position_embeddings": 8192,
                             "rope_type": "llama3"},
            "rope_theta": 500000.0, "tie_word_embeddings": True, "torch_dtype": "bfloat16", "use_cache": True, "vocab_size": 128256}


@pytest.mark.parametrize("with_key", [True, False])
def test_a_llama_1b_config_gives_head_dim_64(tmp_path, with_key):
    conf = _llama_1b_config()
    if not with_key:
        del conf["head_dim"]
    (tmp_path / "config.json").write_text(json.dumps(conf))
    got = shape_from_config(str(tmp_path))
    assert got.head_dim == 64 and (got.hidden, got.heads, got.kv_heads, got.ffn, got.layers, got.vocab) == (2048, 32, 8, 8192, 16, 128256)
    assert got == LlamaShape.llama32_1b() and got.tie_embeddings and got.rope_type == "llama3" and got.rope_factor == 32.0


def test_the_new_presets_build_their_transformers_config():
    want = {"llama32_1b": (2048, 16, 32, 8, 8192, 128256), "tiny64": (512, 3, 8, 2, 1024, 512), "wide64": (2048, 2, 32, 8, 8192, 4096),
            "qwen2_tiny64": (896, 3, 14, 2, 1152, 512)}
    for name, (hidden, layers, heads, kvh, ffn, vocab) in want.items():
        cfg = getattr(LlamaShape, name)()
        assert (cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads, cfg.ffn, cfg.vocab, cfg.head_dim) == (hidden, layers, heads, kvh, ffn, vocab, 64)
        assert cfg.heads * cfg.head_dim == cfg.hidden
        hf = cfg.hf_config()
        assert (hf.hidden_size, hf.num_attention_heads, hf.num_key_value_heads, hf.intermediate_size) == (hidden, heads, kvh, ffn)
        assert getattr(hf, "head_dim", hf.hidden_size // hf.num_attention_heads) == 64 and hf.model_type == cfg.model_type
    q, q64 = LlamaShape.qwen2_tiny(), LlamaShape.qwen2_tiny64()
    assert q64 == LlamaShape(**{**q.__dict__, "heads": 14, "kv_heads": 2, "head_dim": 64})
    # the presets from before are what they were
    assert LlamaShape.tiny() == LlamaShape(vocab=512, hidden=512, layers=3, heads=4, kv_heads=2, ffn=1024, eos_token_id=2, bos_token_id=1)
    assert LlamaShape.llama32_3b() == LlamaShape() and LlamaShape().head_dim == 128


def test_fp32_restatement_reproduces_the_fixture():
    fx = {**np.load(os.path.join(GOLD, "llama_hd64.npz")), **np.load(os.path.join(GOLD, "llama_hd64_train.npz"))}
    cfg = LlamaShape.tiny64()
    sd = make_llama_weights(cfg, int(fx["seed"]))
    ids, lens = torch.from_numpy(fx["ids"]), torch.from_numpy(fx["lens"])
    assert int(fx["batch_seed"]) in lref.BATCH_SEEDS and tuple(lens.tolist()) == lref.LENS
    want_ids, _ = lref.make_batch(cfg, lref.LENS, int(fx["batch_seed"]))
    assert torch.equal(ids, want_ids)
    assert all(os.path.getsize(os.path.join(GOLD, f)) < 1 << 20 for f in ("llama_hd64.npz", "llama_hd64_train.npz"))
    got = lref.outputs(sd, cfg, ids, lens)
    for k in ("hidden", "embedding", "logits_last", "logprobs"):
        e = lref.rel_l2(got[k], fx[k])
        print(f"llama_hd64_ref fp32 vs transformers: {k} rel L2 {e:.2e}")
        assert e <= 2e-6, (k, e)
    lora = lref.make_lora(cfg, int(fx["r"]), int(fx["lora_seed"]))
    loss, grads = lref.loss_and_grads(sd, cfg, lora, float(fx["lora_alpha"]) / int(fx["r"]), ids, lens)
    e = abs(loss - float(fx["loss"])) / float(fx["loss"])
    print(f"llama_hd64_ref fp32 vs transformers: loss {loss:.6f} vs {float(fx['loss']):.6f} rel {e:.2e}")
    assert e <= 2e-6
    worst = max(lref.rel_l2(g, fx[f"grad.{i}.{p}.{h}"]) for (i, p, h), g in grads.items())
    print(f"llama_hd64_ref fp32 vs transformers: worst gradient rel L2 {worst:.2e}")
    assert len(grads) == 2 * 7 * cfg.layers and worst <= 2e-6 + 2.0 ** -16           # the stored gradients keep 16 mantissa bits
    toks = lref.greedy(sd, cfg, ids[2, :5].tolist(), lref.GEN_LEN)[0]
    assert toks == fx["greedy"][2].tolist() and float(fx["greedy_margins"].min()) > 1.0


def test_qwen25_05b_widths_pass_the_gemm_dispatch():
    """Qwen2.5-0.5B: hidden 896 = 7 x 128, FFN 4864 = 38 x 128 (multiples of 128, not of 256), vocabulary 151 936.  The launcher's own
    rule (astts_op_gemm_kernel_kind, a host query) takes every projection of that model: the K-128 tile for a decode step's rows, the
    ring kernel for a prompt's.  No GEMM is run here."""
    from astts import ops
    shapes = {"qkv": (896 + 2 * 128, 896), "o": (896, 896), "gate|up": (2 * 4864, 896), "down": (896, 4864), "head": (151936, 896)}
    for m, want in ((1, "T64k128"), (33, "T64k128"), (130, "ring"), (512, "ring")):
        for name, (n, k) in shapes.items():
            for out_f16 in (False, True):
                kind = ops.gemm_kernel_kind(m, n, k, x_f16=True, out_f16=out_f16)
                assert kind == (want if name != "head" or m > 64 else "T128"), (m, name, out_f16, kind)
