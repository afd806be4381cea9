"""CPU side of the Qwen2 track: what config.json becomes (and what is refused, by key), the plain RoPE frequencies against
transformers' own, the weight generator's stream, and the fp32 restatement of tests/qwen2_ref.py against the transformers fixture
(tests/golden/qwen2_tiny.npz, qwen2_tiny_train.npz)."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qwen2_ref as ref  # noqa: E402
from astts.llm.config import LlamaShape  # noqa: E402
from astts.llm.peft import shape_from_config  # noqa: E402
from astts.llm.weights import BIAS_OUTLIERS, make_llama_weights  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _write(tmp_path, conf) -> str:
    (tmp_path / "config.json").write_text(json.dumps(conf))
    return str(tmp_path)


def _llama3_conf(cfg):
    return dict(cfg.hf_kwargs(), architectures=["LlamaForCausalLM"], model_type="llama", torch_dtype="float16")      # llm_int8_ref.write_base


def test_qwen2_config_gives_bias_plain_rope_and_untied_head(tmp_path):
    cfg = LlamaShape.qwen2_tiny()
    got = shape_from_config(_write(tmp_path, ref.config_json(cfg)))
    assert got.qkv_bias and got.rope_type == "default" and not got.tie_embeddings and got.model_type == "qwen2"
    assert (got.heads, got.kv_heads, got.head_dim, got.rope_theta, got.rms_eps) == (7, 1, 128, 1e6, 1e-6)
    assert got == cfg
    # rope_scaling absent altogether, and transformers >= 5's layout (rope_parameters): the same shape
    conf = ref.config_json(cfg)
    del conf["rope_scaling"]
    assert shape_from_config(_write(tmp_path, conf)) == cfg
    del conf["rope_theta"]
    conf["rope_parameters"] = {"rope_theta": 1e6, "rope_type": "default"}
    assert shape_from_config(_write(tmp_path, conf)) == cfg
    assert shape_from_config(_write(tmp_path, ref.config_json(cfg)), vocab=520).vocab == 520


@pytest.mark.parametrize("name", ["tiny", "wide", "llama32_3b"])
def test_llama3_config_gives_exactly_the_preset(tmp_path, name):
    cfg = getattr(LlamaShape, name)()
    got = shape_from_config(_write(tmp_path, _llama3_conf(cfg)))
    assert got == cfg and got.rope_type == "llama3" and not got.qkv_bias and got.model_type == "llama"


def test_llama_config_without_rope_scaling_gets_plain_rope(tmp_path):
    conf = _llama3_conf(LlamaShape.tiny())
    conf["rope_scaling"] = None
    conf["attention_bias"] = True
    got = shape_from_config(_write(tmp_path, conf))
    assert got.rope_type == "default" and got.qkv_bias and got.model_type == "llama"
    conf["rope_scaling"] = {"type": "llama3", "factor": 8.0}                        # the older spelling of the key
    got = shape_from_config(_write(tmp_path, conf))
    assert got.rope_type == "llama3" and got.rope_factor == 8.0


@pytest.mark.parametrize("change,key", [
    ({"rope_scaling": {"rope_type": "yarn", "factor": 4.0}}, "rope_scaling"),
    ({"rope_scaling": {"type": "linear", "factor": 2.0}}, "rope_scaling"),
    ({"rope_scaling": {"rope_type": "dynamic", "factor": 2.0}}, "rope_scaling"),
    ({"rope_scaling": {"rope_type": "longrope"}}, "rope_scaling"),
    ({"rope_scaling": None, "rope_parameters": {"rope_type": "yarn", "rope_theta": 1e6}}, "rope_parameters"),
    ({"use_sliding_window": True}, "use_sliding_window"),
    ({"mlp_bias": True}, "mlp_bias"),
    ({"model_type": "mistral"}, "model_type"),
    ({"model_type": "qwen3"}, "model_type"),
])
def test_refusals_name_the_key(tmp_path, change, key):
    conf = dict(ref.config_json(LlamaShape.qwen2_tiny()), **change)
    with pytest.raises(ValueError, match=key):
        shape_from_config(_write(tmp_path, conf))


def test_default_inv_freq_is_transformers_bit_for_bit():
    from transformers.models.qwen2.modeling_qwen2 import Qwen2RotaryEmbedding

    from astts.llm.decoder import default_inv_freq, inv_freq, llama3_inv_freq

    cfg = LlamaShape.qwen2_tiny()
    want, factor = Qwen2RotaryEmbedding.compute_default_rope_parameters(cfg.hf_config())
    assert cfg.rope_theta == 1e6 and factor == 1.0 and want.dtype == torch.float32
    assert torch.equal(default_inv_freq(cfg), want) and torch.equal(inv_freq(cfg), want) and torch.equal(ref.inv_freq(cfg), want)
    # the Llama-3 function on its preset: unchanged, and what a Llama shape still gets
    import oracle.llama as ol

    c = LlamaShape.llama32_3b()
    l3 = ol.llama3_inv_freq(c.head_dim, c.rope_theta, c.rope_factor, c.rope_low_freq_factor, c.rope_high_freq_factor, c.rope_original_max_pos)
    assert torch.equal(llama3_inv_freq(c), l3.float()) and torch.equal(inv_freq(c), llama3_inv_freq(c))
    assert not torch.equal(inv_freq(dataclasses.replace(c, rope_type="default")), inv_freq(c))
    with pytest.raises(ValueError, match="rope_type"):
        inv_freq(dataclasses.replace(c, rope_type="yarn"))


def test_generator_stream_is_not_disturbed_by_the_biases():
    cfg = LlamaShape.tiny()
    plain = make_llama_weights(cfg, 0)
    assert not any(k.endswith(".bias") for k in plain)
    biased = make_llama_weights(dataclasses.replace(cfg, qkv_bias=True), 0)
    assert set(plain) < set(biased) and all(torch.equal(plain[k], biased[k]) for k in plain)
    extra = sorted(set(biased) - set(plain))
    assert len(extra) == 3 * cfg.layers and all(k.endswith(("q_proj.bias", "k_proj.bias", "v_proj.bias")) for k in extra)
    # the existing fixture's weights: the untied head is drawn where it was
    fx = np.load(os.path.join(GOLD, "llama_tiny.npz"))
    assert torch.equal(make_llama_weights(cfg, int(fx["seed"]))["model.norm.weight"],
                       make_llama_weights(dataclasses.replace(cfg, qkv_bias=True), int(fx["seed"]))["model.norm.weight"])
    q = make_llama_weights(LlamaShape.qwen2_tiny(), 1)
    for i in range(3):
        for nm, n in (("q", 896), ("k", 128)):
            b = q[f"model.layers.{i}.self_attn.{nm}_proj.bias"]
            assert b.shape == (n,) and sorted(b.abs().topk(len(BIAS_OUTLIERS)).indices.tolist()) == sorted(BIAS_OUTLIERS)
            rest = b[[j for j in range(n) if j not in BIAS_OUTLIERS]]
            assert float(b.abs().max()) == 16.0 and 0.35 < float(rest.std()) < 0.65 and float(rest.abs().max()) < 4.0
        assert float(q[f"model.layers.{i}.self_attn.v_proj.bias"].abs().max()) < 1.0


@pytest.fixture(scope="module")
def fixture():
    fx = {**np.load(os.path.join(GOLD, "qwen2_tiny.npz")), **np.load(os.path.join(GOLD, "qwen2_tiny_train.npz"))}
    cfg = LlamaShape.qwen2_tiny()
    sd = make_llama_weights(cfg, int(fx["seed"]))
    ids, lens = ref.make_batch(cfg, ref.LENS, int(fx["batch_seed"]))
    assert np.array_equal(ids.numpy(), fx["ids"]) and np.array_equal(lens.numpy(), fx["lens"]) and tuple(fx["lens"]) == (130, 64, 5)
    return fx, cfg, sd, ids, lens


def test_fp32_restatement_reproduces_the_fixture(fixture):
    fx, cfg, sd, ids, lens = fixture
    got = ref.outputs(sd, cfg, ref.fp_linear(sd, cfg), ids, lens)
    for k in ("hidden", "embedding", "logits_last", "logprobs"):
        e = ref.rel_l2(got[k], fx[k])
        print(f"qwen2_ref fp32 vs transformers: {k} rel L2 {e:.2e}")
        assert e <= 1e-5, (k, e)
    assert fx["hidden"].shape == (199, cfg.hidden)
    lora = ref.make_lora(cfg, int(fx["r"]), int(fx["lora_seed"]))
    loss, grads = ref.loss_and_grads(sd, cfg, lora, float(fx["lora_alpha"]) / int(fx["r"]), ids, lens)
    e = abs(loss - float(fx["loss"])) / float(fx["loss"])
    print(f"qwen2_ref fp32 vs transformers: loss {loss:.6f} vs {float(fx['loss']):.6f} rel {e:.2e}")
    assert e <= 1e-5
    worst = max(ref.rel_l2(g, fx[f"grad.{i}.{p}.{h}"]) for (i, p, h), g in grads.items())
    print(f"qwen2_ref fp32 vs transformers: worst gradient rel L2 {worst:.2e}")
    assert worst <= 1e-4 and len(grads) == 2 * 7 * cfg.layers          # the fixture's gradients keep 16 mantissa bits (2^-16)


def test_what_the_parent_commit_computed_is_far_from_the_fixture(fixture):
    """Dropping the biases, or scaling the frequencies as Llama-3 does, moves the hidden states by far more than any bound of
    tests/test_qwen2_gpu.py: the fixture sees both differences."""
    fx, cfg, sd, ids, lens = fixture
    zero = {k: (torch.zeros_like(v) if k.endswith(".bias") else v) for k, v in sd.items()}
    e = ref.rel_l2(ref.outputs(zero, cfg, ref.fp_linear(zero, cfg), ids, lens)["hidden"], fx["hidden"])
    assert e > 0.1, e
    from astts.llm.decoder import default_inv_freq, llama3_inv_freq
    l3 = llama3_inv_freq(dataclasses.replace(cfg, rope_type="llama3"))
    assert float((l3 / default_inv_freq(cfg)).min()) < 0.05                     # Llama-3 scaling divides the slow frequencies by 32


def test_written_qwen2_directory_loads_with_its_biases(tmp_path):
    from astts.llm.peft import load_peft_model
    from astts.llm.weights import load_llama_weights

    cfg = LlamaShape.qwen2_tiny()
    sd = make_llama_weights(cfg, 3)
    base = ref.write_base(str(tmp_path / "base"), cfg, sd)
    state = load_llama_weights(base)
    assert set(state) == set(sd) and torch.equal(state["model.layers.2.self_attn.k_proj.bias"], sd["model.layers.2.self_attn.k_proj.bias"].half().float())
    lora = ref.make_lora(cfg, 8, 5)
    ada = ref.write_adapter(str(tmp_path / "adapter"), lora, 8, 32.0, base="org/not-on-this-disk")
    state2, cfg2, ad, _ = load_peft_model(ada, base)
    assert cfg2 == dataclasses.replace(cfg, eos_token_ids=(cfg.eos_token_id,)) and ad.scaling == 4.0 and len(ad.pairs) == 21
    assert "model.layers.0.self_attn.q_proj.bias" in state2


def test_a_directory_without_tokenizer_files_gets_no_tokenizer(tmp_path, capsys):
    """transformers builds an empty Qwen2 tokenizer from config.json alone (every text -> no tokens); the loader looks for the files."""
    from astts.cli.search_milvus import load_tokenizer

    cfg = LlamaShape.qwen2_tiny()
    base = ref.write_base(str(tmp_path / "base"), cfg, {"model.norm.weight": torch.ones(cfg.hidden)})
    assert load_tokenizer(base) is None
    assert "no tokenizer under" in capsys.readouterr().out
