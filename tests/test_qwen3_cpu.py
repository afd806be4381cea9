"""The Qwen3 track without a GPU (DESIGN.md section 2 "Qwen3"): the restatement of tests/qwen3_ref.py reproduces the transformers
fixture, the seeded weights of every earlier shape are what they were, config.json is read and refused by key, and the two new entry
points answer their host-side argument checks."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qwen3_ref as ref  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return {**np.load(os.path.join(GOLD, "qwen3_tiny.npz")), **np.load(os.path.join(GOLD, "qwen3_tiny_train.npz"))}


def test_shapes_keep_hq_and_hidden_apart():
    from astts.llm.config import LlamaShape
    from astts.llm.train import proj_shapes
    cfg, un = LlamaShape.qwen3_tiny(), LlamaShape.qwen3_tiny_untied()
    assert (cfg.vocab, cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.ffn) == (512, 640, 3, 8, 4, 128, 1152)
    assert cfg.heads * cfg.head_dim == 1024 != cfg.hidden and cfg.kv_heads * cfg.head_dim == 512
    assert cfg.qk_norm and not cfg.qkv_bias and cfg.rope_type == "default" and cfg.rope_theta == 1e6 and cfg.rms_eps == 1e-6
    assert cfg.model_type == "qwen3" and cfg.tie_embeddings and un == dataclasses.replace(cfg, tie_embeddings=False)
    assert proj_shapes(cfg)["q_proj"] == (1024, 640) and proj_shapes(cfg)["o_proj"] == (640, 1024) and proj_shapes(cfg)["k_proj"] == (512, 640)
    for old in ("llama32_3b", "tiny", "wide", "qwen2_tiny", "llama32_1b", "tiny64", "wide64", "qwen2_tiny64"):
        assert not getattr(LlamaShape, old)().qk_norm


@pytest.mark.parametrize("name", ref.SHAPES)
def test_fp32_restatement_reproduces_the_fixture(fx, name):
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = getattr(LlamaShape, name)()
    pre = "" if cfg.tie_embeddings else "untied."
    sd = make_llama_weights(cfg, int(fx["seed"]))
    ids, lens = torch.from_numpy(fx["ids"]), torch.from_numpy(fx["lens"])
    got = ref.outputs(sd, cfg, ref.fp_linear(sd, cfg), ids, lens)
    if not cfg.tie_embeddings:
        got["hidden"] = got["hidden"][-int(lens[-1]):]
    for k, v in got.items():
        e = ref.rel_l2(v, fx[pre + k])
        assert e <= 2e-5, (name, k, e)                        # fp32 against fp32 through three layers: a few 1e-6 measured
    off = ref.outputs(sd, cfg, ref.fp_linear(sd, cfg), ids, lens, qk_norm=False)
    assert ref.rel_l2(off["embedding"], fx[pre + "embedding"]) > 0.1      # the norm is what the fixture is about
    toks = [ref.greedy(sd, cfg, ref.fp_linear(sd, cfg), ids[i, :int(n)].tolist(), 2)[0] for i, n in enumerate(lens)]
    assert toks == fx[pre + "greedy"][:, :2].tolist()


def test_fp32_restatement_reproduces_loss_and_gradients(fx):
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights
    cfg = LlamaShape.qwen3_tiny()
    sd = make_llama_weights(cfg, int(fx["seed"]))
    ids, lens = torch.from_numpy(fx["ids"]), torch.from_numpy(fx["lens"])
    lora = ref.make_lora(cfg, int(fx["r"]), int(fx["lora_seed"]))
    loss, grads = ref.loss_and_grads(sd, cfg, lora, float(fx["lora_alpha"]) / int(fx["r"]), ids, lens)
    assert abs(loss - float(fx["loss"])) <= 1e-5 * float(fx["loss"])
    assert len(grads) == 2 * 7 * cfg.layers
    for (i, p, h), g in grads.items():
        assert ref.rel_l2(g, fx[f"grad.{i}.{p}.{h}"]) <= 1e-4 + 2.0 ** -16, (i, p, h)      # the file keeps 16 mantissa bits


def test_qknorm_rope_restatement_has_the_properties_the_kernel_is_held_to():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 3, 64, generator=g, dtype=torch.float64)
    x[1, 2] = 0.0
    w = 1.0 + 0.1 * torch.randn(64, generator=g, dtype=torch.float64)
    w[33] = 0.0
    fr = torch.arange(5, dtype=torch.float64)[:, None] * torch.rand(32, generator=g, dtype=torch.float64)[None, :]
    y = ref.qknorm_rope(x, w, fr.cos(), fr.sin(), 1e-6)
    assert bool(torch.isfinite(y).all()) and not bool(y[1, 2].any())
    # position 0 rotates nothing: the plain norm; a rotation keeps every pair's length
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w
    assert torch.allclose(y[:, 0], n[:, 0], rtol=0, atol=1e-15)
    assert torch.allclose(y[..., :32] ** 2 + y[..., 32:] ** 2, n[..., :32] ** 2 + n[..., 32:] ** 2, rtol=1e-12, atol=1e-15)
    assert float(n[..., 33].abs().max()) == 0.0                          # the zero weight entry


@pytest.mark.parametrize("name", ["tiny", "qwen2_tiny", "tiny64"])
def test_weights_of_earlier_shapes_are_unchanged(name):
    """make_llama_weights draws the q / k norm after everything else and only under qk_norm: an earlier shape gets, tensor for tensor,
    what the generator gives with the norm branch disabled, and no norm tensor."""
    from astts.llm import weights
    from astts.llm.config import LlamaShape
    cfg = getattr(LlamaShape, name)()
    sd = weights.make_llama_weights(cfg, 7)
    assert not [k for k in sd if "q_norm" in k or "k_norm" in k]
    first, last = next(iter(sd)), list(sd)[-1]
    g = torch.Generator().manual_seed(7)
    assert torch.equal(sd[first], torch.randn(cfg.vocab, cfg.hidden, generator=g) * 0.5) and first == "model.embed_tokens.weight"
    # the same shape with the flag raised and the branch disabled (no outlier table, the draw skipped) must not differ anywhere
    on = weights.make_llama_weights(dataclasses.replace(cfg, qk_norm=True), 7)
    assert list(on)[:len(sd)] == list(sd) and all(torch.equal(on[k], sd[k]) for k in sd)
    assert torch.equal(on[last], sd[last])
    extra = [k for k in on if k not in sd]
    assert len(extra) == 2 * cfg.layers and all(on[k].shape == (cfg.head_dim,) for k in extra)
    w = on["model.layers.0.self_attn.q_norm.weight"]
    for at, val in weights.QK_NORM_OUTLIERS:
        assert float(w[at % cfg.head_dim]) == float(torch.tensor(val))
    assert {0.0, 0.02, 8.0} <= {v for _, v in weights.QK_NORM_OUTLIERS}


def _write(tmp_path, cfg, **over):
    c = ref.config_json(cfg)
    c.update(over)
    d = tmp_path / f"cfg{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(c))
    return str(d)


def test_shape_from_config_accepts_qwen3_and_refuses_by_key(tmp_path):
    from astts.llm.config import LlamaShape
    from astts.llm.peft import ConfigError, shape_from_config
    cfg = LlamaShape.qwen3_tiny()
    got = shape_from_config(_write(tmp_path, cfg))
    assert got.head_dim == 128 and got.hidden == 640 and got.heads * got.head_dim == 1024          # head_dim is read, not hidden / heads (80)
    assert got.qk_norm and not got.qkv_bias and got.model_type == "qwen3" and got.rope_type == "default" and got.tie_embeddings
    assert dataclasses.replace(got, max_positions=cfg.max_positions) == cfg
    assert shape_from_config(_write(tmp_path, cfg, attention_bias=True)).qkv_bias
    assert not shape_from_config(_write(tmp_path, LlamaShape.qwen3_tiny_untied(), head_dim=64)).tie_embeddings
    conf = ref.config_json(cfg)
    del conf["head_dim"]                                   # transformers' Qwen3Config: an absent head_dim is 128, never hidden / heads
    (tmp_path / "nohd").mkdir()
    (tmp_path / "nohd" / "config.json").write_text(json.dumps(conf))
    assert shape_from_config(str(tmp_path / "nohd")).head_dim == 128
    with pytest.raises(ConfigError, match="layer_types.*sliding_attention"):
        shape_from_config(_write(tmp_path, cfg, layer_types=["full_attention", "sliding_attention", "full_attention"]))
    with pytest.raises(ConfigError, match="use_sliding_window"):
        shape_from_config(_write(tmp_path, cfg, use_sliding_window=True))
    with pytest.raises(ConfigError, match="model_type='qwen3_moe'"):
        shape_from_config(_write(tmp_path, cfg, model_type="qwen3_moe"))
    with pytest.raises(ConfigError, match="rope_scaling.*yarn"):
        shape_from_config(_write(tmp_path, cfg, rope_scaling={"rope_type": "yarn", "factor": 4.0}))
    # a Llama or Qwen2 config never gets the norm
    from qwen2_ref import config_json as q2_config
    d = tmp_path / "q2"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(q2_config(LlamaShape.qwen2_tiny())))
    assert not shape_from_config(str(d)).qk_norm


def test_model_type_that_contradicts_architectures_is_refused(tmp_path):
    """The families differ in tensors (biases, q / k norms), not in shapes: a config.json whose ``architectures`` names another family's
    class than its ``model_type`` is refused naming both keys, in every direction; other or absent classes decide nothing."""
    from qwen2_ref import config_json as q2_config
    from astts.llm.config import LlamaShape
    from astts.llm.peft import ConfigError, shape_from_config
    q3, q2 = LlamaShape.qwen3_tiny(), q2_config(LlamaShape.qwen2_tiny())
    for over in (dict(architectures=["Qwen2ForCausalLM"]), dict(architectures=["LlamaForCausalLM"]), dict(model_type="qwen2"), dict(model_type="llama")):
        with pytest.raises(ConfigError, match="model_type=.*contradicts architectures"):
            shape_from_config(_write(tmp_path, q3, **over))
    for i, over in enumerate((dict(model_type="qwen3"), dict(model_type="llama"), dict(architectures=["Qwen3ForCausalLM"]))):
        d = tmp_path / f"q2_{i}"
        d.mkdir()
        (d / "config.json").write_text(json.dumps({**q2, **over}))
        with pytest.raises(ConfigError, match="model_type=.*contradicts architectures"):
            shape_from_config(str(d))
    assert shape_from_config(_write(tmp_path, q3, architectures=["Qwen3ForSequenceClassification"])).qk_norm
    conf = ref.config_json(q3)
    del conf["architectures"]
    (tmp_path / "noarch").mkdir()
    (tmp_path / "noarch" / "config.json").write_text(json.dumps(conf))
    assert shape_from_config(str(tmp_path / "noarch")) == shape_from_config(_write(tmp_path, q3))


def test_new_entry_points_are_declared_and_check_their_arguments():
    from astts import _lib, _lib_llm, _lib_train
    assert list(_lib_llm.signatures()) == ["astts_op_qknorm_rope"] and "astts_op_qknorm_rope" not in _lib.declared_symbols()
    assert "astts_train_qknorm_rope_bwd" in _lib_train.declared_symbols()
    lib, tlib = _lib_llm.load(), _lib_train.load()
    assert lib.astts_abi_version() == 6 and tlib.astts_train_abi_version() == 1
    P = 0x10000                                              # fake non-NULL pointers: every case is refused on the host
    fwd = lambda **kw: lib.astts_op_qknorm_rope(*[{**dict(x=P, c=P, s=P, qw=P, kw=P, shift=None, b=1, t=1, tm=0, heads=2, kv=1, ld=384, hd=128,
                                                          pos0=0, eps=1e-6, st=None), **kw}[k]
                                                  for k in ("x", "c", "s", "qw", "kw", "shift", "b", "t", "tm", "heads", "kv", "ld", "hd", "pos0", "eps", "st")])
    assert fwd(x=None) == _lib.ERR_INVALID and fwd(qw=None) == _lib.ERR_INVALID
    for hd in (32, 96, 256):
        assert fwd(hd=hd, ld=3 * hd) == _lib.ERR_UNSUPPORTED
    assert b"head_dim" in lib.astts_last_error_string()
    assert fwd(ld=383) == _lib.ERR_INVALID and fwd(ld=376) == _lib.ERR_INVALID and fwd(x=P + 8) == _lib.ERR_INVALID and fwd(pos0=-1) == _lib.ERR_INVALID
    bwd = lambda **kw: tlib.astts_train_qknorm_rope_bwd(*[{**dict(d=P, ldd=512, x=P, ldx=384, c=P, s=P, qw=P, kw=P, b=1, t=1, heads=2, kv=1, hd=128,
                                                                 pos0=0, eps=1e-6, st=None), **kw}[k]
                                                         for k in ("d", "ldd", "x", "ldx", "c", "s", "qw", "kw", "b", "t", "heads", "kv", "hd", "pos0", "eps", "st")])
    assert bwd(x=None) == _lib.ERR_INVALID and bwd(hd=80) == _lib.ERR_UNSUPPORTED and bwd(ldx=380) == _lib.ERR_INVALID and bwd(ldd=256) == _lib.ERR_INVALID
    assert b"qknorm_rope_bwd" in tlib.astts_train_last_error_string()
