"""CPU checks of the LLM.int8 + LoRA restatement (tests/llm_int8_ref.py) and of the PEFT adapter loader (astts.llm.peft): the
restatement against the fp32 oracle, quantisation on hand-built data, the adapter directory format and every refusal."""
import json
import math
import os
import socket

import pytest
import torch

import llm_int8_ref as ref


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_with_lora_and_no_int8_equals_the_merged_oracle():
    import oracle.llama as ol
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights

    cfg = LlamaShape.tiny()
    sd = make_llama_weights(cfg, 0)
    lora = ref.make_lora(cfg, 8, 2, std_a=0.05, std_b=0.05)
    sc = ref.lora_scaling(8, 32)
    ids = torch.randint(3, cfg.vocab, (13,), generator=torch.Generator().manual_seed(0))
    got = ref.Decoder(sd, cfg, ref.make_linear(sd, cfg, lora, sc, int8=False), 0.0).step(ids)
    want = ol.forward_hidden(ref.merged(sd, lora, sc), cfg, ids[None])[0]
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-5
    # and the LoRA branch matters
    plain = ol.forward_hidden(sd, cfg, ids[None])[0]
    assert float((plain - want).abs().max()) > 1e-3
    # prefill + one-token steps give the same hidden states as one pass
    d = ref.Decoder(sd, cfg, ref.make_linear(sd, cfg, lora, sc, int8=False), 0.0)
    h = torch.cat([d.step(ids[:9]), d.step(ids[9:10]), d.step(ids[10:])])
    assert float((h - got).abs().max() / got.abs().max()) <= 1e-5


def test_weight_quantisation_by_hand():
    w = torch.tensor([[1.0, -0.5, 0.25, 0.0], [0.0, 0.0, 0.0, 0.0], [3.0, 1.5, -0.75, 0.006]])
    cb, scb = ref.quant_weight(w)
    assert scb.tolist() == [1.0, 0.0, 3.0]
    assert cb.tolist() == [[127, -64, 32, 0], [0, 0, 0, 0], [127, 64, -32, 0]]     # 63.5 -> 64, 31.75 -> 32 (round half to even: 63.5 -> 64)


def test_activation_quantisation_by_hand():
    tau = 6.0
    x = torch.tensor([[1.0, 7.0, -2.0, 0.5],      # segment 0: outlier at column 1
                      [2.0, 0.5, -1.0, 0.0],      # segment 0: column 1 zeroed though 0.5 < tau; SCA still counts it
                      [0.0, 0.0, 0.0, 0.0],       # segment 1: all zero -> SCA 0, CA 0
                      [6.0, -9.0, 6.5, 8.0],      # segment 2: every element an outlier -> SCA 0
                      [1.0, 2.0, 3.0, 64.0],      # pad row: its own element >= tau zeroed, no outlier term
                      [4.0, -1.0, 0.5, 2.0]],     # segment 3, a one-row segment
                     dtype=torch.float16)
    seg = torch.tensor([0, 0, 1, 2, -1, 3])
    ca, sca, zeroed, outl = ref.quant_act(x, seg, tau)
    assert sca.tolist() == [2.0, 2.0, 0.0, 0.0, 3.0, 4.0]
    assert ca.tolist() == [[64, 0, -127, 32], [127, 0, -64, 0], [0] * 4, [0] * 4, [42, 85, 127, 0], [127, -32, 16, 64]]
    assert ref.outlier_columns(outl, seg) == {0: [1], 1: [], 2: [0, 1, 2, 3], 3: []}
    assert not outl[4].any() and zeroed[4].tolist() == [False, False, False, True]
    # rows == 1: one row per segment is bitsandbytes' single-row path: the columns are the row's own
    _, _, _, o1 = ref.quant_act(x, torch.arange(6), tau)
    assert ref.outlier_columns(o1, torch.arange(6))[1] == []
    # tau <= 0: no decomposition, SCA is the plain absmax
    ca0, sca0, z0, o0 = ref.quant_act(x, seg, 0.0)
    assert not o0.any() and not z0.any() and sca0.tolist() == [7.0, 2.0, 0.0, 9.0, 64.0, 4.0]


def test_int8_linear_decomposition_is_exact_where_it_should_be():
    """With every column an outlier, y = X (CB SCB / 127)^T exactly: the base term is zero."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(5, 8, generator=g)
    cb, scb = ref.quant_weight(w)
    x = (torch.randn(3, 8, generator=g) * 10 + 20).to(torch.float16)       # every |x| >= 6
    y = ref.int8_linear(x, cb, scb, torch.zeros(3, dtype=torch.long), 6.0)
    assert torch.allclose(y, x.double() @ (cb.double() * scb.double()[:, None] / 127).T, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ the loader
@pytest.fixture()
def dirs(tmp_path):
    from astts.llm.config import LlamaShape
    from astts.llm.weights import make_llama_weights

    cfg = LlamaShape.tiny()
    sd = make_llama_weights(cfg, 0)
    base = ref.write_base(str(tmp_path / "base"), cfg, sd, eos_ids=[2, 7])
    lora = ref.make_lora(cfg, 4, 3)
    return cfg, sd, base, lora, tmp_path


def test_adapter_keys_map_to_layers_and_projections(dirs):
    from astts.llm.peft import is_adapter_dir, load_peft_model

    cfg, sd, base, lora, tmp = dirs
    ada = ref.write_adapter(str(tmp / "ad"), lora, r=4, alpha=16, base=base)
    assert is_adapter_dir(ada) and not is_adapter_dir(base)
    state, cfg2, ad, bdir = load_peft_model(ada)                        # base_model_name_or_path is a directory
    assert bdir == base and ad.scaling == 4.0 and set(ad.targets) == {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"}
    assert len(ad.pairs) == 7 * cfg.layers
    a, b = ad.pairs[(1, "down_proj")]
    assert torch.equal(a, lora[(1, "down")][0]) and torch.equal(b, lora[(1, "down")][1])
    assert (cfg2.hidden, cfg2.layers, cfg2.heads, cfg2.kv_heads, cfg2.ffn, cfg2.vocab) == (cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads, cfg.ffn, cfg.vocab)
    assert cfg2.eos_token_ids == (2, 7) and cfg2.tie_embeddings
    assert torch.equal(state["model.layers.0.self_attn.q_proj.weight"], sd["model.layers.0.self_attn.q_proj.weight"].half().float())


def test_rslora_scaling(dirs):
    from astts.llm.peft import load_adapter

    cfg, sd, base, lora, tmp = dirs
    ad = load_adapter(ref.write_adapter(str(tmp / "ad"), lora, r=4, alpha=16, use_rslora=True, base=base))
    assert ad.scaling == 16 / math.sqrt(4) == ref.lora_scaling(4, 16, True)


def test_target_modules_list_and_regex(dirs):
    from astts.llm.peft import load_adapter

    cfg, sd, base, lora, tmp = dirs
    sub = {k: v for k, v in lora.items() if k[1] in ("q", "v")}
    ad = load_adapter(ref.write_adapter(str(tmp / "a1"), sub, r=4, target_modules=["q_proj", "v_proj"], base=base))
    assert ad.targets == ("q_proj", "v_proj") and len(ad.pairs) == 2 * cfg.layers
    ad = load_adapter(ref.write_adapter(str(tmp / "a2"), sub, r=4, target_modules=r".*\.(q_proj|v_proj)", base=base))
    assert ad.targets == ("q_proj", "v_proj")


def test_resized_vocabulary_from_the_adapter(dirs):
    from astts.llm.peft import load_peft_model

    cfg, sd, base, lora, tmp = dirs
    emb = torch.randn(cfg.vocab + 3, cfg.hidden)
    ada = ref.write_adapter(str(tmp / "ad"), lora, r=4, base=base, embed=emb, lm_head=emb * 0.5)
    state, cfg2, ad, _ = load_peft_model(ada, tokenizer_size=cfg.vocab + 3)
    assert cfg2.vocab == cfg.vocab + 3 and not cfg2.tie_embeddings
    assert torch.equal(state["model.embed_tokens.weight"], emb.half().float())
    assert torch.equal(state["lm_head.weight"], (emb * 0.5).half().float())
    # the same table as lm_head in a tied base: stays tied
    ada2 = ref.write_adapter(str(tmp / "ad2"), lora, r=4, base=base, embed=emb, lm_head=emb)
    assert load_peft_model(ada2)[1].tie_embeddings


@pytest.mark.parametrize("case", ["dora", "bias", "unknown_target", "extra_key", "fan_in_fan_out", "modules_to_save", "tokenizer_size",
                                  "missing_half"])
def test_refusals(dirs, case):
    from astts.llm.peft import AdapterError, load_peft_model

    cfg, sd, base, lora, tmp = dirs
    kw, tok = {}, None
    if case == "dora":
        kw["extra_config"] = {"use_dora": True}
    elif case == "bias":
        kw["extra_config"] = {"bias": "lora_only"}
    elif case == "unknown_target":
        kw["target_modules"] = ["q_proj", "lm_head"]
    elif case == "extra_key":
        kw["extra_keys"] = {"base_model.model.model.layers.0.self_attn.q_proj.lora_magnitude_vector": torch.ones(4)}
    elif case == "fan_in_fan_out":
        kw["extra_config"] = {"fan_in_fan_out": True}
    elif case == "modules_to_save":
        kw["extra_config"] = {"modules_to_save": ["score"]}
    elif case == "tokenizer_size":
        tok = cfg.vocab + 1
    elif case == "missing_half":
        kw["extra_keys"] = {"base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight": torch.ones(4, cfg.hidden)}
        lora = {k: v for k, v in lora.items() if k != (0, "q")}
    ada = ref.write_adapter(str(tmp / "ad"), lora, r=4, base=base, **kw)
    with pytest.raises(AdapterError):
        load_peft_model(ada, tokenizer_size=tok)


def test_base_resolution_order_and_no_network(dirs, monkeypatch):
    from astts.llm import peft

    cfg, sd, base, lora, tmp = dirs

    def no_net(*a, **k):
        raise AssertionError("the loader touched the network")

    monkeypatch.setattr(socket, "socket", no_net)
    monkeypatch.setattr(socket, "create_connection", no_net)
    ada = ref.write_adapter(str(tmp / "ad"), lora, r=4, base="some-org/Llama-3.2-3B-Instruct")
    ad = peft.load_adapter(ada)
    # 1. the flag wins
    other = ref.write_base(str(tmp / "other"), cfg, sd)
    assert peft.resolve_base(ad, other) == other
    # 3. nothing local: the message names the hub id and the flag
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp / "hub"))
    monkeypatch.setenv("HOME", str(tmp / "home"))
    monkeypatch.delenv("HF_HOME", raising=False)
    monkeypatch.delenv("HUGGINGFACE_HUB_CACHE", raising=False)
    with pytest.raises(FileNotFoundError, match=r"some-org/Llama-3\.2-3B-Instruct.*--base_model_path"):
        peft.resolve_base(ad)
    # a local hub-cache snapshot
    snap = tmp / "hub" / "models--some-org--Llama-3.2-3B-Instruct" / "snapshots" / "abc123"
    ref.write_base(str(snap), cfg, sd)
    (tmp / "hub" / "models--some-org--Llama-3.2-3B-Instruct" / "refs").mkdir()
    (tmp / "hub" / "models--some-org--Llama-3.2-3B-Instruct" / "refs" / "main").write_text("abc123")
    assert peft.resolve_base(ad) == str(snap)
    # 2. base_model_name_or_path as a directory comes before the cache
    ad.base_model_name_or_path = base
    assert peft.resolve_base(ad) == base
    with pytest.raises(FileNotFoundError):
        peft.resolve_base(ad, str(tmp / "nope"))


def test_merged_directories_load_as_before(dirs):
    from astts.llm.peft import is_adapter_dir
    from astts.llm.weights import load_llama_weights

    cfg, sd, base, lora, tmp = dirs
    assert not is_adapter_dir(base)
    st = load_llama_weights(base)
    assert set(st) == set(sd) and all(torch.equal(st[k], sd[k].half().float()) for k in sd)


def test_cli_flags():
    from astts.cli import search_json, search_milvus

    a = search_json.build_parser().parse_args(["--input_json", "x", "--model_path", "ad", "--base_model_path", "b", "--llm_precision", "fp16"])
    assert (a.model_path, a.base_model_path, a.llm_precision) == ("ad", "b", "fp16")
    a = search_milvus.build_parser().parse_args(["--model_path", "ad"])
    assert a.base_model_path is None and a.llm_precision is None
    with pytest.raises(SystemExit):
        search_milvus.build_parser().parse_args(["--llm_precision", "nf4"])
