"""PEFT LoRA adapter directories for the embedder: the reference retrieves with one (``--model_path`` = the output of src/ft_llm.py:
LoRA r=32, lora_alpha=128, target_modules="all-linear", bias="none", on a vocabulary resized by trl's setup_chat_format), loaded by
``AutoPeftModelForCausalLM.from_pretrained(..., quantization_config=BitsAndBytesConfig(load_in_8bit=True))``
(milvus/search_json.py:31-70, src/search_milvus.py:36-72).

Restated from peft's published behaviour (neither peft nor bitsandbytes is needed): adapter_config.json + adapter_model.safetensors
(or adapter_model.bin) with keys ``base_model.model.model.layers.{i}.<proj>.lora_{A,B}.weight``; LoRA scaling ``lora_alpha / r``
(``/ sqrt(r)`` with use_rslora); the resized ``embed_tokens`` / ``lm_head`` when saved alongside.  The base checkpoint is resolved
locally only -- nothing is ever fetched."""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass, field, replace
from typing import Dict, Optional, Tuple

import torch

from .config import LlamaShape
from .weights import StateDict, load_llama_weights

PROJ = {"q_proj": "self_attn.q_proj", "k_proj": "self_attn.k_proj", "v_proj": "self_attn.v_proj", "o_proj": "self_attn.o_proj",
        "gate_proj": "mlp.gate_proj", "up_proj": "mlp.up_proj", "down_proj": "mlp.down_proj"}
_KEY = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\.(\w+)\.lora_([AB])\.weight$")
_EMBED_KEYS = ("base_model.model.model.embed_tokens.weight", "base_model.model.model.embed_tokens.modules_to_save.weight")
_HEAD_KEYS = ("base_model.model.lm_head.weight", "base_model.model.lm_head.modules_to_save.weight")


class AdapterError(ValueError):
    """An adapter directory this port refuses to load (and why)."""


def is_adapter_dir(path: str) -> bool:
    return bool(path) and os.path.isfile(os.path.join(path, "adapter_config.json"))


@dataclass
class LoraAdapter:
    r: int
    lora_alpha: float
    use_rslora: bool
    targets: Tuple[str, ...]                       # of PROJ's keys
    base_model_name_or_path: str
    pairs: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]] = field(default_factory=dict)   # (layer, proj) -> (A [r, in], B [out, r]) fp32
    embed: Optional[torch.Tensor] = None           # resized embed_tokens [vocab', hidden]
    lm_head: Optional[torch.Tensor] = None

    @property
    def scaling(self) -> float:
        return self.lora_alpha / math.sqrt(self.r) if self.use_rslora else self.lora_alpha / self.r


def _targets(tm) -> Tuple[str, ...]:
    """peft's target_modules: "all-linear" (every linear but the output layer: the seven projections), a list of module names, or a
    string matched in full against the module path."""
    if tm is None:
        raise AdapterError("adapter_config.json has no target_modules")
    if isinstance(tm, str):
        if tm == "all-linear":
            return tuple(PROJ)
        hit = tuple(p for p, full in PROJ.items() if re.fullmatch(tm, f"model.layers.0.{full}") or re.fullmatch(tm, p))
        if not hit:
            raise AdapterError(f"target_modules regex {tm!r} matches none of {sorted(PROJ)}")
        return hit
    names = [str(t) for t in tm]
    unknown = [t for t in names if t.split(".")[-1] not in PROJ]
    if unknown:
        raise AdapterError(f"unsupported LoRA target modules {unknown}: this port applies LoRA to {sorted(PROJ)} only")
    return tuple(p for p in PROJ if p in {t.split(".")[-1] for t in names})


def load_adapter(path: str) -> LoraAdapter:
    """Read and validate an adapter directory (CPU tensors, fp32)."""
    with open(os.path.join(path, "adapter_config.json")) as f:
        conf = json.load(f)
    if conf.get("peft_type", "LORA") != "LORA":
        raise AdapterError(f"peft_type {conf.get('peft_type')!r}: only LoRA adapters are supported")
    if conf.get("use_dora"):
        raise AdapterError("use_dora=True: DoRA adapters are not supported")
    if conf.get("bias", "none") != "none":
        raise AdapterError(f"bias={conf.get('bias')!r}: only bias='none' adapters are supported")
    if conf.get("fan_in_fan_out"):
        raise AdapterError("fan_in_fan_out=True: transposed (Conv1D) LoRA weights are not supported for Llama")
    mts = conf.get("modules_to_save") or []
    bad = [m for m in mts if m not in ("embed_tokens", "lm_head")]
    if bad:
        raise AdapterError(f"modules_to_save {bad}: only the resized embed_tokens / lm_head are supported")
    r = int(conf["r"])
    ad = LoraAdapter(r=r, lora_alpha=float(conf.get("lora_alpha", 8)), use_rslora=bool(conf.get("use_rslora", False)),
                     targets=_targets(conf.get("target_modules")), base_model_name_or_path=str(conf.get("base_model_name_or_path") or ""))
    st = os.path.join(path, "adapter_model.safetensors")
    if os.path.isfile(st):
        from safetensors.torch import load_file

        sd = load_file(st, device="cpu")
    elif os.path.isfile(os.path.join(path, "adapter_model.bin")):
        sd = torch.load(os.path.join(path, "adapter_model.bin"), map_location="cpu", weights_only=True)
    else:
        raise AdapterError(f"no adapter_model.safetensors / adapter_model.bin under {path!r}")
    halves: Dict[Tuple[int, str], dict] = {}
    for k, v in sd.items():
        if k in _EMBED_KEYS:
            ad.embed = v.float()
            continue
        if k in _HEAD_KEYS:
            ad.lm_head = v.float()
            continue
        m = _KEY.match(k)
        if not m or m.group(3) not in PROJ or PROJ[m.group(3)] != f"{m.group(2)}.{m.group(3)}":
            raise AdapterError(f"unexpected key {k!r} in the adapter (DoRA magnitudes, biases, other modules or adapter names are not "
                               "supported)")
        if m.group(3) not in ad.targets:
            raise AdapterError(f"key {k!r} is for a module outside target_modules {list(ad.targets)}")
        halves.setdefault((int(m.group(1)), m.group(3)), {})[m.group(4)] = v.float()
    for (i, p), ab in halves.items():
        if set(ab) != {"A", "B"}:
            raise AdapterError(f"layer {i} {p}: lora_A and lora_B must both be present")
        a, b = ab["A"], ab["B"]
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != r or b.shape[1] != r:
            raise AdapterError(f"layer {i} {p}: LoRA shapes A {tuple(a.shape)} B {tuple(b.shape)} do not match r={r}")
        ad.pairs[(i, p)] = (a, b)
    return ad


def hf_cache_snapshot(repo_id: str) -> Optional[str]:
    """The local Hugging Face hub cache's snapshot of ``repo_id`` (what ``local_files_only=True`` resolves to), or None.  Reads the
    cache directory only."""
    if not repo_id or "/" not in repo_id:
        return None
    roots = [os.environ.get("HF_HUB_CACHE"), os.environ.get("HUGGINGFACE_HUB_CACHE"),
             os.path.join(os.environ["HF_HOME"], "hub") if os.environ.get("HF_HOME") else None,
             os.path.join(os.path.expanduser("~"), ".cache", "huggingface", "hub")]
    folder = "models--" + repo_id.replace("/", "--")
    for root in roots:
        if not root:
            continue
        d = os.path.join(root, folder)
        snaps = os.path.join(d, "snapshots")
        if not os.path.isdir(snaps):
            continue
        ref = os.path.join(d, "refs", "main")
        if os.path.isfile(ref):
            with open(ref) as f:
                s = os.path.join(snaps, f.read().strip())
            if os.path.isfile(os.path.join(s, "config.json")):
                return s
        for s in sorted(os.listdir(snaps)):
            if os.path.isfile(os.path.join(snaps, s, "config.json")):
                return os.path.join(snaps, s)
    return None


def resolve_base(adapter: LoraAdapter, base_model_path: Optional[str] = None) -> str:
    """--base_model_path, else base_model_name_or_path when it is a directory, else the local hub cache.  Never fetches."""
    if base_model_path:
        if not os.path.isdir(base_model_path):
            raise FileNotFoundError(f"--base_model_path {base_model_path!r} is not a directory")
        return base_model_path
    name = adapter.base_model_name_or_path
    if name and os.path.isdir(name):
        return name
    snap = hf_cache_snapshot(name)
    if snap:
        return snap
    raise FileNotFoundError(f"the adapter's base model {name!r} is not available locally (no such directory and no local hub cache "
                            f"snapshot); download it yourself and pass --base_model_path <dir>")


class ConfigError(ValueError):
    """A config.json this port refuses to run (and which key says so)."""


ARCHITECTURES = {"LlamaForCausalLM": "llama", "Qwen2ForCausalLM": "qwen2", "Qwen3ForCausalLM": "qwen3"}   # transformers class -> model_type


def shape_from_config(base_dir: str, vocab: Optional[int] = None) -> LlamaShape:
    """LlamaShape from a transformers config.json (``vocab``: the row count of the embedding table in use).  ``model_type`` llama,
    qwen2 or qwen3 (full-attention layers only; an absent ``head_dim`` is 128 there, transformers' Qwen3Config default, not hidden / heads);
    RoPE plain (no ``rope_scaling``) or Llama-3 scaled.  Anything that would run but compute another model is refused by key."""
    with open(os.path.join(base_dir, "config.json")) as f:
        c = json.load(f)
    model_type = str(c.get("model_type", "llama"))
    if model_type not in ("llama", "qwen2", "qwen3"):
        raise ConfigError(f"config.json model_type={model_type!r}: only 'llama', 'qwen2' and 'qwen3' checkpoints are supported")
    # the three families differ in tensors, not in shapes (q / k / v biases, q / k norms): a config whose `architectures` names the
    # class of ANOTHER of them would load that family's weights under this one's rules
    claimed = sorted({ARCHITECTURES[a] for a in (c.get("architectures") or ()) if a in ARCHITECTURES} - {model_type})
    if claimed:
        raise ConfigError(f"config.json model_type={model_type!r} contradicts architectures={c['architectures']} (a {claimed[0]} class): "
                          "which family's weights the directory holds is not decidable from it")
    if c.get("use_sliding_window"):
        raise ConfigError("config.json use_sliding_window=true: sliding-window attention is not built")
    other = sorted({str(k) for k in (c.get("layer_types") or ()) if k != "full_attention"})
    if other:
        raise ConfigError(f"config.json layer_types contains {other}: only 'full_attention' layers are built")
    if c.get("mlp_bias"):
        raise ConfigError("config.json mlp_bias=true: biases on the MLP projections are not built")
    rp = c.get("rope_parameters") if isinstance(c.get("rope_parameters"), dict) else {}      # transformers >= 5: theta and scaling in one
    rs_key = "rope_scaling" if c.get("rope_scaling") else "rope_parameters"
    rs = c.get("rope_scaling") or rp
    kind = str(rs.get("rope_type", rs.get("type", "default")))
    if kind not in ("default", "llama3"):
        raise ConfigError(f"config.json {rs_key} type {kind!r}: only plain RoPE (no rope_scaling) and 'llama3' scaling are built")
    d = LlamaShape()
    heads = int(c["num_attention_heads"])
    eos = c.get("eos_token_id", d.eos_token_id)
    eos_l = list(eos) if isinstance(eos, (list, tuple)) else [eos]
    return LlamaShape(vocab=int(vocab or c["vocab_size"]), hidden=int(c["hidden_size"]), layers=int(c["num_hidden_layers"]), heads=heads,
                      kv_heads=int(c.get("num_key_value_heads", heads)), head_dim=int(c.get("head_dim") or (128 if model_type == "qwen3" else c["hidden_size"] // heads)),
                      ffn=int(c["intermediate_size"]), rms_eps=float(c.get("rms_norm_eps", d.rms_eps)),
                      rope_theta=float(c.get("rope_theta", rp.get("rope_theta", d.rope_theta))), rope_factor=float(rs.get("factor", d.rope_factor)),
                      rope_low_freq_factor=float(rs.get("low_freq_factor", d.rope_low_freq_factor)),
                      rope_high_freq_factor=float(rs.get("high_freq_factor", d.rope_high_freq_factor)),
                      rope_original_max_pos=int(rs.get("original_max_position_embeddings", d.rope_original_max_pos)),
                      max_positions=int(c.get("max_position_embeddings", d.max_positions)),
                      tie_embeddings=bool(c.get("tie_word_embeddings", d.tie_embeddings)), eos_token_id=int(eos_l[0]),
                      bos_token_id=int(c.get("bos_token_id", d.bos_token_id) if c.get("bos_token_id") is not None else d.bos_token_id),
                      model_type=model_type, qkv_bias=True if model_type == "qwen2" else bool(c.get("attention_bias", False)),
                      rope_type=kind, qk_norm=model_type == "qwen3")


def generation_eos_ids(base_dir: str) -> Tuple[int, ...]:
    """eos_token_id of generation_config.json (int or list: generate stops at any of them), () when absent."""
    p = os.path.join(base_dir, "generation_config.json")
    if not os.path.isfile(p):
        return ()
    with open(p) as f:
        e = json.load(f).get("eos_token_id")
    if e is None:
        return ()
    return tuple(int(i) for i in (e if isinstance(e, (list, tuple)) else [e]))


def load_peft_model(adapter_dir: str, base_model_path: Optional[str] = None,
                    tokenizer_size: Optional[int] = None) -> Tuple[StateDict, LlamaShape, LoraAdapter, str]:
    """Adapter directory -> (base state dict with the adapter's resized tables in place, shape, adapter, base directory).
    ``tokenizer_size``: len(tokenizer) of the adapter directory's tokenizer, checked against the embedding table."""
    ad = load_adapter(adapter_dir)
    base = resolve_base(ad, base_model_path)
    state = load_llama_weights(base)
    if ad.embed is not None:
        state["model.embed_tokens.weight"] = ad.embed
    vocab = int(state["model.embed_tokens.weight"].shape[0])
    cfg = shape_from_config(base, vocab)
    if ad.lm_head is not None:
        if ad.lm_head.shape[0] != vocab:
            raise AdapterError(f"the adapter's lm_head has {ad.lm_head.shape[0]} rows, its embed_tokens {vocab}")
        if not (cfg.tie_embeddings and torch.equal(ad.lm_head, state["model.embed_tokens.weight"])):
            state["lm_head.weight"] = ad.lm_head
            cfg = replace(cfg, tie_embeddings=False)
    elif not cfg.tie_embeddings and state["lm_head.weight"].shape[0] != vocab:
        raise AdapterError(f"embed_tokens has {vocab} rows but the base's lm_head {state['lm_head.weight'].shape[0]}: the adapter "
                           "resized the vocabulary without saving lm_head")
    if tokenizer_size is not None and int(tokenizer_size) > vocab:
        raise AdapterError(f"the tokenizer has {tokenizer_size} tokens but embed_tokens only {vocab} rows: the adapter's resized "
                           "embedding table is missing (save_embedding_layers) or belongs to another tokenizer")
    for (i, p), (a, b) in ad.pairs.items():
        w = state.get(f"model.layers.{i}.{PROJ[p]}.weight")
        if w is None or i >= cfg.layers:
            raise AdapterError(f"adapter layer {i} {p} has no counterpart in the base model")
        if a.shape[1] != w.shape[1] or b.shape[0] != w.shape[0]:
            raise AdapterError(f"layer {i} {p}: LoRA A {tuple(a.shape)} / B {tuple(b.shape)} do not fit the weight {tuple(w.shape)}")
    cfg = replace(cfg, eos_token_ids=generation_eos_ids(base))
    return state, cfg, ad, base
