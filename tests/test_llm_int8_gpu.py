"""LLM.int8 + LoRA on the GPU (csrc/ops_int8.hip, astts.ops.Int8Weight, LlamaEmbedder(int8=True, lora=...)) against the torch
restatement of tests/llm_int8_ref.py: quantisation bit-exact, the GEMM to 1e-6 of the fp64 restatement, the embedder end to end,
the CLIs on an adapter directory, and one full-depth 3.2-3B-shaped pass."""
import json
import os

import numpy as np
import pytest
import torch

import llm_int8_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _x(m, k, seed, outlier_cols=(), outlier_rows=None, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g) * scale
    for c in outlier_cols:
        rows = range(m) if outlier_rows is None else outlier_rows
        for r in rows:
            x[r, c] = 8.0 + (r % 5)
    return x.to(torch.float16)


def _seg_right(lens, t):
    return torch.tensor([b if i < n else -1 for b, n in enumerate(lens) for i in range(t)], dtype=torch.int32)


def _seg_time_major(lens, t):
    b = len(lens)
    return torch.tensor([j if i >= t - lens[j] else -1 for i in range(t) for j in range(b)], dtype=torch.int32)


def test_weight_quantisation_is_bit_exact():
    from astts import ops

    g = torch.Generator().manual_seed(0)
    w = torch.randn(300, 200, generator=g) * 0.05
    w[7] = 0.0                                   # SCB = 0
    w[9, 3] = 70000.0 / 1e4                      # one large entry dominates its row
    cb, scb = ops.i8_quantize_weight(w.to(DEV))
    rcb, rscb = ref.quant_weight(w)
    assert cb.shape == (384, 256) and scb.shape == (384,)
    assert torch.equal(cb[:300, :200].cpu(), rcb) and torch.equal(scb[:300].cpu(), rscb)
    assert not cb[300:].any() and not cb[:, 200:].any() and not scb[300:].any()
    cb16, scb16 = ops.i8_quantize_weight(w.to(torch.float16).to(DEV))
    assert torch.equal(cb16, cb) and torch.equal(scb16, scb)


@pytest.mark.parametrize("layout", ["right_padded", "time_major", "rows", "tau_off"])
def test_activation_quantisation_is_bit_exact(layout):
    from astts import ops

    k, tau = 200, 6.0                            # K not a multiple of 64
    lens, t = [5, 3, 7], 7
    if layout == "right_padded":
        seg = _seg_right(lens, t)
    elif layout == "time_major":
        seg = _seg_time_major(lens, t)
    else:
        seg = torch.arange(9, dtype=torch.int32)
    if layout == "tau_off":
        tau = 0.0
    m = seg.numel()
    x = _x(m, k, 1, outlier_cols=(3, 150), outlier_rows=[0, 4, m - 2])
    x[1] = 0.0                                    # SCA = 0
    x[2, :] = 9.0                                 # every element an outlier (and SCA = 0 with tau on)
    x[m - 1, 77] = -12.0
    x[5, 60] = 10.0                               # an outlier on a pad row (right-padded layout)
    segments = int(seg.max()) + 1
    act = ops.i8_quantize_act(x.to(DEV), seg.to(DEV), segments, tau)
    ca, sca, zeroed, outl = ref.quant_act(x, seg, tau)
    assert torch.equal(act.ca[:, :k].cpu(), ca) and not act.ca[:, k:].any()
    assert torch.equal(act.sca.cpu(), sca)
    cnt = int(act.cnt.item())
    cols = act.cols[:cnt].cpu().tolist()
    union = sorted(set(c for cs in ref.outlier_columns(outl, seg).values() for c in cs))
    assert cols == union
    xo = act.xo[:, :cnt].cpu()
    want = torch.where(outl[:, cols], x[:, cols], torch.zeros((), dtype=torch.float16)) if cnt else xo
    assert torch.equal(xo, want)
    if tau > 0:
        assert cnt > 0
        # one segment quantised on its own gives the same rows as in the batch
        s0 = (seg == 0).nonzero().flatten()
        one = ops.i8_quantize_act(x[s0].contiguous().to(DEV), torch.zeros(len(s0), dtype=torch.int32, device=DEV), 1, tau)
        assert torch.equal(one.ca.cpu(), act.ca.cpu()[s0]) and torch.equal(one.sca.cpu(), act.sca.cpu()[s0])
    else:
        assert cnt == 0


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("m,n,k", [(1, 200, 200), (7, 333, 264), (300, 640, 1000), (300, 200, 8192)])
def test_int32_accumulator_is_exact(m, n, k):
    from astts import ops

    g = torch.Generator().manual_seed(m + n)
    x = (torch.randn(m, k, generator=g) * 2).to(torch.float16)
    w = torch.randn(n, k, generator=g)
    cb, scb = ops.i8_quantize_weight(w.to(DEV))
    act = ops.i8_quantize_act(x.to(DEV), torch.zeros(m, dtype=torch.int32, device=DEV), 1, 6.0)
    acc = ops.i8_gemm(act, cb, scb, n, out_kind=ops.I8_OUT_ACC)
    want = act.ca.double() @ cb[:n].double().T
    assert torch.equal(acc.double(), want)


SHAPES_3B = [(5120, 3072), (3072, 3072), (16384, 3072), (3072, 8192)]


@pytest.mark.parametrize("m", [1, 7, 300, 15360])
@pytest.mark.parametrize("n,k", SHAPES_3B + [(1000, 3072)])
def test_gemm_matches_fp64_restatement(m, n, k):
    """base + outlier + LoRA (r = 32, alpha = 128) at the 3.2-3B projection shapes; segments of 60 rows as in the bench's batch."""
    from astts import ops

    g = torch.Generator().manual_seed(n + k)
    w = torch.randn(n, k, generator=g) * 0.04
    a = torch.randn(32, k, generator=g) * 0.02
    b = torch.randn(n, 32, generator=g) * 0.02
    W = ops.Int8Weight([(w, a, b)], 128 / 32, DEV)
    x = _x(m, k, m, outlier_cols=(11, k - 5), outlier_rows=list(range(0, m, 97)))
    seg = (torch.arange(m, dtype=torch.int32) // 60).to(DEV)
    xd = x.to(DEV)
    y = W(xd, seg, int(seg.max()) + 1, 6.0)
    cb, scb = W.cb[:n], W.scb[:n]
    r = ref.int8_linear(xd, cb, scb, seg, 6.0, (a.to(DEV), b.to(DEV), 4.0))
    e = _rel(y, r)
    assert e <= 1e-6, e
    if m == 300 and n == 1000:                       # the epilogue options and the plain product
        res = torch.randn(m, n, generator=g).to(DEV)
        assert _rel(W(xd, seg, 5, 6.0, residual=res), r + res.double()) <= 1e-6
        y16 = W(xd, seg, 5, 6.0, out_dtype=torch.float16)
        assert y16.dtype == torch.float16 and _rel(y16, r) <= 1e-3
        plain = ops.Int8Weight([(w, None, None)], 1.0, DEV)
        assert _rel(plain(xd, seg, 5, 0.0), ref.int8_linear(xd, cb, scb, seg, 0.0)) <= 1e-6
        assert _rel(plain(xd, seg, 5, 6.0), ref.int8_linear(xd, cb, scb, seg, 6.0)) <= 1e-6


def test_fused_projection_keeps_each_parts_lora():
    from astts import ops

    g = torch.Generator().manual_seed(5)
    parts = [(torch.randn(n, 512, generator=g) * 0.04, torch.randn(16, 512, generator=g) * 0.02, torch.randn(n, 16, generator=g) * 0.02)
             for n in (512, 256, 256)]
    W = ops.Int8Weight(parts, 2.0, DEV)
    x = _x(40, 512, 3, outlier_cols=(9,), outlier_rows=[2]).to(DEV)
    seg = torch.zeros(40, dtype=torch.int32, device=DEV)
    y = W(x, seg, 1, 6.0)
    off = 0
    for w, a, b in parts:
        cb, scb = ref.quant_weight(w)
        r = ref.int8_linear(x, cb.to(DEV), scb.to(DEV), seg, 6.0, (a.to(DEV), b.to(DEV), 2.0))
        assert _rel(y[:, off:off + w.shape[0]], r) <= 1e-6
        off += w.shape[0]


# ------------------------------------------------------------------------------------------------------------ the embedder
def _model(tmp_path, name, raise_layers=(0,)):
    """Synthetic base (some input_layernorm channels raised so that their activations cross tau) + synthetic r = 32 / alpha = 128
    adapter on disk, loaded back through astts.llm.peft."""
    from astts.llm.config import LlamaShape
    from astts.llm.peft import load_peft_model
    from astts.llm.weights import make_llama_weights

    cfg = getattr(LlamaShape, name)()
    sd = make_llama_weights(cfg, 0)
    for i in raise_layers:
        sd[f"model.layers.{i}.input_layernorm.weight"][[5, 17, 100]] = 25.0
    base = ref.write_base(str(tmp_path / f"base_{name}"), cfg, sd)
    ada = ref.write_adapter(str(tmp_path / f"adapter_{name}"), ref.make_lora(cfg, 32, 1), 32, 128, base="org/not-on-this-disk")
    state, cfg2, ad, _ = load_peft_model(ada, base)
    return state, cfg2, ad, base, ada


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_embedder_int8_lora_end_to_end(tmp_path, name):
    import oracle.llama as ol
    from astts.llm.embedder import LlamaEmbedder

    state, cfg, ad, _, _ = _model(tmp_path, name)
    lora = {(i, p[:-5]): ab for (i, p), ab in ad.pairs.items()}
    emb = LlamaEmbedder(state, cfg, DEV, int8=True, lora=ad)
    g = torch.Generator().manual_seed(3)
    lens = [9, 14, 5, 12]
    texts = [torch.randint(3, cfg.vocab, (n,), generator=g) for n in lens]
    lin = ref.make_linear(state, cfg, lora, ad.scaling, int8=True, tau=6.0)
    one = [emb.embed_ids(t[None]).cpu()[0] for t in texts]
    decs = []
    for t, e in zip(texts, one):
        d = ref.Decoder(state, cfg, lin, 6.0, fp16_io=True)
        r = d.step(t).mean(0)
        decs.append(d)
        cos = float(torch.nn.functional.cosine_similarity(e.double(), r.double(), 0))
        print(f"[int8] {name}: cosine to the restatement {cos:.6f}")
        # a last-bit difference upstream moves a rint by one quantisation step: at the real widths (K up to 8192) the observed
        # cosine is 0.99975 without the fp16 storage points mirrored
        assert cos >= (0.9999 if name == "tiny" else 0.9995), cos
    # outliers: in the raised layer, not in the others
    o0 = [c for d in decs for c in d.outliers[(0, "q")][0]]
    o_rest = [c for d in decs for i in range(1, cfg.layers) for c in d.outliers[(i, "q")][0]]
    assert o0 and not o_rest, (o0[:8], o_rest[:8])
    # tau <= 0 disables the decomposition: a different result
    emb0 = LlamaEmbedder(state, cfg, DEV, int8=True, lora=ad, int8_threshold=0.0)
    e0 = emb0.embed_ids(texts[0][None]).cpu()[0]
    assert float((e0 - one[0]).abs().max()) > 1e-4
    # the quantisation error: int8 + LoRA vs the fp32 merged model (reported; loose bound)
    merged = ref.merged(state, lora, ad.scaling)
    for t, e in zip(texts, one):
        eo = ol.get_embedding(merged, cfg, t[None])[0]
        cos = float(torch.nn.functional.cosine_similarity(e.double(), eo.double(), 0))
        print(f"[int8] {name}: int8+LoRA vs fp32 merged cosine {cos:.6f}")
        assert cos >= 0.99
    # batched == one text at a time (right padding belongs to no segment)
    ids = torch.zeros(len(texts), max(lens), dtype=torch.int64)
    for i, t in enumerate(texts):
        ids[i, :len(t)] = t
    bat = emb.embed_ids(ids, torch.tensor(lens)).cpu()
    e_b = _rel(bat, torch.stack(one))
    print(f"[int8] {name}: batched vs one-at-a-time rel {e_b:.2e}")
    assert e_b <= 1e-5
    # greedy tokens: equal to the restatement while its top-2 margin is decisive; batch == one at a time
    prompts = [t.tolist() for t in texts[:3]]
    gb = emb.generate_greedy_batch(prompts, 6)
    for p, got in zip(prompts, gb):
        assert got == emb.generate_greedy(p, 6)
        toks, margins = ref.generate(state, cfg, lin, p, 6, 6.0, fp16_io=True)
        new = got[len(p):]
        for s, (a, b, mg) in enumerate(zip(new, toks, margins)):
            if mg < 0.25:                            # a near tie: either token is right
                break
            assert a == b, (s, new, toks, margins)


def test_adapter_precision_fp16_merges_lora(tmp_path):
    """--llm_precision fp16 on an adapter: the LoRA merged into the fp16 weights; close to the fp32 merged oracle."""
    import oracle.llama as ol
    from astts.llm.embedder import LlamaEmbedder

    state, cfg, ad, _, _ = _model(tmp_path, "tiny", raise_layers=())
    lora = {(i, p[:-5]): ab for (i, p), ab in ad.pairs.items()}
    emb = LlamaEmbedder(state, cfg, DEV, lora=ad)
    ids = torch.randint(3, cfg.vocab, (1, 11), generator=torch.Generator().manual_seed(0))
    e = emb.embed_ids(ids).cpu()[0]
    eo = ol.get_embedding(ref.merged(state, lora, ad.scaling), cfg, ids)[0]
    assert _rel(e, eo) < 1e-2


def _search_inputs(tmp_path):
    rows = [{"zh_text": t, "speaker": s} for t, s in [("I can't believe you did that!", "ELIZABETH"), ("Fine, whatever.", "JOHN"),
                                                      ("We won the game!", "ANN")]]
    p = tmp_path / "in.jsonl"
    p.write_text("".join(json.dumps(r) + "\n" for r in rows))
    return str(p)


def test_search_clis_on_an_adapter_directory(tmp_path, capsys):
    from astts.cli import search_json, search_milvus
    from astts.llm.embedder import LlamaEmbedder

    state, cfg, ad, base, ada = _model(tmp_path, "wide")
    db = os.path.join(GOLD, "milvus_demo.db")
    inp = _search_inputs(tmp_path)
    argv = ["--input_json", inp, "--db_path", db, "--model_path", ada, "--base_model_path", base]
    res = search_json.main(search_json.build_parser().parse_args(argv + ["--output_file", str(tmp_path / "out.jsonl")]))
    out = capsys.readouterr().out
    assert "Error during" not in out and "Error getting" not in out, out
    api = search_json.main(search_json.build_parser().parse_args(argv), embedder=LlamaEmbedder(state, cfg, DEV, int8=True, lora=ad))
    assert [r["retrieved_file_id"] for r in res] == [r["retrieved_file_id"] for r in api]
    assert all(r["retrieved_file_id"] not in ("Error", "N/A") for r in res)
    margs = search_milvus.build_parser().parse_args(["--db_path", db, "--model_path", ada, "--base_model_path", base, "--top_k", "3"])
    hits = search_milvus.main(margs)
    emb = search_milvus.load_embedder(ada, base_model_path=base)
    assert emb.int8 and emb.cfg.hidden == 3072
    hits_api = search_milvus.main(margs, embedder=LlamaEmbedder(state, cfg, DEV, int8=True, lora=ad))
    assert hits and [h["entity"]["file_id"] for h in hits[0]] == [h["entity"]["file_id"] for h in hits_api[0]]


def test_full_depth_3b_int8_pass():
    """One int8 pass of the 28-layer 3.2-3B shape (seeded weights drawn on the GPU): finishes, close to the fp16 path.  Seeded Gaussian
    weights amplify a perturbation over 28 layers far more than a trained network (fp16 vs fp32 alone: 8.9e-3);
    int8's per-projection error is ~20x fp16's, observed cosine 0.95 to the fp16 path here."""
    from astts.llm.config import LlamaShape
    from astts.llm.embedder import LlamaEmbedder
    from astts.llm.weights import make_llama_weights

    cfg = LlamaShape.llama32_3b()
    sd = make_llama_weights(cfg, 0, device=DEV)
    e8 = LlamaEmbedder(sd, cfg, DEV, int8=True)
    ids = torch.randint(3, 5000, (2, 40), generator=torch.Generator().manual_seed(0))
    a = e8.embed_ids(ids).cpu()
    del e8
    torch.cuda.empty_cache()
    f16 = LlamaEmbedder(sd, cfg, DEV)
    b = f16.embed_ids(ids).cpu()
    cos = torch.nn.functional.cosine_similarity(a.double(), b.double(), 1)
    print(f"[int8] 3.2-3B full depth: int8 vs fp16 cosine {cos.tolist()}")
    assert bool(torch.isfinite(a).all()) and bool((cos >= 0.9).all()), cos
