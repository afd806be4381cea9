"""The relative-position transformer encoder shared by the three networks (text encoder, LM body, flow token encoder), and the
load-time helpers they all use."""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

from .. import ops
from ..ops import PackedWeight

SD = Dict[str, torch.Tensor]


def _dev(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def rel_pos_table(d: int, max_pos: int) -> torch.Tensor:
    """Constant sinusoid table (host-side constant generation): rows rel = -max_pos..max_pos."""
    rel = torch.arange(-max_pos, max_pos + 1, dtype=torch.float32)[:, None]
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(2 * max_pos + 1, d)
    pe[:, 0::2] = torch.sin(rel * div)
    pe[:, 1::2] = torch.cos(rel * div)
    return pe


def fold_layernorm(w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Linear(LayerNorm(x; gamma, beta)) == Linear'((x - mean) * rstd) with W' = W diag(gamma), b' = b + W beta
    (exact algebra, evaluated in fp64 at load): the decode step then normalises without reading gamma / beta --
    eight waves of every workgroup re-read both vectors otherwise, as many bytes as the workgroup's weights."""
    w64, g64, be64 = w.double(), gamma.double(), beta.double()
    return (w64 * g64[None, :]).float(), (b.double() + w64 @ be64).float()


class RelPosEncoder:
    """espnet-style pre-norm encoder with relative-position attention (text encoder, token encoder,
    and the causal LM body).  Holds one precomputed table ``linear_pos(pe(rel))`` per layer.

    ``fold_ln`` (the LM body): the scale / shift of norm1 / norm2 are folded into the q|k|v and FFN-in projections at
    load (``fold_layernorm``); ``n1`` / ``n2`` / ``after`` then hold ones / zeros (``after_norm`` is folded into the
    output head by the owner).  Prefill and decode use the same folded weights."""

    def __init__(self, sd: SD, prefix: str, heads: int, layers: int, act: str, norm_names: Tuple[str, str],
                 legacy_embed: bool, causal: bool, eps: float, max_pos: int, device, pos_dtype=torch.float32, fold_ln: bool = False):
        self.heads, self.layers, self.act, self.causal, self.eps = heads, layers, act, causal, eps
        self.legacy_embed = legacy_embed
        self.center = max_pos
        self.fold_ln = fold_ln
        p = prefix
        self.d = int(sd[p + ".after_norm.weight"].shape[0])
        self.embed = PackedWeight(sd[p + ".embed.out.0.weight"], sd[p + ".embed.out.0.bias"], device)
        self.embed_ln = (_dev(sd[p + ".embed.out.1.weight"], device), _dev(sd[p + ".embed.out.1.bias"], device))
        ident = (torch.ones(self.d, dtype=torch.float32, device=device), torch.zeros(self.d, dtype=torch.float32, device=device))
        self.after = ident if fold_ln else (_dev(sd[p + ".after_norm.weight"], device), _dev(sd[p + ".after_norm.bias"], device))
        pe = rel_pos_table(self.d, max_pos).to(device)
        n1, n2 = norm_names
        self.L: List[dict] = []
        for i in range(layers):
            q = f"{p}.encoders.{i}"
            a = q + ".self_attn"
            g1, b1 = sd[f"{q}.{n1}.weight"].float().cpu(), sd[f"{q}.{n1}.bias"].float().cpu()
            g2, b2 = sd[f"{q}.{n2}.weight"].float().cpu(), sd[f"{q}.{n2}.bias"].float().cpu()
            wq, bq = sd[a + ".linear_q.weight"].float().cpu(), sd[a + ".linear_q.bias"].float().cpu()
            wkv = torch.cat([sd[a + ".linear_k.weight"], sd[a + ".linear_v.weight"]], 0).float().cpu()
            bkv = torch.cat([sd[a + ".linear_k.bias"], sd[a + ".linear_v.bias"]], 0).float().cpu()
            w1, bw1 = sd[q + ".feed_forward.w_1.weight"].float().cpu(), sd[q + ".feed_forward.w_1.bias"].float().cpu()
            if fold_ln:
                wq, bq = fold_layernorm(wq, bq, g1, b1)
                wkv, bkv = fold_layernorm(wkv, bkv, g1, b1)
                w1, bw1 = fold_layernorm(w1, bw1, g2, b2)
            lay = {
                "n1": ident if fold_ln else (_dev(g1, device), _dev(b1, device)),
                "n2": ident if fold_ln else (_dev(g2, device), _dev(b2, device)),
                "wq": PackedWeight(wq, bq, device),
                "wkv": PackedWeight(wkv, bkv, device),
                "wqkv": PackedWeight(torch.cat([wq, wkv], 0), torch.cat([bq, bkv], 0), device),
                "wo": PackedWeight(sd[a + ".linear_out.weight"], sd[a + ".linear_out.bias"], device),
                "w1": PackedWeight(w1, bw1, device),
                "w2": PackedWeight(sd[q + ".feed_forward.w_2.weight"], sd[q + ".feed_forward.w_2.bias"], device),
                "u": _dev(sd[a + ".pos_bias_u"].reshape(-1), device),
                "v": _dev(sd[a + ".pos_bias_v"].reshape(-1), device),
            }
            lay["pos"] = ops.linear(pe, PackedWeight(sd[a + ".linear_pos.weight"], None, device), out_dtype=pos_dtype)
            self.L.append(lay)

    def embed_in(self, x: torch.Tensor) -> torch.Tensor:
        h = ops.linear(x, self.embed)
        if self.legacy_embed:
            # LayerNorm -> ReLU -> * sqrt(d) in one launch (relu commutes with the positive scale)
            return ops.layernorm(h, *self.embed_ln, self.eps, relu_scale=math.sqrt(self.d))
        h = ops.layernorm(h, *self.embed_ln, self.eps)
        return ops.elementwise(ops.EL_SCALE, h, s=math.sqrt(self.d))

    def forward(self, x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """Batch-major full-sequence pass: x [B, T, in_dim], lens int32 [B] -> [B, T, d]."""
        h = self.embed_in(x)
        d = self.d
        for lay in self.L:
            n = ops.layernorm(h, *lay["n1"], self.eps)
            q = ops.linear(n, lay["wq"])
            kv = ops.linear(n, lay["wkv"])
            a = ops.attn_relpos(q, kv[..., :d], kv[..., d:], lay["pos"], lay["u"], lay["v"], self.heads, lens=lens,
                                q_pos0=0, pos_center=self.center, causal=self.causal)
            h = ops.linear(a, lay["wo"], residual=h)
            n = ops.layernorm(h, *lay["n2"], self.eps)
            f = ops.linear(n, lay["w1"], act=self.act)
            h = ops.linear(f, lay["w2"], residual=h)
        return ops.layernorm(h, *self.after, self.eps)
