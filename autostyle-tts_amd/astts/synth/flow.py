"""The flow-matching decoder (token encoder, length regulator, U-Net estimator) and its C++ Euler solver (libastts ``astts_flow_*``)."""
from __future__ import annotations

import ctypes
import math
from typing import List, NamedTuple, Optional

import torch

from .. import _lib, ops
from ..ops import PackedWeight
from .config import SynthConfig
from .encoder import SD, RelPosEncoder, _dev, fold_layernorm


class _Resnet1D:
    def __init__(self, sd: SD, p: str, device, groups: int):
        self.groups = groups
        self.c1 = PackedWeight.from_conv1d(sd[p + ".block1.block.0.weight"], sd[p + ".block1.block.0.bias"], device)
        self.g1 = (_dev(sd[p + ".block1.block.1.weight"], device), _dev(sd[p + ".block1.block.1.bias"], device))
        self.mlp = PackedWeight(sd[p + ".mlp.1.weight"], sd[p + ".mlp.1.bias"], device)
        self.c2 = PackedWeight.from_conv1d(sd[p + ".block2.block.0.weight"], sd[p + ".block2.block.0.bias"], device)
        self.g2 = (_dev(sd[p + ".block2.block.1.weight"], device), _dev(sd[p + ".block2.block.1.bias"], device))
        self.res = PackedWeight.from_conv1d(sd[p + ".res_conv.weight"], sd[p + ".res_conv.bias"], device)
        # 256 -> 256 blocks (all mid blocks): three launches with the GroupNorm + Mish passes folded into the convolutions
        # (ops.resnet_conv) instead of five
        self.fused = all(w.cin == w.cin_pad for w in (self.c1, self.c2, self.res)) and \
            ops.resnet_conv_supported(self.c1.cin, self.c1.n, groups, self.c1.taps) and \
            ops.resnet_conv_supported(self.c2.cin, self.c2.n, groups, self.c2.taps) and \
            ops.resnet_conv_supported(self.res.cin, self.res.n, groups, self.res.taps)
        self.c1_frag, self.c2_frag, self.res_frag = ((ops.conv_pack_frag(self.c1), ops.conv_pack_frag(self.c2), ops.conv_pack_frag(self.res))
                                                     if self.fused else (None, None, None))

    def forward(self, x: torch.Tensor, lens: torch.Tensor, temb_mish: torch.Tensor, tproj: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x must already be zero beyond lens (masked).  ``tproj`` [B, C]: this block's time projection when the caller has
        it already (the solver evaluates the time path of all Euler steps up front)."""
        if tproj is None:
            tproj = ops.linear(temb_mish, self.mlp)                              # [B, C]
        if self.fused:
            x = x.contiguous()
            h1, s1 = ops.resnet_conv(x, self.c1, self.c1_frag, lens=lens, want_stats=True)
            h2, s2 = ops.resnet_conv(h1, self.c2, self.c2_frag, lens=lens, in_gn=(s1, *self.g1), in_add=tproj.contiguous(), want_stats=True)
            return ops.resnet_conv(x, self.res, self.res_frag, lens=lens, res_gn=(h2, s2, *self.g2))
        h = ops.conv1d(x, self.c1, pad=1)
        h = ops.groupnorm(h, *self.g1, self.groups, 1e-5, lens=lens, mish=True, add_bc=tproj, out_dtype=torch.float16)
        h = ops.conv1d(h, self.c2, pad=1)                                       # fp16 in: only consumer is the MFMA
        h = ops.groupnorm(h, *self.g2, self.groups, 1e-5, lens=lens, mish=True)
        return ops.conv1d(x, self.res, residual=h)                              # res_conv(x) + h


class _TfmBlock:
    def __init__(self, sd: SD, p: str, heads: int, device):
        self.heads = heads
        # norm1's scale / shift are folded into the fused q|k|v projection (W' = W diag(gamma), b' = W beta: fold_layernorm), so
        # that the fused LayerNorm + projection + attention kernel (ops.tfm_attn_fused) normalises without them; the unfused
        # path (T > 384) runs the plain LayerNorm kernel with the identity affine on the same weights.
        wqkv = torch.cat([sd[p + ".attn1.to_q.weight"], sd[p + ".attn1.to_k.weight"], sd[p + ".attn1.to_v.weight"]], 0).float().cpu()
        wqkv, bqkv = fold_layernorm(wqkv, torch.zeros(wqkv.shape[0]), sd[p + ".norm1.weight"].float().cpu(), sd[p + ".norm1.bias"].float().cpu())
        c = int(wqkv.shape[1])
        self.n1 = (torch.ones(c, dtype=torch.float32, device=device), torch.zeros(c, dtype=torch.float32, device=device))
        self.wqkv = PackedWeight(wqkv, bqkv, device)
        self.wqkv_frag = ops.tfm_pack_frag(self.wqkv) if c == 256 and wqkv.shape[0] % 32 == 0 else None   # fused kernel's weight image
        self.wo = PackedWeight(sd[p + ".attn1.to_out.0.weight"], sd[p + ".attn1.to_out.0.bias"], device)
        # norm3 folded into the first feed-forward projection in the same way (ops.tfm_ffn_fused: LayerNorm + W1 + GELU + W2 +
        # residual in one launch)
        w1, b1 = fold_layernorm(sd[p + ".ff.net.0.proj.weight"].float().cpu(), sd[p + ".ff.net.0.proj.bias"].float().cpu(),
                                sd[p + ".norm3.weight"].float().cpu(), sd[p + ".norm3.bias"].float().cpu())
        self.n3 = self.n1
        self.w1 = PackedWeight(w1, b1, device)
        self.w2 = PackedWeight(sd[p + ".ff.net.2.weight"], sd[p + ".ff.net.2.bias"], device)
        self.ffn_fused = ops.tfm_ffn_fused_supported(c, int(w1.shape[0]))
        self.w1_frag = ops.tfm_pack_frag(self.w1) if self.ffn_fused else None
        self.w2_frag = ops.tfm_pack_frag(self.w2) if self.ffn_fused else None
        # ... and the attention's output projection + residual as that launch's prologue
        self.wo_frag = ops.tfm_pack_frag(self.wo) if self.ffn_fused and self.wo.cin in (256, 512) else None

    def forward(self, x: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        hd = self.heads * 64
        f16 = torch.float16   # everything between two residual adds feeds MFMA operands only: fp16 in HBM
        if self.wqkv_frag is not None and ops.tfm_attn_fused_supported(x.shape[-1], self.heads, x.shape[1]):
            a = ops.tfm_attn_fused(x, self.wqkv, self.wqkv_frag, self.heads, lens=lens, eps=1e-5)     # LayerNorm + q|k|v + attention: one launch
        else:
            n = ops.layernorm(x, *self.n1, 1e-5, out_dtype=f16)
            qkv = ops.linear(n, self.wqkv, out_dtype=f16)
            a = ops.attn_mha(qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:], self.heads, lens=lens, out_dtype=f16)
        if self.wo_frag is not None:
            return ops.tfm_ffn_fused(x, self.w1, self.w1_frag, self.w2, self.w2_frag, eps=1e-5, attn=a.contiguous(), wo=self.wo, wo_frag=self.wo_frag)
        x = ops.linear(a, self.wo, residual=x)
        if self.ffn_fused:
            return ops.tfm_ffn_fused(x, self.w1, self.w1_frag, self.w2, self.w2_frag, eps=1e-5)
        n = ops.layernorm(x, *self.n3, 1e-5, out_dtype=f16)
        f = ops.linear(n, self.w1, act="gelu", out_dtype=f16)
        return ops.linear(f, self.w2, residual=x)


class _Block(NamedTuple):
    """One U-Net block of the estimator: ResnetBlock1D, its transformer blocks, and (down / up blocks) the convolution that resamples
    behind them -- a plain convolution in the ``last`` block of its group.  Mid blocks have none."""
    res: _Resnet1D
    tfms: List[_TfmBlock]
    resample: Optional[PackedWeight] = None
    last: bool = False


class FlowDecoder:
    """MaskedDiffWithXvec + ConditionalCFM: tokens -> mu -> 10 Euler steps of the U-Net estimator with
    classifier-free guidance (cond and uncond halves run as one 2B batch)."""

    def __init__(self, sd: SD, cfg: SynthConfig, device):
        self.cfg, self.device = cfg, device
        self.use_engine = True          # False: operator-by-operator solve from Python (tests compare the two)
        self.tok_emb = _dev(sd["input_embedding.weight"], device)
        self.spk_aff = PackedWeight(sd["spk_embed_affine_layer.weight"], sd["spk_embed_affine_layer.bias"], device)
        self.enc = RelPosEncoder(sd, "encoder", cfg.flow_heads, cfg.flow_layers, "swish", ("norm_mha", "norm_ff"), False,
                                 False, cfg.ln_eps, cfg.max_positions, device)
        self.enc_proj = PackedWeight(sd["encoder_proj.weight"], sd["encoder_proj.bias"], device)
        self.lr = []
        for j in range(4):
            self.lr.append((PackedWeight.from_conv1d(sd[f"length_regulator.model.{3 * j}.weight"],
                                                     sd[f"length_regulator.model.{3 * j}.bias"], device),
                            _dev(sd[f"length_regulator.model.{3 * j + 1}.weight"], device),
                            _dev(sd[f"length_regulator.model.{3 * j + 1}.bias"], device)))
        self.lr_out = PackedWeight.from_conv1d(sd["length_regulator.model.12.weight"], sd["length_regulator.model.12.bias"], device)
        e = "decoder.estimator"
        self.t1 = PackedWeight(sd[e + ".time_mlp.linear_1.weight"], sd[e + ".time_mlp.linear_1.bias"], device)
        self.t2 = PackedWeight(sd[e + ".time_mlp.linear_2.weight"], sd[e + ".time_mlp.linear_2.bias"], device)
        ch = cfg.est_channels
        g = cfg.est_groups
        self.down, self.mid, self.up = [], [], []
        for i in range(len(ch)):
            p = f"{e}.down_blocks.{i}"
            last = i == len(ch) - 1
            wname = p + ".2" + ("" if last else ".conv")
            self.down.append(_Block(_Resnet1D(sd, p + ".0", device, g),
                                    [_TfmBlock(sd, f"{p}.1.{j}", cfg.est_heads, device) for j in range(cfg.est_tfm_per_block)],
                                    PackedWeight.from_conv1d(sd[wname + ".weight"], sd[wname + ".bias"], device), last))
        for i in range(cfg.est_mid_blocks):
            p = f"{e}.mid_blocks.{i}"
            self.mid.append(_Block(_Resnet1D(sd, p + ".0", device, g),
                                   [_TfmBlock(sd, f"{p}.1.{j}", cfg.est_heads, device) for j in range(cfg.est_tfm_per_block)]))
        for i in range(len(ch)):
            p = f"{e}.up_blocks.{i}"
            last = i == len(ch) - 1
            if last:
                w = PackedWeight.from_conv1d(sd[p + ".2.weight"], sd[p + ".2.bias"], device)
            else:
                w = PackedWeight.from_conv_transpose1d(sd[p + ".2.conv.weight"], sd[p + ".2.conv.bias"], 2, device)
            self.up.append(_Block(_Resnet1D(sd, p + ".0", device, g),
                                  [_TfmBlock(sd, f"{p}.1.{j}", cfg.est_heads, device) for j in range(cfg.est_tfm_per_block)], w, last))
        self.fin_c = PackedWeight.from_conv1d(sd[e + ".final_block.block.0.weight"], sd[e + ".final_block.block.0.bias"], device)
        self.fin_g = (_dev(sd[e + ".final_block.block.1.weight"], device), _dev(sd[e + ".final_block.block.1.bias"], device))
        self.fin_p = PackedWeight.from_conv1d(sd[e + ".final_proj.weight"], sd[e + ".final_proj.bias"], device)

    # ---- token encoder + length regulator
    def mu(self, tokens: torch.Tensor, token_lens: torch.Tensor, mel_total: int, mel_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mel_lens (ragged batch): row b is regulated from token_lens[b] tokens to mel_lens[b] frames, zeros beyond."""
        x = ops.embedding(self.tok_emb, tokens.clamp(min=0))
        x = ops.elementwise(ops.EL_MUL_ROWMASK, x, lens=token_lens)
        h = ops.linear(self.enc.forward(x, token_lens), self.enc_proj)
        h = ops.interp_linear(h, mel_total, in_lens=None if mel_lens is None else token_lens, out_lens=mel_lens)
        for w, ga, be in self.lr:
            h = ops.conv1d(h, w, pad=1)
            h = ops.groupnorm(h, ga, be, 1, 1e-5, lens=mel_lens, mish=True)      # writes 0 beyond the row's length
        h = ops.conv1d(h, self.lr_out)
        return h if mel_lens is None else ops.elementwise(ops.EL_MUL_ROWMASK, h, lens=mel_lens)

    # ---- one estimator evaluation on a (2B) batch
    def time_path(self, t: torch.Tensor) -> List[torch.Tensor]:
        """t fp32 [rows] -> the time projection of every ResnetBlock1D (down, mid, up order), each [rows, C]: sinusoidal
        embedding -> MLP -> Mish (every block applies Mish before its own Linear).  Independent of x: the solver calls it once
        with the rows of ALL Euler steps."""
        temb = ops.time_embedding(t, self.cfg.est_in)
        temb = ops.linear(ops.linear(temb, self.t1, act="silu"), self.t2)
        temb_m = ops.elementwise(ops.EL_MISH, temb)
        return [ops.linear(temb_m, blk.res.mlp) for grp in (self.down, self.mid, self.up) for blk in grp]

    def estimator(self, x, mu, spk, cond, t, lens, full: bool = False, tprojs: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """``full``: every row uses all T frames (fixed-length batch) -- the length masks are identities and are
        not launched.  ``tprojs``: the blocks' time projections for this call's rows (``time_path``), computed here if absent."""
        cfg = self.cfg
        b, T, _ = x.shape
        if full:
            _mask = lambda h, L: h
        else:
            _mask = lambda h, L: ops.elementwise(ops.EL_MUL_ROWMASK, h, lens=L)
        if tprojs is None:
            tprojs = self.time_path(t)
        tp = iter(tprojs)
        temb_m = None
        h = torch.cat([x, mu, spk[:, None, :].expand(b, T, -1), cond], dim=-1)
        hiddens, lens_stack = [], [lens]
        for res, tfms, wds, last in self.down:
            L = lens_stack[-1]
            h = _mask(h, L)
            h = res.forward(h, L, temb_m, next(tp))
            for tb in tfms:
                h = tb.forward(h, L)
            hiddens.append(h)
            hm = _mask(h, L)
            if last:
                h = ops.conv1d(hm, wds, pad=1)
                lens_stack.append(L)
            else:
                h = ops.conv1d(hm, wds, stride=2, pad=1)
                lens_stack.append(torch.div(L + 1, 2, rounding_mode="floor").to(torch.int32))
        L = lens_stack[-1]
        h = _mask(h, L)
        for blk in self.mid:
            h = blk.res.forward(h, L, temb_m, next(tp))
            for tb in blk.tfms:
                h = tb.forward(h, L)
            h = _mask(h, L)
        lens_stack.pop()
        for res, tfms, wus, last in self.up:
            L = lens_stack.pop()
            skip = hiddens.pop()
            h = torch.cat([h[:, :skip.shape[1]], skip], dim=-1)
            h = _mask(h, L)
            h = res.forward(h, L, temb_m, next(tp))
            for tb in tfms:
                h = tb.forward(h, L)
            hm = _mask(h, L)
            if last:
                h = ops.conv1d(hm, wus, pad=1)
            else:
                h = ops.conv_transpose1d(hm, wus, padding=1)
        h = _mask(h[:, :T].contiguous(), lens)
        h = ops.conv1d(h, self.fin_c, pad=1)
        h = ops.groupnorm(h, *self.fin_g, cfg.est_groups, 1e-5, lens=lens, mish=True)
        out = ops.conv1d(h, self.fin_p)
        return _mask(out, lens)

    # ---- C++ solver engine (libastts astts_flow_*): the same operator sequence, issued without Python in the loop
    def _engine(self):
        if getattr(self, "_eng", None) is None:
            cfg = self.cfg
            keep = []           # ctypes arrays referenced by pointer from the block structs

            def W(pw):
                return ops.Weight(pw.data.data_ptr(), None if pw.bias is None else pw.bias.data_ptr(), pw.n, pw.cin, pw.cin_pad, pw.taps)

            def R(r):
                fp = [None if f is None else f.data_ptr() for f in (r.c1_frag, r.c2_frag, r.res_frag)]
                return ops.FlowResnet(W(r.c1), W(r.mlp), W(r.c2), W(r.res), r.g1[0].data_ptr(), r.g1[1].data_ptr(),
                                      r.g2[0].data_ptr(), r.g2[1].data_ptr(), *fp)

            def TF(tfms):
                arr = (ops.FlowTfm * len(tfms))()
                for i, t in enumerate(tfms):
                    arr[i] = ops.FlowTfm(t.n1[0].data_ptr(), t.n1[1].data_ptr(), t.n3[0].data_ptr(), t.n3[1].data_ptr(),
                                         W(t.wqkv), W(t.wo), W(t.w1), W(t.w2), None if t.wqkv_frag is None else t.wqkv_frag.data_ptr(),
                                         None if t.w1_frag is None else t.w1_frag.data_ptr(), None if t.w2_frag is None else t.w2_frag.data_ptr(),
                                         None if t.wo_frag is None else t.wo_frag.data_ptr())
                keep.append(arr)
                return arr

            def blocks(items, kinds):
                arr = (ops.FlowBlock * max(len(items), 1))()
                for i, (blk, kind) in enumerate(zip(items, kinds)):
                    rs = W(blk.resample) if kind != ops.FLOW_RESAMPLE_NONE else ops.Weight()
                    arr[i] = ops.FlowBlock(R(blk.res), TF(blk.tfms), len(blk.tfms), rs, kind)
                keep.append(arr)
                return arr

            down = blocks(self.down, [ops.FLOW_RESAMPLE_CONV if blk.last else ops.FLOW_RESAMPLE_DOWN for blk in self.down])
            mid = blocks(self.mid, [ops.FLOW_RESAMPLE_NONE] * len(self.mid))
            up = blocks(self.up, [ops.FLOW_RESAMPLE_CONV if blk.last else ops.FLOW_RESAMPLE_UP for blk in self.up])
            c = ops.FlowConfig(cfg.mel, cfg.est_channels[0], cfg.est_heads, cfg.est_groups, cfg.est_in, cfg.est_time_dim,
                               len(self.down), len(self.mid), len(self.up), W(self.t1), W(self.t2), W(self.fin_c), W(self.fin_p),
                               self.fin_g[0].data_ptr(), self.fin_g[1].data_ptr())
            h = ctypes.c_void_p()
            _lib.check(_lib.load().astts_flow_create(ctypes.byref(c), down, mid, up, ctypes.byref(h)))
            self._eng, self._eng_keep = h, keep
        return self._eng

    def _schedule(self):
        n = self.cfg.cfm_steps
        ts = 1.0 - torch.cos(torch.linspace(0, 1, n + 1) * 0.5 * math.pi)       # cosine schedule (fp32, as upstream)
        return [float(ts[s]) for s in range(n)], [float(ts[s + 1] - ts[s]) for s in range(n)]

    def _batch_args(self, x, mu, spk_e, cond, lens, tv, dv):
        """The arguments ``astts_flow_solve`` and ``astts_flow_session_admit`` share: the batch's tensors (checked: contiguous fp32),
        its shape, the schedule ``tv`` / ``dv`` as C arrays, the guidance rate."""
        b, t, _ = x.shape
        assert x.is_contiguous() and mu.is_contiguous() and cond.is_contiguous() and spk_e.is_contiguous()
        assert x.dtype == mu.dtype == cond.dtype == spk_e.dtype == torch.float32
        n = len(tv)
        return (x.data_ptr(), mu.data_ptr(), spk_e.data_ptr(), cond.data_ptr(), None if lens is None else lens.data_ptr(), b, t, n,
                (ctypes.c_float * n)(*tv), (ctypes.c_float * n)(*dv), self.cfg.cfg_rate)

    def solve(self, x: torch.Tensor, mu: torch.Tensor, spk_e: torch.Tensor, cond: torch.Tensor,
              lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Euler solve with classifier-free guidance, in place on ``x`` [B, T, mel] (in: noise, out: mel).
        ``lens`` None = fixed-length batch.  Runs in the C++ engine; ``solve_ops`` is the operator-by-operator form."""
        lib = _lib.load()
        eng = self._engine()
        args = self._batch_args(x, mu, spk_e, cond, lens, *self._schedule())
        need = int(lib.astts_flow_workspace_bytes(eng, x.shape[0], x.shape[1]))
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        _lib.check(lib.astts_flow_solve(eng, *args, ws.data_ptr(), need, _lib.stream_ptr()))
        return x

    def solve_ops(self, x, mu, spk_e, cond, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Same solve, one Python call per operator (the form the C++ engine is checked against, bit for bit)."""
        b, t, _ = x.shape
        full = lens is None
        if full:
            lens = torch.full((b,), t, dtype=torch.int32, device=x.device)
        lens2 = torch.cat([lens, lens])
        mu2 = torch.cat([mu, torch.zeros_like(mu)], 0)
        spk2 = torch.cat([spk_e, torch.zeros_like(spk_e)], 0)
        cond2 = torch.cat([cond, torch.zeros_like(cond)], 0)
        tv, dv = self._schedule()
        b2 = 2 * b
        t_all = torch.tensor(tv, dtype=torch.float32, device=x.device).repeat_interleave(b2)      # rows of all steps, as the engine
        tp_all = self.time_path(t_all)
        for s in range(len(tv)):
            t2 = t_all[s * b2:(s + 1) * b2]
            d = self.estimator(torch.cat([x, x], 0), mu2, spk2, cond2, t2, lens2, full=full,
                               tprojs=[tp[s * b2:(s + 1) * b2] for tp in tp_all])
            x = ops.elementwise(ops.EL_CFG_EULER, x, z=d, s=dv[s], s2=self.cfg.cfg_rate)
        return x

    def decode(self, tokens, token_lens, prompt_mel, spk, z, mel_total: int) -> torch.Tensor:
        """tokens [B, Tp+Ts], prompt_mel [B, Tm_p, mel], spk [B, spk_dim], z [B, mel_total, mel]
        -> mel [B, mel_total - Tm_p, mel] (fixed-length batch)."""
        x, mu, spk_e, cond, tmp = self.prepare(tokens, token_lens, prompt_mel, spk, z, mel_total)
        x = (self.solve if self.use_engine else self.solve_ops)(x, mu, spk_e, cond)
        return x[:, tmp:].contiguous()

    def session(self, t: int, slots: int = 4, rows_max: int = 32, stream=None) -> "FlowSession":
        """A chain of estimator passes that up to ``slots`` batches of ``t`` frames (``rows_max`` rows together) share: see FlowSession."""
        return FlowSession(self, t, slots, rows_max, stream)

    def prepare(self, tokens, token_lens, prompt_mel, spk, z, mel_total: int):
        """What ``decode`` computes before its solve (token encoder, speaker affine, prompt condition, the start noise's copy)
        -> (x, mu, spk_e, cond, prompt frames): the arguments of ``solve`` / ``FlowSession.admit``; the mel is ``x[:, prompt frames:]``."""
        b = tokens.shape[0]
        mu = self.mu(tokens, token_lens, mel_total)
        spk_e = ops.linear(torch.nn.functional.normalize(spk, dim=1), self.spk_aff)
        tmp = prompt_mel.shape[1]
        cond = torch.zeros((b, mel_total, self.cfg.mel), dtype=torch.float32, device=self.device)
        cond[:, :tmp] = prompt_mel
        return z.clone(), mu, spk_e, cond, tmp

    def decode_ragged(self, tokens: List[torch.Tensor], prompt_mels: List[torch.Tensor], spk: torch.Tensor,
                      zs: List[torch.Tensor]) -> List[torch.Tensor]:
        """Ragged batch: row i = (prompt + generated tokens [Ti], prompt mel [Tm_p_i, mel], noise z [mel_total_i, mel]).
        Padded to the longest row, every stage masked by the row lengths -> list of mels [mel_total_i - Tm_p_i, mel],
        each equal to running that utterance alone."""
        cfg, dev = self.cfg, self.device
        b = len(tokens)
        tl = [int(t.numel()) for t in tokens]
        tmp = [int(m.shape[0]) for m in prompt_mels]
        mt = [int(z.shape[0]) for z in zs]
        tmax, mmax = max(tl), max(mt)
        tok = torch.zeros((b, tmax), dtype=torch.int32, device=dev)
        cond = torch.zeros((b, mmax, cfg.mel), dtype=torch.float32, device=dev)
        x = torch.zeros((b, mmax, cfg.mel), dtype=torch.float32, device=dev)
        for i in range(b):
            tok[i, :tl[i]] = tokens[i].to(dev).view(-1)
            cond[i, :tmp[i]] = prompt_mels[i].to(dev)
            x[i, :mt[i]] = zs[i].to(dev)
        tok_lens = torch.tensor(tl, dtype=torch.int32, device=dev)
        mel_lens = torch.tensor(mt, dtype=torch.int32, device=dev)
        mu = self.mu(tok, tok_lens, mmax, mel_lens)
        spk_e = ops.linear(torch.nn.functional.normalize(spk.to(dev), dim=1), self.spk_aff)
        x = (self.solve if self.use_engine else self.solve_ops)(x, mu, spk_e, cond, mel_lens)
        return [x[i, tmp[i]:mt[i]].contiguous() for i in range(b)]


class FlowJob:
    """One batch in a FlowSession: ``x`` [B, T, mel] is the mel (in place) once ``FlowSession.step`` has returned the job.  The job
    keeps the tensors the session's kernels read until the batch's last step."""

    def __init__(self, x, mu, spk_e, cond, lens, n_steps: int):
        self.x, self.mu, self.spk_e, self.cond, self.lens = x, mu, spk_e, cond, lens
        self.n_steps, self.next, self.slot = int(n_steps), 0, -1


class FlowSession:
    """A chain of estimator passes of the C++ solver that up to ``slots`` batches of the same frame count ``t`` share
    (include/session/astts_flow_session.h): a batch admitted while others are being solved JOINS them, and every launch of a pass carries
    the sequences of all of them, each batch at its own Euler step.  A batch's mel is bit-identical to ``FlowDecoder.solve`` of that
    batch alone (tested).  All calls enqueue on ``stream`` (the stream current at construction by default) and none waits for the GPU;
    they are not thread-safe: one thread drives a session."""

    def __init__(self, flow: FlowDecoder, t: int, slots: int = 4, rows_max: int = 32, stream=None):
        from .. import _lib_session
        self.flow, self.t, self.slots, self.rows_max = flow, int(t), int(slots), int(rows_max)
        self.stream = stream if stream is not None else torch.cuda.current_stream(flow.device)
        self._lib = _lib_session.load()
        self._tv, self._dv = flow._schedule()
        eng = flow._engine()
        need = int(self._lib.astts_flow_session_bytes(eng, self.t, self.slots, self.rows_max, len(self._tv)))
        if need == 0:
            raise ValueError(f"FlowSession: t={t} slots={slots} rows_max={rows_max} steps={len(self._tv)}")
        with torch.cuda.stream(self.stream):
            self._ws = torch.empty(need, dtype=torch.uint8, device=flow.device)
        h = ctypes.c_void_p()
        _lib.check(self._lib.astts_flow_session_create(eng, self.t, self.slots, self.rows_max, len(self._tv), self._ws.data_ptr(), need,
                                                       _lib.stream_ptr(self.stream), ctypes.byref(h)))
        self._h = h
        self._ctx: List[Optional[FlowJob]] = [None] * self.slots       # per slot: the job of the batch that holds it

    def close(self) -> None:
        if self._h is not None:
            h, self._h = self._h, None
            _lib.check(self._lib.astts_flow_session_destroy(h))

    def active(self) -> int:
        return sum(c is not None for c in self._ctx)

    def steps_left(self) -> List[int]:
        return [c.n_steps - c.next for c in self._ctx if c is not None]

    def can_admit(self, b: int, t: int) -> bool:
        return int(self._lib.astts_flow_session_can_admit(self._h, int(b), int(t), len(self._tv))) >= 0

    def state(self) -> List[int]:
        """active-slot mask, rows in use, passes enqueued, batches those passes carried (summed), steps left of slots 0..3"""
        out = (ctypes.c_int32 * 8)()
        _lib.check(self._lib.astts_flow_session_state(self._h, out))
        return list(out)

    def admit(self, x: torch.Tensor, mu: torch.Tensor, spk_e: torch.Tensor, cond: torch.Tensor,
              lens: Optional[torch.Tensor] = None) -> FlowJob:
        """The arguments of ``FlowDecoder.solve``: ``x`` [B, T, mel] (noise) is solved in place."""
        args = self.flow._batch_args(x, mu, spk_e, cond, lens, self._tv, self._dv)
        job = FlowJob(x, mu, spk_e, cond, lens, len(self._tv))
        slot = ctypes.c_int32(-1)
        with torch.cuda.stream(self.stream):
            _lib.check(self._lib.astts_flow_session_admit(self._h, *args, ctypes.byref(slot)))
        job.slot = int(slot.value)
        self._ctx[job.slot] = job
        return job

    def step(self, k: int = 1) -> List[FlowJob]:
        """Enqueue up to ``k`` estimator passes (with every batch's Euler update) over all admitted batches -> the jobs that ended."""
        mask = ctypes.c_uint32(0)
        k = int(k)
        with torch.cuda.stream(self.stream):
            _lib.check(self._lib.astts_flow_session_step(self._h, k, ctypes.byref(mask)))
        done = []
        for slot, c in enumerate(self._ctx):
            if c is None:
                continue
            c.next = min(c.n_steps, c.next + k)
            if mask.value >> slot & 1:
                done.append(c)
                self._ctx[slot] = None
        return done

    def run(self) -> None:
        """Enqueue every remaining step of the admitted batches."""
        while self.active():
            self.step(max(self.steps_left()))
