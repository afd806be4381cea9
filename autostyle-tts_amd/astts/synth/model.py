"""Synthesis engine: acoustic transformer -> flow-matching decoder -> HiFT vocoder on one MI355X.

This is the arithmetic the reference reaches through ``cosyvoice.inference_tts_with_st``
(/root/reference/tts_with_rag.py:195, tts_with_style_and_timbre.py:93), ``inference_zero_shot``
(:133 / :47) and ``inference_vc`` (:141 / :57).  Every tensor operation below is a hand-written
HIP kernel reached through astts.ops (C ABI); torch only owns the HBM buffers, views and
concatenations.  Activations are fp32 channels-last, weights fp16 (packed once at load), all
contractions run on fp16 MFMA with fp32 accumulation.

Randomness is injected by the caller (sampling uniforms, CFM start noise, source phases/noise) so
that the CPU oracle (oracle/synth.py) can be driven with identical draws.

By concern: ``encoder`` (the shared relative-position encoder), ``lm`` (acoustic LM and its decode engine), ``decode`` (decode
state, sessions, 32-row groups), ``flow``, ``vocoder``, ``pipeline`` (the stream pipeline over batches).  This module holds the
three stages put together and re-exports the public names of the others.
"""
from __future__ import annotations

from typing import Dict

import torch

from .config import SynthConfig
from .decode import LmSession, Prefill
from .encoder import SD, RelPosEncoder, fold_layernorm, rel_pos_table
from .flow import FlowDecoder
from .lm import AcousticLM
from .pipeline import PipelinedSynth
from .vocoder import HiftVocoder

__all__ = ["AcousticLM", "FlowDecoder", "HiftVocoder", "LmSession", "PipelinedSynth", "RelPosEncoder", "SynthEngine",
           "fold_layernorm", "rel_pos_table"]


class SynthEngine:
    """All three stages on one GPU."""

    def __init__(self, state: Dict[str, SD], cfg: SynthConfig, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("astts.synth needs a ROCm GPU; there is no CPU fallback in the product path")
        self.cfg = cfg
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self.lm = AcousticLM(state["llm"], cfg, self.device)
            self.flow = FlowDecoder(state["flow"], cfg, self.device)
            self.hift = HiftVocoder(state["hift"], cfg, self.device)

    def tts(self, text, text_lens, lm_spk, lm_prompt_tokens, n_tokens: int, uniforms, flow_prompt_tokens, flow_prompt_mel,
            flow_spk, z, phase0, noise, forced_tokens=None, wide: bool = False):
        """One fixed-length batch end to end (all inputs on the GPU):
        LM decode (style-conditioned) -> flow (timbre-conditioned) -> vocoder.  Returns
        (tokens [B, n_tokens], mel [B, Tm, 80], wav [B, 256*Tm])."""
        toks = self.tts_tokens(text, text_lens, lm_spk, lm_prompt_tokens, n_tokens, uniforms, forced_tokens, wide)
        mel, wav = self.tts_render(toks, flow_prompt_tokens, flow_prompt_mel, flow_spk, z, phase0, noise)
        return toks, mel, wav

    # the two halves of tts(): the latency-bound autoregressive stage and the throughput-bound rendering stage
    def tts_tokens(self, text, text_lens, lm_spk, lm_prompt_tokens, n_tokens: int, uniforms, forced_tokens=None, wide: bool = False) -> torch.Tensor:
        pre = self.lm.prefix(text, text_lens, lm_spk, lm_prompt_tokens)
        return self.lm.decode(pre, n_tokens, uniforms, ignore_eos=True, forced_tokens=forced_tokens, wide=wide)

    # the same in two halves (<= 32 rows): what precedes the first sampled token, and the decode steps (PipelinedSynth)
    def tts_prefill(self, text, text_lens, lm_spk, lm_prompt_tokens, n_tokens: int) -> Prefill:
        return self.lm.prefill(self.lm.prefix(text, text_lens, lm_spk, lm_prompt_tokens), n_tokens)

    def tts_decode(self, state: Prefill, uniforms, forced_tokens=None) -> torch.Tensor:
        return self.lm.decode_prefilled(state, uniforms, ignore_eos=True, forced_tokens=forced_tokens)

    def tts_render(self, toks, flow_prompt_tokens, flow_prompt_mel, flow_spk, z, phase0, noise):
        cfg = self.cfg
        all_tok = torch.cat([flow_prompt_tokens.to(torch.int32), toks], dim=1)
        b = all_tok.shape[0]
        tok_lens = torch.full((b,), all_tok.shape[1], dtype=torch.int32, device=self.device)
        mel_total = flow_prompt_mel.shape[1] + cfg.mel_frames_for_tokens(toks.shape[1])
        mel = self.flow.decode(all_tok, tok_lens, flow_prompt_mel, flow_spk, z, mel_total)
        wav = self.hift.forward(mel, phase0, noise)
        return mel, wav
