"""Models, seeded weights and inputs shared by test_xtts_cond_cpu.py and
test_xtts_cond_gpu.py.

Weights are random and scaled so that the activations stay O(1) through the blocks (conv and linear
weights N(0, gain / fan_in), norm gains 1 + 0.1 N, shifts and biases 0.1 N); ``proj_out`` is not zero (the
reference zero-initialises it, a trained checkpoint does not).

Composed outputs (``get_style_emb``, the latents) are held to the project's composed gates, tests/_util.py
``tol(mode)``: they meet them (DESIGN.md section 4 "XTTS conditioning", Parity), so no other yardstick is set."""
from __future__ import annotations

import functools
import math
from typing import Dict

import torch

import _xtts_cond_ref as R

MODELS: Dict[str, dict] = {
    # G = 32 with 4 channels per group; I = 341 (odd)
    "narrow": dict(model_dim=128, heads=2, attn_blocks=2, perceiver_depth=2),
    # head size 32; G = 32 with 3 channels per group; I = 256
    "narrow32": dict(model_dim=96, heads=3, attn_blocks=2, perceiver_depth=1),
    # the reference widths, one block and one layer: I = 2730, the qkv permutation at full width
    "reference1": dict(model_dim=1024, heads=16, attn_blocks=1, perceiver_depth=1),
}
MODEL_SEED = {"narrow": 31, "narrow32": 32, "reference1": 33}
NUM_LATENTS, DIM_HEAD, P_HEADS, FF_MULT = 32, 64, 8, 4
STYLE_T = (29, 65, 517)


def ff_inner(E: int) -> int:
    return int(E * FF_MULT * 2 / 3)


@functools.lru_cache(maxsize=None)
def state_dict(model: str) -> Dict[str, torch.Tensor]:
    c = MODELS[model]
    E, inner, I = c["model_dim"], P_HEADS * DIM_HEAD, ff_inner(c["model_dim"])
    g = torch.Generator().manual_seed(MODEL_SEED[model])

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    sd = {"conditioning_encoder.init.weight": rn(E, 80, 1, std=1.0 / 80**0.5),
          "conditioning_encoder.init.bias": rn(E, std=0.1)}
    for i in range(c["attn_blocks"]):
        p = f"conditioning_encoder.attn.{i}."
        sd[p + "norm.weight"] = 1.0 + rn(E, std=0.1)
        sd[p + "norm.bias"] = rn(E, std=0.1)
        sd[p + "qkv.weight"] = rn(3 * E, E, 1, std=1.5 / E**0.5)
        sd[p + "qkv.bias"] = rn(3 * E, std=0.1)
        sd[p + "proj_out.weight"] = rn(E, E, 1, std=1.0 / E**0.5)
        sd[p + "proj_out.bias"] = rn(E, std=0.1)
    sd["conditioning_perceiver.latents"] = rn(NUM_LATENTS, E, std=0.8)
    for i in range(c["perceiver_depth"]):
        p = f"conditioning_perceiver.layers.{i}."
        sd[p + "0.to_q.weight"] = rn(inner, E, std=1.0 / E**0.5)
        sd[p + "0.to_kv.weight"] = rn(2 * inner, E, std=1.0 / E**0.5)
        sd[p + "0.to_out.weight"] = rn(E, inner, std=0.7 / inner**0.5)
        sd[p + "1.0.weight"] = rn(2 * I, E, std=1.0 / E**0.5)
        sd[p + "1.0.bias"] = rn(2 * I, std=0.1)
        sd[p + "1.2.weight"] = rn(E, I, std=0.7 / I**0.5)
        sd[p + "1.2.bias"] = rn(E, std=0.1)
    sd["conditioning_perceiver.norm.gamma"] = 1.0 + rn(E, std=0.1)
    return sd


def ctor_kwargs(model: str) -> dict:
    return dict(MODELS[model], num_latents=NUM_LATENTS, perceiver_dim_head=DIM_HEAD, perceiver_heads=P_HEADS,
                ff_mult=FF_MULT)


@functools.lru_cache(maxsize=None)
def mel_input(T: int, B: int = 2) -> torch.Tensor:
    """A log-mel-like input [B, 80, T], O(1)."""
    g = torch.Generator().manual_seed(500 + T)
    return torch.randn(B, 80, T, generator=g) * 0.8 - 0.3


@functools.lru_cache(maxsize=None)
def style_oracle(model: str, T: int) -> torch.Tensor:
    """fp64 get_style_emb of mel_input(T) [2, E, 32], computed once and shared."""
    return R.style_emb(state_dict(model), mel_input(T), MODELS[model]["heads"], P_HEADS, DIM_HEAD)


@functools.lru_cache(maxsize=None)
def mel_norms() -> torch.Tensor:
    g = torch.Generator().manual_seed(77)
    return 2.0 + 3.0 * torch.rand(80, generator=g)


def clip(N: int, seed: int = 0, sr: int = 22050, amp: float = 0.4) -> torch.Tensor:
    """A reference-clip stand-in [1, N]: a 1 kHz sine, a 180 Hz sine and noise."""
    g = torch.Generator().manual_seed(900 + seed)
    t = torch.arange(N, dtype=torch.float64) / sr
    x = amp * (0.5 * torch.sin(2 * math.pi * 1000.0 * t) + 0.4 * torch.sin(2 * math.pi * 180.0 * t + 0.3))
    x = x + 0.1 * torch.randn(N, generator=g, dtype=torch.float64)
    return x.clamp(-1, 1).float()[None]


def full_checkpoint(model: str, gpt_sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A synthetic full XTTS checkpoint: the GPT's keys and the conditioning keys under ``gpt.``, decoder and
    speaker-encoder stand-ins under ``hifigan_decoder.``, and ``mel_stats``."""
    full = {"gpt." + k: v for k, v in gpt_sd.items()}
    full.update({"gpt." + k: v for k, v in state_dict(model).items()})
    full["gpt.gpt_inference.transformer.h.0.ln_1.weight"] = torch.ones(4)
    full["hifigan_decoder.waveform_decoder.conv_pre.weight"] = torch.zeros(2, 2, 7)
    full["hifigan_decoder.speaker_encoder.conv1.weight"] = torch.zeros(2, 1, 3, 3)
    full["mel_stats"] = mel_norms()
    return full
