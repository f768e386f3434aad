"""Models, seeds, cases and margins shared by test_xtts_gpt_cpu.py and test_xtts_gpt_gpu.py.

The GPU tests compare discrete choices (greedy codes, sampled tokens) with the fp64 oracle's, which is
only meaningful when the oracle's own choice is not a near tie.  The conditions below (``MARGIN``) are
checked on the oracle alone by the CPU tests, for every case and every step, and the seeds here are
chosen so that it passes them all.

MARGIN: 100 x the fp32 logit error measured on the GPU.  The worst |logit - oracle| measured on MI355X
over the fp32 cases of test_xtts_gpt_gpu.py is 3.8e-6 (narrow), 2.6e-6 (narrow32) and 7.1e-6
(reference2), so 100 x the largest is 7.1e-4; the margin stays at the provisional 1e-3, which is above it.
The sample-op cases take their logits as given (no model in front), so their margins only have to cover the
kernel's own fp32 arithmetic (one division, expf, 2^-40 fixed point); they are held to the same 1e-3.
"""
from __future__ import annotations

import itertools
from typing import Dict

import torch

MARGIN = 1e-3
LOGIT_ERR_FP32 = {"narrow": 3.8e-6, "narrow32": 2.6e-6, "reference2": 7.1e-6}

_NARROW = dict(layers=2, model_dim=128, heads=2, n_text=40, n_audio=67, start_text=39, stop_text=0,
               start_audio=65, stop_audio=66, text_positions=12, mel_positions=40, P=5)
MODELS: Dict[str, dict] = {
    "narrow": dict(_NARROW),
    "narrow32": dict(_NARROW, heads=4),
    "reference2": dict(layers=2, model_dim=1024, heads=16, n_text=96, n_audio=1026, start_text=95, stop_text=0,
                       start_audio=1024, stop_audio=1025, text_positions=16, mel_positions=40, P=32),
}
MODEL_SEED = {"narrow": 11, "narrow32": 12, "reference2": 13}


def ctor_kwargs(cfg: dict) -> dict:
    """Constructor keywords of tts_amd.tts.XttsGPT (the reference GPT's) for a model."""
    return dict(layers=cfg["layers"], model_dim=cfg["model_dim"], heads=cfg["heads"],
                max_text_tokens=cfg["text_positions"] - 2, max_mel_tokens=cfg["mel_positions"] - 3,
                max_conditioning_inputs=1, number_text_tokens=cfg["n_text"], num_audio_tokens=cfg["n_audio"],
                start_text_token=cfg["start_text"], stop_text_token=cfg["stop_text"],
                start_audio_token=cfg["start_audio"], stop_audio_token=cfg["stop_audio"])


def state_dict(cfg: dict, seed: int) -> Dict[str, torch.Tensor]:
    """Random fp32 weights with the checkpoint's keys, scaled so that the hidden states stay O(1) through
    the layers and the logits spread by O(1)."""
    g = torch.Generator().manual_seed(seed)
    E, L = cfg["model_dim"], cfg["layers"]

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    sd = {
        "text_embedding.weight": rn(cfg["n_text"], E, std=0.7),
        "mel_embedding.weight": rn(cfg["n_audio"], E, std=0.7),
        "text_pos_embedding.emb.weight": rn(cfg["text_positions"], E, std=0.5),
        "mel_pos_embedding.emb.weight": rn(cfg["mel_positions"], E, std=0.5),
    }
    for i in range(L):
        p = f"gpt.h.{i}."
        for ln in ("ln_1", "ln_2"):
            sd[p + ln + ".weight"] = 1.0 + rn(E, std=0.1)
            sd[p + ln + ".bias"] = rn(E, std=0.1)
        sd[p + "attn.c_attn.weight"] = rn(E, 3 * E, std=1.5 / E**0.5)
        sd[p + "attn.c_attn.bias"] = rn(3 * E, std=0.1)
        sd[p + "attn.c_proj.weight"] = rn(E, E, std=1.0 / E**0.5)
        sd[p + "attn.c_proj.bias"] = rn(E, std=0.1)
        sd[p + "mlp.c_fc.weight"] = rn(E, 4 * E, std=1.0 / E**0.5)
        sd[p + "mlp.c_fc.bias"] = rn(4 * E, std=0.1)
        sd[p + "mlp.c_proj.weight"] = rn(4 * E, E, std=1.0 / (4 * E) ** 0.5)
        sd[p + "mlp.c_proj.bias"] = rn(E, std=0.1)
    for ln in ("gpt.ln_f", "final_norm"):
        sd[ln + ".weight"] = 1.0 + rn(E, std=0.1)
        sd[ln + ".bias"] = rn(E, std=0.1)
    sd["text_head.weight"] = rn(cfg["n_text"], E, std=1.0 / E**0.5)
    sd["text_head.bias"] = rn(cfg["n_text"], std=0.1)
    sd["mel_head.weight"] = rn(cfg["n_audio"], E, std=1.5 / E**0.5)
    sd["mel_head.bias"] = rn(cfg["n_audio"], std=0.3)
    return sd


def inputs(cfg: dict, seed: int, B: int, T: int):
    """(cond [B, P, E] fp32, text [B, T] int64 without the start / stop ids)."""
    g = torch.Generator().manual_seed(1000 + seed)
    cond = torch.randn(B, cfg["P"], cfg["model_dim"], generator=g) * 0.8
    text = torch.randint(1, cfg["n_text"] - 1, (B, T), generator=g)
    return cond, text


# ---- free-run cases: (model, input seed, B, T_text, text lengths or None, steps, repetition penalty) ----
FREE_RUN = {
    "narrow_greedy24": ("narrow", 1, 2, 7, None, 24, 10.0),
    "narrow32_greedy24": ("narrow32", 2, 2, 7, None, 24, 10.0),
    "narrow_ragged": ("narrow", 3, 3, 9, [9, 4, 6], 12, 10.0),
    "reference2_6": ("reference2", 4, 2, 6, None, 6, 10.0),
}

# ---- stopping: mel_head's stop-row bias raised so that the ragged batch ends at three different steps
# (the oracle ends the utterances after 21, 23 and 12 codes of at most 30) ----
STOP_CASE = dict(model="narrow", seed=21, B=3, T=8, lens=[8, 5, 3], steps=30, penalty=10.0, stop_bias=2.0,
                 n=[21, 23, 12])


def stop_state_dict():
    cfg = MODELS[STOP_CASE["model"]]
    sd = state_dict(cfg, MODEL_SEED[STOP_CASE["model"]])
    sd["mel_head.bias"][cfg["stop_audio"]] += STOP_CASE["stop_bias"]
    return sd


# ---- a sampled free run with the reference's defaults (top_k 50, top_p 0.85, temperature 0.75, penalty 10) ----
SAMPLED_RUN = dict(model="narrow", seed=9, B=2, T=6, steps=6, useed=5, top_k=50, top_p=0.85, temperature=0.75,
                   penalty=10.0)


def sampled_run_uniforms():
    s = SAMPLED_RUN
    return torch.rand(s["B"], s["steps"], generator=torch.Generator().manual_seed(s["useed"]))


# ---- sample-op cases: normal logits of V tokens, previous codes, every processor combination ----
# The draw margin asks that u sits 1e-3 of probability inside the drawn token's CDF interval, so that
# token needs some probability: the logits' spread grows with V to keep the distribution peaked.
SAMPLE_V = (67, 1026, 8194)
SAMPLE_STD = {67: 2.0, 1026: 3.0, 8194: 4.0}
SAMPLE_SEED = {67: 10, 1026: 37, 8194: 18}
SAMPLE_PREV = 9  # earlier codes per row (with a repeat)


def sample_combos(V: int):
    """(top_k, top_p, repetition penalty, temperature): every combination the issue lists."""
    return list(itertools.product((1, 50, V), (0.85, 1.0), (1.0, 10.0), (0.75, 1.0)))


def sample_case(V: int, B: int = 2):
    """(logits [B, V] fp32, prev [B, SAMPLE_PREV] int64, u [B] fp32)."""
    g = torch.Generator().manual_seed(SAMPLE_SEED[V])
    logits = torch.randn(B, V, generator=g) * SAMPLE_STD[V]
    prev = torch.randint(0, V, (B, SAMPLE_PREV), generator=g)
    prev[:, -1] = prev[:, 0]
    u = torch.rand(B, generator=g)
    return logits, prev, u
