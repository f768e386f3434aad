"""Tacotron2 configurations, seeded state dicts, inputs and oracle outputs shared by the CPU and GPU
tests (computed once per process and never modified)."""
from __future__ import annotations

import functools

import torch

import _tacotron2_ref as R
from tts_amd import synthetic
from tts_amd.config import TACOTRON2

ATTN_TILE = 128  # encoder positions one pass of the attention kernel covers (csrc/tacotron2.hpp kT2AttnTile)
NARROW = dict(encoder_dim=64, query_dim=96, prenet_dim=32, attention_dim=24, location_filters=8,
              location_kernel_size=31)
MODELS = {
    # every width narrow, a speaker embedding
    "narrow": dict(TACOTRON2, **NARROW, num_chars=30, out_channels=20, num_speakers=3, use_speaker_embedding=True,
                   speaker_embedding_dim=16),
    "narrow_dvec": dict(TACOTRON2, **NARROW, num_chars=30, out_channels=20, use_d_vector_file=True, d_vector_dim=12),
    # 80 mel channels for the vocoder
    "narrow80": dict(TACOTRON2, **NARROW, num_chars=30, out_channels=80),
    # the reference's widths
    "reference": dict(TACOTRON2, num_chars=60, out_channels=80),
}
SEEDS = {"narrow": 36, "narrow_dvec": 34, "narrow80": 33, "reference": 34}
SPEAKERS = (2, 0, 1, 1)


def model_args(name: str, r: int = 2, attention_norm: str = "sigmoid") -> dict:
    return dict(MODELS[name], r=r, attention_norm=attention_norm)


@functools.lru_cache(maxsize=None)
def state_dict(name: str, r: int = 2, attention_norm: str = "sigmoid"):
    # the v layer's scale follows the normalisation
    return synthetic.tacotron2_state_dict(model_args(name, r, attention_norm), seed=SEEDS[name] + 100 * r)


def tokens(B: int, T: int, seed: int) -> torch.Tensor:
    # ids >= 1: id 0 is the padding row
    return 1 + synthetic.tokens(B, T, 29, seed=seed)


def d_vectors(B: int) -> torch.Tensor:
    return torch.randn(B, 12, generator=torch.Generator().manual_seed(77)) * 0.3


def edge_lengths(T: int):
    """(T_en, tile edge, tile edge + 1, 1), clipped to T_en."""
    return (T, min(T, ATTN_TILE), min(T, ATTN_TILE + 1), 1)


# around the location kernel's halo (15), three past the first tile edge, and 257: three tile passes of the
# attention kernel, the middle one with both halos in neighbouring tiles
EDGE_T = (1, 7, 31, 33, ATTN_TILE + 3, 2 * ATTN_TILE + 1)

# ---- the cases: name -> (model, r, norm, B, T_en, token seed, lengths or None, steps, stop_threshold)
STOP_OFF = 2.0
CASES = {
    "free": ("narrow", 2, "sigmoid", 3, 23, 5, (23, 16, 9), 40, STOP_OFF),
    "free_softmax": ("narrow", 2, "softmax", 3, 23, 5, (23, 16, 9), 40, STOP_OFF),
    "free_dvec": ("narrow_dvec", 2, "sigmoid", 3, 23, 6, (23, 16, 9), 40, STOP_OFF),
    "chunk": ("narrow", 2, "sigmoid", 3, 23, 5, (23, 16, 9), 11, STOP_OFF),
    "reference": ("reference", 2, "sigmoid", 2, 19, 8, None, 12, STOP_OFF),
    "synth": ("narrow80", 2, "sigmoid", 2, 17, 9, (17, 11), 14, STOP_OFF),
}
for _T in EDGE_T:
    CASES[f"edge{_T}"] = ("narrow", 2, "sigmoid", 4, _T, 40 + _T, edge_lengths(_T), 6, STOP_OFF)
for _s in (1, 2):
    for _r in (1, 2, 3):
        for _n in ("sigmoid", "softmax"):
            CASES[f"few_s{_s}_r{_r}_{_n}"] = ("narrow", _r, _n, 2, 13, 3, None, _s, STOP_OFF)
# the stop case: 24 steps of the free inputs; the threshold is chosen from the oracle's trajectories
STOP_STEPS = 24
CASES["stop_probe"] = ("narrow", 2, "sigmoid", 3, 23, 5, (23, 16, 9), STOP_STEPS, STOP_OFF)

# Whether the device is held to the gates on the long free-running cases: only where torch's own CPU
# evaluation of the oracle in that arithmetic (fp32; bf16-rounded RNN matrices and conv operands) stays inside half of them
# (test_tacotron2_cpu.py measures this and checks these entries); else the error is logged only.
FP32_GATED = {"free": True, "free_softmax": True, "free_dvec": True, "reference": True}
# bf16 "free": the analogue's model_outputs are 2.9e-2 off at the worst element, half a gate is 2.5e-2
BF16_GATED = {"free": False, "free_softmax": True, "free_dvec": True, "reference": True}


def case_inputs(name: str):
    model, r, norm, B, T, seed, lengths, steps, thr = CASES[name]
    kw = {}
    if lengths is not None:
        kw["x_lengths"] = torch.tensor(lengths)
    if MODELS[model].get("use_speaker_embedding"):
        kw["speaker_ids"] = torch.tensor(SPEAKERS[:B])
    if MODELS[model].get("use_d_vector_file"):
        kw["d_vectors"] = d_vectors(B)
    return tokens(B, T, seed), kw


def bf16_round(w: torch.Tensor) -> torch.Tensor:
    return w.to(torch.bfloat16).to(w.dtype)


@functools.lru_cache(maxsize=None)
def reference(name: str, arith: str = "fp64", stop_threshold: float | None = None):
    """The oracle's outputs of a case: arith "fp64", "fp32" (its own fp32 evaluation) or "bf16w" (fp32
    with the four big RNN matrices and the operands of every conv rounded to bf16: the bf16 mode's analogue)."""
    model, r, norm, B, T, seed, lengths, steps, thr = CASES[name]
    tok, kw = case_inputs(name)
    return R.inference(state_dict(model, r, norm), model_args(model, r, norm), tok, **kw,
                       stop_threshold=thr if stop_threshold is None else stop_threshold, max_decoder_steps=steps,
                       dtype=torch.float64 if arith == "fp64" else torch.float32,
                       weight_cast=bf16_round if arith == "bf16w" else None)


@functools.lru_cache(maxsize=None)
def stop_threshold():
    """A threshold on the 24-step stop trajectories of "stop_probe" such that (a) at least two utterances
    stop at different steps >= 1, (b) one never stops, (c) every stop probability up to and including each
    stop step is at least 1e-3 from the threshold.  Returns (threshold, expected steps [B])."""
    p = reference("stop_probe")["stop_tokens"]  # [B, 24]
    B, S = p.shape
    best = None
    for cand in torch.unique(p[:, 1:]).tolist():
        thr = cand - 2e-3
        steps = []
        for b in range(B):
            hit = [t for t in range(1, S) if p[b, t] > thr]
            steps.append(hit[0] + 1 if hit else S)
        stopped = sorted({s for s in steps if s < S})
        if len(stopped) < 2 or steps.count(S) < 1:
            continue
        margin = min(float((p[b, 1 : steps[b]] - thr).abs().min()) for b in range(B))
        if margin >= 1e-3 and (best is None or margin > best[2]):
            best = (thr, tuple(steps), margin)
    assert best is not None, "no threshold meets the stop test's conditions: change the seed"
    return best[0], best[1]
