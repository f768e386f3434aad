"""The whole-generator cases the MelGAN CPU and GPU tests share: the three zoo configurations, their
synthetic state dicts and the fp64 oracle outputs (computed once per process)."""
from __future__ import annotations

import functools

import torch

import _melgan_ref as R
from tts_amd import synthetic
from tts_amd.config import FULLBAND_MELGAN, MELGAN, MULTIBAND_MELGAN

# name -> (class name in tts_amd.vocoder, constructor arguments, has a PQMF)
CONFIGS = {
    "multiband": ("MultibandMelganGenerator", dict(in_channels=80, out_channels=4, base_channels=384, **MULTIBAND_MELGAN), True),
    "fullband": ("FullbandMelganGenerator", dict(in_channels=80, out_channels=1, base_channels=512, **FULLBAND_MELGAN), False),
    "melgan": ("MelganGenerator", dict(in_channels=80, out_channels=1, base_channels=512, **MELGAN), False),
}
# (config, B, T): T = 61 puts more than one 64-column tile in the multi-band generator's first stack
CASES = [("multiband", 3, 1), ("multiband", 2, 12), ("multiband", 2, 61), ("fullband", 1, 5), ("melgan", 1, 5)]
CASE_IDS = [f"{c}_b{b}_t{t}" for c, b, t in CASES]
# (config, B, T, inference): forward (no inference padding) reflect-pads the mel itself by 3, which
# torch refuses for T <= 3, so the T = 1 case runs as inference only (its forward must raise)
RUNS = [(c, b, t, inf) for c, b, t in CASES for inf in (False, True) if inf or t > 3]
RUN_IDS = [f"{c}_b{b}_t{t}_{'inference' if inf else 'forward'}" for c, b, t, inf in RUNS]
# The oracle's own fp32 forward is about 1e-6 rel-RMS off its fp64 forward on these generators (20 to
# 50 convs deep; conv_pre alone gives 3e-7): 0.84e-6 to 1.9e-6 over 26 seeds tried.  This seed is the
# best-conditioned of them (worst case 8.4e-7, waveform std 0.077 .. 0.130), which keeps the fp32 gates
# (rel-RMS 5e-6) at five times the reference's own error.
SEED = 26


@functools.lru_cache(maxsize=None)
def state_dict(config: str, weight_norm: bool = True):
    _, ctor, pqmf = CONFIGS[config]
    return synthetic.melgan_state_dict(**ctor, pqmf=pqmf, seed=SEED, weight_norm=weight_norm)


def ref_cfg(config: str) -> dict:
    ctor = CONFIGS[config][1]
    return dict(upsample_factors=ctor["upsample_factors"], num_res_blocks=ctor["num_res_blocks"])


def mel(B: int, T: int) -> torch.Tensor:
    return synthetic.mel(B, T, seed=100 * B + T)


@functools.lru_cache(maxsize=None)
def oracle(config: str, B: int, T: int, inference: bool, dtype=torch.float64) -> torch.Tensor:
    """fp64 (or fp32) CPU output of forward / inference; do not modify the returned tensor."""
    pqmf = CONFIGS[config][2]
    with torch.no_grad():
        return R.melgan_forward(state_dict(config), mel(B, T), pad=2 if inference else 0, synth=inference and pqmf,
                                dtype=dtype, **ref_cfg(config))
