"""Drop-in ``MultibandMelganGenerator`` (``TTS/vocoder/models/multiband_melgan_generator.py``, Coqui
TTS 0.22.0): a ``MelganGenerator`` that emits ``out_channels`` sub-bands, and a ``PQMF`` that merges
them.  ``forward`` returns the sub-bands ``[B, 4, L]``; ``inference`` returns
``pqmf_layer.synthesis(layers(padded))``, ``[B, 1, 4 L]``, with the synthesis fused into the last
launch (the sub-bands never reach HBM).  Math modes: see ``melgan_generator.py``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .hifigan_generator import _host
from .melgan_generator import MelganGenerator
from .pqmf import PQMF


class MultibandMelganGenerator(MelganGenerator):
    def __init__(
        self,
        in_channels: int = 80,
        out_channels: int = 4,
        proj_kernel: int = 7,
        base_channels: int = 384,
        upsample_factors: Sequence[int] = (2, 8, 2, 2),
        res_kernel: int = 3,
        num_res_blocks: int = 3,
        math_mode: Optional[str] = None,
    ):
        super().__init__(
            in_channels=in_channels,
            out_channels=out_channels,
            proj_kernel=proj_kernel,
            base_channels=base_channels,
            upsample_factors=upsample_factors,
            res_kernel=res_kernel,
            num_res_blocks=num_res_blocks,
            math_mode=math_mode,
        )
        self.pqmf_layer = PQMF(N=4, taps=62, cutoff=0.15, beta=9.0)
        self._cfg.pqmf_bands = self.pqmf_layer.N
        self._cfg.pqmf_taps = self.pqmf_layer.taps
        self._validate_cfg()

    def _extra_weights(self) -> List[np.ndarray]:
        return [_host(self.pqmf_layer.G)]

    def pqmf_analysis(self, x):
        return self.pqmf_layer.analysis(x)

    def pqmf_synthesis(self, x):
        return self.pqmf_layer.synthesis(x)

    @torch.no_grad()
    def inference(self, cond_features: torch.Tensor) -> torch.Tensor:
        return self._run(cond_features, self.inference_padding, 1)
