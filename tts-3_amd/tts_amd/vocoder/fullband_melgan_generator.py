"""Drop-in ``FullbandMelganGenerator`` (``TTS/vocoder/models/fullband_melgan_generator.py``, Coqui TTS
0.22.0): ``MelganGenerator`` with other defaults; see ``melgan_generator.py`` for the math modes."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .melgan_generator import MelganGenerator


class FullbandMelganGenerator(MelganGenerator):
    def __init__(
        self,
        in_channels: int = 80,
        out_channels: int = 1,
        proj_kernel: int = 7,
        base_channels: int = 512,
        upsample_factors: Sequence[int] = (2, 8, 2, 2),
        res_kernel: int = 3,
        num_res_blocks: int = 4,
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

    @torch.no_grad()
    def inference(self, cond_features: torch.Tensor) -> torch.Tensor:
        return self._run(cond_features, self.inference_padding, 0)
