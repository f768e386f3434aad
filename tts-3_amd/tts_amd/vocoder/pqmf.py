"""``PQMF`` of the multi-band MelGAN generator (``TTS/vocoder/layers/pqmf.py``, Coqui TTS 0.22.0).

The buffers ``H``, ``G`` and ``updown_filter`` are built exactly as the reference builds them (they
are part of a checkpoint's state dict).  ``synthesis`` runs ``tts_pqmf_synthesis`` on the ROCm
device: the zero-stuffing ``conv_transpose1d`` followed by the ``conv1d`` with ``G`` is evaluated in
its polyphase form (taps + 1 products per output sample instead of N (taps + 1), no zero-stuffed
intermediate).  ``analysis`` is used in training only and raises ``NotImplementedError``.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .. import _native as _nat


def _firwin_kaiser(numtaps: int, cutoff: float, beta: float) -> np.ndarray:
    """``scipy.signal.firwin(numtaps, cutoff, window=("kaiser", beta))``; scipy's own when present."""
    try:
        from scipy.signal import firwin
    except ImportError:
        m = np.arange(numtaps) - 0.5 * (numtaps - 1)
        h = cutoff * np.sinc(cutoff * m) * np.kaiser(numtaps, beta)
        return h / h.sum()
    return firwin(numtaps, cutoff, window=("kaiser", beta))


class PQMF(nn.Module):
    def __init__(self, N: int = 4, taps: int = 62, cutoff: float = 0.15, beta: float = 9.0):  # noqa: N803
        super().__init__()
        self.N = N
        self.taps = taps
        self.cutoff = cutoff
        self.beta = beta

        QMF = _firwin_kaiser(taps + 1, cutoff, beta)  # noqa: N806
        H = np.zeros((N, len(QMF)))  # noqa: N806
        G = np.zeros((N, len(QMF)))  # noqa: N806
        for k in range(N):
            constant_factor = (2 * k + 1) * (np.pi / (2 * N)) * (np.arange(taps + 1) - ((taps - 1) / 2))
            phase = (-1) ** k * np.pi / 4
            H[k] = 2 * QMF * np.cos(constant_factor + phase)
            G[k] = 2 * QMF * np.cos(constant_factor - phase)
        H = torch.from_numpy(H[:, None, :]).float()  # noqa: N806
        G = torch.from_numpy(G[None, :, :]).float()  # noqa: N806
        self.register_buffer("H", H)
        self.register_buffer("G", G)
        updown_filter = torch.zeros((N, N, N)).float()
        for k in range(N):
            updown_filter[k, k, 0] = 1.0
        self.register_buffer("updown_filter", updown_filter)

    def forward(self, x):
        return self.analysis(x)

    def analysis(self, x):
        raise NotImplementedError("PQMF.analysis is training-only; tts_amd implements inference (PQMF.synthesis)")

    @torch.no_grad()
    def synthesis(self, x: torch.Tensor) -> torch.Tensor:
        """[B, N, L] sub-bands -> [B, 1, N L]."""
        if self.G.device.type != "cuda":
            raise RuntimeError(
                "PQMF (tts_amd) runs only on a ROCm device: move the module with .to('cuda') first "
                "(there is no CPU fallback)"
            )
        if x.dim() != 3 or x.shape[1] != self.N:
            raise ValueError(f"expected [B, {self.N}, L] sub-bands, got shape {tuple(x.shape)}")
        dev = self.G.device
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        B, _, L = x.shape
        out = torch.empty(B, 1, self.N * L, device=dev, dtype=torch.float32)
        g = self.G.to(torch.float32).contiguous()
        _nat.call("tts_pqmf_synthesis", _nat.ptr(x), B, self.N, L, _nat.ptr(g), self.taps, _nat.ptr(out),
                  _nat.stream_ptr(dev))
        return out
