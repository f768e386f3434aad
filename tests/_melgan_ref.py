"""fp64 / fp32 oracle of the MelGAN family for the tests: a ``torch.nn.functional`` restatement of
``TTS/vocoder/models/{melgan,multiband_melgan,fullband_melgan}_generator.py``, ``layers/melgan.py``
and ``layers/pqmf.py`` (Coqui TTS 0.22.0) that works from a state dict.  Shares no code with
``tts_amd.vocoder``."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def folded(sd, name: str, dtype) -> torch.Tensor:
    """The conv weight of ``name``: plain, or torch's own weight-norm fold of (original0 = g, original1 = v)."""
    if f"{name}.weight" in sd:
        return sd[f"{name}.weight"].to(dtype)
    g = sd[f"{name}.parametrizations.weight.original0"]
    v = sd[f"{name}.parametrizations.weight.original1"]
    return torch._weight_norm(v, g, 0).to(dtype)


def bias(sd, name: str, dtype) -> torch.Tensor:
    return sd[f"{name}.bias"].to(dtype)


def res_block(x, w1, b1, w2, b2, ws, bs, dilation: int, zero_pad: bool = False):
    """shortcut(x) + block(x) of one ResidualStack block; ``zero_pad`` swaps the reflection for zeros."""
    k = w1.shape[-1]
    p = ((k - 1) // 2) * dilation
    h = F.leaky_relu(x, 0.2)
    h = F.pad(h, (p, p)) if zero_pad else F.pad(h, (p, p), "reflect")
    h = F.conv1d(h, w1, b1, dilation=dilation)
    h = F.conv1d(F.leaky_relu(h, 0.2), w2, b2)
    return F.conv1d(x, ws, bs) + h


def melgan_layers(sd, c, upsample_factors, num_res_blocks: int, res_kernel: int = 3, proj_kernel: int = 7,
                  dtype=torch.float64, counter=None) -> torch.Tensor:
    """``self.layers(c)``.  ``counter``: a dict that receives the MACs of every conv, by layer name."""
    def count(name, w, columns):
        # conv [Cout][Cin][K]: Cout Cin K MACs per output column; conv_transpose [Cin][Cout][K]: per input column
        if counter is not None:
            counter[name] = counter.get(name, 0) + w.numel() * columns

    x = c.to(dtype)
    p = (proj_kernel - 1) // 2
    w = folded(sd, "layers.1", dtype)
    x = F.conv1d(F.pad(x, (p, p), "reflect"), w, bias(sd, "layers.1", dtype))
    count("conv_pre", w, x.shape[0] * x.shape[-1])
    for i, u in enumerate(upsample_factors):
        name = f"layers.{3 + 3 * i}"
        w = folded(sd, name, dtype)
        count(f"ups.{i}", w, x.shape[0] * x.shape[-1])
        x = F.conv_transpose1d(F.leaky_relu(x, 0.2), w, bias(sd, name, dtype), stride=u, padding=u // 2 + u % 2,
                               output_padding=u % 2)
        st = f"layers.{4 + 3 * i}"
        for j in range(num_res_blocks):
            ws = [folded(sd, f"{st}.blocks.{j}.2", dtype), folded(sd, f"{st}.blocks.{j}.4", dtype),
                  folded(sd, f"{st}.shortcuts.{j}", dtype)]
            x = res_block(x, ws[0], bias(sd, f"{st}.blocks.{j}.2", dtype), ws[1], bias(sd, f"{st}.blocks.{j}.4", dtype),
                          ws[2], bias(sd, f"{st}.shortcuts.{j}", dtype), res_kernel**j)
            for wj in ws:
                count(f"stack.{i}", wj, x.shape[0] * x.shape[-1])
    n = len(upsample_factors)
    name = f"layers.{4 + 3 * n}"
    w = folded(sd, name, dtype)
    x = F.conv1d(F.pad(F.leaky_relu(x, 0.2), (p, p), "reflect"), w, bias(sd, name, dtype))
    count("tail", w, x.shape[0] * x.shape[-1])
    return torch.tanh(x)


def melgan_forward(sd, c, pad: int = 0, synth: bool = False, dtype=torch.float64, **cfg) -> torch.Tensor:
    """forward (pad 0) / inference (pad 2: replicate) of the three generators; ``synth``: the
    multi-band generator's PQMF synthesis of the sub-bands with the state dict's own filters."""
    x = c.to(dtype)
    if pad:
        x = F.pad(x, (pad, pad), "replicate")
    y = melgan_layers(sd, x, dtype=dtype, **cfg)
    if synth:
        y = pqmf_synthesis(y, sd["pqmf_layer.G"].to(dtype), sd["pqmf_layer.updown_filter"].to(dtype))
    return y


def pqmf_filters(N: int = 4, taps: int = 62, cutoff: float = 0.15, beta: float = 9.0):
    """(H [N,1,taps+1], G [1,N,taps+1], updown [N,N,N]) in float32, the scipy formula of layers/pqmf.py."""
    from scipy.signal import firwin

    qmf = firwin(taps + 1, cutoff, window=("kaiser", beta))
    H = np.zeros((N, len(qmf)))
    G = np.zeros((N, len(qmf)))
    for k in range(N):
        cf = (2 * k + 1) * (np.pi / (2 * N)) * (np.arange(taps + 1) - ((taps - 1) / 2))
        phase = (-1) ** k * np.pi / 4
        H[k] = 2 * qmf * np.cos(cf + phase)
        G[k] = 2 * qmf * np.cos(cf - phase)
    up = torch.zeros(N, N, N)
    for k in range(N):
        up[k, k, 0] = 1.0
    return torch.from_numpy(H[:, None, :]).float(), torch.from_numpy(G[None, :, :]).float(), up


def pqmf_synthesis(x, G, updown) -> torch.Tensor:
    """PQMF.synthesis: conv_transpose1d with updown_filter * N (zero stuffing), then conv1d with G."""
    N = G.shape[1]
    taps = G.shape[-1] - 1
    x = F.conv_transpose1d(x, updown * N, stride=N)
    return F.conv1d(x, G, padding=taps // 2)


def pqmf_polyphase(x: np.ndarray, G: np.ndarray) -> np.ndarray:
    """y[n] = N sum_k sum_{j: (n + j - taps/2) % N == 0, 0 <= m < L} G[k][j] x_k[m], m = (n + j - taps/2) / N."""
    B, N, L = x.shape
    taps = G.shape[-1] - 1
    g = G.reshape(N, taps + 1)
    y = np.zeros((B, 1, N * L), np.float64)
    for n in range(N * L):
        for j in range(taps + 1):
            q = n + j - taps // 2
            if q % N == 0 and 0 <= q // N < L:
                y[:, 0, n] += N * (x[:, :, q // N] * g[:, j]).sum(axis=1)
    return y
