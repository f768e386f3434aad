"""Alignment helpers of ``TTS/tts/utils/helpers.py`` on MI355X: ``maximum_path`` (Monotonic Alignment
Search) runs in ``libtts_mi355x.so`` on the device the value matrix lives on, where the reference
copies the matrix to the host and runs a Cython loop."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _native as N


def mas_logp(o_mean: torch.Tensor, o_log_scale: Optional[torch.Tensor], z: torch.Tensor) -> torch.Tensor:
    """The [B, T_en, T_de] log-likelihood of every (token, frame) pair (glow_tts.py:218-228) from the
    encoder's ``o_mean``, ``o_log_scale`` [B, C, T_en] (``None``: zeros, ``mean_only``) and the decoder's
    ``z`` [B, C, T_de]."""
    N.require_device_tensor(o_mean, "o_mean")
    dev = o_mean.device
    o_mean = o_mean.to(torch.float32).contiguous()
    z = z.to(device=dev, dtype=torch.float32).contiguous()
    if o_log_scale is not None:
        o_log_scale = o_log_scale.to(device=dev, dtype=torch.float32).contiguous()
    B, C, T_en = o_mean.shape
    T_de = z.shape[2]
    logp = torch.empty(B, T_en, T_de, device=dev)
    N.call("tts_glow_mas_logp", N.ptr(o_mean), N.ptr(o_log_scale), N.ptr(z), B, C, T_en, T_de, N.ptr(logp),
           N.stream_ptr(dev))
    return logp


def maximum_path_lengths(value: torch.Tensor, t_x: torch.Tensor, t_y: torch.Tensor, mask: Optional[torch.Tensor] = None,
                         want_path: bool = True) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Monotonic Alignment Search over ``value`` [B, T_en, T_de] with the valid sizes given as lengths
    ``t_x``, ``t_y`` [B] (equal to the reference's ``attn_mask = x_mask (x) y_mask`` without the dense
    mask).  Returns ``(path [B, T_en, T_de] or None, durations [B, T_en], log(1 + durations))``, fp32.
    Items with ``t_x < 1`` or ``t_y < t_x`` (the reference reads out of bounds) give zeros."""
    N.require_device_tensor(value, "value")
    dev = value.device
    value = value.to(torch.float32).contiguous()
    B, T_en, T_de = value.shape
    if mask is not None:
        mask = mask.to(device=dev, dtype=torch.float32).contiguous()
        if mask.shape != value.shape:
            raise ValueError(f"mask must be {tuple(value.shape)}, got {tuple(mask.shape)}")
    t_x = t_x.to(device=dev, dtype=torch.int64).reshape(B).contiguous()
    t_y = t_y.to(device=dev, dtype=torch.int64).reshape(B).contiguous()
    nbytes = N.lib().tts_maximum_path_workspace_bytes(B, T_en, T_de)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)  # oversize shapes: the call reports them
    path = torch.empty(B, T_en, T_de, device=dev) if want_path else None
    dur = torch.empty(B, T_en, device=dev)
    log_dur = torch.empty(B, T_en, device=dev)
    N.call("tts_maximum_path", N.ptr(value), N.ptr(mask), N.ptr(t_x), N.ptr(t_y), B, T_en, T_de, N.ptr(ws),
           N.ptr(path), N.ptr(dur), N.ptr(log_dur), N.stream_ptr(dev))
    return path, dur, log_dur


def maximum_path(value: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Drop-in for ``TTS.tts.utils.helpers.maximum_path(value, mask)``: ``value``, ``mask``
    [B, T_en, T_de]; ``value * mask`` is searched with ``t_x = mask.sum(1)[:, 0]``, ``t_y =
    mask.sum(2)[:, 0]``.  Returns the 0/1 path in ``value``'s dtype on its device."""
    if not isinstance(value, torch.Tensor) or value.device.type != "cuda":
        raise RuntimeError("maximum_path (tts_amd) runs only on a ROCm device: move value and mask with .to('cuda') first")
    mask = mask.to(value.device)
    t_x = mask.sum(1)[:, 0].to(torch.int64)
    t_y = mask.sum(2)[:, 0].to(torch.int64)
    path, _, _ = maximum_path_lengths(value, t_x, t_y, mask=mask)
    return path.to(value.dtype)


__all__ = ["mas_logp", "maximum_path", "maximum_path_lengths"]
