"""``wav_to_spec`` of ``TTS/tts/models/vits.py`` (Coqui TTS 0.22.0) on MI355X: the linear spectrogram
the VITS posterior encoder consumes, one C-ABI call (``tts_stft_forward``: a GEMM of the windowed DFT
matrix with the wav's frames on the matrix cores, magnitude fused; no FFT library involved)."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import _native as N


class _StftPlan:
    """One ``tts_stft_create`` handle (the packed DFT matrix lives on its device)."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, mode: str, device_index: int):
        c = N.TtsStftCfg()
        c.n_fft, c.hop_length, c.win_length = n_fft, hop_length, win_length
        c.math_mode = N.MATH_MODES[mode]
        self.cfg = c
        # torch.hann_window(win_length): periodic, created in fp32 as the reference does
        win = np.ascontiguousarray(torch.hann_window(win_length, dtype=torch.float32).numpy())
        self.handle = ctypes.c_void_p()
        N.call("tts_stft_create", ctypes.byref(c), N.ptr(win), device_index, ctypes.byref(self.handle))

    def num_frames(self, n: int) -> int:
        return N.lib().tts_stft_num_frames(ctypes.byref(self.cfg), n)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                N.lib().tts_stft_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


_PLANS: Dict[Tuple[int, int, int, str, int], _StftPlan] = {}


def _mode(math_mode: Optional[str]) -> str:
    if math_mode is None:
        math_mode = N.default_math_mode()
    if math_mode not in N.MATH_MODES:
        raise ValueError(f"math_mode must be one of {sorted(N.MATH_MODES)}")
    return "fp32x6" if math_mode == "fp32" else math_mode


def _plan(n_fft: int, hop_length: int, win_length: int, mode: str, dev: torch.device) -> _StftPlan:
    key = (int(n_fft), int(hop_length), int(win_length), mode, dev.index or 0)
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = _StftPlan(*key)
    return p


def _rows(y: torch.Tensor):
    if not isinstance(y, torch.Tensor) or y.device.type != "cuda":
        raise RuntimeError("wav_to_spec (tts_amd) runs only on a ROCm device: move the wav with .to('cuda')")
    if y.dim() == 3 and y.shape[1] == 1:
        y = y[:, 0, :]
    if y.dim() != 2:
        raise ValueError(f"wav has shape {tuple(y.shape)}, expected [B, 1, N] or [B, N]")
    return y.to(torch.float32).contiguous()


def wav_to_spec(y: torch.Tensor, n_fft: int, hop_length: int, win_length: int, center: bool = False,
                math_mode: Optional[str] = None) -> torch.Tensor:
    """Linear spectrogram ``sqrt(|STFT(y)|^2 + 1e-6)`` as VITS computes it: ``y`` [B, 1, N] or [B, N] on a
    ROCm device -> [B, n_fft // 2 + 1, T] fp32.  The wav is reflect-padded by ``(n_fft - hop_length) // 2``
    samples on both sides (so N must exceed that: ``ValueError`` otherwise, as torch's reflect pad
    raises), framed every ``hop_length`` samples (T = 1 + (N + 2 pad - n_fft) // hop_length; trailing
    samples that do not fill a frame are dropped) and windowed with ``torch.hann_window(win_length)``.

    Supported: n_fft a multiple of 32 in [64, 2048], hop_length a multiple of 8 in [8, n_fft],
    1 <= win_length <= n_fft.  ``math_mode``: ``"f16x3"`` (default), ``"fp32x6"`` or ``"bf16"``; the op has no
    exact-fp32 MFMA kernel, so ``"fp32"`` runs as ``"fp32x6"`` (fp32 operands split exactly into bf16 pieces).
    ``center=True`` raises ``NotImplementedError`` (VITS never passes it).  The reference's printed warnings
    for samples outside [-1, 1] are not reproduced.  Plans (the packed DFT matrix) are cached per
    (n_fft, hop_length, win_length, mode, device)."""
    if center:
        raise NotImplementedError("wav_to_spec: center=True is not implemented (VITS calls it with center=False)")
    y = _rows(y)
    B, n = y.shape
    plan = _plan(n_fft, hop_length, win_length, _mode(math_mode), y.device)
    pad = (int(n_fft) - int(hop_length)) // 2
    if n <= pad:
        raise ValueError(f"wav_to_spec: reflect padding of {pad} samples needs a wav longer than that, got {n}")
    T = plan.num_frames(n)
    if T < 0:
        msg = N.lib().tts_last_error().decode(errors="replace")
        if -T == N.TTS_ERR_INVALID:
            raise ValueError(msg)
        raise N.NativeError("tts_stft_num_frames", -T, msg)
    spec = torch.empty(B, n_fft // 2 + 1, T, device=y.device, dtype=torch.float32)
    N.call("tts_stft_forward", plan.handle, N.ptr(y), B, n, n, N.ptr(spec), N.stream_ptr(y.device))
    return spec


def wav_to_spec_profile(y: torch.Tensor, n_fft: int, hop_length: int, win_length: int,
                        math_mode: Optional[str] = None):
    """One pass with a hipEvent pair around every launch: (spec, [{name, flops, bytes, ms}])."""
    y = _rows(y)
    B, n = y.shape
    plan = _plan(n_fft, hop_length, win_length, _mode(math_mode), y.device)
    T = plan.num_frames(n)
    if T < 0:
        N.check("tts_stft_num_frames", -T)
    spec = torch.empty(B, n_fft // 2 + 1, T, device=y.device, dtype=torch.float32)
    cap = 8
    recs = (N.TtsLaunchRecord * cap)()
    cnt = ctypes.c_int(0)
    N.call("tts_stft_forward_profiled", plan.handle, N.ptr(y), B, n, n, N.ptr(spec), N.stream_ptr(y.device), recs, cap,
           ctypes.byref(cnt))
    rows = [{"name": recs[i].name.decode(), "flops": recs[i].flops, "bytes": recs[i].bytes, "ms": recs[i].ms}
            for i in range(min(cnt.value, cap))]
    return spec, rows
