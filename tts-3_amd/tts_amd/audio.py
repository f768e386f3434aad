"""Audio ops of the voice-cloning path on the device: ``resample`` (``torchaudio.functional.resample`` at
its defaults: ``sinc_interp_hann``, ``lowpass_filter_width`` 6, ``rolloff`` 0.99, through ``tts_resample_*``)
and the pieces of ``wav_to_mel_cloning`` (``TTS/tts/models/xtts.py``) that are built on the host:
torchaudio's ``melscale_fbanks`` and the periodic Hann window.  The mel itself is computed by an
``XttsConditioning`` handle (``tts_xtts_cond_mel``); ``wav_to_mel_cloning`` here is the reference's
function, with its signature, on a cached handle of the smallest width."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Tuple

import numpy as np
import torch

from . import _native as _nat


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int,
                    norm: str = "slaney", mel_scale: str = "htk") -> np.ndarray:
    """torchaudio.functional.melscale_fbanks in fp64: fb [n_freqs, n_mels] (triangular filters)."""
    if mel_scale != "htk":
        raise NotImplementedError("only mel_scale='htk' is implemented")
    if norm not in (None, "slaney"):
        raise ValueError("norm must be None or 'slaney'")
    all_freqs = np.linspace(0.0, sample_rate // 2, n_freqs, dtype=np.float64)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = np.linspace(m_min, m_max, n_mels + 2, dtype=np.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]
    return fb


def hann_window(win_length: int) -> np.ndarray:
    """torch.hann_window(win_length) (periodic) in fp64."""
    n = np.arange(win_length, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)


def resample_kernel(orig_freq: int, new_freq: int) -> Tuple[np.ndarray, int]:
    """torchaudio's ``_get_sinc_resample_kernel`` (fp64): ``(kern [n, 2 w + o], w)`` with ``o`` and ``n`` the
    frequencies over their gcd."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * 0.99
    w = int(math.ceil(6 * o / base))
    k = np.arange(-w, w + o, dtype=np.float64)[None, :] / o
    t = (-np.arange(n, dtype=np.float64)[:, None] / n + k) * base
    t = np.clip(t, -6.0, 6.0)
    window = np.cos(t * np.pi / 12.0) ** 2
    a = t * np.pi
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return sinc * window * (base / o), w


class _Resampler:
    def __init__(self, orig_freq: int, new_freq: int, device: torch.device):
        self.handle = ctypes.c_void_p()
        _nat.call("tts_resample_create", int(orig_freq), int(new_freq), device.index or 0, ctypes.byref(self.handle))

    def __del__(self):
        try:
            if self.handle:
                _nat.lib().tts_resample_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


_RESAMPLERS: Dict[Tuple[int, int, int], _Resampler] = {}  # one table per (ratio, device), kept until the interpreter exits


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """``torchaudio.functional.resample(waveform, orig_freq, new_freq)``: ``[..., N]`` on the device ->
    ``[..., ceil(new N / orig)]``.  Equal frequencies return the input."""
    _nat.require_device_tensor(waveform, "waveform")
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("orig_freq and new_freq must be positive")
    if orig_freq == new_freq:
        return waveform
    dev = waveform.device
    key = (orig_freq, new_freq, dev.index or 0)
    r = _RESAMPLERS.get(key)
    if r is None:
        r = _RESAMPLERS[key] = _Resampler(orig_freq, new_freq, dev)
    shape = waveform.shape
    x = waveform.to(torch.float32).reshape(-1, shape[-1]).contiguous()
    B, N = x.shape
    n_out = _nat.lib().tts_resample_num_samples(r.handle, N)
    if n_out < 0:
        _nat.check("tts_resample_num_samples", int(-n_out))
    y = torch.empty(B, n_out, device=dev, dtype=torch.float32)
    _nat.call("tts_resample_forward", r.handle, _nat.ptr(x), B, N, _nat.ptr(y), _nat.stream_ptr(dev))
    return y.reshape(shape[:-1] + (n_out,))


_MEL_PLANS: Dict[tuple, object] = {}  # like _RESAMPLERS: kept until the interpreter exits


def _mel_plan(device: torch.device, n_fft, hop_length, win_length, sample_rate, f_min, f_max, n_mels):
    """An ``XttsConditioning`` of the smallest width, kept only for its mel plan (window and filterbank in
    its arena), one per parameter set and device."""
    from .tts.xtts_cond import XttsConditioning

    key = (int(n_fft), int(hop_length), int(win_length), int(sample_rate), float(f_min), float(f_max), int(n_mels),
           device.index or 0)
    plan = _MEL_PLANS.get(key)
    if plan is None:
        # the library has no mel-only handle: the plan rides on the narrowest module it accepts, whose own
        # weights (a few KB) are never run
        plan = XttsConditioning(model_dim=32, heads=1, attn_blocks=0, perceiver_depth=1, num_latents=1,
                                perceiver_dim_head=1, perceiver_heads=1, ff_mult=1, spec_dim=int(n_mels), math_mode="fp32",
                                n_fft=n_fft, hop_length=hop_length, win_length=win_length, sample_rate=sample_rate,
                                f_min=f_min, f_max=f_max)
        _MEL_PLANS[key] = plan = plan.eval().to(device)
    return plan


def wav_to_mel_cloning(wav: torch.Tensor, mel_norms_file=None, mel_norms=None, device=None, n_fft=2048, hop_length=256,
                       win_length=1024, power=2, normalized=False, sample_rate=22050, f_min=0, f_max=8000,
                       n_mels=80) -> torch.Tensor:
    """``wav_to_mel_cloning`` of ``TTS/tts/models/xtts.py`` with its signature: wav [B, N] on the device ->
    log-mel [B, n_mels, 1 + N // hop_length] divided by ``mel_norms`` [n_mels].  The plan (window and
    filterbank on the device) is built once per parameter set.  ``mel_norms_file`` (a file read on the host)
    is not loaded here: pass ``mel_norms``; ``device`` is accepted and ignored (the wav's device is used)."""
    if mel_norms is None:
        raise NotImplementedError("loading mel_norms_file is not implemented on the device (DESIGN.md section 8): "
                                  "pass mel_norms")
    if power != 2 or normalized:
        raise NotImplementedError("only power=2, normalized=False (the reference's values) are implemented")
    _nat.require_device_tensor(wav, "wav")
    plan = _mel_plan(wav.device, n_fft, hop_length, win_length, sample_rate, f_min, f_max, n_mels)
    return plan.wav_to_mel_cloning(wav, mel_norms)


__all__ = ["hann_window", "melscale_fbanks", "resample", "resample_kernel", "wav_to_mel_cloning"]
