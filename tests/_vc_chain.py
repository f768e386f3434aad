"""The CPU oracle of VITS voice conversion (``Vits.voice_conversion`` / ``inference_voice_conversion``,
TTS/tts/models/vits.py): the linear spectrogram by ``torch.stft`` as ``wav_to_spec`` calls it, then
posterior encoder -> flow forward (source speaker) -> flow reverse (target speaker) -> HiFiGAN decoder.
Test infrastructure: it calls only torch on the CPU, oracle/ and tts_amd.synthetic (numpy weights)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import hifigan_ref, vits_ref
from tts_amd import synthetic
from tts_amd.config import VITS_DECODER, VITS_FLOW, VITS_POSTERIOR


def spec_ref(y: torch.Tensor, n_fft: int, hop: int, win: int, dtype=torch.float64) -> torch.Tensor:
    """wav_to_spec (vits.py) on the CPU in ``dtype``: y [B, N] -> [B, n_fft // 2 + 1, T].  The hann window
    is created in fp32, as the reference does, and cast."""
    p = int((n_fft - hop) / 2)
    yp = F.pad(y.to(dtype).unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    window = torch.hann_window(win, dtype=torch.float32).to(dtype)
    s = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=window, center=False, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    s = torch.view_as_real(s)
    return torch.sqrt(s.pow(2).sum(-1) + 1e-6)


def signal(kind: str, B: int, N: int, seed: int = 0) -> torch.Tensor:
    """fp32 test wavs [B, N]: 'noise' (0.3 * standard normal) or 'sines' (0.9 sin 440 Hz + 0.05 sin 5000.3 Hz
    at 22050 Hz: a large dynamic range and bins that are numerically zero)."""
    if kind == "noise":
        return 0.3 * torch.randn(B, N, generator=torch.Generator().manual_seed(seed))
    t = torch.arange(N, dtype=torch.float64) / 22050.0
    y = 0.9 * torch.sin(2 * torch.pi * 440.0 * t) + 0.05 * torch.sin(2 * torch.pi * 5000.3 * t)
    return y.float().unsqueeze(0).repeat(B, 1)


# the small model of the voice-conversion tests: 4 posterior layers, a 128-channel decoder
POST_CFG = dict(VITS_POSTERIOR, num_layers=4)
DEC_CFG = dict(VITS_DECODER, upsample_initial_channel=128)


def vits_args(gin: int, by_id: bool) -> dict:
    a = dict(num_chars=16, num_layers_text_encoder=1, num_layers_posterior_encoder=POST_CFG["num_layers"],
             upsample_initial_channel_decoder=DEC_CFG["upsample_initial_channel"])
    if by_id:
        a.update(use_speaker_embedding=True, num_speakers=5, speaker_embedding_channels=gin)
    else:
        a.update(use_d_vector_file=True, d_vector_dim=gin)
    return a


def state_dicts(gin: int, seed: int = 11):
    psd = synthetic.vits_posterior_state_dict(**dict(POST_CFG, cond_channels=gin), seed=seed)
    fsd = synthetic.vits_flow_state_dict(**dict(VITS_FLOW, cond_channels=gin), seed=seed + 1)
    dsd = synthetic.hifigan_state_dict(**dict(DEC_CFG, cond_channels=gin), seed=seed + 2, weight_norm=True)
    return psd, fsd, dsd


def oracle_vc(sds, y, lengths, eps, g_src, g_tgt, dtype=torch.float64):
    """(z, z_p, z_hat, wav, y_mask) of the chain in ``dtype``; y [B, 513, T], lengths [B], eps [B, 192, T],
    g_* [B, gin, 1]."""
    psd, fsd, dsd = sds
    gin = g_src.shape[1]
    B, _, T = y.shape
    mask = (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]).to(dtype).unsqueeze(1)
    z, _, _ = vits_ref.vits_posterior(psd, y, mask, eps, g_src, dtype=dtype, **dict(POST_CFG, cond_channels=gin))
    fcfg = dict(VITS_FLOW, cond_channels=gin)
    z_p = vits_ref.vits_flow_forward(fsd, z, mask, g_src, dtype=dtype, **fcfg)
    z_hat = vits_ref.vits_flow_reverse(fsd, z_p, mask, g_tgt, dtype=dtype, **fcfg)
    wav = hifigan_ref.hifigan_forward(dsd, z_hat * mask, pad=0, g=g_tgt.to(dtype), dtype=dtype, fold_dtype=dtype,
                                      **dict(DEC_CFG, cond_channels=gin))
    return z, z_p, z_hat, wav, mask
