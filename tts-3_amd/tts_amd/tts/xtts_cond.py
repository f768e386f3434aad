"""XTTS voice cloning on the MI355X path: ``XttsConditioning`` holds the ``conditioning_encoder``
(``TTS/tts/layers/xtts/latent_encoder.py`` ``ConditioningEncoder``) and the ``conditioning_perceiver``
(``perceiver_encoder.py`` ``PerceiverResampler``) of the ``gpt.*`` slice of an XTTS checkpoint, with the
reference's parameter tree, and runs ``get_style_emb`` (reference mel -> the 32 x E prompt of the GPT)
and ``wav_to_mel_cloning`` through ``tts_xtts_cond_*``.  The kernel-test ops of the path
(``group_norm``, ``wide_multi_head_attention``, ``cross_attention``, ``perceiver_feed_forward``,
``rms_norm``) are functions of this module.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from .. import _native as _nat
from ..audio import hann_window, melscale_fbanks


def _f32(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        return np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32))


def _mode(math_mode: Optional[str]) -> str:
    mode = _nat.default_math_mode() if math_mode is None else math_mode
    if mode not in _nat.MATH_MODES:
        raise ValueError(f"math_mode={mode!r}: must be one of {sorted(_nat.MATH_MODES)}")
    return mode


def _dev32(t: torch.Tensor, what: str) -> torch.Tensor:
    _nat.require_device_tensor(t, what)
    return t.to(torch.float32).contiguous()


def normalization_groups(channels: int) -> int:
    """The group count of the reference's ``normalization(channels)`` (``latent_encoder.py``)."""
    groups = 32
    if channels <= 16:
        groups = 8
    elif channels <= 64:
        groups = 16
    while channels % groups != 0:
        groups = int(groups / 2)
    return groups


# ---------------------------------------------------------------------------------------- kernel-test ops
def group_norm(x: torch.Tensor, num_groups: int, weight: torch.Tensor, bias: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    """``F.group_norm`` over planes ``x`` [B, C, T] (``tts_op_groupnorm``)."""
    x = _dev32(x, "x")
    if x.dim() != 3:
        raise ValueError(f"expected x [B, C, T], got shape {tuple(x.shape)}")
    B, C, T = x.shape
    w, b = _dev32(weight.to(x.device), "weight"), _dev32(bias.to(x.device), "bias")
    if w.shape != (C,) or b.shape != (C,):
        raise ValueError(f"weight and bias must be [{C}]")
    y = torch.empty_like(x)
    _nat.call("tts_op_groupnorm", _nat.ptr(x), B, C, T, int(num_groups), _nat.ptr(w), _nat.ptr(b), float(eps),
              _nat.ptr(y), _nat.stream_ptr(x.device))
    return y


def wide_multi_head_attention(qkv: torch.Tensor, num_heads: int, key_lengths: Optional[torch.Tensor] = None,
                              math_mode: Optional[str] = None) -> torch.Tensor:
    """``multi_head_attention`` at up to 2048 channels with head sizes 32, 64, 128 (``tts_op_mha_wide``):
    ``qkv`` [B, 3E, T] (rows q | k | v) -> [B, E, T]."""
    qkv = _dev32(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[1] % 3 != 0:
        raise ValueError(f"expected qkv [B, 3E, T], got shape {tuple(qkv.shape)}")
    mode = _mode(math_mode)
    dev = qkv.device
    B, E3, T = qkv.shape
    kl = None
    if key_lengths is not None:
        kl = torch.as_tensor(key_lengths).to(device=dev, dtype=torch.int64).contiguous()
        if kl.shape != (B,):
            raise ValueError(f"expected key_lengths [{B}], got shape {tuple(kl.shape)}")
    out = torch.empty(B, E3 // 3, T, device=dev, dtype=torch.float32)
    _nat.call("tts_op_mha_wide", _nat.ptr(qkv), _nat.ptr(kl), B, E3 // 3, int(num_heads), T, _nat.MATH_MODES[mode],
              _nat.ptr(out), _nat.stream_ptr(dev))
    return out


def cross_attention(q: torch.Tensor, kv_latents: torch.Tensor, kv_context: torch.Tensor, heads: int) -> torch.Tensor:
    """The perceiver's attention (``tts_op_cross_attn``): ``q`` [B, heads d, L] against the keys of
    ``kv_latents`` [B, 2 heads d, L] and then ``kv_context`` [B, 2 heads d, T] (k rows, then v rows)
    -> [B, heads d, L]."""
    q, kl, kc = _dev32(q, "q"), _dev32(kv_latents, "kv_latents"), _dev32(kv_context, "kv_context")
    B, inner, L = q.shape
    if inner % heads != 0 or kl.shape != (B, 2 * inner, L) or kc.dim() != 3 or kc.shape[:2] != (B, 2 * inner):
        raise ValueError("expected q [B, inner, L], kv_latents [B, 2 inner, L], kv_context [B, 2 inner, T]")
    out = torch.empty_like(q)
    _nat.call("tts_op_cross_attn", _nat.ptr(q), _nat.ptr(kl), _nat.ptr(kc), B, int(heads), inner // heads, L,
              kc.shape[2], _nat.ptr(out), _nat.stream_ptr(q.device))
    return out


def perceiver_feed_forward(x: torch.Tensor, w0, b0, w2, b2, math_mode: Optional[str] = None) -> torch.Tensor:
    """``x + W2 (gelu(gate) a) + b2`` with ``[a | gate] = W0 x + b0`` over planes ``x`` [B, E, L]
    (``tts_op_cond_ff``); ``w0`` [2I, E], ``b0`` [2I], ``w2`` [E, I], ``b2`` [E] (host or device tensors)."""
    x = _dev32(x, "x")
    B, E, L = x.shape
    w0, b0, w2, b2 = _f32(w0), _f32(b0), _f32(w2), _f32(b2)
    I = w2.shape[1]
    if w0.shape != (2 * I, E) or b0.shape != (2 * I,) or w2.shape != (E, I) or b2.shape != (E,):
        raise ValueError("expected w0 [2I, E], b0 [2I], w2 [E, I], b2 [E]")
    out = torch.empty_like(x)
    _nat.call("tts_op_cond_ff", _nat.ptr(x), B, E, I, L, _nat.ptr(w0), _nat.ptr(b0), _nat.ptr(w2), _nat.ptr(b2),
              _nat.MATH_MODES[_mode(math_mode)], _nat.ptr(out), _nat.stream_ptr(x.device))
    return out


def rms_norm(x: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    """``F.normalize(x, dim=channels) * sqrt(E) * gamma`` over planes ``x`` [B, E, L] (``tts_op_rmsnorm``)."""
    x = _dev32(x, "x")
    B, E, L = x.shape
    g = _dev32(gamma.to(x.device), "gamma")
    if g.shape != (E,):
        raise ValueError(f"gamma must be [{E}]")
    y = torch.empty_like(x)
    _nat.call("tts_op_rmsnorm", _nat.ptr(x), B, E, L, _nat.ptr(g), _nat.ptr(y), _nat.stream_ptr(x.device))
    return y


# ------------------------------------------------------------------------------------------- module tree
class _AttentionBlock(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.norm = nn.GroupNorm(normalization_groups(channels), channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.proj_out = nn.Conv1d(channels, channels, 1)


class ConditioningEncoder(nn.Module):
    def __init__(self, spec_dim: int, embedding_dim: int, attn_blocks: int = 6, num_attn_heads: int = 4):
        super().__init__()
        self.init = nn.Conv1d(spec_dim, embedding_dim, kernel_size=1)
        self.attn = nn.Sequential(*[_AttentionBlock(embedding_dim) for _ in range(attn_blocks)])
        self.dim = embedding_dim
        self.num_attn_heads = num_attn_heads


class _PerceiverAttention(nn.Module):
    def __init__(self, dim: int, dim_head: int, heads: int):
        super().__init__()
        inner = dim_head * heads
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, inner * 2, bias=False)
        self.to_out = nn.Linear(inner, dim, bias=False)


class _GEGLU(nn.Module):
    pass


class _RMSNorm(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))


def ff_inner_dim(dim: int, ff_mult: int) -> int:
    return int(dim * ff_mult * 2 / 3)


class PerceiverResampler(nn.Module):
    def __init__(self, dim: int, depth: int = 2, num_latents: int = 32, dim_head: int = 64, heads: int = 8,
                 ff_mult: int = 4):
        super().__init__()
        self.latents = nn.Parameter(torch.randn(num_latents, dim) * 0.02)
        inner = ff_inner_dim(dim, ff_mult)
        self.layers = nn.ModuleList([
            nn.ModuleList([
                _PerceiverAttention(dim, dim_head, heads),
                nn.Sequential(nn.Linear(dim, inner * 2), _GEGLU(), nn.Linear(inner, dim)),
            ]) for _ in range(depth)
        ])
        self.norm = _RMSNorm(dim)


class XttsConditioning(nn.Module):
    """The conditioning encoder and the perceiver resampler of XTTS v2's GPT.  ``get_style_emb(cond_input)``
    is gpt.py's: mel [B, 80, T] (or [B, 1, 80, T]) -> [B, model_dim, num_latents]."""

    def __init__(self, model_dim: int = 1024, heads: int = 16, attn_blocks: int = 6, perceiver_depth: int = 2,
                 num_latents: int = 32, perceiver_dim_head: int = 64, perceiver_heads: int = 8, ff_mult: int = 4,
                 spec_dim: int = 80, math_mode: Optional[str] = None, *, n_fft: int = 2048, hop_length: int = 256,
                 win_length: int = 1024, sample_rate: int = 22050, f_min: float = 0, f_max: float = 8000):
        """The keyword-only arguments are ``wav_to_mel_cloning``'s (the mel front end's plan)."""
        super().__init__()
        self.n_fft, self.hop_length, self.win_length = int(n_fft), int(hop_length), int(win_length)
        self.sample_rate, self.f_min, self.f_max = int(sample_rate), f_min, f_max
        self.math_mode = _mode(math_mode)
        self.model_dim, self.heads, self.attn_blocks = int(model_dim), int(heads), int(attn_blocks)
        self.perceiver_depth, self.num_latents = int(perceiver_depth), int(num_latents)
        self.perceiver_dim_head, self.perceiver_heads = int(perceiver_dim_head), int(perceiver_heads)
        self.ff_mult, self.spec_dim = int(ff_mult), int(spec_dim)
        c = self._make_cfg()
        n = _nat.lib().tts_xtts_cond_num_weights(ctypes.byref(c))  # validates before any module is built
        if n < 0:
            _nat.check("tts_xtts_cond_num_weights", -n)
        self.conditioning_encoder = ConditioningEncoder(self.spec_dim, self.model_dim, attn_blocks=self.attn_blocks,
                                                        num_attn_heads=self.heads)
        self.conditioning_perceiver = PerceiverResampler(self.model_dim, depth=self.perceiver_depth,
                                                         num_latents=self.num_latents,
                                                         dim_head=self.perceiver_dim_head,
                                                         heads=self.perceiver_heads, ff_mult=self.ff_mult)
        self._handle = None
        self._handle_key = None

    # ------------------------------------------------------------------ native handle
    def _make_cfg(self) -> "_nat.TtsXttsCondCfg":
        c = _nat.TtsXttsCondCfg()
        c.spec_dim, c.model_dim, c.heads = self.spec_dim, self.model_dim, self.heads
        c.attn_blocks, c.perceiver_depth, c.num_latents = self.attn_blocks, self.perceiver_depth, self.num_latents
        c.perceiver_dim_head, c.perceiver_heads, c.ff_mult = self.perceiver_dim_head, self.perceiver_heads, self.ff_mult
        c.n_fft, c.hop_length, c.win_length = self.n_fft, self.hop_length, self.win_length
        c.math_mode = _nat.MATH_MODES[self.math_mode]
        return c

    def _weight_list(self) -> List[np.ndarray]:
        e, p = self.conditioning_encoder, self.conditioning_perceiver
        ws = [_f32(e.init.weight), _f32(e.init.bias)]
        for b in e.attn:
            ws.extend(_f32(t) for t in (b.norm.weight, b.norm.bias, b.qkv.weight, b.qkv.bias, b.proj_out.weight,
                                        b.proj_out.bias))
        ws.append(_f32(p.latents))
        for attn, ff in p.layers:
            ws.extend(_f32(t) for t in (attn.to_q.weight, attn.to_kv.weight, attn.to_out.weight, ff[0].weight,
                                        ff[0].bias, ff[2].weight, ff[2].bias))
        ws.append(_f32(p.norm.gamma))
        # the front end's constants, in fp64 on the host
        ws.append(_f32(hann_window(self.win_length)))
        ws.append(_f32(melscale_fbanks(self.n_fft // 2 + 1, self.f_min, self.f_max, self.spec_dim, self.sample_rate)))
        return ws

    def _device(self) -> torch.device:
        dev = self.conditioning_perceiver.latents.device
        if dev.type != "cuda":
            raise RuntimeError("XttsConditioning (tts_amd) runs only on a ROCm device: move it with .to('cuda') "
                               "first (there is no CPU fallback)")
        return dev

    def _native_handle(self):
        key = tuple((p.data_ptr(), p._version, p.device) for p in self.parameters())
        if self._handle is not None and key == self._handle_key:
            return self._handle
        self._release()
        dev = self._device()
        cfg = self._make_cfg()
        ws = self._weight_list()
        lib = _nat.lib()
        n = lib.tts_xtts_cond_num_weights(ctypes.byref(cfg))
        if n < 0:
            _nat.check("tts_xtts_cond_num_weights", -n)
        if n != len(ws):
            raise ValueError(f"{len(ws)} weights, the library expects {n}")
        for i, w in enumerate(ws):
            n = lib.tts_xtts_cond_weight_numel(ctypes.byref(cfg), i)
            if n != w.size:
                raise ValueError(f"weight {i} has {w.size} elements, expected {n}")
        arr = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        h = ctypes.c_void_p()
        _nat.call("tts_xtts_cond_create", ctypes.byref(cfg), arr, dev.index or 0, ctypes.byref(h))
        self._handle, self._handle_key = h, key
        return h

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            _nat.lib().tts_xtts_cond_destroy(self._handle)
            self._handle = None
            self._handle_key = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _apply(self, fn, *args, **kwargs):
        self._release()
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def wav_to_mel_cloning(self, wav: torch.Tensor, mel_norms: torch.Tensor) -> torch.Tensor:
        """wav [B, N] at 22 050 Hz -> log-mel [B, spec_dim, 1 + N // hop], divided by ``mel_norms`` [spec_dim]."""
        dev = self._device()
        _nat.require_device_tensor(wav, "wav")
        x = wav.to(device=dev, dtype=torch.float32)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise ValueError(f"wav must be [B, N], got shape {tuple(wav.shape)}")
        x = x.contiguous()
        norms = torch.as_tensor(mel_norms).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if norms.shape != (self.spec_dim,):
            raise ValueError(f"mel_norms must be [{self.spec_dim}], got {tuple(norms.shape)}")
        h = self._native_handle()
        B, N = x.shape
        T = _nat.lib().tts_xtts_cond_num_frames(h, N)
        if T < 0:
            _nat.check("tts_xtts_cond_num_frames", int(-T))
        mel = torch.empty(B, self.spec_dim, T, device=dev, dtype=torch.float32)
        _nat.call("tts_xtts_cond_mel", h, _nat.ptr(x), B, N, _nat.ptr(norms), _nat.ptr(mel), _nat.stream_ptr(dev))
        return mel

    @torch.no_grad()
    def get_style_emb(self, cond_input: torch.Tensor, return_latent: bool = False, profile: bool = False):
        """gpt.py ``get_style_emb``: ``perceiver(encoder(mel).permute(0, 2, 1)).transpose(1, 2)``,
        [B, model_dim, num_latents].  ``profile=True`` also returns the launch records."""
        dev = self._device()
        _nat.require_device_tensor(cond_input, "cond_input")
        x = cond_input.to(device=dev, dtype=torch.float32)
        if x.dim() == 4:
            x = x.squeeze(1)
        if x.dim() != 3 or x.shape[1] != self.spec_dim:
            raise ValueError(f"cond_input must be [B, {self.spec_dim}, T], got shape {tuple(cond_input.shape)}")
        x = x.contiguous()
        B, _, T = x.shape
        h = self._native_handle()
        out = torch.empty(B, self.model_dim, self.num_latents, device=dev, dtype=torch.float32)
        args = (h, _nat.ptr(x), B, T, _nat.ptr(out), _nat.stream_ptr(dev))
        if profile:
            from .xtts_gpt import _profiled

            return out, _profiled("tts_xtts_cond_style_emb_profiled", args)
        _nat.call("tts_xtts_cond_style_emb", *args)
        return out

    forward = get_style_emb

    def load_checkpoint(self, checkpoint_path, eval=True, strict=True):
        """Loads the ``gpt.conditioning_encoder.*`` / ``gpt.conditioning_perceiver.*`` slice of an XTTS
        checkpoint (or a bare state dict of the two modules)."""
        state = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        state = state["model"] if "model" in state else state
        self.load_state_dict(conditioning_checkpoint_filter(state), strict=strict)
        if eval:
            self.eval()


_PREFIXES = ("conditioning_encoder.", "conditioning_perceiver.")


def conditioning_checkpoint_filter(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The ``conditioning_encoder.*`` / ``conditioning_perceiver.*`` keys of a full XTTS checkpoint
    (``gpt.`` in front), of its ``gpt.*`` slice, or of a bare state dict."""
    out = {}
    for k, v in state.items():
        kk = k[len("gpt."):] if k.startswith("gpt.conditioning_") else k
        if kk.startswith(_PREFIXES):
            out[kk] = v
    return out


__all__ = ["ConditioningEncoder", "PerceiverResampler", "XttsConditioning", "conditioning_checkpoint_filter",
           "cross_attention", "ff_inner_dim", "group_norm", "normalization_groups", "perceiver_feed_forward",
           "rms_norm", "wide_multi_head_attention"]
