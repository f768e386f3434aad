"""Drop-in ``MelganGenerator`` whose compute runs in ``libtts_mi355x.so`` on MI355X.

Mirrors ``TTS/vocoder/models/melgan_generator.py`` and ``TTS/vocoder/layers/melgan.py`` (Coqui TTS
0.22.0): the same constructor arguments and the same parameter tree (one ``nn.Sequential`` named
``layers`` whose residual stacks hold ``blocks`` and ``shortcuts``), so reference checkpoints load
strictly, weight-norm parametrized or folded.  ``forward``, ``inference`` (replicate pad of
``inference_padding`` = 2 frames), ``remove_weight_norm`` and ``load_checkpoint`` behave like the
reference.  The ``torch.nn`` modules only hold parameters; their ``forward`` is never called.

Math modes (``math_mode`` keyword, as on ``HifiganGenerator``): the residual-block kernel exists
in ``"fp32x6"`` (three exact bf16 pieces per operand, six products: fp32-faithful) and ``"bf16"``.
``"fp32"`` and the package default ``"f16x3"`` run the fp32x6 kernels (a true f16x3 block kernel
would need the producer max-abs chain through the whole-block kernel); both are held to the fp32
parity gates.  The last conv, tanh and the PQMF synthesis are plain fp32 FMA in every mode.

There is no CPU path: a module whose parameters are on the CPU raises instead of computing elsewhere.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn
from torch.nn.utils.parametrizations import weight_norm
from torch.nn.utils.parametrize import is_parametrized, remove_parametrizations

from .. import _native as N
from .hifigan_generator import _effective_weight, _host


class ResidualStack(nn.Module):
    """Parameter container of ``ResidualStack`` (layers/melgan.py): ``x = shortcut(x) + block(x)`` per
    block, the shortcut on the raw ``x``; dilation ``kernel_size ** idx``."""

    def __init__(self, channels: int, num_res_blocks: int, kernel_size: int):
        super().__init__()
        assert (kernel_size - 1) % 2 == 0, " [!] kernel_size must be odd number."
        base_padding = (kernel_size - 1) // 2
        self.blocks = nn.ModuleList()
        for idx in range(num_res_blocks):
            layer_kernel_size = kernel_size
            layer_dilation = layer_kernel_size**idx
            layer_padding = base_padding * layer_dilation
            self.blocks += [
                nn.Sequential(
                    nn.LeakyReLU(0.2),
                    nn.ReflectionPad1d(layer_padding),
                    weight_norm(nn.Conv1d(channels, channels, kernel_size=kernel_size, dilation=layer_dilation, bias=True)),
                    nn.LeakyReLU(0.2),
                    weight_norm(nn.Conv1d(channels, channels, kernel_size=1, bias=True)),
                )
            ]
        self.shortcuts = nn.ModuleList(
            [weight_norm(nn.Conv1d(channels, channels, kernel_size=1, bias=True)) for _ in range(num_res_blocks)]
        )

    def convs(self) -> List[nn.Module]:
        """C-ABI (= state dict) order: every block's two convs, then the shortcuts."""
        out: List[nn.Module] = []
        for b in self.blocks:
            out += [b[2], b[4]]
        return out + list(self.shortcuts)

    def remove_weight_norm(self):
        for l in self.convs():
            if is_parametrized(l, "weight"):
                remove_parametrizations(l, "weight")


class MelganGenerator(nn.Module):
    def __init__(
        self,
        in_channels: int = 80,
        out_channels: int = 1,
        proj_kernel: int = 7,
        base_channels: int = 512,
        upsample_factors: Sequence[int] = (8, 8, 2, 2),
        res_kernel: int = 3,
        num_res_blocks: int = 3,
        math_mode: Optional[str] = None,
    ):
        super().__init__()
        # assert model parameters
        assert (proj_kernel - 1) % 2 == 0, " [!] proj_kernel should be an odd number."
        if math_mode is None:
            math_mode = N.default_math_mode()
        if math_mode not in N.MATH_MODES:
            raise ValueError(f"math_mode must be one of {sorted(N.MATH_MODES)}")
        self.math_mode = math_mode
        upsample_factors = [int(u) for u in upsample_factors]
        if len(upsample_factors) > N.MAX_UPSAMPLES:
            raise ValueError("too many upsample layers for the native configuration")
        self.upsample_factors = upsample_factors
        self.hop_length = int(np.prod(upsample_factors))
        self.proj_kernel = proj_kernel
        self.res_kernel = res_kernel
        self.num_res_blocks = num_res_blocks
        self.in_channels = in_channels
        self.out_channels = out_channels

        # initial layer
        base_padding = (proj_kernel - 1) // 2
        act_slope = 0.2
        self.inference_padding = 2
        layers: List[nn.Module] = [
            nn.ReflectionPad1d(base_padding),
            weight_norm(nn.Conv1d(in_channels, base_channels, kernel_size=proj_kernel, stride=1, bias=True)),
        ]
        # upsampling layers and residual stacks
        for idx, upsample_factor in enumerate(upsample_factors):
            layer_in_channels = base_channels // (2**idx)
            layer_out_channels = base_channels // (2 ** (idx + 1))
            layer_filter_size = upsample_factor * 2
            layer_stride = upsample_factor
            layer_output_padding = upsample_factor % 2
            layer_padding = upsample_factor // 2 + layer_output_padding
            layers += [
                nn.LeakyReLU(act_slope),
                weight_norm(
                    nn.ConvTranspose1d(
                        layer_in_channels,
                        layer_out_channels,
                        layer_filter_size,
                        stride=layer_stride,
                        padding=layer_padding,
                        output_padding=layer_output_padding,
                        bias=True,
                    )
                ),
                ResidualStack(channels=layer_out_channels, num_res_blocks=num_res_blocks, kernel_size=res_kernel),
            ]
        layers += [nn.LeakyReLU(act_slope)]
        # final layer
        layers += [
            nn.ReflectionPad1d(base_padding),
            weight_norm(nn.Conv1d(layer_out_channels, out_channels, proj_kernel, stride=1, bias=True)),
            nn.Tanh(),
        ]
        self.layers = nn.Sequential(*layers)

        self._cfg = N.TtsMelganCfg()
        c = self._cfg
        c.in_channels = in_channels
        c.out_channels = out_channels
        c.proj_kernel = proj_kernel
        c.base_channels = base_channels
        c.num_ups = len(upsample_factors)
        for i, u in enumerate(upsample_factors):
            c.upsample_factors[i] = u
        c.res_kernel = res_kernel
        c.num_res_blocks = num_res_blocks
        c.pqmf_bands = 0
        c.pqmf_taps = 0
        c.math_mode = N.MATH_MODES[math_mode]
        self._handle = None
        self._handle_key = None
        self._validate_cfg()

    def _validate_cfg(self) -> None:
        """Fail at construction for configurations the native path cannot run."""
        n = N.lib().tts_melgan_num_weights(ctypes.byref(self._cfg))
        if n < 0:
            N.check("tts_melgan_num_weights", -n)

    # ------------------------------------------------------------------ native handle
    def _conv_modules(self) -> List[nn.Module]:
        out: List[nn.Module] = []
        for m in self.layers:
            if isinstance(m, ResidualStack):
                out += m.convs()
            elif isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
                out.append(m)
        return out

    def _extra_weights(self) -> List[np.ndarray]:
        return []

    def _weight_list(self) -> List[np.ndarray]:
        """Folded fp32 weights in the C-ABI order (include/tts_mi355x.h)."""
        ws: List[np.ndarray] = []
        for cv in self._conv_modules():
            ws += [_effective_weight(cv), _host(cv.bias)]
        return ws + self._extra_weights()

    def _param_key(self):
        return tuple((p.data_ptr(), p._version, p.device) for p in list(self.parameters()) + list(self.buffers()))

    def _device(self) -> torch.device:
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__} (tts_amd) runs only on a ROCm device: move the module with "
                ".to('cuda') first (there is no CPU fallback)"
            )
        return dev

    def _native_handle(self):
        key = self._param_key()
        if self._handle is not None and key == self._handle_key:
            return self._handle
        self._release()
        dev = self._device()
        ws = self._weight_list()
        lib = N.lib()
        expected = lib.tts_melgan_num_weights(ctypes.byref(self._cfg))
        if expected < 0:
            N.check("tts_melgan_num_weights", -expected)
        if expected != len(ws):
            raise RuntimeError(f"internal: {len(ws)} weight tensors, library expects {expected}")
        for i, w in enumerate(ws):
            n = lib.tts_melgan_weight_numel(ctypes.byref(self._cfg), i)
            if n != w.size:
                raise ValueError(f"weight {i} has {w.size} elements, expected {n}")
        arr = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        h = ctypes.c_void_p()
        N.call("tts_melgan_create", ctypes.byref(self._cfg), arr, dev.index or 0, ctypes.byref(h))
        self._handle, self._handle_key = h, key
        return h

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            N.lib().tts_melgan_destroy(self._handle)
            self._handle = None
            self._handle_key = None

    def __del__(self):
        try:
            self._release()
        except Exception:  # interpreter shutdown
            pass

    def _apply(self, fn, *args, **kwargs):
        self._release()
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------ reference API
    def _length_error(self, T: int, pad: int) -> Optional[str]:
        """The reflection pad that torch would refuse for a [.., T] input (pad >= the plane it pads),
        as the library decides it on the host; None when every pad fits."""
        p = (self.proj_kernel - 1) // 2
        length = T + 2 * pad
        if T < 1:
            return "T must be positive"
        if p >= length:
            return f"reflection pad {p} of the first conv must be smaller than its input length {length}"
        for i, u in enumerate(self.upsample_factors):
            length *= u
            for j in range(self.num_res_blocks):
                d = ((self.res_kernel - 1) // 2) * self.res_kernel**j
                if d >= length:
                    return (f"reflection pad {d} of residual block {j} in stack {i} must be smaller than its "
                            f"input length {length}")
        if p >= length:
            return "reflection pad of the last conv must be smaller than its input length"
        return None

    def _run(self, x: torch.Tensor, pad: int, synth: int) -> torch.Tensor:
        if x.dim() != 3:
            raise ValueError(f"expected [B, C, T] input, got shape {tuple(x.shape)}")
        B, C, T = x.shape
        if C != self._cfg.in_channels:
            raise ValueError(f"input has {C} channels, generator expects {self._cfg.in_channels}")
        on_device = next(self.parameters()).device.type == "cuda"
        err = self._length_error(T, pad)
        if err is not None:
            if on_device:  # the library's own decision (and message: tts_last_error())
                n = N.lib().tts_melgan_output_length(self._native_handle(), T, pad, synth)
                if n >= 0:
                    raise RuntimeError(f"internal: the library accepts T={T}, pad={pad} ({err})")
                err = N.lib().tts_last_error().decode(errors="replace")
            raise ValueError(f"{type(self).__name__}: {err}")
        h = self._native_handle()
        dev = self._device()
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        n = N.lib().tts_melgan_output_length(h, T, pad, synth)
        if n < 0:
            N.check("tts_melgan_output_length", int(-n))
        out = torch.empty(B, 1 if synth else self._cfg.out_channels, n, device=dev, dtype=torch.float32)
        N.call("tts_melgan_forward", h, N.ptr(x), B, C, T, pad, synth, N.ptr(out), N.stream_ptr(dev))
        return out

    def forward(self, c: torch.Tensor) -> torch.Tensor:
        """``self.layers(c)``.  Inference only."""
        with torch.no_grad():
            return self._run(c, 0, 0)

    @torch.no_grad()
    def inference(self, c: torch.Tensor) -> torch.Tensor:
        """Move to the weight device, replicate-pad ``inference_padding`` frames, ``self.layers``."""
        return self._run(c, self.inference_padding, 0)

    def profile(self, c: torch.Tensor, pad: Optional[int] = None, synth: int = 0):
        """One forward with a hipEvent pair around every launch: (out, [{name, flops, bytes, ms}, ...])."""
        h = self._native_handle()
        dev = self._device()
        pad = self.inference_padding if pad is None else pad
        x = c.to(device=dev, dtype=torch.float32).contiguous()
        B, C, T = x.shape
        n = N.lib().tts_melgan_output_length(h, T, pad, synth)
        if n < 0:
            N.check("tts_melgan_output_length", int(-n))
        out = torch.empty(B, 1 if synth else self._cfg.out_channels, n, device=dev, dtype=torch.float32)
        cap = 256
        recs = (N.TtsLaunchRecord * cap)()
        cnt = ctypes.c_int(0)
        N.call("tts_melgan_forward_profiled", h, N.ptr(x), B, C, T, pad, synth, N.ptr(out), N.stream_ptr(dev), recs,
               cap, ctypes.byref(cnt))
        rows = [
            {"name": recs[i].name.decode(), "flops": recs[i].flops, "bytes": recs[i].bytes, "ms": recs[i].ms}
            for i in range(min(cnt.value, cap))
        ]
        return out, rows

    def remove_weight_norm(self):
        for layer in self.layers:
            if isinstance(layer, ResidualStack):
                layer.remove_weight_norm()
            elif is_parametrized(layer, "weight"):
                remove_parametrizations(layer, "weight")
        self._release()

    def load_checkpoint(self, config, checkpoint_path, eval=False, cache=False):  # noqa: A002
        """Checkpoints are read with weights_only=True."""
        from ..io import load_fsspec

        state = load_fsspec(checkpoint_path, map_location=torch.device("cpu"), cache=cache)
        self.load_state_dict(state["model"])
        if eval:
            self.eval()
            assert not self.training
            self.remove_weight_norm()
