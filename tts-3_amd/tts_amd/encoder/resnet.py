"""Drop-in ``ResNetSpeakerEncoder`` (``TTS/encoder/models/resnet.py`` + ``base_encoder.py``) on the
MI355X path: reference wav (or features) in, d-vector out, all of it in ``tts_speaker_encoder_forward``.

The module tree exists for its ``state_dict()``: the key set and shapes are the reference's, so its
checkpoints (and the ``speaker_encoder.*`` slice of an XTTS checkpoint) load unchanged.  No submodule
is ever called; there is no PyTorch fallback.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch
from torch import nn

from .. import _native as N

XTTS_AUDIO_CONFIG = dict(fft_size=512, win_length=400, hop_length=160, sample_rate=16000, preemphasis=0.97, num_mels=64)


def mel_filterbank(n_freqs: int, sample_rate: int, n_mels: int) -> torch.Tensor:
    """torchaudio ``melscale_fbanks(n_freqs, 0, sample_rate / 2, n_mels, sample_rate, norm=None, "htk")``:
    [n_freqs, n_mels], computed in fp64."""
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)  # noqa: E731
    all_freqs = np.linspace(0.0, float(sample_rate // 2), n_freqs)
    m_pts = np.linspace(hz2mel(0.0), hz2mel(sample_rate / 2.0), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.from_numpy(np.maximum(0.0, np.minimum(down, up)))


def window_offsets(max_len: int, num_frames: int, num_eval: int):
    """``compute_embedding``'s windows: (start, end) pairs over a clip of ``max_len``."""
    num_frames = min(num_frames, max_len)
    return [(int(o), int(o + num_frames)) for o in np.linspace(0, max_len - num_frames, num=num_eval)]


class SELayer(nn.Module):
    def __init__(self, channel, reduction=8):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction), nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel), nn.Sigmoid())


class SEBasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, reduction=8):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.se = SELayer(planes, reduction)
        self.downsample = downsample
        self.stride = stride


class PreEmphasis(nn.Module):
    def __init__(self, coefficient=0.97):
        super().__init__()
        self.coefficient = coefficient
        self.register_buffer("filter", torch.FloatTensor([-self.coefficient, 1.0]).unsqueeze(0).unsqueeze(0))


class _Spectrogram(nn.Module):
    def __init__(self, win_length):
        super().__init__()
        self.register_buffer("window", torch.hamming_window(win_length))


class _MelScale(nn.Module):
    def __init__(self, n_freqs, sample_rate, n_mels):
        super().__init__()
        self.register_buffer("fb", mel_filterbank(n_freqs, sample_rate, n_mels).float())


class _MelSpectrogram(nn.Module):
    """The buffers of ``torchaudio.transforms.MelSpectrogram`` (``spectrogram.window``, ``mel_scale.fb``)."""

    def __init__(self, sample_rate, n_fft, win_length, hop_length, n_mels):
        super().__init__()
        self.spectrogram = _Spectrogram(win_length)
        self.mel_scale = _MelScale(n_fft // 2 + 1, sample_rate, n_mels)


def _host(t: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


class ResNetSpeakerEncoder(nn.Module):
    def __init__(self, input_dim=64, proj_dim=512, layers=(3, 4, 6, 3), num_filters=(32, 64, 128, 256),
                 encoder_type="ASP", log_input=False, use_torch_spec=False, audio_config=None,
                 math_mode: Optional[str] = None):
        super().__init__()
        layers, num_filters = list(layers), list(num_filters)
        if len(layers) != 4 or len(num_filters) != 4:
            raise ValueError("layers and num_filters must have four entries")
        if encoder_type not in ("ASP", "SAP"):
            raise ValueError("Undefined encoder")
        if use_torch_spec and audio_config is None:
            raise ValueError("use_torch_spec needs an audio_config")
        if math_mode is None:
            math_mode = N.default_math_mode()
        if math_mode not in N.MATH_MODES:
            raise ValueError(f"math_mode={math_mode!r}: must be one of {sorted(N.MATH_MODES)}")
        self.math_mode = math_mode
        self.encoder_type = encoder_type
        self.input_dim = input_dim
        self.log_input = log_input
        self.use_torch_spec = use_torch_spec
        self.audio_config = audio_config
        self.proj_dim = proj_dim

        self.conv1 = nn.Conv2d(1, num_filters[0], kernel_size=3, stride=1, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.bn1 = nn.BatchNorm2d(num_filters[0])
        self.inplanes = num_filters[0]
        self.layer1 = self.create_layer(SEBasicBlock, num_filters[0], layers[0])
        self.layer2 = self.create_layer(SEBasicBlock, num_filters[1], layers[1], stride=(2, 2))
        self.layer3 = self.create_layer(SEBasicBlock, num_filters[2], layers[2], stride=(2, 2))
        self.layer4 = self.create_layer(SEBasicBlock, num_filters[3], layers[3], stride=(2, 2))
        self.instancenorm = nn.InstanceNorm1d(input_dim)
        if self.use_torch_spec:
            ac = audio_config
            self.torch_spec = nn.Sequential(
                PreEmphasis(ac["preemphasis"]),
                _MelSpectrogram(ac["sample_rate"], ac["fft_size"], ac["win_length"], ac["hop_length"], ac["num_mels"]))
        else:
            self.torch_spec = None
        outmap_size = int(self.input_dim / 8)
        D = num_filters[3] * outmap_size
        self.attention = nn.Sequential(nn.Conv1d(D, 128, kernel_size=1), nn.ReLU(), nn.BatchNorm1d(128),
                                       nn.Conv1d(128, D, kernel_size=1), nn.Softmax(dim=2))
        self.fc = nn.Linear(D if encoder_type == "SAP" else 2 * D, proj_dim)

        c = N.TtsSpeakerEncoderCfg()
        c.input_dim = input_dim
        c.proj_dim = proj_dim
        for i in range(4):
            c.layers[i] = layers[i]
            c.num_filters[i] = num_filters[i]
        c.encoder_type = N.SPK_ASP if encoder_type == "ASP" else N.SPK_SAP
        c.log_input = int(bool(log_input))
        c.use_torch_spec = int(bool(use_torch_spec))
        if use_torch_spec:
            if audio_config["num_mels"] != input_dim:
                raise ValueError("audio_config['num_mels'] must equal input_dim")
            c.fft_size, c.win_length, c.hop_length = (audio_config[k] for k in ("fft_size", "win_length", "hop_length"))
        c.math_mode = N.MATH_MODES[math_mode]
        self._cfg = c
        self._handle = None
        self._handle_key = None
        n = N.lib().tts_speaker_encoder_num_weights(ctypes.byref(c))  # fail at construction
        if n < 0:
            N.check("tts_speaker_encoder_num_weights", -n)

    def create_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    # ------------------------------------------------------------------ native handle
    @staticmethod
    def _bn(m) -> List[np.ndarray]:
        return [_host(m.weight), _host(m.bias), _host(m.running_mean), _host(m.running_var)]

    def _weight_list(self) -> List[np.ndarray]:
        """fp32 weights in the C-ABI order (include/tts_mi355x.h)."""
        ws: List[np.ndarray] = []
        if self.use_torch_spec:
            ws += [_host(self.torch_spec[0].filter).reshape(-1), _host(self.torch_spec[1].spectrogram.window),
                   _host(self.torch_spec[1].mel_scale.fb)]
        ws += [_host(self.conv1.weight), _host(self.conv1.bias)] + self._bn(self.bn1)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for b in layer:
                ws += [_host(b.conv1.weight)] + self._bn(b.bn1) + [_host(b.conv2.weight)] + self._bn(b.bn2)
                ws += [_host(b.se.fc[0].weight), _host(b.se.fc[0].bias), _host(b.se.fc[2].weight), _host(b.se.fc[2].bias)]
                if b.downsample is not None:
                    ws += [_host(b.downsample[0].weight)] + self._bn(b.downsample[1])
        a = self.attention
        ws += [_host(a[0].weight), _host(a[0].bias)] + self._bn(a[2]) + [_host(a[3].weight), _host(a[3].bias)]
        ws += [_host(self.fc.weight), _host(self.fc.bias)]
        return ws

    def _param_key(self):
        return tuple((p.data_ptr(), p._version, p.device) for p in list(self.parameters()) + list(self.buffers()))

    def _device(self) -> torch.device:
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__} (tts_amd) runs only on a ROCm device: move the module with "
                ".to('cuda') first (there is no CPU fallback)")
        return dev

    def _native_handle(self):
        key = self._param_key()
        if self._handle is not None and key == self._handle_key:
            return self._handle
        self._release()
        dev = self._device()
        ws = self._weight_list()
        lib = N.lib()
        expected = lib.tts_speaker_encoder_num_weights(ctypes.byref(self._cfg))
        if expected < 0:
            N.check("tts_speaker_encoder_num_weights", -expected)
        if expected != len(ws):
            raise RuntimeError(f"internal: {len(ws)} weight tensors, library expects {expected}")
        for i, w in enumerate(ws):
            n = lib.tts_speaker_encoder_weight_numel(ctypes.byref(self._cfg), i)
            if n != w.size:
                raise ValueError(f"weight {i} has {w.size} elements, expected {n}")
        arr = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        h = ctypes.c_void_p()
        N.call("tts_speaker_encoder_create", ctypes.byref(self._cfg), arr, dev.index or 0, ctypes.byref(h))
        self._handle, self._handle_key = h, key
        return h

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            N.lib().tts_speaker_encoder_destroy(self._handle)
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
    def _input(self, x: torch.Tensor):
        dev = self._device()
        N.require_device_tensor(x, f"{type(self).__name__} input")
        x = x.to(device=dev, dtype=torch.float32)
        if x.dim() == 3 and x.shape[1] == 1 and (self.use_torch_spec or self.input_dim != 1):
            x = x.squeeze(1)  # the reference's x.squeeze_(1)
        if self.use_torch_spec:
            if x.dim() != 2:
                raise ValueError(f"expected a [B, samples] wav, got shape {tuple(x.shape)}")
        elif x.dim() != 3 or x.shape[1] != self.input_dim:
            raise ValueError(f"expected [B, {self.input_dim}, T] features, got shape {tuple(x.shape)}")
        return dev, x.contiguous()

    def num_frames(self, n: int) -> int:
        """Frames of an ``n``-sample wav (``use_torch_spec``), as the library counts them; raises
        ``NativeError`` outside the limits."""
        t = N.lib().tts_speaker_encoder_num_frames(self._native_handle(), n)
        if t < 0:
            N.check("tts_speaker_encoder_num_frames", int(-t))
        return int(t)

    def forward(self, x: torch.Tensor, l2_norm: bool = False) -> torch.Tensor:
        """x: [B, samples] wav at ``audio_config['sample_rate']`` (``use_torch_spec``) or
        [B, input_dim, T] features -> [B, proj_dim].  Inference only; no host synchronisation."""
        with torch.no_grad():
            dev, x = self._input(x)
            h = self._native_handle()
            B, n = x.shape[0], x.shape[-1]
            out = torch.empty(B, self.proj_dim, device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                N.call("tts_speaker_encoder_forward", h, N.ptr(x), B, n, int(bool(l2_norm)), N.ptr(out), N.stream_ptr(dev))
            return out

    @torch.no_grad()
    def inference(self, x: torch.Tensor, l2_norm: bool = True) -> torch.Tensor:
        return self.forward(x, l2_norm)

    @torch.no_grad()
    def features(self, x: torch.Tensor) -> torch.Tensor:
        """The trunk's input [B, input_dim, T]: front end (``use_torch_spec``), log, instance norm."""
        dev, x = self._input(x)
        h = self._native_handle()
        B, n = x.shape[0], x.shape[-1]
        out = torch.empty(B, self.input_dim, self.num_frames(n), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            N.call("tts_speaker_encoder_features", h, N.ptr(x), B, n, N.ptr(out), N.stream_ptr(dev))
        return out

    def profile(self, x: torch.Tensor, l2_norm: bool = False):
        """One forward with a hipEvent pair around every launch: (out, [{name, flops, bytes, ms}, ...])."""
        dev, x = self._input(x)
        h = self._native_handle()
        B, n = x.shape[0], x.shape[-1]
        out = torch.empty(B, self.proj_dim, device=dev, dtype=torch.float32)
        cap = 512
        recs = (N.TtsLaunchRecord * cap)()
        cnt = ctypes.c_int(0)
        with torch.cuda.device(dev):
            N.call("tts_speaker_encoder_forward_profiled", h, N.ptr(x), B, n, int(bool(l2_norm)), N.ptr(out),
                   N.stream_ptr(dev), recs, cap, ctypes.byref(cnt))
        rows = [{"name": recs[i].name.decode(), "flops": recs[i].flops, "bytes": recs[i].bytes, "ms": recs[i].ms}
                for i in range(min(cnt.value, cap))]
        return out, rows

    @torch.no_grad()
    def compute_embedding(self, x, num_frames=250, num_eval=10, return_mean=True, l2_norm=True):
        """``num_eval`` windows of ``num_frames`` frames spread evenly over the clip (x: [1, samples]
        with ``use_torch_spec``, else [1, input_dim, T]), one batched forward, their mean."""
        if self.use_torch_spec:
            num_frames = num_frames * self.audio_config["hop_length"]
        max_len = x.shape[-1] if not self.use_torch_spec else x.shape[1]
        frames_batch = [x[..., a:b] for a, b in window_offsets(max_len, num_frames, num_eval)]
        embeddings = self.inference(torch.cat(frames_batch, dim=0), l2_norm=l2_norm)
        if return_mean:
            embeddings = torch.mean(embeddings, dim=0, keepdim=True)
        return embeddings

    def load_checkpoint(self, checkpoint_path: str, eval: bool = False, use_cuda: bool = False, criterion=None,  # noqa: A002
                        cache=False):
        """Checkpoints are read with weights_only=True; ``model`` holds the state dict (criterion keys
        of a training checkpoint are ignored)."""
        from ..io import load_fsspec

        state = load_fsspec(checkpoint_path, map_location=torch.device("cpu"), cache=cache)
        state = state["model"] if "model" in state else state
        own = set(self.state_dict().keys())
        self.load_state_dict({k: v for k, v in state.items() if k in own})
        if use_cuda:
            self.cuda()
        if eval:
            self.eval()
            assert not self.training
        return None


__all__ = ["ResNetSpeakerEncoder", "XTTS_AUDIO_CONFIG", "mel_filterbank", "window_offsets"]
