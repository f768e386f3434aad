"""Drop-in ForwardTTS (FastPitch / FastSpeech) whose inference runs in ``libtts_mi355x.so``.

* ``ForwardTTS`` is the inference surface of ``TTS/tts/models/forward_tts.py`` (Coqui TTS 0.22.0) with
  the ``"fftransformer"`` encoder and decoder: ``inference(x, aux_input)`` runs embedding -> encoder ->
  duration / pitch predictors -> expansion -> positional encoding -> decoder on the device and returns
  the reference's dict.  The nn modules below (``FFTransformer``, ``FFTransformerBlock``, ``Encoder``,
  ``Decoder``, ``PositionalEncoding``, the Glow ``DurationPredictor``) only hold parameters, under the
  reference's names, so reference checkpoints load unchanged (``aligner.*`` is training-only and
  dropped).  ``load_checkpoint`` reads the ``model`` dict with ``torch.load(weights_only=True)``.
* ``multi_head_attention`` is the attention proper of ``nn.MultiheadAttention`` as the ``FFTransformer``
  layers run it (``TTS/tts/layers/generic/transformer.py``): one ``tts_op_mha`` launch, online softmax on
  the matrix cores, any sequence length, head sizes up to 384.

Three extensions, each off by default (the default is the reference's behaviour):

* ``aux_input["x_lengths"]`` [B]: the reference takes every token of the batch as valid; with lengths
  the token mask is ragged (the encoder's keys are masked, padded tokens get duration 0).
* ``aux_input["durations"]`` [B, T_en] (integers): used in place of the predicted ones.
* ``ForwardTTS(..., mask_decoder_keys=True)``: the reference calls its decoder block without a mask, so
  in a ragged batch the decoder's queries attend over the padded frames too; with the flag the
  decoder's keys are masked with ``y_mask``.

The text side always runs the fp32-faithful fp32x6 arithmetic, so the durations do not depend on
``math_mode``; ``math_mode="bf16"`` selects single bf16 products for the decoder.
"""
from __future__ import annotations

import ctypes
import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from .. import _native as _nat
from ..config import FAST_PITCH
from .glow_tts import DurationPredictor

MAX_FRAMES = _nat.FORWARD_TTS_MAX_FRAMES


def mha_tile() -> int:
    """Queries one workgroup of the attention kernel computes."""
    return int(_nat.lib().tts_op_mha_tile())


@torch.no_grad()
def multi_head_attention(qkv: torch.Tensor, num_heads: int, key_lengths: torch.Tensor | None = None,
                         math_mode: str | None = None) -> torch.Tensor:
    """``qkv`` [B, 3E, T] (rows q | k | v, the ``in_proj`` output; head h = channels h dk ...) ->
    [B, E, T], the heads' outputs before ``out_proj``.  The ``dk ** -0.5`` query scale is applied here.

    ``key_lengths`` [B] (integer, values in [1, T]) is the key padding mask ``~sequence_mask(key_lengths)``:
    keys past an utterance's length get probability exactly 0; every query column is computed.  A length
    outside [1, T] is clamped to [0, T]; an item of length 0 (no key at all) comes out all zeros, where
    torch's softmax over nothing gives NaN.
    ``math_mode``: ``"bf16"`` for single bf16 products; every other mode (the package default included)
    runs the fp32-faithful fp32x6 kernel."""
    _nat.require_device_tensor(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[1] % 3 != 0:
        raise ValueError(f"expected qkv [B, 3E, T], got shape {tuple(qkv.shape)}")
    mode = _nat.default_math_mode() if math_mode is None else math_mode
    if mode not in _nat.MATH_MODES:
        raise ValueError(f"math_mode={mode!r}: must be one of {sorted(_nat.MATH_MODES)}")
    dev = qkv.device
    qkv = qkv.to(torch.float32).contiguous()
    B, E3, T = qkv.shape
    kl = None
    if key_lengths is not None:
        kl = torch.as_tensor(key_lengths).to(device=dev, dtype=torch.int64).contiguous()
        if kl.shape != (B,):
            raise ValueError(f"expected key_lengths [{B}], got shape {tuple(kl.shape)}")
    out = torch.empty(B, E3 // 3, T, device=dev, dtype=torch.float32)
    _nat.call("tts_op_mha", _nat.ptr(qkv), _nat.ptr(kl), B, E3 // 3, num_heads, T, _nat.MATH_MODES[mode],
              _nat.ptr(out), _nat.stream_ptr(dev))
    return out


# ------------------------------------------------------------------ parameter-only modules
class FFTransformer(nn.Module):
    """generic/transformer.py FFTransformer (parameters only)."""

    def __init__(self, in_out_channels, num_heads, hidden_channels_ffn=1024, kernel_size_fft=3, dropout_p=0.1):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(in_out_channels, num_heads, dropout=dropout_p)
        padding = (kernel_size_fft - 1) // 2
        self.conv1 = nn.Conv1d(in_out_channels, hidden_channels_ffn, kernel_size=kernel_size_fft, padding=padding)
        self.conv2 = nn.Conv1d(hidden_channels_ffn, in_out_channels, kernel_size=kernel_size_fft, padding=padding)
        self.norm1 = nn.LayerNorm(in_out_channels)
        self.norm2 = nn.LayerNorm(in_out_channels)


class FFTransformerBlock(nn.Module):
    """generic/transformer.py FFTransformerBlock (parameters only)."""

    def __init__(self, in_out_channels, num_heads, hidden_channels_ffn, num_layers, dropout_p):
        super().__init__()
        self.num_heads = num_heads
        self.hidden_channels_ffn = hidden_channels_ffn
        self.fft_layers = nn.ModuleList([
            FFTransformer(in_out_channels=in_out_channels, num_heads=num_heads, hidden_channels_ffn=hidden_channels_ffn,
                          dropout_p=dropout_p) for _ in range(num_layers)])


class FFTransformerDecoder(nn.Module):
    """feed_forward/decoder.py FFTransformerDecoder (parameters only)."""

    def __init__(self, in_channels, out_channels, params):
        super().__init__()
        self.transformer_block = FFTransformerBlock(in_channels, **params)
        self.postnet = nn.Conv1d(in_channels, out_channels, 1)


def _fft_params(params: Dict, what: str) -> Dict:
    p = {"hidden_channels_ffn": 1024, "num_heads": 2, "num_layers": 6, "dropout_p": 0.1}
    p.update(params or {})
    unknown = set(p) - {"hidden_channels_ffn", "num_heads", "num_layers", "dropout_p"}
    if unknown:
        raise ValueError(f"{what}: unknown fftransformer parameters {sorted(unknown)}")
    return p


class Encoder(nn.Module):
    """feed_forward/encoder.py Encoder, ``"fftransformer"`` only (parameters only)."""

    def __init__(self, in_hidden_channels, out_channels, encoder_type="fftransformer", encoder_params=None, c_in_channels=0):
        super().__init__()
        if encoder_type.lower() != "fftransformer":
            raise NotImplementedError(
                f"encoder_type={encoder_type!r}: only 'fftransformer' runs on the device (the relative_position_"
                "transformer and residual_conv_bn blocks of SpeedySpeech are follow-ups, DESIGN.md section 8)")
        assert in_hidden_channels == out_channels, "in_hidden_channels must be equal to out_channels"
        self.encoder = FFTransformerBlock(in_hidden_channels, **_fft_params(encoder_params, "encoder_params"))


class Decoder(nn.Module):
    """feed_forward/decoder.py Decoder, ``"fftransformer"`` only (parameters only)."""

    def __init__(self, out_channels, in_hidden_channels, decoder_type="fftransformer", decoder_params=None, c_in_channels=0):
        super().__init__()
        if decoder_type.lower() != "fftransformer":
            raise NotImplementedError(
                f"decoder_type={decoder_type!r}: only 'fftransformer' runs on the device (DESIGN.md section 8)")
        self.decoder = FFTransformerDecoder(in_hidden_channels, out_channels,
                                            _fft_params(decoder_params, "decoder_params"))


class PositionalEncoding(nn.Module):
    """generic/pos_encoding.py PositionalEncoding: the ``pe`` buffer [1, C, 5000], built as the
    reference builds it (a checkpoint's state dict carries it)."""

    def __init__(self, channels, dropout_p=0.0, max_len=MAX_FRAMES):
        super().__init__()
        if channels % 2 != 0:
            raise ValueError(f"Cannot use sin/cos positional encoding with odd channels (got channels={channels})")
        pe = torch.zeros(max_len, channels)
        position = torch.arange(0, max_len).unsqueeze(1)
        div_term = torch.pow(10000, torch.arange(0, channels, 2).float() / channels)
        pe[:, 0::2] = torch.sin(position.float() / div_term)
        pe[:, 1::2] = torch.cos(position.float() / div_term)
        pe = pe.unsqueeze(0).transpose(1, 2)
        self.register_buffer("pe", pe)
        self.channels = channels


@dataclass
class ForwardTTSArgs:
    """``ForwardTTSArgs`` of the reference, FastPitch defaults (``tts_amd.config.FAST_PITCH``)."""

    num_chars: Optional[int] = None
    out_channels: int = FAST_PITCH["out_channels"]
    hidden_channels: int = FAST_PITCH["hidden_channels"]
    use_aligner: bool = True
    use_pitch: bool = True
    pitch_predictor_hidden_channels: int = 256
    pitch_predictor_kernel_size: int = 3
    pitch_predictor_dropout_p: float = 0.1
    pitch_embedding_kernel_size: int = 3
    use_energy: bool = False
    duration_predictor_hidden_channels: int = 256
    duration_predictor_kernel_size: int = 3
    duration_predictor_dropout_p: float = 0.1
    positional_encoding: bool = True
    length_scale: float = 1
    encoder_type: str = "fftransformer"
    encoder_params: dict = field(default_factory=lambda: dict(FAST_PITCH["encoder_params"]))
    decoder_type: str = "fftransformer"
    decoder_params: dict = field(default_factory=lambda: dict(FAST_PITCH["decoder_params"]))
    num_speakers: int = 1
    use_speaker_embedding: bool = False
    use_d_vector_file: bool = False
    d_vector_dim: int = 0


def _f32(t: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())


class ForwardTTS(nn.Module):
    def __init__(self, args: ForwardTTSArgs | Dict, math_mode: Optional[str] = None, mask_decoder_keys: bool = False):
        super().__init__()
        if isinstance(args, dict):
            names = {f.name for f in dataclasses.fields(ForwardTTSArgs)}
            args = ForwardTTSArgs(**{k: v for k, v in args.items() if k in names})
        self.args = args
        if args.num_chars is None:
            raise ValueError("num_chars is required")
        if args.use_energy:
            raise NotImplementedError("use_energy=True (FastSpeech2) is not implemented (DESIGN.md section 8)")
        if args.use_d_vector_file:
            raise NotImplementedError("use_d_vector_file=True is not implemented (DESIGN.md section 8)")
        mode = _nat.default_math_mode() if math_mode is None else math_mode
        if mode not in _nat.MATH_MODES:
            raise ValueError(f"math_mode must be one of {sorted(_nat.MATH_MODES)}")
        self.math_mode = mode
        self.mask_decoder_keys = bool(mask_decoder_keys)
        self.length_scale = float(args.length_scale)
        self.num_speakers = args.num_speakers
        H = args.hidden_channels
        self.emb = nn.Embedding(args.num_chars, H)
        self.encoder = Encoder(H, H, args.encoder_type, args.encoder_params)
        if args.positional_encoding:
            self.pos_encoder = PositionalEncoding(H)
        self.decoder = Decoder(args.out_channels, H, args.decoder_type, args.decoder_params)
        self.duration_predictor = DurationPredictor(H, args.duration_predictor_hidden_channels,
                                                    args.duration_predictor_kernel_size,
                                                    args.duration_predictor_dropout_p)
        if args.use_pitch:
            self.pitch_predictor = DurationPredictor(H, args.pitch_predictor_hidden_channels,
                                                     args.pitch_predictor_kernel_size, args.pitch_predictor_dropout_p)
            k = args.pitch_embedding_kernel_size
            self.pitch_emb = nn.Conv1d(1, H, kernel_size=k, padding=int((k - 1) / 2))
        if args.use_speaker_embedding:  # init_multispeaker
            self.emb_g = nn.Embedding(args.num_speakers, H)
            nn.init.uniform_(self.emb_g.weight, -0.1, 0.1)
        ep, dp = self.encoder.encoder, self.decoder.decoder.transformer_block
        c = _nat.TtsForwardTtsCfg()
        c.num_chars = args.num_chars
        c.out_channels = args.out_channels
        c.hidden_channels = H
        c.encoder_ffn_channels, c.encoder_num_heads, c.encoder_num_layers = (
            ep.hidden_channels_ffn, ep.num_heads, len(ep.fft_layers))
        c.decoder_ffn_channels, c.decoder_num_heads, c.decoder_num_layers = (
            dp.hidden_channels_ffn, dp.num_heads, len(dp.fft_layers))
        c.duration_predictor_hidden_channels = args.duration_predictor_hidden_channels
        c.duration_predictor_kernel_size = args.duration_predictor_kernel_size
        c.use_pitch = 1 if args.use_pitch else 0
        c.pitch_predictor_hidden_channels = args.pitch_predictor_hidden_channels
        c.pitch_predictor_kernel_size = args.pitch_predictor_kernel_size
        c.pitch_embedding_kernel_size = args.pitch_embedding_kernel_size
        c.positional_encoding = 1 if args.positional_encoding else 0
        c.num_speakers = args.num_speakers if args.use_speaker_embedding else 0
        c.math_mode = _nat.MATH_MODES[mode]
        self._cfg = c
        self._handle = None
        self._handle_key = None
        n = _nat.lib().tts_forward_tts_num_weights(ctypes.byref(c))
        if n < 0:
            _nat.check("tts_forward_tts_num_weights", -n)

    # ------------------------------------------------------------------ native handle
    def _weight_list(self) -> List[np.ndarray]:
        ws: List[np.ndarray] = [_f32(self.emb.weight)]

        def block(b: FFTransformerBlock):
            for L in b.fft_layers:
                a = L.self_attn
                ws.extend(_f32(t) for t in (a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                                            L.conv1.weight, L.conv1.bias, L.conv2.weight, L.conv2.bias,
                                            L.norm1.weight, L.norm1.bias, L.norm2.weight, L.norm2.bias))

        def predictor(p: DurationPredictor):
            for conv, norm in ((p.conv_1, p.norm_1), (p.conv_2, p.norm_2)):
                ws.extend([_f32(conv.weight), _f32(conv.bias), _f32(norm.gamma).reshape(-1), _f32(norm.beta).reshape(-1)])
            ws.extend([_f32(p.proj.weight), _f32(p.proj.bias)])

        block(self.encoder.encoder)
        if self.args.positional_encoding:
            ws.append(_f32(self.pos_encoder.pe[0]))
        block(self.decoder.decoder.transformer_block)
        ws.extend([_f32(self.decoder.decoder.postnet.weight), _f32(self.decoder.decoder.postnet.bias)])
        predictor(self.duration_predictor)
        if self.args.use_pitch:
            predictor(self.pitch_predictor)
            ws.extend([_f32(self.pitch_emb.weight), _f32(self.pitch_emb.bias)])
        if hasattr(self, "emb_g"):
            ws.append(_f32(self.emb_g.weight))
        return ws

    def _device(self) -> torch.device:
        dev = self.emb.weight.device
        if dev.type != "cuda":
            raise RuntimeError("ForwardTTS (tts_amd) runs only on a ROCm device: move it with .to('cuda') first "
                               "(there is no CPU fallback)")
        return dev

    def _native_handle(self):
        key = tuple((p.data_ptr(), p._version, p.device) for p in list(self.parameters()) + list(self.buffers()))
        if self._handle is not None and key == self._handle_key:
            return self._handle
        self._release()
        dev = self._device()
        ws = self._weight_list()
        lib = _nat.lib()
        for i, w in enumerate(ws):
            n = lib.tts_forward_tts_weight_numel(ctypes.byref(self._cfg), i)
            if n != w.size:
                raise ValueError(f"weight {i} has {w.size} elements, expected {n}")
        arr = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        h = ctypes.c_void_p()
        _nat.call("tts_forward_tts_create", ctypes.byref(self._cfg), arr, dev.index or 0, ctypes.byref(h))
        self._handle, self._handle_key = h, key
        return h

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            _nat.lib().tts_forward_tts_destroy(self._handle)
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
    def _inputs(self, x, aux_input):
        aux = aux_input or {}
        dev = self._device()
        tok = x.to(device=dev, dtype=torch.int64).contiguous()
        if tok.dim() != 2:
            raise ValueError(f"x must be [B, T_en] token ids, got shape {tuple(tok.shape)}")
        B, T = tok.shape
        if aux.get("d_vectors") is not None:
            raise NotImplementedError("d_vectors (use_d_vector_file) are not implemented (DESIGN.md section 8)")
        spk = aux.get("speaker_ids")
        if hasattr(self, "emb_g"):
            if spk is None:
                raise ValueError("this model has a speaker embedding: pass aux_input['speaker_ids']")
            spk = torch.as_tensor(spk).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            if spk.shape != (B,):
                raise ValueError(f"speaker_ids must be [{B}], got {tuple(spk.shape)}")
        else:
            spk = None  # the reference ignores speaker ids without emb_g
        lens = aux.get("x_lengths")
        lens = torch.full((B,), T, dtype=torch.int64, device=dev) if lens is None else \
            torch.as_tensor(lens).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if lens.shape != (B,):
            raise ValueError(f"x_lengths must be [{B}], got {tuple(lens.shape)}")
        given = aux.get("durations")
        if given is not None:
            given = torch.as_tensor(given)
            if given.shape != (B, T):
                raise ValueError(f"durations must be [{B}, {T}], got {tuple(given.shape)}")
            frames = int(given.sum(1).max())
            if frames < 1:
                raise ValueError("durations: no frames")
            self._check_frames(frames)  # before any launch
            given = given.to(device=dev, dtype=torch.float32).contiguous()
        return dev, tok, lens, spk, given

    def _check_frames(self, frames: int) -> None:
        if self.args.positional_encoding and frames > MAX_FRAMES:
            raise ValueError(f"{frames} frames: the positional encoding holds {MAX_FRAMES} "
                             "(the reference raises RuntimeError in PositionalEncoding.forward)")

    def _run(self, x, aux_input, profile: bool = False):
        h = self._native_handle()
        dev, tok, lens, spk, given = self._inputs(x, aux_input)
        B, T = tok.shape
        H = self.args.hidden_channels
        f = dict(device=dev, dtype=torch.float32)
        o_en = torch.empty(B, H, T, **f)
        x_mask = torch.empty(B, 1, T, **f)
        dlog = torch.empty(B, 1, T, **f)
        pitch = torch.empty(B, 1, T, **f) if self.args.use_pitch else None
        dur = torch.empty(B, T, **f)
        y_len = torch.empty(B, dtype=torch.int64, device=dev)
        stream = _nat.stream_ptr(dev)
        rows: List[Dict] = []
        cap = 1024
        recs = (_nat.TtsLaunchRecord * cap)()
        n = ctypes.c_int(0)

        def collect():
            rows.extend({"name": recs[i].name.decode(), "flops": recs[i].flops, "bytes": recs[i].bytes,
                         "ms": recs[i].ms} for i in range(min(n.value, cap)))

        enc_args = (h, _nat.ptr(tok), _nat.ptr(lens), _nat.ptr(spk), _nat.ptr(given), B, T, float(self.length_scale),
                    _nat.ptr(o_en), _nat.ptr(x_mask), _nat.ptr(dlog), _nat.ptr(pitch), _nat.ptr(dur), _nat.ptr(y_len),
                    stream)
        if profile:
            _nat.call("tts_forward_tts_encode_profiled", *enc_args, recs, cap, ctypes.byref(n))
            collect()
        else:
            _nat.call("tts_forward_tts_encode", *enc_args)
        T_de = int(y_len.max().item())  # the one host read: sequence_mask(y_lengths, None)
        if T_de < 1:
            raise ValueError("no frames: every duration is 0")
        self._check_frames(T_de)
        out = torch.empty(B, self.args.out_channels, T_de, **f)
        attn = torch.empty(B, T, T_de, **f)
        y_mask = torch.empty(B, 1, T_de, **f)
        dec_args = (h, _nat.ptr(o_en), _nat.ptr(dur), _nat.ptr(x_mask), _nat.ptr(y_len), B, T, T_de,
                    1 if self.mask_decoder_keys else 0, _nat.ptr(out), _nat.ptr(attn), _nat.ptr(y_mask), stream)
        if profile:
            _nat.call("tts_forward_tts_decode_profiled", *dec_args, recs, cap, ctypes.byref(n))
            collect()
        else:
            _nat.call("tts_forward_tts_decode", *dec_args)
        outputs = {"model_outputs": out.transpose(1, 2), "alignments": attn.transpose(1, 2), "pitch": pitch,
                   "energy": None, "durations_log": dlog}
        return outputs, rows

    @torch.no_grad()
    def inference(self, x, aux_input={"d_vectors": None, "speaker_ids": None}):  # noqa: B006
        """forward_tts.py inference: x [B, T_en] token ids -> {"model_outputs" [B, T_de, C], "alignments"
        [B, T_de, T_en], "pitch" [B, 1, T_en], "energy" None, "durations_log" [B, 1, T_en]}.  The
        rounded durations are ``alignments.sum(1)``.  ``aux_input`` may also carry the extensions
        ``x_lengths`` and ``durations`` (module docstring)."""
        return self._run(x, aux_input)[0]

    @torch.no_grad()
    def profile(self, x, aux_input=None):
        """One inference with a hipEvent pair around every launch: (outputs, [{name, flops, bytes, ms}])."""
        return self._run(x, aux_input, profile=True)

    @torch.no_grad()
    def fft_block(self, x: torch.Tensor, key_lengths: Optional[torch.Tensor] = None, decoder: bool = False):
        """``FFTransformerBlock.forward`` of the encoder (fp32x6) or the decoder (the model's math mode):
        x [B, H, T] -> [B, H, T]; ``key_lengths`` [B] is the key padding mask.  Every column is computed,
        the padded ones included (the reference masks nothing but the keys)."""
        h = self._native_handle()
        dev = self._device()
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        B, H, T = x.shape
        if H != self.args.hidden_channels:
            raise ValueError(f"expected [B, {self.args.hidden_channels}, T], got {tuple(x.shape)}")
        kl = None if key_lengths is None else torch.as_tensor(key_lengths).to(device=dev, dtype=torch.int64).contiguous()
        y = torch.empty_like(x)
        _nat.call("tts_forward_tts_block", h, 1 if decoder else 0, _nat.ptr(x), _nat.ptr(kl), B, T, _nat.ptr(y),
                  _nat.stream_ptr(dev))
        return y

    def load_checkpoint(self, config, checkpoint_path, eval=True, cache=False):
        state = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        state = state["model"] if "model" in state else state
        self.load_state_dict({k: v for k, v in state.items() if not k.startswith("aligner.")})
        if eval:
            self.eval()
            assert not self.training


__all__ = ["ForwardTTS", "ForwardTTSArgs", "multi_head_attention"]
