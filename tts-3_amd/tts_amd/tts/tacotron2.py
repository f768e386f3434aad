"""Drop-in Tacotron2 whose inference runs in ``libtts_mi355x.so``.

* ``Tacotron2`` is the inference surface of ``TTS/tts/models/tacotron2.py`` (Coqui TTS 0.22.0) with the
  ``"original"`` location-sensitive attention and prenet: ``inference(x, aux_input)`` runs embedding ->
  encoder (convs, biLSTM) -> the recurrent decoder (attention RNN, attention, decoder RNN, projection,
  stopnet; at most 5 launches per step, no host synchronisation per step) -> postnet on the device and
  returns the reference's dict.  The nn modules below only hold parameters, under the reference's
  names, so reference checkpoints load unchanged (``coarse_decoder.*``, the training-only second
  decoder of double-decoder consistency, is dropped).
* ``lstm_cell`` is one ``nn.LSTMCell`` step through the decoder's kernel (``tts_op_lstm_cell``).

Extensions, each off by default (the default is the reference's behaviour, whose loop only works at
B = 1):

* ``aux_input["x_lengths"]`` [B]: the biLSTM runs with ``pack_padded_sequence`` semantics (the reverse
  direction starts at each utterance's last token, padded outputs are zero) and the attention masks the
  keys at or beyond the length.
* per-utterance stopping in a batch: utterance b ends at its own first step t >= 1 with
  ``stop_b > stop_threshold``; its rows after that are zero and ``outputs["y_lengths"][b] = steps_b * r``.
* width keywords (``encoder_dim``, ``query_dim``, ``prenet_dim``, ``attention_dim``, ``location_filters``,
  ``location_kernel_size``, ``speaker_embedding_dim``): the widths the reference hard-codes.

Memory: the library fills caller-supplied ``[B, max_decoder_steps, ...]`` buffers, so ``inference`` allocates
(and the decoder clears) ``decoder_outputs``, ``alignments`` and ``stop_tokens`` for all ``max_decoder_steps``
steps before it knows where the utterances end, and trims them afterwards: ``4 B max_decoder_steps
(C r + T_en + 1)`` bytes, 12 MB at B = 1, T_en = 128 with the default 10000 steps, 2.8 GB at B = 32,
T_en = 2048.  Set ``model.max_decoder_steps`` to what the texts can need for large batches of long texts.

``math_mode="bf16"`` stores the attention and decoder RNN matrices as bf16 and runs the convs in bf16;
every other mode keeps fp32 weights with exact fp32 products in the recurrent kernels.
"""
from __future__ import annotations

import ctypes
import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from .. import _native as _nat
from ..config import TACOTRON2

MAX_BATCH = _nat.TACOTRON2_MAX_BATCH
MAX_TOKENS = _nat.TACOTRON2_MAX_TOKENS
POSTNET_DIM = 512


def _f32(t: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())


@torch.no_grad()
def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh, math_mode: Optional[str] = None):
    """``nn.LSTMCell``: x [B, I], h, c [B, H] on the device, torch-layout weights -> (h', c').
    B <= 32, H a multiple of 4.  ``math_mode="bf16"``: bf16-stored matrices; else exact fp32 products."""
    _nat.require_device_tensor(x, "x")
    mode = _nat.default_math_mode() if math_mode is None else math_mode
    if mode not in _nat.MATH_MODES:
        raise ValueError(f"math_mode={mode!r}: must be one of {sorted(_nat.MATH_MODES)}")
    dev = x.device
    x, h, c = (t.to(device=dev, dtype=torch.float32).contiguous() for t in (x, h, c))
    B, I = x.shape
    H = h.shape[1]
    if h.shape != (B, H) or c.shape != (B, H) or tuple(w_ih.shape) != (4 * H, I) or tuple(w_hh.shape) != (4 * H, H):
        raise ValueError("lstm_cell: inconsistent shapes")
    ws = [_f32(w_ih), _f32(w_hh), _f32(b_ih), _f32(b_hh)]
    ho, co = torch.empty_like(h), torch.empty_like(c)
    _nat.call("tts_op_lstm_cell", _nat.ptr(x), _nat.ptr(h), _nat.ptr(c), B, I, H, *[_nat.ptr(w) for w in ws],
              _nat.MATH_MODES[mode], _nat.ptr(ho), _nat.ptr(co), _nat.stream_ptr(dev))
    return ho, co


# ------------------------------------------------------------------ parameter-only modules
class Linear(nn.Module):
    """common_layers.py Linear (parameters only)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear_layer = nn.Linear(in_features, out_features, bias=bias)


class ConvBNBlock(nn.Module):
    """tacotron2.py ConvBNBlock (parameters only)."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        self.convolution1d = nn.Conv1d(in_channels, out_channels, kernel_size, padding=(kernel_size - 1) // 2)
        self.batch_normalization = nn.BatchNorm1d(out_channels, momentum=0.1, eps=1e-5)


class Encoder(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.convolutions = nn.ModuleList([ConvBNBlock(dim, dim, 5) for _ in range(3)])
        self.lstm = nn.LSTM(dim, dim // 2, num_layers=1, batch_first=True, bias=True, bidirectional=True)


class Postnet(nn.Module):
    def __init__(self, channels):
        super().__init__()
        dims = [channels] + [POSTNET_DIM] * 4 + [channels]
        self.convolutions = nn.ModuleList([ConvBNBlock(dims[i], dims[i + 1], 5) for i in range(5)])


class Prenet(nn.Module):
    def __init__(self, in_features, dim):
        super().__init__()
        self.linear_layers = nn.ModuleList([Linear(in_features, dim, bias=False), Linear(dim, dim, bias=False)])


class LocationLayer(nn.Module):
    def __init__(self, attention_dim, filters, kernel_size):
        super().__init__()
        self.location_conv1d = nn.Conv1d(2, filters, kernel_size, padding=(kernel_size - 1) // 2, bias=False)
        self.location_dense = Linear(filters, attention_dim, bias=False)


class OriginalAttention(nn.Module):
    def __init__(self, query_dim, embedding_dim, attention_dim, filters, kernel_size):
        super().__init__()
        self.query_layer = Linear(query_dim, attention_dim, bias=False)
        self.inputs_layer = Linear(embedding_dim, attention_dim, bias=False)
        self.v = Linear(attention_dim, 1, bias=True)
        self.location_layer = LocationLayer(attention_dim, filters, kernel_size)


class Decoder(nn.Module):
    def __init__(self, in_channels, frame_channels, r, query_dim, prenet_dim, attention_dim, filters, kernel_size):
        super().__init__()
        self.prenet = Prenet(frame_channels, prenet_dim)
        self.attention_rnn = nn.LSTMCell(prenet_dim + in_channels, query_dim, bias=True)
        self.attention = OriginalAttention(query_dim, in_channels, attention_dim, filters, kernel_size)
        self.decoder_rnn = nn.LSTMCell(query_dim + in_channels, query_dim, bias=True)
        self.linear_projection = Linear(query_dim + in_channels, frame_channels * r)
        self.stopnet = nn.Sequential(nn.Dropout(0.1), Linear(query_dim + frame_channels * r, 1, bias=True))


@dataclass
class Tacotron2Args:
    """The fields ``Tacotron2Config`` feeds the model (defaults: ``tts_amd.config.TACOTRON2``), and the
    width keywords (the reference's hard-coded values)."""

    num_chars: Optional[int] = None
    out_channels: int = TACOTRON2["out_channels"]
    r: int = TACOTRON2["r"]
    attention_type: str = "original"
    attention_norm: str = "sigmoid"
    location_attn: bool = True
    windowing: bool = False
    use_forward_attn: bool = False
    transition_agent: bool = False
    forward_attn_mask: bool = False
    prenet_type: str = "original"
    prenet_dropout: bool = True
    prenet_dropout_at_inference: bool = False
    separate_stopnet: bool = True
    stop_threshold: float = 0.5
    max_decoder_steps: int = TACOTRON2["max_decoder_steps"]
    num_speakers: int = 1
    use_speaker_embedding: bool = False
    use_d_vector_file: bool = False
    d_vector_dim: int = 0
    double_decoder_consistency: bool = False
    use_gst: bool = False
    use_capacitron_vae: bool = False
    encoder_dim: int = 512
    query_dim: int = 1024
    prenet_dim: int = 256
    attention_dim: int = 128
    location_filters: int = 32
    location_kernel_size: int = 31
    speaker_embedding_dim: int = 512


_EXCLUDED = "not implemented on the device (DESIGN.md section 8)"


class Tacotron2(nn.Module):
    def __init__(self, args: Tacotron2Args | Dict, math_mode: Optional[str] = None, chunk: int = 32):
        super().__init__()
        if isinstance(args, dict):
            names = {f.name for f in dataclasses.fields(Tacotron2Args)}
            args = Tacotron2Args(**{k: v for k, v in args.items() if k in names})
        self.args = a = args
        if a.num_chars is None:
            raise ValueError("num_chars is required")
        if a.attention_type != "original":
            raise NotImplementedError(f"attention_type={a.attention_type!r} (Graves, dynamic convolution) is {_EXCLUDED}")
        if not a.location_attn:
            raise NotImplementedError(f"location_attn=False is {_EXCLUDED}")
        if a.windowing:
            raise NotImplementedError(f"windowing=True is {_EXCLUDED}")
        if a.use_forward_attn or a.transition_agent:
            raise NotImplementedError(f"use_forward_attn / transition_agent are {_EXCLUDED}")
        if a.prenet_type != "original":
            raise NotImplementedError(f"prenet_type={a.prenet_type!r} is {_EXCLUDED}")
        if a.prenet_dropout_at_inference:
            raise NotImplementedError(f"prenet_dropout_at_inference=True is {_EXCLUDED}")
        if a.use_gst:
            raise NotImplementedError(f"GST (use_gst=True) is {_EXCLUDED}")
        if a.use_capacitron_vae:
            raise NotImplementedError(f"Capacitron (use_capacitron_vae=True) is {_EXCLUDED}")
        if a.attention_norm not in ("sigmoid", "softmax"):
            raise ValueError(f"attention_norm={a.attention_norm!r}: must be 'sigmoid' or 'softmax'")
        if a.use_speaker_embedding and a.use_d_vector_file:
            raise ValueError("use_speaker_embedding and use_d_vector_file exclude each other")
        mode = _nat.default_math_mode() if math_mode is None else math_mode
        if mode not in _nat.MATH_MODES:
            raise ValueError(f"math_mode must be one of {sorted(_nat.MATH_MODES)}")
        self.math_mode = mode
        self.chunk = int(chunk)
        self.stop_threshold = float(a.stop_threshold)
        self.max_decoder_steps = int(a.max_decoder_steps)
        self.embedded_speaker_dim = a.speaker_embedding_dim if a.use_speaker_embedding else \
            (a.d_vector_dim if a.use_d_vector_file else 0)
        E = a.encoder_dim
        D = E + self.embedded_speaker_dim
        self.embedding = nn.Embedding(a.num_chars, E, padding_idx=0)
        self.encoder = Encoder(E)
        self.decoder = Decoder(D, a.out_channels, a.r, a.query_dim, a.prenet_dim, a.attention_dim, a.location_filters,
                               a.location_kernel_size)
        self.postnet = Postnet(a.out_channels)
        if a.use_speaker_embedding:
            self.speaker_embedding = nn.Embedding(a.num_speakers, a.speaker_embedding_dim)
            self.speaker_embedding.weight.data.normal_(0, 0.3)
        c = _nat.TtsTacotron2Cfg()
        c.num_chars, c.out_channels, c.r = a.num_chars, a.out_channels, a.r
        c.encoder_dim, c.query_dim, c.prenet_dim, c.attention_dim = E, a.query_dim, a.prenet_dim, a.attention_dim
        c.location_filters, c.location_kernel_size = a.location_filters, a.location_kernel_size
        c.attention_norm = 1 if a.attention_norm == "softmax" else 0
        c.embed_dim = self.embedded_speaker_dim
        c.num_speakers = a.num_speakers if a.use_speaker_embedding else 0
        c.chunk = self.chunk
        c.math_mode = _nat.MATH_MODES[mode]
        self._cfg = c
        self._handle = None
        self._handle_key = None
        n = _nat.lib().tts_tacotron2_num_weights(ctypes.byref(c))
        if n < 0:
            _nat.check("tts_tacotron2_num_weights", -n)

    # ------------------------------------------------------------------ native handle
    def _weight_list(self) -> List[np.ndarray]:
        def conv_bn(b: ConvBNBlock):
            bn = b.batch_normalization
            return [_f32(t) for t in (b.convolution1d.weight, b.convolution1d.bias, bn.weight, bn.bias, bn.running_mean,
                                      bn.running_var)]

        def cell(m):
            return [_f32(t) for t in (m.weight_ih, m.weight_hh, m.bias_ih, m.bias_hh)]

        ws: List[np.ndarray] = [_f32(self.embedding.weight)]
        for b in self.encoder.convolutions:
            ws.extend(conv_bn(b))
        L = self.encoder.lstm
        for sfx in ("", "_reverse"):
            ws.extend(_f32(getattr(L, n + "_l0" + sfx)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        d = self.decoder
        ws.extend(_f32(l.linear_layer.weight) for l in d.prenet.linear_layers)
        ws.extend(cell(d.attention_rnn))
        at = d.attention
        ws.extend([_f32(at.query_layer.linear_layer.weight), _f32(at.inputs_layer.linear_layer.weight),
                   _f32(at.v.linear_layer.weight).reshape(-1), _f32(at.v.linear_layer.bias),
                   _f32(at.location_layer.location_conv1d.weight),
                   _f32(at.location_layer.location_dense.linear_layer.weight)])
        ws.extend(cell(d.decoder_rnn))
        ws.extend([_f32(d.linear_projection.linear_layer.weight), _f32(d.linear_projection.linear_layer.bias),
                   _f32(d.stopnet[1].linear_layer.weight).reshape(-1), _f32(d.stopnet[1].linear_layer.bias)])
        for b in self.postnet.convolutions:
            ws.extend(conv_bn(b))
        if hasattr(self, "speaker_embedding"):
            ws.append(_f32(self.speaker_embedding.weight))
        return ws

    def _device(self) -> torch.device:
        dev = self.embedding.weight.device
        if dev.type != "cuda":
            raise RuntimeError("Tacotron2 (tts_amd) runs only on a ROCm device: move it with .to('cuda') first "
                               "(there is no CPU fallback)")
        return dev

    def _native_handle(self):
        self._cfg.chunk = int(self.chunk)
        key = (self._cfg.chunk,) + tuple((p.data_ptr(), p._version, p.device)
                                         for p in list(self.parameters()) + list(self.buffers()))
        if self._handle is not None and key == self._handle_key:
            return self._handle
        self._release()
        dev = self._device()
        ws = self._weight_list()
        lib = _nat.lib()
        for i, w in enumerate(ws):
            n = lib.tts_tacotron2_weight_numel(ctypes.byref(self._cfg), i)
            if n != w.size:
                raise ValueError(f"weight {i} has {w.size} elements, expected {n}")
        arr = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        h = ctypes.c_void_p()
        _nat.call("tts_tacotron2_create", ctypes.byref(self._cfg), arr, dev.index or 0, ctypes.byref(h))
        self._handle, self._handle_key = h, key
        return h

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            _nat.lib().tts_tacotron2_destroy(self._handle)
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
        # torch's embedding raises on an id outside the table; the library would read the padding row
        if tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= self.args.num_chars):
            raise IndexError(f"token ids must lie in [0, {self.args.num_chars})")
        spk = dvec = None
        if hasattr(self, "speaker_embedding"):
            spk = aux.get("speaker_ids")
            if spk is None:
                raise ValueError("this model has a speaker embedding: pass aux_input['speaker_ids']")
            spk = torch.as_tensor(spk).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            if spk.shape != (B,):
                raise ValueError(f"speaker_ids must be [{B}], got {tuple(spk.shape)}")
            if int(spk.min()) < 0 or int(spk.max()) >= self.args.num_speakers:
                raise IndexError(f"speaker ids must lie in [0, {self.args.num_speakers})")
        elif self.args.use_d_vector_file:
            dvec = aux.get("d_vectors")
            if dvec is None:
                raise ValueError("this model takes d-vectors: pass aux_input['d_vectors']")
            dvec = torch.as_tensor(dvec).to(device=dev, dtype=torch.float32).reshape(B, -1).contiguous()
            if dvec.shape != (B, self.args.d_vector_dim):
                raise ValueError(f"d_vectors must be [{B}, {self.args.d_vector_dim}], got {tuple(dvec.shape)}")
        lens = aux.get("x_lengths")
        if lens is not None:
            lens = torch.as_tensor(lens).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            if lens.shape != (B,):
                raise ValueError(f"x_lengths must be [{B}], got {tuple(lens.shape)}")
        return dev, tok, lens, spk, dvec

    @torch.no_grad()
    def encode(self, x, aux_input=None):
        """The encoder alone: (inputs [B, T_en, D], processed_inputs [B, A, T_en])."""
        h = self._native_handle()
        dev, tok, lens, spk, dvec = self._inputs(x, aux_input)
        B, T = tok.shape
        D = self.args.encoder_dim + self.embedded_speaker_dim
        inputs = torch.empty(B, T, D, device=dev, dtype=torch.float32)
        pinp = torch.empty(B, self.args.attention_dim, T, device=dev, dtype=torch.float32)
        _nat.call("tts_tacotron2_encode", h, _nat.ptr(tok), _nat.ptr(lens), _nat.ptr(spk), _nat.ptr(dvec), B, T,
                  _nat.ptr(inputs), _nat.ptr(pinp), _nat.stream_ptr(dev))
        return inputs, pinp

    def _run(self, x, aux_input, profile: bool = False):
        h = self._native_handle()
        dev, tok, lens, spk, dvec = self._inputs(x, aux_input)
        B, T = tok.shape
        a = self.args
        S, Cr = int(self.max_decoder_steps), a.out_channels * a.r
        f = dict(device=dev, dtype=torch.float32)
        stream = _nat.stream_ptr(dev)
        inputs = torch.empty(B, T, a.encoder_dim + self.embedded_speaker_dim, **f)
        pinp = torch.empty(B, a.attention_dim, T, **f)
        _nat.call("tts_tacotron2_encode", h, _nat.ptr(tok), _nat.ptr(lens), _nat.ptr(spk), _nat.ptr(dvec), B, T,
                  _nat.ptr(inputs), _nat.ptr(pinp), stream)
        S = max(S, 0)  # max_decoder_steps < 1: the library's error
        dec = torch.empty(B, S, Cr, **f)
        align = torch.empty(B, S, T, **f)
        stop = torch.empty(B, S, **f)
        steps = torch.empty(B, dtype=torch.int32, device=dev)
        n = ctypes.c_int(0)
        rows: List[Dict] = []
        args = (h, _nat.ptr(inputs), _nat.ptr(pinp), _nat.ptr(lens), B, T, S, float(self.stop_threshold), _nat.ptr(dec),
                _nat.ptr(align), _nat.ptr(stop), _nat.ptr(steps), ctypes.byref(n), stream)
        if profile:
            cap = 8192
            recs = (_nat.TtsLaunchRecord * cap)()
            nr = ctypes.c_int(0)
            _nat.call("tts_tacotron2_decode_profiled", *args, recs, cap, ctypes.byref(nr))
            rows.extend({"name": recs[i].name.decode(), "flops": recs[i].flops, "bytes": recs[i].bytes,
                         "ms": recs[i].ms} for i in range(min(nr.value, cap)))
        else:
            _nat.call("tts_tacotron2_decode", *args)
        n = n.value
        out = torch.empty(B, n * a.r, a.out_channels, **f)
        _nat.call("tts_tacotron2_postnet", h, _nat.ptr(dec), _nat.ptr(steps), B, n, S, _nat.ptr(out), stream)
        outputs = {"model_outputs": out, "decoder_outputs": dec[:, :n].reshape(B, n * a.r, a.out_channels),
                   "alignments": align[:, :n], "stop_tokens": stop[:, :n], "y_lengths": steps.to(torch.int64) * a.r}
        return outputs, rows

    @torch.no_grad()
    def inference(self, x, aux_input=None):
        """tacotron2.py inference: x [B, T_en] token ids -> {"model_outputs" [B, steps r, C], "decoder_outputs"
        [B, steps r, C], "alignments" [B, steps, T_en], "stop_tokens" [B, steps], "y_lengths" [B]}, trimmed to
        the longest utterance's steps; rows past an utterance's own end are zero.  ``aux_input``:
        ``speaker_ids`` / ``d_vectors`` and the extension ``x_lengths`` (module docstring)."""
        return self._run(x, aux_input)[0]

    @torch.no_grad()
    def profile(self, x, aux_input=None):
        """One inference with a hipEvent pair around every decoder launch: (outputs, [{name, flops, bytes, ms}])."""
        return self._run(x, aux_input, profile=True)

    def load_checkpoint(self, config, checkpoint_path, eval=True, cache=False):
        state = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        state = state["model"] if "model" in state else state
        self.load_state_dict({k: v for k, v in state.items() if not k.startswith("coarse_decoder.")})
        if eval:
            self.eval()
            assert not self.training


__all__ = ["Tacotron2", "Tacotron2Args", "lstm_cell"]
