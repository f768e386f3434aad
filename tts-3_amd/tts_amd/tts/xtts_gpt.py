"""XTTS on the MI355X path: the autoregressive GPT-2 trunk ``XttsGPT`` (``TTS/tts/layers/xtts/gpt.py``,
``gpt_inference.py``) and ``Xtts`` (``TTS/tts/models/xtts.py``: ``inference``), which chains it with the
``HifiDecoder``.

``XttsGPT`` has the parameter tree of the ``gpt.*`` slice of an XTTS checkpoint (``text_embedding``,
``mel_embedding``, ``text_pos_embedding.emb``, ``mel_pos_embedding.emb``, ``gpt.h.{i}`` with the HF GPT-2
names and ``Conv1D`` weights stored ``[in][out]``, ``gpt.ln_f``, ``final_norm``, ``text_head``, ``mel_head``)
and runs ``generate`` (text tokens + conditioning latents -> audio codes) and ``forward(...,
return_latent=True)`` (codes -> the decoder's latents) through ``tts_xtts_gpt_*``.  The conditioning
latents are an input, as they are for the reference's ``Xtts.inference``; ``Xtts.get_conditioning_latents``
computes them from reference clips with an ``XttsConditioning`` (``xtts_cond.py``).  The tokenizer, beam
search, ``inference_stream``, audio file loading and training stay out.

Sampling draws by inverse CDF from uniforms ``torch.rand(B, max_new_tokens, generator=generator)``: the
reference's distribution, not ``torch.multinomial``'s stream of draws.  Extensions to the reference's
batch of one: ``text_lengths`` (ragged batches; utterance b is bitwise its own batch of one).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from .. import _native as _nat
from ..synthesizer import mel_handoff
from .xtts_decoder import HifiDecoder

_EXCLUDED = "not implemented on the device (DESIGN.md section 8)"


def _f32(t: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())


def causal_multi_head_attention(qkv: torch.Tensor, num_heads: int, key_lengths: Optional[torch.Tensor] = None,
                                math_mode: Optional[str] = None) -> torch.Tensor:
    """``multi_head_attention`` with a causal mask (``tts_op_mha_causal``): ``qkv`` [B, 3E, T] (rows q | k | v)
    -> [B, E, T], query i attending to the keys j <= i below ``key_lengths[b]``.  Head sizes 32, 64, 128."""
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
    _nat.call("tts_op_mha_causal", _nat.ptr(qkv), _nat.ptr(kl), B, E3 // 3, num_heads, T, _nat.MATH_MODES[mode],
              _nat.ptr(out), _nat.stream_ptr(dev))
    return out


class Conv1D(nn.Module):
    """HF GPT-2's ``Conv1D``: ``y = x @ weight + bias`` with ``weight [in][out]`` (the transpose of
    ``nn.Linear``); the library takes it as stored."""

    def __init__(self, nf: int, nx: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(nx, nf).normal_(std=0.02))
        self.bias = nn.Parameter(torch.zeros(nf))


class _Attention(nn.Module):
    def __init__(self, E: int):
        super().__init__()
        self.c_attn = Conv1D(3 * E, E)
        self.c_proj = Conv1D(E, E)


class _MLP(nn.Module):
    def __init__(self, E: int):
        super().__init__()
        self.c_fc = Conv1D(4 * E, E)
        self.c_proj = Conv1D(E, 4 * E)


class _Block(nn.Module):
    def __init__(self, E: int):
        super().__init__()
        self.ln_1 = nn.LayerNorm(E, eps=1e-5)
        self.attn = _Attention(E)
        self.ln_2 = nn.LayerNorm(E, eps=1e-5)
        self.mlp = _MLP(E)


class _Trunk(nn.Module):
    def __init__(self, layers: int, E: int):
        super().__init__()
        self.h = nn.ModuleList([_Block(E) for _ in range(layers)])
        self.ln_f = nn.LayerNorm(E, eps=1e-5)


class LearnedPositionEmbeddings(nn.Module):
    def __init__(self, seq_len: int, model_dim: int, init: float = 0.02):
        super().__init__()
        self.emb = nn.Embedding(seq_len, model_dim)
        self.emb.weight.data.normal_(mean=0.0, std=init)


_DROPPED_PREFIXES = ("conditioning_encoder.", "conditioning_perceiver.", "gpt_inference.")


def gpt_checkpoint_filter(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The keys of a ``gpt.*`` checkpoint slice this module loads: without the conditioning encoder /
    perceiver, the ``gpt_inference.*`` duplicates, HF's ``attn.bias`` / ``attn.masked_bias`` buffers and
    the ``*_layer_pos_embedding`` keys."""
    out = {}
    for k, v in state.items():
        if k.startswith(_DROPPED_PREFIXES) or "_layer_pos_embedding" in k:
            continue
        if k.startswith("gpt.h.") and (k.endswith(".attn.bias") or k.endswith(".attn.masked_bias")):
            continue
        out[k] = v
    return out


class XttsGPT(nn.Module):
    def __init__(
        self,
        start_text_token=261,
        stop_text_token=0,
        layers=8,
        model_dim=512,
        heads=8,
        max_text_tokens=120,
        max_mel_tokens=250,
        max_prompt_tokens=70,
        max_conditioning_inputs=1,
        code_stride_len=1024,
        number_text_tokens=256,
        num_audio_tokens=8194,
        start_audio_token=8192,
        stop_audio_token=8193,
        train_solo_embeddings=False,
        checkpointing=False,
        average_conditioning_embeddings=False,
        label_smoothing=0.0,
        use_perceiver_resampler=False,
        perceiver_cond_length_compression=256,
        math_mode: Optional[str] = None,
        chunk: int = 32,
    ):
        super().__init__()
        if train_solo_embeddings:
            raise NotImplementedError(f"train_solo_embeddings=True is {_EXCLUDED}")
        mode = _nat.default_math_mode() if math_mode is None else math_mode
        if mode not in _nat.MATH_MODES:
            raise ValueError(f"math_mode must be one of {sorted(_nat.MATH_MODES)}")
        self.math_mode = mode
        self.chunk = int(chunk)
        self.layers, self.model_dim, self.heads = int(layers), int(model_dim), int(heads)
        self.number_text_tokens, self.num_audio_tokens = int(number_text_tokens), int(num_audio_tokens)
        self.start_text_token = int(number_text_tokens if start_text_token is None else start_text_token)
        self.stop_text_token = int(stop_text_token)
        self.start_audio_token, self.stop_audio_token = int(start_audio_token), int(stop_audio_token)
        self.max_text_tokens, self.max_mel_tokens = int(max_text_tokens), int(max_mel_tokens)
        self.max_prompt_tokens = int(max_prompt_tokens)
        self.max_conditioning_inputs = int(max_conditioning_inputs)
        self.code_stride_len = int(code_stride_len)
        E = self.model_dim
        self.text_embedding = nn.Embedding(self.number_text_tokens, E)
        self.mel_embedding = nn.Embedding(self.num_audio_tokens, E)
        self.text_pos_embedding = LearnedPositionEmbeddings(self.max_text_tokens + 2, E)
        self.mel_pos_embedding = LearnedPositionEmbeddings(self.max_mel_tokens + 2 + self.max_conditioning_inputs, E)
        self.gpt = _Trunk(self.layers, E)
        self.final_norm = nn.LayerNorm(E, eps=1e-5)
        self.text_head = nn.Linear(E, self.number_text_tokens)  # loaded (strict tree), unused by inference
        self.mel_head = nn.Linear(E, self.num_audio_tokens)
        self._handle = None
        self._handle_key = None
        c = self._make_cfg(0)
        n = _nat.lib().tts_xtts_gpt_num_weights(ctypes.byref(c))
        if n < 0:
            _nat.check("tts_xtts_gpt_num_weights", -n)

    # ------------------------------------------------------------------ native handle
    def _make_cfg(self, prompt_rows: int) -> "_nat.TtsXttsGptCfg":
        c = _nat.TtsXttsGptCfg()
        c.layers, c.model_dim, c.heads = self.layers, self.model_dim, self.heads
        c.n_text_tokens, c.n_audio_tokens = self.number_text_tokens, self.num_audio_tokens
        c.start_text_token, c.stop_text_token = self.start_text_token, self.stop_text_token
        c.start_audio_token, c.stop_audio_token = self.start_audio_token, self.stop_audio_token
        c.text_positions = self.max_text_tokens + 2
        c.mel_positions = self.max_mel_tokens + 2 + self.max_conditioning_inputs
        c.prompt_positions = int(prompt_rows)
        c.chunk = int(self.chunk)
        c.math_mode = _nat.MATH_MODES[self.math_mode]
        return c

    def _weight_list(self) -> List[np.ndarray]:
        ws = [_f32(self.text_embedding.weight), _f32(self.mel_embedding.weight),
              _f32(self.text_pos_embedding.emb.weight), _f32(self.mel_pos_embedding.emb.weight)]
        for b in self.gpt.h:
            # the Conv1D weights go as stored, [in][out]: the packer reads them in that layout
            ws.extend(_f32(t) for t in (b.ln_1.weight, b.ln_1.bias, b.attn.c_attn.weight, b.attn.c_attn.bias,
                                        b.attn.c_proj.weight, b.attn.c_proj.bias, b.ln_2.weight, b.ln_2.bias,
                                        b.mlp.c_fc.weight, b.mlp.c_fc.bias, b.mlp.c_proj.weight, b.mlp.c_proj.bias))
        ws.extend(_f32(t) for t in (self.gpt.ln_f.weight, self.gpt.ln_f.bias, self.final_norm.weight,
                                    self.final_norm.bias, self.mel_head.weight, self.mel_head.bias))
        return ws

    def _device(self) -> torch.device:
        dev = self.mel_embedding.weight.device
        if dev.type != "cuda":
            raise RuntimeError("XttsGPT (tts_amd) runs only on a ROCm device: move it with .to('cuda') first "
                               "(there is no CPU fallback)")
        return dev

    def _native_handle(self, prompt_rows: int):
        key = (int(self.chunk), int(prompt_rows)) + tuple((p.data_ptr(), p._version, p.device)
                                                          for p in self.parameters())
        if self._handle is not None and key == self._handle_key:
            return self._handle
        self._release()
        dev = self._device()
        cfg = self._make_cfg(prompt_rows)
        ws = self._weight_list()
        lib = _nat.lib()
        n = lib.tts_xtts_gpt_num_weights(ctypes.byref(cfg))
        if n < 0:
            _nat.check("tts_xtts_gpt_num_weights", -n)
        if n != len(ws):
            raise ValueError(f"{len(ws)} weights, the library expects {n}")
        for i, w in enumerate(ws):
            n = lib.tts_xtts_gpt_weight_numel(ctypes.byref(cfg), i)
            if n != w.size:
                raise ValueError(f"weight {i} has {w.size} elements, expected {n}")
        arr = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        h = ctypes.c_void_p()
        _nat.call("tts_xtts_gpt_create", ctypes.byref(cfg), arr, dev.index or 0, ctypes.byref(h))
        self._handle, self._handle_key = h, key
        return h

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            _nat.lib().tts_xtts_gpt_destroy(self._handle)
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
    def _prefix(self, cond_latents, text_inputs, text_lengths):
        tok = torch.as_tensor(text_inputs)
        if tok.dim() == 1:
            tok = tok.unsqueeze(0)
        if tok.dim() != 2:
            raise ValueError(f"text_inputs must be [B, T] token ids, got shape {tuple(tok.shape)}")
        # torch's embedding raises on an id outside the table; the library would clamp it
        if tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= self.number_text_tokens):
            raise IndexError(f"text token ids must lie in [0, {self.number_text_tokens})")
        dev = self._device()
        tok = tok.to(device=dev, dtype=torch.int64).contiguous()
        B, T = tok.shape
        cond = torch.as_tensor(cond_latents).to(device=dev, dtype=torch.float32)
        if cond.dim() == 2:
            cond = cond.unsqueeze(0)
        if cond.dim() != 3 or cond.shape[0] != B or cond.shape[2] != self.model_dim:
            raise ValueError(f"cond_latents must be [{B}, P, {self.model_dim}], got {tuple(cond.shape)}")
        cond = cond.contiguous()
        lens = None
        if text_lengths is not None:
            lens = torch.as_tensor(text_lengths).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            if lens.shape != (B,):
                raise ValueError(f"text_lengths must be [{B}], got {tuple(lens.shape)}")
            if int(lens.min()) < 0 or int(lens.max()) > T:
                raise ValueError(f"text_lengths must lie in [0, {T}]")
        return dev, cond, tok, lens

    def _prefill(self, h, dev, cond, tok, lens, max_new: int, rows: Optional[List[Dict]] = None):
        B, T = tok.shape
        args = (h, _nat.ptr(cond), _nat.ptr(tok), _nat.ptr(lens), B, T, int(max_new), _nat.stream_ptr(dev))
        if rows is None:
            _nat.call("tts_xtts_gpt_prefill", *args)
        else:
            rows.extend(_profiled("tts_xtts_gpt_prefill_profiled", args))

    @torch.no_grad()
    def _generate(self, cond_latents, text_inputs, do_sample=True, top_k=50, top_p=0.85, temperature=0.75,
                  repetition_penalty=10.0, max_new_tokens=None, generator=None, text_lengths=None, uniforms=None,
                  return_logits=False, return_latents=False, profile=False) -> Dict:
        dev, cond, tok, lens = self._prefix(cond_latents, text_inputs, text_lengths)
        B = tok.shape[0]
        S = int(self.max_mel_tokens if max_new_tokens is None else max_new_tokens)
        h = self._native_handle(cond.shape[1])
        rows: Optional[List[Dict]] = [] if profile else None
        self._prefill(h, dev, cond, tok, lens, S, rows)  # refuses S < 1
        u = None
        if do_sample:
            if uniforms is not None:
                u = torch.as_tensor(uniforms).to(device=dev, dtype=torch.float32).reshape(B, S).contiguous()
            else:
                u = torch.rand(B, S, generator=generator, device=generator.device if generator is not None else dev)
                u = u.to(device=dev, dtype=torch.float32).contiguous()
        codes = torch.empty(B, S, dtype=torch.int32, device=dev)
        n = torch.empty(B, dtype=torch.int32, device=dev)
        logits = torch.empty(B, S, self.num_audio_tokens, device=dev) if return_logits else None
        lat = torch.empty(B, S, self.model_dim, device=dev) if return_latents else None
        ran = ctypes.c_int(0)
        args = (h, S, float(repetition_penalty), float(temperature), int(top_k), float(top_p), _nat.ptr(u),
                _nat.ptr(codes), _nat.ptr(n), _nat.ptr(logits), _nat.ptr(lat), ctypes.byref(ran), _nat.stream_ptr(dev))
        if profile:
            rows.extend(_profiled("tts_xtts_gpt_generate_profiled", args))
        else:
            _nat.call("tts_xtts_gpt_generate", *args)
        return {"codes": codes, "lengths": n, "logits": logits, "latents": lat, "steps_run": ran.value, "profile": rows}

    def generate(self, cond_latents, text_inputs, do_sample=True, top_k=50, top_p=0.85, temperature=0.75,
                 repetition_penalty=10.0, max_new_tokens=None, generator=None, text_lengths=None, num_beams=1,
                 input_tokens=None, return_attentions=False, **hf_generate_kwargs):
        """gpt.py ``generate``: audio codes [B, n] int64, trimmed to the longest utterance's n_b (its stop
        token included); codes past an utterance's own end are ``stop_audio_token`` (HF's pad)."""
        if num_beams is not None and int(num_beams) > 1:
            raise NotImplementedError(f"num_beams > 1 (beam search, length_penalty) is {_EXCLUDED}")
        if input_tokens is not None:
            raise NotImplementedError(f"input_tokens (a forced audio prefix) is {_EXCLUDED}")
        if return_attentions or hf_generate_kwargs.get("output_attentions"):
            raise NotImplementedError(f"return_attentions is {_EXCLUDED}")
        out = self._generate(cond_latents, text_inputs, do_sample=do_sample, top_k=top_k, top_p=top_p,
                             temperature=temperature, repetition_penalty=repetition_penalty,
                             max_new_tokens=max_new_tokens, generator=generator, text_lengths=text_lengths)
        n = int(out["lengths"].max())
        return out["codes"][:, :n].to(torch.int64)

    @torch.no_grad()
    def forward(self, text_inputs, text_lengths, audio_codes, wav_lengths, cond_mels=None, cond_idxs=None,
                cond_lens=None, cond_latents=None, return_attentions=False, return_latent=True, code_lengths=None,
                return_logits=False):
        """gpt.py ``forward(..., return_latent=True)``: the teacher-forced pass over ``[cond | start_text,
        text, stop_text | start_audio, codes, stop_audio]``; returns ``final_norm(ln_f(h))`` at the mel
        positions without the last 4, ``[B, max(n_b) - 2, E]`` with zero rows at or past ``n_b - 2``.
        ``n_b = ceil(wav_lengths / code_stride_len)`` (or ``code_lengths``, an extension).  ``text_lengths``
        may be None (every token valid)."""
        if return_attentions:
            raise NotImplementedError(f"return_attentions is {_EXCLUDED}")
        if not return_latent:
            raise NotImplementedError(f"forward without return_latent (the training losses) is {_EXCLUDED}")
        if cond_mels is not None:
            raise NotImplementedError(f"cond_mels (the conditioning encoder / perceiver) is {_EXCLUDED}: pass cond_latents")
        if cond_latents is None:
            raise ValueError("cond_latents is required")
        codes = torch.as_tensor(audio_codes)
        if codes.dim() == 1:
            codes = codes.unsqueeze(0)
        if codes.dim() != 2 or codes.shape[1] < 1:
            raise ValueError(f"audio_codes must be [B, S], got {tuple(codes.shape)}")
        if int(codes.min()) < 0 or int(codes.max()) >= self.num_audio_tokens:
            raise IndexError(f"audio codes must lie in [0, {self.num_audio_tokens})")
        dev, cond, tok, lens = self._prefix(cond_latents, text_inputs, text_lengths)
        B = tok.shape[0]
        if codes.shape[0] != B:
            raise ValueError(f"audio_codes must be [{B}, S], got {tuple(codes.shape)}")
        codes = codes.to(device=dev, dtype=torch.int32).contiguous()
        S = codes.shape[1]
        if code_lengths is None:
            if wav_lengths is None:
                raise ValueError("wav_lengths (or code_lengths) is required")
            wl = torch.as_tensor(wav_lengths).to(torch.float64).reshape(-1).cpu()
            code_lengths = torch.ceil(wl / self.code_stride_len).to(torch.int64)
        n = torch.as_tensor(code_lengths).to(torch.int64).reshape(-1).cpu()
        if n.shape != (B,) or int(n.min()) < 0 or int(n.max()) > S:
            raise ValueError(f"code lengths must be [{B}] values in [0, {S}]")
        rows = int(n.max()) + 2 if return_logits else int(n.max()) - 2
        if rows < 1:
            raise ValueError("fewer than 3 codes: no latent row is left after the reference's trim of 4")
        h = self._native_handle(cond.shape[1])
        self._prefill(h, dev, cond, tok, lens, rows)
        nd = n.to(device=dev, dtype=torch.int32).contiguous()
        lat = torch.empty(B, rows, self.model_dim, device=dev)
        logits = torch.empty(B, rows, self.num_audio_tokens, device=dev) if return_logits else None
        _nat.call("tts_xtts_gpt_latents", h, _nat.ptr(codes), _nat.ptr(nd), S, rows, _nat.ptr(lat), _nat.ptr(logits),
                  _nat.stream_ptr(dev))
        if return_logits:
            return lat[:, : max(int(n.max()) - 2, 0)], logits
        return lat

    def load_checkpoint(self, checkpoint_path, eval=True, strict=True):
        """Loads the ``gpt.*`` slice of an XTTS checkpoint (or a bare GPT state dict), dropping the keys
        ``gpt_checkpoint_filter`` names."""
        state = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        state = state["model"] if "model" in state else state
        if any(k.startswith("gpt.gpt.") for k in state):
            state = {k[len("gpt."):]: v for k, v in state.items() if k.startswith("gpt.")}
        self.load_state_dict(gpt_checkpoint_filter(state), strict=strict)
        if eval:
            self.eval()


def _profiled(fn: str, args) -> List[Dict]:
    cap = 65536
    recs = (_nat.TtsLaunchRecord * cap)()
    nr = ctypes.c_int(0)
    _nat.call(fn, *args, recs, cap, ctypes.byref(nr))
    return [{"name": recs[i].name.decode(), "flops": recs[i].flops, "bytes": recs[i].bytes, "ms": recs[i].ms}
            for i in range(min(nr.value, cap))]


class Xtts(nn.Module):
    """``TTS/tts/models/xtts.py`` ``Xtts.inference`` on token ids: ``XttsGPT`` -> latents -> ``HifiDecoder``,
    and, with ``conditioning`` (an ``XttsConditioning``) and ``mel_stats`` (the checkpoint's buffer),
    ``get_conditioning_latents`` on reference clips that are already device tensors."""

    def __init__(self, gpt: XttsGPT, hifigan_decoder: HifiDecoder, gpt_max_new_tokens: Optional[int] = None,
                 conditioning=None, mel_stats: Optional[torch.Tensor] = None):
        super().__init__()
        self.gpt = gpt
        self.hifigan_decoder = hifigan_decoder
        self.gpt_max_new_tokens = gpt_max_new_tokens
        if conditioning is not None:  # opt-in: the default module tree is unchanged
            self.conditioning = conditioning
            stats = torch.ones(conditioning.spec_dim) if mel_stats is None else torch.as_tensor(mel_stats)
            self.register_buffer("mel_stats", stats.detach().to(torch.float32).reshape(-1).clone())

    # ------------------------------------------------------------------ voice cloning
    def _conditioning(self):
        cond = getattr(self, "conditioning", None)
        if cond is None:
            raise RuntimeError("this Xtts was built without its conditioning encoder / perceiver: pass "
                               "conditioning=XttsConditioning(...)")
        return cond

    @staticmethod
    def _clip(audio, what="audio") -> torch.Tensor:
        if isinstance(audio, (str, bytes)) or hasattr(audio, "__fspath__"):
            raise NotImplementedError(f"loading {what} from a file path is {_EXCLUDED}: pass the clip as a [1, N] tensor")
        _nat.require_device_tensor(audio, what)
        if audio.dim() == 1:
            audio = audio.unsqueeze(0)
        if audio.dim() != 2 or audio.shape[0] != 1 or audio.shape[1] < 1:
            raise ValueError(f"{what} must be a [1, N] tensor, got shape {tuple(audio.shape)}")
        return audio.to(torch.float32)

    @torch.no_grad()
    def get_gpt_cond_latents(self, audio, sr, length: int = 30, chunk_length: int = 6):
        """xtts.py ``get_gpt_cond_latents`` (the perceiver path): audio [1, N] at ``sr`` -> [1, num_latents, E],
        the mean over the clip's ``chunk_length``-second chunks of ``get_style_emb`` of their mels."""
        from ..audio import resample

        cond = self._conditioning()
        audio = self._clip(audio)
        if int(sr) != 22050:
            audio = resample(audio, int(sr), 22050)
        if length > 0:
            audio = audio[:, : 22050 * int(length)]
        step = 22050 * int(chunk_length)
        if step < 1:
            raise ValueError("chunk_length must be positive")
        total, n = None, 0
        for i in range(0, audio.shape[1], step):
            chunk = audio[:, i : i + step]
            if chunk.shape[-1] < 22050 * 0.33:  # the reference skips a too short last chunk
                continue
            mel = cond.wav_to_mel_cloning(chunk, self.mel_stats)
            emb = cond.get_style_emb(mel)
            total = emb if total is None else total + emb  # chunk order: one fixed order of the sum
            n += 1
        if n == 0:
            raise ValueError("the reference clip is shorter than 0.33 s: no chunk is left")
        return (total / n).transpose(1, 2)

    @torch.no_grad()
    def get_speaker_embedding(self, audio, sr):
        """xtts.py ``get_speaker_embedding``: audio [1, N] at ``sr`` -> [1, d_vector_dim, 1] (resampled to 16 kHz)."""
        from ..audio import resample

        if getattr(self.hifigan_decoder, "speaker_encoder", None) is None:
            raise RuntimeError("the HifiDecoder was built without its speaker encoder: pass with_speaker_encoder=True")
        audio_16k = resample(self._clip(audio), int(sr), 16000)
        return self.hifigan_decoder.speaker_embedding(audio_16k)

    @torch.no_grad()
    def get_conditioning_latents(self, audio_path, max_ref_length=30, gpt_cond_len=6, gpt_cond_chunk_len=6,
                                 librosa_trim_db=None, sound_norm_refs=False, load_sr=22050):
        """xtts.py ``get_conditioning_latents`` on clips that are already loaded: ``audio_path`` is a [1, N]
        device tensor at ``load_sr`` or a list of them (file loading and ``librosa_trim_db`` stay on the host).
        Returns ``(gpt_cond_latent [1, num_latents, E], speaker_embedding [1, d_vector_dim, 1])``."""
        if librosa_trim_db is not None:
            raise NotImplementedError(f"librosa_trim_db (trimming the reference clip) is {_EXCLUDED}")
        clips = audio_path if isinstance(audio_path, (list, tuple)) else [audio_path]
        if len(clips) == 0:
            raise ValueError("no reference clip")
        self._conditioning()
        audios, embs = [], []
        for clip in clips:
            audio = self._clip(clip, "audio_path")[:, : int(load_sr) * int(max_ref_length)]
            if sound_norm_refs:
                audio = (audio / torch.abs(audio).max()) * 0.75
            embs.append(self.get_speaker_embedding(audio, load_sr))
            audios.append(audio)
        full_audio = torch.cat(audios, dim=-1)
        gpt_cond_latents = self.get_gpt_cond_latents(full_audio, load_sr, length=gpt_cond_len,
                                                     chunk_length=gpt_cond_chunk_len)
        speaker_embedding = embs[0]
        for e in embs[1:]:
            speaker_embedding = speaker_embedding + e
        speaker_embedding = speaker_embedding / len(embs)
        return gpt_cond_latents, speaker_embedding

    @torch.no_grad()
    def inference(self, text_tokens, gpt_cond_latent, speaker_embedding, temperature=0.75, length_penalty=1.0,
                  repetition_penalty=10.0, top_k=50, top_p=0.85, do_sample=True, num_beams=1, length_scale=1.0,
                  generator=None, text_lengths=None, uniforms=None, **hf_generate_kwargs) -> Dict:
        """text_tokens [B, T] ids (the tokenizer is out of scope), gpt_cond_latent [B, P, E], speaker_embedding
        [B, d_vector_dim, 1] -> {"wav" [B, 1, n], "gpt_latents" [B, max(n_b) - 2, E], "speaker_embedding",
        and the extensions "gpt_codes" [B, max(n_b)] and "lengths" [B]}.  The latents are the hidden states the
        generation itself passed through (the reference recomputes the same values in a second pass)."""
        if num_beams is not None and int(num_beams) > 1:
            raise NotImplementedError(f"num_beams > 1 (beam search, length_penalty) is {_EXCLUDED}")
        if hf_generate_kwargs.get("input_tokens") is not None:
            raise NotImplementedError(f"input_tokens (a forced audio prefix) is {_EXCLUDED}")
        out = self.gpt._generate(gpt_cond_latent, text_tokens, do_sample=do_sample, top_k=top_k, top_p=top_p,
                                 temperature=temperature, repetition_penalty=repetition_penalty,
                                 max_new_tokens=self.gpt_max_new_tokens, generator=generator,
                                 text_lengths=text_lengths, uniforms=uniforms, return_latents=True)
        n = out["lengths"].to(torch.int64)
        nmax = int(n.max())
        if nmax < 3:
            raise ValueError("the GPT ended after fewer than 3 codes: no latent row is left")
        lat = out["latents"][:, : nmax - 2]
        keep = torch.arange(nmax - 2, device=lat.device)[None, :] < (n - 2)[:, None]
        lat = (lat * keep[:, :, None]).contiguous()
        if float(length_scale) != 1.0:
            lat = mel_handoff(lat, None, None, time_major=True, scale_factor=float(length_scale))
            lat = lat.transpose(1, 2).contiguous()
        g = speaker_embedding.to(device=lat.device, dtype=torch.float32)
        wav = self.hifigan_decoder(lat, g=g)
        return {"wav": wav, "gpt_latents": lat, "speaker_embedding": speaker_embedding,
                "gpt_codes": out["codes"][:, :nmax].to(torch.int64), "lengths": n}


__all__ = ["Conv1D", "LearnedPositionEmbeddings", "Xtts", "XttsGPT", "causal_multi_head_attention",
           "gpt_checkpoint_filter"]
