"""Acoustic-model surface: the Glow-TTS ``Encoder`` / ``Decoder`` (both directions) /
``GlowTTS.inference`` / ``GlowTTS.decoder_inference`` / ``GlowTTS.forward`` / ``GlowTTS.inference_with_MAS``
with ``maximum_path`` (Monotonic Alignment Search), and the VITS ``ResidualCouplingBlocks`` flow
(both directions), ``PosteriorEncoder``, the linear spectrogram ``wav_to_spec`` and ``Vits``
(``inference``, ``voice_conversion``, ``inference_voice_conversion``) with its text side
(``TextEncoder``, ``StochasticDurationPredictor``), and ``ForwardTTS`` (FastPitch / FastSpeech:
``inference``) with the self-attention of its ``FFTransformer`` layers, ``multi_head_attention``, and
``Tacotron2`` (``inference``: recurrent decoder with location-sensitive attention) with its ``lstm_cell``
step, and XTTS (``XttsGPT``: the autoregressive GPT-2 trunk with its KV cache, ``Xtts.inference`` with the
``HifiDecoder``, and ``XttsConditioning``: the conditioning encoder and perceiver resampler behind
``Xtts.get_conditioning_latents``), on MI355X."""
from .forward_tts import ForwardTTS, ForwardTTSArgs, multi_head_attention
from .glow_decoder import Decoder
from .glow_tts import Encoder, GlowTTS
from .helpers import maximum_path
from .tacotron2 import Tacotron2, Tacotron2Args, lstm_cell
from .spectrogram import wav_to_spec, wav_to_spec_profile
from .vits_flow import PosteriorEncoder, ResidualCouplingBlocks
from .vits_text import DurationPredictor, StochasticDurationPredictor, TextEncoder, Vits
from .xtts_decoder import HifiDecoder
from .xtts_cond import XttsConditioning
from .xtts_gpt import Xtts, XttsGPT

__all__ = ["Decoder", "DurationPredictor", "Encoder", "ForwardTTS", "ForwardTTSArgs", "GlowTTS", "HifiDecoder", "PosteriorEncoder", "ResidualCouplingBlocks",
           "StochasticDurationPredictor", "Tacotron2", "Tacotron2Args", "TextEncoder", "Vits", "Xtts", "XttsConditioning", "XttsGPT", "lstm_cell", "maximum_path",
           "multi_head_attention", "wav_to_spec", "wav_to_spec_profile"]
