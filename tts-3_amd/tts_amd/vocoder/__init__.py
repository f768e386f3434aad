"""Vocoder surface: ``HifiganGenerator``, the MelGAN family (``MelganGenerator``,
``FullbandMelganGenerator``, ``MultibandMelganGenerator`` and its ``PQMF``), ``GAN`` (inference part)
and ``setup_generator`` (``TTS/vocoder/models/__init__.py:34-41``)."""
from .fullband_melgan_generator import FullbandMelganGenerator
from .gan import GAN, setup_generator
from .hifigan_generator import HifiganGenerator
from .melgan_generator import MelganGenerator
from .multiband_melgan_generator import MultibandMelganGenerator
from .pqmf import PQMF

__all__ = ["GAN", "HifiganGenerator", "MelganGenerator", "FullbandMelganGenerator", "MultibandMelganGenerator",
           "PQMF", "setup_generator"]
