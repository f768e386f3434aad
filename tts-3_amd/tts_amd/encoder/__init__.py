"""Speaker-encoder side of the MI355X path (``TTS/encoder``): the SE-ResNet d-vector model and the
Conv2d op of its trunk."""
from .ops import conv2d_3x3, conv2d_tile
from .resnet import XTTS_AUDIO_CONFIG, ResNetSpeakerEncoder, mel_filterbank, window_offsets

__all__ = ["ResNetSpeakerEncoder", "XTTS_AUDIO_CONFIG", "conv2d_3x3", "conv2d_tile", "mel_filterbank", "window_offsets"]
