"""Cases of the speaker-encoder tests: seeded synthetic weights (tts_amd.synthetic's recipe: conv
N(0, 2 / fan_in), linear N(0, 1 / in), BatchNorm gain / variance U(0.8, 1.2), shifts, means and biases
0.1 N(0, 1), every bn2's gain and shift times 0.5), the synthetic reference wavs
clamp(0.25 N(0, 1) + 0.2 sin(2 pi 440 t) + 0.3 sin(2 pi 70 t), -1, 1), and the fp64 oracle of each
case computed once."""
import functools

import torch

import _speaker_encoder_ref as R
from tts_amd import synthetic

SR = 16000
REF_AUDIO = dict(fft_size=512, win_length=400, hop_length=160, sample_rate=SR, preemphasis=0.97, num_mels=64)
SMALL_AUDIO = dict(REF_AUDIO, num_mels=16)

# name -> constructor arguments of ResNetSpeakerEncoder (without math_mode)
MODELS = {
    "ref": dict(input_dim=64, proj_dim=512, layers=[3, 4, 6, 3], num_filters=[32, 64, 128, 256], encoder_type="ASP",
                log_input=True, use_torch_spec=True, audio_config=REF_AUDIO),
    "small": dict(input_dim=16, proj_dim=64, layers=[2, 1, 1, 1], num_filters=[16, 32, 64, 128], encoder_type="ASP",
                  log_input=True, use_torch_spec=True, audio_config=SMALL_AUDIO),
    "small_sap": dict(input_dim=16, proj_dim=64, layers=[2, 1, 1, 1], num_filters=[16, 32, 64, 128], encoder_type="SAP",
                      log_input=True, use_torch_spec=True, audio_config=SMALL_AUDIO),
    "small_nolog": dict(input_dim=16, proj_dim=64, layers=[2, 1, 1, 1], num_filters=[16, 32, 64, 128], encoder_type="ASP",
                        log_input=False, use_torch_spec=True, audio_config=SMALL_AUDIO),
    "small_feat": dict(input_dim=16, proj_dim=64, layers=[2, 1, 1, 1], num_filters=[16, 32, 64, 128], encoder_type="ASP",
                       log_input=False, use_torch_spec=False, audio_config=None),
}
# (model, B, N): N samples of wav, or N frames of features for small_feat
RUNS = {
    "small": ("small", 3, 5920),
    "edge": ("small", 3, 1120),  # T' = 1: softmax over one column, every ASP variance at the clamp
    "ref": ("ref", 2, 16000),
    "small_sap": ("small_sap", 3, 5920),
    "small_nolog": ("small_nolog", 3, 5920),
    "small_feat": ("small_feat", 3, 38),
}


@functools.lru_cache(maxsize=None)
def state_dict(model: str):
    c = MODELS[model]
    return synthetic.speaker_encoder_state_dict(
        input_dim=c["input_dim"], proj_dim=c["proj_dim"], layers=tuple(c["layers"]), num_filters=tuple(c["num_filters"]),
        encoder_type=c["encoder_type"], use_torch_spec=c["use_torch_spec"], audio_config=c["audio_config"],
        seed=11 + len(model))


def wav(B: int, N: int, seed: int = 0) -> torch.Tensor:
    return synthetic.speaker_wav(B, N, SR, seed=seed)


@functools.lru_cache(maxsize=None)
def inputs(run: str) -> torch.Tensor:
    model, B, N = RUNS[run]
    if MODELS[model]["use_torch_spec"]:
        return wav(B, N, seed=N)
    # features: positive, like a mel power spectrogram
    g = torch.Generator().manual_seed(N)
    return torch.rand(B, MODELS[model]["input_dim"], N, generator=g) * 4.0 + 0.05


def ref_kwargs(model: str) -> dict:
    c = MODELS[model]
    return dict(layers=c["layers"], encoder_type=c["encoder_type"], log_input=c["log_input"],
                use_torch_spec=c["use_torch_spec"], audio_config=c["audio_config"])


@functools.lru_cache(maxsize=None)
def oracle(run: str, l2_norm: bool = False) -> torch.Tensor:
    """The fp64 embedding of a run (computed once per process)."""
    model = RUNS[run][0]
    return R.forward(state_dict(model), inputs(run), l2_norm=l2_norm, dtype=torch.float64, **ref_kwargs(model))


@functools.lru_cache(maxsize=None)
def oracle_features(model: str, B: int, N: int) -> torch.Tensor:
    c = MODELS[model]
    return R.features(state_dict(model), wav(B, N, seed=N), c["log_input"], True, c["audio_config"], torch.float64)
