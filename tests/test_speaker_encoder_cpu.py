"""The speaker encoder without a device: the drop-in module's state-dict keys and shapes, the mel
filterbank, compute_embedding's windows, constructor and limit errors, the new C-ABI symbols, the
synthetic weights' recipe, and the opt-in HifiDecoder keyword."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _speaker_encoder_cases as SC
import _speaker_encoder_ref as R
from tts_amd import _native as N
from tts_amd import encoder, synthetic
from tts_amd.encoder import ResNetSpeakerEncoder
from tts_amd.tts.xtts_decoder import HifiDecoder

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tts_mi355x.h")
BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def expected_keys(input_dim, proj_dim, layers, filters, encoder_type, torch_spec, win=400, n_freqs=257):
    """The reference's state-dict keys and shapes, written out literally."""
    k = {"conv1.weight": (filters[0], 1, 3, 3), "conv1.bias": (filters[0],)}

    def bn(p, n):
        for s in BN:
            k[f"{p}.{s}"] = () if s == "num_batches_tracked" else (n,)

    bn("bn1", filters[0])
    cin = filters[0]
    for li in range(4):
        C = filters[li]
        for i in range(layers[li]):
            p = f"layer{li + 1}.{i}"
            k[p + ".conv1.weight"] = (C, cin, 3, 3)
            bn(p + ".bn1", C)
            k[p + ".conv2.weight"] = (C, C, 3, 3)
            bn(p + ".bn2", C)
            k[p + ".se.fc.0.weight"] = (C // 8, C)
            k[p + ".se.fc.0.bias"] = (C // 8,)
            k[p + ".se.fc.2.weight"] = (C, C // 8)
            k[p + ".se.fc.2.bias"] = (C,)
            if (li > 0 and i == 0) or cin != C:
                k[p + ".downsample.0.weight"] = (C, cin, 1, 1)
                bn(p + ".downsample.1", C)
            cin = C
    if torch_spec:
        k["torch_spec.0.filter"] = (1, 1, 2)
        k["torch_spec.1.spectrogram.window"] = (win,)
        k["torch_spec.1.mel_scale.fb"] = (n_freqs, input_dim)
    D = filters[3] * input_dim // 8
    k["attention.0.weight"] = (128, D, 1)
    k["attention.0.bias"] = (128,)
    bn("attention.2", 128)
    k["attention.3.weight"] = (D, 128, 1)
    k["attention.3.bias"] = (D,)
    k["fc.weight"] = (proj_dim, 2 * D if encoder_type == "ASP" else D)
    k["fc.bias"] = (proj_dim,)
    return k


@pytest.mark.parametrize("model", ["ref", "small", "small_sap", "small_feat"])
def test_state_dict_keys_and_shapes(model):
    c = SC.MODELS[model]
    m = ResNetSpeakerEncoder(**c)
    want = expected_keys(c["input_dim"], c["proj_dim"], c["layers"], c["num_filters"], c["encoder_type"], c["use_torch_spec"])
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    sd = SC.state_dict(model)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    m.load_state_dict(sd, strict=True)
    assert list(m.state_dict().keys()) == list(sd.keys())


def test_reference_widths_literal():
    m = ResNetSpeakerEncoder()
    sd = m.state_dict()
    assert sd["layer2.0.downsample.0.weight"].shape == (64, 32, 1, 1)
    assert "layer1.0.downsample.0.weight" not in sd and "layer2.1.downsample.0.weight" not in sd
    assert sd["layer4.2.se.fc.0.weight"].shape == (32, 256) and sd["attention.0.weight"].shape == (128, 2048, 1)
    assert sd["fc.weight"].shape == (512, 4096) and not any(k.startswith("torch_spec") for k in sd)
    assert len([k for k in sd if k.endswith("conv1.weight") or k.endswith("conv2.weight")]) == 33


def test_weight_inventory_matches_the_library():
    for model in ("ref", "small_sap", "small_feat"):
        m = ResNetSpeakerEncoder(**SC.MODELS[model])
        m.load_state_dict(SC.state_dict(model))
        ws = m._weight_list()
        lib = N.lib()
        assert lib.tts_speaker_encoder_num_weights(ctypes.byref(m._cfg)) == len(ws)
        for i, w in enumerate(ws):
            assert lib.tts_speaker_encoder_weight_numel(ctypes.byref(m._cfg), i) == w.size, (model, i)
        assert lib.tts_speaker_encoder_weight_numel(ctypes.byref(m._cfg), len(ws)) == -1


def test_filterbank_against_the_formula():
    """fb = max(0, min(down, up)) from the slopes between the mel points, in fp64."""
    n_freqs, sr, n_mels = 257, 16000, 64
    fb = encoder.mel_filterbank(n_freqs, sr, n_mels)
    assert fb.dtype == torch.float64 and fb.shape == (n_freqs, n_mels)
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)  # noqa: E731
    freqs = np.linspace(0, sr // 2, n_freqs)
    m_pts = np.linspace(hz2mel(0.0), hz2mel(sr / 2), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    want = np.zeros((n_freqs, n_mels))
    for m in range(n_mels):
        lo, ce, hi = f_pts[m], f_pts[m + 1], f_pts[m + 2]
        for i, f in enumerate(freqs):
            want[i, m] = max(0.0, min((f - lo) / (ce - lo), (hi - f) / (hi - ce)))
    assert np.abs(fb.numpy() - want).max() < 1e-12
    assert np.abs(R.mel_filterbank(n_freqs, sr, n_mels).numpy() - want).max() < 1e-12
    # the module's and the synthetic buffers are this matrix rounded to fp32
    m = ResNetSpeakerEncoder(**SC.MODELS["ref"])
    assert torch.equal(m.torch_spec[1].mel_scale.fb, fb.float())
    assert torch.equal(SC.state_dict("ref")["torch_spec.1.mel_scale.fb"], fb.float())
    assert torch.equal(m.torch_spec[1].spectrogram.window, torch.hamming_window(400))
    assert torch.equal(m.torch_spec[0].filter, torch.tensor([[[-0.97, 1.0]]]))


@pytest.mark.parametrize("max_len", [20000, 40000, 48000])
def test_compute_embedding_window_offsets(max_len):
    """A clip shorter than, equal to and longer than num_frames * hop (250 * 160 = 40000)."""
    nf = min(250 * 160, max_len)
    want = [(int(o), int(o + nf)) for o in np.linspace(0, max_len - nf, num=10)]
    got = encoder.window_offsets(max_len, 250 * 160, 10)
    assert got == want and len(got) == 10
    assert got[0][0] == 0 and got[-1][1] == max_len and all(b - a == nf for a, b in got)
    if max_len <= 40000:
        assert all(w == (0, max_len) for w in got)


def test_constructor_errors():
    with pytest.raises(ValueError, match="Undefined encoder"):
        ResNetSpeakerEncoder(encoder_type="XYZ")
    with pytest.raises(ValueError, match="audio_config"):
        ResNetSpeakerEncoder(use_torch_spec=True)
    with pytest.raises(ValueError, match="math_mode"):
        ResNetSpeakerEncoder(math_mode="fp8")
    with pytest.raises(ValueError, match="num_mels"):
        ResNetSpeakerEncoder(input_dim=32, use_torch_spec=True, audio_config=SC.REF_AUDIO)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ResNetSpeakerEncoder()(torch.zeros(1, 64, 10))


@pytest.mark.parametrize("kw,word", [
    (dict(input_dim=60), "input_dim"),
    (dict(num_filters=[32, 64, 128, 512]), "num_filters"),
    (dict(num_filters=[12, 64, 128, 256]), "num_filters"),
    (dict(proj_dim=5000), "proj_dim"),
    (dict(layers=[30, 30, 3, 3]), "64 residual blocks"),
    (dict(use_torch_spec=True, audio_config=dict(SC.REF_AUDIO, hop_length=100)), "hop_length"),
    (dict(use_torch_spec=True, audio_config=dict(SC.REF_AUDIO, fft_size=500)), "n_fft"),
])
def test_limits_are_refused_at_construction(kw, word):
    with pytest.raises(N.NativeError) as e:
        ResNetSpeakerEncoder(**kw)
    assert e.value.code == N.TTS_ERR_UNSUPPORTED and word in str(e.value), str(e.value)


def test_new_symbols_declared_exported_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = ["tts_op_conv2d_3x3", "tts_op_conv2d_3x3_tile", "tts_speaker_encoder_num_weights",
             "tts_speaker_encoder_weight_numel", "tts_speaker_encoder_create", "tts_speaker_encoder_destroy",
             "tts_speaker_encoder_num_frames", "tts_speaker_encoder_forward", "tts_speaker_encoder_forward_profiled",
             "tts_speaker_encoder_features", "tts_stft_create_centered", "tts_stft_num_frames_centered"]
    lib = N.lib()
    for n in names:
        assert re.search(rf"\b{n}\s*\(", src), f"{n} not declared"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in N.SIGNATURES, f"{n} not bound"
    assert lib.tts_abi_version() == 115
    assert lib.tts_op_conv2d_3x3_tile() == 64
    assert ctypes.sizeof(N.TtsSpeakerEncoderCfg) == 17 * 4


def test_centered_stft_frame_count():
    cfg = N.TtsStftCfg(512, 160, 400, N.MATH_MODES["fp32x6"])
    lib = N.lib()
    for n in (257, 1120, 5920, 16000):
        assert lib.tts_stft_num_frames_centered(ctypes.byref(cfg), n) == 1 + n // 160
    assert lib.tts_stft_num_frames_centered(ctypes.byref(cfg), 256) == -N.TTS_ERR_INVALID
    assert b"n_fft / 2" in lib.tts_last_error()
    # the uncentred entry keeps its count: pad (n_fft - hop) / 2
    assert lib.tts_stft_num_frames(ctypes.byref(cfg), 5920) == 1 + (5920 + 2 * 176 - 512) // 160


def test_synthetic_recipe():
    sd = SC.state_dict("ref")
    w = sd["layer3.1.conv1.weight"]
    assert abs(w.std().item() / (2.0 / (128 * 9)) ** 0.5 - 1) < 0.02
    assert abs(sd["fc.weight"].std().item() / (1.0 / 4096) ** 0.5 - 1) < 0.02
    g1, g2 = sd["layer3.1.bn1.weight"], sd["layer3.1.bn2.weight"]
    assert 0.8 <= g1.min() and g1.max() <= 1.2 and 0.4 <= g2.min() and g2.max() <= 0.6
    assert sd["layer3.1.bn2.bias"].std() < 0.75 * sd["layer3.1.bn1.bias"].std()
    v = sd["layer3.1.bn2.running_var"]
    assert 0.8 <= v.min() and v.max() <= 1.2
    x = synthetic.speaker_wav(2, 16000, seed=3)
    assert x.shape == (2, 16000) and x.abs().max() <= 1.0 and 0.3 < x.std() < 0.45
    # the mel power of these wavs stays far above the 1e-6 floor of the log
    mel = R.torch_spec(sd, x, SC.REF_AUDIO)
    assert mel.min() > 1e-5, mel.min()


def test_hifidecoder_default_tree_is_unchanged():
    plain = HifiDecoder()
    assert not any(k.startswith("speaker_encoder") for k in plain.state_dict())
    assert not hasattr(plain, "speaker_encoder")
    assert set(plain.state_dict()) == {"waveform_decoder." + k for k in plain.waveform_decoder.state_dict()}
    with pytest.raises(RuntimeError, match="with_speaker_encoder"):
        plain.speaker_embedding(torch.zeros(1, 16000))
    full = HifiDecoder(with_speaker_encoder=True)
    keys = set(full.state_dict())
    assert {k for k in keys if not k.startswith("speaker_encoder.")} == set(plain.state_dict())
    want = expected_keys(64, 512, [3, 4, 6, 3], [32, 64, 128, 256], "ASP", True)
    assert {k[len("speaker_encoder."):]: tuple(v.shape) for k, v in full.state_dict().items()
            if k.startswith("speaker_encoder.")} == want
    assert full.speaker_encoder.log_input and full.speaker_encoder.use_torch_spec


def test_hifidecoder_load_checkpoint_keeps_the_speaker_encoder(tmp_path):
    src = HifiDecoder(with_speaker_encoder=True)
    src.speaker_encoder.load_state_dict(SC.state_dict("ref"))
    path = str(tmp_path / "xtts.pth")
    torch.save({"model": src.state_dict()}, path)
    dst = HifiDecoder(with_speaker_encoder=True)
    dst.load_checkpoint(path)
    for k, v in SC.state_dict("ref").items():
        assert torch.equal(dst.speaker_encoder.state_dict()[k], v), k
    HifiDecoder().load_checkpoint(path)  # the default drops the keys, as before
