"""MelGAN family without a device: the drop-in modules' parameter tree and keys, weight-norm folding,
the C-ABI weight inventory and validation, the PQMF buffers, the polyphase identity the kernels
rely on, and the conditioning of the synthetic generators the GPU parity tests use."""
import ctypes

import numpy as np
import pytest
import torch

import _melgan_cases as MC
import _melgan_ref as R
from _util import FP32_REL_RMS, WAV_MAX_ABS, max_abs, rel_rms
from tts_amd import _native as N
from tts_amd import synthetic, vocoder
from tts_amd.vocoder import PQMF, MelganGenerator, MultibandMelganGenerator


def build(config: str, **kw):
    cls, ctor, _ = MC.CONFIGS[config]
    return getattr(vocoder, cls)(**ctor, **kw)


@pytest.mark.parametrize("config", list(MC.CONFIGS))
@pytest.mark.parametrize("wn", [True, False], ids=["parametrized", "folded"])
def test_strict_load_and_key_order(config, wn):
    g = build(config)
    sd = MC.state_dict(config, wn)
    if not wn:
        g.remove_weight_norm()
    g.load_state_dict(sd, strict=True)
    assert list(g.state_dict().keys()) == list(sd.keys())
    keys = list(sd.keys())
    if wn:
        assert keys[:3] == ["layers.1.bias", "layers.1.parametrizations.weight.original0",
                            "layers.1.parametrizations.weight.original1"]
    stack = [k for k in keys if k.startswith("layers.4.")]
    first_shortcut = min(i for i, k in enumerate(stack) if ".shortcuts." in k)
    assert all(".blocks." in k for k in stack[:first_shortcut]) and all(".shortcuts." in k for k in stack[first_shortcut:])
    assert "layers.4.blocks.0.2.bias" in keys and "layers.4.blocks.0.4.bias" in keys
    if MC.CONFIGS[config][2]:
        assert keys[-3:] == ["pqmf_layer.H", "pqmf_layer.G", "pqmf_layer.updown_filter"]


def test_defaults_match_reference():
    g = MelganGenerator()
    assert g.inference_padding == 2 and g.hop_length == 256
    m = MultibandMelganGenerator()
    assert m.layers[1].weight.shape == (384, 80, 7) and m.layers[-2].weight.shape == (4, 24, 7)
    assert m.pqmf_layer.N == 4 and m.pqmf_layer.taps == 62
    f = vocoder.FullbandMelganGenerator()
    assert len(f.layers[4].blocks) == 4 and f.upsample_factors == [2, 8, 2, 2]
    with pytest.raises(AssertionError):
        MelganGenerator(proj_kernel=6)


def test_remove_weight_norm_equals_torch_fold():
    g = build("multiband")
    sd = MC.state_dict("multiband")
    g.load_state_dict(sd)
    g.remove_weight_norm()
    out = g.state_dict()
    assert not any("parametrizations" in k for k in out)
    for name in ("layers.1", "layers.3", "layers.4.blocks.2.2", "layers.4.shortcuts.3", "layers.13"):
        assert torch.equal(out[f"{name}.weight"], R.folded(sd, name, torch.float32)), name
    # the folded state dict of synthetic matches too (same random stream)
    for k, v in MC.state_dict("multiband", False).items():
        torch.testing.assert_close(out[k], v, rtol=1e-6, atol=1e-7)


def native_cfg(config: str):
    return build(config)._cfg


@pytest.mark.parametrize("config", list(MC.CONFIGS))
def test_weight_inventory(config):
    g = build(config)
    g.load_state_dict(MC.state_dict(config))
    ws = g._weight_list()
    lib = N.lib()
    assert lib.tts_melgan_num_weights(ctypes.byref(g._cfg)) == len(ws)
    for i, w in enumerate(ws):
        assert lib.tts_melgan_weight_numel(ctypes.byref(g._cfg), i) == w.size, i
    assert lib.tts_melgan_weight_numel(ctypes.byref(g._cfg), len(ws)) == -1
    # the convs in state-dict order, (weight, bias) each, the folded values; G last
    folded = MC.state_dict(config, False)
    convs = [k[:-len(".weight")] for k in folded if k.endswith(".weight")]
    assert 2 * len(convs) == len(ws) - (1 if MC.CONFIGS[config][2] else 0)
    for i, name in enumerate(convs):
        assert np.allclose(ws[2 * i], folded[f"{name}.weight"].numpy(), rtol=1e-6, atol=1e-8), name
        assert np.array_equal(ws[2 * i + 1], folded[f"{name}.bias"].numpy()), name
    if MC.CONFIGS[config][2]:
        assert np.array_equal(ws[-1], folded["pqmf_layer.G"].numpy())


@pytest.mark.parametrize("change,code,word", [
    (dict(upsample_factors=[8, 3, 2]), N.TTS_ERR_UNSUPPORTED, "2, 4 or 8"),
    (dict(res_kernel=5), N.TTS_ERR_UNSUPPORTED, "res_kernel must be 3"),
    (dict(num_res_blocks=5), N.TTS_ERR_UNSUPPORTED, "at most 4"),
    (dict(base_channels=1024), N.TTS_ERR_UNSUPPORTED, "512"),
])
def test_validation_codes(change, code, word):
    ctor = dict(MC.CONFIGS["melgan"][1])
    ctor.update(change)
    with pytest.raises(N.NativeError) as e:
        MelganGenerator(**ctor)
    assert e.value.code == code and word in str(e.value)


def test_validation_even_proj_kernel_in_the_library():
    c = native_cfg("melgan")
    c.proj_kernel = 6
    assert N.lib().tts_melgan_num_weights(ctypes.byref(c)) == -N.TTS_ERR_INVALID
    assert b"proj_kernel" in N.lib().tts_last_error()
    c.proj_kernel = 7
    c.res_kernel = 4  # the module's own assert refuses these before the library sees them
    assert N.lib().tts_melgan_num_weights(ctypes.byref(c)) == -N.TTS_ERR_INVALID
    assert b"res_kernel must be odd" in N.lib().tts_last_error()
    c.res_kernel = 3
    c.base_channels = 8
    assert N.lib().tts_melgan_num_weights(ctypes.byref(c)) == -N.TTS_ERR_INVALID
    assert b"base_channels >> num_ups" in N.lib().tts_last_error()
    c.base_channels = 512
    c.math_mode = 9
    assert N.lib().tts_melgan_num_weights(ctypes.byref(c)) == -N.TTS_ERR_INVALID


def test_short_input_raises_value_error_without_a_device():
    g = vocoder.FullbandMelganGenerator()  # factors (2, 8, 2, 2), 4 blocks: T = 1 -> first stack 10 < 27
    with pytest.raises(ValueError, match="reflection pad 27"):
        g.inference(torch.zeros(1, 80, 1))
    with pytest.raises(ValueError, match="reflection pad 3 of the first conv"):
        g.forward(torch.zeros(1, 80, 3))
    with pytest.raises(ValueError, match="channels"):
        g.inference(torch.zeros(1, 79, 20))
    with pytest.raises(RuntimeError, match="ROCm device"):
        g.inference(torch.zeros(1, 80, 20))
    with pytest.raises(RuntimeError, match="ROCm device"):
        PQMF().synthesis(torch.zeros(1, 4, 8))
    with pytest.raises(NotImplementedError):
        PQMF().analysis(torch.zeros(1, 1, 64))


def test_pqmf_buffers_bitwise():
    pytest.importorskip("scipy")
    H, G, up = R.pqmf_filters(4, 62, 0.15, 9.0)
    p = PQMF(N=4, taps=62, cutoff=0.15, beta=9.0)
    assert p.H.dtype == torch.float32 and p.H.shape == (4, 1, 63) and p.G.shape == (1, 4, 63)
    assert torch.equal(p.H, H) and torch.equal(p.G, G) and torch.equal(p.updown_filter, up)
    assert list(p.state_dict().keys()) == ["H", "G", "updown_filter"]


@pytest.mark.parametrize("L", [1, 7, 8, 33])
def test_oracle_synthesis_is_the_polyphase_sum(L):
    pytest.importorskip("scipy")
    _, G, up = R.pqmf_filters()
    x = torch.randn(2, 4, L, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    y = R.pqmf_synthesis(x, G.double(), up.double())
    assert y.shape == (2, 1, 4 * L)
    assert np.abs(y.numpy() - R.pqmf_polyphase(x.numpy(), G.double().numpy())).max() < 1e-12


@pytest.mark.parametrize("config,B,T,inference", MC.RUNS, ids=MC.RUN_IDS)
def test_generator_cases_are_well_conditioned(config, B, T, inference):
    """The oracle's own fp32 forward stays within a fifth of the fp32 gates of its fp64 forward, and the
    waveform is neither tiny nor saturated, so the GPU gates on these cases are meaningful."""
    y64 = MC.oracle(config, B, T, inference)
    y32 = MC.oracle(config, B, T, inference, torch.float32)
    hop = int(np.prod(MC.CONFIGS[config][1]["upsample_factors"]))
    L = T + (4 if inference else 0)
    if MC.CONFIGS[config][2]:
        assert y64.shape == ((B, 1, 4 * hop * L) if inference else (B, 4, hop * L))
    else:
        assert y64.shape == (B, 1, hop * L)
    ma, rr = max_abs(y32.numpy(), y64.numpy()), rel_rms(y32.numpy(), y64.numpy())
    sd, peak = float(y64.std()), float(y64.abs().max())
    print(f"{config} B={B} T={T} inference={inference}: fp32 vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e} std={sd:.3f} peak={peak:.4f}")
    assert ma <= WAV_MAX_ABS / 5 and rr <= FP32_REL_RMS / 5
    assert 0.05 <= sd <= 0.5 and peak < 0.999


def test_mac_count_of_the_multiband_generator():
    """The per-frame MAC count DESIGN.md quotes, counted from the oracle."""
    counter = {}
    T = 40
    with torch.no_grad():
        R.melgan_layers(MC.state_dict("multiband"), MC.mel(1, T), counter=counter, **MC.ref_cfg("multiband"))
    per_frame = {k: v / T for k, v in counter.items()}
    total = sum(per_frame.values())
    print({k: round(v / 1e6, 3) for k, v in per_frame.items()}, round(total / 1e6, 3))
    assert abs(per_frame["stack.0"] - 8 * 4 * 5 * 192 * 192) < 1
    assert 17.5e6 < total < 18.5e6  # 36 MFLOP per frame


def test_synthetic_state_dict_is_seeded():
    a = synthetic.melgan_state_dict(seed=1, base_channels=64)
    b = synthetic.melgan_state_dict(seed=1, base_channels=64)
    assert all(torch.equal(a[k], b[k]) for k in a)
