"""MelGAN family on MI355X against the fp64 oracle (tests/_melgan_ref.py): the PQMF synthesis op, the
whole-residual-block kernel at its tile and reflection edges, and the three generators end to end.
Gates: tests/_util.py tol(); every measured error is logged with log_error (TTS_ERRLOG)."""
import ctypes

import numpy as np
import pytest
import torch

import _melgan_cases as MC
import _melgan_ref as R
from _util import assert_close_fp32, goldens, max_abs, tol
from tts_amd import _native as N
from tts_amd import synthetic, vocoder
from tts_amd.synthesizer import Synthesizer, mel_handoff

pytestmark = pytest.mark.gpu
MODES = [None, "fp32x6", "bf16"]  # None: the package default


def build(config, dev, mode=None, weight_norm=True):
    cls, ctor, _ = MC.CONFIGS[config]
    g = getattr(vocoder, cls)(**ctor, math_mode=mode)
    if not weight_norm:
        g.remove_weight_norm()
    g.load_state_dict(MC.state_dict(config, weight_norm))
    g.eval()
    return g.to(dev)


@pytest.fixture(scope="module")
def gens(cuda_device):
    cache = {}

    def get(config, mode=None):
        if (config, mode) not in cache:
            cache[(config, mode)] = build(config, cuda_device, mode)
        return cache[(config, mode)]

    return get


# ------------------------------------------------------------------ PQMF synthesis
@pytest.mark.parametrize("L", [1, 7, 8, 300])
def test_pqmf_synthesis_op(cuda_device, L):
    p = vocoder.PQMF().to(cuda_device)
    x = torch.randn(2, 4, L, generator=torch.Generator().manual_seed(L))
    y = p.synthesis(x.to(cuda_device))
    _, G, up = R.pqmf_filters()
    assert torch.equal(p.G.cpu(), G)
    ref = R.pqmf_synthesis(x.double(), G.double(), up.double())
    assert y.shape == (2, 1, 4 * L)
    assert_close_fp32(y.cpu(), ref, f"pqmf_synthesis L={L}", **tol("fp32", op=True))


# ------------------------------------------------------------------ residual block op
def block_weights(C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale  # noqa: E731
    return dict(w1=r(C, C, 3, scale=(3 * C) ** -0.5), b1=r(C, scale=0.1), w2=r(C, C, 1, scale=C**-0.5), b2=r(C, scale=0.1),
                ws=r(C, C, 1, scale=C**-0.5), bs=r(C, scale=0.1))


def run_block(dev, x, w, d, mode):
    B, C, L = x.shape
    xd = x.to(dev).contiguous()
    out = torch.empty_like(xd)
    h = {k: np.ascontiguousarray(v.numpy()) for k, v in w.items()}
    N.call("tts_op_melgan_block", N.ptr(xd), B, C, L, d, N.ptr(h["w1"]), N.ptr(h["b1"]), N.ptr(h["w2"]), N.ptr(h["b2"]),
           N.ptr(h["ws"]), N.ptr(h["bs"]), N.MATH_MODES[mode], N.ptr(out), N.stream_ptr(dev))
    return out.cpu()


def block_ref(x, w, d, zero_pad=False):
    w64 = {k: v.double() for k, v in w.items()}
    return R.res_block(x.double(), w64["w1"], w64["b1"], w64["w2"], w64["b2"], w64["ws"], w64["bs"], d, zero_pad)


def block_lengths(d):
    W = N.lib().tts_op_melgan_block_tile()
    return sorted({d + 1, 40, W - 1, W, W + 1, 2 * W + d})


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
@pytest.mark.parametrize("C", [32, 48, 192])
@pytest.mark.parametrize("d", [1, 27])
def test_block_op(cuda_device, mode, C, d):
    assert N.lib().tts_op_melgan_block_tile() == 64
    w = block_weights(C, 7 * C + d)
    for L in block_lengths(d):
        x = torch.randn(2, C, L, generator=torch.Generator().manual_seed(L))
        y = run_block(cuda_device, x, w, d, mode)
        assert_close_fp32(y, block_ref(x, w, d), f"melgan_block {mode} C={C} d={d} L={L}", **tol(mode, op=True))


def test_block_op_sees_the_reflected_ends(cuda_device):
    C, d, L = 48, 27, 65
    w = block_weights(C, 5)
    x = torch.randn(1, C, L, generator=torch.Generator().manual_seed(1))
    y = run_block(cuda_device, x, w, d, "fp32x6")
    assert_close_fp32(y, block_ref(x, w, d), "melgan_block reflect", **tol("fp32x6", op=True))
    wrong = max_abs(y.numpy(), block_ref(x, w, d, zero_pad=True).numpy())
    assert wrong > 1000 * tol("fp32x6", op=True)["max_abs_tol"], wrong


def test_block_op_errors(cuda_device):
    w = block_weights(32, 1)
    x = torch.randn(1, 32, 27)
    with pytest.raises(N.NativeError) as e:
        run_block(cuda_device, x, w, 27, "fp32x6")
    assert e.value.code == N.TTS_ERR_INVALID and "reflection pad" in str(e.value)


# ------------------------------------------------------------------ whole generators
@pytest.mark.parametrize("mode", MODES, ids=["default", "fp32x6", "bf16"])
@pytest.mark.parametrize("config,B,T,inference", MC.RUNS, ids=MC.RUN_IDS)
def test_generator_vs_oracle(cuda_device, gens, config, B, T, inference, mode):
    g = gens(config, mode)
    mel = MC.mel(B, T).to(cuda_device)
    y = g.inference(mel) if inference else g.forward(mel)
    ref = MC.oracle(config, B, T, inference)
    hop = g.hop_length
    L = T + (4 if inference else 0)
    if config == "multiband":
        assert y.shape == ((B, 1, 4 * hop * L) if inference else (B, 4, hop * L)) and hop == 64
    else:
        assert y.shape == (B, 1, hop * L) and hop == 256
    assert_close_fp32(y.cpu(), ref, f"{config} B={B} T={T} {'inference' if inference else 'forward'} {mode}",
                      **tol(mode or "f16x3"))


def test_forward_refuses_what_torch_refuses(cuda_device, gens):
    g = gens("multiband")
    with pytest.raises(ValueError, match="reflection pad 3"):
        g.forward(MC.mel(3, 1).to(cuda_device))  # T = 1 without the inference padding


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_batch_invariance(cuda_device, gens, mode):
    g = gens("multiband", mode)
    mel = MC.mel(3, 12).to(cuda_device)
    full = g.inference(mel)
    sub = g.forward(mel)
    for b in range(3):
        assert torch.equal(g.inference(mel[b:b + 1])[0], full[b])
        assert torch.equal(g.forward(mel[b:b + 1])[0], sub[b])


def test_inference_is_synthesis_of_forward(cuda_device, gens):
    g = gens("multiband", "fp32x6")
    mel = MC.mel(2, 12).to(cuda_device)
    padded = torch.nn.functional.pad(mel, (2, 2), "replicate")
    a = g.inference(mel)
    b = g.pqmf_synthesis(g.forward(padded))
    assert_close_fp32(a.cpu(), b.cpu().double(), "inference vs pqmf_synthesis(forward)", **tol("fp32x6", op=True))


@pytest.mark.parametrize("config", ["multiband", "melgan"])
def test_parametrized_and_folded_loads_agree_bitwise(cuda_device, gens, config):
    a = gens(config)
    b = build(config, cuda_device, weight_norm=False)
    c = build(config, cuda_device)
    c.remove_weight_norm()
    mel = MC.mel(1, 5).to(cuda_device)
    ya = a.inference(mel)
    assert torch.equal(ya, c.inference(mel))
    # synthetic's folded dict is folded in fp64 numpy, torch's fold in fp32: equal to rounding
    assert_close_fp32(b.inference(mel).cpu(), ya.cpu().double(), "folded state dict", **tol("f16x3"))


def test_handle_follows_parameter_changes(cuda_device):
    g = build("multiband", cuda_device)
    mel = MC.mel(1, 5).to(cuda_device)
    y0 = g.inference(mel)
    with torch.no_grad():
        g.layers[-2].bias.add_(0.25)
    y1 = g.inference(mel)
    assert not torch.equal(y0, y1)


def test_synthesizer_with_multiband_melgan(cuda_device, gens):
    from test_glow_tts_gpu import build_glow_tts

    name, meta, arr = [g for g in goldens("glow_tts") if g[0] == "glow_tts_b3_t23"][0]
    m = build_glow_tts(meta, cuda_device)
    voc = gens("multiband")
    tok = torch.from_numpy(arr["tokens"]).to(cuda_device)
    lens = torch.from_numpy(arr["lengths"]).to(cuda_device)
    torch.manual_seed(5)  # the decoder's latent noise: the same draw for both chains
    wav, voc_in = Synthesizer(m, voc).tts_batch(tok, lens)
    torch.manual_seed(5)
    out = m.inference(tok, {"x_lengths": lens})
    hand_in = mel_handoff(out["model_outputs"], None, None, time_major=True)
    hand = voc.inference(hand_in)
    assert torch.equal(voc_in, hand_in) and torch.equal(wav, hand)
    assert wav.shape == (3, 1, 256 * (voc_in.shape[-1] + 4)) and torch.isfinite(wav).all()


def test_device_errors(cuda_device, gens):
    g = gens("multiband")
    with pytest.raises(ValueError, match="channels"):
        g.inference(torch.zeros(1, 79, 20, device=cuda_device))
    f = vocoder.FullbandMelganGenerator().to(cuda_device)  # factors (2, 8, 2, 2), 4 blocks
    with pytest.raises(ValueError, match="reflection pad 27"):
        f.inference(torch.zeros(1, 80, 1, device=cuda_device))
    assert b"reflection pad" in N.lib().tts_last_error()
    # the library's own channel check
    x = torch.zeros(1, 79, 20, device=cuda_device)
    out = torch.empty(1, 4, 64 * 20, device=cuda_device)
    st = N.lib().tts_melgan_forward(g._native_handle(), N.ptr(x), 1, 79, 20, 0, 0, N.ptr(out), N.stream_ptr(cuda_device))
    assert st == N.TTS_ERR_INVALID and b"channels" in N.lib().tts_last_error()
    x80 = torch.zeros(1, 80, 20, device=cuda_device)
    out = torch.empty(1, 1, 256 * 20, device=cuda_device)
    st = N.lib().tts_melgan_forward(gens("melgan")._native_handle(), N.ptr(x80), 1, 80, 20, 0, 1, N.ptr(out),
                                    N.stream_ptr(cuda_device))
    assert st == N.TTS_ERR_INVALID and b"PQMF" in N.lib().tts_last_error()


def test_profiled_forward_lists_the_launches(cuda_device, gens):
    g = gens("multiband", "fp32x6")
    mel = MC.mel(1, 12).to(cuda_device)
    y, rows = g.profile(mel, synth=1)
    assert torch.equal(y, g.inference(mel))
    names = [r["name"] for r in rows]
    assert names[0] == "mel_gather" and names[-1] == "tail_pqmf" and len(names) == 2 + 3 + 12 + 1
    assert sum(n.startswith("res_block") for n in names) == 12
