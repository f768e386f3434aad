"""XTTS voice cloning without a device: the parameter tree and checkpoint slice of ``XttsConditioning``, the
C-ABI inventory and limits, the excluded options, the fp64 oracle (tests/_xtts_cond_ref.py) against an
independent formulation with torch's own ops, the scale of the test weights, the
resample table, the mel filterbank, and the host code under AddressSanitizer + UBSan
(``make -C tts-3_amd asan-check-cond``)."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _xtts_cond_cases as C
import _xtts_cond_ref as R
import _xtts_gpt_cases as GC
from _util import max_abs
from tts_amd import _native as N
from tts_amd import audio
from tts_amd.tts import HifiDecoder, Xtts, XttsConditioning, XttsGPT
from tts_amd.tts import xtts_cond as XC

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd")
NEW_SYMBOLS = ["tts_xtts_cond_num_weights", "tts_xtts_cond_weight_numel", "tts_xtts_cond_create", "tts_xtts_cond_destroy",
               "tts_xtts_cond_num_frames", "tts_xtts_cond_mel", "tts_xtts_cond_style_emb",
               "tts_xtts_cond_style_emb_profiled", "tts_resample_create", "tts_resample_destroy",
               "tts_resample_num_samples", "tts_resample_forward", "tts_op_groupnorm", "tts_op_mha_wide",
               "tts_op_cross_attn", "tts_op_cond_ff", "tts_op_rmsnorm"]


def cfg(**over):
    c = N.TtsXttsCondCfg()
    base = dict(spec_dim=80, model_dim=128, heads=2, attn_blocks=2, perceiver_depth=2, num_latents=32,
                perceiver_dim_head=64, perceiver_heads=8, ff_mult=4, n_fft=2048, hop_length=256, win_length=1024,
                math_mode=0)
    base.update(over)
    for k, v in base.items():
        setattr(c, k, v)
    return c


# ------------------------------------------------------------------------------------ tree, checkpoint
@pytest.mark.parametrize("name", list(C.MODELS))
def test_parameter_tree_and_shapes(name):
    m = XttsConditioning(**C.ctor_kwargs(name))
    sd, want = m.state_dict(), C.state_dict(name)
    assert list(sd) == list(want)  # the reference's keys, in its order
    assert all(sd[k].shape == want[k].shape for k in want)
    E = C.MODELS[name]["model_dim"]
    assert XC.ff_inner_dim(E, 4) == {128: 341, 96: 256, 1024: 2730}[E]
    assert m.conditioning_encoder.attn[0].norm.num_groups == 32
    m.load_state_dict(want, strict=True)


def test_strict_load_from_a_full_checkpoint(tmp_path):
    """The conditioning slice and the GPT's slice of one synthetic full checkpoint, each strict; the GPT's
    tree and filter are what they were."""
    gcfg = GC.MODELS["narrow"]
    gpt_sd = GC.state_dict(gcfg, GC.MODEL_SEED["narrow"])
    full = C.full_checkpoint("narrow", gpt_sd)
    path = tmp_path / "model.pth"
    torch.save({"model": full}, path)
    m = XttsConditioning(**C.ctor_kwargs("narrow"))
    m.load_checkpoint(path)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in C.state_dict("narrow").items())
    gpt = XttsGPT(**GC.ctor_kwargs(gcfg))
    gpt.load_checkpoint(path, strict=True)
    assert set(gpt.state_dict()) == set(gpt_sd) and all(torch.equal(gpt.state_dict()[k], v) for k, v in gpt_sd.items())
    # the gpt.* slice and a bare state dict load too; a missing key is an error
    assert set(XC.conditioning_checkpoint_filter({k[4:]: v for k, v in full.items() if k.startswith("gpt.")})) == \
        set(C.state_dict("narrow"))
    bad = dict(C.state_dict("narrow"))
    del bad["conditioning_perceiver.norm.gamma"]
    with pytest.raises(RuntimeError):
        XttsConditioning(**C.ctor_kwargs("narrow")).load_state_dict(bad, strict=True)


# ------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_exported_and_version_unchanged():
    lib = N.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in N.SIGNATURES
    assert lib.tts_abi_version() == 115 == N.ABI_VERSION


@pytest.mark.parametrize("name", list(C.MODELS))
def test_weight_inventory_matches_the_module(name):
    m = XttsConditioning(**C.ctor_kwargs(name))
    c = m._make_cfg()
    lib = N.lib()
    ws = m._weight_list()
    assert lib.tts_xtts_cond_num_weights(ctypes.byref(c)) == len(ws) == len(C.state_dict(name)) + 2
    for i, w in enumerate(ws):
        assert lib.tts_xtts_cond_weight_numel(ctypes.byref(c), i) == w.size
    assert lib.tts_xtts_cond_weight_numel(ctypes.byref(c), len(ws)) == -1
    assert lib.tts_xtts_cond_weight_numel(ctypes.byref(c), -1) == -1
    assert ws[-2].shape == (1024,) and ws[-1].shape == (1025, 80)


@pytest.mark.parametrize("over,code", [
    (dict(model_dim=2112, heads=33), N.TTS_ERR_UNSUPPORTED),   # more than 2048 channels
    (dict(model_dim=96, heads=2), N.TTS_ERR_UNSUPPORTED),      # head size 48
    (dict(num_latents=65), N.TTS_ERR_UNSUPPORTED),
    (dict(perceiver_dim_head=512), N.TTS_ERR_UNSUPPORTED),
    (dict(model_dim=128, heads=3), N.TTS_ERR_INVALID),         # heads do not divide the channels
    (dict(perceiver_depth=0), N.TTS_ERR_INVALID),
    (dict(math_mode=9), N.TTS_ERR_INVALID),
])
def test_limits_rejected_before_any_launch(over, code):
    lib = N.lib()
    assert lib.tts_xtts_cond_num_weights(ctypes.byref(cfg(**over))) == -code
    assert lib.tts_xtts_cond_weight_numel(ctypes.byref(cfg(**over)), 0) == -1
    assert lib.tts_xtts_cond_num_weights(None) == -N.TTS_ERR_INVALID


def test_module_refuses_what_the_library_refuses():
    with pytest.raises(N.NativeError) as e:
        XttsConditioning(model_dim=96, heads=2)
    assert e.value.code == N.TTS_ERR_UNSUPPORTED and "head size" in str(e.value)
    with pytest.raises(ValueError):
        XttsConditioning(math_mode="fp8")


def test_null_handles_and_bad_resample_ratios():
    lib = N.lib()
    assert lib.tts_xtts_cond_style_emb(None, None, 1, 1, None, None) == N.TTS_ERR_INVALID
    assert lib.tts_xtts_cond_mel(None, None, 1, 4096, None, None, None) == N.TTS_ERR_INVALID
    assert lib.tts_xtts_cond_num_frames(None, 4096) == -N.TTS_ERR_INVALID
    assert lib.tts_resample_forward(None, None, 1, 10, None, None) == N.TTS_ERR_INVALID
    h = ctypes.c_void_p()
    assert lib.tts_resample_create(22051, 16000, 0, ctypes.byref(h)) == N.TTS_ERR_UNSUPPORTED and not h.value
    assert lib.tts_resample_create(0, 16000, 0, ctypes.byref(h)) == N.TTS_ERR_INVALID
    assert lib.tts_op_groupnorm(None, 1, 32, 4, 8, None, None, 1e-5, None, None) == N.TTS_ERR_INVALID
    assert lib.tts_op_rmsnorm(None, 1, 32, 4, None, None, None) == N.TTS_ERR_INVALID
    assert lib.tts_op_cross_attn(None, None, None, 1, 8, 64, 32, 4, None, None) == N.TTS_ERR_INVALID


# ------------------------------------------------------------------------------------ excluded options
def test_excluded_options_and_missing_parts_raise():
    gpt = XttsGPT(**GC.ctor_kwargs(GC.MODELS["narrow"]))
    dec = HifiDecoder(decoder_input_dim=128, upsample_initial_channel_decoder=128, d_vector_dim=32)
    x = Xtts(gpt, dec, conditioning=XttsConditioning(**C.ctor_kwargs("narrow")), mel_stats=C.mel_norms())
    assert torch.equal(x.mel_stats, C.mel_norms())
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        x.get_conditioning_latents("speaker.wav")
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        x.get_conditioning_latents(["a.wav", "b.wav"])
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        x.get_conditioning_latents(torch.zeros(1, 22050), librosa_trim_db=20)
    with pytest.raises(RuntimeError, match="ROCm device"):  # no CPU fallback
        x.get_gpt_cond_latents(torch.zeros(1, 22050), 22050)
    with pytest.raises(RuntimeError, match="speaker encoder"):
        x.get_speaker_embedding(torch.zeros(1, 22050), 22050)
    bare = Xtts(gpt, dec)
    assert "mel_stats" not in bare.state_dict() and not hasattr(bare, "conditioning")  # the tree of before
    with pytest.raises(RuntimeError, match="conditioning"):
        bare.get_gpt_cond_latents(torch.zeros(1, 22050), 22050)
    with pytest.raises(RuntimeError, match="conditioning"):
        bare.get_conditioning_latents(torch.zeros(1, 22050))
    with pytest.raises(RuntimeError, match="ROCm device"):
        XttsConditioning(**C.ctor_kwargs("narrow")).get_style_emb(torch.zeros(1, 80, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        audio.resample(torch.zeros(1, 100), 22050, 16000)


# ---------------------------------------------------------------------------------------------- oracle
def independent_style_emb(sd, mel, heads):
    """The same function with torch's own ops: nn.functional.group_norm, scaled_dot_product_attention,
    F.gelu, F.normalize."""
    dt = torch.float64
    p = "conditioning_encoder."
    h = F.conv1d(mel.to(dt), sd[p + "init.weight"].to(dt), sd[p + "init.bias"].to(dt))
    B, E, T = h.shape
    dk = E // heads
    i = 0
    while f"{p}attn.{i}.qkv.weight" in sd:
        q_ = f"{p}attn.{i}."
        xn = F.group_norm(h, R.normalization_groups(E), sd[q_ + "norm.weight"].to(dt), sd[q_ + "norm.bias"].to(dt), 1e-5)
        qkv = F.conv1d(xn, sd[q_ + "qkv.weight"].to(dt), sd[q_ + "qkv.bias"].to(dt)).reshape(B, heads, 3, dk, T)
        q, k, v = (qkv[:, :, j].transpose(2, 3) for j in range(3))  # [B, heads, T, dk]
        a = F.scaled_dot_product_attention(q, k, v).transpose(2, 3).reshape(B, E, T)
        h = xn + F.conv1d(a, sd[q_ + "proj_out.weight"].to(dt), sd[q_ + "proj_out.bias"].to(dt))
        i += 1
    ctx = h.transpose(1, 2)
    p = "conditioning_perceiver."
    lat = sd[p + "latents"].to(dt)[None].repeat(B, 1, 1)
    i = 0
    while f"{p}layers.{i}.0.to_q.weight" in sd:
        q_ = f"{p}layers.{i}."
        kvin = torch.cat((lat, ctx), dim=1)
        q = F.linear(lat, sd[q_ + "0.to_q.weight"].to(dt))
        k, v = F.linear(kvin, sd[q_ + "0.to_kv.weight"].to(dt)).chunk(2, dim=-1)
        hd = lambda t: t.unflatten(-1, (8, 64)).transpose(1, 2)  # noqa: E731
        o = F.scaled_dot_product_attention(hd(q), hd(k), hd(v)).transpose(1, 2).flatten(2)
        lat = F.linear(o, sd[q_ + "0.to_out.weight"].to(dt)) + lat
        x, gate = F.linear(lat, sd[q_ + "1.0.weight"].to(dt), sd[q_ + "1.0.bias"].to(dt)).chunk(2, dim=-1)
        lat = F.linear(F.gelu(gate) * x, sd[q_ + "1.2.weight"].to(dt), sd[q_ + "1.2.bias"].to(dt)) + lat
        i += 1
    out = F.normalize(lat, dim=-1) * math.sqrt(E) * sd[p + "norm.gamma"].to(dt)
    return out.transpose(1, 2)


@pytest.mark.parametrize("name", list(C.MODELS))
def test_oracle_matches_an_independent_formulation(name):
    T = 29
    ref = C.style_oracle(name, T)
    ind = independent_style_emb(C.state_dict(name), C.mel_input(T), C.MODELS[name]["heads"])
    assert ref.shape == ind.shape == (2, C.MODELS[name]["model_dim"], 32)
    assert max_abs(ref.numpy(), ind.numpy()) < 1e-12
    # [B, 1, 80, T] is squeezed
    assert torch.equal(R.style_emb(C.state_dict(name), C.mel_input(T).unsqueeze(1), C.MODELS[name]["heads"]), ref)


def test_test_weights_keep_the_activations_of_order_one():
    sd = C.state_dict("narrow")
    h = R.conditioning_encoder(sd, C.mel_input(65), 2)
    assert 0.5 < float(h.std()) < 2.0
    pre = "conditioning_perceiver."
    lat = sd[pre + "latents"].double()[None].expand(2, -1, -1)
    for i in range(2):
        lp = f"{pre}layers.{i}."
        lat = R.perceiver_attention(sd, lp + "0.", lat, h.permute(0, 2, 1), 8, 64)
        lat = R.feed_forward(*(sd[lp + k].double() for k in ("1.0.weight", "1.0.bias", "1.2.weight", "1.2.bias")), lat)
        assert 0.5 < float(lat.std()) < 2.0
    assert float(sd["conditioning_encoder.attn.0.proj_out.weight"].abs().max()) > 0  # not the zero init


# ------------------------------------------------------------------------------ resample table, filterbank
@pytest.mark.parametrize("orig,new,o,n,w", [(22050, 16000, 441, 320, 9), (24000, 22050, 160, 147, 7),
                                            (22050, 24000, 147, 160, 7)])
def test_resample_table_rows(orig, new, o, n, w):
    """Every phase's taps sum to 1 within 1e-3 (the table carries the factor base / o, and a phase's sinc
    samples, spaced base / o apart, sum to o / base), so a DC input comes out as DC away from the edges."""
    kern, o_, n_, w_ = R.resample_table(orig, new)
    assert (o_, n_, w_) == (o, n, w) and kern.shape == (n, 2 * w + o)
    assert float((kern.sum(dim=1) - 1.0).abs().max()) < 1e-3
    base = min(o, n) * 0.99
    assert abs(float(kern[0, w]) - base / o) < 1e-12  # t = 0: sinc = window = 1
    k2, w2 = audio.resample_kernel(orig, new)
    assert w2 == w and np.abs(k2 - kern.numpy()).max() < 1e-15
    x = torch.ones(1, 20 * o, dtype=torch.float64)
    y = R.resample(x, orig, new)
    assert y.shape == (1, 20 * n)
    assert float((y[0, 2 * n : -2 * n] - 1.0).abs().max()) < 1e-3
    for N_ in (1, o - 1, o, o + 1):
        assert R.resample(torch.zeros(1, N_), orig, new).shape[1] == -(-n * N_ // o)


def test_mel_filterbank():
    fb = audio.melscale_fbanks(1025, 0, 8000, 80, 22050)
    assert fb.shape == (1025, 80) and fb.dtype == np.float64 and (fb >= 0).all()
    freqs = np.linspace(0, 11025, 1025)
    assert (fb[freqs > 8000] == 0).all() and (fb[0] == 0).all()
    assert (fb.sum(axis=0) > 0).all()  # no empty band
    assert np.abs(fb - R.mel_filterbank().numpy()).max() < 1e-15
    # slaney: every triangle has unit area in Hz (up to the bin grid)
    area = fb.sum(axis=0) * (11025 / 1024)
    assert np.abs(area - 1.0).max() < 0.05
    win = audio.hann_window(1024)
    assert np.abs(win - torch.hann_window(1024, periodic=True, dtype=torch.float64).numpy()).max() < 1e-15
    with pytest.raises(NotImplementedError):
        audio.melscale_fbanks(1025, 0, 8000, 80, 22050, mel_scale="slaney")


def test_oracle_mel_is_torch_stft_with_the_reference_parameters():
    wav = C.clip(7277, seed=1)
    mel = R.wav_to_mel_cloning(wav, C.mel_norms())
    assert mel.shape == (1, 80, 29)
    silent = R.wav_to_mel_cloning(torch.zeros(1, 7277), C.mel_norms())
    assert float((silent[0] - (math.log(1e-5) / C.mel_norms().double())[:, None]).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------- host code
@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/llvm/bin/clang++"),
                    reason="needs make and the ROCm clang++")
def test_conditioning_host_code_clean_under_asan_ubsan():
    r = subprocess.run(["make", "-C", PKG, "asan-check-cond"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "conditioning host code OK" in r.stdout
