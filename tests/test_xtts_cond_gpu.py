"""XTTS voice cloning on MI355X against the fp64 oracle (tests/_xtts_cond_ref.py): the GroupNorm, wide
attention, cross-attention, feed-forward and RMSNorm ops, the mel front end, the resampler,
``XttsConditioning.get_style_emb`` per model, and ``Xtts.get_gpt_cond_latents`` /
``get_conditioning_latents`` down to ``Xtts.inference``.

Gates: tests/_util.py ``tol(mode, op=True)`` on single ops, ``tol(mode)`` on ``get_style_emb`` and the
latents.  Every measured error goes through ``log_error`` (TTS_ERRLOG)."""
import math

import pytest
import torch

import _speaker_encoder_cases as SC
import _speaker_encoder_ref as SR
import _xtts_cond_cases as C
import _xtts_cond_ref as R
import _xtts_gpt_cases as GC
from _util import assert_close_fp32, tol
from tts_amd import _native as N
from tts_amd import audio, synthetic
from tts_amd.encoder import ResNetSpeakerEncoder
from tts_amd.tts import HifiDecoder, Xtts, XttsConditioning, XttsGPT, multi_head_attention
from tts_amd.tts import xtts_cond as XC

pytestmark = pytest.mark.gpu

_MODELS = {}


def model(name, dev, mode="fp32"):
    k = (name, mode)
    if k not in _MODELS:
        m = XttsConditioning(**C.ctor_kwargs(name), math_mode=mode)
        m.load_state_dict(C.state_dict(name), strict=True)
        _MODELS[k] = m.eval().to(dev)
    return _MODELS[k]


def rnd(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


# ------------------------------------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize("T", [1, 63, 64, 65, 517])
@pytest.mark.parametrize("Cc", [96, 128, 1024])
def test_groupnorm_op_vs_fp64(cuda_device, Cc, T):
    """Per-group mean 100 with unit spread: E[x^2] - E[x]^2 in fp32 would lose the variance entirely."""
    B, G = 3, R.normalization_groups(Cc)
    x = rnd(B, Cc, T, seed=Cc + T) + 100.0
    w, b = 1.0 + rnd(Cc, seed=1, std=0.1), rnd(Cc, seed=2, std=0.1)
    y = XC.group_norm(x.to(cuda_device), G, w, b)
    ref = R.group_norm(x.double(), G, w.double(), b.double())
    assert_close_fp32(y.cpu(), ref, f"groupnorm C={Cc} T={T}", **tol("fp32", op=True))


def test_groupnorm_limits(cuda_device):
    x = torch.zeros(1, 96, 4, device=cuda_device)
    w = torch.ones(96, device=cuda_device)
    with pytest.raises(N.NativeError) as e:
        XC.group_norm(x, 7, w, w)  # 96 % 7 != 0
    assert e.value.code == N.TTS_ERR_INVALID


# -------------------------------------------------------------------------------------- wide attention
def mha_ref(qkv, heads):
    B, E3, T = qkv.shape
    E = E3 // 3
    dk = E // heads
    q, k, v = (t.reshape(B, heads, dk, T) for t in qkv.double().split(E, dim=1))
    w = torch.softmax(torch.einsum("bhdi,bhdj->bhij", q, k) / math.sqrt(dk), dim=-1)
    return torch.einsum("bhij,bhdj->bhdi", w, v).reshape(B, E, T)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 64, 65, 130])
@pytest.mark.parametrize("E,heads", [(1024, 16), (2048, 16), (96, 3)])
def test_wide_attention_op_vs_fp64(cuda_device, E, heads, T, mode):
    qkv = rnd(2, 3 * E, T, seed=E + T)
    out = XC.wide_multi_head_attention(qkv.to(cuda_device), heads, math_mode=mode)
    assert_close_fp32(out.cpu(), mha_ref(qkv, heads), f"wide mha {mode} E={E} T={T}", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_wide_attention_is_bitwise_tts_op_mha_where_both_accept(cuda_device, mode):
    qkv = rnd(2, 3 * 128, 130, seed=4).to(cuda_device)
    kl = torch.tensor([130, 77])
    a = XC.wide_multi_head_attention(qkv, 2, key_lengths=kl, math_mode=mode)
    b = multi_head_attention(qkv, 2, key_lengths=kl, math_mode=mode)
    assert torch.equal(a, b)


def test_wide_attention_limits_and_unchanged_neighbours(cuda_device):
    lib = N.lib()
    out = torch.full((1, 2112, 4), 7.0, device=cuda_device)

    def status(fn, E, heads):
        qkv = torch.zeros(1, 3 * E, 4, device=cuda_device)
        st = getattr(lib, fn)(N.ptr(qkv), None, 1, E, heads, 4, 0, N.ptr(out), N.stream_ptr(cuda_device))
        torch.cuda.synchronize(cuda_device)
        assert bool((out == 7.0).all())
        return st

    assert status("tts_op_mha_wide", 2112, 33) == N.TTS_ERR_UNSUPPORTED  # dk 64, E > 2048
    assert status("tts_op_mha_wide", 768, 4) == N.TTS_ERR_UNSUPPORTED    # dk 192: tts_op_mha's ground
    assert status("tts_op_mha", 1024, 16) == N.TTS_ERR_UNSUPPORTED       # tts_op_mha still stops at 512 channels


# ------------------------------------------------------------------------------------- cross-attention
def cross_ref(q, kvl, kvc, heads):
    B, inner, L = q.shape
    dh = inner // heads
    kv = torch.cat((kvl, kvc), dim=2).double()  # latents first
    k, v = kv[:, :inner], kv[:, inner:]
    qh, kh, vh = (t.reshape(B, heads, dh, -1) for t in (q.double(), k, v))
    w = torch.softmax(torch.einsum("bhdi,bhdj->bhij", qh, kh) * dh**-0.5, dim=-1)
    return torch.einsum("bhij,bhdj->bhdi", w, vh).reshape(B, inner, L)


@pytest.mark.parametrize("L", [32, 7])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 97, 517])
def test_cross_attention_op_vs_fp64(cuda_device, T, L):
    B, heads, dh = 2, 8, 64
    q = rnd(B, heads * dh, L, seed=T + L)
    kvl, kvc = rnd(B, 2 * heads * dh, L, seed=T + 1), rnd(B, 2 * heads * dh, T, seed=T + 2)
    out = XC.cross_attention(q.to(cuda_device), kvl.to(cuda_device), kvc.to(cuda_device), heads)
    assert_close_fp32(out.cpu(), cross_ref(q, kvl, kvc, heads), f"cross attention T={T} L={L}", **tol("fp32", op=True))


@pytest.mark.parametrize("where", ["context", "latents"])
def test_cross_attention_dominant_key_comes_from_its_buffer(cuda_device, where):
    """Every query equals u; one key is 40 u / |u|^2 sqrt(dh), so its score is 40 and its softmax weight 1 up to
    e^-30: the output is that key's value, from the context buffer (key 5 of it) or the latents' (key 3)."""
    B, heads, dh, L, T = 1, 8, 64, 32, 97
    inner = heads * dh
    u = rnd(inner, seed=5)
    q = u[None, :, None].expand(B, inner, L).contiguous()
    kvl, kvc = rnd(B, 2 * inner, L, seed=6, std=0.1), rnd(B, 2 * inner, T, seed=7, std=0.1)
    uh = u.reshape(heads, dh)
    big = (40.0 * math.sqrt(dh) * uh / (uh * uh).sum(dim=1, keepdim=True)).reshape(inner)
    buf, j = (kvc, 5) if where == "context" else (kvl, 3)
    buf[0, :inner, j] = big
    out = XC.cross_attention(q.to(cuda_device), kvl.to(cuda_device), kvc.to(cuda_device), heads).cpu()
    assert_close_fp32(out, cross_ref(q, kvl, kvc, heads), f"cross attention dominant {where}", **tol("fp32", op=True))
    want = buf[0, inner:, j]
    assert float((out[0] - want[:, None]).abs().max()) < 1e-5


def test_cross_attention_limits(cuda_device):
    lib = N.lib()
    out = torch.full((1, 512, 65), 7.0, device=cuda_device)
    z = torch.zeros(1, 1024, 65, device=cuda_device)

    def st(L, T):
        s = lib.tts_op_cross_attn(N.ptr(z), N.ptr(z), N.ptr(z), 1, 8, 64, L, T, N.ptr(out), N.stream_ptr(cuda_device))
        torch.cuda.synchronize(cuda_device)
        assert bool((out == 7.0).all())
        return s

    assert st(N.XTTS_COND_MAX_LATENTS + 1, 4) == N.TTS_ERR_UNSUPPORTED
    assert st(32, N.XTTS_COND_MAX_KEYS - 31) == N.TTS_ERR_UNSUPPORTED
    assert st(0, 4) == N.TTS_ERR_INVALID


# ------------------------------------------------------------------------------- feed-forward, RMSNorm
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E,I", [(128, 341), (96, 256), (1024, 2730)])
def test_feed_forward_geglu_op_vs_fp64(cuda_device, E, I, B, mode):
    L = 32
    x = rnd(B, E, L, seed=I + B)
    w0, b0 = rnd(2 * I, E, seed=1, std=1.0 / E**0.5), rnd(2 * I, seed=2, std=0.1)
    w2, b2 = rnd(E, I, seed=3, std=1.5 / I**0.5), rnd(E, seed=4, std=0.1)
    out = XC.perceiver_feed_forward(x.to(cuda_device), w0, b0, w2, b2, math_mode=mode)
    ref = R.feed_forward(w0.double(), b0.double(), w2.double(), b2.double(), x.double().transpose(1, 2)).transpose(1, 2)
    assert_close_fp32(out.cpu(), ref, f"perceiver ff {mode} I={I} B={B}", **tol(mode, op=True))


def test_rmsnorm_with_an_all_zero_row(cuda_device):
    B, E, L = 2, 96, 7
    x = rnd(B, E, L, seed=9)
    x[1, :, 4] = 0.0
    gamma = 1.0 + rnd(E, seed=10, std=0.1)
    y = XC.rms_norm(x.to(cuda_device), gamma).cpu()
    ref = R.rms_norm(x.double().transpose(1, 2), gamma.double()).transpose(1, 2)
    assert torch.isfinite(y).all() and bool((y[1, :, 4] == 0).all())
    assert_close_fp32(y, ref, "rmsnorm", **tol("fp32", op=True))


# ------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("n", [7277, 132300, 132301])
def test_mel_front_end_vs_fp64(cuda_device, n):
    """A 1 kHz sine plus noise, and digital silence in the second row: that row is log(1e-5) / mel_norms."""
    m = model("narrow32", cuda_device)
    wav = torch.cat((C.clip(n, seed=n), torch.zeros(1, n)))
    norms = C.mel_norms()
    mel = m.wav_to_mel_cloning(wav.to(cuda_device), norms).cpu()
    T = {7277: 29, 132300: 517, 132301: 517}[n]
    assert mel.shape == (2, 80, T)
    assert_close_fp32(mel, R.wav_to_mel_cloning(wav, norms), f"mel cloning N={n}", **tol("fp32", op=True))
    # the silent row: every frame the same bits, log(1e-5f) / mel_norms in fp32 (the device's logf and its
    # division may each differ from the host's by an ulp: 2 ulps of the fp32 value, against the fp64 one)
    silent = math.log(1e-5) / norms.double()
    assert bool((mel[1] == mel[1, :, :1]).all())
    assert bool(((mel[1, :, 0].double() - silent).abs() <= 2 * 2.0**-23 * silent.abs()).all())
    again = audio.wav_to_mel_cloning(wav.to(cuda_device), mel_norms=norms)  # the reference's signature
    assert torch.equal(again.cpu(), mel)


def test_mel_front_end_limits(cuda_device):
    m = model("narrow32", cuda_device)
    with pytest.raises(N.NativeError) as e:
        m.wav_to_mel_cloning(torch.zeros(1, 1024, device=cuda_device), C.mel_norms())
    assert e.value.code == N.TTS_ERR_UNSUPPORTED and "n_fft / 2 + 1" in str(e.value)
    with pytest.raises(NotImplementedError):
        audio.wav_to_mel_cloning(torch.zeros(1, 4096, device=cuda_device), "mel_stats.pth")
    # another plan: n_fft 1024, window 512 (T = 1 + N // 256 all the same)
    other = audio.wav_to_mel_cloning(C.clip(4096).to(cuda_device), mel_norms=C.mel_norms(), n_fft=1024, win_length=512)
    assert other.shape == (1, 80, 17) and torch.isfinite(other).all()


@pytest.mark.parametrize("n", [1, 440, 441, 442, 44100])
@pytest.mark.parametrize("orig,new", [(22050, 16000), (24000, 22050)])
def test_resample_vs_fp64(cuda_device, orig, new, n):
    x = torch.cat((C.clip(n, seed=n, sr=orig), C.clip(n, seed=n + 1, sr=orig)))
    y = audio.resample(x.to(cuda_device), orig, new).cpu()
    table = R.resample_table(orig, new)
    _, o, nn_, _ = table
    assert y.shape == (2, -(-nn_ * n // o))
    assert_close_fp32(y, R.resample(x, orig, new, table=table), f"resample {orig}->{new} N={n}", **tol("fp32", op=True))


@pytest.mark.parametrize("orig,new", [(22050, 16000), (24000, 22050)])
def test_resample_impulse_reproduces_the_table(cuda_device, orig, new):
    kern, o, n, w = R.resample_table(orig, new)
    N_, i0 = 3 * o + 5, o + 2
    x = torch.zeros(1, N_)
    x[0, i0] = 1.0
    y = audio.resample(x.to(cuda_device), orig, new).cpu()[0]
    want = torch.zeros_like(y)
    for i in range(y.numel()):
        f, p = divmod(i, n)
        k = i0 + w - f * o
        if 0 <= k < 2 * w + o:
            want[i] = kern[p, k].float()
    assert float((y - want).abs().max()) <= 1e-7  # the two hosts' sin / cos may differ in the last fp64 bit


def test_resample_limits_and_identity(cuda_device):
    x = torch.zeros(1, 100, device=cuda_device)
    assert audio.resample(x, 22050, 22050) is x
    with pytest.raises(N.NativeError) as e:
        audio.resample(x, 22051, 16000)  # coprime: 22051 phases
    assert e.value.code == N.TTS_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError):
        audio.resample(torch.zeros(1, 100), 22050, 16000)


# --------------------------------------------------------------------------------------- get_style_emb
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("T", C.STYLE_T)
@pytest.mark.parametrize("name", list(C.MODELS))
def test_get_style_emb_vs_fp64(cuda_device, name, T, mode):
    """B = 2 and B = 1 against the oracle; row b of the batch of two is bitwise its own batch of one, and a
    second call returns the same bits."""
    m = model(name, cuda_device, mode)
    mel = C.mel_input(T).to(cuda_device)
    ref = C.style_oracle(name, T)
    out = m.get_style_emb(mel)
    assert out.shape == (2, C.MODELS[name]["model_dim"], C.NUM_LATENTS)
    ma, rr = assert_close_fp32(out.cpu(), ref, f"style emb {name} {mode} T={T}", **tol(mode))
    print(f"style emb {name} {mode} T={T}: max|d| {ma:.2e} rel-RMS {rr:.2e}")
    for b in range(2):
        one = m.get_style_emb(mel[b : b + 1].unsqueeze(1))  # [1, 1, 80, T] is squeezed
        assert torch.equal(one[0], out[b])
    assert torch.equal(m.get_style_emb(mel), out)


def test_style_emb_launch_records(cuda_device):
    m = model("narrow", cuda_device)
    out, rows = m.get_style_emb(C.mel_input(65).to(cuda_device), profile=True)
    assert torch.equal(out, m.get_style_emb(C.mel_input(65).to(cuda_device)))
    names = [r["name"] for r in rows]
    block = ["group_norm", "qkv", "attention", "proj_out"]
    layer = ["to_q", "to_kv_latents", "to_kv_context", "cross_attention", "to_out", "ff_in_geglu", "ff_out"]
    assert names == ["init"] + 2 * block + ["latents"] + 2 * layer + ["rms_norm"]
    assert all(r["ms"] > 0 for r in rows)


def test_style_emb_limits_leave_the_output_untouched(cuda_device):
    m = model("narrow32", cuda_device)
    h = m._native_handle()
    lib = N.lib()
    out = torch.full((1, 96, 32), 7.0, device=cuda_device)
    mel = torch.zeros(1, 80, 8, device=cuda_device)
    for B, T, code in ((N.XTTS_COND_MAX_BATCH + 1, 8, N.TTS_ERR_UNSUPPORTED), (1, N.XTTS_COND_MAX_KEYS, N.TTS_ERR_UNSUPPORTED),
                       (0, 8, N.TTS_ERR_INVALID)):
        st = lib.tts_xtts_cond_style_emb(h, N.ptr(mel), B, T, N.ptr(out), N.stream_ptr(cuda_device))
        torch.cuda.synchronize(cuda_device)
        assert st == code and bool((out == 7.0).all())
    with pytest.raises(ValueError):
        m.get_style_emb(torch.zeros(1, 64, 8, device=cuda_device))
    with pytest.raises(RuntimeError):
        m.get_style_emb(torch.zeros(1, 80, 8))


# ------------------------------------------------------------------------------------------------ Xtts
DEC = dict(decoder_input_dim=128, upsample_rates_decoder=(8, 8, 2, 2), upsample_initial_channel_decoder=128,
           upsample_kernel_sizes_decoder=(16, 16, 4, 4), d_vector_dim=64)
DEC_CFG = dict(in_channels=128, out_channels=1, resblock_type="1", resblock_dilation_sizes=[[1, 3, 5]] * 3,
               resblock_kernel_sizes=[3, 7, 11], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=128,
               upsample_factors=[8, 8, 2, 2], inference_padding=0, cond_channels=64, conv_pre_weight_norm=False,
               conv_post_weight_norm=False, conv_post_bias=False, cond_in_each_up_layer=True)
_XTTS = {}


def xtts(dev):
    """Xtts on the narrow GPT, the narrow conditioning modules, a narrow decoder and the small speaker encoder."""
    if "x" not in _XTTS:
        cfg = GC.MODELS["narrow"]
        gpt = XttsGPT(**GC.ctor_kwargs(cfg), math_mode="fp32")
        gpt.load_state_dict(GC.state_dict(cfg, GC.MODEL_SEED["narrow"]), strict=True)
        dec = HifiDecoder(**DEC, math_mode="fp32")
        dec.waveform_decoder.load_state_dict(synthetic.hifigan_state_dict(**DEC_CFG, seed=98, weight_norm=True))
        spk = ResNetSpeakerEncoder(**SC.MODELS["small"], math_mode="fp32")
        spk.load_state_dict(SC.state_dict("small"))
        dec.speaker_encoder = spk
        _XTTS["x"] = Xtts(gpt.eval(), dec.eval(), gpt_max_new_tokens=8, conditioning=model("narrow", dev),
                          mel_stats=C.mel_norms()).to(dev)
    return _XTTS["x"]


@pytest.mark.parametrize("seconds,chunks", [(13.2, 3), (6.2, 1)])
def test_get_gpt_cond_latents_chunk_mean(cuda_device, seconds, chunks):
    """13.2 s: chunks of 6 s, 6 s and 1.2 s; 6.2 s: the 0.2 s rest is skipped."""
    x = xtts(cuda_device)
    wav = C.clip(int(round(seconds * 22050)), seed=3)
    lat = x.get_gpt_cond_latents(wav.to(cuda_device), 22050, length=30, chunk_length=6)
    ref, n = R.gpt_cond_latents(C.state_dict("narrow"), wav, 22050, C.mel_norms(), 2, length=30, chunk_length=6)
    assert n == chunks and lat.shape == (1, 32, 128) and lat.device.type == "cuda"
    assert_close_fp32(lat.cpu(), ref, f"gpt cond latents {seconds} s", **tol("fp32"))


def test_get_gpt_cond_latents_resamples_and_cuts(cuda_device):
    x = xtts(cuda_device)
    wav = C.clip(36000, seed=4, sr=24000)  # 1.5 s at 24 kHz, cut to 1 s after the resample
    lat = x.get_gpt_cond_latents(wav.to(cuda_device), 24000, length=1, chunk_length=6)
    ref, n = R.gpt_cond_latents(C.state_dict("narrow"), wav, 24000, C.mel_norms(), 2, length=1, chunk_length=6)
    assert n == 1
    assert_close_fp32(lat.cpu(), ref, "gpt cond latents 24 kHz", **tol("fp32"))


@pytest.mark.parametrize("sound_norm_refs", [False, True])
def test_get_conditioning_latents_and_inference(cuda_device, sound_norm_refs):
    """Two clips: the latent of their concatenation and the mean d-vector against the oracle, and
    Xtts.inference on that pair bitwise the inference on the separately computed tensors."""
    x = xtts(cuda_device)
    clips = [C.clip(33075, seed=5), C.clip(22050, seed=6, amp=0.2)]  # 1.5 s and 1 s
    lat, g = x.get_conditioning_latents([c.to(cuda_device) for c in clips], sound_norm_refs=sound_norm_refs)
    assert lat.shape == (1, 32, 128) and g.shape == (1, 64, 1)
    ref_clips = [(c.double() / c.double().abs().max() * 0.75) if sound_norm_refs else c.double() for c in clips]
    ref_lat, _ = R.gpt_cond_latents(C.state_dict("narrow"), torch.cat(ref_clips, dim=-1), 22050, C.mel_norms(), 2,
                                    length=6, chunk_length=6)
    assert_close_fp32(lat.cpu(), ref_lat, f"conditioning latents norm={sound_norm_refs}", **tol("fp32"))
    embs = [SR.forward(SC.state_dict("small"), R.resample(c, 22050, 16000), l2_norm=True, dtype=torch.float64,
                       **SC.ref_kwargs("small")) for c in ref_clips]
    ref_g = ((embs[0] + embs[1]) / 2).unsqueeze(-1)
    assert_close_fp32(g.cpu(), ref_g, f"conditioning d-vector norm={sound_norm_refs}", **tol("fp32"))
    # the same pair from the separate entry points
    dev_clips = [c.to(cuda_device) for c in clips]
    if sound_norm_refs:
        dev_clips = [(c / c.abs().max()) * 0.75 for c in dev_clips]
    lat2 = x.get_gpt_cond_latents(torch.cat(dev_clips, dim=-1), 22050, length=6, chunk_length=6)
    g2 = (x.get_speaker_embedding(dev_clips[0], 22050) + x.get_speaker_embedding(dev_clips[1], 22050)) / 2
    assert torch.equal(lat, lat2) and torch.equal(g, g2)
    _, text = GC.inputs(GC.MODELS["narrow"], 1, 1, 7)
    a = x.inference(text, lat, g, do_sample=False)
    b = x.inference(text, lat2.clone(), g2.clone(), do_sample=False)
    assert torch.equal(a["wav"], b["wav"]) and torch.equal(a["gpt_codes"], b["gpt_codes"])
    assert a["wav"].shape[0] == 1 and torch.isfinite(a["wav"]).all()


def test_excluded_and_missing_parts_raise(cuda_device):
    x = xtts(cuda_device)
    wav = C.clip(22050).to(cuda_device)
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        x.get_conditioning_latents("speaker.wav")
    with pytest.raises(NotImplementedError, match="DESIGN.md section 8"):
        x.get_conditioning_latents(wav, librosa_trim_db=30)
    bare = Xtts(x.gpt, HifiDecoder(**DEC, math_mode="fp32"))
    with pytest.raises(RuntimeError, match="conditioning"):
        bare.get_gpt_cond_latents(wav, 22050)
    with pytest.raises(RuntimeError, match="speaker encoder"):
        bare.get_speaker_embedding(wav, 22050)


def test_checkpoint_slice_runs_like_the_state_dict(cuda_device, tmp_path):
    """XttsConditioning.load_checkpoint on a synthetic full checkpoint, then XttsGPT.load_checkpoint on the same
    file: both strict, the GPT's tree unchanged, and the loaded conditioning module computes the same bits."""
    cfg = GC.MODELS["narrow"]
    gpt_sd = GC.state_dict(cfg, GC.MODEL_SEED["narrow"])
    path = tmp_path / "model.pth"
    torch.save({"model": C.full_checkpoint("narrow", gpt_sd)}, path)
    m = XttsConditioning(**C.ctor_kwargs("narrow"), math_mode="fp32")
    m.load_checkpoint(path)
    gpt = XttsGPT(**GC.ctor_kwargs(cfg), math_mode="fp32")
    gpt.load_checkpoint(path, strict=True)
    assert set(gpt.state_dict()) == set(gpt_sd)
    assert all(torch.equal(gpt.state_dict()[k], v) for k, v in gpt_sd.items())
    mel = C.mel_input(29).to(cuda_device)
    assert torch.equal(m.to(cuda_device).get_style_emb(mel), model("narrow", cuda_device).get_style_emb(mel))
