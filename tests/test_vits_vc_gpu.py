"""VITS voice conversion on MI355X: the linear-spectrogram kernel (``wav_to_spec``) against ``torch.stft``
in fp64 on the CPU, and ``Vits.voice_conversion`` / ``Vits.inference_voice_conversion`` against the fp64
oracle chain (tests/_vc_chain.py)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _util import FP32_MAX_ABS, FP32_REL_RMS, assert_close_fp32, max_abs, rel_rms, tol
from _vc_chain import oracle_vc, signal, spec_ref, state_dicts, vits_args
from tts_amd import _native as NATIVE
from tts_amd.tts import Vits, spectrogram, wav_to_spec

pytestmark = pytest.mark.gpu

# (n_fft, hop, win, B, N, signal); the kernel's frame tile is 32 frames, or 64 with two column blocks
# per wave (TTS_MI355X_STFT_TN forces either): the last four cases put BN + 1 and 2 BN + 5 frames on both
CASES = {
    "vits_b2": (1024, 256, 1024, 2, 256 * 37, "noise"),
    "sines": (1024, 256, 1024, 1, 256 * 33 + 100, "sines"),
    "win800": (1024, 256, 800, 1, 5000, "noise"),
    "fft512_b3": (512, 128, 512, 3, 128 * 9 + 5, "noise"),
    "two_frames": (1024, 256, 1024, 1, 640, "noise"),    # both reflections reach into the same frames
    "one_frame": (1024, 256, 1024, 1, 385, "noise"),     # the smallest legal N
    "hop512": (1024, 512, 1024, 1, 4096, "noise"),
    "hop264": (1024, 264, 1024, 1, 5000, "noise"),       # hop does not divide n_fft; p = 380
    "tile32_plus1": (1024, 256, 1024, 1, 256 * 33, "noise"),
    "tile32_x2_plus5": (1024, 256, 1024, 1, 256 * 69, "noise"),
    "tile64_plus1": (1024, 256, 1024, 1, 256 * 65, "noise"),
    "tile64_x2_plus5": (1024, 256, 1024, 2, 256 * 133 + 17, "noise"),
}
TILE = {"tile32_plus1": "1", "tile32_x2_plus5": "1", "tile64_plus1": "2", "tile64_x2_plus5": "2"}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(wav fp32 [B, N], fp64 reference, E32 = max error of the reference's own fp32 path), computed once."""
    n_fft, hop, win, B, N, kind = CASES[name]
    y = signal(kind, B, N, seed=len(name))
    ref = spec_ref(y, n_fft, hop, win, torch.float64)
    e32 = max_abs(spec_ref(y, n_fft, hop, win, torch.float32).numpy(), ref.numpy())
    return y, ref, e32


def _spec(name, mode, dev):
    n_fft, hop, win, B, N, _ = CASES[name]
    y = _case(name)[0].to(dev)
    return wav_to_spec(y.unsqueeze(1), n_fft, hop, win, center=False, math_mode=mode)


def _spec_into_nan(name, mode, dev, stride=0):
    """The C-ABI call itself, into an output pre-filled with NaN; stride > N: the rows lie that many floats
    apart in a NaN-filled buffer."""
    n_fft, hop, win, B, N, _ = CASES[name]
    y = _case(name)[0]
    if stride:
        buf = torch.full((B, stride), float("nan"))
        buf[:, :N] = y
        y = buf
    y = y.to(dev)
    plan = spectrogram._plan(n_fft, hop, win, mode, dev)
    out = torch.full((B, n_fft // 2 + 1, plan.num_frames(N)), float("nan"), device=dev)
    NATIVE.call("tts_stft_forward", plan.handle, NATIVE.ptr(y), B, N, stride, NATIVE.ptr(out), NATIVE.stream_ptr(dev))
    return out


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("mode", ["fp32x6", "f16x3", "bf16"])
def test_wav_to_spec_vs_stft(cuda_device, monkeypatch, mode, name):
    """fp32x6 / f16x3: rel-RMS <= 5e-6 and max|d| <= max(1e-4, 5 E32), E32 the error of torch.stft's own
    fp32 CPU path on the same input (the factor _util.py keeps between its gate and the reference's fp32
    forward); bf16: the bf16 op gate."""
    n_fft, hop, win, B, N, _ = CASES[name]
    y, ref, e32 = _case(name)
    assert ref.shape == (B, n_fft // 2 + 1, 1 + (N + 2 * int((n_fft - hop) / 2) - n_fft) // hop)
    if name in TILE:
        monkeypatch.setenv("TTS_MI355X_STFT_TN", TILE[name])
    out = _spec_into_nan(name, mode, cuda_device)  # every element must be written: NaN fails the gate
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert torch.equal(out, _spec(name, mode, cuda_device)), "wav_to_spec differs from the C-ABI call"
    o = out.cpu().numpy()
    ma, rr = max_abs(o, ref.numpy()), rel_rms(o, ref.numpy())
    print(f"wav_to_spec {name} {mode}: max|d|={ma:.3e} rel-RMS={rr:.3e} E32={e32:.3e} max|ref|={float(ref.max()):.4g}")
    if mode == "bf16":
        gate = tol("bf16", op=True)
    else:
        gate = dict(max_abs_tol=max(FP32_MAX_ABS, 5 * e32), rel_rms_tol=FP32_REL_RMS)
    assert_close_fp32(o, ref.numpy(), f"wav_to_spec {name} ({mode})", **gate)


@pytest.mark.parametrize("mode", ["fp32x6", "f16x3", "bf16"])
def test_wav_to_spec_strided_rows(cuda_device, mode):
    """Rows a stride apart in a wider (NaN-filled) buffer give the bits of the packed wav."""
    N = CASES["fft512_b3"][4]
    out = _spec_into_nan("fft512_b3", mode, cuda_device, stride=N + 11)
    assert torch.isfinite(out).all()
    assert torch.equal(out, _spec("fft512_b3", mode, cuda_device))


@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
def test_wav_to_spec_batch_invariant(cuda_device, mode):
    n_fft, hop, win, B, N, _ = CASES["fft512_b3"]
    y = _case("fft512_b3")[0].to(cuda_device)
    a = wav_to_spec(y, n_fft, hop, win, math_mode=mode)
    b = wav_to_spec(y, n_fft, hop, win, math_mode=mode)
    assert torch.equal(a, b)
    for i in range(B):
        assert torch.equal(wav_to_spec(y[i:i + 1], n_fft, hop, win, math_mode=mode)[0], a[i]), f"row {i}"


def test_wav_to_spec_tile_shape_invariant(cuda_device, monkeypatch):
    """32- and 64-frame tiles give the same bits (one k order per output, whatever the launch shape)."""
    y = _case("tile64_x2_plus5")[0].to(cuda_device)
    outs = []
    for tn in ("1", "2"):
        monkeypatch.setenv("TTS_MI355X_STFT_TN", tn)
        outs.append(wav_to_spec(y, 1024, 256, 1024, math_mode="f16x3"))
    assert torch.equal(outs[0], outs[1])


def test_wav_to_spec_rejects(cuda_device):
    with pytest.raises(ValueError):
        wav_to_spec(torch.zeros(1, 1, 384, device=cuda_device), 1024, 256, 1024)
    with pytest.raises(NotImplementedError):
        wav_to_spec(torch.zeros(1, 1, 4096, device=cuda_device), 1024, 256, 1024, center=True)
    assert wav_to_spec(torch.zeros(1, 1, 385, device=cuda_device), 1024, 256, 1024).shape == (1, 513, 1)


def test_wav_to_spec_zero_bins(cuda_device):
    """Bins that are exactly zero come out as sqrt(1e-6) = 1e-3."""
    out = wav_to_spec(torch.zeros(2, 4096, device=cuda_device), 1024, 256, 1024)
    assert torch.allclose(out, torch.full_like(out, 1e-3), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------ voice conversion
GIN = 16


def _model(dev, mode, by_id):
    v = Vits(vits_args(GIN, by_id), flow_math_mode=mode, decoder_math_mode=mode, posterior_math_mode=mode)
    psd, fsd, dsd = state_dicts(GIN)
    v.posterior_encoder.load_state_dict(psd)
    v.flow.load_state_dict(fsd)
    v.waveform_decoder.load_state_dict(dsd)
    if by_id:
        g = torch.Generator().manual_seed(21)
        v.emb_g.weight.data.copy_(torch.randn(5, GIN, generator=g))
    return v.to(dev)


def _check_chain(mode, what, got, ref):
    """z, z_p, z_hat at the op gate, the waveform at the project's waveform gate (measured on MI355X in f16x3:
    wav max|d| 6.6e-7, rel-RMS 4.7e-7; the fp32 oracle chain itself is 5.4e-7 / 4.2e-7 off fp64)."""
    wav_gate = tol(mode)
    (z, z_p, z_hat), wav = got
    zr, zpr, zhr, wr = ref
    for name, a, b in (("z", z, zr), ("z_p", z_p, zpr), ("z_hat", z_hat, zhr)):
        print(f"{what} {name} ({mode}): max|d|={max_abs(a.cpu().numpy(), b.numpy()):.3e} "
              f"rel-RMS={rel_rms(a.cpu().numpy(), b.numpy()):.3e}")
    print(f"{what} wav ({mode}): max|d|={max_abs(wav.cpu().numpy(), wr.numpy()):.3e} "
          f"rel-RMS={rel_rms(wav.cpu().numpy(), wr.numpy()):.3e} gate {wav_gate}")
    for name, a, b in (("z", z, zr), ("z_p", z_p, zpr), ("z_hat", z_hat, zhr)):
        assert_close_fp32(a.cpu(), b, f"{what} {name} ({mode})", **tol(mode, op=True))
    assert_close_fp32(wav.cpu(), wr, f"{what} wav ({mode})", **wav_gate)


@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
def test_voice_conversion_from_spec(cuda_device, mode):
    gen = torch.Generator().manual_seed(5)
    B, T = 2, 37
    lengths = torch.tensor([37, 21])
    y = torch.randn(B, 513, T, generator=gen).abs()
    eps = torch.randn(B, 192, T, generator=gen)
    d_src, d_tgt = torch.randn(B, GIN, generator=gen), torch.randn(B, GIN, generator=gen)
    g_src, g_tgt = F.normalize(d_src.double()).unsqueeze(-1), F.normalize(d_tgt.double()).unsqueeze(-1)
    sds = state_dicts(GIN)
    zr, zpr, zhr, wr, mr = oracle_vc(sds, y, lengths, eps, g_src, g_tgt)
    v = _model(cuda_device, mode, by_id=False)
    o_hat, y_mask, zs = v.voice_conversion(y.to(cuda_device), lengths.to(cuda_device), d_src.to(cuda_device),
                                           d_tgt.to(cuda_device), noise=eps.to(cuda_device))
    assert o_hat.shape == (B, 1, T * 256)
    assert torch.equal(y_mask.cpu().double(), mr)
    _check_chain(mode, "vc from spec", (zs, o_hat), (zr, zpr, zhr, wr))


@pytest.mark.parametrize("by_id", [True, False], ids=["speaker_ids", "d_vectors"])
def test_inference_voice_conversion_wav_to_wav(cuda_device, by_id):
    mode = "f16x3"
    N = 256 * 24 + 57
    wav = signal("noise", 1, N, seed=77)
    y64 = spec_ref(wav, 1024, 256, 1024, torch.float64)
    T = y64.shape[-1]
    assert T == 24
    gen = torch.Generator().manual_seed(9)
    eps = torch.randn(1, 192, T, generator=gen)
    v = _model(cuda_device, mode, by_id)
    if by_id:
        kw = dict(reference_speaker_id=1, speaker_id=3)
        table = v.emb_g.weight.detach().cpu().double()
        g_src, g_tgt = table[1].reshape(1, GIN, 1), table[3].reshape(1, GIN, 1)
    else:
        d_src, d_tgt = torch.randn(1, GIN, generator=gen), torch.randn(1, GIN, generator=gen)
        kw = dict(reference_d_vector=d_src.to(cuda_device), d_vector=d_tgt.to(cuda_device))
        g_src, g_tgt = F.normalize(d_src.double()).unsqueeze(-1), F.normalize(d_tgt.double()).unsqueeze(-1)
    sds = state_dicts(GIN)
    lengths = torch.tensor([T])
    zr, zpr, zhr, wr, _ = oracle_vc(sds, y64, lengths, eps, g_src, g_tgt)
    # the public method draws the posterior's noise itself: inject the test's through a wrapper
    seen = {}
    forward = v.posterior_encoder.forward

    def seeded(y, y_lengths, g=None, noise=None):
        seen["y"] = y
        return forward(y, y_lengths, g=g, noise=eps.to(cuda_device))

    v.posterior_encoder.forward = seeded
    out = v.inference_voice_conversion(wav.unsqueeze(1).to(cuda_device), **kw)
    assert out.shape == (1, 1, 24 * 256)
    assert_close_fp32(seen["y"].cpu(), y64, "vc spectrogram", max_abs_tol=FP32_MAX_ABS, rel_rms_tol=FP32_REL_RMS)
    ma, rr = max_abs(out.cpu().numpy(), wr.numpy()), rel_rms(out.cpu().numpy(), wr.numpy())
    gate = tol(mode)
    print(f"wav-to-wav ({'ids' if by_id else 'd-vectors'}): max|d|={ma:.3e} rel-RMS={rr:.3e} gate {gate}")
    assert_close_fp32(out.cpu(), wr, f"vc wav-to-wav ({'ids' if by_id else 'd-vectors'})", **gate)


def test_voice_conversion_same_speaker_roundtrip(cuda_device):
    gen = torch.Generator().manual_seed(6)
    B, T = 2, 37
    y = torch.randn(B, 513, T, generator=gen).abs()
    d = torch.randn(B, GIN, generator=gen)
    v = _model(cuda_device, "f16x3", by_id=False)
    _, y_mask, (z, _, z_hat) = v.voice_conversion(y.to(cuda_device), torch.tensor([37, 21]), d, d)
    assert torch.allclose(z_hat * y_mask, z * y_mask, atol=1e-4)
    assert float((z * y_mask).abs().max()) > 0.1


def test_inference_does_not_touch_posterior(cuda_device):
    v = _model(cuda_device, "f16x3", by_id=False)
    tokens = torch.tensor([[1, 5, 3, 7, 2, 9]], device=cuda_device)
    d = torch.randn(1, GIN, generator=torch.Generator().manual_seed(3))
    out = v.inference(tokens, aux_input={"d_vectors": d.to(cuda_device),
                                         "durations": torch.full((6,), 2.0, device=cuda_device)})
    assert out["model_outputs"].shape == (1, 1, 12 * 256)
    assert v.posterior_encoder._handle is None
    assert v.flow._handle is not None
