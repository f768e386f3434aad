"""The speaker encoder on MI355X.  The Conv2d kernel of its SE-ResNet trunk against torch's fp64
``F.conv2d``: exact-integer data at every tile edge (bitwise in every math mode), random data at the
trunk's widths, repeatability and batch invariance, and the limits.  Then the encoder against the fp64
oracle (tests/_speaker_encoder_ref.py): the centred STFT, the front end, the models in both math modes,
bitwise repeatability and batch invariance, compute_embedding, the XTTS chain and the input limits.
Gates: tests/_util.py tol(mode) on L2-normalised embeddings and waveforms, tol(mode, op=True) on raw
embeddings, features and the conv op; every measured error is logged with log_error (TTS_ERRLOG)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import _speaker_encoder_cases as SC
import _speaker_encoder_ref as R
from _util import assert_close_fp32, goldens, log_error, max_abs, rel_rms, tol
from tts_amd import _native as N
from tts_amd import encoder, synthetic
from tts_amd.encoder import ResNetSpeakerEncoder
from tts_amd.tts import HifiDecoder

pytestmark = pytest.mark.gpu

ALL_MODES = ["fp32", "fp32x6", "f16x3", "bf16"]
# (Cin, Cout, ksize, stride, epilogue): the stem (bias + ReLU + affine), a 16-channel conv, the strided
# first conv of a layer, a full 64-channel conv (two staged chunks) and the downsample form
SHAPES = [(1, 16, 3, 1, True), (16, 16, 3, 1, False), (32, 64, 3, 2, False), (64, 64, 3, 1, False),
          (32, 64, 1, 2, False)]
SHAPE_IDS = ["stem_1_16", "c16_16", "c32_64_s2", "c64_64", "down_32_64_s2"]
ROWS = [1, 2, 8, 9]


def widths(stride):
    W = encoder.conv2d_tile()
    ts = {1, 2, W - 1, W, W + 1, 2 * W + 3}
    if stride == 2:  # the same edges on the output side: To = W - 1 .. W + 1, from even and odd T
        ts |= {2 * W - 2, 2 * W - 1, 2 * W, 2 * W + 1}
    return sorted(ts)


def reference(x, w, bias, stride, relu, scale, shift):
    """scale * act(conv2d(x, w, bias)) + shift in fp64."""
    k = w.shape[-1]
    y = F_.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride=stride, padding=(k - 1) // 2)
    if relu:
        y = torch.relu(y)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    return y


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def test_tile_is_64():
    assert encoder.conv2d_tile() == 64


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv_op_exact_integers(cuda_device, shape, mode):
    """Inputs in [-4, 4], weights in [-2, 2], integer bias / scale / shift: every product and partial
    sum is an integer below 2^24 and every operand has at most 3 significant bits, so the bf16 and
    the split operands are exact and any summation order gives the fp64 result bit for bit."""
    Cin, Cout, k, stride, epi = shape
    g = torch.Generator().manual_seed(1000 * Cin + Cout + k)
    w = ints(g, -2, 2, Cout, Cin, k, k)
    bias = ints(g, -3, 3, Cout) if epi else None
    scale = ints(g, -3, 3, Cout) if epi else None
    shift = ints(g, -5, 5, Cout) if epi else None
    for Fr in ROWS:
        for T in widths(stride):
            x = ints(g, -4, 4, 2, Cin, Fr, T)
            y = encoder.conv2d_3x3(x.to(cuda_device), w, bias, stride=stride, relu=epi, scale=scale, shift=shift,
                                   math_mode=mode).cpu()
            ref = reference(x, w, bias, stride, epi, scale, shift)
            assert y.shape == ref.shape == (2, Cout, -(-Fr // stride), -(-T // stride))
            assert torch.equal(y.double(), ref), f"{mode} {shape} F={Fr} T={T}: max|d|={(y.double() - ref).abs().max()}"


def random_case(Cin, Cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    bias = 0.1 * torch.randn(Cout, generator=g)
    scale = 0.8 + 0.4 * torch.rand(Cout, generator=g)
    shift = 0.1 * torch.randn(Cout, generator=g)
    return g, w, bias, scale, shift


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv_op_random(cuda_device, shape, mode):
    Cin, Cout, k, stride, epi = shape
    g, w, bias, scale, shift = random_case(Cin, Cout, k, 7 * Cin + Cout)
    if not epi:
        bias = None
    W = encoder.conv2d_tile()
    for Fr, T in [(1, 1), (2, W + 1), (8, 2 * W + 3), (9, W)]:
        x = torch.randn(2, Cin, Fr, T, generator=g)
        y = encoder.conv2d_3x3(x.to(cuda_device), w, bias, stride=stride, relu=epi, scale=scale, shift=shift, math_mode=mode)
        assert_close_fp32(y.cpu(), reference(x, w, bias, stride, epi, scale, shift),
                          f"conv2d {mode} {SHAPE_IDS[SHAPES.index(shape)]} F={Fr} T={T}", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
@pytest.mark.parametrize("C,stride", [(128, 1), (256, 1), (256, 2)])
def test_conv_op_random_wide(cuda_device, C, stride, mode):
    """The 128- and 256-channel layers (4 and 8 row blocks, 4 and 8 staged chunks) at F = 8."""
    g, w, _, scale, shift = random_case(C, C, 3, C + stride)
    x = torch.randn(2, C, 8, 70, generator=g)
    for relu in (True, False):
        y = encoder.conv2d_3x3(x.to(cuda_device), w, stride=stride, relu=relu, scale=scale, shift=shift, math_mode=mode)
        assert_close_fp32(y.cpu(), reference(x, w, None, stride, relu, scale, shift),
                          f"conv2d {mode} C={C} stride={stride} relu={relu}", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_conv_op_is_repeatable_and_batch_invariant(cuda_device, mode):
    g, w, bias, scale, shift = random_case(48, 80, 3, 5)
    x = torch.randn(3, 48, 5, 131, generator=g).to(cuda_device)
    run = lambda t: encoder.conv2d_3x3(t, w, bias, stride=2, relu=True, scale=scale, shift=shift, math_mode=mode)  # noqa: E731
    y = run(x)
    assert torch.equal(y, run(x))
    for b in range(3):
        assert torch.equal(y[b:b + 1], run(x[b:b + 1])), b


def test_conv_op_limits(cuda_device):
    """Every unsupported configuration is refused with TTS_ERR_UNSUPPORTED and a message that names
    the limit; the output tensor is left untouched (nothing was launched)."""
    x = torch.zeros(1, 4, 3, 5, device=cuda_device)
    cases = [
        (dict(w=torch.zeros(8, 4, 5, 5)), "3x3"),
        (dict(w=torch.zeros(8, 4, 3, 3), stride=3), "stride"),
        (dict(w=torch.zeros(4097, 4, 3, 3)), "[1, 4096]"),
    ]
    for kw, word in cases:
        with pytest.raises(N.NativeError) as e:
            encoder.conv2d_3x3(x, **kw)
        assert e.value.code == N.TTS_ERR_UNSUPPORTED and word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        encoder.conv2d_3x3(x, torch.zeros(8, 5, 3, 3))
    with pytest.raises(RuntimeError):
        encoder.conv2d_3x3(x.cpu(), torch.zeros(8, 4, 3, 3))
    # the raw entry: a sentinel-filled output survives a refused call
    out = torch.full((1, 8, 3, 5), 7.0, device=cuda_device)
    w = np.zeros((8, 4, 3, 3), np.float32)
    st = N.lib().tts_op_conv2d_3x3(N.ptr(x), 1, 4, 3, 5, N.ptr(w), 8, 3, 4, None, 0, None, None, N.MATH_MODES["bf16"],
                                   N.ptr(out), N.stream_ptr(cuda_device))
    assert st == N.TTS_ERR_UNSUPPORTED and b"stride" in N.lib().tts_last_error()
    assert bool((out == 7.0).all())


# ====================================================================== the encoder
MODEL_MODES = ["fp32x6", "bf16"]


@pytest.fixture(scope="module")
def models(cuda_device):
    cache = {}

    def get(model, mode="fp32x6"):
        if (model, mode) not in cache:
            m = ResNetSpeakerEncoder(**SC.MODELS[model], math_mode=mode)
            m.load_state_dict(SC.state_dict(model))
            cache[(model, mode)] = m.eval().to(cuda_device)
        return cache[(model, mode)]

    return get


# ------------------------------------------------------------------ centred STFT
@pytest.mark.parametrize("mode", ["fp32x6", "f16x3"])
def test_centered_stft_vs_torch(cuda_device, mode):
    """tts_stft_create_centered against torch.stft(center=True, pad_mode="reflect") in fp64, Hamming
    window of 400 in an n_fft of 512, at the shortest legal wav and across the 32-frame tile."""
    cfg = N.TtsStftCfg(512, 160, 400, N.MATH_MODES[mode])
    win = torch.hamming_window(400)
    h = ctypes.c_void_p()
    N.call("tts_stft_create_centered", ctypes.byref(cfg), N.ptr(win.numpy()), cuda_device.index or 0, ctypes.byref(h))
    try:
        for n in (257, 4800, 4960, 5120, 5920):
            y = SC.wav(3, n, seed=n)
            T = N.lib().tts_stft_num_frames_centered(ctypes.byref(cfg), n)
            assert T == 1 + n // 160
            yd = y.to(cuda_device)
            spec = torch.empty(3, 257, T, device=cuda_device)
            N.call("tts_stft_forward", h, N.ptr(yd), 3, n, n, N.ptr(spec), N.stream_ptr(cuda_device))
            X = torch.stft(y.double(), 512, hop_length=160, win_length=400, window=win.double(), center=True,
                           pad_mode="reflect", return_complex=True)
            ref = torch.sqrt(X.real**2 + X.imag**2 + 1e-6)
            assert_close_fp32(spec.cpu(), ref, f"stft centered {mode} N={n}", **tol(mode, op=True))
    finally:
        N.lib().tts_stft_destroy(h)


# ------------------------------------------------------------------ front end
# N = 257: the shortest legal wav (T = 2); 4800 / 4960 / 5120: T = 31 / 32 / 33 around the STFT's 32-frame tile
@pytest.mark.parametrize("n", [257, 1120, 4800, 4960, 5120, 5920])
def test_front_end_vs_oracle(cuda_device, models, n):
    """Log-mel + instance norm of the reference widths against fp64, B = 3.

    At N = 257 the instance norm runs over T = 2 frames, where it amplifies the log-mel's rounding
    by 1 / sigma: torch's own fp32 front end measures max|d| 1.02e-4 / rel-RMS 6.19e-6 against fp64
    there, above the project's gates (1e-4 / 5e-6), so that case is gated at twice those figures
    (2.04e-4 / 1.24e-5).  Every other length is held to tol("fp32", op=True)."""
    m = models("ref")
    x = SC.wav(3, n, seed=n)
    assert m.num_frames(n) == 1 + n // 160
    f = m.features(x.to(cuda_device))
    ref = SC.oracle_features("ref", 3, n)
    gate = dict(max_abs_tol=2.04e-4, rel_rms_tol=1.24e-5) if n == 257 else tol("fp32", op=True)
    assert_close_fp32(f.cpu(), ref, f"speaker front end N={n}", **gate)


def test_front_end_does_not_depend_on_the_math_mode(cuda_device, models):
    x = SC.wav(2, 5920, seed=1).to(cuda_device)
    assert torch.equal(models("ref", "fp32x6").features(x), models("ref", "bf16").features(x))


# ------------------------------------------------------------------ models
@pytest.mark.parametrize("mode", MODEL_MODES)
@pytest.mark.parametrize("run", list(SC.RUNS))
def test_model_vs_oracle(cuda_device, models, run, mode):
    """Raw embeddings within tol(mode, op=True), L2-normalised ones within tol(mode), of the fp64
    oracle (its own fp32 forward is 3.6e-6 / 6.5e-7 off on the raw `ref` embedding, its bf16-emulated
    convs 1.5e-2 / 3.1e-3)."""
    model, B, n = SC.RUNS[run]
    m = models(model, mode)
    x = SC.inputs(run).to(cuda_device)
    raw = m(x)
    assert raw.shape == (B, SC.MODELS[model]["proj_dim"])
    assert_close_fp32(raw.cpu(), SC.oracle(run), f"speaker encoder {run} {mode} raw", **tol(mode, op=True))
    nrm = m(x, l2_norm=True)
    assert_close_fp32(nrm.cpu(), SC.oracle(run, True), f"speaker encoder {run} {mode} l2", **tol(mode))
    assert torch.equal(m.inference(x), nrm)


@pytest.mark.parametrize("mode", MODEL_MODES)
@pytest.mark.parametrize("run", ["small", "ref"])
def test_model_is_repeatable_and_batch_invariant(cuda_device, models, run, mode):
    model, B, n = SC.RUNS[run]
    m = models(model, mode)
    x = SC.inputs(run).to(cuda_device)
    y = m(x)
    assert torch.equal(y, m(x))
    for b in range(B):
        assert torch.equal(y[b:b + 1], m(x[b:b + 1])), b


@pytest.mark.parametrize("return_mean", [True, False])
def test_compute_embedding_vs_oracle(cuda_device, models, return_mean):
    """A 3 s clip: 10 windows of 250 frames (40000 samples) spread over 48000 samples, one forward."""
    m = models("small")
    x = SC.wav(1, 48000, seed=5)
    e = m.compute_embedding(x.to(cuda_device), return_mean=return_mean)
    ref = R.compute_embedding(SC.state_dict("small"), x, hop_length=160, return_mean=return_mean, **SC.ref_kwargs("small"))
    assert e.shape == ((1, 64) if return_mean else (10, 64))
    assert_close_fp32(e.cpu(), ref, f"compute_embedding mean={return_mean}", **tol("fp32x6"))
    short = SC.wav(1, 20000, seed=6)  # shorter than a window: every window is the whole clip
    e = m.compute_embedding(short.to(cuda_device), return_mean=False)
    assert torch.equal(e, e[:1].expand(10, -1))


def test_profile_lists_the_launches(cuda_device, models):
    m = models("small")
    x = SC.inputs("small").to(cuda_device)
    out, rows = m.profile(x, l2_norm=True)
    assert torch.equal(out, m(x, l2_norm=True))
    names = [r["name"] for r in rows]
    assert names[:4] == ["preemphasis", "stft_fp32x6", "mel_filterbank", "log_instance_norm"] and names[-1] == "l2_norm"
    # 5 blocks, 3 of them with a downsample: 4 launches per block, 5 with the downsample
    trunk = names[5:names.index("attention0_c256")]
    assert len(trunk) == 2 * 4 + 3 * 5 and trunk.count("se_gate") == 5
    assert all(r["ms"] > 0 and r["flops"] > 0 for r in rows)


# ------------------------------------------------------------------ the XTTS chain
@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
def test_hifidecoder_speaker_embedding_chain(cuda_device, mode):
    name, meta, arr = goldens("xtts_decoder")[0]
    d = HifiDecoder(math_mode=mode, with_speaker_encoder=True)
    d.waveform_decoder.load_state_dict(synthetic.hifigan_state_dict(**meta["config"], seed=meta["seed"], weight_norm=True))
    d.speaker_encoder.load_state_dict(SC.state_dict("ref"))
    d = d.eval().to(cuda_device)
    wav = SC.inputs("ref").to(cuda_device)  # [2, 16000]
    g = d.speaker_embedding(wav)
    assert g.shape == (2, 512, 1) and g.device.type == "cuda"
    g_ref = SC.oracle("ref", True).unsqueeze(-1)
    ma, rr = max_abs(g.cpu().numpy(), g_ref.numpy()), rel_rms(g.cpu().numpy(), g_ref.numpy())
    log_error(f"xtts chain g {mode}", ma, rr)
    lat = torch.from_numpy(arr["latents"])
    assert lat.shape[0] == 2
    out = d(lat, g)
    ref = d(lat, g_ref.float().to(cuda_device))
    assert_close_fp32(out.cpu(), ref.cpu().double(), f"xtts chain wav {mode}", **tol(mode))


# ------------------------------------------------------------------ limits
def test_model_limits(cuda_device, models):
    """Inputs outside the limits are refused with TTS_ERR_UNSUPPORTED and a message that names the
    limit, before any launch (the output keeps its sentinel)."""
    m = models("small")
    h = m._native_handle()
    lib = N.lib()

    def refused(x, B, n, word):
        out = torch.full((max(B, 1), 64), 7.0, device=cuda_device)
        st = lib.tts_speaker_encoder_forward(h, N.ptr(x), B, n, 0, N.ptr(out), N.stream_ptr(cuda_device))
        assert st == N.TTS_ERR_UNSUPPORTED and word in lib.tts_last_error().decode(), lib.tts_last_error()
        torch.cuda.synchronize(cuda_device)
        assert bool((out == 7.0).all())

    x = torch.zeros(1, 256, device=cuda_device)
    refused(x, 1, 256, "fft_size / 2 + 1")
    with pytest.raises(N.NativeError) as e:
        m(x)
    assert e.value.code == N.TTS_ERR_UNSUPPORTED
    refused(x, N.SPK_MAX_BATCH + 1, 5920, "rows per forward")  # refused on the shape alone: x is not read
    refused(x, 1, 160 * N.SPK_MAX_FRAMES, "frames per forward")
    with pytest.raises(ValueError):
        m(torch.zeros(1, 16, 40, device=cuda_device))  # features into a wav model
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 5920))
