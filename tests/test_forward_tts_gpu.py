"""ForwardTTS (FastPitch) on MI355X against the fp64 oracle (tests/_forward_tts_ref.py, torch's own
``F.multi_head_attention_forward``): the self-attention op ``tts_op_mha`` (both kernels at the tile
edges, with and without the key padding mask, with scores whose range needs the running-max rescale,
bitwise batch invariance), one FFTransformerBlock through the executor, and the whole model.  Gates:
tests/_util.py tol(); every measured error is logged with log_error (TTS_ERRLOG)."""
import functools

import numpy as np
import pytest
import torch

import _forward_tts_cases as C
import _forward_tts_ref as R
from _util import assert_close_fp32, log_error, max_abs, rel_rms, tol
from tts_amd import _native as N
from tts_amd.tts import ForwardTTS, multi_head_attention
from tts_amd.tts.forward_tts import mha_tile

pytestmark = pytest.mark.gpu
SHAPES = [(64, 2), (256, 2), (384, 1), (384, 2)]  # (E, heads): head sizes 32, 128, 384, 192
B = 2


def lengths():
    W = mha_tile()
    return [1, 17, W - 1, W, W + 1, 2 * W + 5]


def key_length_cases(T):
    return [None, (T, 1), (T, max(1, T - 7))]


@functools.lru_cache(maxsize=None)
def case(E, heads, T, kl, qscale=1.0):
    """(qkv fp32, fp64 oracle output): computed once, shared by the modes."""
    g = torch.Generator().manual_seed(1000 * E + 10 * T + heads)
    qkv = torch.randn(B, 3 * E, T, generator=g)
    qkv[:, :E] *= qscale
    ref, _ = R.mha_from_qkv(qkv, heads, None if kl is None else torch.tensor(kl))
    return qkv, ref


def run(dev, qkv, heads, kl, mode):
    klt = None if kl is None else torch.tensor(kl, device=dev)
    return multi_head_attention(qkv.to(dev), heads, klt, math_mode=mode).cpu()


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
@pytest.mark.parametrize("E,heads", SHAPES)
def test_mha_op(cuda_device, E, heads, mode):
    assert mha_tile() == 64
    for T in lengths():
        for kl in key_length_cases(T):
            qkv, ref = case(E, heads, T, kl)
            out = run(cuda_device, qkv, heads, kl, mode)
            assert_close_fp32(out, ref, f"mha {mode} E={E} heads={heads} T={T} key_lengths={kl}", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_mha_wide_score_range(cuda_device, mode):
    """Scaled queries: the scores span more than 80, and the row maximum moves between key tiles.
    Scale 11: the scores of 2 x 133 x 133 normal draws range over about 8.4 sigma, so sigma = 11
    spans 92."""
    E, heads, T = 384, 1, 2 * mha_tile() + 5
    qkv, ref = case(E, heads, T, None, 11.0)
    s = R.scores(qkv, heads)
    assert (s.max() - s.min()).item() > 80.0
    # the row maximum moves to a later key tile for many queries: the rescale path runs
    first = s[..., : 32].max(-1).values
    assert ((s.max(-1).values - first) > 1.0).float().mean().item() > 0.25
    out = run(cuda_device, qkv, heads, None, mode)
    assert_close_fp32(out, ref, f"mha {mode} E={E} heads={heads} T={T} scores span > 80", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
@pytest.mark.parametrize("E,heads", [(384, 1), (64, 2)])
def test_mha_running_max_rescale(cuda_device, E, heads, mode):
    """Every query scores its first 40 keys about 100 below the others (one channel carries the
    offset; the other keys hold 0 there, so their scores are untouched in either arithmetic).  The
    first key tile alone sets a maximum near -100; the second raises it by 100: O and the running sum
    are rescaled by exp(-100), and exp() against the first tile's maximum would overflow fp32."""
    T, dk = 2 * mha_tile() + 5, E // heads
    qkv = case(E, heads, T, None)[0].clone()
    for h in range(heads):
        qkv[:, h * dk] = 16.0
        qkv[:, E + h * dk, :40] = -100.0 * dk**0.5 / 16.0
        qkv[:, E + h * dk, 40:] = 0.0
    s = R.scores(qkv, heads)
    assert (s[..., 40:].min(-1).values - s[..., :40].max(-1).values).min().item() > 80.0
    ref, _ = R.mha_from_qkv(qkv, heads)
    out = run(cuda_device, qkv, heads, None, mode)
    assert_close_fp32(out, ref, f"mha {mode} E={E} heads={heads} T={T} first tile 100 below", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_mha_masked_keys_contribute_nothing(cuda_device, mode):
    """Keys under the padding mask have probability exactly 0: their values do not reach the output,
    bitwise, whatever they hold."""
    E, heads, T = 384, 1, mha_tile() + 9
    kl = (T - 20, 3)
    qkv, _ = case(E, heads, T, kl)
    a = run(cuda_device, qkv, heads, kl, mode)
    other = qkv.clone()
    for b, n in enumerate(kl):
        other[b, E:, n:] = 1e30  # keys and values of the padded columns
    assert torch.equal(run(cuda_device, other, heads, kl, mode), a)


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_mha_batch_invariance(cuda_device, mode):
    """Item b of a B = 3 call is bitwise the B = 1 call at the same T."""
    E, heads, T = 384, 1, mha_tile() + 3
    qkv = torch.randn(3, 3 * E, T, generator=torch.Generator().manual_seed(5))
    kl = (T, 40, 7)
    full = run(cuda_device, qkv, heads, kl, mode)
    for b in range(3):
        one = run(cuda_device, qkv[b : b + 1], heads, kl[b : b + 1], mode)
        assert torch.equal(one[0], full[b]), f"item {b}"


def test_mha_default_mode_is_fp32_faithful(cuda_device):
    """fp32 and the package default f16x3 run the fp32x6 kernel."""
    E, heads, T = 256, 2, 17
    qkv, ref = case(E, heads, T, None)
    x6 = run(cuda_device, qkv, heads, None, "fp32x6")
    for mode in (None, "fp32", "f16x3"):
        assert torch.equal(run(cuda_device, qkv, heads, None, mode), x6)


def test_mha_long_sequence(cuda_device):
    """No whole-row buffer: a sequence past the text attention's 3072-column limit runs (100 key
    tiles of running max and sum)."""
    E, heads, T = 64, 2, 3200
    qkv = torch.randn(1, 3 * E, T, generator=torch.Generator().manual_seed(9))
    out = run(cuda_device, qkv, heads, None, "fp32x6")
    p = torch.softmax(R.scores(qkv, heads), -1)
    v = qkv[:, 2 * E :].double().reshape(1, heads, E // heads, T)
    ref = torch.einsum("bhij,bhdj->bhdi", p, v).reshape(1, E, T)
    assert_close_fp32(out, ref, f"mha fp32x6 E={E} heads={heads} T={T}", **tol("fp32", op=True))


def test_mha_rejects_before_launch(cuda_device):
    x = torch.zeros(1, 3 * 96, 8, device=cuda_device)
    with pytest.raises(N.NativeError) as e:
        multi_head_attention(x, 2)  # head size 48
    assert e.value.code == N.TTS_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError):
        multi_head_attention(torch.zeros(1, 192, 8), 2)  # a CPU tensor: no fallback


# ------------------------------------------------------------------ the executor
def build(name, dev, mode=None, mask_decoder_keys=False):
    m = ForwardTTS(C.ARGS[name], math_mode=mode, mask_decoder_keys=mask_decoder_keys)
    m.load_state_dict(C.state_dict(name))
    m.eval()
    return m.to(dev)


@pytest.fixture(scope="module")
def models(cuda_device):
    cache = {}

    def get(name, mode=None, mask_decoder_keys=False):
        key = (name, mode, mask_decoder_keys)
        if key not in cache:
            cache[key] = build(name, cuda_device, mode, mask_decoder_keys)
        return cache[key]

    return get


def close(out, ref, what, mode, gated=True):
    """assert_close_fp32 at the mode's gates; gated = False: measure and log only."""
    if gated:
        return assert_close_fp32(out, ref, what, **tol(mode))
    o, r = out.detach().cpu().numpy(), ref.detach().cpu().numpy()
    assert o.shape == r.shape and np.isfinite(o).all(), what
    log_error(what + " (logged, not gated)", max_abs(o, r), rel_rms(o, r), **tol(mode))


@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("decoder", [False, True])
def test_fft_block(cuda_device, models, name, decoder):
    """One FFTransformerBlock through the executor's block path, ragged key mask: every column is
    compared, the padded ones included (the reference masks nothing but the keys, and the k3 convs
    read the padded columns into the last valid ones).  The fastpitch widths run at the small depth
    (two layers); the whole-model test covers the six-layer stacks."""
    m = models(name, "fp32x6")
    for T in (1, 2, mha_tile() + 1):
        pre, p, x, kl, mask = C.block_case(name, decoder, T)
        with torch.no_grad():
            ref = R.fft_block(C.state_dict(name), pre, x, p["num_heads"], p["num_layers"], mask)
            ref_nomask = R.fft_block(C.state_dict(name), pre, x, p["num_heads"], p["num_layers"], None)
        what = f"fft_block {name} {'decoder' if decoder else 'encoder'} T={T}"
        assert_close_fp32(m.fft_block(x, kl, decoder=decoder).cpu(), ref, what + " ragged", **tol("fp32"))
        assert_close_fp32(m.fft_block(x, None, decoder=decoder).cpu(), ref_nomask, what + " no mask", **tol("fp32"))


def test_fft_block_bf16(cuda_device, models):
    m = models("small", "bf16")
    T = mha_tile() + 1
    pre, p, x, kl, mask = C.block_case("small", True, T)
    with torch.no_grad():
        ref = R.fft_block(C.state_dict("small"), pre, x, p["num_heads"], p["num_layers"], mask)
    assert_close_fp32(m.fft_block(x, kl, decoder=True).cpu(), ref, f"fft_block small decoder bf16 T={T}", **tol("bf16"))


def run_variant(m, name, variant, dev):
    kw = C.variant_kwargs(name, variant)
    aux = {"d_vectors": None, "speaker_ids": kw.get("speaker_ids")}
    if "x_lengths" in kw:
        aux["x_lengths"] = kw["x_lengths"]
    if "durations" in kw:
        aux["durations"] = kw["durations"]
    return m.inference(C.tokens(name).to(dev), aux)


def check_outputs(out, ref, what, mode, gated=True):
    assert set(out) == {"model_outputs", "alignments", "pitch", "energy", "durations_log"} and out["energy"] is None
    # durations and alignments: exact
    assert torch.equal(out["alignments"].cpu().double(), ref["alignments"]), what
    assert torch.equal(out["alignments"].sum(1).cpu().double(), ref["durations"]), what
    # the text side runs fp32x6 in every mode
    assert_close_fp32(out["pitch"].cpu(), ref["pitch"], what + " pitch", **tol("fp32"))
    assert_close_fp32(out["durations_log"].cpu(), ref["durations_log"], what + " durations_log", **tol("fp32"))
    close(out["model_outputs"].cpu(), ref["model_outputs"], what + " model_outputs", mode, gated)


@pytest.mark.parametrize("mode", [None, "fp32x6", "bf16"])
@pytest.mark.parametrize("variant", ["plain", "lengths", "durations", "plain+keys", "lengths+keys", "durations+keys"])
def test_small_model(cuda_device, models, variant, mode):
    """B = 3, T_en = 13, speaker ids; without and with x_lengths (13, 9, 1), with given durations, the
    decoder's keys unmasked (the reference) and masked."""
    m = models("small", mode, variant.endswith("+keys"))
    out = run_variant(m, "small", variant, cuda_device)
    check_outputs(out, C.reference("small", variant), f"forward_tts small {variant} {mode}", mode or "fp32")


@pytest.mark.parametrize("mode", [None, "bf16"])
def test_fastpitch_model(cuda_device, models, mode):
    """The FastPitch defaults (6 + 6 layers, one head of 384), B = 2, T_en = 11.  bf16 at this depth is
    logged, not gated: torch's own bf16 forward of the decoder is outside half the bf16 gate
    (test_forward_tts_cpu.py test_bf16_analogue_decides_the_bf16_gates).  Measured on MI355X: mel
    rel-RMS 2.4e-6, max|d| 9.6e-6 in the fp32-faithful mode (the max is close to its gate of 1e-5; the
    split conv kernels' accumulation, DESIGN.md section 4 "ForwardTTS"), bf16 6.0e-3 / 2.3e-2."""
    m = models("fastpitch", mode)
    out = run_variant(m, "fastpitch", "plain", cuda_device)
    gated = mode != "bf16" or C.BF16_GATED["fastpitch"]
    check_outputs(out, C.reference("fastpitch"), f"forward_tts fastpitch {mode}", mode or "fp32", gated)


def test_model_batch_invariance(cuda_device, models):
    """Item b of the B = 3 call is bitwise the B = 1 call (given durations: equal frame counts)."""
    m = models("small", None, True)
    tok = C.tokens("small").to(cuda_device)
    B, T = tok.shape
    dur = torch.full((B, T), 5)
    spk = torch.tensor(C.SMALL_SPEAKERS)
    full = m.inference(tok, {"speaker_ids": spk, "durations": dur})
    for b in range(B):
        one = m.inference(tok[b : b + 1], {"speaker_ids": spk[b : b + 1], "durations": dur[b : b + 1]})
        for k in ("model_outputs", "pitch", "durations_log", "alignments"):
            assert torch.equal(one[k][0], full[k][b]), (k, b)


def test_workspace_reuse(cuda_device, models):
    """A large call, then a small one, then the large one again on one handle: identical results."""
    m = models("small")
    spk = torch.tensor(C.SMALL_SPEAKERS)
    big = (C.tokens("small").to(cuda_device), {"speaker_ids": spk, "durations": torch.full((3, 13), 9)})
    small = (C.tokens("small")[:1, :4].to(cuda_device), {"speaker_ids": spk[:1], "durations": torch.full((1, 4), 1)})
    a = m.inference(*big)
    s1 = m.inference(*small)
    b = m.inference(*big)
    s2 = m.inference(*small)
    for k in ("model_outputs", "pitch", "durations_log", "alignments"):
        assert torch.equal(a[k], b[k]) and torch.equal(s1[k], s2[k]), k


def test_frame_limit_raises_before_launch(cuda_device, models):
    m = models("small")
    tok = C.tokens("small")[:1].to(cuda_device)
    dur = torch.zeros(1, 13, dtype=torch.int64)
    dur[0, 0] = 5001
    with pytest.raises(ValueError, match="5000"):
        m.inference(tok, {"speaker_ids": torch.tensor([0]), "durations": dur})
    # the library's own check
    h = m._native_handle()
    st = N.lib().tts_forward_tts_decode(h, N.ptr(tok), N.ptr(tok), N.ptr(tok), N.ptr(tok), 1, 13, 5001, 0, N.ptr(tok),
                                        None, N.ptr(tok), N.stream_ptr(cuda_device))
    assert st == N.TTS_ERR_INVALID and b"5000" in N.lib().tts_last_error()
    dur[0, 0] = 5000
    out = m.inference(tok, {"speaker_ids": torch.tensor([0]), "durations": dur})
    assert out["model_outputs"].shape == (1, 5000, 80) and torch.isfinite(out["model_outputs"]).all()
    with pytest.raises(ValueError, match="speaker"):
        m.inference(tok, {"speaker_ids": None})


def test_synthesizer_forward_tts_hifigan(cuda_device, models):
    """Synthesizer(ForwardTTS, HifiganGenerator).tts_batch with a reduced-width HiFiGAN: the waveform has
    the right length and matches oracle mel -> HiFiGAN oracle."""
    from oracle import hifigan_ref
    from tts_amd import synthetic
    from tts_amd.config import HIFIGAN_V1
    from tts_amd.synthesizer import Synthesizer
    from tts_amd.vocoder import HifiganGenerator

    cfg = dict(in_channels=80, out_channels=1, **dict(HIFIGAN_V1, upsample_initial_channel=128))
    sd = synthetic.hifigan_state_dict(**cfg, seed=7, weight_norm=True)
    g = HifiganGenerator(**cfg)
    g.load_state_dict(sd)
    g.eval()
    g.remove_weight_norm()
    g = g.to(cuda_device)
    m = models("fastpitch")
    tok = C.tokens("fastpitch").to(cuda_device)
    lens = torch.full((tok.shape[0],), tok.shape[1])
    wav, voc_in = Synthesizer(m, g).tts_batch(tok, lens)
    ref = C.reference("fastpitch")
    mel = ref["model_outputs"].transpose(1, 2)
    assert voc_in.shape == mel.shape
    assert wav.shape == (mel.shape[0], 1, 256 * (mel.shape[2] + 10))
    with torch.no_grad():
        wref = hifigan_ref.hifigan_forward(sd, mel, pad=5, dtype=torch.float64, **cfg)
    assert_close_fp32(wav.cpu(), wref, "Synthesizer(ForwardTTS fastpitch, HiFiGAN 128)", **tol("fp32"))
