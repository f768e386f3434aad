"""ForwardTTS (FastPitch) and its attention op past one tile and at their limits, on MI355X, against the
fp64 oracle (tests/_forward_tts_ref.py).  test_forward_tts_gpu.py stops at 13 tokens, a few dozen frames
and 65 block columns; here:

* ``tts_op_mha`` at E = 512 (its channel limit) with 2 and 8 heads: the head sizes 256 (the last on the
  K-prefetch path in fp32x6) and 64, and ``blockIdx.y`` up to 7; key lengths outside [1, T] (clamped; a
  length of 0 gives zeros, for the op and for a whole empty utterance);
* one FFTransformerBlock at T = 259 = 256 + 3 = 2*128 + 3 = 4*64 + 3 = 16*16 + 3 columns, key lengths
  [259, 129]: three columns past every conv, attention and LayerNorm tile edge;
* the whole model with predicted durations at 259 tokens / 800 frames (``small_long``) and at the
  fastpitch widths with 131 tokens / 433 frames (``wide_long``): a second, third and fourth workgroup
  column of every glue kernel, a second trip of the duration kernel's loop, positional-encoding rows up
  to 803, the pitch-embedding halo across a workgroup edge;
* 5000 frames (the positional encoding's length) compared with the oracle, not only "finite";
* ``ForwardTTS.profile`` and the clamps on out-of-range token and speaker ids.

The inputs are in tests/_forward_tts_cases.py; the conditions they meet (durations away from every
rounding edge, the oracle's own fp32 evaluation inside half of each gate) are the "long" tests of
test_forward_tts_cpu.py, so no comparison here depends on a rounding tie and no token is left out.
Gates: tests/_util.py tol(); every measured error is logged with log_error (TTS_ERRLOG;
profiles/parity_errors_forward_tts_long.jsonl is one such run).  bf16 on small_long is logged, not gated:
torch's own bf16 forward of that decoder is outside half the bf16 gate (C.LONG_BF16_GATED).

Measured on MI355X (max|d| / rel-RMS, the worst of each group).  fp32x6: the op 7.3e-7 / 3.1e-7; the
blocks at T = 259 9.4e-6 / 9.6e-7 (wide decoder, ragged: the max is close to its gate of 1e-5, as the
fastpitch model's is in test_forward_tts_gpu.py; the oracle's own fp32 evaluation is 2.1e-6 there); the
mel 7.1e-6 / 1.5e-6 (wide_long), small_long 4.4e-6 / 5.6e-7, 5000 frames 3.0e-6 / 5.5e-7; pitch and
durations_log 5.5e-6 / 1.7e-6.  bf16: the op 8.1e-3 / 3.2e-3, the small decoder block 1.7e-2 / 3.2e-3,
the small_long mel 1.8e-2 / 3.6e-3 (logged; it would pass the bf16 gates of 5e-2 / 3e-2)."""
import math

import pytest
import torch

import _forward_tts_cases as C
import test_forward_tts_gpu as G
from _util import assert_close_fp32, tol
from tts_amd import _native as N
from tts_amd.tts import multi_head_attention
from tts_amd.tts.forward_tts import mha_tile

pytestmark = pytest.mark.gpu
models = G.models  # the module-scoped model cache of test_forward_tts_gpu.py (one per module)
LIMIT_SHAPES = [(512, 2), (512, 8)]  # (E, heads) at kMhaMaxE: head sizes 256 and 64
OUTPUTS = ("model_outputs", "pitch", "durations_log", "alignments")


# ------------------------------------------------------------------ tts_op_mha
@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
@pytest.mark.parametrize("E,heads", LIMIT_SHAPES)
def test_mha_op_at_the_channel_limit(cuda_device, E, heads, mode):
    """The sweep of test_mha_op (tile-edge lengths x key-length cases) on the two instantiations it
    never launches."""
    for T in G.lengths():
        for kl in G.key_length_cases(T):
            qkv, ref = G.case(E, heads, T, kl)
            out = G.run(cuda_device, qkv, heads, kl, mode)
            assert_close_fp32(out, ref, f"mha {mode} E={E} heads={heads} T={T} key_lengths={kl}", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_mha_running_max_rescale_head_256(cuda_device, mode):
    G.test_mha_running_max_rescale(cuda_device, 512, 2, mode)


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_mha_batch_invariance_eight_heads(cuda_device, mode):
    """Item b of a B = 3 call is bitwise the B = 1 call at E = 512 with eight heads."""
    E, heads, T = 512, 8, mha_tile() + 3
    qkv = torch.randn(3, 3 * E, T, generator=torch.Generator().manual_seed(5))
    kl = (T, 40, 7)
    full = G.run(cuda_device, qkv, heads, kl, mode)
    for b in range(3):
        one = G.run(cuda_device, qkv[b : b + 1], heads, kl[b : b + 1], mode)
        assert torch.equal(one[0], full[b]), f"item {b}"


@pytest.mark.parametrize("E,heads", [(576, 3), (768, 2)])
def test_mha_more_than_512_channels_rejected_before_launch(cuda_device, E, heads):
    """Accepted head sizes (192, 384) with E > 512."""
    with pytest.raises(N.NativeError) as e:
        multi_head_attention(torch.zeros(1, 3 * E, 8, device=cuda_device), heads)
    assert e.value.code == N.TTS_ERR_UNSUPPORTED


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
@pytest.mark.parametrize("E,heads", [(64, 2), (512, 8)])
def test_mha_key_lengths_outside_the_range(cuda_device, E, heads, mode):
    """Lengths past T count as T; a length of 0 (or below) leaves no key: that item comes out all
    zeros - an invalid item gives zeros - and its neighbour is bitwise its own B = 1 call."""
    T = mha_tile() + 5
    qkv, _ = G.case(E, heads, T, None)
    plain = G.run(cuda_device, qkv, heads, None, mode)
    assert torch.equal(G.run(cuda_device, qkv, heads, (T + 5, T + 5), mode), plain)
    one = G.run(cuda_device, qkv[:1], heads, (T - 7,), mode)
    for empty in (0, -3):
        out = G.run(cuda_device, qkv, heads, (T - 7, empty), mode)
        assert torch.equal(out[0], one[0]), empty
        assert torch.count_nonzero(out[1]) == 0 and torch.isfinite(out).all(), empty


def test_model_with_an_empty_utterance(cuda_device, models):
    """x_lengths = (13, 0, 5), decoder keys masked, predicted durations: the empty item gets no frames
    and an all-zero mel, nothing is NaN, and its neighbours are bitwise the call without it."""
    m = models("small", None, True)
    tok = C.tokens("small").to(cuda_device)
    spk, lens = torch.tensor(C.SMALL_SPEAKERS), torch.tensor((13, 0, 5))
    out = m.inference(tok, {"speaker_ids": spk, "x_lengths": lens})
    for k in OUTPUTS:
        assert torch.isfinite(out[k]).all(), k
    assert out["alignments"][1].sum().item() == 0  # y_length 0
    assert out["alignments"][0].sum().item() >= 13 and out["alignments"][2].sum().item() >= 5
    assert torch.count_nonzero(out["model_outputs"][1]) == 0
    keep = torch.tensor([0, 2])
    two = m.inference(tok[keep.to(cuda_device)], {"speaker_ids": spk[keep], "x_lengths": lens[keep]})
    for k in OUTPUTS:
        assert torch.equal(out[k][keep.to(cuda_device)], two[k]), k


# ------------------------------------------------------------------ one block at T = 259
@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("decoder", [False, True])
def test_fft_block_past_the_tiles(cuda_device, models, name, decoder):
    """test_fft_block at 259 columns, keys [259, 129]: the text tile (16 columns) and the frames tile
    conv_tile_for picks, each with the doubled out_proj, the ReLU epilogue and the residual, across
    their edges; 5 query tiles and 9 key tiles of the attention."""
    m = models(name, "fp32x6")
    T = C.LONG_BLOCK_T
    _, _, x, kl, _ = C.block_case(name, decoder, T)
    what = f"fft_block {name} {'decoder' if decoder else 'encoder'} T={T}"
    assert_close_fp32(m.fft_block(x, kl, decoder=decoder).cpu(), C.long_block_reference(name, decoder, True),
                      what + " ragged", **tol("fp32"))
    assert_close_fp32(m.fft_block(x, None, decoder=decoder).cpu(), C.long_block_reference(name, decoder, False),
                      what + " no mask", **tol("fp32"))


def test_fft_block_past_the_tiles_bf16(cuda_device, models):
    m = models("small", "bf16")
    T = C.LONG_BLOCK_T
    _, _, x, kl, _ = C.block_case("small", True, T)
    assert_close_fp32(m.fft_block(x, kl, decoder=True).cpu(), C.long_block_reference("small", True, True),
                      f"fft_block small decoder bf16 T={T}", **tol("bf16"))


# ------------------------------------------------------------------ the whole model, hundreds of tokens and frames
def run_long(m, name, variant, dev):
    kw = C.long_kwargs(name, variant)
    aux = {"d_vectors": None, "speaker_ids": kw.get("speaker_ids")}
    if "x_lengths" in kw:
        aux["x_lengths"] = kw["x_lengths"]
    return m.inference(C.long_tokens(name).to(dev), aux)


def assert_padding_is_zero(out, ref, x_lengths, what):
    """mel columns past y_lengths and alignment rows of padded tokens: exactly 0."""
    mel, attn = out["model_outputs"].cpu(), out["alignments"].cpu()  # [B, T_de, C], [B, T_de, T_en]
    y_len = ref["durations"].sum(1).long().tolist()
    assert min(y_len) < mel.shape[1] == max(y_len), what
    for b, n in enumerate(y_len):
        assert torch.count_nonzero(mel[b, n:]) == 0, f"{what}: mel of item {b} past frame {n}"
        assert torch.count_nonzero(attn[b, n:]) == 0, f"{what}: alignment of item {b} past frame {n}"
        if x_lengths is not None:
            assert torch.count_nonzero(attn[b, :, x_lengths[b]:]) == 0, f"{what}: padded tokens of item {b}"


@pytest.mark.parametrize("name,variant,mode", [
    ("small_long", "lengths", None), ("small_long", "lengths+keys", None), ("small_long", "plain", None),
    ("wide_long", "lengths", None), ("wide_long", "lengths+keys", None), ("small_long", "lengths+keys", "bf16")])
def test_long_model(cuda_device, models, name, variant, mode):
    """small_long: B = 4, T_en = 259, x_lengths (259, 256, 65, 1), 557 / 800 / 157 / 5 frames (plain:
    557 / 804 / 613 / 580); wide_long: the fastpitch widths at two layers, B = 2, T_en = 131, x_lengths
    (131, 64), 433 / 244 frames.  Predicted durations; alignments and durations exact, pitch and
    durations_log at the fp32 gates, the mel at the mode's gates (bf16: C.LONG_BF16_GATED)."""
    case = C.LONG[name]
    m = models(case["model"], mode, variant.endswith("+keys"))
    out = run_long(m, name, variant, cuda_device)
    ref = C.long_reference(name, variant)
    what = f"forward_tts {name} {variant} {mode}"
    gated = mode != "bf16" or C.LONG_BF16_GATED[name]
    G.check_outputs(out, ref, what, mode or "fp32", gated)
    assert_padding_is_zero(out, ref, case["lengths"] if variant.startswith("lengths") else None, what)


def test_long_model_batch_invariance(cuda_device, models):
    """small_long with given durations of 1036 frames per item (equal frame counts: the k3 convs read
    the columns past an utterance's end): item b of the B = 4 call is bitwise the B = 1 call.  The
    duration kernel sums 259 given values per item: a second trip of its 256-token loop."""
    case = C.LONG["small_long"]
    m = models("small", None, True)
    tok = C.long_tokens("small_long").to(cuda_device)
    B, T = tok.shape
    lens, spk = torch.tensor(case["lengths"]), torch.tensor(case["speakers"])
    frames = 4 * T
    dur = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(case["lengths"]):
        dur[b, :n] = frames // n
        dur[b, n - 1] += frames - n * (frames // n)  # the remainder on the last valid token (258, 255, 64, 0)
    assert (dur.sum(1) == frames).all()
    full = m.inference(tok, {"speaker_ids": spk, "x_lengths": lens, "durations": dur})
    assert full["model_outputs"].shape == (B, frames, 80)
    assert torch.equal(full["alignments"].sum(1).cpu(), dur.float())
    for b in range(B):
        one = m.inference(tok[b : b + 1], {"speaker_ids": spk[b : b + 1], "x_lengths": lens[b : b + 1],
                                           "durations": dur[b : b + 1]})
        for k in OUTPUTS:
            assert torch.equal(one[k][0], full[k][b]), (k, b)


# ------------------------------------------------------------------ the frame limit
@pytest.mark.parametrize("keys", [False, True])
def test_frame_limit_against_the_oracle(cuda_device, models, keys):
    """13 tokens, given durations of 12 x 384 + 392 = 5000 frames: positional-encoding rows up to 4999,
    79 query tiles and 157 key tiles, compared with the oracle."""
    m = models("small", "fp32x6", keys)
    tok, kw = C.limit_inputs()
    out = m.inference(tok.to(cuda_device), {"speaker_ids": kw["speaker_ids"], "durations": kw["durations"]})
    assert out["model_outputs"].shape == (1, 5000, 80)
    G.check_outputs(out, C.limit_reference(keys), f"forward_tts small 5000 frames keys masked {keys}", "fp32")


# ------------------------------------------------------------------ profile() and the id clamps
def expected_launches(enc_layers, dec_layers):
    """The executor's launch sequence (forward_tts.cpp encode, decode; vits_text.cpp VitsDp::forward)."""
    def block(tag, n):
        return [f"{tag}_{s}" for s in ("in_proj", "attention", "out_proj", "layernorm", "ffn1", "ffn2", "layernorm")] * n

    predictor = ["dp_input", "dp_conv", "dp_layernorm", "dp_conv", "dp_layernorm", "dp_proj"]
    return (["enc_embed"] + block("enc", enc_layers) + ["enc_mask_speaker"] + predictor + ["durations"] + predictor +
            ["pitch_emb", "expand", "pos_encoding"] + block("dec", dec_layers) + ["dec_postnet"])


def test_profile_is_inference_with_a_record_per_launch(cuda_device, models):
    m = models("small")
    tok = C.tokens("small").to(cuda_device)
    aux = {"speaker_ids": torch.tensor(C.SMALL_SPEAKERS), "x_lengths": torch.tensor(C.SMALL_LENGTHS)}
    ref = m.inference(tok, aux)
    out, rows = m.profile(tok, aux)
    assert set(out) == set(ref) and out["energy"] is None
    for k in OUTPUTS:
        assert torch.equal(out[k], ref[k]), k
    assert [r["name"] for r in rows] == expected_launches(2, 2)
    for r in rows:
        assert math.isfinite(r["ms"]) and r["ms"] >= 0, r
        assert r["flops"] >= 0 and r["bytes"] > 0, r
    assert sum(r["flops"] for r in rows if r["name"].endswith("_attention")) > 0


def test_out_of_range_ids_are_clamped(cuda_device, models):
    """Token ids -3 and num_chars + 7 give bitwise the result of ids 0 and num_chars - 1 (the reference
    raises IndexError; the kernels clamp instead of reading out of bounds); speaker ids likewise."""
    m = models("small")
    n_chars, n_spk = C.ARGS["small"]["num_chars"], C.ARGS["small"]["num_speakers"]
    tok = C.tokens("small")
    bad, good = tok.clone(), tok.clone()
    bad[0, 0], good[0, 0] = -3, 0
    bad[1, 2], good[1, 2] = n_chars + 7, n_chars - 1
    bad[2, 12], good[2, 12] = n_chars, n_chars - 1
    spk = torch.tensor(C.SMALL_SPEAKERS)
    ref = m.inference(good.to(cuda_device), {"speaker_ids": spk})
    out = m.inference(bad.to(cuda_device), {"speaker_ids": spk})
    for k in OUTPUTS:
        assert torch.equal(out[k], ref[k]), ("token ids", k)
    ref = m.inference(tok.to(cuda_device), {"speaker_ids": torch.tensor((0, n_spk - 1, 1))})
    out = m.inference(tok.to(cuda_device), {"speaker_ids": torch.tensor((-3, n_spk + 7, 1))})
    for k in OUTPUTS:
        assert torch.equal(out[k], ref[k]), ("speaker ids", k)
    assert C.SMALL_SPEAKERS != (0, n_spk - 1, 1)  # the clamped ids are not the case's own
