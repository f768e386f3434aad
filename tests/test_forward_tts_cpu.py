"""ForwardTTS (FastPitch) without a GPU: the C-ABI's argument checks (every rejection comes before a
launch, so it needs no device), the module's parameter tree against the reference's state-dict
inventory and the library's weight list, the rejected configurations, and the properties of the
oracle and of the synthetic inputs that the GPU tests lean on (so they cannot pass vacuously or flake)."""
import ctypes

import pytest
import torch

import _forward_tts_cases as C
import _forward_tts_ref as R
from _util import FP32_MAX_ABS, FP32_REL_RMS, WAV_MAX_ABS, max_abs, rel_rms
from tts_amd import _native as N
from tts_amd import synthetic
from tts_amd.tts import ForwardTTS, ForwardTTSArgs, multi_head_attention

X6 = N.MATH_MODES["fp32x6"]


# ------------------------------------------------------------------ tts_op_mha
def call(E, heads, T, B=1, mode=X6, qkv=True, out=True):
    buf = ctypes.create_string_buffer(64)
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    return N.lib().tts_op_mha(a if qkv else None, None, B, E, heads, T, mode, b if out else None, None)


def test_tile_and_null_arguments():
    lib = N.lib()
    assert lib.tts_op_mha_tile() == 64
    assert call(64, 2, 8, qkv=False) == N.TTS_ERR_INVALID
    assert b"NULL" in lib.tts_last_error()
    assert call(64, 2, 8, out=False) == N.TTS_ERR_INVALID
    assert lib.tts_forward_tts_create(None, None, 0, None) == N.TTS_ERR_INVALID
    assert lib.tts_forward_tts_encode(None, None, None, None, None, 1, 1, 1.0, None, None, None, None, None, None,
                                      None) == N.TTS_ERR_INVALID
    assert lib.tts_forward_tts_decode(None, None, None, None, None, 1, 1, 1, 0, None, None, None, None) == N.TTS_ERR_INVALID
    assert lib.tts_forward_tts_block(None, 0, None, None, 1, 1, None, None) == N.TTS_ERR_INVALID
    assert lib.tts_forward_tts_destroy(None) == N.TTS_OK


@pytest.mark.parametrize("E,heads,T,B,mode,code", [
    (96, 2, 8, 1, X6, N.TTS_ERR_UNSUPPORTED),     # head size 48
    (16, 1, 8, 1, X6, N.TTS_ERR_UNSUPPORTED),     # head size 16
    (768, 2, 8, 1, X6, N.TTS_ERR_UNSUPPORTED),    # an accepted head size, more than 512 channels
    (512, 1, 8, 1, X6, N.TTS_ERR_UNSUPPORTED),    # head size 512
    (384, 1, 1 << 19, 1, X6, N.TTS_ERR_UNSUPPORTED),  # a qkv plane of 2.25 GiB
    (64, 3, 8, 1, X6, N.TTS_ERR_INVALID),         # channels do not divide into the heads
    (64, 2, 0, 1, X6, N.TTS_ERR_INVALID),
    (64, 2, 8, 0, X6, N.TTS_ERR_INVALID),
    (64, 2, 8, 1, 7, N.TTS_ERR_INVALID),          # unknown math mode
])
def test_rejected_before_any_launch(E, heads, T, B, mode, code):
    assert call(E, heads, T, B, mode) == code
    assert N.lib().tts_last_error() != b""


def test_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        multi_head_attention(torch.zeros(1, 192, 8), 2)


def test_oracle_is_the_plain_formula():
    """torch's multi_head_attention_forward with identity projections = softmax((q dk^-0.5)^T k) v with
    exact zeros under the key padding mask."""
    E, heads, T = 64, 2, 19
    qkv = torch.randn(2, 3 * E, T, generator=torch.Generator().manual_seed(0))
    kl = torch.tensor([T, 5])
    out, w = R.mha_from_qkv(qkv, heads, kl)
    s = R.scores(qkv, heads).masked_fill(R.key_padding_mask(kl, T)[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    assert max_abs(w, p) < 1e-14
    assert (w[1, :, :, 5:] == 0).all()
    v = qkv[:, 2 * E:].double().reshape(2, heads, E // heads, T)
    assert max_abs(out, torch.einsum("bhij,bhdj->bhdi", p, v).reshape(2, E, T)) < 1e-13
    assert R.mha_macs(2, E, T) == 2 * 2 * E * T * T


@pytest.mark.parametrize("qscale", [1.0, 11.0])
def test_oracle_fp32_within_half_the_fp32_gates(qscale):
    """The oracle's own fp32 evaluation stays inside half of each fp32 gate of its fp64 one at the
    widest shape the GPU tests run, plain and with the scaled queries: the gates are reachable."""
    E, heads, T = 384, 1, 133
    qkv = torch.randn(2, 3 * E, T, generator=torch.Generator().manual_seed(3))
    qkv[:, :E] *= qscale
    ref, _ = R.mha_from_qkv(qkv, heads)
    f32, _ = R.mha_from_qkv(qkv, heads, dtype=torch.float32)
    ma, rr = max_abs(f32, ref), rel_rms(f32, ref)
    print(f"oracle fp32 vs fp64 (qscale {qscale}): max|d|={ma:.3e} rel-RMS={rr:.3e}")
    assert ma <= FP32_MAX_ABS / 2 and rr <= FP32_REL_RMS / 2


# ------------------------------------------------------------------ the module and the library's inventory
def inventory(args):
    """The reference's state-dict keys (module tree of TTS/tts/models/forward_tts.py) with shapes."""
    H, out = args["hidden_channels"], args["out_channels"]
    inv = {"emb.weight": (args["num_chars"], H), "pos_encoder.pe": (1, H, 5000)}

    def block(pre, p):
        F = p["hidden_channels_ffn"]
        for i in range(p["num_layers"]):
            q = f"{pre}fft_layers.{i}."
            inv.update({q + "self_attn.in_proj_weight": (3 * H, H), q + "self_attn.in_proj_bias": (3 * H,),
                        q + "self_attn.out_proj.weight": (H, H), q + "self_attn.out_proj.bias": (H,),
                        q + "conv1.weight": (F, H, 3), q + "conv1.bias": (F,), q + "conv2.weight": (H, F, 3),
                        q + "conv2.bias": (H,), q + "norm1.weight": (H,), q + "norm1.bias": (H,),
                        q + "norm2.weight": (H,), q + "norm2.bias": (H,)})

    def predictor(pre, hidden, k):
        inv.update({pre + "conv_1.weight": (hidden, H, k), pre + "conv_1.bias": (hidden,),
                    pre + "norm_1.gamma": (1, hidden, 1), pre + "norm_1.beta": (1, hidden, 1),
                    pre + "conv_2.weight": (hidden, hidden, k), pre + "conv_2.bias": (hidden,),
                    pre + "norm_2.gamma": (1, hidden, 1), pre + "norm_2.beta": (1, hidden, 1),
                    pre + "proj.weight": (1, hidden, 1), pre + "proj.bias": (1,)})

    block("encoder.encoder.", args["encoder_params"])
    block("decoder.decoder.transformer_block.", args["decoder_params"])
    inv.update({"decoder.decoder.postnet.weight": (out, H, 1), "decoder.decoder.postnet.bias": (out,)})
    predictor("duration_predictor.", args["duration_predictor_hidden_channels"], args["duration_predictor_kernel_size"])
    predictor("pitch_predictor.", args["pitch_predictor_hidden_channels"], args["pitch_predictor_kernel_size"])
    k = args["pitch_embedding_kernel_size"]
    inv.update({"pitch_emb.weight": (H, 1, k), "pitch_emb.bias": (H,)})
    if args["use_speaker_embedding"]:
        inv["emb_g.weight"] = (args["num_speakers"], H)
    return inv


@pytest.mark.parametrize("name", ["small", "fastpitch"])
def test_state_dict_keys_and_weight_inventory(name, tmp_path):
    args = C.ARGS[name]
    m = ForwardTTS(args)
    inv = inventory(args)
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == inv
    syn = C.state_dict(name)
    assert {k: tuple(v.shape) for k, v in syn.items()} == inv
    # the library's weight list: count and sizes
    ws = m._weight_list()
    assert N.lib().tts_forward_tts_num_weights(ctypes.byref(m._cfg)) == len(ws)
    assert sum(w.size for w in ws) == sum(v.numel() for v in sd.values())
    for i, w in enumerate(ws):
        assert N.lib().tts_forward_tts_weight_numel(ctypes.byref(m._cfg), i) == w.size, i
    assert N.lib().tts_forward_tts_weight_numel(ctypes.byref(m._cfg), len(ws)) == -1
    # a reference checkpoint (with the training-only aligner) loads unchanged
    ck = dict(syn)
    ck["aligner.key_proj.0.conv.weight"] = torch.zeros(3)
    torch.save({"model": ck}, tmp_path / "ck.pth")
    m.load_checkpoint(None, str(tmp_path / "ck.pth"), eval=True)
    assert not m.training and torch.equal(m.state_dict()["emb.weight"], syn["emb.weight"])
    assert m.length_scale == 1.0


def test_pe_buffer_is_the_formula_bit_for_bit():
    for name in ("small", "fastpitch"):
        H = C.ARGS[name]["hidden_channels"]
        pe = R.make_pe(H)
        assert torch.equal(ForwardTTS(C.ARGS[name]).pos_encoder.pe, pe)
        assert torch.equal(C.state_dict(name)["pos_encoder.pe"], pe)
    # pe[0, 2i, t] = sin(t / 10000^(2i/C)), pe[0, 2i+1, t] = cos(...)
    t, i, Cc = 37, 5, 64
    pe = R.make_pe(Cc)
    assert abs(pe[0, 2 * i, t].item() - torch.sin(torch.tensor(t / 10000 ** (2 * i / Cc))).item()) < 1e-6
    assert abs(pe[0, 2 * i + 1, t].item() - torch.cos(torch.tensor(t / 10000 ** (2 * i / Cc))).item()) < 1e-6


def test_rejected_configurations():
    base = C.ARGS["small"]
    for over in (dict(use_energy=True), dict(use_d_vector_file=True), dict(encoder_type="relative_position_transformer"),
                 dict(decoder_type="residual_conv_bn"), dict(encoder_type="fftransformer", decoder_type="wavenet")):
        with pytest.raises(NotImplementedError):
            ForwardTTS(dict(base, **over))
    with pytest.raises(ValueError):
        ForwardTTS(dict(base, num_chars=None))
    # head size 48: refused by the library with its status code, before anything is built
    bad = dict(base, hidden_channels=96)
    with pytest.raises(N.NativeError) as e:
        ForwardTTS(bad)
    assert e.value.code == N.TTS_ERR_UNSUPPORTED
    with pytest.raises(N.NativeError) as e:
        ForwardTTS(dict(base, duration_predictor_kernel_size=4))
    assert e.value.code == N.TTS_ERR_UNSUPPORTED
    m = ForwardTTS(ForwardTTSArgs(num_chars=10))
    assert m.args.hidden_channels == 384 and m._cfg.encoder_num_layers == 6 and m._cfg.decoder_num_heads == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(torch.zeros(1, 4, dtype=torch.int64))


def test_duration_rule_on_hand_values():
    """round(max((exp(o) - 1) * mask * length_scale, 1)), torch.round = half to even."""
    want = {0.0: 1, 0.3: 1, 0.5: 1, 0.999: 1, 1.0: 1, 1.5: 2, 2.5: 2, 3.5: 4, 4.5: 4, 2.49: 2, 2.51: 3, 7.0: 7}
    for dtype in (torch.float32, torch.float64):
        raw = torch.tensor(list(want), dtype=dtype)
        assert R.round_durations(raw).tolist() == [float(v) for v in want.values()]
    # through the exponential, away from the edges, with a mask and a length scale
    raw = torch.tensor([0.2, 1.3, 2.7, 6.1], dtype=torch.float64)
    o = torch.log(raw + 1).reshape(1, 1, -1)
    m = torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=torch.float64).reshape(1, 1, -1)
    dur, back = R.format_durations(o, m)
    assert max_abs(back[0], raw * m[0, 0]) < 1e-12
    assert dur[0].tolist() == [1.0, 1.0, 3.0, 1.0]  # the reference clamps a masked token to 1 as well
    assert R.format_durations(o, m, length_scale=2.0)[0][0].tolist() == [1.0, 3.0, 5.0, 1.0]


def test_mac_count_per_decoder_frame():
    """The oracle's MAC counter at the benchmark's shape (896 frames): per frame and decoder layer
    in_proj + out_proj 4 H^2, scores + PV 2 H T, the two k3 FFN convs 6 H F (DESIGN.md quotes these)."""
    args = C.ARGS["fastpitch"]
    H, F, T = 384, 1024, 896
    counter = {}
    x = torch.zeros(1, H, 8)
    with torch.no_grad():
        R.fft_block(C.state_dict("fastpitch"), "decoder.decoder.transformer_block.", x, 1, 6, None, torch.float32,
                    counter=counter, tag="decoder")
    per_col = {k: v / 8 for k, v in counter.items()}
    assert per_col["decoder.in_proj"] == 6 * 3 * H * H and per_col["decoder.out_proj"] == 6 * H * H
    assert per_col["decoder.ffn"] == 6 * 6 * H * F
    assert per_col["decoder.attn"] == 6 * 2 * H * 8
    layer = 4 * H * H + 2 * H * T + 6 * H * F
    assert layer == 3637248  # 3.6 MMAC per frame and layer: 0.59 + 0.69 + 2.36
    assert args["decoder_params"]["num_layers"] * layer + 80 * H == 21854208  # 21.9 MMAC per decoder frame


# ------------------------------------------------------------------ conditions on the GPU tests' inputs
@pytest.mark.parametrize("name", ["small", "fastpitch"])
def test_condition_a_attention_is_peaked(name):
    """With the synthetic weights the mean over query rows of the largest attention probability is at
    least 10 / T in every layer (64 tokens, 192 frames): the softmax is far from uniform, so an error in
    the scores or in the running maximum shows in the output."""
    args = C.ARGS[name]
    x = synthetic.tokens(1, 64, args["num_chars"], seed=1)
    probs = []
    kw = dict(speaker_ids=torch.tensor([1])) if args["use_speaker_embedding"] else {}
    with torch.no_grad():
        R.inference(C.state_dict(name), args, x, durations=torch.full((1, 64), 3), dtype=torch.float32, probs=probs, **kw)
    assert len(probs) == args["encoder_params"]["num_layers"] + args["decoder_params"]["num_layers"]
    for i, (tag, w) in enumerate(probs):
        T = w.shape[-1]
        peak = w.max(-1).values.mean().item()
        print(f"{name} {tag} layer {i}: T={T} mean max p={peak:.3f} (10/T={10 / T:.3f})")
        assert peak >= 10.0 / T, (tag, i)


def predicted_variants(name):
    return ["plain", "lengths"] if name == "small" else ["plain"]


@pytest.mark.parametrize("name", ["small", "fastpitch"])
def test_condition_b_durations_are_away_from_the_rounding_edges(name):
    """On every end-to-end case the oracle's durations before rounding are at least 1e-3 from any
    half-integer and from the clamp at 1, and its fp32 and fp64 durations are equal."""
    for variant in predicted_variants(name):
        ref, f32 = C.reference(name, variant), C.reference(name, variant, fp32=True)
        raw = ref["durations_raw"]
        valid = raw != 0  # padded tokens: (exp(0) - 1) * 0
        above = raw[valid & (raw > 1)]  # below the clamp every value becomes 1: 0.5 is no edge there
        assert (((above - torch.floor(above)) - 0.5).abs() >= 1e-3).all(), (variant, raw)
        assert ((raw[valid] - 1.0).abs() >= 1e-3).all(), (variant, raw)
        assert torch.equal(ref["durations"], f32["durations"].double())
        print(f"{name} {variant}: durations {ref['durations'].tolist()}")
        assert ref["durations"].max() >= 4 and ref["durations"][ref["durations"] > 0].min() <= 2  # spread out


def bf16_analogue(name):
    """torch's bf16 CPU forward of the decoder (the part ``math_mode="bf16"`` runs in bf16) on the
    oracle's fp64 decoder input, against fp64: (max|d|, rel-RMS)."""
    ref = C.reference(name)
    with torch.no_grad():
        out = R.decoder(C.state_dict(name), C.ARGS[name], ref["decoder_input"], ref["y_mask"], dtype=torch.bfloat16)
    return max_abs(out.double(), ref["model_outputs"]), rel_rms(out.double(), ref["model_outputs"])


def test_bf16_analogue_decides_the_bf16_gates():
    """Condition (c) for bf16.  The small case is always held to the bf16 gates; the fastpitch case is
    gated where torch's own bf16 forward stays inside half of them at that depth, and only logged where
    it does not.  (torch rounds every activation to bf16; the device path keeps fp32 activations and
    rounds the MFMA operands only, so its error is expected below this analogue's.)"""
    from _util import BF16_MAX_ABS, BF16_REL_RMS

    assert C.BF16_GATED["small"]
    for name in ("small", "fastpitch"):
        ma, rr = bf16_analogue(name)
        inside = ma <= BF16_MAX_ABS / 2 and rr <= BF16_REL_RMS / 2
        print(f"{name}: torch bf16 decoder vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e} inside half the gate: {inside}")
    assert inside == C.BF16_GATED["fastpitch"]


@pytest.mark.parametrize("name", ["small", "wide"])
def test_condition_c_block_inputs(name):
    """The same for the block tests' inputs (T = 65: the widest)."""
    for decoder in (False, True):
        pre, p, x, _, mask = C.block_case(name, decoder, 65)
        with torch.no_grad():
            ref = R.fft_block(C.state_dict(name), pre, x, p["num_heads"], p["num_layers"], mask)
            f32 = R.fft_block(C.state_dict(name), pre, x, p["num_heads"], p["num_layers"], mask.float(), torch.float32)
        ma, rr = max_abs(f32, ref), rel_rms(f32, ref)
        print(f"{name} {'decoder' if decoder else 'encoder'} block: oracle fp32 vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e}")
        assert ma <= WAV_MAX_ABS / 2 and rr <= FP32_REL_RMS / 2


@pytest.mark.parametrize("name", ["small", "fastpitch"])
def test_condition_c_oracle_fp32_within_half_the_gates(name):
    """The oracle's own fp32 forward is within half of each fp32 gate of its fp64 forward."""
    variants = ["plain", "lengths", "durations", "plain+keys", "lengths+keys", "durations+keys"] if name == "small" else ["plain"]
    for variant in variants:
        ref, f32 = C.reference(name, variant), C.reference(name, variant, fp32=True)
        for key in ("model_outputs", "pitch", "durations_log"):
            ma, rr = max_abs(f32[key], ref[key]), rel_rms(f32[key], ref[key])
            print(f"{name} {variant} {key}: oracle fp32 vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e}")
            assert ma <= WAV_MAX_ABS / 2 and rr <= FP32_REL_RMS / 2, (variant, key)
        assert torch.equal(f32["alignments"].double(), ref["alignments"])


# ------------------------------------------------------------------ conditions on the long GPU tests' inputs
def long_predicted_variants(name):
    """The variants whose durations differ (the decoder's key mask does not reach the durations)."""
    return [v for v in C.LONG_VARIANTS[name] if "+" not in v]


@pytest.mark.parametrize("name", ["small_long", "wide_long"])
def test_condition_b_long_durations_are_away_from_the_rounding_edges(name):
    """Condition (b) for the long cases (test_forward_tts_long_gpu.py), without and - small_long - with
    every token valid: before rounding the oracle's durations are at least 1e-3 from any half-integer and
    from the clamp at 1, its fp32 and fp64 durations are equal, and the frame counts are the documented
    ones (several 256-frame workgroups, more than one conv tile)."""
    for variant in long_predicted_variants(name):
        ref, f32 = C.long_reference(name, variant), C.long_reference(name, variant, fp32=True)
        raw = ref["durations_raw"]
        valid = raw != 0
        above = raw[valid & (raw > 1)]
        half = ((above - torch.floor(above)) - 0.5).abs().min().item()
        clamp = (raw[valid] - 1.0).abs().min().item()
        frames = tuple(int(v) for v in ref["durations"].sum(1))
        print(f"{name} {variant}: frames {frames}, distance from a half-integer {half:.2e}, from the clamp {clamp:.2e}")
        assert half >= 1e-3 and clamp >= 1e-3, variant
        assert torch.equal(ref["durations"], f32["durations"].double())
        assert frames == C.LONG_FRAMES[name, variant]
        assert ref["durations"].max() >= 4 and ref["durations"][ref["durations"] > 0].min() <= 2
        if variant == "lengths":  # padded tokens get no frames
            pad = torch.arange(raw.shape[1])[None, :] >= torch.tensor(C.LONG[name]["lengths"])[:, None]
            assert pad.any() and (ref["durations"][pad] == 0).all()


@pytest.mark.parametrize("name", ["small_long", "wide_long"])
def test_condition_c_long_oracle_fp32_within_half_the_gates(name):
    """Condition (c) for the long cases: the oracle's own fp32 forward is within half of each fp32 gate."""
    for variant in C.LONG_VARIANTS[name]:
        ref, f32 = C.long_reference(name, variant), C.long_reference(name, variant, fp32=True)
        for key in ("model_outputs", "pitch", "durations_log"):
            ma, rr = max_abs(f32[key], ref[key]), rel_rms(f32[key], ref[key])
            print(f"{name} {variant} {key}: oracle fp32 vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e}")
            assert ma <= WAV_MAX_ABS / 2 and rr <= FP32_REL_RMS / 2, (variant, key)
        assert torch.equal(f32["alignments"].double(), ref["alignments"])


@pytest.mark.parametrize("name", ["small", "wide"])
def test_condition_c_long_block_inputs(name):
    """The same for the block tests' inputs at T = 259, ragged ([259, 129] keys) and unmasked."""
    for decoder in (False, True):
        for ragged in (True, False):
            ref = C.long_block_reference(name, decoder, ragged)
            f32 = C.long_block_reference(name, decoder, ragged, fp32=True)
            assert ref.shape == (2, C.ARGS[name]["hidden_channels"], C.LONG_BLOCK_T)
            ma, rr = max_abs(f32, ref), rel_rms(f32, ref)
            print(f"{name} {'decoder' if decoder else 'encoder'} block T={C.LONG_BLOCK_T} "
                  f"{'ragged' if ragged else 'no mask'}: oracle fp32 vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e}")
            assert ma <= WAV_MAX_ABS / 2 and rr <= FP32_REL_RMS / 2
    assert C.block_case(name, True, C.LONG_BLOCK_T)[3].tolist() == [259, 129]


@pytest.mark.parametrize("keys", [False, True])
def test_condition_c_frame_limit_case(keys):
    """The 5000-frame case: the durations sum to the positional encoding's length exactly, and the
    oracle's fp32 forward is within half of the fp32 gates there too."""
    assert sum(C.LIMIT_DURATIONS) == R.MAX_FRAMES and len(C.LIMIT_DURATIONS) == 13
    ref, f32 = C.limit_reference(keys), C.limit_reference(keys, fp32=True)
    assert ref["model_outputs"].shape == (1, R.MAX_FRAMES, 80)
    ma, rr = max_abs(f32["model_outputs"], ref["model_outputs"]), rel_rms(f32["model_outputs"], ref["model_outputs"])
    print(f"frame limit, keys masked {keys}: oracle fp32 vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e}")
    assert ma <= WAV_MAX_ABS / 2 and rr <= FP32_REL_RMS / 2
    assert torch.equal(f32["alignments"].double(), ref["alignments"])


def test_bf16_analogue_decides_the_long_bf16_gate():
    """Condition (c) for bf16 on small_long lengths+keys, by the rule of
    test_bf16_analogue_decides_the_bf16_gates: gated where torch's own bf16 CPU forward of the decoder
    (keys masked, as the case runs) stays inside half of the bf16 gates, logged only where it does not."""
    from _util import BF16_MAX_ABS, BF16_REL_RMS

    ref = C.long_reference("small_long", "lengths+keys")
    with torch.no_grad():
        out = R.decoder(C.state_dict("small"), C.ARGS["small"], ref["decoder_input"], ref["y_mask"],
                        mask_decoder_keys=True, dtype=torch.bfloat16)
    ma, rr = max_abs(out.double(), ref["model_outputs"]), rel_rms(out.double(), ref["model_outputs"])
    inside = ma <= BF16_MAX_ABS / 2 and rr <= BF16_REL_RMS / 2
    print(f"small_long lengths+keys: torch bf16 decoder vs fp64 max|d|={ma:.3e} rel-RMS={rr:.3e} inside half the gate: {inside}")
    assert inside == C.LONG_BF16_GATED["small_long"]


def test_long_mha_shapes_rejected_before_any_launch():
    """Valid head sizes (192, 384) with more than 512 channels; 512 channels are accepted shapes."""
    assert call(576, 3, 8) == N.TTS_ERR_UNSUPPORTED
    assert call(768, 2, 8) == N.TTS_ERR_UNSUPPORTED
    assert b"512" in N.lib().tts_last_error()
