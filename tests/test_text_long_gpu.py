"""The text-side kernels past one workgroup tile and at their documented token limits, on MI355X,
against the fp64 oracles (oracle/vits_text_ref.py, oracle/glow_tts_ref.py, _vits_chain.oracle_chain)
with synthetic weights.

The standard shape is B = 4, T = 259, lengths [259, 256, 65, 1]: 259 = 4*64 + 3 = 256 + 3 = 2*128 + 3
= 16*16 + 3 = 32*8 + 3 ends three columns past every tile edge of the text side (64-column depthwise /
LayerNorm2 / embed workgroups, 256-position spline / affine workgroups, 128-column conv tiles,
16-column LayerNorm blocks, 8-query attention blocks, 64-key chunks); the rows end on a tile edge, one
past a tile edge and at a single token.  Further shapes: T_x = 700 (three tokens per thread of
expand_kernel's scan, several 256-frame workgroups), T = 901 and 3072 (attention rows past 64 KiB of
LDS, and the last token count launch_attention accepts), T_x = 16384 (the last token count
launch_expand accepts: 64 KiB of dynamic LDS beside 1 KiB of static).

Gates are the existing ones: ``_op_tol(mode)`` of test_vits_text_gpu.py, ``ENC_MAX_ABS`` /
``ENC_REL_RMS`` of test_glow_tts_gpu.py, the waveform / z gates of the Vits.inference tests; the
integer / selection outputs bit for bit.  Durations are ceil()-quantised, so a token whose fp64
duration lies within ``NEAR_INT`` of an integer may legitimately round either way in fp32: those
tokens (and only those) are left out of the duration comparison, and each test asserts they are at
most ``NEAR_INT_MAX_SHARE`` of the unmasked tokens.

Every fp64 reference is computed once per session (lru_cache) and shared, read-only.
"""
import functools

import numpy as np
import pytest
import torch

from _util import assert_close_fp32
from _vits_chain import oracle_chain
from oracle import glow_tts_ref, vits_text_ref
from test_glow_tts_gpu import ENC_MAX_ABS, ENC_REL_RMS, build_encoder
from test_vits_text_gpu import VT, _op_tol, _vits
from tts_amd import _native as N
from tts_amd import synthetic
from tts_amd.config import GLOW_TTS_ENCODER, VITS_SDP, VITS_TEXT_ENCODER
from tts_amd.tts import DurationPredictor, StochasticDurationPredictor, TextEncoder
from tts_amd.tts.vits_text import vits_durations, vits_expand

pytestmark = pytest.mark.gpu

B_STD, T_STD = 4, 259
LENS_STD = (259, 256, 65, 1)
NUM_CHARS = 64
TE_CFG = dict(VITS_TEXT_ENCODER, num_chars=NUM_CHARS)
TE_SEED, SDP_SEED, DP_SEED, NOISE_SEED = 3, 31, 41, 17
LANG, GIN = 4, 16
NEAR_INT = 1e-3            # |w - round(w)| of the fp64 duration below which ceil(w) is not compared
NEAR_INT_MAX_SHARE = 0.02  # of the unmasked tokens
ATTN_MAX_T = 3072          # text.hpp
EXPAND_MAX_TX = 16384      # text.hpp


def _mask(lens, T):
    return (torch.arange(T)[None] < torch.as_tensor(lens)[:, None]).float().unsqueeze(1)


def _lang_emb(B):
    return 0.5 * torch.randn(B, LANG, 1, generator=torch.Generator().manual_seed(19))


def _assert_exact(out, ref, what):
    """bit-for-bit agreement of values (integer / selection work), recorded like every other comparison"""
    assert_close_fp32(out.cpu().double(), ref.cpu().double(), what, max_abs_tol=0.0, rel_rms_tol=0.0)


def _assert_masked_zero(o, xm, what):
    o = o.cpu()
    pad = (xm == 0).expand_as(o)
    assert torch.count_nonzero(o[pad]) == 0, f"{what}: non-zero output at a masked position"


# ------------------------------------------------------------------------------- fp64 references
@functools.lru_cache(maxsize=None)
def _te_ref(B, T, lens, L):
    """(tokens, lengths, lang_emb or None, state dict, (x, m_p, logs_p, x_mask) in fp64)"""
    tok = synthetic.tokens(B, T, NUM_CHARS, seed=T + L)
    lens = torch.tensor(lens)
    le = _lang_emb(B) if L else None
    sd = synthetic.vits_text_encoder_state_dict(**TE_CFG, language_emb_dim=L, seed=TE_SEED)
    ref = vits_text_ref.text_encoder(sd, tok, lens, dtype=torch.float64, lang_emb=le, **TE_CFG)
    return tok, lens, le, sd, ref


def _sdp_noise():
    return torch.randn(B_STD, 2, T_STD, generator=torch.Generator().manual_seed(NOISE_SEED))


def _speaker_g():
    return torch.randn(B_STD, GIN, 1, generator=torch.Generator().manual_seed(23))


@functools.lru_cache(maxsize=None)
def _sdp_ref(noise_scale, cond):
    """(state dict, x fp32 [B, 192 (+ LANG), T], x_mask fp32, g, lang_emb, noise, logw fp64) on the
    oracle text encoder's output at the standard shape; ``cond``: speaker vector + language embedding"""
    L, gin = (LANG, GIN) if cond else (0, 0)
    _, _, le, _, (x, _, _, xm) = _te_ref(B_STD, T_STD, LENS_STD, L)
    g = _speaker_g() if cond else None
    noise = _sdp_noise()
    cfg = dict(VITS_SDP, in_channels=VITS_SDP["in_channels"] + L)
    sd = synthetic.vits_sdp_state_dict(**cfg, cond_channels=gin, language_emb_dim=L, seed=SDP_SEED)
    x = x.float()  # the device's input: both sides start from the same fp32 tensor
    logw = vits_text_ref.sdp_reverse(sd, x, xm, noise, g=None if g is None else g.double(), lang_emb=le,
                                     noise_scale=noise_scale, dtype=torch.float64, **VITS_SDP)
    return sd, x, xm.float(), g, le, noise, logw


def _sdp(dev, mode, cond):
    L, gin = (LANG, GIN) if cond else (0, 0)
    sdp = StochasticDurationPredictor(VITS_SDP["in_channels"], VITS_SDP["hidden_channels"], VITS_SDP["kernel_size"], 0.5,
                                      VITS_SDP["num_flows"], cond_channels=gin, language_emb_dim=L, math_mode=mode)
    sdp.load_state_dict(_sdp_ref(1.0, cond)[0])
    return sdp.to(dev)


def _sdp_logw(dev, mode, noise_scale, cond=False):
    _, x, xm, g, le, noise, ref = _sdp_ref(noise_scale, cond)
    logw = _sdp(dev, mode, cond)(x.to(dev), xm.to(dev), g=None if g is None else g.to(dev), reverse=True,
                                 noise_scale=noise_scale, lang_emb=None if le is None else le.to(dev),
                                 noise=noise.to(dev))
    return logw, xm, ref


def _near_integer(w64, xm):
    """(kept, share): the unmasked tokens whose fp64 duration is >= NEAR_INT from every integer, and
    the share of unmasked tokens left out"""
    un = xm.bool()
    near = (w64 - torch.round(w64)).abs() < NEAR_INT
    share = float((near & un).sum()) / float(un.sum())
    return un & ~near, share


# ------------------------------------------------------------------- 1. TextEncoder past one tile
@pytest.mark.parametrize("mode,L", [("fp32", 0), ("fp32x6", 0), ("bf16", 0), ("fp32x6", LANG)],
                         ids=["fp32", "fp32x6", "bf16", "fp32x6-lang4"])
def test_text_encoder_past_one_tile(cuda_device, mode, L):
    """x, m_p, logs_p at the standard shape against the fp64 oracle; x_mask exact; every output exactly
    0.0 at a masked position.  L = 4: embed_kernel's language channels over four 64-column blocks."""
    tok, lens, le, sd, (x64, m64, logs64, xm64) = _te_ref(B_STD, T_STD, LENS_STD, L)
    c = TE_CFG
    te = TextEncoder(c["num_chars"], c["out_channels"], c["hidden_channels"], c["hidden_channels_ffn"], c["num_heads"],
                     c["num_layers"], c["kernel_size"], 0.1, language_emb_dim=L or None, math_mode=mode)
    te.load_state_dict(sd)
    te = te.to(cuda_device)
    x, m, logs, xm = te(tok.to(cuda_device), lens.to(cuda_device), lang_emb=None if le is None else le.to(cuda_device))
    _assert_exact(xm, xm64, f"long TextEncoder x_mask T={T_STD} L={L} ({mode})")
    for n, o, r in (("x", x, x64), ("m_p", m, m64), ("logs_p", logs, logs64)):
        assert_close_fp32(o.cpu(), r, f"long TextEncoder {n} T={T_STD} L={L} ({mode})", **_op_tol(mode))
        _assert_masked_zero(o, xm64, f"{n} ({mode})")


# ------------------------------------------------------------- 2. duration predictors past one tile
@pytest.mark.parametrize("noise_scale", [0.0, 1.0, 4.0])
def test_sdp_reverse_past_one_tile(cuda_device, noise_scale):
    """logw at the standard shape (five 64-column depthwise workgroups with taps across every seam at
    dilations 1, 3, 9; two 256-position spline workgroups); noise_scale 4 takes the linear tails."""
    logw, _, ref = _sdp_logw(cuda_device, "fp32x6", noise_scale)
    assert_close_fp32(logw.cpu(), ref, f"long sdp logw T={T_STD} noise_scale={noise_scale}", **_op_tol("fp32x6"))


def test_sdp_reverse_speaker_and_language(cuda_device):
    """cond(g) + cond_lang(lang_emb): the per-utterance vectors summed in place (vec_add_kernel with
    out aliasing a), on the language-conditioned encoder's 196-channel x."""
    logw, _, ref = _sdp_logw(cuda_device, "fp32x6", 1.0, cond=True)
    assert_close_fp32(logw.cpu(), ref, f"long sdp logw T={T_STD} speaker+language", **_op_tol("fp32x6"))


def test_sdp_reverse_past_one_tile_bf16(cuda_device):
    logw, _, ref = _sdp_logw(cuda_device, "bf16", 1.0)
    assert_close_fp32(logw.cpu(), ref, f"long sdp logw T={T_STD} (bf16)", **_op_tol("bf16"))


@functools.lru_cache(maxsize=None)
def _dp_ref():
    _, x, xm, *_ = _sdp_ref(1.0, False)
    sd = synthetic.vits_dp_state_dict(VITS_TEXT_ENCODER["hidden_channels"], 256, 3, seed=DP_SEED)
    return sd, x, xm, vits_text_ref.dp_forward(sd, x, xm, dtype=torch.float64)


@pytest.mark.parametrize("mode", ["fp32x6", "bf16"])
def test_duration_predictor_past_one_tile(cuda_device, mode):
    """The deterministic DurationPredictor (use_sdp=False) over three 128-column conv tiles."""
    sd, x, xm, ref = _dp_ref()
    dp = DurationPredictor(VITS_TEXT_ENCODER["hidden_channels"], 256, 3, 0.5, math_mode=mode)
    dp.load_state_dict(sd)
    logw = dp.to(cuda_device)(x.to(cuda_device), xm.to(cuda_device))
    assert_close_fp32(logw.cpu(), ref, f"long dp logw T={T_STD} ({mode})", **_op_tol(mode))


# ------------------------------------------------------------------- 3. durations from those logw
@pytest.mark.parametrize("noise_scale", [0.0, 1.0])
def test_durations_from_long_logw(cuda_device, noise_scale):
    """vits_durations on the device's logw = ceil of the fp64 oracle's w at every unmasked token whose
    fp64 w is at least 1e-3 from an integer (at most 2 % are nearer; on the oracle alone 3 and 2 of
    581); masked tokens get 0 frames; y_lengths is the clamped sum of the device's own w_ceil."""
    logw, xm, ref = _sdp_logw(cuda_device, "fp32x6", noise_scale)
    w_ceil, y_len = vits_durations(logw, xm.to(cuda_device), 1.0)
    w_ceil = w_ceil.cpu()
    w64 = torch.exp(ref) * xm.double()
    keep, share = _near_integer(w64, xm)
    print(f"durations noise_scale={noise_scale}: near-integer share {share:.4f} of {int(xm.sum())} tokens")
    assert share <= NEAR_INT_MAX_SHARE
    _assert_exact(w_ceil[keep], torch.ceil(w64)[keep], f"long w_ceil noise_scale={noise_scale}")
    assert torch.count_nonzero(w_ceil[xm == 0]) == 0
    _assert_exact(y_len, torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long(), f"long y_lengths noise_scale={noise_scale}")


# ----------------------------------------- 4. alignment glue: seg > 1, several frame workgroups
TX_GLUE, LENS_GLUE, C_GLUE = 700, (700, 513, 2), 8


def test_glow_glue_scan_segments(cuda_device):
    """tts_glow_durations / tts_glow_expand at T_x = 700 (expand_kernel: three tokens per scan thread,
    three 256-frame workgroups) against glow_tts_ref.durations / expand run in fp32."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(43)
    B, Tx, C = len(LENS_GLUE), TX_GLUE, C_GLUE
    xm = _mask(LENS_GLUE, Tx)
    logw = 0.5 * torch.randn(B, 1, Tx, generator=gen)
    om = torch.randn(B, C, Tx, generator=gen)
    w_ceil = torch.empty(B, 1, Tx, device=dev)
    y_len = torch.empty(B, dtype=torch.int64, device=dev)
    dur = torch.empty(B, 1, Tx, device=dev)
    s = N.stream_ptr(dev)
    logw_d, xm_d, om_d = logw.to(dev), xm.to(dev), om.to(dev)  # held: N.ptr keeps no reference
    N.call("tts_glow_durations", N.ptr(logw_d), N.ptr(xm_d), B, Tx, 1.0, N.ptr(w_ceil), N.ptr(y_len), N.ptr(dur), s)
    ref_wc, _ = glow_tts_ref.durations(logw, xm)
    keep, share = _near_integer((torch.exp(logw.double()) - 1) * xm.double(), xm)
    print(f"glow glue: near-integer share {share:.4f} of {int(xm.sum())} tokens")
    assert share <= NEAR_INT_MAX_SHARE
    cmp = keep | (xm == 0)  # padded tokens: exactly 1 frame (clamp_min after the mask)
    _assert_exact(w_ceil.cpu()[cmp], ref_wc[cmp], f"glow glue w_ceil T_x={Tx}")
    # the rest on the device's own durations (identical to the reference's wherever compared above)
    wc = w_ceil.cpu()
    ref_yl = torch.clamp_min(torch.sum(wc, [1, 2]), 1).long()
    _assert_exact(y_len, ref_yl, f"glow glue y_lengths T_x={Tx}")
    Ty = int(ref_yl.max())
    assert Ty > 2 * 256
    noise = torch.randn(B, C, Ty, generator=gen)
    noise_d = noise.to(dev)
    z = torch.empty(B, C, Ty, device=dev)
    ym = torch.empty(B, 1, Ty, device=dev)
    ymean = torch.empty(B, C, Ty, device=dev)
    yls = torch.empty(B, C, Ty, device=dev)
    attn = torch.empty(B, Tx, Ty, device=dev)
    N.call("tts_glow_expand", N.ptr(w_ceil), N.ptr(xm_d), N.ptr(y_len), N.ptr(om_d), N.ptr(None), N.ptr(noise_d), 0.33,
           B, C, Tx, Ty, N.ptr(z), N.ptr(ym), N.ptr(ymean), N.ptr(yls), N.ptr(attn), s)
    rz, rym, rmean, _, rattn, _ = glow_tts_ref.expand(wc, xm, ref_yl, om, torch.zeros_like(om), noise, 0.33)
    _assert_exact(attn, rattn, f"glow glue attn T_x={Tx}")
    _assert_exact(ym, rym, f"glow glue y_mask T_x={Tx}")
    _assert_exact(ymean, rmean, f"glow glue y_mean T_x={Tx}")
    _assert_exact(yls, torch.zeros(B, C, Ty), f"glow glue y_log_scale T_x={Tx}")
    assert_close_fp32(z.cpu(), rz, f"glow glue z T_x={Tx}", max_abs_tol=1e-6)


def test_vits_expand_scan_segments(cuda_device):
    """vits_expand at T_x = 700 with integer durations cycling 0, 1, 2, 3 (a 0-frame token repeats its
    predecessor's cumsum, so the binary search must skip it): attn, y_mask and the gathered m_p /
    logs_p bit for bit against vits_text_ref.vits_expand."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(47)
    B, Tx, C = len(LENS_GLUE), TX_GLUE, C_GLUE
    xm = _mask(LENS_GLUE, Tx)
    wc = ((torch.arange(Tx)[None] + torch.arange(B)[:, None]) % 4).float().unsqueeze(1) * xm
    y_len = torch.clamp_min(torch.sum(wc, [1, 2]), 1).long()
    Ty = int(y_len.max())
    assert Ty > 4 * 256
    m_p = torch.randn(B, C, Tx, generator=gen)
    logs_p = 0.3 * torch.randn(B, C, Tx, generator=gen)
    noise = torch.randn(B, C, Ty, generator=gen)
    _, ym, mp, lp, attn = vits_expand(wc.to(dev), xm.to(dev), y_len.to(dev), m_p.to(dev), logs_p.to(dev),
                                      noise.to(dev), 0.667)
    _, rym, rmp, rlp, rattn = vits_text_ref.vits_expand(wc, xm, y_len, m_p, logs_p, noise, 0.667)
    _assert_exact(attn, rattn, f"vits expand attn T_x={Tx}")
    _assert_exact(ym, rym, f"vits expand y_mask T_x={Tx}")
    _assert_exact(mp, rmp, f"vits expand m_p T_x={Tx}")
    _assert_exact(lp, rlp, f"vits expand logs_p T_x={Tx}")


# --------------------------------------------- 5. attention past 64 KiB of LDS, and its token cap
def test_text_encoder_attention_past_64k_lds(cuda_device):
    """VITS TextEncoder, six layers, T = 901: attention_lds_bytes = 37,376 + 32 * 901 > 64 KiB, so
    launch_attention must raise the kernel's dynamic-LDS limit before it launches."""
    B, T, lens = 2, 901, (901, 450)
    tok, lens, _, sd, (x64, m64, logs64, xm64) = _te_ref(B, T, lens, 0)
    c = TE_CFG
    te = TextEncoder(c["num_chars"], c["out_channels"], c["hidden_channels"], c["hidden_channels_ffn"], c["num_heads"],
                     c["num_layers"], c["kernel_size"], 0.1, math_mode="fp32x6")
    te.load_state_dict(sd)
    x, m, logs, xm = te.to(cuda_device)(tok.to(cuda_device), lens.to(cuda_device))
    _assert_exact(xm, xm64, f"long TextEncoder x_mask T={T}")
    for n, o, r in (("x", x, x64), ("m_p", m, m64), ("logs_p", logs, logs64)):
        assert_close_fp32(o.cpu(), r, f"long TextEncoder {n} T={T}", **_op_tol("fp32x6"))
        _assert_masked_zero(o, xm64, n)


def _glow_one_layer_cfg(window):
    ep = dict(GLOW_TTS_ENCODER["encoder_params"], num_layers=1, rel_attn_window_size=window)
    return dict(GLOW_TTS_ENCODER, num_chars=50, encoder_params=ep)


@pytest.mark.parametrize("window", [None, 4])
def test_glow_encoder_at_attention_cap(cuda_device, window):
    """Glow Encoder (rel_pos_transformer, one layer) at exactly ATTN_MAX_T = 3072 tokens, the longest
    score row the attention kernel keeps in LDS (135,680 bytes)."""
    cfg = _glow_one_layer_cfg(window)
    T = ATTN_MAX_T
    e = build_encoder(cfg, 7, cuda_device, "fp32")
    tok = synthetic.tokens(1, T, 50, seed=T)
    lens = torch.tensor([T])
    outs = e(tok.to(cuda_device), lens.to(cuda_device))
    sd = synthetic.glow_encoder_state_dict(**cfg, seed=7)
    ref = glow_tts_ref.encoder_forward(sd, tok, lens, hidden_channels=192, encoder_params=cfg["encoder_params"],
                                       mean_only=True, use_prenet=True)
    for n, o, r in zip(["x_m", "x_logs", "logw"], outs, ref):
        assert_close_fp32(o.cpu(), r, f"{n} T={T} window={window}", ENC_MAX_ABS, ENC_REL_RMS)


def _small_encoder(kind, dev):
    if kind == "glow":
        return build_encoder(_glow_one_layer_cfg(4), 7, dev, "fp32")
    c = dict(TE_CFG, num_layers=1)
    te = TextEncoder(c["num_chars"], c["out_channels"], c["hidden_channels"], c["hidden_channels_ffn"], c["num_heads"],
                     c["num_layers"], c["kernel_size"], 0.1, math_mode="fp32")
    te.load_state_dict(synthetic.vits_text_encoder_state_dict(**c, seed=TE_SEED))
    return te.to(dev)


@pytest.mark.parametrize("kind", ["glow", "vits"])
def test_attention_cap_rejected(cuda_device, kind):
    """ATTN_MAX_T + 1 tokens: the host-side checks (before any attention launch) raise NativeError, and
    the same module then gives a T = 8 input the output it gave before the refused call, bit for bit."""
    e = _small_encoder(kind, cuda_device)
    tok8 = synthetic.tokens(2, 8, 50, seed=8).to(cuda_device)
    len8 = torch.tensor([8, 5], device=cuda_device)
    before = [o.clone() for o in e(tok8, len8)]
    T = ATTN_MAX_T + 1
    with pytest.raises(N.NativeError):
        e(synthetic.tokens(1, T, 50, seed=1).to(cuda_device), torch.tensor([T], device=cuda_device))
    after = e(tok8, len8)
    for i, (a, b) in enumerate(zip(before, after)):
        _assert_exact(b, a, f"{kind} encoder output {i} after the refused T={T} call")


# --------------------------------------------------------------------- 6. expansion at its cap
def _cap_durations(Tx):
    gen = torch.Generator().manual_seed(53)
    wc = torch.zeros(1, 1, Tx)
    idx = torch.randperm(Tx - 1, generator=gen)[:300]
    wc[0, 0, idx] = torch.randint(1, 4, (300,), generator=gen).float()
    wc[0, 0, Tx - 1] = 2.0
    return wc, gen


def test_vits_expand_at_token_cap(cuda_device):
    """EXPAND_MAX_TX = 16384 tokens in one utterance: 64 tokens per scan thread, a 64 KiB cumsum in
    dynamic LDS beside the 1 KiB of static partials.  300 random tokens carry 1-3 frames, the rest 0,
    the last token 2: the gathered m_p / logs_p and y_mask bit for bit against the oracle."""
    dev = cuda_device
    Tx, C = EXPAND_MAX_TX, 8
    wc, gen = _cap_durations(Tx)
    xm = torch.ones(1, 1, Tx)
    y_len = torch.sum(wc, [1, 2]).long()
    m_p = torch.randn(1, C, Tx, generator=gen)
    logs_p = 0.3 * torch.randn(1, C, Tx, generator=gen)
    noise = torch.randn(1, C, int(y_len.max()), generator=gen)
    _, ym, mp, lp, attn = vits_expand(wc.to(dev), xm.to(dev), y_len.to(dev), m_p.to(dev), logs_p.to(dev), noise.to(dev),
                                      0.667, want_attn=False)
    assert attn is None
    _, rym, rmp, rlp, _ = vits_text_ref.vits_expand(wc, xm, y_len, m_p, logs_p, noise, 0.667)
    _assert_exact(ym, rym, f"vits expand y_mask T_x={Tx}")
    _assert_exact(mp, rmp, f"vits expand m_p T_x={Tx}")
    _assert_exact(lp, rlp, f"vits expand logs_p T_x={Tx}")


def test_vits_expand_past_token_cap_rejected(cuda_device):
    """EXPAND_MAX_TX + 1 tokens: launch_expand's host check raises before the launch."""
    dev = cuda_device
    Tx, C = EXPAND_MAX_TX + 1, 8
    wc, _ = _cap_durations(Tx)
    y_len = torch.sum(wc, [1, 2]).long()
    with pytest.raises(N.NativeError):
        vits_expand(wc.to(dev), torch.ones(1, 1, Tx, device=dev), y_len.to(dev), torch.zeros(1, C, Tx, device=dev),
                    torch.zeros(1, C, Tx, device=dev), torch.zeros(1, C, int(y_len.max()), device=dev), 0.667,
                    want_attn=False)


# ------------------------------------------------------------------------ 7. one end-to-end row
def test_vits_inference_long_given_durations(cuda_device):
    """Vits.inference (tokens -> waveform) at [2, 259] tokens, lengths [259, 130], with given durations
    cycling 0, 1, 2, 3 (T_y = 387: no ceil to flake), against the fp64 chain on the same durations."""
    d = cuda_device
    name, meta, arr = VT[0]
    B, T = 2, T_STD
    tok = synthetic.tokens(B, T, meta["text_encoder"]["num_chars"], seed=61)
    lens = torch.tensor([259, 130])
    dur = (torch.arange(T) % 4).float().reshape(1, T)
    T_y = int(dur.sum())
    noise_z = torch.randn(B, 192, T_y, generator=torch.Generator().manual_seed(67))
    v = _vits(meta, d, "fp32x6", "f16x3", "f16x3", arr=arr)
    out = v.inference(tok.to(d), {"x_lengths": lens.to(d), "durations": dur.to(d), "noise_z": noise_z.to(d)})
    wc = dur.reshape(1, 1, T).expand(B, 1, T).contiguous()
    # the chain's own duration predictor is replaced by w_ceil; it still wants a draw of this shape
    arr2 = dict(arr, tokens=tok.numpy(), lengths=lens.numpy(), noise_dp=np.zeros((B, 2, T), np.float32))
    ref = oracle_chain(meta, arr2, w_ceil=wc, noise_z=noise_z)
    _assert_exact(out["durations"], wc, f"{name} long durations")
    _assert_exact(out["alignments"], ref["attn"], f"{name} long alignments")
    assert_close_fp32(out["z"].cpu(), ref["z"], f"{name} long z (given durations)", max_abs_tol=1e-4)
    assert_close_fp32(out["model_outputs"].cpu(), ref["wav"], f"{name} long wav (given durations)")
