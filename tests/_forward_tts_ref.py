"""fp64 / fp32 oracle of ForwardTTS (FastPitch) for the tests: a ``torch.nn.functional`` restatement of
``TTS/tts/models/forward_tts.py`` (inference), ``layers/generic/transformer.py``,
``layers/feed_forward/{encoder,decoder}.py``, ``layers/generic/pos_encoding.py`` and
``layers/glow_tts/duration_predictor.py`` (Coqui TTS 0.22.0) that works from a state dict, with a MAC
counter.  The attention is torch's own ``F.multi_head_attention_forward``; ``mha_from_qkv`` is its
attention proper (identity projections) for the op tests.  Shares no code with ``tts_amd``."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def key_padding_mask(lengths, T: int):
    """True = padded key (``~sequence_mask(lengths, T)``); None without lengths."""
    if lengths is None:
        return None
    return torch.arange(T)[None, :] >= torch.as_tensor(lengths)[:, None]


def mha_from_qkv(qkv, heads: int, key_lengths=None, dtype=torch.float64):
    """``qkv`` [B, 3E, T] (rows q | k | v: the in_proj output, heads as contiguous channel blocks) ->
    (out [B, E, T] before out_proj, probabilities [B, heads, T, T]).  The projections are identities
    (exact), so this is torch's scaling, masking (-inf under the key padding mask) and softmax."""
    B, E3, T = qkv.shape
    E = E3 // 3
    q, k, v = (t.permute(2, 0, 1).to(dtype) for t in qkv.split(E, 1))
    eye = torch.eye(E, dtype=dtype)
    out, w = F.multi_head_attention_forward(
        q, k, v, E, heads, in_proj_weight=None, in_proj_bias=None, bias_k=None, bias_v=None, add_zero_attn=False,
        dropout_p=0.0, out_proj_weight=eye, out_proj_bias=None, training=False,
        key_padding_mask=key_padding_mask(key_lengths, T), need_weights=True, use_separate_proj_weight=True,
        q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye, average_attn_weights=False)
    return out.permute(1, 2, 0), w


def scores(qkv, heads: int):
    """The scaled scores (q dk^-0.5)^T k in fp64: [B, heads, T, T]."""
    B, E3, T = qkv.shape
    E = E3 // 3
    dk = E // heads
    q, k, _ = (t.double().reshape(B, heads, dk, T) for t in qkv.split(E, 1))
    return torch.einsum("bhdi,bhdj->bhij", q * dk**-0.5, k)


def mha_macs(B: int, E: int, T: int, T_keys: int | None = None) -> int:
    """Multiply-accumulates of the two products (Q K^T and P V): E per (query, key) pair each."""
    return 2 * B * E * T * (T if T_keys is None else T_keys)


# ------------------------------------------------------------------ the model
MAX_FRAMES = 5000


def _count(counter, name, macs):
    if counter is not None:
        counter[name] = counter.get(name, 0) + int(macs)


def fft_layer(sd, pre: str, x, heads: int, kpm, dtype, probs=None, counter=None, tag="fft"):
    """``FFTransformer.forward``: x [B, C, T] -> [B, C, T]; ``kpm`` [B, T] bool or None."""
    g = lambda n: sd[pre + n].to(dtype)  # noqa: E731
    B, C, T = x.shape
    src = x.permute(2, 0, 1)
    src2, w = F.multi_head_attention_forward(
        src, src, src, C, heads, g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias"), None, None, False, 0.0,
        g("self_attn.out_proj.weight"), g("self_attn.out_proj.bias"), training=False, key_padding_mask=kpm,
        need_weights=probs is not None, average_attn_weights=False)  # as the reference's [0]: torch's fused path
    if probs is not None:
        probs.append((tag, w))
    _count(counter, f"{tag}.in_proj", 3 * C * C * B * T)
    _count(counter, f"{tag}.attn", mha_macs(B, C, T))
    _count(counter, f"{tag}.out_proj", C * C * B * T)
    src = src + src2
    src = F.layer_norm(src + src2, (C,), g("norm1.weight"), g("norm1.bias"), 1e-5)  # LN(x + 2 a), as the reference
    src = src.permute(1, 2, 0)
    w1, w2 = g("conv1.weight"), g("conv2.weight")
    p = (w1.shape[-1] - 1) // 2
    src2 = F.conv1d(F.relu(F.conv1d(src, w1, g("conv1.bias"), padding=p)), w2, g("conv2.bias"), padding=p)
    _count(counter, f"{tag}.ffn", (w1.numel() + w2.numel()) * B * T)
    src = src + src2
    return F.layer_norm(src.transpose(1, 2), (C,), g("norm2.weight"), g("norm2.bias"), 1e-5).transpose(1, 2)


def fft_block(sd, pre: str, x, heads: int, num_layers: int, mask=None, dtype=torch.float64, probs=None,
              counter=None, tag="fft"):
    """``FFTransformerBlock.forward``: ``mask`` [B, 1, T] or None; nothing but the keys is masked."""
    kpm = None if mask is None else ~mask.squeeze(1).bool()
    x = x.to(dtype)
    for i in range(num_layers):
        x = fft_layer(sd, f"{pre}fft_layers.{i}.", x, heads, kpm, dtype, probs, counter, tag)
    return x


def duration_predictor(sd, pre: str, x, m, dtype, counter=None):
    g = lambda n: sd[pre + n].to(dtype)  # noqa: E731

    def norm(v, n):
        mean = v.mean(1, keepdim=True)
        var = ((v - mean) ** 2).mean(1, keepdim=True)
        return (v - mean) * torch.rsqrt(var + 1e-4) * g(n + ".gamma") + g(n + ".beta")

    k = sd[pre + "conv_1.weight"].shape[-1]
    cols = x.shape[0] * x.shape[-1]
    for n in ("conv_1", "conv_2", "proj"):
        _count(counter, pre + n, sd[f"{pre}{n}.weight"].numel() * cols)
    x = norm(F.relu(F.conv1d(x * m, g("conv_1.weight"), g("conv_1.bias"), padding=k // 2)), "norm_1")
    x = norm(F.relu(F.conv1d(x * m, g("conv_2.weight"), g("conv_2.bias"), padding=k // 2)), "norm_2")
    return F.conv1d(x * m, g("proj.weight"), g("proj.bias")) * m


def make_pe(C: int, max_len: int = MAX_FRAMES) -> torch.Tensor:
    """The ``pe`` buffer [1, C, max_len] as ``PositionalEncoding.__init__`` builds it (fp32)."""
    pe = torch.zeros(max_len, C)
    position = torch.arange(0, max_len).unsqueeze(1)
    div_term = torch.pow(10000, torch.arange(0, C, 2).float() / C)
    pe[:, 0::2] = torch.sin(position.float() / div_term)
    pe[:, 1::2] = torch.cos(position.float() / div_term)
    return pe.unsqueeze(0).transpose(1, 2).contiguous()


def round_durations(raw):
    """``o_dr[o_dr < 1] = 1.0; o_dr = torch.round(o_dr)`` (half to even)."""
    o_dr = raw.clone()
    o_dr[o_dr < 1] = 1.0
    return torch.round(o_dr)


def format_durations(o_dr_log, x_mask, length_scale=1.0):
    """(rounded durations [B, T_en], the value before the clamp and the rounding)."""
    raw = (torch.exp(o_dr_log) - 1) * x_mask * length_scale
    return round_durations(raw).squeeze(1), raw.squeeze(1)


def generate_path(dur, x_mask, y_mask):
    """attn [B, T_en, T_de]: token i covers frames [cum[i-1], cum[i]), times both masks."""
    cum = torch.cumsum(dur, 1)
    j = torch.arange(y_mask.shape[-1], dtype=dur.dtype, device=dur.device)[None, None, :]
    path = ((j < cum[:, :, None]) & (j >= (cum - dur)[:, :, None])).to(dur.dtype)
    return path * x_mask.squeeze(1)[:, :, None] * y_mask


def inference(sd, args: dict, x, x_lengths=None, speaker_ids=None, durations=None, mask_decoder_keys=False,
              dtype=torch.float64, counter=None, probs=None):
    """``ForwardTTS.inference`` with the three extensions of the device path (``x_lengths``, given
    ``durations``, ``mask_decoder_keys``), each off by default.  Returns the reference's dict plus
    ``durations`` (rounded, [B, T_en]) and ``durations_raw`` (before the clamp and the rounding)."""
    H = args["hidden_channels"]
    ep, dp = args["encoder_params"], args["decoder_params"]
    B, T_en = x.shape
    dev = x.device  # the benchmark runs this restatement on the GPU
    if x_lengths is None:
        x_mask = torch.ones(B, 1, T_en, dtype=dtype, device=dev)
    else:
        x_mask = (torch.arange(T_en, device=dev)[None, :] < torch.as_tensor(x_lengths, device=dev)[:, None]).to(dtype).unsqueeze(1)
    o_en = sd["emb.weight"].to(dtype)[x].transpose(1, 2)
    o_en = fft_block(sd, "encoder.encoder.", o_en, ep["num_heads"], ep["num_layers"], x_mask, dtype, probs,
                     counter, "encoder") * x_mask
    if "emb_g.weight" in sd:
        o_en = o_en + sd["emb_g.weight"].to(dtype)[speaker_ids].unsqueeze(-1)
    o_dr_log = duration_predictor(sd, "duration_predictor.", o_en, x_mask, dtype, counter)
    o_dr, raw = format_durations(o_dr_log, x_mask, float(args.get("length_scale", 1.0)))
    if x_lengths is not None:
        o_dr = o_dr * x_mask.squeeze(1)  # extension: padded tokens get no frames
    if durations is not None:
        o_dr = torch.as_tensor(durations).to(device=dev, dtype=dtype)
    y_lengths = o_dr.sum(1)
    o_pitch = None
    if args.get("use_pitch", True):
        o_pitch = duration_predictor(sd, "pitch_predictor.", o_en, x_mask, dtype, counter)
        kp = sd["pitch_emb.weight"].shape[-1]
        o_en = o_en + F.conv1d(o_pitch, sd["pitch_emb.weight"].to(dtype), sd["pitch_emb.bias"].to(dtype),
                               padding=(kp - 1) // 2)
    T_de = int(y_lengths.max().item())
    y_mask = (torch.arange(T_de, device=dev)[None, :] < y_lengths[:, None]).to(dtype).unsqueeze(1)
    attn = generate_path(o_dr, x_mask, y_mask)
    o_en_ex = torch.matmul(attn.transpose(1, 2), o_en.transpose(1, 2)).transpose(1, 2)
    if "pos_encoder.pe" in sd:
        if T_de > MAX_FRAMES:
            raise RuntimeError("more frames than the positional encoding holds")
        o_en_ex = o_en_ex * torch.tensor(float(H), dtype=dtype).sqrt() + sd["pos_encoder.pe"].to(dtype)[:, :, :T_de] * y_mask
    o = fft_block(sd, "decoder.decoder.transformer_block.", o_en_ex, dp["num_heads"], dp["num_layers"],
                  y_mask if mask_decoder_keys else None, dtype, probs, counter, "decoder") * y_mask
    wp = sd["decoder.decoder.postnet.weight"].to(dtype)
    _count(counter, "decoder.postnet", wp.numel() * B * T_de)
    o_de = F.conv1d(o, wp, sd["decoder.decoder.postnet.bias"].to(dtype)) * y_mask
    return {"model_outputs": o_de.transpose(1, 2), "alignments": attn.transpose(1, 2), "pitch": o_pitch,
            "energy": None, "durations_log": o_dr_log, "durations": o_dr, "durations_raw": raw,
            "decoder_input": o_en_ex, "y_mask": y_mask}


def decoder(sd, args: dict, o_en_ex, y_mask, mask_decoder_keys=False, dtype=torch.float64):
    """``Decoder.forward`` on a given input: [B, H, T_de] -> model_outputs [B, T_de, out]."""
    dp = args["decoder_params"]
    y_mask = y_mask.to(dtype)
    o = fft_block(sd, "decoder.decoder.transformer_block.", o_en_ex, dp["num_heads"], dp["num_layers"],
                  y_mask if mask_decoder_keys else None, dtype) * y_mask
    o_de = F.conv1d(o, sd["decoder.decoder.postnet.weight"].to(dtype), sd["decoder.decoder.postnet.bias"].to(dtype))
    return (o_de * y_mask).transpose(1, 2)
