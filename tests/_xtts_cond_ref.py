"""fp64 (or fp32) oracle of XTTS voice cloning, written from the description in DESIGN.md section 4
"XTTS conditioning" (Coqui TTS 0.22.0: ``TTS/tts/layers/xtts/latent_encoder.py``, ``perceiver_encoder.py``,
``gpt.py`` ``get_style_emb``, ``TTS/tts/models/xtts.py``, torchaudio's ``MelSpectrogram`` and
``functional.resample``) on a state dict, in plain torch, for clarity rather than speed.  It shares no
code with ``tts_amd``.

Every function takes ``dtype`` (torch.float64 by default); at ``dtype=torch.float32`` on the device it is the
torch-eager side of scripts/xtts_cond_bench.py."""
import functools
import math

import torch
import torch.nn.functional as F

N_FFT, HOP, WIN, N_MELS, SR, F_MAX = 2048, 256, 1024, 80, 22050, 8000.0


# ------------------------------------------------------------------------------------------ front end
@functools.lru_cache(maxsize=None)
def mel_filterbank(n_freqs=N_FFT // 2 + 1, f_min=0.0, f_max=F_MAX, n_mels=N_MELS, sample_rate=SR):
    """torchaudio melscale_fbanks(..., norm="slaney", mel_scale="htk"): fb [n_freqs, n_mels], fp64."""
    hz2mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)  # noqa: E731
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_pts = torch.linspace(hz2mel(f_min), hz2mel(f_max), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    fb = torch.zeros(n_freqs, n_mels, dtype=torch.float64)
    for m in range(n_mels):  # triangle m: rises over [f_m, f_m+1], falls over [f_m+1, f_m+2], area-normalised
        lo, mid, hi = f_pts[m], f_pts[m + 1], f_pts[m + 2]
        tri = torch.minimum((all_freqs - lo) / (mid - lo), (hi - all_freqs) / (hi - mid)).clamp(min=0.0)
        fb[:, m] = tri * (2.0 / (hi - lo))
    return fb


def mel_constants(device, dtype):
    """(window, filterbank) on ``device`` in ``dtype``: what torchaudio's MelSpectrogram module keeps as buffers."""
    win = torch.hann_window(WIN, periodic=True, dtype=torch.float64).to(device=device, dtype=dtype)
    return win, mel_filterbank().to(device=device, dtype=dtype)


def wav_to_mel_cloning(wav, mel_norms, dtype=torch.float64, constants=None):
    """wav [B, N] at 22 050 Hz -> log(clamp(fb^T |STFT|^2, 1e-5)) / mel_norms[:, None], [B, 80, 1 + N // 256].
    ``constants``: mel_constants(device, dtype) built once by the caller (a timed caller keeps them resident)."""
    x = wav.to(dtype)
    win, fb = constants if constants is not None else mel_constants(x.device, dtype)
    X = torch.stft(x, N_FFT, hop_length=HOP, win_length=WIN, window=win, center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    power = X.real**2 + X.imag**2
    mel = torch.matmul(power.transpose(1, 2), fb).transpose(1, 2)
    return torch.log(torch.clamp(mel, min=1e-5)) / mel_norms.to(device=x.device, dtype=dtype)[None, :, None]


def resample_table(orig, new):
    """(kern [n, 2 w + o] fp64, o, n, w) of torchaudio's sinc_interp_hann resampler (width 6, rolloff 0.99)."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    w = int(math.ceil(6 * o / base))
    kern = torch.zeros(n, 2 * w + o, dtype=torch.float64)
    for p in range(n):
        for k in range(2 * w + o):
            t = (-p / n + (k - w) / o) * base
            t = max(-6.0, min(6.0, t))
            s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            kern[p, k] = s * math.cos(math.pi * t / 12.0) ** 2 * base / o
    return kern, o, n, w


def resample(x, orig, new, dtype=torch.float64, table=None, kernel=None):
    """x [B, N] -> [B, ceil(n N / o)]: y[f n + p] = sum_k kern[p][k] xpad[f o + k], xpad padded by (w, w + o).
    The table is stored fp32, as the library stores it."""
    if orig == new:
        return x.to(dtype)
    kern, o, n, w = table if table is not None else resample_table(orig, new)
    kern = kernel if kernel is not None else kern.float().to(dtype)  # kernel: the same, resident with the caller
    B, N = x.shape
    xp = F.pad(x.to(dtype), (w, w + o))
    y = F.conv1d(xp[:, None], kern[:, None], stride=o)  # [B, n, frames]
    y = y.transpose(1, 2).reshape(B, -1)
    return y[:, : -(-n * N // o)]


# -------------------------------------------------------------------------------------------- encoder
def normalization_groups(channels):
    groups = 32
    if channels <= 16:
        groups = 8
    elif channels <= 64:
        groups = 16
    while channels % groups != 0:
        groups = int(groups / 2)
    return groups


def group_norm(x, groups, weight, bias, eps=1e-5):
    """x [B, C, T]: statistics over (C / groups channels x T) per (b, group), written out."""
    B, C, T = x.shape
    xg = x.reshape(B, groups, (C // groups) * T)
    mean = xg.mean(dim=2, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=2, keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(B, C, T)
    return y * weight[None, :, None] + bias[None, :, None]


def qkv_attention(qkv, heads):
    """QKVAttentionLegacy: qkv [B, 3E, T], the 3E channels head-major and interleaved -> [B, E, T]."""
    B, W, T = qkv.shape
    ch = W // (3 * heads)
    q, k, v = qkv.reshape(B * heads, 3 * ch, T).split(ch, dim=1)
    scale = 1.0 / math.sqrt(math.sqrt(ch))
    w = torch.einsum("bct,bcs->bts", q * scale, k * scale)
    w = torch.softmax(w, dim=-1)
    a = torch.einsum("bts,bcs->bct", w, v)
    return a.reshape(B, heads * ch, T)


def attention_block(sd, pre, x, heads):
    C = x.shape[1]
    dt = x.dtype
    xn = group_norm(x, normalization_groups(C), sd[pre + "norm.weight"].to(dt), sd[pre + "norm.bias"].to(dt))
    qkv = F.conv1d(xn, sd[pre + "qkv.weight"].to(dt), sd[pre + "qkv.bias"].to(dt))
    a = qkv_attention(qkv, heads)
    h = F.conv1d(a, sd[pre + "proj_out.weight"].to(dt), sd[pre + "proj_out.bias"].to(dt))
    return xn + h  # the residual is the normalised input (x = norm(x) in the reference's forward)


def conditioning_encoder(sd, mel, heads, dtype=torch.float64, pre="conditioning_encoder."):
    """mel [B, 80, T] -> h [B, E, T]."""
    h = F.conv1d(mel.to(dtype), sd[pre + "init.weight"].to(dtype), sd[pre + "init.bias"].to(dtype))
    i = 0
    while f"{pre}attn.{i}.norm.weight" in sd:
        h = attention_block(sd, f"{pre}attn.{i}.", h, heads)
        i += 1
    return h


# ------------------------------------------------------------------------------------------ perceiver
def perceiver_attention(sd, pre, lat, ctx, heads, dim_head):
    """lat [B, L, E], ctx [B, T, E] -> lat + to_out(attention): keys and values from cat(lat, ctx)."""
    dt = lat.dtype
    B, L, _ = lat.shape
    kvin = torch.cat((lat, ctx), dim=1)
    q = lat @ sd[pre + "to_q.weight"].to(dt).T
    k, v = (kvin @ sd[pre + "to_kv.weight"].to(dt).T).chunk(2, dim=-1)
    split = lambda t: t.reshape(B, t.shape[1], heads, dim_head).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = split(q), split(k), split(v)
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * dim_head**-0.5
    attn = torch.softmax(sim, dim=-1)
    o = torch.einsum("bhij,bhjd->bhid", attn, v).permute(0, 2, 1, 3).reshape(B, L, heads * dim_head)
    return o @ sd[pre + "to_out.weight"].to(dt).T + lat


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def feed_forward(w0, b0, w2, b2, lat):
    """lat [.., E] -> lat + W2 (gelu(gate) x) + b2, [x | gate] = W0 lat + b0."""
    u = lat @ w0.T + b0
    x, gate = u.chunk(2, dim=-1)
    return (gelu_erf(gate) * x) @ w2.T + b2 + lat


def rms_norm(x, gamma):
    """x [.., E]: x / max(||x||, 1e-12) sqrt(E) gamma."""
    norm = torch.sqrt((x * x).sum(dim=-1, keepdim=True)).clamp(min=1e-12)
    return x / norm * math.sqrt(x.shape[-1]) * gamma


def perceiver(sd, ctx, heads=8, dim_head=64, dtype=torch.float64, pre="conditioning_perceiver."):
    """ctx [B, T, E] -> [B, L, E]."""
    B = ctx.shape[0]
    lat = sd[pre + "latents"].to(dtype)[None].expand(B, -1, -1)
    i = 0
    while f"{pre}layers.{i}.0.to_q.weight" in sd:
        lp = f"{pre}layers.{i}."
        lat = perceiver_attention(sd, lp + "0.", lat, ctx, heads, dim_head)
        lat = feed_forward(sd[lp + "1.0.weight"].to(dtype), sd[lp + "1.0.bias"].to(dtype),
                           sd[lp + "1.2.weight"].to(dtype), sd[lp + "1.2.bias"].to(dtype), lat)
        i += 1
    return rms_norm(lat, sd[pre + "norm.gamma"].to(dtype))


def style_emb(sd, mel, heads, perceiver_heads=8, dim_head=64, dtype=torch.float64):
    """gpt.py get_style_emb: mel [B, 80, T] (or [B, 1, 80, T]) -> [B, E, L]."""
    if mel.dim() == 4:
        mel = mel.squeeze(1)
    h = conditioning_encoder(sd, mel, heads, dtype)
    return perceiver(sd, h.permute(0, 2, 1), perceiver_heads, dim_head, dtype).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ Xtts
def gpt_cond_latents(sd, audio, sr, mel_norms, heads, length=30, chunk_length=6, dtype=torch.float64,
                     perceiver_heads=8, dim_head=64, constants=None):
    """audio [1, N] at sr -> [1, L, E]: the mean over the chunks' style embeddings, in chunk order."""
    audio = audio.to(dtype)
    if sr != SR:
        audio = resample(audio, sr, SR, dtype)
    if length > 0:
        audio = audio[:, : SR * length]
    embs = []
    for i in range(0, audio.shape[1], SR * chunk_length):
        chunk = audio[:, i : i + SR * chunk_length]
        if chunk.shape[-1] < SR * 0.33:
            continue
        mel = wav_to_mel_cloning(chunk, mel_norms, dtype, constants)
        embs.append(style_emb(sd, mel, heads, perceiver_heads, dim_head, dtype))
    total = embs[0]
    for e in embs[1:]:
        total = total + e
    return (total / len(embs)).transpose(1, 2), len(embs)
