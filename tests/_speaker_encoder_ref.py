"""fp64 / fp32 oracle of Coqui's ``ResNetSpeakerEncoder`` (TTS/encoder/models/resnet.py,
base_encoder.py) written from its description, on a state dict, with torch's own ``F.conv2d``,
``F.batch_norm``, ``torch.stft`` and ``F.instance_norm``.  It shares no code with ``tts_amd``.

``weight_cast``: applied to the operands of the trunk's convs and of the two attention convs (weights
and inputs), e.g. ``lambda t: t.bfloat16().to(t.dtype)`` to emulate the bf16 math mode; everything
else stays in ``dtype``."""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def mel_filterbank(n_freqs, sample_rate, n_mels, dtype=torch.float64):
    """melscale_fbanks(n_freqs, 0, sr / 2, n_mels, sr, norm=None, "htk") -> [n_freqs, n_mels]."""
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)  # noqa: E731
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_pts = torch.linspace(hz2mel(0.0), hz2mel(sample_rate / 2.0), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0).to(dtype)


def _get(sd, key, dtype):
    return sd[key].to(dtype)


def _bn(sd, pre, x, dtype):
    return F.batch_norm(x, _get(sd, pre + ".running_mean", dtype), _get(sd, pre + ".running_var", dtype),
                        _get(sd, pre + ".weight", dtype), _get(sd, pre + ".bias", dtype), False, 0.0, BN_EPS)


def torch_spec(sd, wav, audio_config, dtype=torch.float64):
    """PreEmphasis + MelSpectrogram(center=True, reflect, power 2, hamming window): [B, N] -> [B, n_mels, T]."""
    ac = audio_config
    x = wav.to(dtype)
    filt = _get(sd, "torch_spec.0.filter", dtype)  # [1, 1, 2] = [-coef, 1]
    x = F.conv1d(F.pad(x.unsqueeze(1), (1, 0), "reflect"), filt).squeeze(1)
    win = _get(sd, "torch_spec.1.spectrogram.window", dtype)
    X = torch.stft(x, ac["fft_size"], hop_length=ac["hop_length"], win_length=ac["win_length"], window=win, center=True,
                   pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    power = X.real**2 + X.imag**2  # [B, n_freqs, T]
    fb = _get(sd, "torch_spec.1.mel_scale.fb", dtype)  # [n_freqs, n_mels]
    return torch.matmul(power.transpose(1, 2), fb).transpose(1, 2)


def features(sd, x, log_input, use_torch_spec, audio_config=None, dtype=torch.float64):
    """The trunk's input [B, input_dim, T]: front end, log, instance norm."""
    x = x.to(dtype)
    if use_torch_spec:
        x = torch_spec(sd, x, audio_config, dtype)
    if log_input:
        x = (x + 1e-6).log()
    return F.instance_norm(x, eps=1e-5)


def _block(sd, p, x, stride, dtype, cast):
    out = F.conv2d(cast(x), cast(_get(sd, p + ".conv1.weight", dtype)), None, stride=stride, padding=1)
    out = _bn(sd, p + ".bn1", torch.relu(out), dtype)
    out = F.conv2d(cast(out), cast(_get(sd, p + ".conv2.weight", dtype)), None, padding=1)
    out = _bn(sd, p + ".bn2", out, dtype)
    y = out.mean(dim=(2, 3))
    y = torch.relu(F.linear(y, _get(sd, p + ".se.fc.0.weight", dtype), _get(sd, p + ".se.fc.0.bias", dtype)))
    y = torch.sigmoid(F.linear(y, _get(sd, p + ".se.fc.2.weight", dtype), _get(sd, p + ".se.fc.2.bias", dtype)))
    out = out * y[:, :, None, None]
    res = x
    if p + ".downsample.0.weight" in sd:
        res = F.conv2d(cast(x), cast(_get(sd, p + ".downsample.0.weight", dtype)), None, stride=stride)
        res = _bn(sd, p + ".downsample.1", res, dtype)
    return torch.relu(out + res)


def forward(sd, x, layers, encoder_type="ASP", log_input=False, use_torch_spec=False, audio_config=None, l2_norm=False,
            dtype=torch.float64, weight_cast=None):
    """x: [B, N] wav (use_torch_spec) or [B, input_dim, T] features -> [B, proj_dim]."""
    cast = weight_cast or (lambda t: t)
    x = features(sd, x, log_input, use_torch_spec, audio_config, dtype).unsqueeze(1)
    x = F.conv2d(cast(x), cast(_get(sd, "conv1.weight", dtype)), _get(sd, "conv1.bias", dtype), padding=1)
    x = _bn(sd, "bn1", torch.relu(x), dtype)
    for li, n in enumerate(layers):
        for i in range(n):
            x = _block(sd, f"layer{li + 1}.{i}", x, 2 if (li > 0 and i == 0) else 1, dtype, cast)
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    a = F.conv1d(cast(x), cast(_get(sd, "attention.0.weight", dtype)), _get(sd, "attention.0.bias", dtype))
    a = _bn(sd, "attention.2", torch.relu(a), dtype)
    a = F.conv1d(cast(a), cast(_get(sd, "attention.3.weight", dtype)), _get(sd, "attention.3.bias", dtype))
    w = torch.softmax(a, dim=2)
    mu = torch.sum(x * w, dim=2)
    if encoder_type == "ASP":
        sg = torch.sqrt((torch.sum((x**2) * w, dim=2) - mu**2).clamp(min=1e-5))
        x = torch.cat((mu, sg), 1)
    else:
        x = mu
    x = F.linear(x, _get(sd, "fc.weight", dtype), _get(sd, "fc.bias", dtype))
    if l2_norm:
        x = F.normalize(x, p=2, dim=1)
    return x


def compute_embedding(sd, x, layers, hop_length=None, num_frames=250, num_eval=10, return_mean=True, l2_norm=True, **kw):
    """x: [1, N] wav.  The windows are concatenated on the batch axis and run in one forward."""
    if kw.get("use_torch_spec"):
        num_frames = num_frames * hop_length
    max_len = x.shape[1]
    num_frames = min(num_frames, max_len)
    offsets = np.linspace(0, max_len - num_frames, num=num_eval)
    batch = torch.cat([x[:, int(o):int(o + num_frames)] for o in offsets], dim=0)
    emb = forward(sd, batch, layers, l2_norm=l2_norm, **kw)
    return emb.mean(dim=0, keepdim=True) if return_mean else emb


def bf16_cast(t):
    return t.to(torch.bfloat16).to(t.dtype)
