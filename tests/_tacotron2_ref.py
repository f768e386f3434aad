"""Oracle of Tacotron2 inference (``TTS/tts/models/tacotron2.py``, ``layers/tacotron/{tacotron2,attentions,
common_layers}.py``, Coqui TTS 0.22.0) that works from a state dict in fp64 or fp32, with a MAC counter.
It shares no code with ``tts_amd`` and leans on torch's own ``F.conv1d`` / ``F.batch_norm`` /
``nn.LSTM`` / ``nn.LSTMCell`` / ``pack_padded_sequence``; the only hand-written recurrence is the
attention state and the stop bookkeeping.

Batched semantics (the reference's loop only works at B = 1): with ``x_lengths`` the biLSTM is packed
and the attention masks keys at or past the length; utterance b ends at its own first step t >= 1 with
stop_b > stop_threshold (or at max_decoder_steps), rows after its last step are zero, and the postnet
sees each utterance with zero padding past its own end (what a batch of one sees).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

POSTNET_LAYERS = 5


def _count(counter, name, macs):
    if counter is not None:
        counter[name] = counter.get(name, 0) + int(macs)


def _conv_bn(sd, pre, x, dtype, counter, tag, weight_cast=None):
    w = sd[pre + "convolution1d.weight"].to(dtype)
    if weight_cast is not None:  # the bf16 mode's convs: bf16 operands, fp32 accumulation
        w, x = weight_cast(w), weight_cast(x)
    x = F.conv1d(x, w, sd[pre + "convolution1d.bias"].to(dtype), padding=(w.shape[2] - 1) // 2)
    _count(counter, tag, x.shape[0] * x.shape[2] * w.numel())
    bn = pre + "batch_normalization."
    return F.batch_norm(x, sd[bn + "running_mean"].to(dtype), sd[bn + "running_var"].to(dtype),
                        sd[bn + "weight"].to(dtype), sd[bn + "bias"].to(dtype), training=False, eps=1e-5)


def _lstm(sd, pre, E, dtype):
    m = nn.LSTM(E, E // 2, num_layers=1, batch_first=True, bias=True, bidirectional=True)
    m = m.to(device=sd[pre + "weight_ih_l0"].device, dtype=dtype)
    m.load_state_dict({k[len(pre):]: v.to(dtype) for k, v in sd.items() if k.startswith(pre)})
    return m.eval()


def _cell(sd, pre, dtype):
    w_ih, w_hh = sd[pre + "weight_ih"], sd[pre + "weight_hh"]
    m = nn.LSTMCell(w_ih.shape[1], w_hh.shape[1], bias=True).to(device=w_ih.device, dtype=dtype)
    m.load_state_dict({k[len(pre):]: v.to(dtype) for k, v in sd.items() if k.startswith(pre)})
    return m.eval()


def encoder(sd, tokens, x_lengths=None, dtype=torch.float64, counter=None, weight_cast=None):
    """[B, T] token ids -> [B, T, E]."""
    x = F.embedding(tokens, sd["embedding.weight"].to(dtype)).transpose(1, 2)
    for i in range(3):
        x = F.relu(_conv_bn(sd, f"encoder.convolutions.{i}.", x, dtype, counter, "encoder.convs", weight_cast))
    x = x.transpose(1, 2)
    B, T, E = x.shape
    lstm = _lstm(sd, "encoder.lstm.", E, dtype)
    if weight_cast is not None:  # W_ih x runs on the conv path
        x = weight_cast(x)
        with torch.no_grad():
            lstm.weight_ih_l0.copy_(weight_cast(lstm.weight_ih_l0))
            lstm.weight_ih_l0_reverse.copy_(weight_cast(lstm.weight_ih_l0_reverse))
    _count(counter, "encoder.lstm", B * T * 2 * 4 * (E // 2) * (E + E // 2))
    if x_lengths is None:
        return lstm(x)[0]
    packed = pack_padded_sequence(x, x_lengths.cpu(), batch_first=True, enforce_sorted=False)
    out, _ = pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=T)
    return out


def speaker_inputs(sd, enc, speaker_ids=None, d_vectors=None):
    if speaker_ids is not None:
        g = F.embedding(speaker_ids, sd["speaker_embedding.weight"].to(enc.dtype))
    elif d_vectors is not None:
        g = d_vectors.to(enc.dtype)
    else:
        return enc
    return torch.cat([enc, g[:, None, :].expand(-1, enc.shape[1], -1)], dim=-1)


def decoder(sd, inputs, r, C, x_lengths=None, attention_norm="sigmoid", stop_threshold=0.5, max_decoder_steps=10000,
            dtype=torch.float64, counter=None, weight_cast=None):
    """inputs [B, T, D] -> decoder_outputs [B, S r, C], alignments [B, S, T], stop_tokens [B, S], steps [B]
    (S = the largest step count).  ``weight_cast`` (the bf16 mode's analogue) rounds the four big RNN
    matrices here, and the operands of every conv in the encoder and the postnet."""
    inputs = inputs.to(dtype)
    B, T, D = inputs.shape
    p = "decoder."
    W0 = sd[p + "prenet.linear_layers.0.linear_layer.weight"].to(dtype)
    W1 = sd[p + "prenet.linear_layers.1.linear_layer.weight"].to(dtype)
    arnn, drnn = _cell(sd, p + "attention_rnn.", dtype), _cell(sd, p + "decoder_rnn.", dtype)
    if weight_cast is not None:
        with torch.no_grad():
            for m in (arnn, drnn):
                m.weight_ih.copy_(weight_cast(m.weight_ih))
                m.weight_hh.copy_(weight_cast(m.weight_hh))
    Wq = sd[p + "attention.query_layer.linear_layer.weight"].to(dtype)
    Win = sd[p + "attention.inputs_layer.linear_layer.weight"].to(dtype)
    v_w = sd[p + "attention.v.linear_layer.weight"].to(dtype)
    v_b = sd[p + "attention.v.linear_layer.bias"].to(dtype)
    Wl = sd[p + "attention.location_layer.location_conv1d.weight"].to(dtype)
    Wd = sd[p + "attention.location_layer.location_dense.linear_layer.weight"].to(dtype)
    Wp = sd[p + "linear_projection.linear_layer.weight"].to(dtype)
    bp = sd[p + "linear_projection.linear_layer.bias"].to(dtype)
    Ws = sd[p + "stopnet.1.linear_layer.weight"].to(dtype)
    bs = sd[p + "stopnet.1.linear_layer.bias"].to(dtype)
    Q = Wq.shape[1]
    dev = inputs.device
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
    query, c_a, h_d, c_d, context = z(B, Q), z(B, Q), z(B, Q), z(B, Q), z(B, D)
    aw, awc, memory = z(B, T), z(B, T), z(B, C)
    processed = F.linear(inputs, Win)
    _count(counter, "decoder.inputs_layer", B * T * Win.numel())
    mask = None if x_lengths is None else (torch.arange(T, device=dev)[None, :] >= x_lengths.to(dev)[:, None])
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    steps = torch.zeros(B, dtype=torch.int64, device=dev)
    outs, aligns, stops = [], [], []
    per_step = (W0.numel() + W1.numel() + arnn.weight_ih.numel() + arnn.weight_hh.numel() + Wq.numel() +
                T * (Wl.numel() + Wd.numel() + v_w.numel() + D) + drnn.weight_ih.numel() + drnn.weight_hh.numel() +
                Wp.numel() + Ws.numel())
    t = 0
    while True:
        pre = F.relu(F.linear(F.relu(F.linear(memory, W0)), W1))
        query, c_a = arnn(torch.cat([pre, context], -1), (query, c_a))
        loc = F.conv1d(torch.stack([aw, awc], 1), Wl, padding=(Wl.shape[2] - 1) // 2)
        loc = F.linear(loc.transpose(1, 2), Wd)
        e = F.linear(torch.tanh(F.linear(query, Wq)[:, None, :] + loc + processed), v_w, v_b).squeeze(-1)
        if mask is not None:
            e = e.masked_fill(mask, float("-inf"))
        if attention_norm == "softmax":
            a = torch.softmax(e, -1)
        else:
            s = torch.sigmoid(e)
            a = s / s.sum(1, keepdim=True)
        awc = awc + a
        aw = a
        context = torch.bmm(a[:, None, :], inputs).squeeze(1)
        h_d, c_d = drnn(torch.cat([query, context], -1), (h_d, c_d))
        out = F.linear(torch.cat([h_d, context], -1), Wp, bp)
        stop = torch.sigmoid(F.linear(torch.cat([h_d, out], -1), Ws, bs)).squeeze(-1)
        if counter is not None:  # the count reads `done` on the host: not in a timed run
            _count(counter, "decoder.steps", int((~done).sum()) * per_step)
        live = (~done).to(dtype)
        outs.append(out * live[:, None])
        aligns.append(a * live[:, None])
        stops.append(stop * live)
        ends = ~done & (((stop > stop_threshold) & (t >= 1)) | (t + 1 >= max_decoder_steps))
        steps[ends] = t + 1
        done = done | ends
        if bool(done.all()):
            break
        memory = out[:, (r - 1) * C:]
        t += 1
    S = len(outs)
    dec = torch.stack(outs, 1).reshape(B, S * r, C)
    return dec, torch.stack(aligns, 1), torch.stack(stops, 1), steps


def postnet(sd, dec, y_lengths, dtype=torch.float64, counter=None, weight_cast=None):
    """dec [B, L, C] -> dec + postnet(dec) per utterance at its own length; rows past it zero."""
    out = torch.zeros_like(dec)
    for b in range(dec.shape[0]):
        n = int(y_lengths[b])
        x = dec[b : b + 1, :n].transpose(1, 2)
        y = x
        for i in range(POSTNET_LAYERS):
            y = _conv_bn(sd, f"postnet.convolutions.{i}.", y, dtype, counter, "postnet", weight_cast)
            if i < POSTNET_LAYERS - 1:
                y = torch.tanh(y)
        out[b, :n] = (x + y).transpose(1, 2)[0]
    return out


def inference(sd, args, tokens, x_lengths=None, speaker_ids=None, d_vectors=None, stop_threshold=None,
              max_decoder_steps=None, dtype=torch.float64, counter=None, weight_cast=None):
    a = args if isinstance(args, dict) else vars(args)
    with torch.no_grad():
        enc = encoder(sd, tokens, x_lengths, dtype, counter, weight_cast)
        inputs = speaker_inputs(sd, enc, speaker_ids, d_vectors)
        dec, align, stop, steps = decoder(
            sd, inputs, a["r"], a["out_channels"], x_lengths, a.get("attention_norm", "sigmoid"),
            a.get("stop_threshold", 0.5) if stop_threshold is None else stop_threshold,
            a.get("max_decoder_steps", 10000) if max_decoder_steps is None else max_decoder_steps, dtype, counter,
            weight_cast)
        y_len = steps * a["r"]
        return {"inputs": inputs, "decoder_outputs": dec, "model_outputs": postnet(sd, dec, y_len, dtype, counter, weight_cast),
                "alignments": align, "stop_tokens": stop, "y_lengths": y_len}
