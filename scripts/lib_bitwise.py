"""Outputs of every executor of the library named by TTS_MI355X_LIB (or the in-tree one) for fixed
seeded inputs, one entry per executor and math mode, saved to an .npz: run once per library, then
compare the files (host-side refactors and variant A/Bs that must be bitwise equal to another build).
Where the Python class has a ``profile`` call, the launch-record names are saved as ``<entry>/launches``.
Run it twice on the same library to see which entries that library itself reproduces.
usage: python scripts/lib_bitwise.py OUT.npz [compare.npz]   (exit status 1 when an entry differs)"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tts-3_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))  # the shared ForwardTTS / MelGAN test cases
import _forward_tts_cases as FC  # noqa: E402
import _melgan_cases as MC  # noqa: E402
from tts_amd import synthetic, vocoder  # noqa: E402
from tts_amd.config import GLOW_TTS_ENCODER, HIFIGAN_V1, VITS_FLOW, VITS_POSTERIOR, VITS_SDP, VITS_TEXT_ENCODER  # noqa: E402
from tts_amd.tts import (Decoder, DurationPredictor, Encoder, ForwardTTS, PosteriorEncoder,  # noqa: E402
                         ResidualCouplingBlocks, StochasticDurationPredictor, TextEncoder, wav_to_spec,
                         wav_to_spec_profile)

dev = torch.device("cuda", 0)
ALL = ("fp32", "fp32x6", "f16x3", "bf16")
TEXT = ("fp32", "fp32x6", "bf16")  # the text side has no f16x3 statistics
outs = {}


def save(key, out, rows=None):
    for i, o in enumerate(out if isinstance(out, (tuple, list)) else [out]):
        if o is not None:  # e.g. x_logs of a mean-only encoder
            outs[f"{key}/{i}"] = o.cpu().numpy()
    if rows is not None:
        outs[f"{key}/launches"] = np.array([r["name"] for r in rows])


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def mask(lengths, T):
    return (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).float().unsqueeze(1)


# HiFiGAN v1, 4 x 150 frames
cfg = dict(in_channels=80, out_channels=1, **HIFIGAN_V1)
sd = synthetic.hifigan_state_dict(**cfg, seed=1234, weight_norm=True)
mel = synthetic.mel(4, 150, seed=3).to(dev)
for mode in ALL:
    g = vocoder.HifiganGenerator(**cfg, math_mode=mode)
    g.load_state_dict(sd)
    g.eval()
    g.remove_weight_norm()
    g = g.to(dev)
    save(f"hifigan/{mode}", g.inference(mel), g.profile(mel)[1])

# Glow decoder: the smoke configuration, 2 x 40 frames, the second utterance cut at 31
cfg = dict(in_channels=80, hidden_channels=192, kernel_size=5, dilation_rate=1, num_flow_blocks=12,
           num_coupling_layers=4, num_splits=4, num_squeeze=2)
sd = synthetic.glow_decoder_state_dict(**cfg, seed=1)
x, m = randn(2, 80, 40, seed=0).to(dev), mask([40, 31], 40).to(dev)
for mode in ALL:
    d = Decoder(**cfg, math_mode=mode)
    d.load_state_dict(sd)
    d.eval()
    d.store_inverse()
    d = d.to(dev)
    save(f"glow_decoder/{mode}", d(x, m, reverse=True)[0], d.profile(x, m)[1])

# VITS flow, both directions (test_vits_gpu.py's other-shapes case with a speaker vector)
cfg = dict(VITS_FLOW, channels=64, hidden_channels=96, num_layers=3, num_flows=3, dilation_rate=2, cond_channels=4)
sd = synthetic.vits_flow_state_dict(**cfg, seed=15)
x, m, gv = randn(3, 64, 77, seed=5).to(dev), mask([77, 40, 3], 77).to(dev), randn(3, 4, 1, seed=6).to(dev)
for mode in ALL:
    f = ResidualCouplingBlocks(cfg["channels"], cfg["hidden_channels"], cfg["kernel_size"], cfg["dilation_rate"],
                               cfg["num_layers"], num_flows=cfg["num_flows"], cond_channels=4, math_mode=mode)
    f.load_state_dict(sd)
    f = f.to(dev)
    for rev in (True, False):
        save(f"vits_flow_{'reverse' if rev else 'forward'}/{mode}", f(x, m, g=gv, reverse=rev),
             f.profile(x, m, g=gv, reverse=rev)[1])

# posterior encoder with a stored eps
cfg = dict(VITS_POSTERIOR, in_channels=80, out_channels=32, hidden_channels=64, num_layers=3)
sd = synthetic.vits_posterior_state_dict(**cfg, seed=7)
x, lens, eps = randn(2, 80, 50, seed=8).abs().to(dev), torch.tensor([50, 23]).to(dev), randn(2, 32, 50, seed=9).to(dev)
for mode in ALL:
    pe = PosteriorEncoder(**cfg, math_mode=mode)
    pe.load_state_dict(sd)
    pe = pe.to(dev)
    save(f"vits_posterior/{mode}", pe(x, lens, noise=eps)[:3], pe.profile(x, lens, noise=eps)[1])

# Glow encoder (rel_pos_transformer, two layers), VITS text encoder, SDP with stored noise, DP
tok, lens = synthetic.tokens(3, 37, 40, seed=2).to(dev), torch.tensor([37, 20, 1]).to(dev)
cfg = dict(GLOW_TTS_ENCODER, num_chars=40, encoder_params=dict(GLOW_TTS_ENCODER["encoder_params"], num_layers=2,
                                                               rel_attn_window_size=4))
sd = synthetic.glow_encoder_state_dict(**cfg, seed=3)
for mode in TEXT:
    e = Encoder(40, cfg["out_channels"], cfg["hidden_channels"], cfg["hidden_channels_dp"], "rel_pos_transformer",
                cfg["encoder_params"], mean_only=cfg["mean_only"], use_prenet=cfg["use_prenet"], math_mode=mode)
    e.load_state_dict(sd)
    e.eval()
    e = e.to(dev)
    save(f"glow_encoder/{mode}", e(tok, lens), e.profile(tok, lens)[1])

cfg = dict(VITS_TEXT_ENCODER, num_layers=2)
sd = synthetic.vits_text_encoder_state_dict(num_chars=40, **cfg, seed=4)
for mode in TEXT:
    te = TextEncoder(40, cfg["out_channels"], cfg["hidden_channels"], cfg["hidden_channels_ffn"], cfg["num_heads"],
                     cfg["num_layers"], cfg["kernel_size"], 0.1, math_mode=mode)
    te.load_state_dict(sd)
    te = te.to(dev)
    save(f"vits_text_encoder/{mode}", te(tok, lens), te.profile(tok, lens)[1])

xm = mask([37, 20, 1], 37)
x, noise = (randn(3, 192, 37, seed=17) * xm).to(dev), randn(3, 2, 37, seed=18).to(dev)
xm = xm.to(dev)
sd = synthetic.vits_sdp_state_dict(**VITS_SDP, seed=31)
for mode in TEXT:
    sdp = StochasticDurationPredictor(192, 192, 3, 0.5, 4, math_mode=mode)
    sdp.load_state_dict(sd)
    sdp = sdp.to(dev)
    save(f"vits_sdp/{mode}", sdp(x, xm, reverse=True, noise_scale=1.0, noise=noise),
         sdp.profile(x, xm, noise_scale=1.0, noise=noise)[1])
sd = synthetic.vits_dp_state_dict(192, 256, 3, seed=32)
for mode in TEXT:
    dp = DurationPredictor(192, 256, 3, 0.5, math_mode=mode)
    dp.load_state_dict(sd)
    dp = dp.to(dev)
    save(f"vits_dp/{mode}", dp(x, xm), dp.profile(x, xm)[1])

# ForwardTTS inference with given durations (the small case: 3 x 13 tokens, lengths 13, 9, 1)
kw = FC.variant_kwargs("small", "durations")
aux = {"speaker_ids": kw["speaker_ids"], "x_lengths": kw["x_lengths"], "durations": kw["durations"]}
for mode in ("fp32x6", "bf16"):
    ft = ForwardTTS(FC.ARGS["small"], math_mode=mode)
    ft.load_state_dict(FC.state_dict("small"))
    ft.eval()
    ft = ft.to(dev)
    o = ft.inference(FC.tokens("small").to(dev), aux)
    save(f"forward_tts/{mode}", [o["model_outputs"], o["alignments"], o["pitch"], o["durations_log"]],
         ft.profile(FC.tokens("small").to(dev), aux)[1])

# multi-band MelGAN inference (PQMF synthesis included), the first whole-generator case
config, B, T = MC.CASES[0]
cls, ctor, _ = MC.CONFIGS[config]
mel = MC.mel(B, T).to(dev)
for mode in ("fp32x6", "bf16"):
    g = getattr(vocoder, cls)(**ctor, math_mode=mode)
    g.load_state_dict(MC.state_dict(config))
    g.eval()
    g = g.to(dev)
    save(f"melgan_{config}/{mode}", g.inference(mel), g.profile(mel, synth=1)[1])

# linear spectrogram, 3 rows of 128 * 9 + 5 samples at n_fft 512
y = randn(3, 128 * 9 + 5, seed=9).to(dev)
for mode in ("fp32x6", "f16x3", "bf16"):
    save(f"wav_to_spec/{mode}", wav_to_spec(y, 512, 128, 512, math_mode=mode),
         wav_to_spec_profile(y, 512, 128, 512, math_mode=mode)[1])

np.savez(sys.argv[1], **outs)
print(f"{len(outs)} arrays saved to {sys.argv[1]}")
if len(sys.argv) > 2:
    ref = np.load(sys.argv[2])
    differs = [k for k, v in outs.items() if k not in ref or not np.array_equal(v, ref[k], equal_nan=v.dtype.kind == "f")]
    for k in outs:
        print(k, "DIFFERS" if k in differs else "bitwise equal")
    print(f"{len(outs) - len(differs)} of {len(outs)} entries bitwise equal to {sys.argv[2]}; differing: {differs}")
    sys.exit(1 if differs else 0)
