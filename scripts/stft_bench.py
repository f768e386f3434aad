#!/usr/bin/env python
"""Time ``tts_amd.tts.wav_to_spec`` on the device (the numbers of DESIGN.md's linear-spectrogram section):
hipEvent pairs around single calls, warm, median of 20, per (shape, math mode); one
``tts_stft_forward_profiled`` record per mode; ``torch.stft`` (wav_to_spec as the reference writes it) on
the same device and input as the comparison point.  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tts-3_amd"))

from tts_amd.tts import wav_to_spec, wav_to_spec_profile  # noqa: E402

N_FFT, HOP, WIN = 1024, 256, 1024


def torch_spec(y):
    p = (N_FFT - HOP) // 2
    yp = F.pad(y.unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    s = torch.stft(yp, N_FFT, hop_length=HOP, win_length=WIN, window=torch.hann_window(WIN, device=y.device),
                   center=False, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    return torch.sqrt(torch.view_as_real(s).pow(2).sum(-1) + 1e-6)


def median_ms(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f16x3,bf16,fp32x6")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.stft comparison point")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    shapes = [(1, 22050 * 10), (32, 256 * 1024)]
    for B, N in shapes:
        y = 0.3 * torch.randn(B, N, generator=torch.Generator().manual_seed(1)).to(dev)
        T = 1 + (N + 2 * ((N_FFT - HOP) // 2) - N_FFT) // HOP
        flops = 2.0 * 2 * (N_FFT // 2 + 1) * N_FFT * T * B
        ref = None
        if not args.no_torch:
            ref = torch_spec(y)
            med, lo, hi = median_ms(lambda: torch_spec(y))
            print(json.dumps({"op": "torch.stft wav_to_spec", "B": B, "N": N, "T": T, "median_ms": med, "min_ms": lo,
                              "max_ms": hi}), flush=True)
        for mode in args.modes.split(","):
            out = wav_to_spec(y, N_FFT, HOP, WIN, math_mode=mode)
            med, lo, hi = median_ms(lambda: wav_to_spec(y, N_FFT, HOP, WIN, math_mode=mode))
            row = {"op": "wav_to_spec", "mode": mode, "B": B, "N": N, "T": T, "median_ms": med, "min_ms": lo,
                   "max_ms": hi, "gemm_tflops": flops / (med * 1e-3) / 1e12}
            if ref is not None:
                row["max_abs_vs_torch_fp32"] = float((out - ref).abs().max())
            print(json.dumps(row), flush=True)
            _, recs = wav_to_spec_profile(y, N_FFT, HOP, WIN, math_mode=mode)
            print(json.dumps({"op": "tts_stft_forward_profiled", "mode": mode, "B": B, "N": N, "records": recs}),
                  flush=True)


if __name__ == "__main__":
    main()
