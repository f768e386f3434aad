#!/usr/bin/env python
"""Time the MelGAN-family vocoders on the device (the numbers of DESIGN.md's MelGAN section): the
multi-band zoo configuration (``inference``: PQMF synthesis included) and the full-band one at
32 x 1024 mel frames, in the fp32-faithful mode and in bf16; hipEvent pairs around single calls, warm,
median of ``--reps``.  The comparison point is the oracle restatement (tests/_melgan_ref.py,
``torch.nn.functional`` ops as the reference writes them) run by torch on the same device and input in
fp32.  Also prints the per-launch table of ``tts_melgan_forward_profiled``.  One JSON line per
measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tts-3_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import _melgan_ref as R  # noqa: E402
from tts_amd import synthetic, vocoder  # noqa: E402
from tts_amd.config import FULLBAND_MELGAN, MULTIBAND_MELGAN  # noqa: E402

CONFIGS = {
    "multiband": (vocoder.MultibandMelganGenerator, dict(in_channels=80, out_channels=4, base_channels=384, **MULTIBAND_MELGAN), True),
    "fullband": (vocoder.FullbandMelganGenerator, dict(in_channels=80, out_channels=1, base_channels=512, **FULLBAND_MELGAN), False),
}


def median_ms(fn, reps, warm):
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
    ap.add_argument("--configs", default="multiband,fullband")
    ap.add_argument("--modes", default="fp32x6,bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ROCm comparison point")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batch": args.batch,
                      "frames": args.frames, "reps": args.reps, "warmup": args.warmup}), flush=True)
    B, T = args.batch, args.frames
    mel = synthetic.mel(B, T, seed=3).to(dev)
    for name in args.configs.split(","):
        cls, ctor, pqmf = CONFIGS[name]
        sd = synthetic.melgan_state_dict(**ctor, pqmf=pqmf, seed=26)
        rcfg = dict(upsample_factors=ctor["upsample_factors"], num_res_blocks=ctor["num_res_blocks"])
        counter = {}
        with torch.no_grad():
            R.melgan_layers(sd, synthetic.mel(1, 16, seed=0), counter=counter, dtype=torch.float32, **rcfg)
        macs_per_frame = sum(counter.values()) / 16
        flops = 2.0 * macs_per_frame * B * (T + 4)
        ref = None
        if not args.no_torch:
            sdd = {k: v.to(dev) for k, v in sd.items()}
            with torch.no_grad():
                run = lambda: R.melgan_forward(sdd, mel, pad=2, synth=pqmf, dtype=torch.float32, **rcfg)  # noqa: E731
                ref = run()
                med, lo, hi = median_ms(run, args.reps, args.warmup)
            print(json.dumps({"op": "torch-ROCm fp32 (oracle restatement)", "config": name, "median_ms": med, "min_ms": lo,
                              "max_ms": hi, "tflops": flops / (med * 1e-3) / 1e12}), flush=True)
        for mode in args.modes.split(","):
            g = cls(**ctor, math_mode=mode)
            g.load_state_dict(sd)
            g.eval()
            g.remove_weight_norm()
            g = g.to(dev)
            out = g.inference(mel)
            med, lo, hi = median_ms(lambda: g.inference(mel), args.reps, args.warmup)
            row = {"op": "inference", "config": name, "mode": mode, "median_ms": med, "min_ms": lo, "max_ms": hi,
                   "mflop_per_frame": 2e-6 * macs_per_frame, "tflops": flops / (med * 1e-3) / 1e12,
                   "audio_seconds_per_second": B * out.shape[-1] / 22050 / (med * 1e-3)}
            if ref is not None:
                row["max_abs_vs_torch_fp32"] = float((out - ref).abs().max())
            print(json.dumps(row), flush=True)
            _, recs = g.profile(mel, synth=1 if pqmf else 0)
            agg = {}
            for r in recs:
                a = agg.setdefault(r["name"], {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
                a["launches"] += 1
                a["ms"] += r["ms"]
                a["flops"] += r["flops"]
                a["bytes"] += r["bytes"]
            for k, a in agg.items():
                a["tflops"] = a["flops"] / max(a["ms"], 1e-9) / 1e9
                a["gb_per_s"] = a["bytes"] / max(a["ms"], 1e-9) / 1e6
            print(json.dumps({"op": "tts_melgan_forward_profiled", "config": name, "mode": mode, "launches": agg}), flush=True)
            del g


if __name__ == "__main__":
    main()
