#!/usr/bin/env python
"""Time the ResNet speaker encoder on the device (the numbers of DESIGN.md's speaker-encoder section):
the reference widths (input_dim 64, layers [3, 4, 6, 3], filters [32, 64, 128, 256], ASP, the XTTS
front end) on ``compute_embedding``'s default shape (10 windows x 40,000 samples of a 3 s clip) and on
B = 16 clips of 6 s through ``forward``, in the fp32-faithful mode and in bf16.  A host clock around
windows of ``--calls`` whole calls that end in a device synchronise, warm; per call: median, minimum
and maximum over ``--reps`` windows.  The comparison point is torch on the same device and inputs in
fp32 eager, in the same process: the oracle restatement (tests/_speaker_encoder_ref.py: ``F.conv2d``,
``F.batch_norm``, ``torch.stft``, ``F.instance_norm``).  Also prints the per-launch table of
``tts_speaker_encoder_forward_profiled`` and, per 3x3 conv shape, the achieved MFMA rate against
the mode's ceiling (``--peak-tflops`` dense bf16, divided by the 6 bf16 products per MAC of fp32x6).
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tts-3_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import _speaker_encoder_ref as R  # noqa: E402
from tts_amd import synthetic  # noqa: E402
from tts_amd.encoder import XTTS_AUDIO_CONFIG, ResNetSpeakerEncoder  # noqa: E402

CFG = dict(input_dim=64, proj_dim=512, layers=[3, 4, 6, 3], num_filters=[32, 64, 128, 256], encoder_type="ASP",
           log_input=True, use_torch_spec=True, audio_config=XTTS_AUDIO_CONFIG)


def median_ms(fn, reps, warm, calls):
    """ms per call over ``reps`` windows of ``calls`` calls: (median, min, max)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / calls)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fp32x6,bf16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tflops", type=float, default=2500.0, help="dense bf16 MFMA peak of the device")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = synthetic.speaker_encoder_state_dict(use_torch_spec=True, audio_config=XTTS_AUDIO_CONFIG, seed=7)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    kw = dict(layers=CFG["layers"], encoder_type="ASP", log_input=True, use_torch_spec=True, audio_config=XTTS_AUDIO_CONFIG)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": args.reps,
                      "calls_per_window": args.calls, "warmup": args.warmup}), flush=True)
    clip = synthetic.speaker_wav(1, 48000, seed=1).to(dev)
    batch = synthetic.speaker_wav(16, 96000, seed=2).to(dev)
    shapes = {"compute_embedding 10 x 40000": ("ce", clip), "forward B=16 x 6 s": ("fw", batch)}
    for label, (kind, x) in shapes.items():
        ref = None
        if not args.no_torch:
            if kind == "ce":
                run = lambda: R.compute_embedding(sdd, x, hop_length=160, dtype=torch.float32, **kw)  # noqa: E731
            else:
                run = lambda: R.forward(sdd, x, l2_norm=True, dtype=torch.float32, **kw)  # noqa: E731
            ref = run()
            med, lo, hi = median_ms(run, args.reps, args.warmup, args.calls)
            print(json.dumps({"op": "torch-ROCm fp32 eager (oracle restatement)", "shape": label, "median_ms": med,
                              "min_ms": lo, "max_ms": hi}), flush=True)
        for mode in args.modes.split(","):
            m = ResNetSpeakerEncoder(**CFG, math_mode=mode)
            m.load_state_dict(sd)
            m = m.eval().to(dev)
            run = (lambda: m.compute_embedding(x)) if kind == "ce" else (lambda: m(x, l2_norm=True))
            out = run()
            med, lo, hi = median_ms(run, args.reps, args.warmup, args.calls)
            row = {"op": "ResNetSpeakerEncoder", "shape": label, "mode": mode, "median_ms": med, "min_ms": lo, "max_ms": hi}
            if ref is not None:
                row["max_abs_vs_torch_fp32"] = float((out - ref).abs().max())
            print(json.dumps(row), flush=True)
            if kind == "ce":
                from tts_amd.encoder import window_offsets

                xb = torch.cat([x[:, a:b] for a, b in window_offsets(x.shape[1], 40000, 10)], dim=0)
            else:
                xb = x
            m.profile(xb, l2_norm=True)  # warm
            _, recs = m.profile(xb, l2_norm=True)
            agg = {}
            for r in recs:
                a = agg.setdefault(r["name"], {"launches": 0, "ms": 0.0, "flops": 0.0})
                a["launches"] += 1
                a["ms"] += r["ms"]
                a["flops"] += r["flops"]
            ceiling = args.peak_tflops / (1.0 if mode == "bf16" else 6.0)
            for name, a in agg.items():
                a["us_per_launch"] = 1e3 * a["ms"] / a["launches"]
                a["tflops"] = a["flops"] / max(a["ms"], 1e-9) / 1e9
                if name.startswith("conv") or name.startswith("stem"):
                    a["mfma_utilisation"] = a["tflops"] / ceiling
                del a["flops"]
            print(json.dumps({"op": "tts_speaker_encoder_forward_profiled", "shape": label, "mode": mode,
                              "total_ms": sum(r["ms"] for r in recs), "launches": agg}), flush=True)
            del m


if __name__ == "__main__":
    main()
