#!/usr/bin/env python
"""Time Tacotron2 on the device (the numbers of DESIGN.md's Tacotron2 section): the reference widths
(E = 512, Q = 1024, P = 256, A = 128, F = 32, C = 80), r = 2, T_en = 128, stop disabled, 400 decoder steps,
at B = 1 and B = 16, ``inference`` in the fp32-faithful mode and in bf16.  A host clock around windows of
``--calls`` whole calls that end in a device synchronise (the decoder synchronises once per chunk
itself), warm; per call: median, minimum and maximum over ``--reps`` windows.  The time per decoder step is
the slope between runs of ``--steps`` and ``--steps`` / 2 steps, so the encoder and the postnet cancel; it is
reported from the medians, with the range the windows' extremes allow.  The comparison point is torch
on the same device and inputs in fp32 eager, in the same process: the oracle restatement
(tests/_tacotron2_ref.py: ``nn.LSTM``, ``nn.LSTMCell``, ``F.conv1d``, ``F.linear``), which like the reference
reads the stop flag on the host every step; a call of it also rebuilds its ``nn.LSTM`` / ``nn.LSTMCell``
modules from the state dict, which the slope cancels and the whole-call figure includes.  Also prints the
per-launch table of ``tts_tacotron2_decode_profiled``.  One JSON line per measurement."""
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

import _tacotron2_ref as R  # noqa: E402
from tts_amd import synthetic  # noqa: E402
from tts_amd.config import TACOTRON2  # noqa: E402
from tts_amd.tts import Tacotron2  # noqa: E402


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


def slope_us(full, half, dsteps):
    """µs per step from (median, min, max) of the long and the short run: the medians' slope and its range."""
    return {"us_per_step": 1e3 * (full[0] - half[0]) / dsteps,
            "us_per_step_min": 1e3 * (full[1] - half[2]) / dsteps, "us_per_step_max": 1e3 * (full[2] - half[1]) / dsteps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0, help="calls per timed window (0: 10 for the library, 2 for torch)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = dict(TACOTRON2, num_chars=60, r=2)
    sd = synthetic.tacotron2_state_dict(cfg, seed=34)
    S = args.steps
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tokens": args.tokens,
                      "steps": S, "r": cfg["r"], "reps": args.reps, "calls_per_window": args.calls or "10 / 2 (torch)", "warmup": args.warmup,
                      "chunk": args.chunk}),
          flush=True)
    weights_mb = {m: sum(sd[f"decoder.{n}.weight_{k}"].numel() for n in ("attention_rnn", "decoder_rnn")
                         for k in ("ih", "hh")) * (2 if m == "bf16" else 4) / 1e6 for m in ("fp32", "bf16")}
    sdd = {k: v.to(dev) for k, v in sd.items()}
    for B in (int(b) for b in args.batches.split(",")):
        tok = (1 + synthetic.tokens(B, args.tokens, cfg["num_chars"] - 1, seed=3)).to(dev)
        ref = None
        if not args.no_torch:
            run = lambda n: R.inference(sdd, cfg, tok, stop_threshold=2.0, max_decoder_steps=n,  # noqa: E731
                                        dtype=torch.float32)
            ref = run(S)["model_outputs"]
            full = median_ms(lambda: run(S), args.reps, args.warmup, args.calls or 2)
            half = median_ms(lambda: run(S // 2), args.reps, args.warmup, args.calls or 2)
            print(json.dumps({"op": "torch-ROCm fp32 eager (oracle restatement)", "batch": B, "median_ms": full[0],
                              "min_ms": full[1], "max_ms": full[2], **slope_us(full, half, S - S // 2)}), flush=True)
        for mode in args.modes.split(","):
            m = Tacotron2(cfg, math_mode=mode, chunk=args.chunk)
            m.load_state_dict(sd)
            m = m.eval().to(dev)
            m.stop_threshold = 2.0

            def run(n):
                m.max_decoder_steps = n
                return m.inference(tok)

            out = run(S)["model_outputs"]
            full = median_ms(lambda: run(S), args.reps, args.warmup, args.calls or 10)
            half = median_ms(lambda: run(S // 2), args.reps, args.warmup, args.calls or 10)
            sl = slope_us(full, half, S - S // 2)
            us = sl["us_per_step"]
            row = {"op": "Tacotron2.inference", "mode": mode, "batch": B, "median_ms": full[0], "min_ms": full[1],
                   "max_ms": full[2], **sl, "rnn_weight_mb_per_step": weights_mb[mode],
                   "rnn_weight_tb_per_s": weights_mb[mode] * 1e6 / (max(us, 1e-9) * 1e-6) / 1e12}
            if ref is not None:
                row["max_abs_vs_torch_fp32"] = float((out - ref).abs().max())
            print(json.dumps(row), flush=True)
            m.max_decoder_steps = S
            _, recs = m.profile(tok)
            agg = {}
            for r in recs:
                a = agg.setdefault(r["name"], {"launches": 0, "ms": 0.0, "bytes": 0.0})
                a["launches"] += 1
                a["ms"] += r["ms"]
                a["bytes"] += r["bytes"]
            for a in agg.values():
                a["us_per_launch"] = 1e3 * a["ms"] / a["launches"]
                a["gb_per_s"] = a["bytes"] / max(a["ms"], 1e-9) / 1e6
                del a["bytes"]
            print(json.dumps({"op": "tts_tacotron2_decode_profiled", "mode": mode, "batch": B, "launches": agg}),
                  flush=True)
            del m


if __name__ == "__main__":
    main()
