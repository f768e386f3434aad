#!/usr/bin/env python
"""Time the XTTS GPT step loop on the device (the numbers of DESIGN.md's XTTS GPT section): the reference
widths (30 layers, E = 1024, 16 heads, 1026 audio tokens, P = 32 conditioning rows, 64 text tokens), stop
disabled (mel_head's stop-row bias at -1e4), greedy, ``--steps`` = 256 steps, at B = 1 and B = 8, in the
fp32-faithful mode and in bf16.  A host clock around windows of ``--calls`` whole calls (prefill + generate)
that end in a device synchronise, warm; per call: median, minimum and maximum over ``--reps`` windows.  The time
per step is the slope between runs of ``--steps`` and ``--steps`` / 2 steps, so the prefill cancels; it is
reported from the medians, with the range the windows' extremes allow.  Each step is set against
  - the weight-stream floor: the bytes of the layers' matrices and mel_head, read once per step, at the
    6.3 TB/s the HBM sustains (1.5 GB in fp32: far beyond the 256 MiB Infinity Cache, so they stream
    from HBM every step);
  - the KV-cache bytes a step reads (averaged over the steps the slope spans);
  - the slope of torch on the same device and inputs in fp32 eager with a KV cache, in the same
    process (tests/_xtts_gpt_ref.py ``EagerGpt``).
Also prints the per-launch table of ``tts_xtts_gpt_generate_profiled``.  One JSON line per measurement."""
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

import _xtts_gpt_cases as C  # noqa: E402
import _xtts_gpt_ref as R  # noqa: E402
from tts_amd.tts import XttsGPT  # noqa: E402

HBM_TB_S = 6.3


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
    return {"us_per_step": 1e3 * (full[0] - half[0]) / dsteps,
            "us_per_step_min": 1e3 * (full[1] - half[2]) / dsteps, "us_per_step_max": 1e3 * (full[2] - half[1]) / dsteps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S, T = args.steps, args.tokens
    cfg = dict(layers=args.layers, model_dim=1024, heads=16, n_text=256, n_audio=1026, start_text=255, stop_text=0,
               start_audio=1024, stop_audio=1025, text_positions=T + 2, mel_positions=608, P=32)
    E, L = cfg["model_dim"], cfg["layers"]
    sd = C.state_dict(cfg, seed=5)
    sd["mel_head.bias"][cfg["stop_audio"]] = -1e4  # stop disabled
    matrix_elems = L * 12 * E * E + cfg["n_audio"] * E
    prefix = cfg["P"] + T + 2
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "layers": L, "model_dim": E,
                      "heads": 16, "text_tokens": T, "prefix_rows": prefix, "steps": S, "reps": args.reps,
                      "calls_per_window": args.calls, "warmup": args.warmup, "chunk": args.chunk}), flush=True)
    eager = None if args.no_torch else R.EagerGpt(sd, cfg, dev)
    for B in (int(b) for b in args.batches.split(",")):
        cond, text = C.inputs(cfg, 3, B, T)
        cond, text = cond.to(dev), text.to(dev)
        # keys and values a step reads, averaged over the steps [S / 2, S)
        kv_mb = L * 2 * B * (prefix + 0.75 * S) * E * 4 / 1e6
        ref = None
        if eager is not None:
            ref = eager.generate(cond, text, S)
            full = median_ms(lambda: eager.generate(cond, text, S), args.reps, args.warmup, args.calls)
            half = median_ms(lambda: eager.generate(cond, text, S // 2), args.reps, args.warmup, args.calls)
            print(json.dumps({"op": "torch-ROCm fp32 eager with a KV cache (oracle restatement)", "batch": B,
                              "median_ms": full[0], "min_ms": full[1], "max_ms": full[2],
                              **slope_us(full, half, S - S // 2)}), flush=True)
        for mode in args.modes.split(","):
            m = XttsGPT(**C.ctor_kwargs(cfg), math_mode=mode, chunk=args.chunk)
            m.load_state_dict(sd)
            m = m.eval().to(dev)
            kw = dict(do_sample=False, repetition_penalty=1.0)
            out = m._generate(cond, text, max_new_tokens=S, **kw)
            assert int(out["lengths"].min()) == S, "the stop token was drawn"
            full = median_ms(lambda: m._generate(cond, text, max_new_tokens=S, **kw), args.reps, args.warmup, args.calls)
            half = median_ms(lambda: m._generate(cond, text, max_new_tokens=S // 2, **kw), args.reps, args.warmup,
                             args.calls)
            sl = slope_us(full, half, S - S // 2)
            us = max(sl["us_per_step"], 1e-9)
            wmb = matrix_elems * (2 if mode == "bf16" else 4) / 1e6
            row = {"op": "XttsGPT generate (prefill + steps)", "mode": mode, "batch": B, "median_ms": full[0],
                   "min_ms": full[1], "max_ms": full[2], **sl, "matrix_mb_per_step": wmb,
                   "weight_stream_floor_us": wmb / HBM_TB_S, "matrix_tb_per_s": wmb / us,
                   "kv_mb_per_step": kv_mb, "kv_floor_us": kv_mb / HBM_TB_S}
            if ref is not None:
                row["codes_equal_to_torch_fp32"] = float((out["codes"].to(torch.int64) == ref).float().mean())
            print(json.dumps(row), flush=True)
            recs = m._generate(cond, text, max_new_tokens=S, profile=True, **kw)["profile"]
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
            print(json.dumps({"op": "tts_xtts_gpt_{prefill,generate}_profiled", "mode": mode, "batch": B,
                              "launches": agg}), flush=True)
            del m


if __name__ == "__main__":
    main()
