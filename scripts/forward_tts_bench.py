#!/usr/bin/env python
"""Time ForwardTTS (FastPitch) on the device (the numbers of DESIGN.md's ForwardTTS section): the
FastPitch defaults (6 + 6 layers, one head of 384) at 16 utterances x 128 tokens with given durations
of 7 (896 frames), ``inference`` in the fp32-faithful mode and in bf16, and the attention op alone at
[16, 1 head, 896, 384]; hipEvent pairs around single calls, warm, median of ``--reps``.  The comparison
points run by torch on the same device and inputs in fp32, in the same process: the oracle restatement
(tests/_forward_tts_ref.py) for the model, ``F.scaled_dot_product_attention`` for the op.  Also prints
the per-launch table of the ``_profiled`` entry points.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tts-3_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import _forward_tts_ref as R  # noqa: E402
from tts_amd import synthetic  # noqa: E402
from tts_amd.config import FAST_PITCH  # noqa: E402
from tts_amd.tts import ForwardTTS, multi_head_attention  # noqa: E402


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


def bench_op(args, dev):
    B, H, E, T = args.batch, 1, 384, args.tokens * args.duration
    qkv = torch.randn(B, 3 * E, T, generator=torch.Generator().manual_seed(0)).to(dev)
    flops = 2.0 * R.mha_macs(B, E, T)

    def heads_first(t):  # [B][E][T] -> [B][heads][T][dk]
        return t.reshape(B, H, E // H, T).transpose(2, 3).contiguous()

    with torch.no_grad():
        def sdpa():
            q, k, v = (heads_first(t) for t in qkv.split(E, 1))
            return F.scaled_dot_product_attention(q, k, v).transpose(2, 3).reshape(B, E, T)

        ref = sdpa()
        med, lo, hi = median_ms(sdpa, args.reps, args.warmup)
        print(json.dumps({"op": "torch-ROCm fp32 scaled_dot_product_attention, from and to [B][E][T]", "median_ms": med,
                          "min_ms": lo, "max_ms": hi, "tflops": flops / (med * 1e-3) / 1e12}), flush=True)
        q, k, v = (heads_first(t) for t in qkv.split(E, 1))
        med, lo, hi = median_ms(lambda: F.scaled_dot_product_attention(q, k, v), args.reps, args.warmup)
        print(json.dumps({"op": "torch-ROCm fp32 scaled_dot_product_attention alone", "median_ms": med, "min_ms": lo,
                          "max_ms": hi, "tflops": flops / (med * 1e-3) / 1e12}), flush=True)
    for mode in args.modes.split(","):
        out = multi_head_attention(qkv, H, math_mode=mode)
        med, lo, hi = median_ms(lambda: multi_head_attention(qkv, H, math_mode=mode), args.reps, args.warmup)
        print(json.dumps({"op": "tts_op_mha", "shape": [B, H, T, E], "mode": mode, "median_ms": med, "min_ms": lo,
                          "max_ms": hi, "tflops": flops / (med * 1e-3) / 1e12,
                          "max_abs_vs_torch_fp32": float((out - ref).abs().max())}), flush=True)


def bench_model(args, dev):
    cfg = dict(FAST_PITCH, num_chars=60)
    sd = synthetic.forward_tts_state_dict(cfg, seed=12)
    B, T = args.batch, args.tokens
    tok = synthetic.tokens(B, T, cfg["num_chars"], seed=3)
    dur = torch.full((B, T), args.duration)
    frames = B * T * args.duration
    counter = {}
    with torch.no_grad():
        R.inference(sd, cfg, tok[:1, :8], durations=dur[:1, :8], dtype=torch.float32, counter=counter)
    # the attention's MACs grow with the sequence: counted at 8 tokens, restated at the run's lengths
    attn = {k: v for k, v in counter.items() if k.endswith(".attn")}
    fixed = sum(v for k, v in counter.items() if k.startswith("decoder") and k not in attn) / (8 * args.duration)
    dec_macs_per_frame = fixed + cfg["decoder_params"]["num_layers"] * 2 * cfg["hidden_channels"] * T * args.duration
    flops = 2.0 * dec_macs_per_frame * frames
    sdd = {k: v.to(dev) for k, v in sd.items()}
    tokd, durd = tok.to(dev), dur.to(dev)
    with torch.no_grad():
        run = lambda: R.inference(sdd, cfg, tokd, durations=durd, dtype=torch.float32)  # noqa: E731
        ref = run()["model_outputs"]
        med, lo, hi = median_ms(run, args.reps, args.warmup)
    print(json.dumps({"op": "torch-ROCm fp32 (oracle restatement)", "median_ms": med, "min_ms": lo, "max_ms": hi,
                      "decoder_tflops": flops / (med * 1e-3) / 1e12}), flush=True)
    for mode in args.modes.split(","):
        m = ForwardTTS(cfg, math_mode=mode)
        m.load_state_dict(sd)
        m = m.eval().to(dev)
        aux = {"durations": durd}
        out = m.inference(tokd, aux)["model_outputs"]
        med, lo, hi = median_ms(lambda: m.inference(tokd, aux), args.reps, args.warmup)
        print(json.dumps({"op": "ForwardTTS.inference", "mode": mode, "median_ms": med, "min_ms": lo, "max_ms": hi,
                          "decoder_mmac_per_frame": 1e-6 * dec_macs_per_frame, "decoder_tflops": flops / (med * 1e-3) / 1e12,
                          "frames_per_second": frames / (med * 1e-3),
                          "max_abs_vs_torch_fp32": float((out - ref).abs().max())}), flush=True)
        _, recs = m.profile(tokd, aux)
        agg = {}
        for r in recs:
            a = agg.setdefault(r["name"], {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            a["launches"] += 1
            a["ms"] += r["ms"]
            a["flops"] += r["flops"]
            a["bytes"] += r["bytes"]
        for a in agg.values():
            a["tflops"] = a["flops"] / max(a["ms"], 1e-9) / 1e9
            a["gb_per_s"] = a["bytes"] / max(a["ms"], 1e-9) / 1e6
        print(json.dumps({"op": "tts_forward_tts_{encode,decode}_profiled", "mode": mode, "launches": agg}), flush=True)
        del m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fp32x6,bf16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--duration", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--what", default="op,model")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batch": args.batch,
                      "tokens": args.tokens, "frames": args.tokens * args.duration, "reps": args.reps,
                      "warmup": args.warmup}), flush=True)
    if "op" in args.what.split(","):
        bench_op(args, dev)
    if "model" in args.what.split(","):
        bench_model(args, dev)


if __name__ == "__main__":
    main()
