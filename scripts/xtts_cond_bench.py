#!/usr/bin/env python
"""Time XTTS voice cloning on the device (the numbers of DESIGN.md's "XTTS conditioning" section): the
reference widths (E = 1024, 16 heads, 6 attention blocks, perceiver depth 2, 32 latents) on 6 s and 30 s of
22 050 Hz audio (1 and 5 chunks of 517 frames), in the fp32-faithful mode and in bf16, against the same ops in
torch fp32 eager on the same device, inputs and weights, in the same process (tests/_xtts_cond_ref.py at
dtype float32: torch.stft + matmul for the mel, F.conv1d / einsum / softmax for the encoder and the
perceiver, F.conv1d with the resample table).  Stages: ``mel`` (one 6 s chunk), ``style_emb`` (one chunk's
mel -> 32 x E), ``latents`` (get_gpt_cond_latents of the whole clip: mel + style_emb per chunk + mean) and
``resample`` (30 s, 22 050 -> 16 000 Hz).  Every constant of both sides (window, filterbank, resample table,
weights, mel_norms) is on the device before anything is timed.  The mel and the resampler are the same code in
every math mode and are timed once per round.  ``--rounds`` rounds, the contestants' order rotating from round
to round; every round's figures are printed.  A host clock around windows of ``--calls`` calls that end in a
device synchronise, warm; per call: median, minimum and maximum over ``--reps`` windows.  Also prints the
per-launch table of ``tts_xtts_cond_style_emb_profiled`` summed by name.  One JSON line per measurement."""
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

import _xtts_cond_cases as C  # noqa: E402
import _xtts_cond_ref as R  # noqa: E402
from tts_amd import audio  # noqa: E402
from tts_amd.tts import Xtts, XttsConditioning  # noqa: E402


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
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--seconds", default="6,30")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    C.MODELS["bench"] = dict(model_dim=1024, heads=16, attn_blocks=args.blocks, perceiver_depth=args.depth)
    C.MODEL_SEED["bench"] = 41
    sd = C.state_dict("bench")
    norms = C.mel_norms()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "model_dim": 1024,
                      "heads": 16, "attn_blocks": args.blocks, "perceiver_depth": args.depth, "reps": args.reps,
                      "calls_per_window": args.calls, "warmup": args.warmup}), flush=True)
    clips = {s: C.clip(int(s) * 22050, seed=int(s)).to(dev) for s in args.seconds.split(",")}
    chunk = next(iter(clips.values()))[:, : 6 * 22050].contiguous()
    long_clip = C.clip(30 * 22050, seed=30).to(dev)

    def emit(stage, mode, t, **kw):
        print(json.dumps(dict(stage=stage, mode=mode, ms=round(t[0], 4), ms_min=round(t[1], 4), ms_max=round(t[2], 4),
                              **kw)), flush=True)

    # every operand of both sides is resident on the device before anything is timed: the library keeps its
    # window, filterbank and resample table in its arena, eager gets the same as fp32 device tensors
    f32 = torch.float32
    sdd = {k: v.to(dev) for k, v in sd.items()}
    nd = norms.to(dev)
    consts = R.mel_constants(dev, f32)
    kern, o, n, w = R.resample_table(22050, 16000)
    table = (kern, o, n, w)
    kern_dev = kern.float().to(dev)
    models = {}
    for mode in args.modes.split(","):
        m = XttsConditioning(**C.ctor_kwargs("bench"), math_mode=mode)
        m.load_state_dict(sd, strict=True)
        models[mode] = m.eval().to(dev)
    mel = models[args.modes.split(",")[0]].wav_to_mel_cloning(chunk, norms)
    T = mel.shape[-1]

    def timed(fn):
        return median_ms(fn, args.reps, args.warmup, args.calls)

    def run_lib(mode, rnd):
        m = models[mode]
        x = Xtts(None, None, conditioning=m, mel_stats=norms).to(dev)
        emit("style_emb", mode, timed(lambda: m.get_style_emb(mel)), frames=T, round=rnd)
        for s, wav in clips.items():
            emit("latents", mode, timed(lambda: x.get_gpt_cond_latents(wav, 22050, length=30, chunk_length=6)),
                 seconds=int(s), round=rnd)

    def run_front(rnd):  # the same code in every math mode: timed once per round
        m = models[args.modes.split(",")[0]]
        emit("mel", "library", timed(lambda: m.wav_to_mel_cloning(chunk, nd)), frames=T, round=rnd)
        emit("resample", "library", timed(lambda: audio.resample(long_clip, 22050, 16000)), seconds=30, round=rnd)

    def run_torch(rnd):
        with torch.no_grad():
            emit("mel", "torch_eager", timed(lambda: R.wav_to_mel_cloning(chunk, nd, f32, consts)), frames=T, round=rnd)
            emit("style_emb", "torch_eager", timed(lambda: R.style_emb(sdd, mel, 16, 8, 64, f32)), frames=T, round=rnd)
            for s, wav in clips.items():
                emit("latents", "torch_eager",
                     timed(lambda: R.gpt_cond_latents(sdd, wav, 22050, nd, 16, dtype=f32, constants=consts)),
                     seconds=int(s), round=rnd)
            emit("resample", "torch_eager",
                 timed(lambda: R.resample(long_clip, 22050, 16000, f32, table=table, kernel=kern_dev)), seconds=30,
                 round=rnd)

    # the order of the contestants rotates from round to round, so that no one always runs first (cold clocks)
    jobs = [("front", run_front)] + [(mode, (lambda r, mode=mode: run_lib(mode, r))) for mode in models]
    if not args.no_torch:
        jobs.append(("torch", run_torch))
    for rnd in range(args.rounds):
        order = jobs[rnd % len(jobs):] + jobs[:rnd % len(jobs)]
        print(json.dumps({"round": rnd, "order": [j[0] for j in order]}), flush=True)
        for _, fn in order:
            fn(rnd)
    for mode, m in models.items():
        _, rows = m.get_style_emb(mel, profile=True)
        by = {}
        for r in rows:
            e = by.setdefault(r["name"], [0, 0.0])
            e[0] += 1
            e[1] += r["ms"]
        total = sum(v[1] for v in by.values())
        print(json.dumps({"stage": "style_emb_launches", "mode": mode, "launches": len(rows), "sum_ms": round(total, 4),
                          "by_name": {k: {"n": v[0], "ms": round(v[1], 4)} for k, v in by.items()}}), flush=True)


if __name__ == "__main__":
    main()
