"""XTTS GPT on MI355X against the fp64 oracle (tests/_xtts_gpt_ref.py, no KV cache): the decode attention
and logits -> token ops, decode steps, greedy free runs, stopping, ragged batches, the latent pass, the
limits, and Xtts.inference down to the waveform.

Discrete choices (codes, sampled tokens) are compared exactly; test_xtts_gpt_cpu.py checks on the oracle
alone that none of them is a near tie (tests/_xtts_gpt_cases.py MARGIN).  Worst errors measured on
MI355X (max|d| / rel-RMS against fp64; DESIGN.md section 4 "XTTS GPT", Parity): decode attention 4.3e-7 /
1.5e-7; causal attention fp32x6 5.4e-7 / 1.3e-7, bf16 1.1e-2 / 2.8e-3; fp32 logits 7.1e-6 / 1.1e-6, hidden
states 5.0e-6 / 1.1e-6 and one-pass latents 7.0e-6 / 1.5e-6 over every model and run (the narrow models
3.8e-6 / 5.7e-7); step kernels against the one-pass path 3.2e-6 / 5.5e-7; bf16 logits 3.2e-2 / 4.6e-3 and
latents 2.7e-2 / 4.6e-3; Xtts.inference waveform 9.0e-7 / 5.8e-7.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _xtts_gpt_cases as C
import _xtts_gpt_ref as R
from _util import assert_close_fp32, tol
from oracle import hifigan_ref
from tts_amd import _native as N
from tts_amd import synthetic
from tts_amd.tts import HifiDecoder, Xtts, XttsGPT

pytestmark = pytest.mark.gpu

_MODELS = {}


def model(name, dev, mode="fp32", chunk=32, sd=None, key=None):
    k = (name, mode, chunk, key)
    if k not in _MODELS:
        m = XttsGPT(**C.ctor_kwargs(C.MODELS[name]), math_mode=mode, chunk=chunk)
        m.load_state_dict(sd if sd is not None else C.state_dict(C.MODELS[name], C.MODEL_SEED[name]), strict=True)
        _MODELS[k] = m.eval().to(dev)
    return _MODELS[k]


@functools.lru_cache(maxsize=None)
def oracle_sd(name):
    return R.to64(C.state_dict(C.MODELS[name], C.MODEL_SEED[name]))


@functools.lru_cache(maxsize=None)
def oracle_free_run(case):
    """Per utterance of a FREE_RUN case: the oracle's greedy run (computed once, shared)."""
    name, seed, B, T, lens, steps, pen = C.FREE_RUN[case]
    cfg = C.MODELS[name]
    cond, text = C.inputs(cfg, seed, B, T)
    outs = []
    for b in range(B):
        L = T if lens is None else lens[b]
        outs.append(R.generate(oracle_sd(name), cfg, cond[b], text[b, :L].tolist(), steps, penalty=pen))
    return cond, text, outs


# ------------------------------------------------------------------------------------ decode attention op
def attn_op(q, k, v, lens, heads):
    B, cap, E = k.shape
    out = torch.full((B, E), 7.0, device=q.device)
    N.call("tts_op_gpt_decode_attn", N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(lens), B, E, heads, cap, N.ptr(out),
           N.stream_ptr(q.device))
    return out


@pytest.mark.parametrize("dk", [32, 64, 128])
def test_decode_attention_vs_fp64(cuda_device, dk):
    """Cache lengths 1, 2, each side of every wave's split edge (64 w - 1, 64 w, 64 w + 1 for w = 1 ... waves,
    the last being the edge where the tiles wrap round the waves), one tile past the wrap, and the maximum
    (a reference-sized 1044 rows); ragged (one length per row); rows bitwise their own batch of one."""
    W = N.lib().tts_op_gpt_decode_attn_waves()
    heads, cap = 2, 1044
    lens = [1, 2] + [64 * w + d for w in range(1, W + 1) for d in (-1, 0, 1)] + [64 * (W + 1) + 1, cap]
    assert len(lens) <= N.XTTS_GPT_MAX_BATCH
    B, E = len(lens), heads * dk
    g = torch.Generator().manual_seed(dk)
    q = torch.randn(B, E, generator=g)
    k = torch.randn(B, cap, E, generator=g)
    v = torch.randn(B, cap, E, generator=g)
    ld = torch.tensor(lens, dtype=torch.int32, device=cuda_device)
    out = attn_op(q.to(cuda_device), k.to(cuda_device), v.to(cuda_device), ld, heads)
    ref = torch.empty(B, E, dtype=torch.float64)
    for b, n in enumerate(lens):
        qh = q[b].double().reshape(heads, 1, dk)
        kh = k[b, :n].double().reshape(n, heads, dk).transpose(0, 1)
        vh = v[b, :n].double().reshape(n, heads, dk).transpose(0, 1)
        ref[b] = (F.softmax(qh @ kh.transpose(1, 2) / dk**0.5, dim=-1) @ vh).reshape(E)
    ma, rr = assert_close_fp32(out.cpu(), ref, f"gpt decode attention dk{dk}", **tol("fp32"))
    print(f"decode attention dk {dk}: max|d| {ma:.2e} rel-RMS {rr:.2e}")
    for b in (0, 3, 9, 16, B - 1):
        one = attn_op(q[b:b + 1].to(cuda_device), k[b:b + 1].to(cuda_device), v[b:b + 1].to(cuda_device), ld[b:b + 1], heads)
        assert torch.equal(one[0], out[b]), f"row {b} depends on the batch"


def test_decode_attention_limits(cuda_device):
    q = torch.zeros(1, 32, device=cuda_device)
    kv = torch.zeros(1, 4, 32, device=cuda_device)
    out = torch.full((1, 32), 7.0, device=cuda_device)
    ln = torch.ones(1, dtype=torch.int32, device=cuda_device)
    st = N.lib().tts_op_gpt_decode_attn(N.ptr(q), N.ptr(kv), N.ptr(kv), N.ptr(ln), 1, 32, 2, 4, N.ptr(out),
                                        N.stream_ptr(cuda_device))
    assert st == N.TTS_ERR_UNSUPPORTED and "32, 64 or 128" in N.lib().tts_last_error().decode()  # dk 16
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------ causal attention op
def causal_ref(qkv, heads, kl):
    B, E3, T = qkv.shape
    E = E3 // 3
    dk = E // heads
    x = qkv.double()
    out = torch.zeros(B, E, T, dtype=torch.float64)
    i = torch.arange(T)
    for b in range(B):
        n = T if kl is None else int(kl[b])
        mask = (i[None, :] <= i[:, None]) & (i[None, :] < n)  # [query, key]
        q, k, v = (x[b, s * E:(s + 1) * E].reshape(heads, dk, T) for s in range(3))
        s = (q.transpose(1, 2) @ k) / dk**0.5
        p = F.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
        out[b] = (v @ p.transpose(1, 2)).reshape(E, T)
    return out


@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("Tsel", [0, 1, 2, 3, 4])
def test_mha_causal_vs_fp64(cuda_device, dk, Tsel):
    """T in {1, tile - 1, tile, tile + 1, 2 tile + 3}; B 1 and 3; with and without ragged key_lengths; fp32x6
    and bf16; row b does not depend on B."""
    from tts_amd.tts.xtts_gpt import causal_multi_head_attention as cmha

    tile = N.lib().tts_op_mha_tile()
    T = [1, tile - 1, tile, tile + 1, 2 * tile + 3][Tsel]
    heads = 2
    E = heads * dk
    qkv = torch.randn(3, 3 * E, T, generator=torch.Generator().manual_seed(100 * dk + T))
    kl = torch.tensor([T, max(1, T // 2), max(1, T - 1)])
    qd = qkv.to(cuda_device)
    for lens in (None, kl):
        ref = causal_ref(qkv, heads, lens)
        for mode in ("fp32", "bf16"):
            out = cmha(qd, heads, lens, math_mode=mode)
            ma, rr = assert_close_fp32(out.cpu(), ref, f"mha causal {mode} dk={dk} T={T} ragged={lens is not None}",
                                       **tol(mode, op=True))
            if mode == "fp32":
                print(f"mha causal dk {dk} T {T} ragged {lens is not None}: max|d| {ma:.2e} rel-RMS {rr:.2e}")
                one = cmha(qd[1:2], heads, None if lens is None else lens[1:2], math_mode=mode)
                assert torch.equal(one[0], out[1]), "row 1 depends on the batch"


@pytest.mark.parametrize("dk", [32, 64, 128])
def test_mha_causal_nothing_flows_back(cuda_device, dk):
    """Changing q, k and v at the positions > i leaves the outputs at the positions <= i bitwise unchanged,
    for cuts inside a tile, at a tile edge and in the last tile."""
    from tts_amd.tts.xtts_gpt import causal_multi_head_attention as cmha

    tile = N.lib().tts_op_mha_tile()
    T, heads = 2 * tile + 3, 2
    qkv = torch.randn(2, 3 * heads * dk, T, generator=torch.Generator().manual_seed(dk)).to(cuda_device)
    base = cmha(qkv, heads, None, math_mode="fp32")
    for i in (0, 5, tile - 1, tile, tile + 17, T - 2):
        other = qkv.clone()
        other[:, :, i + 1:] = torch.randn(2, 3 * heads * dk, T - i - 1, generator=torch.Generator().manual_seed(i)).to(cuda_device) * 3
        out = cmha(other, heads, None, math_mode="fp32")
        assert torch.equal(out[:, :, : i + 1], base[:, :, : i + 1]), f"cut after position {i}"
        assert not torch.equal(out[:, :, i + 1:], base[:, :, i + 1:])


def test_mha_causal_limits(cuda_device):
    qkv = torch.zeros(1, 3 * 32, 4, device=cuda_device)
    out = torch.full((1, 32, 4), 7.0, device=cuda_device)
    st = N.lib().tts_op_mha_causal(N.ptr(qkv), None, 1, 32, 2, 4, 1, N.ptr(out), N.stream_ptr(cuda_device))
    assert st == N.TTS_ERR_UNSUPPORTED and "32, 64, 128" in N.lib().tts_last_error().decode()  # dk 16
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------ logits -> token op
def sample_op(logits, prev, u, start, pen, temp, k, p):
    dev = logits.device
    B, V = logits.shape
    codes = torch.cat([prev.to(torch.int32), torch.full((B, 1), -5, dtype=torch.int32)], dim=1).to(dev).contiguous()
    N.call("tts_op_gpt_sample", N.ptr(logits), B, V, N.ptr(codes), prev.shape[1], start, float(pen), float(temp),
           int(k), float(p), N.ptr(u), N.stream_ptr(dev))
    assert torch.equal(codes[:, :-1].cpu(), prev.to(torch.int32))
    return codes[:, -1].cpu().tolist()


@pytest.mark.parametrize("V", C.SAMPLE_V)
def test_sample_op_token_equals_oracle(cuda_device, V):
    """Every combination of top_k in {1, 50, V}, top_p in {0.85, 1}, penalty in {1, 10}, temperature in
    {0.75, 1}, and greedy: the token is the oracle's."""
    logits, prev, u = C.sample_case(V)
    ld, ud = logits.to(cuda_device), u.to(cuda_device)
    start = V - 2
    for (k, p, pen, temp) in C.sample_combos(V):
        got = sample_op(ld, prev, ud, start, pen, temp, k, p)
        want = [R.process(logits[b], [1, start, *prev[b].tolist()], pen, temp, k, p, float(u[b]))[0]
                for b in range(logits.shape[0])]
        assert got == want, (V, k, p, pen, temp)
    for pen in (1.0, 10.0):
        got = sample_op(ld, prev, None, start, pen, 1.0, 50, 0.85)
        want = [R.process(logits[b], [1, start, *prev[b].tolist()], pen)[0] for b in range(logits.shape[0])]
        assert got == want, (V, "greedy", pen)


def test_sample_op_draws_follow_the_cdf(cuda_device):
    """Plain sampling of a 4-token distribution: u walks through the CDF's intervals in token order."""
    p = torch.tensor([0.1, 0.2, 0.3, 0.4])
    us = torch.tensor([0.05, 0.25, 0.45, 0.95, 0.0, 0.999])
    logits = p.log().repeat(len(us), 1).to(cuda_device)
    prev = torch.zeros(len(us), 0, dtype=torch.int64)
    assert sample_op(logits, prev, us.to(cuda_device), 3, 1.0, 1.0, 0, 1.0) == [0, 1, 2, 3, 0, 3]


def test_sample_op_greedy_tie_takes_the_lowest_id(cuda_device):
    V = 1026
    logits = torch.randn(3, V, generator=torch.Generator().manual_seed(3))
    top = 8.0  # above every other logit; 80 / 10 is exactly 8 in fp32
    logits[0, [700, 40, 999]] = top
    logits[1, [5, 1025]] = top
    logits[2, 1] = top * 10.0  # id 1 is always penalised: top * 10 / 10 ties with id 900
    logits[2, 900] = top
    prev = torch.zeros(3, 0, dtype=torch.int64)
    assert sample_op(logits.to(cuda_device), prev, None, V - 2, 10.0, 1.0, 0, 1.0) == [40, 5, 1]


def test_sample_op_limits(cuda_device):
    logits = torch.zeros(1, 8195, device=cuda_device)
    codes = torch.full((1, 1), -5, dtype=torch.int32, device=cuda_device)
    st = N.lib().tts_op_gpt_sample(N.ptr(logits), 1, 8195, N.ptr(codes), 0, 0, 1.0, 1.0, 0, 1.0, None,
                                   N.stream_ptr(cuda_device))
    assert st == N.TTS_ERR_UNSUPPORTED and "8194" in N.lib().tts_last_error().decode()
    assert int(codes[0, 0]) == -5


# ------------------------------------------------------------------------------------ decode steps
@pytest.mark.parametrize("name", list(C.MODELS))
def test_one_and_two_decode_steps_vs_oracle(cuda_device, name):
    """The logits of steps 0 and 1 (prefill through the step kernels, then two steps) against the oracle."""
    cfg = C.MODELS[name]
    cond, text = C.inputs(cfg, 7, 2, 5)
    m = model(name, cuda_device)
    out = m._generate(cond, text, do_sample=False, repetition_penalty=10.0, max_new_tokens=2, return_logits=True)
    for b in range(2):
        ref = R.generate(oracle_sd(name), cfg, cond[b], text[b].tolist(), 2, penalty=10.0)
        assert out["codes"][b, : ref["n"]].cpu().tolist() == ref["codes"]
        ma, rr = assert_close_fp32(out["logits"][b, : ref["n"]].cpu(), ref["logits"], f"gpt {name} two steps", **tol("fp32"))
        print(f"{name} two steps b{b}: logits max|d| {ma:.2e} rel-RMS {rr:.2e}")


def test_empty_prompt_and_empty_text(cuda_device):
    """No conditioning rows and no text token: the prefix is [start_text, stop_text] alone (the prefill gets
    NULL pointers for both inputs), for generation and for the latent pass."""
    name = "narrow"
    cfg = C.MODELS[name]
    cond = torch.zeros(1, 0, cfg["model_dim"])
    text = torch.zeros(1, 0, dtype=torch.int64)
    m = model(name, cuda_device)
    out = m._generate(cond, text, do_sample=False, repetition_penalty=10.0, max_new_tokens=5, return_logits=True)
    ref = R.generate(oracle_sd(name), cfg, cond[0], [], 5, penalty=10.0)
    assert min(i["greedy_gap"] for i in ref["infos"]) >= C.MARGIN
    n = ref["n"]
    assert out["codes"][0, :n].cpu().tolist() == ref["codes"]
    assert_close_fp32(out["logits"][0, :n].cpu(), ref["logits"], "gpt empty prefix logits", **tol("fp32"))
    if n >= 3:
        lat = m.forward(text, None, out["codes"][:, :n], None, cond_latents=cond, code_lengths=torch.tensor([n]))
        assert_close_fp32(lat[0].cpu(), R.latents(oracle_sd(name), cfg, cond[0], [], ref["codes"]),
                          "gpt empty prefix latents", **tol("fp32"))


@pytest.mark.parametrize("case", ["narrow_greedy24", "narrow32_greedy24", "reference2_6"])
def test_greedy_free_run_vs_oracle(cuda_device, case):
    """Codes identical to the oracle's, lengths, per-step logits and hidden states within the fp32 gates."""
    name, seed, B, T, lens, steps, pen = C.FREE_RUN[case]
    cond, text, outs = oracle_free_run(case)
    m = model(name, cuda_device)
    out = m._generate(cond, text, do_sample=False, repetition_penalty=pen, max_new_tokens=steps, return_logits=True,
                      return_latents=True)
    stop = C.MODELS[name]["stop_audio"]
    for b, ref in enumerate(outs):
        n = ref["n"]
        assert int(out["lengths"][b]) == n
        assert out["codes"][b, :n].cpu().tolist() == ref["codes"]
        assert bool((out["codes"][b, n:] == stop).all())
        ma, rr = assert_close_fp32(out["logits"][b, :n].cpu(), ref["logits"], f"gpt {case} logits", **tol("fp32"))
        la, lr = assert_close_fp32(out["latents"][b, :n].cpu(), ref["latents"], f"gpt {case} hidden", **tol("fp32"))
        print(f"{case} b{b}: n {n} logits max|d| {ma:.2e} rel-RMS {rr:.2e}; hidden max|d| {la:.2e} rel-RMS {lr:.2e}")
        assert bool((out["logits"][b, n:] == 0).all()) and bool((out["latents"][b, n:] == 0).all())


def test_cache_consistency_generate_then_latent_pass(cuda_device):
    """12 greedy steps (the skinny step kernels reading the KV cache), then the one-pass latent path over
    the same codes (the whole sequence on the conv path with the causal MFMA attention): the hidden states
    at the mel positions agree within the fp32 gate, and the one-pass latents agree with the oracle's."""
    name, seed, B, T, lens, steps, pen = C.FREE_RUN["narrow_ragged"]
    cfg = C.MODELS[name]
    cond, text, outs = oracle_free_run("narrow_ragged")
    m = model(name, cuda_device)
    out = m._generate(cond, text, do_sample=False, repetition_penalty=pen, max_new_tokens=steps, text_lengths=lens,
                      return_latents=True)
    codes, n = out["codes"], out["lengths"]
    assert n.cpu().tolist() == [o["n"] for o in outs] == [12, 12, 12]
    lat = m.forward(text, lens, codes, None, cond_latents=cond, code_lengths=n)
    assert lat.shape == (B, 10, cfg["model_dim"])
    ma, rr = assert_close_fp32(lat.cpu(), out["latents"][:, :10].double().cpu(), "gpt cache consistency", **tol("fp32"))
    print(f"cache consistency, step kernels vs one pass: max|d| {ma:.2e} rel-RMS {rr:.2e}")
    assert not torch.equal(lat, out["latents"][:, :10])  # two code paths, not one run twice
    for b in range(B):
        ref = R.latents(oracle_sd(name), cfg, cond[b], text[b, : lens[b]].tolist(), outs[b]["codes"])
        assert_close_fp32(lat[b].cpu(), ref, "gpt latents vs one-pass oracle", **tol("fp32"))


def test_ragged_batch_row_is_bitwise_its_own_batch_of_one(cuda_device):
    name, seed, B, T, lens, steps, pen = C.FREE_RUN["narrow_ragged"]
    cond, text, outs = oracle_free_run("narrow_ragged")
    m = model(name, cuda_device)
    kw = dict(do_sample=False, repetition_penalty=pen, max_new_tokens=steps, return_logits=True)
    full = m._generate(cond, text, text_lengths=lens, **kw)
    for b in range(B):
        assert full["codes"][b].cpu().tolist() == outs[b]["codes"]
        one = m._generate(cond[b:b + 1], text[b:b + 1, : lens[b]], **kw)
        assert torch.equal(one["codes"][0], full["codes"][b])
        assert torch.equal(one["logits"][0], full["logits"][b]), f"utterance {b} depends on the batch"


def test_sampled_run_is_reproducible_and_follows_the_oracle(cuda_device):
    """do_sample with the reference's defaults (top_k 50, top_p 0.85, temperature 0.75, penalty 10): the same
    generator seed gives the same codes, and they are the oracle's draws from the same uniforms."""
    sr = C.SAMPLED_RUN
    name = sr["model"]
    cfg = C.MODELS[name]
    cond, text = C.inputs(cfg, sr["seed"], sr["B"], sr["T"])
    m = model(name, cuda_device)
    S = sr["steps"]
    u = C.sampled_run_uniforms()
    a = m._generate(cond, text, max_new_tokens=S, uniforms=u)
    b = m._generate(cond, text, max_new_tokens=S, uniforms=u)
    assert torch.equal(a["codes"], b["codes"])
    g1 = m.generate(cond, text, max_new_tokens=S, generator=torch.Generator().manual_seed(5))
    g2 = m.generate(cond, text, max_new_tokens=S, generator=torch.Generator().manual_seed(5))
    assert g1.dtype == torch.int64 and torch.equal(g1, g2)
    for i in range(2):
        # the draw margins of every step of this case are checked on the oracle in test_xtts_gpt_cpu.py
        ref = R.generate(oracle_sd(name), cfg, cond[i], text[i].tolist(), S, sr["penalty"], sr["temperature"],
                         sr["top_k"], sr["top_p"], u[i].tolist())
        assert a["codes"][i, : ref["n"]].cpu().tolist() == ref["codes"]
        assert int(a["lengths"][i]) == ref["n"]


# ------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("case", ["narrow_greedy24", "reference2_6"])
def test_bf16_teacher_forced_on_the_oracle_codes(cuda_device, case):
    name, seed, B, T, lens, steps, pen = C.FREE_RUN[case]
    cfg = C.MODELS[name]
    cond, text, outs = oracle_free_run(case)
    n = [o["n"] for o in outs]
    codes = torch.full((B, max(n)), cfg["stop_audio"], dtype=torch.int64)
    for b, o in enumerate(outs):
        codes[b, : n[b]] = torch.tensor(o["codes"])
    m = model(name, cuda_device, mode="bf16")
    lat, logits = m.forward(text, None, codes, None, cond_latents=cond, code_lengths=torch.tensor(n), return_logits=True)
    for b, o in enumerate(outs):
        rl, rg = R.teacher_forced(oracle_sd(name), cfg, cond[b], text[b].tolist(), o["codes"])
        ma, rr = assert_close_fp32(logits[b, : n[b] + 2].cpu(), rg, f"gpt {case} bf16 logits", **tol("bf16"))
        la, lr = assert_close_fp32(lat[b, : n[b] - 2].cpu(), rl[:-4], f"gpt {case} bf16 latents", **tol("bf16"))
        print(f"{case} bf16 b{b}: logits max|d| {ma:.2e} rel-RMS {rr:.2e}; latents max|d| {la:.2e} rel-RMS {lr:.2e}")


# ------------------------------------------------------------------------------------ stopping
def test_stopping_ragged_batch_and_chunks(cuda_device):
    s = C.STOP_CASE
    cfg = C.MODELS[s["model"]]
    cond, text = C.inputs(cfg, s["seed"], s["B"], s["T"])
    S, stop = s["steps"], cfg["stop_audio"]
    first = None
    for chunk in (1, 5, 32):
        m = model(s["model"], cuda_device, chunk=chunk, sd=C.stop_state_dict(), key="stop")
        out = m._generate(cond, text, do_sample=False, repetition_penalty=s["penalty"], max_new_tokens=S,
                          text_lengths=s["lens"], return_logits=True)
        n = out["lengths"].cpu().tolist()
        assert n == s["n"]
        for b in range(s["B"]):
            assert int(out["codes"][b, n[b] - 1]) == stop and bool((out["codes"][b, n[b]:] == stop).all())
            assert not bool((out["codes"][b, : n[b] - 1] == stop).any())
        # the loop ends within one chunk of the last end
        assert out["steps_run"] == min(S, -(-max(n) // chunk) * chunk)
        if first is None:
            first = out
        else:
            assert torch.equal(out["codes"], first["codes"]) and torch.equal(out["logits"], first["logits"])
    assert m.generate(cond, text, do_sample=False, max_new_tokens=S, text_lengths=s["lens"]).shape == (3, max(s["n"]))


# ------------------------------------------------------------------------------------ latent pass
def test_latent_pass_trimming_and_zero_rows(cuda_device):
    name = "narrow"
    cfg = C.MODELS[name]
    cond, text = C.inputs(cfg, 13, 3, 6)
    n = [12, 7, 9]
    codes = torch.randint(0, cfg["n_audio"] - 2, (3, 12), generator=torch.Generator().manual_seed(4))
    m = model(name, cuda_device)
    lat = m.forward(text, None, codes, torch.tensor([v * m.code_stride_len - 3 for v in n]), cond_latents=cond)
    assert lat.shape == (3, 10, cfg["model_dim"])
    for b in range(3):
        ref = R.latents(oracle_sd(name), cfg, cond[b], text[b].tolist(), codes[b, : n[b]].tolist())
        assert ref.shape[0] == n[b] - 2
        assert_close_fp32(lat[b, : n[b] - 2].cpu(), ref, "gpt latent pass", **tol("fp32"))
        assert bool((lat[b, n[b] - 2:] == 0).all())


def test_reference2_latents(cuda_device):
    name, seed, B, T, lens, steps, pen = C.FREE_RUN["reference2_6"]
    cfg = C.MODELS[name]
    cond, text, outs = oracle_free_run("reference2_6")
    codes = torch.tensor([o["codes"] for o in outs])
    lat = model(name, cuda_device).forward(text, None, codes, None, cond_latents=cond, code_lengths=torch.tensor([6, 6]))
    for b in range(B):
        ref = R.latents(oracle_sd(name), cfg, cond[b], text[b].tolist(), outs[b]["codes"])
        ma, rr = assert_close_fp32(lat[b].cpu(), ref, "gpt reference2 latents", **tol("fp32"))
        print(f"reference2 latents b{b}: max|d| {ma:.2e} rel-RMS {rr:.2e}")


# ------------------------------------------------------------------------------------ limits, workspace
def test_limits_leave_the_outputs_untouched(cuda_device):
    name = "narrow"
    cfg = C.MODELS[name]
    m = model(name, cuda_device)
    lib = N.lib()
    cond, text = C.inputs(cfg, 1, 1, 4)
    m._generate(cond, text, do_sample=False, max_new_tokens=4)  # a valid prefix in the handle
    h = m._native_handle(cfg["P"])
    stream = N.stream_ptr(cuda_device)
    E = cfg["model_dim"]

    def prefill(B, T, S):
        c = torch.zeros(B, cfg["P"], E, device=cuda_device)
        t = torch.ones(B, T, dtype=torch.int64, device=cuda_device)
        return lib.tts_xtts_gpt_prefill(h, N.ptr(c), N.ptr(t), None, B, T, S, stream)

    assert prefill(N.XTTS_GPT_MAX_BATCH + 1, 4, 4) == N.TTS_ERR_UNSUPPORTED
    assert "more than 32 utterances" in lib.tts_last_error().decode()
    assert prefill(1, cfg["text_positions"] - 1, 4) == N.TTS_ERR_INVALID  # T + 2 > the text positions
    assert "text positions" in lib.tts_last_error().decode()
    assert prefill(1, 4, cfg["mel_positions"] + 1) == N.TTS_ERR_INVALID
    assert "mel positions" in lib.tts_last_error().decode()
    # generate and latents refuse what the prefill did not reserve, and fill nothing
    codes = torch.full((1, 8), -7, dtype=torch.int32, device=cuda_device)
    lens = torch.full((1,), -7, dtype=torch.int32, device=cuda_device)
    logits = torch.full((1, 8, cfg["n_audio"]), 7.0, device=cuda_device)
    ran = ctypes.c_int(-1)

    def generate(S):
        return lib.tts_xtts_gpt_generate(h, S, 10.0, 1.0, 0, 1.0, None, N.ptr(codes), N.ptr(lens), N.ptr(logits), None,
                                         ctypes.byref(ran), stream)

    assert prefill(1, 4, 4) == N.TTS_OK
    assert generate(8) == N.TTS_ERR_INVALID  # more steps than the prefill reserved
    assert "max_new_tokens" in lib.tts_last_error().decode()
    assert generate(0) == N.TTS_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((codes == -7).all()) and bool((lens == -7).all()) and bool((logits == 7.0).all()) and ran.value == -1
    lat = torch.full((1, 8, E), 7.0, device=cuda_device)
    st = lib.tts_xtts_gpt_latents(h, N.ptr(codes), N.ptr(lens), 8, 8, N.ptr(lat), None, stream)
    assert st == N.TTS_ERR_INVALID and bool((lat == 7.0).all())
    with pytest.raises(IndexError):
        m.generate(cond, torch.full((1, 4), cfg["n_text"]))


def test_workspace_reuse_across_sizes(cuda_device):
    name = "narrow"
    cfg = C.MODELS[name]
    m = model(name, cuda_device)
    kw = dict(do_sample=False, repetition_penalty=10.0, return_logits=True)
    c1, t1 = C.inputs(cfg, 21, 1, 3)
    c3, t3 = C.inputs(cfg, 22, 3, 9)
    a = m._generate(c1, t1, max_new_tokens=6, **kw)
    big = m._generate(c3, t3, max_new_tokens=20, **kw)
    b = m._generate(c1, t1, max_new_tokens=6, **kw)
    assert torch.equal(a["codes"], b["codes"]) and torch.equal(a["logits"], b["logits"])
    big2 = m._generate(c3, t3, max_new_tokens=20, **kw)
    assert torch.equal(big["codes"], big2["codes"]) and torch.equal(big["logits"], big2["logits"])


# ------------------------------------------------------------------------------------ Xtts.inference
DEC = dict(decoder_input_dim=128, upsample_rates_decoder=(8, 8, 2, 2), upsample_initial_channel_decoder=128,
           upsample_kernel_sizes_decoder=(16, 16, 4, 4), d_vector_dim=32)
DEC_CFG = dict(in_channels=128, out_channels=1, resblock_type="1", resblock_dilation_sizes=[[1, 3, 5]] * 3,
               resblock_kernel_sizes=[3, 7, 11], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=128,
               upsample_factors=[8, 8, 2, 2], inference_padding=0, cond_channels=32, conv_pre_weight_norm=False,
               conv_post_weight_norm=False, conv_post_bias=False, cond_in_each_up_layer=True)


@pytest.mark.parametrize("length_scale", [1.0, 1.25])
def test_xtts_inference_waveform_vs_oracle_chain(cuda_device, length_scale):
    """Token ids -> codes -> latents -> 24 kHz waveform against the GPT oracle followed by the fp64 decoder
    chain (the reference's two F.interpolate calls and oracle/hifigan_ref), greedy so that the codes are the
    oracle's."""
    name, seed, B, T, lens, steps, pen = C.FREE_RUN["narrow_greedy24"]
    cfg = C.MODELS[name]
    cond, text, outs = oracle_free_run("narrow_greedy24")
    dsd = synthetic.hifigan_state_dict(**DEC_CFG, seed=99, weight_norm=True)
    dec = HifiDecoder(**DEC, math_mode="fp32")
    dec.waveform_decoder.load_state_dict(dsd)
    dec = dec.eval().to(cuda_device)
    x = Xtts(model(name, cuda_device), dec, gpt_max_new_tokens=steps)
    g = torch.randn(1, 32, 1, generator=torch.Generator().manual_seed(8)) * 0.5
    out = x.inference(text[:1], cond[:1], g.to(cuda_device), do_sample=False, repetition_penalty=pen,
                      length_scale=length_scale)
    ref = outs[0]
    n = ref["n"]
    assert out["gpt_codes"][0].cpu().tolist() == ref["codes"] and out["lengths"].cpu().tolist() == [n]
    lat = R.latents(oracle_sd(name), cfg, cond[0], text[0].tolist(), ref["codes"]).unsqueeze(0)
    if length_scale != 1.0:
        lat = F.interpolate(lat.transpose(1, 2), scale_factor=length_scale, mode="linear").transpose(1, 2)
    assert_close_fp32(out["gpt_latents"].cpu(), lat, "xtts inference latents", **tol("fp32"))
    z = F.interpolate(lat.transpose(1, 2), scale_factor=[1024 / 256], mode="linear")
    z = F.interpolate(z, scale_factor=[24000 / 22050], mode="linear")
    wav = hifigan_ref.hifigan_forward(dsd, z, pad=0, g=g, dtype=torch.float64, fold_dtype=torch.float64, **DEC_CFG)
    ma, rr = assert_close_fp32(out["wav"].cpu(), wav, f"xtts inference wav x{length_scale}", **tol("fp32"))
    print(f"xtts inference length_scale {length_scale}: wav {tuple(out['wav'].shape)} max|d| {ma:.2e} rel-RMS {rr:.2e}")
