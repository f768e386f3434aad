"""Tacotron2 on MI355X against the fp64 oracle (tests/_tacotron2_ref.py): the LSTM-cell op, single steps
of the decoder, the token-axis edges of the attention kernel and the packed biLSTM, free-running
decoding, chunking, per-utterance stopping, batch invariance, the reference widths, the limits and the
Synthesizer chain.  Gates: tests/_util.py tol(); every measured error is logged with log_error
(TTS_ERRLOG)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _tacotron2_cases as C
import _tacotron2_ref as R
from _util import assert_close_fp32, log_error, max_abs, rel_rms, tol
from tts_amd import _native as N
from tts_amd.tts import Tacotron2, lstm_cell

pytestmark = pytest.mark.gpu
OUTPUTS = ("model_outputs", "decoder_outputs", "alignments", "stop_tokens")


# ------------------------------------------------------------------ the op
@functools.lru_cache(maxsize=None)
def cell_case(H, I, B):
    """(x, h, c, weights, fp64 LSTMCell outputs): computed once, shared by the modes."""
    g = torch.Generator().manual_seed(1000 * H + 10 * I + B)
    x, h, c = (torch.randn(B, n, generator=g) for n in (I, H, H))
    w_ih = torch.randn(4 * H, I, generator=g) / I**0.5
    w_hh = torch.randn(4 * H, H, generator=g) / H**0.5
    b_ih, b_hh = torch.randn(4 * H, generator=g) * 0.1, torch.randn(4 * H, generator=g) * 0.1
    m = torch.nn.LSTMCell(I, H).double()
    with torch.no_grad():
        for p, v in zip((m.weight_ih, m.weight_hh, m.bias_ih, m.bias_hh), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(v)
        hr, cr = m(x.double(), (h.double(), c.double()))
    return (x, h, c), (w_ih, w_hh, b_ih, b_hh), (hr, cr)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("H,I", [(8, 5), (40, 24), (96, 128), (1024, 1792)])
def test_lstm_cell_op(cuda_device, H, I, mode):
    """Against fp64 ``nn.LSTMCell``, B = 1, 3 and 32.  Measured on MI355X (worst over the shapes, max|d| /
    rel-RMS): fp32 6.1e-7 / 3.4e-7, bf16 7.3e-3 / 2.6e-3."""
    for B in (1, 3, 32):
        (x, h, c), w, (hr, cr) = cell_case(H, I, B)
        ho, co = lstm_cell(x.to(cuda_device), h.to(cuda_device), c.to(cuda_device), *w, math_mode=mode)
        assert_close_fp32(ho.cpu(), hr, f"lstm_cell {mode} H={H} I={I} B={B} h", **tol(mode, op=True))
        assert_close_fp32(co.cpu(), cr, f"lstm_cell {mode} H={H} I={I} B={B} c", **tol(mode, op=True))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_lstm_cell_batch_invariance(cuda_device, mode):
    """Column b of a B = 3 call is bitwise the B = 1 call of that column."""
    (x, h, c), w, _ = cell_case(96, 128, 3)
    dev = cuda_device
    full = lstm_cell(x.to(dev), h.to(dev), c.to(dev), *w, math_mode=mode)
    for b in range(3):
        one = lstm_cell(x[b : b + 1].to(dev), h[b : b + 1].to(dev), c[b : b + 1].to(dev), *w, math_mode=mode)
        assert torch.equal(one[0][0], full[0][b]) and torch.equal(one[1][0], full[1][b]), b


def test_lstm_cell_rejects_before_launch(cuda_device):
    dev = cuda_device
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(N.NativeError) as e:
        lstm_cell(z(33, 5), z(33, 8), z(33, 8), torch.zeros(32, 5), torch.zeros(32, 8), torch.zeros(32), torch.zeros(32))
    assert e.value.code == N.TTS_ERR_UNSUPPORTED and "32" in str(e.value)
    with pytest.raises(N.NativeError) as e:  # H = 6: no multiple of the unit block
        lstm_cell(z(1, 5), z(1, 6), z(1, 6), torch.zeros(24, 5), torch.zeros(24, 6), torch.zeros(24), torch.zeros(24))
    assert e.value.code == N.TTS_ERR_UNSUPPORTED


# ------------------------------------------------------------------ the executor
@pytest.fixture(scope="module")
def models(cuda_device):
    cache = {}

    def get(name, r=2, norm="sigmoid", mode="fp32", chunk=32):
        key = (name, r, norm, mode)
        if key not in cache:
            m = Tacotron2(C.model_args(name, r, norm), math_mode=mode)
            m.load_state_dict(C.state_dict(name, r, norm))
            m.eval()
            cache[key] = m.to(cuda_device)
        cache[key].chunk = chunk
        return cache[key]

    return get


def run_case(models, name, dev, mode="fp32", chunk=32, stop_threshold=None, rows=None):
    model, r, norm, B, T, seed, lengths, steps, thr = C.CASES[name]
    m = models(model, r, norm, mode, chunk)
    m.stop_threshold = thr if stop_threshold is None else stop_threshold
    m.max_decoder_steps = steps
    tok, kw = C.case_inputs(name)
    if rows is not None:
        tok, kw = tok[rows], {k: v[rows] for k, v in kw.items()}
    return m.inference(tok.to(dev), kw)


def check(out, ref, what, mode="fp32", gated=True):
    assert set(out) == set(OUTPUTS) | {"y_lengths"}
    assert torch.equal(out["y_lengths"].cpu(), ref["y_lengths"]), what
    worst = {}
    for k in OUTPUTS:
        o, r = out[k].cpu(), ref[k]
        if gated:
            worst[k] = assert_close_fp32(o, r, f"{what} {k}", **tol(mode))
        else:
            assert o.shape == r.shape and torch.isfinite(o).all(), what
            worst[k] = (max_abs(o, r), rel_rms(o, r))
            log_error(f"{what} {k} (logged, not gated)", *worst[k], **tol(mode))
    return worst


@pytest.mark.parametrize("norm", ["sigmoid", "softmax"])
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("steps", [1, 2])
def test_few_steps(cuda_device, models, steps, r, norm):
    """One and two decoder steps (stop disabled), B = 2, T_en = 13: every kernel of the step before errors
    can grow.  Measured on MI355X (worst over the 12 cases and four outputs): max|d| 1.4e-6, rel-RMS 1.2e-6."""
    name = f"few_s{steps}_r{r}_{norm}"
    out = run_case(models, name, cuda_device)
    assert out["decoder_outputs"].shape == (2, steps * r, 20) and out["alignments"].shape == (2, steps, 13)
    check(out, C.reference(name), f"tacotron2 {name}")


@pytest.mark.parametrize("T", C.EDGE_T)
def test_token_axis_edges(cuda_device, models, T):
    """T_en shorter than the location kernel's halo, around it, three past the attention tile's edge (131) and
    257 (three tile passes, the middle one with both halos in neighbouring tiles); B = 4 with x_lengths
    (T_en, tile edge, tile edge + 1, 1) clipped to T_en; 6 steps.  Measured on MI355X: max|d| 1.8e-6, rel-RMS
    9.5e-7 (T_en = 257: 1.5e-6 / 9.2e-7)."""
    name = f"edge{T}"
    check(run_case(models, name, cuda_device), C.reference(name), f"tacotron2 {name}")


@pytest.mark.parametrize("T", C.EDGE_T)
def test_encoder_alone(cuda_device, models, T):
    """The encoder at the same lengths: the packed reverse direction starts at each utterance's own last
    token, padded rows are exactly zero (the speaker columns are filled at every position).  Measured on
    MI355X: max|d| 1.5e-6, rel-RMS 4.5e-7."""
    name = f"edge{T}"
    tok, kw = C.case_inputs(name)
    inputs, pinp = models("narrow").encode(tok.to(cuda_device), kw)
    ref = C.reference(name)["inputs"]
    assert_close_fp32(inputs.cpu(), ref, f"tacotron2 encoder T={T}", **tol("fp32"))
    for b, n in enumerate(C.edge_lengths(T)):
        assert float(inputs[b, n:, :64].abs().max() if n < T else 0.0) == 0.0
    sd = C.state_dict("narrow")
    pref = torch.nn.functional.linear(ref, sd["decoder.attention.inputs_layer.linear_layer.weight"].double())
    assert_close_fp32(pinp.cpu(), pref.transpose(1, 2), f"tacotron2 inputs_layer T={T}", **tol("fp32", op=True))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["free", "free_softmax", "free_dvec"])
def test_free_run(cuda_device, models, name, mode):
    """40 free-running steps, B = 3, ragged lengths (23, 16, 9), a speaker embedding or d-vectors.  Gated
    where torch's own CPU evaluation in that arithmetic stays inside half the gates
    (_tacotron2_cases.FP32_GATED / BF16_GATED, checked by test_tacotron2_cpu.py), else logged.  Measured on
    MI355X (worst output, max|d| / rel-RMS): fp32 3.3e-6 / 1.2e-6 (free), 2.0e-6 / 9.0e-7 (free_softmax), 2.4e-6 /
    2.5e-6 (free_dvec); bf16 1.3e-2 / 6.0e-3 (free: logged, the analogue's own error is 2.9e-2), 9.4e-3 / 8.8e-3,
    9.2e-3 / 8.1e-3."""
    gated = (C.BF16_GATED if mode == "bf16" else C.FP32_GATED)[name]
    out = run_case(models, name, cuda_device, mode)
    assert out["model_outputs"].shape == (3, 80, 20)
    check(out, C.reference(name), f"tacotron2 {name} {mode}", mode, gated)


def test_default_mode_is_fp32_faithful(cuda_device, models):
    """The package default (f16x3) and fp32x6 run the same kernels as fp32."""
    a = run_case(models, "chunk", cuda_device, "fp32")
    for mode in (None, "fp32x6"):
        b = run_case(models, "chunk", cuda_device, mode)
        for k in OUTPUTS:
            assert torch.equal(a[k], b[k]), (mode, k)


def test_chunking_is_bitwise_invisible(cuda_device, models):
    """11 steps enqueued in chunks of 1, 5 and 32: the same bits."""
    outs = [run_case(models, "chunk", cuda_device, chunk=c) for c in (1, 5, 32)]
    assert outs[0]["decoder_outputs"].shape == (3, 22, 20)
    for o in outs[1:]:
        for k in OUTPUTS + ("y_lengths",):
            assert torch.equal(o[k], outs[0][k]), k
    check(outs[0], C.reference("chunk"), "tacotron2 chunk")


@pytest.mark.parametrize("chunk", [32, 5])
def test_stopping(cuda_device, models, chunk):
    """Per-utterance stopping at a threshold the oracle's trajectories clear by 1e-3 (test_tacotron2_cpu.py):
    two utterances stop at different steps, one is cut by max_decoder_steps = 24.  y_lengths are equal,
    rows after an utterance's end exactly zero, rows before it inside the gates; with chunk = 5 the steps
    enqueued after the last needed one leave the outputs untouched.  Measured on MI355X: max|d| 1.8e-6,
    rel-RMS 8.7e-7 at either chunk size."""
    thr, steps = C.stop_threshold()
    out = run_case(models, "stop_probe", cuda_device, chunk=chunk, stop_threshold=thr)
    ref = C.reference("stop_probe", "fp64", thr)
    assert tuple(int(v) for v in out["y_lengths"].cpu()) == tuple(2 * n for n in steps)
    for b, n in enumerate(steps):
        for k, f in (("decoder_outputs", 2), ("model_outputs", 2), ("alignments", 1), ("stop_tokens", 1)):
            assert out[k].shape[1] == f * C.STOP_STEPS
            if n < C.STOP_STEPS:
                assert float(out[k][b, f * n:].abs().max()) == 0.0, (k, b)
    check(out, ref, f"tacotron2 stopping chunk={chunk}")


def test_stopping_ends_the_loop_early(cuda_device, models):
    """Every utterance stops at step 1: the outputs are trimmed to two steps.  With chunk = 5 the steps 2 to 4
    are enqueued after the last utterance ended; the same bits come out as with chunk = 1, where nothing is
    enqueued past the end, and in the untrimmed buffers of the decode entry point every row from step 2 on
    is exactly zero."""
    p = C.reference("stop_probe")["stop_tokens"]
    thr = float(p[:, 1].min()) - 2e-3  # every utterance is above it at step 1
    assert float((p[:, 1] - thr).abs().min()) >= 1e-3
    out = run_case(models, "stop_probe", cuda_device, chunk=5, stop_threshold=thr)
    assert out["decoder_outputs"].shape == (3, 4, 20) and out["y_lengths"].tolist() == [4, 4, 4]
    ref = C.reference("stop_probe", "fp64", thr)
    check(out, ref, "tacotron2 all stop at step 1")
    exact = run_case(models, "stop_probe", cuda_device, chunk=1, stop_threshold=thr)
    for k in OUTPUTS + ("y_lengths",):
        assert torch.equal(out[k], exact[k]), k
    # the decode entry point's own buffers, all 24 rows
    m = models("narrow", chunk=5)
    tok, kw = C.case_inputs("stop_probe")
    inputs, pinp = m.encode(tok.to(cuda_device), kw)
    S, dev = C.STOP_STEPS, cuda_device
    dec, align = torch.full((3, S, 40), 7.0, device=dev), torch.full((3, S, 23), 7.0, device=dev)
    stop, steps = torch.full((3, S), 7.0, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev)
    lens, n = kw["x_lengths"].to(dev), ctypes.c_int(0)
    N.call("tts_tacotron2_decode", m._native_handle(), N.ptr(inputs), N.ptr(pinp), N.ptr(lens), 3, 23, S, float(thr),
           N.ptr(dec), N.ptr(align), N.ptr(stop), N.ptr(steps), ctypes.byref(n), N.stream_ptr(dev))
    assert n.value == 2 and steps.tolist() == [2, 2, 2]
    for buf, key in ((dec, "decoder_outputs"), (align, "alignments"), (stop, "stop_tokens")):
        assert float(buf[:, 2:].abs().max()) == 0.0, key
        assert torch.equal(buf[:, :2].reshape(out[key].shape), out[key]), key


def test_batch_invariance(cuda_device, models):
    """Utterance b of the B = 3 ragged run is bitwise its own B = 1 run at the same padded T_en and length."""
    full = run_case(models, "chunk", cuda_device)
    for b in range(3):
        one = run_case(models, "chunk", cuda_device, rows=slice(b, b + 1))
        for k in OUTPUTS:
            assert torch.equal(one[k][0], full[k][b]), (k, b)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_reference_widths(cuda_device, models, mode):
    """E = 512, Q = 1024, P = 256, A = 128, F = 32, C = 80: B = 2, T_en = 19, r = 2, 12 steps.  Measured on MI355X
    (worst output, max|d| / rel-RMS): fp32 3.3e-6 / 2.9e-6, bf16 1.6e-2 / 2.1e-2 (the alignments; gate 3e-2)."""
    gated = (C.BF16_GATED if mode == "bf16" else C.FP32_GATED)["reference"]
    out = run_case(models, "reference", cuda_device, mode)
    assert out["model_outputs"].shape == (2, 24, 80)
    check(out, C.reference("reference"), f"tacotron2 reference widths {mode}", mode, gated)


def test_limits(cuda_device, models):
    """B = 32 runs; T_en at the maximum runs for 2 steps; one past either limit is TTS_ERR_UNSUPPORTED with
    a message, as are max_decoder_steps < 1; token and speaker ids outside their tables raise IndexError."""
    m = models("narrow")
    m.stop_threshold, m.max_decoder_steps = 2.0, 2
    spk = torch.zeros(33, dtype=torch.int64)
    tok = C.tokens(33, 9, seed=1).to(cuda_device)
    out = m.inference(tok[:32], {"speaker_ids": spk[:32]})
    assert out["model_outputs"].shape == (32, 4, 20) and torch.isfinite(out["model_outputs"]).all()
    one = m.inference(tok[31:32], {"speaker_ids": spk[:1]})
    assert torch.equal(one["model_outputs"][0], out["model_outputs"][31])
    with pytest.raises(N.NativeError) as e:
        m.inference(tok, {"speaker_ids": spk})
    assert e.value.code == N.TTS_ERR_UNSUPPORTED and "32" in str(e.value)
    long = C.tokens(1, N.TACOTRON2_MAX_TOKENS + 1, seed=2).to(cuda_device)
    out = m.inference(long[:, :-1], {"speaker_ids": spk[:1]})
    assert out["alignments"].shape == (1, 2, N.TACOTRON2_MAX_TOKENS) and torch.isfinite(out["model_outputs"]).all()
    assert abs(float(out["alignments"][0, 1].sum()) - 1.0) < 1e-4
    with pytest.raises(N.NativeError) as e:
        m.inference(long, {"speaker_ids": spk[:1]})
    assert e.value.code == N.TTS_ERR_UNSUPPORTED and str(N.TACOTRON2_MAX_TOKENS) in str(e.value)
    m.max_decoder_steps = 0
    with pytest.raises(N.NativeError) as e:
        m.inference(tok[:1], {"speaker_ids": spk[:1]})
    assert e.value.code == N.TTS_ERR_UNSUPPORTED and "max_decoder_steps" in str(e.value)
    # ids outside the tables raise as torch's embedding does, before any launch
    m.max_decoder_steps = 2
    with pytest.raises(IndexError, match="token"):
        m.inference(torch.full((1, 4), 30, device=cuda_device), {"speaker_ids": spk[:1]})
    with pytest.raises(IndexError, match="speaker"):
        m.inference(tok[:1], {"speaker_ids": torch.tensor([3])})
    # the decode entry point's own checks, before any launch
    h = m._native_handle()
    for B, T in ((33, 9), (1, N.TACOTRON2_MAX_TOKENS + 1)):
        st = N.lib().tts_tacotron2_decode(h, N.ptr(tok), N.ptr(tok), None, B, T, 2, 2.0, N.ptr(tok), N.ptr(tok),
                                          N.ptr(tok), N.ptr(tok), None, N.stream_ptr(cuda_device))
        assert st == N.TTS_ERR_UNSUPPORTED and N.lib().tts_last_error()


def test_workspace_reuse(cuda_device, models):
    """A large call, a small one, the large one again on one handle: identical results."""
    a = run_case(models, "chunk", cuda_device)
    s = run_case(models, "chunk", cuda_device, rows=slice(2, 3))
    b = run_case(models, "chunk", cuda_device)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(s["model_outputs"][0], a["model_outputs"][2])


def test_synthesizer_tacotron2_hifigan(cuda_device, models):
    """Synthesizer(Tacotron2 narrow with 80 channels, HifiganGenerator small).tts_batch: the waveform has the
    right length and matches oracle mel -> HiFiGAN oracle.  Measured on MI355X: max|d| 5.1e-7, rel-RMS 1.5e-6."""
    from oracle import hifigan_ref
    from tts_amd import synthetic
    from tts_amd.config import HIFIGAN_V1
    from tts_amd.synthesizer import Synthesizer
    from tts_amd.vocoder import HifiganGenerator

    cfg = dict(in_channels=80, out_channels=1, **dict(HIFIGAN_V1, upsample_initial_channel=128))
    sd = synthetic.hifigan_state_dict(**cfg, seed=7, weight_norm=True)
    g = HifiganGenerator(**cfg)
    g.load_state_dict(sd)
    g.eval()
    g.remove_weight_norm()
    g = g.to(cuda_device)
    model, r, norm, B, T, seed, lengths, steps, thr = C.CASES["synth"]
    m = models(model, r, norm)
    m.stop_threshold, m.max_decoder_steps = thr, steps
    tok, kw = C.case_inputs("synth")
    wav, voc_in = Synthesizer(m, g).tts_batch(tok.to(cuda_device), kw["x_lengths"])
    mel = C.reference("synth")["model_outputs"].transpose(1, 2)
    assert voc_in.shape == mel.shape == (2, 80, 2 * steps)
    assert wav.shape == (2, 1, 256 * (mel.shape[2] + 10))
    with torch.no_grad():
        wref = hifigan_ref.hifigan_forward(sd, mel, pad=5, dtype=torch.float64, **cfg)
    assert_close_fp32(wav.cpu(), wref, "Synthesizer(Tacotron2 narrow80, HiFiGAN 128)", **tol("fp32"))
