"""Every fused MRF kernel form at its tile edges, checked exactly in every math mode that takes it.

``_mrf_exact.py`` builds generators whose activations are small non-negative multiples of a power
of two (0 / 1 weights, zero biases, a 0 / 1 mel, ``conv_post`` = 2^-16), so fp32x6, f16x3 and bf16
must all reproduce ``conv_post``'s argument bit for bit and only ``tanhf`` is inexact; its module
docstring has the argument, the table of forms with their tile strides S, and what is out of scope
(geometries behind environment variables cached in a function-local ``static``, Winograd launches,
the plain fp32 mode, which takes no fused form).  ``test_mrf_exact_cpu.py`` asserts, without a
GPU, that the inputs have the properties the argument needs.

Per form the stage under test runs at: the smallest reachable length, the longest one shorter than
the form's lead / halo, the nearest ones below and above the stride S, S itself where reachable,
and 3 S + 10 rounded up (four tiles, the last ragged).  Reachable is a multiple of the product of
the upsampling factors up to the stage under test: 2 for most forms, 8 for the forms on bf16
activation planes (first factor 8), 4 for the one form whose second stage is under test.  B = 3.

Per (form, length, mode), for each of the form's weight seeds (together they put a weight into
every (32-row block, 16-channel group, tap) of every conv of the block):

* the profiled forward runs the form's launch the expected number of times and no ``mrf_wino_*``
  launch at all (in any stage, which is more than the stage under test), and the first
  upsampler's profiled bytes show bf16 activation planes exactly in the ``_x8`` forms;
* max |out - fp64 oracle| <= ``GATE`` = 2^-16 (1 - tanh(0.25)^2) / 8 = 1.8e-6, an eighth of what one
  unit error moves the waveform by at one kernel per stage and half of it at four;
* the plain forward equals the profiled one, every row of the B = 3 run equals its B = 1 run, and
  two runs are equal, all bitwise.

``test_modes_bitwise_equal`` then holds the modes of a case to each other, bitwise: the same
argument through the same ``tanhf``.

The dense arm repeats the topologies and lengths of the forms that exist only in the bf16 scheme
(and of the bf16 activation planes) with ordinary synthetic weights, against the fp64 oracle at
``tol("bf16")``, and at ``tol("f16x3")`` where f16x3 takes the form too.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import _mrf_exact as X
from _util import assert_close_fp32, log_error, max_abs, tol
from tts_amd.vocoder import HifiganGenerator

EXACT = [(f.name, n, m) for f in X.FORMS for m in f.modes for n in f.lengths()]
MULTI = [(f.name, n) for f in X.FORMS if len(f.modes) > 1 for n in f.lengths()]
DENSE = [(f.name, n, m) for f in X.FORMS if f.dense for m in f.modes if m in ("bf16", "f16x3") for n in f.lengths()]
DEV = torch.device("cuda", 0)


@contextlib.contextmanager
def _env(form):
    """The form's switches, and none of the others, for the length of the block: they are read when
    a generator's first forward creates its native handle."""
    saved = {k: os.environ.pop(k, None) for k in X.ENV_SWITCHES}
    os.environ.update(dict(form.env))
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=8)  # the cases are ordered by form: a few generators stay alive
def _generator(name, mode, weights):
    """``weights``: a seed of the exact arm, or "dense"."""
    form = X.FORM[name]
    g = HifiganGenerator(**form.cfg, math_mode=mode)
    g.remove_weight_norm()
    g.load_state_dict(X.dense_sd(name) if weights == "dense" else X.exact_sd(name, weights))
    g.eval()
    return g.to(DEV)


def _profiled(form, g, mel, mode, what):
    out, rows = g.profile(mel, pad=0)
    names = [r["name"] for r in rows]
    assert names.count(form.launch) == form.count, f"{what}: expected {form.count} x {form.launch}, ran {names}"
    assert not [n for n in names if n.startswith("mrf_wino")], f"{what}: a Winograd launch ran: {names}"
    # bf16 activation planes are on exactly where the form says (bf16 behind a x8 first upsampler):
    # the first upsampler's profiled bytes count 2 bytes per activation then, 4 otherwise
    # (hifigan.cpp forward_plain, ``ubytes``)
    u, cin = form.cfg["upsample_factors"][0], form.cfg["upsample_initial_channel"]
    T = mel.shape[2]
    es = 2 if (mode == "bf16" and u == 8) else 4
    row = next(r for r in rows if r["name"] == f"ups_u{u}_c{cin // 2}")
    want = es * (X.B * cin * T + X.B * (cin // 2) * T * u) + 4 * cin * (cin // 2) * 2 * u
    assert row["bytes"] == want, f"{what}: {row['name']} moved {row['bytes']} bytes, {want} with {es}-byte planes"
    return out


@functools.lru_cache(maxsize=None)
def _exact_out(name, stage_len, mode, seed):
    """One exact case with all its assertions; the output (a small array) is kept, so the cross-mode
    test compares what the per-mode test produced, whichever of them runs first."""
    form = X.FORM[name]
    what = f"exact {name} L={stage_len} {mode} seed={seed}"
    with _env(form):
        g = _generator(name, mode, seed)
        mel = X.exact_input(name, stage_len, seed).to(DEV)
        out = _profiled(form, g, mel, mode, what)
        ref = X.exact_oracle(name, stage_len, seed)
        o = out.cpu().numpy()
        assert o.shape == tuple(ref.shape) and np.isfinite(o).all(), what
        err = max_abs(o, ref.numpy())
        log_error(what, err, 0.0, X.GATE)
        assert err <= X.GATE, f"{what}: max|d| = {err:.3e}, gate {X.GATE:.3e} (one wrong element moves it by >= {2 * X.GATE:.1e})"
        assert torch.equal(g(mel), out), f"{what}: profiled and plain forward differ"
        for row in range(X.B):
            one = g(mel[row:row + 1]).cpu().numpy()
            assert np.array_equal(one[0], o[row]), f"{what}: row {row} depends on the batch"
        assert np.array_equal(g(mel).cpu().numpy(), o), f"{what}: two runs differ"
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage_len,mode", EXACT)
def test_exact(cuda_device, name, stage_len, mode):
    for seed in range(X.FORM[name].n_seeds):
        _exact_out(name, stage_len, mode, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage_len", MULTI)
def test_modes_bitwise_equal(cuda_device, name, stage_len):
    form = X.FORM[name]
    for seed in range(form.n_seeds):
        first = _exact_out(name, stage_len, form.modes[0], seed)
        for mode in form.modes[1:]:
            n = int((_exact_out(name, stage_len, mode, seed) != first).sum())
            assert n == 0, f"{name} L={stage_len} seed={seed}: {mode} and {form.modes[0]} differ at {n} samples"


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage_len,mode", DENSE)
def test_dense(cuda_device, name, stage_len, mode):
    form = X.FORM[name]
    what = f"dense {name} L={stage_len} {mode}"
    with _env(form):
        g = _generator(name, mode, "dense")
        mel = X.dense_input(name, stage_len).to(DEV)
        out = _profiled(form, g, mel, mode, what)
        assert_close_fp32(out.cpu(), X.dense_oracle(name, stage_len), what, **tol(mode))
        assert torch.equal(g(mel), out), f"{what}: profiled and plain forward differ"
