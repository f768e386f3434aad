"""The 64-channel f16x3 kernels on 256-column tiles (swizzled 64-byte LDS rows), at their tile edges.

``_geo64_wide.py`` lists the forms (the pair at kernels 3 / 7 / 11, the kernel-11 pair with
``conv_post`` in its epilogue, the kernel-3 whole block, and that block as its stage's last launch
with the next stage's x2 upsampler in its tail, at kernels [3] and [3, 7]) with the tile strides S
restated from the source.  B = 2, stage lengths 4, S - 2, S, S + 2, 2 S and 3 S + 6.

Exact arm (``_mrf_exact``'s 0 / 1 weights: every activation an integer multiple of a power of two,
``conv_post`` = 2^-16, only ``tanhf`` inexact), per case and weight seed:

* the profiled forward runs the form's launch the expected number of times, no Winograd launch,
  and, with the tail, no upsampler launch for the second stage;
* max |out - fp64 oracle| <= ``_mrf_exact.GATE`` (an eighth of what one wrong element of the stage
  moves the waveform by);
* the output equals, bit for bit, that of the same generator created with
  ``TTS_MI355X_GEO64_WIDE=0`` (the narrow tiles the existing suite holds to the same reference: the
  same integer argument through the same ``tanhf``);
* the plain forward equals the profiled one, row 0 of the B = 2 run equals the B = 1 run, and two
  runs are equal, all bitwise.

Dense arm (ordinary synthetic weights, L = S + 2 and 3 S + 6): against the fp64 oracle under the
f16x3 gates of ``_util.tol``, against the narrow-tile arm at twice those gates (the two differ only
in the per-tile power-of-two scales of the staged operands), two runs and B = 1 against row 0
bitwise.

The launch names are the same for both geometries, and on these generators the dense outputs of
the two arms come out bitwise equal as well (the per-tile scales are powers of two and nothing
here reaches fp16 subnormals), so no output tells them apart: that the default runs the 256-column
kernels is held by the dispatch lines ``test_geo64_wide_cpu.py`` pins, and was shown once by
mutating only the 256-column instances, which fails these tests.
"""
import functools

import numpy as np
import pytest
import torch

import _geo64_wide as W
import _mrf_exact as X
from _util import assert_close_fp32, log_error, max_abs, tol
from tts_amd.vocoder import HifiganGenerator

DEV = torch.device("cuda", 0)


@functools.lru_cache(maxsize=8)
def _generator(name, weights, wide):
    """``weights``: a seed of the exact arm, or "dense".  Call and use inside ``W.env(form, wide)``."""
    form = W.FORM[name]
    g = HifiganGenerator(**form.cfg, math_mode=W.MODE)
    g.remove_weight_norm()
    g.load_state_dict(W.dense_sd(name) if weights == "dense" else W.exact_sd(name, weights))
    g.eval()
    return g.to(DEV)


def _profiled(form, g, mel, what):
    out, rows = g.profile(mel, pad=0)
    names = [r["name"] for r in rows]
    assert names.count(form.launch) == form.count, f"{what}: expected {form.count} x {form.launch}, ran {names}"
    assert not [n for n in names if n.startswith("mrf_wino")], f"{what}: a Winograd launch ran: {names}"
    if form.name in W.TAIL:
        assert W.TAIL[form.name] not in names, f"{what}: the upsampler ran as its own launch: {names}"
        if form.name == "block_up_k7":
            assert names.count("mrf_pair_k7_c64") == 3, f"{what}: {names}"
    return out


def _invariants(g, mel, out, what):
    assert torch.equal(g(mel), out), f"{what}: profiled and plain forward differ"
    assert torch.equal(g(mel), out), f"{what}: two runs differ"
    assert torch.equal(g(mel[:1])[0], out[0]), f"{what}: row 0 depends on the batch"


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage_len", W.CASES)
def test_exact(cuda_device, name, stage_len):
    form = W.FORM[name]
    for seed in range(form.n_seeds):
        what = f"geo64 exact {name} L={stage_len} seed={seed}"
        mel = W.exact_input(name, stage_len, seed).to(DEV)
        with W.env(form, True):
            g = _generator(name, seed, True)
            out = _profiled(form, g, mel, what)
            _invariants(g, mel, out, what)
        ref = W.exact_oracle(name, stage_len, seed)
        o = out.cpu().numpy()
        assert o.shape == tuple(ref.shape) and np.isfinite(o).all(), what
        err = max_abs(o, ref.numpy())
        log_error(what, err, 0.0, X.GATE)
        assert err <= X.GATE, f"{what}: max|d| = {err:.3e}, gate {X.GATE:.3e} (one wrong element moves it by >= {2 * X.GATE:.1e})"
        with W.env(form, False):
            narrow = _profiled(form, _generator(name, seed, False), mel, what + " narrow")
        n = int((narrow != out).sum())
        assert n == 0, f"{what}: differs from the narrow tiles at {n} samples"


@functools.lru_cache(maxsize=None)
def _dense_arms(name, stage_len):
    """(wide, narrow) outputs of one dense case, on the CPU; the wide arm with its invariants."""
    form = W.FORM[name]
    what = f"geo64 dense {name} L={stage_len}"
    mel = W.dense_input(name, stage_len).to(DEV)
    with W.env(form, True):
        g = _generator(name, "dense", True)
        out = _profiled(form, g, mel, what)
        _invariants(g, mel, out, what)
    with W.env(form, False):
        narrow = _profiled(form, _generator(name, "dense", False), mel, what + " narrow")
    return out.cpu(), narrow.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage_len", W.DENSE_CASES)
def test_dense(cuda_device, name, stage_len):
    what = f"geo64 dense {name} L={stage_len}"
    out, narrow = _dense_arms(name, stage_len)
    gates = tol(W.MODE)
    assert_close_fp32(out, W.dense_oracle(name, stage_len), what, **gates)
    assert_close_fp32(out, narrow.double(), what + " against the narrow tiles",
                      max_abs_tol=2 * gates["max_abs_tol"], rel_rms_tol=2 * gates["rel_rms_tol"])
