"""The 32-channel f16x3 whole block on 512-column tiles (swizzled 64-byte LDS rows), at its tile edges.

``_geo32_wide.py`` lists the forms (the kernel-7 branch as one whole-block launch, first of two
branches and second of four, the position it has in HiFiGAN-v1; the kernel-11 block under
``TTS_MI355X_RB1_WHOLE_K``) with the tile strides S restated from the source: 440 / 392 at kernels
7 / 11.  B = 2, stage lengths 4, S - 2, S, S + 2, 2 S and 3 S + 6.

Exact arm (``_mrf_exact``'s 0 / 1 weights: every activation an integer multiple of a power of two,
``conv_post`` = 2^-16, only ``tanhf`` inexact), per case and weight seed:

* the profiled forward runs ``mrf_block_k{K}_c32`` once, the other launches of the form's table
  the listed number of times (no kernel-7 pair where the block took the branch) and no Winograd
  launch;
* max |out - fp64 oracle| <= ``_mrf_exact.GATE`` (an eighth of what one wrong element of the stage
  moves the waveform by);
* the output equals, bit for bit, that of the same generator created with
  ``TTS_MI355X_GEO32_WIDE=0`` (the kernel-7 pairs and the 256-column block, which the existing suite
  holds to the same reference: the same integer argument through the same ``tanhf``);
* the plain forward equals the profiled one, row 0 of the B = 2 run equals the B = 1 run, and two
  runs are equal, all bitwise.

Dense arm (ordinary synthetic weights, L = S + 2 and 3 S + 6): against the fp64 oracle under the
f16x3 gates of ``_util.tol``, against the ``=0`` arm at twice those gates (the arms differ in the
power-of-two scales of the staged operands: per tile in a block, per utterance in a pair), two runs
and B = 1 against row 0 bitwise.

``test_last_k7_branch_keeps_the_pairs``: with kernels [3, 7] the kernel-7 branch is its stage's last
MRF writer and still runs as pairs with ``conv_post`` in the last one.

The kernel-11 launch name is the same on both tiles, so no output tells the tiles apart: that
the default runs the 512-column kernels is held by the dispatch lines
``test_geo32_wide_cpu.py`` pins, and was shown once by mutating only the 512-column instances
(DESIGN.md), which fails these tests.
"""
import functools

import numpy as np
import pytest
import torch

import _geo32_wide as W
import _mrf_exact as X
from _util import assert_close_fp32, log_error, max_abs, tol
from tts_amd.vocoder import HifiganGenerator

DEV = torch.device("cuda", 0)


@functools.lru_cache(maxsize=8)
def _generator(name, weights, wide):
    """``weights``: a seed of the exact arm, or "dense".  Call and use inside ``W.env(form, wide)``."""
    form = W.ALL_FORM[name]
    g = HifiganGenerator(**form.cfg, math_mode=W.MODE)
    g.remove_weight_norm()
    g.load_state_dict(W.dense_sd(name) if weights == "dense" else W.exact_sd(name, weights))
    g.eval()
    return g.to(DEV)


def _profiled(g, mel, counts, what):
    out, rows = g.profile(mel, pad=0)
    names = [r["name"] for r in rows]
    for launch, n in counts.items():
        assert names.count(launch) == n, f"{what}: expected {n} x {launch}, ran {names}"
    assert not [n for n in names if n.startswith("mrf_wino")], f"{what}: a Winograd launch ran: {names}"
    return out


def _invariants(g, mel, out, what):
    assert torch.equal(g(mel), out), f"{what}: profiled and plain forward differ"
    assert torch.equal(g(mel), out), f"{what}: two runs differ"
    assert torch.equal(g(mel[:1])[0], out[0]), f"{what}: row 0 depends on the batch"


def _exact_case(form, counts_wide, counts_narrow, stage_len):
    name = form.name
    for seed in range(form.n_seeds):
        what = f"geo32 exact {name} L={stage_len} seed={seed}"
        mel = W.exact_input(name, stage_len, seed).to(DEV)
        with W.env(form, True):
            g = _generator(name, seed, True)
            out = _profiled(g, mel, counts_wide, what)
            _invariants(g, mel, out, what)
        ref = W.exact_oracle(name, stage_len, seed)
        o = out.cpu().numpy()
        assert o.shape == tuple(ref.shape) and np.isfinite(o).all(), what
        err = max_abs(o, ref.numpy())
        log_error(what, err, 0.0, X.GATE)
        assert err <= X.GATE, f"{what}: max|d| = {err:.3e}, gate {X.GATE:.3e} (one wrong element moves it by >= {2 * X.GATE:.1e})"
        with W.env(form, False):
            narrow = _profiled(_generator(name, seed, False), mel, counts_narrow, what + " switch at 0")
        n = int((narrow != out).sum())
        assert n == 0, f"{what}: differs from the arm with the switch at 0 at {n} samples"


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage_len", W.CASES)
def test_exact(cuda_device, name, stage_len):
    form = W.FORM[name]
    wide, narrow = W.LAUNCHES[name]
    assert wide[form.launch] == form.count == 1
    _exact_case(form, wide, narrow, stage_len)


@pytest.mark.gpu
@pytest.mark.parametrize("stage_len", W.LAST_K7_LENGTHS)
def test_last_k7_branch_keeps_the_pairs(cuda_device, stage_len):
    _exact_case(W.LAST_K7, W.LAST_K7_LAUNCHES, W.LAST_K7_LAUNCHES, stage_len)


@functools.lru_cache(maxsize=None)
def _dense_arms(name, stage_len):
    """(default, switch at 0) outputs of one dense case, on the CPU; the default arm with its invariants."""
    form = W.FORM[name]
    wide, narrow = W.LAUNCHES[name]
    what = f"geo32 dense {name} L={stage_len}"
    mel = W.dense_input(name, stage_len).to(DEV)
    with W.env(form, True):
        g = _generator(name, "dense", True)
        out = _profiled(g, mel, wide, what)
        _invariants(g, mel, out, what)
    with W.env(form, False):
        other = _profiled(_generator(name, "dense", False), mel, narrow, what + " switch at 0")
    return out.cpu(), other.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage_len", W.DENSE_CASES)
def test_dense(cuda_device, name, stage_len):
    what = f"geo32 dense {name} L={stage_len}"
    out, narrow = _dense_arms(name, stage_len)
    gates = tol(W.MODE)
    assert_close_fp32(out, W.dense_oracle(name, stage_len), what, **gates)
    assert_close_fp32(out, narrow.double(), what + " against the switch at 0",
                      max_abs_tol=2 * gates["max_abs_tol"], rel_rms_tol=2 * gates["rel_rms_tol"])
