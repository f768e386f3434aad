"""The x2 upsampler folded into the previous stage's kernel-3 whole block (f16x3).

Two small generators, ``upsample_initial_channel`` 256 and 128 with factors ``[2, 2]``: stage 0 (128
or 64 channels) is the fused stage, its ``mrf_block_k3_c{C}`` launch runs last in the stage, forms
the MRF mean in registers and applies ``ups.1`` to it, so no ``ups_u2_c{C/2}`` launch follows.
``TTS_MI355X_UPS_FUSION=0`` (read when a generator's handle is created) keeps the separate launches
and is the reference arm.  Kernels ``[3]`` (one branch, the mean is the block's x) and ``[3, 7, 11]``
(the block after two other branches, ((r0 + r1) + r2) / 3).

* dense weights: the fp64 oracle under ``tol("f16x3")`` and the unfused arm under twice its
  max-abs gate (the rule of ``test_whole_block_fusion_matches_unfused``), at three tiles and a
  ragged fourth; B = 3;
* exact integers (``_mrf_exact``: 0 / 1 weights and mel, ``conv_post`` = 2^-16, the upsampler a
  selection): the fused arm equals the unfused arm bit for bit at every tile edge of the tail
  (``_ups_fusion.edge_lengths``; the stage follows a x2 layer, so odd lengths are taken at their
  even neighbours).  ``_mrf_exact`` builds exact means for 1, 2 or 4 kernels only (a division by 3
  is not exact, and then the two arms' operand scales round differently), so the exact arm runs
  ``[3]`` and the two-branch ``[3, 7]``, the latter with the direct kernel-7 convs
  (``TTS_MI355X_WINO=0``: Winograd's transforms are not exact either);
* batch invariance and run-to-run determinism, ``torch.equal``;
* B = 1, a stream per branch: bitwise the profiled one-stream forward;
* launch names with the switch on and off; the workspace does not grow after ``reserve``;
* the XTTS topology (``cond_in_each_up_layer``) and bf16 generators keep their upsampler launches.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import _mrf_exact as X
import _ups_fusion as U
from _util import assert_close_fp32, goldens, max_abs, tol
from oracle import hifigan_ref
from tts_amd import _native as N
from tts_amd import synthetic
from tts_amd.tts import HifiDecoder
from tts_amd.vocoder import HifiganGenerator

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MODE = "f16x3"
B = X.B
KERNELS = ((3,), (3, 7, 11))
EXACT_KERNELS = ((3,), (3, 7))
DENSE_T = 161  # mel frames: the fused stage runs 322 columns, three tiles of 104 and a ragged fourth
EXACT = [(C0, k, n) for C0 in sorted(U.TOPOLOGIES) for k in EXACT_KERNELS for n in U.edge_lengths(U.TOPOLOGIES[C0])]


@contextlib.contextmanager
def _env(**kv):
    """Switches for the length of the block, every other one of ``_mrf_exact`` cleared."""
    keys = tuple(X.ENV_SWITCHES) + (U.SWITCH, "TTS_MI355X_MRF_STREAMS", "TTS_MI355X_SUBBATCH")
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update({k: v for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _dense_sd(C0, kernels):
    return synthetic.hifigan_state_dict(**U.cfg(C0, kernels), seed=500 + C0 + len(kernels), weight_norm=False)


@functools.lru_cache(maxsize=None)
def _dense_mel():
    return synthetic.mel(B, DENSE_T, seed=77)


@functools.lru_cache(maxsize=None)
def _dense_oracle(C0, kernels):
    with torch.no_grad():
        return hifigan_ref.hifigan_forward(_dense_sd(C0, kernels), _dense_mel(), pad=0, dtype=torch.float64,
                                           **U.cfg(C0, kernels))


@functools.lru_cache(maxsize=None)
def _generator(C0, kernels, fused, weights, mode=MODE):
    """``weights``: "dense", or a seed of the exact arm.  The handle is created here, under the
    arm's switches."""
    g = HifiganGenerator(**U.cfg(C0, kernels), math_mode=mode)
    g.remove_weight_norm()
    g.load_state_dict(_dense_sd(C0, kernels) if weights == "dense" else X.exact_state_dict(U.cfg(C0, kernels), 0, weights))
    g.eval()
    g = g.to(DEV)
    with _env(**{U.SWITCH: "1" if fused else "0", "TTS_MI355X_WINO": None if weights == "dense" else "0"}):
        g._native_handle()
    return g


def _names(rows):
    return [r["name"] for r in rows]


def _check_names(names, C0, fused):
    C = U.TOPOLOGIES[C0]
    assert names.count(f"mrf_block_k3_c{C}") == 1, names
    assert names.count(f"ups_u2_c{C}") == 1, names  # the first upsampler has no stage in front of it
    assert names.count(f"ups_u2_c{C // 2}") == (0 if fused else 1), names


@pytest.mark.parametrize("kernels", KERNELS)
@pytest.mark.parametrize("C0", sorted(U.TOPOLOGIES))
def test_vs_oracle_and_unfused(cuda_device, C0, kernels):
    mel = _dense_mel().to(DEV)
    outs = {}
    for fused in (True, False):
        g = _generator(C0, kernels, fused, "dense")
        out, rows = g.profile(mel, pad=0)
        _check_names(_names(rows), C0, fused)
        assert torch.equal(g(mel), out), f"fused={fused}: profiled and plain forward differ"
        outs[fused] = out.cpu()
        ma, rr = assert_close_fp32(outs[fused], _dense_oracle(C0, kernels), f"ups fusion C0={C0} {kernels} fused={fused}",
                                   **tol(MODE))
        print(f"C0={C0} kernels={kernels} fused={fused}: max|d|={ma:.3e} rel-RMS={rr:.3e}")
    d = max_abs(outs[True].numpy(), outs[False].numpy())
    print(f"C0={C0} kernels={kernels}: fused vs unfused max|d|={d:.3e}")
    assert d <= 2 * tol(MODE)["max_abs_tol"], f"fused vs unfused: max|d| = {d:.3e}"


@pytest.mark.parametrize("C0,kernels,stage_len", EXACT)
def test_exact_fused_equals_unfused(cuda_device, C0, kernels, stage_len):
    cfg = U.cfg(C0, kernels)
    n_seeds = max(-(-(U.TOPOLOGIES[C0] // 16) * k // 32) for k in kernels)
    for seed in range(n_seeds):
        mel = X.exact_mel(B, stage_len // 2, seed + 17 * stage_len).to(DEV)
        outs = {}
        for fused in (True, False):
            g = _generator(C0, kernels, fused, seed)
            out, rows = g.profile(mel, pad=0)
            names = _names(rows)
            _check_names(names, C0, fused)
            assert not [n for n in names if n.startswith("mrf_wino")], names
            outs[fused] = out.cpu()
        what = f"exact C0={C0} {kernels} L={stage_len} seed={seed}"
        with torch.no_grad():
            ref = hifigan_ref.hifigan_forward(X.exact_state_dict(cfg, 0, seed), mel.cpu(), pad=0, dtype=torch.float64, **cfg)
        err = max_abs(outs[True].numpy(), ref.numpy())
        assert err <= X.GATE, f"{what}: max|fused - oracle| = {err:.3e}, gate {X.GATE:.3e}"
        n = int((outs[True] != outs[False]).sum())
        assert n == 0, f"{what}: fused and unfused differ at {n} samples"


@pytest.mark.parametrize("kernels", KERNELS)
@pytest.mark.parametrize("C0", sorted(U.TOPOLOGIES))
def test_batch_invariant_and_deterministic(cuda_device, C0, kernels):
    g = _generator(C0, kernels, True, "dense")
    mel = _dense_mel().to(DEV)
    full = g(mel)
    assert torch.isfinite(full).all()
    assert torch.equal(g(mel), full), "two runs differ"
    for row in range(B):
        assert torch.equal(g(mel[row:row + 1])[0], full[row]), f"row {row} depends on the batch"


@pytest.mark.parametrize("C0", sorted(U.TOPOLOGIES))
def test_stream_per_branch_bitwise(cuda_device, C0):
    """B = 1 runs one lane with a stream per MRF branch: the block waits for the other branches'
    events and the next stage for the block.  Bitwise the profiled forward, which is one stream."""
    g = _generator(C0, (3, 7, 11), True, "dense")
    mel = _dense_mel()[:1].to(DEV)
    out, rows = g.profile(mel, pad=0)
    _check_names(_names(rows), C0, True)
    for _ in range(3):
        assert torch.equal(g(mel), out)


@pytest.mark.parametrize("C0", sorted(U.TOPOLOGIES))
def test_workspace_does_not_grow_after_reserve(cuda_device, C0):
    """The fused schedule takes no more planes than the unfused one, and a forward after
    ``reserve`` allocates nothing: free device memory stays within a fraction of one activation
    plane (6.3 / 12.6 MB at these shapes; the workspace can only grow by whole planes)."""
    kernels, T = (3, 7, 11), 4096
    lib = N.lib()
    sizes = {}
    for fused in (True, False):
        g = _generator(C0, kernels, fused, "dense")
        sizes[fused] = lib.tts_hifigan_workspace_bytes(g._native_handle(), B, T, 0)
    assert sizes[True] == sizes[False] > 0, sizes
    g = _generator(C0, kernels, True, "dense")
    mel = synthetic.mel(B, T, seed=5).to(DEV)
    g(mel[:, :, :8])  # streams and events exist, torch's allocator has served a small output
    warm = torch.empty(B, 1, 4 * T, device=DEV)
    del warm  # the output buffer of the call below comes from torch's cache
    g.reserve(B, T, 0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(DEV)[0]
    out = g(mel)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(DEV)[0]
    plane = 4 * B * C0 * T
    assert torch.isfinite(out).all()
    assert free0 - free1 < plane // 4, f"free memory fell by {free0 - free1} bytes during the call (a plane is {plane})"


def test_fallbacks_keep_their_upsamplers(cuda_device):
    # XTTS: conds[i](g) is added to every upsampler's output, which the tail does not do
    name, meta, arr = goldens("xtts_decoder")[0]
    with _env():
        d = HifiDecoder(math_mode=MODE)
        d.waveform_decoder.load_state_dict(synthetic.hifigan_state_dict(**meta["config"], seed=meta["seed"], weight_norm=True))
        d.eval()
        d = d.to(DEV)
        z = torch.from_numpy(arr["z_ref_fp32"]).to(DEV)
        _, rows = d.waveform_decoder.profile(z, pad=0, g=torch.from_numpy(arr["g"]).to(DEV))
    names = _names(rows)
    assert names.count("ups_u2_c64") == 1 and names.count("ups_u2_c32") == 1, names
    # bf16: fp32 planes behind a x2 first layer, bf16 planes behind a x8 one
    for factors in ([2, 2], [8, 2]):
        cfg = X.topology(256, factors, [3])
        with _env():
            g = HifiganGenerator(**cfg, math_mode="bf16")
            g.remove_weight_norm()
            g.load_state_dict(synthetic.hifigan_state_dict(**cfg, seed=9, weight_norm=False))
            g = g.eval().to(DEV)
            _, rows = g.profile(synthetic.mel(2, 8, seed=1).to(DEV), pad=0)
        names = _names(rows)
        assert names.count("ups_u2_c64") == 1 and names.count("mrf_block_k3_c128") == 1, names
