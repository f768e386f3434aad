"""The whole kernel-3 ResBlock1 at 128 channels (``mrf_block_k3_c128``, resblock3_kernel) on its own.

A small generator whose first MRF stage is that block: conv_pre to 256 channels, one x2 upsampler
(kernel 4) to 128 channels, ``resblock_kernel_sizes [3]`` with dilations ``[1, 3, 5]``, so that
stage's length is twice the mel length.  conv_post takes at most 64 input channels, so a second x2
upsampler and a 64-channel stage (the long-tested ``mrf_block_k3_c64``) follow before it; the
waveform is four mel lengths long.  The kernel's tile keeps 104 of 128 columns and leads by 12,
and the lengths of the 128-channel stage cover: shorter than the lead (2), one partial tile (16), a tile that ends two
columns short (102), exactly one tile (104), a second tile that keeps 2 columns (106), four tiles
with a ragged last one (314).  A second topology ``[7, 3]`` makes the block the last MRF branch,
so its epilogue adds the running z and divides (zmode 3).

Checked in f16x3 (two workgroups per CU on swizzled 64-byte LDS rows) and bf16: the fp64 oracle
under the per-mode gates of ``_util.tol``, batch invariance (rows of a B = 3 run bitwise equal to
B = 1 runs) and determinism (two B = 3 runs bitwise equal: with co-resident workgroups the test
that catches a shared-LDS or reduction-slot mistake).  The non-GPU test holds the oracle itself,
run in fp32, to the fp32 gates on the same inputs, so the inputs are known to be well conditioned.
"""
import functools

import numpy as np
import pytest
import torch

from _util import assert_close_fp32, tol
from oracle import hifigan_ref
from tts_amd import synthetic
from tts_amd.vocoder import HifiganGenerator

B = 3
STAGE_LENGTHS = (2, 16, 102, 104, 106, 314)  # 128-channel samples; the mel is half as long
MODES = ("f16x3", "bf16")


def _cfg(kernels):
    return dict(in_channels=80, out_channels=1, resblock_type="1",
                resblock_dilation_sizes=[[1, 3, 5]] * len(kernels), resblock_kernel_sizes=list(kernels),
                upsample_kernel_sizes=[4, 4], upsample_initial_channel=256, upsample_factors=[2, 2],
                inference_padding=5)


TOPOLOGIES = {"k3": _cfg([3]), "k7_k3": _cfg([7, 3])}
CASES = [("k3", n) for n in STAGE_LENGTHS] + [("k7_k3", 106), ("k7_k3", 314)]


@functools.lru_cache(maxsize=None)
def _state_dict(topo):
    return synthetic.hifigan_state_dict(**TOPOLOGIES[topo], seed=128 + len(topo), weight_norm=False)


@functools.lru_cache(maxsize=None)
def _mel(stage_len):
    assert stage_len % 2 == 0
    return synthetic.mel(B, stage_len // 2, seed=stage_len)


@functools.lru_cache(maxsize=None)
def _oracle(topo, stage_len):
    """fp64 reference of the B = 3 forward, computed once per case and shared by the tests."""
    ref = hifigan_ref.hifigan_forward(_state_dict(topo), _mel(stage_len), pad=0, dtype=torch.float64,
                                      **TOPOLOGIES[topo])
    ref.requires_grad_(False)
    return ref


@functools.lru_cache(maxsize=None)
def _generator(topo, mode, dev):
    g = HifiganGenerator(**TOPOLOGIES[topo], math_mode=mode)
    g.remove_weight_norm()
    g.load_state_dict(_state_dict(topo))
    g.eval()
    return g.to(dev)


@pytest.mark.parametrize("topo,stage_len", CASES)
def test_oracle_fp32_inside_gates(topo, stage_len):
    """The reference's own fp32 forward against its fp64 forward stays inside the fp32 gates."""
    ref = _oracle(topo, stage_len)
    assert ref.shape == (B, 1, 2 * stage_len)
    out = hifigan_ref.hifigan_forward(_state_dict(topo), _mel(stage_len), pad=0, dtype=torch.float32,
                                      **TOPOLOGIES[topo])
    assert_close_fp32(out, ref, f"oracle fp32 {topo} L={stage_len}", **tol("f16x3"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("topo,stage_len", CASES)
def test_block_vs_oracle(cuda_device, topo, stage_len, mode):
    g = _generator(topo, mode, cuda_device)
    mel = _mel(stage_len).to(cuda_device)
    out, rows = g.profile(mel, pad=0)
    names = [r["name"] for r in rows]
    assert names.count("mrf_block_k3_c128") == 1, names  # the whole block, in one launch
    assert_close_fp32(out.cpu(), _oracle(topo, stage_len), f"{mode} {topo} L={stage_len}", **tol(mode))
    assert torch.equal(g(mel), out), "profiled and plain forward differ"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("topo,stage_len", CASES)
def test_block_batch_invariant(cuda_device, topo, stage_len, mode):
    g = _generator(topo, mode, cuda_device)
    mel = _mel(stage_len).to(cuda_device)
    full = g(mel).cpu().numpy()
    for row in range(B):
        one = g(mel[row:row + 1]).cpu().numpy()
        assert np.array_equal(one[0], full[row]), f"{mode} {topo} L={stage_len}: row {row} depends on the batch"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("topo,stage_len", CASES)
def test_block_deterministic(cuda_device, topo, stage_len, mode):
    g = _generator(topo, mode, cuda_device)
    mel = _mel(stage_len).to(cuda_device)
    first = g(mel).cpu().numpy()
    second = g(mel).cpu().numpy()
    assert np.isfinite(first).all()
    assert np.array_equal(first, second), f"{mode} {topo} L={stage_len}: two runs differ"
