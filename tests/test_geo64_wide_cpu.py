"""The inputs and constants of ``test_geo64_wide_gpu.py`` are what that test needs them to be.

Nothing here runs a kernel.  ``test_strides_match_the_library_source`` pins, word for word, the
source lines from which ``_geo64_wide`` restates the tile strides of the 64-channel f16x3 defaults
(pair S = 254 / 250 / 246 at kernels 3 / 7 / 11, 240 with ``conv_post`` fused; block S = 232), and the
dispatch lines that put the 256-column forms in front of the narrow ones.  For every (form, stage
length, seed) the exact-integer inputs must have the properties ``_mrf_exact``'s argument rests on
(bf16-exact activations, nothing negative, ``conv_post``'s argument at most 0.25), and every
element of the stage under test must reach ``conv_post`` with a weight of at least 2^-16.
"""
import os

import numpy as np
import pytest
import torch

import _geo64_wide as W
import _mrf_exact as X


def test_strides_match_the_library_source():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd", "csrc")
    text = {}
    for fname, line in W.SOURCE_LINES:
        if fname not in text:
            with open(os.path.join(csrc, fname)) as fh:
                text[fname] = fh.read()
        assert line in text[fname], f"{fname} no longer holds {line!r}: re-derive the tile strides in _geo64_wide.py"
    # the wide branches stand in front of the narrow ones they fall back to
    src = text["kernels_resblock.hip"]
    assert src.index("launch_pair_t<S, K, 64, 0, true>(a, B, s);") < src.index("else if (C == 64) launch_pair_t<S, K, 64, 1>(a, B, s);")
    assert src.index("launch_res3_wide64<S, false>(a, B, s);") < src.index("} else launch_res3_t<S, 64, 2, 3>(a, B, s);")
    assert [W.pair_stride(K)[0] for K in (3, 7, 11)] == [254, 250, 246]
    assert W.pair_stride(11, True) == (240, 8) and W.block_stride() == (232, 12)


def test_form_table():
    assert {f.launch for f in W.FORMS} == {"mrf_pair_k3_c64", "mrf_pair_k7_c64", "mrf_pair_k11_c64", "mrf_pair_post_k11_c64",
                                           "mrf_block_k3_c64"}
    for f in W.FORMS:
        assert f.channels == 64 and f.step == 2 and f.S % 2 == 0
        assert W.lengths(f) == [4, f.S - 2, f.S, f.S + 2, 2 * f.S, 3 * f.S + 6]
        assert set(W.dense_lengths(f)) <= set(W.lengths(f))
    assert [FK.cfg["resblock_kernel_sizes"] for FK in (W.FORM["block_up"], W.FORM["block_up_k7"])] == [[3], [3, 7]]


@pytest.mark.parametrize("name", [f.name for f in W.FORMS])
def test_weight_coverage_and_reach(name):
    f = W.FORM[name]
    union = X.coverage_union(f.cfg, 0, range(f.n_seeds))
    for conv, m in union.items():
        assert m.all(), f"{name} {conv}: (row block, channel group, tap) triples without a weight"
    for seed in range(f.n_seeds):
        sd = W.exact_sd(name, seed)
        for n in W.lengths(f):
            r = X.reach(f.cfg, sd, 0, n)
            assert r.shape == (64, n) and r.min().item() >= 2.0 ** -16, \
                f"{name} seed {seed} L={n}: {int((r < 2.0 ** -16).sum())} elements of the stage never reach conv_post"


@pytest.mark.parametrize("name,stage_len", W.CASES)
def test_exact_inputs(name, stage_len):
    f = W.FORM[name]
    for seed in range(f.n_seeds):
        what = f"{name} L={stage_len} seed={seed}"
        sd, mel = W.exact_sd(name, seed), W.exact_input(name, stage_len, seed)
        assert set(np.unique(mel.numpy())) <= {0.0, 1.0} and all(mel[b].any() for b in range(W.B)), what
        ref, emu, stages, arg = X.reference(f.cfg, sd, mel)
        assert ref.shape == (W.B, 1, stage_len // f.step * f.hop), what
        assert torch.equal(ref, W.exact_oracle(name, stage_len, seed)), what
        assert torch.equal(emu, ref), f"{what}: the bf16-emulated oracle differs from the fp64 oracle"
        for key, v in stages.items():
            assert v.min().item() >= 0.0, f"{what}: stage {key} goes negative"
        assert 0.0 < arg.max().item() <= X.MAX_ARG, f"{what}: conv_post argument {arg.max().item()}"
        terr = (torch.tanh(arg.float()).double() - torch.tanh(arg)).abs().max().item()
        assert terr <= X.GATE / 10, f"{what}: fp32 tanh is {terr:.2e} off, gate {X.GATE:.2e}"
        x_in, z = stages["ups.0"], stages["mrf.0"]
        assert x_in.shape == (W.B, 64, stage_len), what
        if stage_len >= 10:
            frac = (z != x_in).double().mean(dim=2)
            assert frac.min().item() > 0.5, f"{what}: a channel of the block passes its input through"
        else:
            assert all(z[b].any() for b in range(W.B)), f"{what}: an utterance's stage is all zero"
