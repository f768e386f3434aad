"""The inputs and constants of ``test_geo32_wide_gpu.py`` are what that test needs them to be.

Nothing here runs a kernel.  ``test_strides_match_the_library_source`` pins, word for word, the
source lines from which ``_geo32_wide`` restates the tile strides of the 32-channel f16x3 whole
block (S = 440 / 392 at kernels 7 / 11) and the dispatch lines that put the 512-column
forms in front of the 256-column ones and make a kernel-7 branch a whole block where a later branch
follows; the older tables of library lines (``_mrf_exact``, ``_geo64_wide``, ``_ups_fusion``) must
still hold beside them.  For every (form, stage length, seed) the exact-integer inputs must have
the properties ``_mrf_exact``'s argument rests on (bf16-exact activations, nothing negative,
``conv_post``'s argument at most 0.25), and every element of the stage under test must reach
``conv_post`` with a weight of at least 2^-16.
"""
import os

import numpy as np
import pytest
import torch

import _geo32_wide as W
import _geo64_wide as W64
import _mrf_exact as X
import _ups_fusion as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd", "csrc")


def _source(fname, cache={}):
    if fname not in cache:
        with open(os.path.join(CSRC, fname)) as fh:
            cache[fname] = fh.read()
    return cache[fname]


def test_strides_match_the_library_source():
    for fname, line in W.SOURCE_LINES:
        assert line in _source(fname), f"{fname} no longer holds {line!r}: re-derive the tile strides in _geo32_wide.py"
    # the 512-column branches stand in front of the 256-column lines they fall back to
    src = _source("kernels_resblock.hip")
    new = src.index("if (C == 32 && (K == 7 || K == 11) && (wide64 & kWide32Block) && a.planes == 0) {")
    for old in ("if (C == 32) launch_res3_t<S, 32, 0, 7>(a, B, s);", "if (C == 32) launch_res3_t<S, 32, 0, 11>(a, B, s);"):
        assert new < src.index(old), old
    # the strides, from Res3Cfg's GEO 5: RP_W = 512, RP_BN = RP_W - 2 r3_lead(K), r3_lead(K) = 12 (K - 1) / 2
    hpp = _source("resblock_block.hpp")
    geo5 = hpp[hpp.index("struct Res3Cfg<S, C, 5, K, NCV, XO, LEAD, UP, SW> {"):]
    geo5 = geo5[:geo5.index("};")]
    assert "static constexpr int RP_W = 512;" in geo5 and "static constexpr int RP_BN = RP_W - 2 * LEAD;" in geo5
    assert [W.block_stride(K) for K in (7, 11)] == [(440, 36), (392, 60)]
    # LDS of the two instances: 2 groups x (512 + 2 XO) rows x 64 B, XO = 5 (K - 1) / 2, under 80 KB
    lds = [2 * (512 + 2 * 5 * ((K - 1) // 2)) * 64 for K in (7, 11)]
    assert lds == [69376, 71936] and all(b + 32 + 6 * 32 * 4 <= 80 * 1024 for b in lds)


@pytest.mark.parametrize("table", [X, W64, U], ids=["mrf_exact", "geo64_wide", "ups_fusion"])
def test_older_source_tables_still_hold(table):
    for fname, line in table.SOURCE_LINES:
        assert line in _source(fname), f"{fname} no longer holds {line!r} ({table.__name__}.SOURCE_LINES)"


def test_form_table():
    assert [f.launch for f in W.FORMS] == ["mrf_block_k7_c32", "mrf_block_k7_c32", "mrf_block_k11_c32"]
    assert [f.S for f in W.FORMS] == [440, 440, 392]
    for f in W.FORMS:
        assert f.channels == 32 and f.step == 2 and f.S % 2 == 0 and f.n_seeds == 1
        assert W.lengths(f) == [4, f.S - 2, f.S, f.S + 2, 2 * f.S, 3 * f.S + 6] and max(W.lengths(f)) <= 1326
        assert set(W.dense_lengths(f)) <= set(W.lengths(f))
        wide, narrow = W.LAUNCHES[f.name]
        assert wide[f.launch] == 1 and set(wide) == set(narrow)
    assert [W.FORM[n].cfg["resblock_kernel_sizes"] for n in ("block_k7_first", "block_k7_mid")] == [[7, 3], [3, 7, 11, 3]]
    assert dict(W.FORM["block_k11"].env) == {"TTS_MI355X_RB1_WHOLE_K": "7,11"}
    # with the switch at 0 the kernel-7 branch is the three pair launches again
    for n in ("block_k7_first", "block_k7_mid"):
        assert W.LAUNCHES[n][1]["mrf_block_k7_c32"] == 0 and W.LAUNCHES[n][1]["mrf_pair_k7_c32"] == 3
    # the dispatch case is _mrf_exact's pair_post_k7_c32 topology and launch
    assert W.LAST_K7.cfg == X.FORM["pair_post_k7_c32"].cfg and W.LAST_K7.launch == X.FORM["pair_post_k7_c32"].launch
    assert W.LAST_K7_LAUNCHES["mrf_block_k7_c32"] == 0


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
            assert r.shape == (32, n) and r.min().item() >= 2.0 ** -16, \
                f"{name} seed {seed} L={n}: {int((r < 2.0 ** -16).sum())} elements of the stage never reach conv_post"


@pytest.mark.parametrize("name,stage_len", W.CASES + [("last_k7", n) for n in W.LAST_K7_LENGTHS])
def test_exact_inputs(name, stage_len):
    f = W.ALL_FORM[name]
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
        assert x_in.shape == (W.B, 32, stage_len), what
        if stage_len >= 10:
            frac = (z != x_in).double().mean(dim=2)
            assert frac.min().item() > 0.5, f"{what}: a channel of the block passes its input through"
        else:
            assert all(z[b].any() for b in range(W.B)), f"{what}: an utterance's stage is all zero"
