"""What ``test_ups_fusion_gpu.py`` rests on, checked without a GPU: the source lines the tail's tile
stride S' is restated from still stand word for word, the edge lengths straddle the tile edges, and
the exact-integer inputs make the upsampler behind the fused stage a selection of whole values (so
the per-tile operand scale of the fused arm and the per-utterance one of the unfused arm give the
same bits)."""
import os

import numpy as np
import pytest

import _mrf_exact as X
import _ups_fusion as U


def test_tail_stride_matches_the_library_source():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd", "csrc")
    text = {}
    for fname, line in U.SOURCE_LINES:
        if fname not in text:
            with open(os.path.join(csrc, fname)) as fh:
                text[fname] = fh.read()
        assert line in text[fname], f"{fname} no longer holds {line!r}: re-derive the tail's stride in _ups_fusion.py"


@pytest.mark.parametrize("C", sorted(U.TOPOLOGIES.values()))
def test_edge_lengths(C):
    S, lead, halo = U.up_stride(C)
    assert (S, lead, halo) == (104, 12, 1)
    ls = U.edge_lengths(C)
    assert all(n % 2 == 0 for n in ls), "the fused stage follows a x2 upsampler"
    assert ls[0] == 2 and any(n < lead for n in ls[1:])
    for k in (1, 2):  # the even lengths on both sides of k S' - 1 and k S' + 1, and k S' itself
        assert {k * S - 2, k * S, k * S + 2} <= set(ls)
    assert ls[-1] > 3 * S and ls[-1] % S not in (0, S - 1)


@pytest.mark.parametrize("C0", sorted(U.TOPOLOGIES))
@pytest.mark.parametrize("kernels", [(3,), (3, 7)])
def test_exact_upsampler_is_a_selection(C0, kernels):
    """ups.1, the layer the block applies, has one nonzero (a 1) per output row and phase and reads
    every input channel: each of its outputs is one whole value of the MRF mean."""
    cfg = U.cfg(C0, kernels)
    sd = X.exact_state_dict(cfg, 0, 0)
    w = sd["ups.1.weight"].numpy()  # [cin][cout][4]
    assert set(np.unique(w)) == {0.0, 1.0}
    per_phase = [(w[:, :, [r, r + 2]] != 0).sum(axis=(0, 2)) for r in range(2)]
    assert all((p == 1).all() for p in per_phase)
    assert (w != 0).any(axis=(1, 2)).all()
    assert float(sd["conv_post.weight"].max()) == 2.0 ** -16
