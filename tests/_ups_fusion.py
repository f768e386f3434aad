"""Shared by ``test_ups_fusion_cpu.py`` and ``test_ups_fusion_gpu.py``: the x2 upsampler folded into
the previous stage's kernel-3 whole block (``resblock3_kernel`` with ``UP``, hifigan.cpp
``ups_fused_``).

``up_stride`` restates the tail's tile geometry from the kernel's constants the way
``_mrf_exact.block1_stride`` restates ``Res3Cfg``; ``SOURCE_LINES`` are the lines it is read from
and the CPU test pins them word for word.
"""
from __future__ import annotations

from typing import List, Tuple

import _mrf_exact as X

SWITCH = "TTS_MI355X_UPS_FUSION"


def up_stride(C: int) -> Tuple[int, int, int]:
    """(S', lead, halo) of the whole block with the upsampling tail at C channels.

    kernels_resblock.hip launch_res3_up_t: ``Res3Cfg<S, C, GEO, 3, 6, r3_xoff(3), r3_lead(3), true>``
    with GEO 4 at 128 channels and GEO 2 at 64, both 128 columns, ``grid(ceil_div(a.T, P::RP_BN))``:
    the tiles, lead (12) and stride (104) of the plain kernel-3 block.  The tail's two taps read the
    MRF mean at columns c - 1 and c, so its halo is one column, on the left; the block's valid
    columns [11, 117) hold one to spare on either side of the kept [12, 116).  Column T (the
    transposed conv's last) is emitted by the last workgroup (``mm == T && last_wg``).
    """
    assert C in (64, 128)
    S, lead = X.block1_stride(3, C)
    return S, lead, 1


# (file under tts-3_amd/csrc, text): what up_stride restates beyond _mrf_exact.SOURCE_LINES
SOURCE_LINES = (
    ("kernels_resblock.hip", "using P = Res3Cfg<S, C, GEO, 3, 6, r3_xoff(3), r3_lead(3), true>;"),
    ("kernels_resblock.hip", "dim3 grid(ceil_div(a.T, P::RP_BN), 1, B);"),
    ("kernels_resblock.hip", "if (C == 128) launch_res3_up_t<SchemeH3, 128, 4>(a, B, s);"),
    ("kernels_resblock.hip", "else launch_res3_up_t<SchemeH3, 64, 2>(a, B, s);"),
    ("kernels_resblock.hip", "return lo <= r3_lead(K) - 1 && hi >= rp_w - r3_lead(K) + 1;"),
    ("resblock_block.hpp", "const bool keep = col >= LEAD && mm <= T && (col < LEAD + P::RP_BN || (mm == T && last_wg));"),
    ("resblock_block.hpp", "conv_k(a.up_w, XO - 1, 1, std::integral_constant<int, 2>{});  // taps at X rows column - 1 + k"),
    ("resblock_block.hpp", "static constexpr int RP_W = GEO == 0 ? 256 : (GEO == 1 ? 192 : 128);"),
    ("resblock_block.hpp", "static constexpr int RP_BN = RP_W - 2 * LEAD;"),
    ("resblock_block.hpp", "constexpr int R3_LEAD = 12;"),
)

# C0 -> channels of the fused stage (stage 0); both topologies are [2, 2]
TOPOLOGIES = {256: 128, 128: 64}


def cfg(C0: int, kernels) -> dict:
    return X.topology(C0, [2, 2], list(kernels))


def edge_lengths(C: int) -> List[int]:
    """Lengths of the fused stage at the tail's tile edges.  The stage follows a x2 upsampler, so
    only even lengths are reachable from a mel: each odd length asked for (1, S' - 1, S' + 1,
    2 S' - 1, 2 S' + 1, an odd one past three tiles) is taken at the even lengths on both sides
    of it where they exist, and "one below the halo" (0 columns) as the smallest length, 2."""
    S, lead, halo = up_stride(C)
    out = {2, lead - 2, S - 2, S, S + 2, 2 * S - 2, 2 * S, 2 * S + 2, 3 * S + 10, 3 * S + 12}
    return sorted(n for n in out if n >= 2)
