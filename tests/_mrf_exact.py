"""Exact-integer inputs for the fused MRF kernels, and the table of their forms.

The fused ResBlock kernels (the pair kernel of ``kernels_resblock.hip``, the whole-block ResBlock1 /
ResBlock2 kernel of ``resblock_block.hpp``) have no op entry point: the suite reaches them through
whole generators.  This module builds generators whose every activation is a small non-negative
multiple of a power of two, so that every math mode that takes a fused form (fp32x6, f16x3, bf16;
the plain fp32 mode is not a split mode and runs every conv as its own launch) must reproduce
``conv_post``'s argument bit for bit:

* every weight is 0 or 1 and sparse, every bias 0, the mel 0 / 1, ``conv_post`` the constant 2^-16;
* activations are then >= 0 (leaky-ReLU is the identity) and carry at most 8 significant bits, so
  the bf16 operand, the fp16 hi / lo split, the three-piece bf16 split and every fp32 partial sum
  are exact whatever the order of the sum; the only inexact step on the device is ``tanhf``;
* inside the block under test every value is an integer, so one wrong, missing or doubled element
  there is off by at least 1, by at least 1 / ``num_kernels`` after the MRF mean, and, carried by
  weights of 1 to ``conv_post``, moves its argument by at least 2^-16 / num_kernels >= 2^-18.  The
  gate is an eighth of 2^-16 times tanh's smallest slope: half of that smallest step at four
  kernels, an eighth of it at one.

``exact_state_dict`` makes only the MRF stage under test grow: ResBlock1 about doubles a value per
iteration, and two growing stages would pass 8 significant bits.  The other stages' resblock convs
hold a single nonzero weight each, and the upsamplers behind the stage under test are selections
(one nonzero per output row and phase).  ``num_kernels`` is 1, 2 or 4 (3 would divide by 3).

In the block under test the nonzeros are placed by a rule, not drawn: row ``i`` of 32-row block
``rb`` takes, for seed ``s``, entry ``(i + 32 s + 5 rb) mod (G K)`` of a fixed permutation of the
block's (16-channel group, tap) pairs.  ``n_seeds`` = ceil(G K / 32) consecutive seeds therefore put
a nonzero into every (32-row block, 16-channel group, tap) triple of every conv, which is the unit
the kernels' weight packing and staging are indexed by; ``coverage_union`` returns the union of the
masks for the CPU test that asserts it.

``FORMS`` lists the default geometry of every fused form with the tile stride S (kept columns per
workgroup, in columns of the stage under test) derived from the kernels' own constants; the source
line each figure comes from is quoted beside the function that derives it.

Out of scope:

* geometries chosen by environment variables that the library caches in a function-local
  ``static`` (``TTS_MI355X_PAIR_GEO64``, ``TTS_MI355X_PAIR128_GEO``, ``TTS_MI355X_PAIR256_GEO``):
  they cannot be switched inside one test process;
* Winograd launches: their transforms are not exact and the op tests sweep their edges.  No
  topology below runs one in any stage (the wide kernel-7 / 11 convs appear in the bf16 mode only,
  where they are direct pairs); every GPU test asserts from the profile that no ``mrf_wino_*`` ran;
* the plain ``fp32`` math mode: it takes none of the fused forms;
* errors that only move a value to another channel at the same time step, where the stage under
  test is the last one (every 32 / 64-channel form): the constant ``conv_post`` sums over all
  channels and seven taps, so its argument does not change.  Where a stage follows (the 128 / 256
  channel forms) the upsampler behind the stage sends each channel to its own row and phase.

Every element of the stage under test does reach the waveform: ``reach`` returns the weight with
which it enters ``conv_post``'s argument, and the CPU test asserts that none is zero.
"""
from __future__ import annotations

import functools
import math
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import hifigan_ref
from tts_amd import synthetic

B = 3
MODES3 = ("fp32x6", "f16x3", "bf16")
# an eighth of the smallest change a unit error can cause: 2^-16 in conv_post's argument, times
# tanh's slope at the largest argument the CPU test admits (0.25)
MAX_ARG = 0.25
GATE = 2.0 ** -16 * (1.0 - math.tanh(MAX_ARG) ** 2) / 8.0
# every switch the forms use, cleared before a form sets its own (read when a generator's handle is
# created, hifigan.cpp Hifigan::Hifigan)
ENV_SWITCHES = ("TTS_MI355X_RESBLOCK3", "TTS_MI355X_RB1_WHOLE_K", "TTS_MI355X_RB2_ALL", "TTS_MI355X_RB2_GEO64",
                "TTS_MI355X_POST_FUSION", "TTS_MI355X_WINO", "TTS_MI355X_NO_PAIR_FUSION", "TTS_MI355X_BF16_PLANES",
                "TTS_MI355X_PAIR128", "TTS_MI355X_PAIR256", "TTS_MI355X_PAIR256_K11", "TTS_MI355X_WINO_K3",
                "TTS_MI355X_WINO_BF16", "TTS_MI355X_WINDOW_FRAMES")


# ---------------------------------------------------------------------------------------------
# Tile strides, from the kernels' constants
# ---------------------------------------------------------------------------------------------
def pair_stride(K: int, C: int, post: bool = False) -> Tuple[int, int]:
    """(S, halo) of ``resblock_pair_kernel``.

    kernels_resblock.hip PairCfg:
      ``RP_W = (GEO == 0 || GEO == 4 || GEO == 5 || GEO == 7) ? 256 : (GEO == 1 ? 192 : 128)``
      ``LEAD = (K - 1) / 2``, ``RP_BN = RP_W - 2 * LEAD``
      ``STRIDE = POST ? RP_BN - 2 * kPostHalo : RP_BN`` with ``kPostHalo = 3``
    launch_pair_k (defaults): ``C == 32 -> launch_pair_t<S, K, 32, 0>``, ``C == 64 ->
    launch_pair_t<S, K, 64, 1>``, bf16 ``C == 128 -> GEO 7``, bf16 ``C == 256 -> GEO 8``.
    """
    rp_w = {32: 256, 64: 192, 128: 256, 256: 128}[C]
    lead = (K - 1) // 2
    rp_bn = rp_w - 2 * lead
    return (rp_bn - 6, lead + 3) if post else (rp_bn, lead)


def block1_stride(K: int, C: int) -> Tuple[int, int]:
    """(S, lead) of the whole ResBlock1 (``resblock3_kernel``, NCV = 6).

    resblock_block.hpp Res3Cfg: ``RP_W = GEO == 0 ? 256 : (GEO == 1 ? 192 : 128)``,
    ``RP_BN = RP_W - 2 * LEAD``; ``R3_LEAD = 12``, ``r3_lead(K) = R3_LEAD * ((K - 1) / 2)``.
    kernels_resblock.hip launch_res3_s: K 7 / 11 ``launch_res3_t<S, C, 0, K>`` (256 columns);
    K 3: ``C == 32 -> GEO 0``, ``C == 128 -> GEO 4`` (two-piece scheme) ``/ GEO 3``, else
    ``launch_res3_t<S, 64, 2, 3>`` (128 columns).
    """
    rp_w = 256 if (K != 3 or C == 32) else 128
    lead = 12 * ((K - 1) // 2)
    return rp_w - 2 * lead, lead


def block2_stride(K: int, C: int, geo64: int) -> Tuple[int, int]:
    """(S, lead) of the whole ResBlock2 (``resblock3_kernel``, NCV = 2).

    resblock_block.hpp: ``rb2_halo(K) = K == 3 ? 4 : (K == 5 ? 12 : (K == 7 ? 9 : 15))``,
    launch_rb2_t: ``Res3Cfg<S, C, GEO, K, 2, H, H>`` (LEAD = H), ``grid(ceil_div(a.T, P::RP_BN))``;
    launch_rb2_s: ``C == 32 -> GEO 0`` (256), ``C == 64 -> geo64 == 1 ? GEO 1 (192) : GEO 2 (128)``,
    C = 128 ``GEO 3`` (128).
    """
    rp_w = 256 if C == 32 else (192 if (C == 64 and geo64 == 1) else 128)
    lead = {3: 4, 5: 12, 7: 9, 11: 15}[K]
    return rp_w - 2 * lead, lead


# The lines of the library that the three functions above restate, (file under tts-3_amd/csrc,
# text).  The CPU test asserts that each still stands there word for word: a changed default
# geometry fails it, instead of silently moving the lengths below off the tile edges.
SOURCE_LINES = (
    ("kernels_resblock.hip", "static constexpr int RP_W = (GEO == 0 || GEO == 4 || GEO == 5 || GEO == 7) ? 256 : (GEO == 1 ? 192 : 128);"),
    ("kernels_resblock.hip", "static constexpr int LEAD = (K - 1) / 2;"),
    ("kernels_resblock.hip", "static constexpr int RP_BN = RP_W - 2 * LEAD;"),
    ("kernels_resblock.hip", "static constexpr int STRIDE = POST ? RP_BN - 2 * kPostHalo : RP_BN;"),
    ("kernels_resblock.hip", "constexpr int kPostHalo = 3;"),
    ("kernels_resblock.hip", "dim3 grid(ceil_div(a.c1.Tout, P::STRIDE), 1, B);"),
    ("kernels_resblock.hip", "dim3 grid(ceil_div(a.c1.Tout, P::RP_BN), 1, B);"),
    ("kernels_resblock.hip", "return e && e[0] == '2' ? 2 : (e && e[0] == '0' ? 0 : (e && e[0] == '4' ? 4 : (e && e[0] == '5' ? 5 : 7)));"),
    ("kernels_resblock.hip", "return e && e[0] == '2' ? 2 : (e && e[0] == '6' ? 6 : 8);"),
    ("kernels_resblock.hip", "if (C == 32) launch_pair_t<S, K, 32, 0>(a, B, s);"),
    ("kernels_resblock.hip", "else if (C == 64) launch_pair_t<S, K, 64, 1>(a, B, s);"),
    ("kernels_resblock.hip", "return e && std::atoi(e) == 2 ? 2 : (e && std::atoi(e) == 4 ? 4 : 1);"),
    ("kernels_resblock.hip", "using P = Res3Cfg<S, C, GEO, K, 6, r3_xoff(K), r3_lead(K)>;"),
    ("kernels_resblock.hip", "if (C == 32) launch_res3_t<S, 32, 0, 7>(a, B, s);"),
    ("kernels_resblock.hip", "else launch_res3_t<S, 64, 0, 7>(a, B, s);"),
    ("kernels_resblock.hip", "if (C == 32) launch_res3_t<S, 32, 0, 11>(a, B, s);"),
    ("kernels_resblock.hip", "else launch_res3_t<S, 64, 0, 11>(a, B, s);"),
    ("kernels_resblock.hip", "if (C == 32) launch_res3_t<S, 32, 0, 3>(a, B, s);"),
    ("kernels_resblock.hip", "if constexpr (S::NP == 2) launch_res3_t<S, 128, 4, 3>(a, B, s);"),
    ("kernels_resblock.hip", "else if constexpr (S::ROWB <= 80) launch_res3_t<S, 128, 3, 3>(a, B, s);"),
    ("kernels_resblock.hip", "} else launch_res3_t<S, 64, 2, 3>(a, B, s);"),
    ("resblock_block.hpp", "static constexpr int RP_W = GEO == 0 ? 256 : (GEO == 1 ? 192 : 128);"),
    ("resblock_block.hpp", "static constexpr int RP_BN = RP_W - 2 * LEAD;"),
    ("resblock_block.hpp", "constexpr int R3_LEAD = 12;"),
    ("resblock_block.hpp", "constexpr int r3_lead(int K) { return R3_LEAD * ((K - 1) / 2); }"),
    ("resblock_block.hpp", "constexpr int rb2_halo(int K) { return K == 3 ? 4 : (K == 5 ? 12 : (K == 7 ? 9 : 15)); }"),
    ("resblock_block.hpp", "using P = Res3Cfg<S, C, GEO, K, 2, H, H>;"),
    ("resblock_block.hpp", "dim3 grid(ceil_div(a.T, P::RP_BN), 1, B);"),
    ("resblock_block.hpp", "if (C == 32) launch_rb2_k<S, 32, 0>(a, B, K, s);"),
    ("resblock_block.hpp", "if (geo64 == 1) launch_rb2_k<S, 64, 1>(a, B, K, s);"),
    ("resblock_block.hpp", "else launch_rb2_k<S, 64, 2>(a, B, K, s);"),
    ("resblock_block.hpp", "if (K == 3) launch_rb2_t<S, 128, 3, 3>(a, B, s);"),
    ("resblock_block.hpp", "else launch_rb2_t<S, 128, 3, 5>(a, B, s);"),
)


# ---------------------------------------------------------------------------------------------
# Forms
# ---------------------------------------------------------------------------------------------
def topology(C0: int, factors: Sequence[int], kernels: Sequence[int], rtype: str = "1", dil=None) -> dict:
    if dil is None:
        dil = [[1, 3, 5]] * len(kernels) if rtype == "1" else [[1, 3]] * len(kernels)
    return dict(in_channels=80, out_channels=1, resblock_type=rtype,
                resblock_dilation_sizes=[list(d) for d in dil], resblock_kernel_sizes=list(kernels),
                upsample_kernel_sizes=[2 * u for u in factors], upsample_initial_channel=C0,
                upsample_factors=list(factors), inference_padding=5)


@dataclass(frozen=True)
class Form:
    name: str
    cfg: dict = field(hash=False, compare=False)
    stage: int            # the MRF stage under test
    env: tuple            # ((switch, value), ...) set while the generator is built and run
    launch: str           # profiled launch name of the form
    count: int            # and how often one forward runs it
    modes: tuple          # the math modes that take the form
    S: int                # tile stride, columns of the stage under test
    lead: int             # the form's lead / halo per side
    dense: bool = False   # part of the dense-weight arm (forms that exist only in the bf16 scheme)

    @property
    def channels(self) -> int:
        return self.cfg["upsample_initial_channel"] >> (self.stage + 1)

    @property
    def step(self) -> int:
        """Stage lengths reachable from an integer mel length."""
        return int(np.prod(self.cfg["upsample_factors"][: self.stage + 1]))

    @property
    def hop(self) -> int:
        return int(np.prod(self.cfg["upsample_factors"]))

    @property
    def n_seeds(self) -> int:
        G = self.channels // 16
        return max(-(-G * k // 32) for k in self.cfg["resblock_kernel_sizes"])

    def lengths(self) -> List[int]:
        """Stage lengths at the form's tile edges (module docstring of the GPU test)."""
        q, S = self.step, self.S
        down = lambda n: (n // q) * q
        up = lambda n: -(-n // q) * q
        out = {q, down(S - 2), up(S + 2), up(3 * S + 10)}
        if down(self.lead - 1) >= q:
            out.add(down(self.lead - 1))
        if S % q == 0:
            out.add(S)
        return sorted(n for n in out if n >= q)


def _wide(C: int) -> Tuple[int, List[int]]:
    """(C0, x2 factors) of the narrowest topology whose first stage has C channels and whose last
    has at most 64 (conv_post's limit)."""
    n = 1
    while (C >> (n - 1)) > 64:
        n += 1
    return 2 * C, [2] * n


def _forms() -> List[Form]:
    fs: List[Form] = []

    def add(name, cfg, launch, count, modes, S_lead, env=(), stage=0, dense=False):
        fs.append(Form(name, cfg, stage, tuple(env), launch, count, tuple(modes), S_lead[0], S_lead[1], dense))

    R3OFF = ("TTS_MI355X_RESBLOCK3", "0")
    NOPOST = ("TTS_MI355X_POST_FUSION", "0")
    # ---- ResBlock1 pair launches, one kernel per topology (zmode 1)
    for C in (32, 64):
        C0, fac = _wide(C)
        for K in (3, 7, 11):
            add(f"pair_k{K}_c{C}", topology(C0, fac, [K]), f"mrf_pair_k{K}_c{C}", 3, MODES3, pair_stride(K, C),
                env=[R3OFF] if K == 3 else [])
    # two kernels: the pair as the last branch (zmode 3), conv_post fused into it or not
    add("pair_post_k7_c32", topology(64, [2], [3, 7]), "mrf_pair_post_k7_c32", 1, MODES3, pair_stride(7, 32, True))
    add("pair_nopost_k7_c32", topology(64, [2], [3, 7]), "mrf_pair_k7_c32", 3, MODES3, pair_stride(7, 32), env=[NOPOST])
    add("pair_post_k3_c32", topology(64, [2], [7, 3]), "mrf_pair_post_k3_c32", 1, MODES3, pair_stride(3, 32, True),
        env=[R3OFF])
    add("pair_post_k11_c64", topology(128, [2], [3, 11]), "mrf_pair_post_k11_c64", 1, MODES3, pair_stride(11, 64, True))
    add("pair_nopost_k11_c64", topology(128, [2], [3, 11]), "mrf_pair_k11_c64", 3, MODES3, pair_stride(11, 64),
        env=[NOPOST])
    add("pair_post_k3_c64", topology(128, [2], [11, 3]), "mrf_pair_post_k3_c64", 1, MODES3, pair_stride(3, 64, True),
        env=[R3OFF])
    # the pair as the first of two branches (zmode 1 beside a zmode-3 pair)
    add("pair_first_k11_c32", topology(64, [2], [11, 7]), "mrf_pair_k11_c32", 3, MODES3, pair_stride(11, 32), env=[NOPOST])
    # bf16 only: 128 channels (GEO 7) at kernels 7 / 11, 256 channels (GEO 8) at kernels 3 / 7
    for K in (7, 11):
        add(f"pair_k{K}_c128", topology(256, [2, 2], [K]), f"mrf_pair_k{K}_c128", 3, ("bf16",), pair_stride(K, 128), dense=True)
        add(f"pair_k{K}_c128_x8", topology(256, [8, 2], [K]), f"mrf_pair_k{K}_c128", 3, ("bf16",), pair_stride(K, 128), dense=True)
    for K in (3, 7):
        add(f"pair_k{K}_c256", topology(512, [2, 2, 2], [K]), f"mrf_pair_k{K}_c256", 3, ("bf16",), pair_stride(K, 256), dense=True)
        add(f"pair_k{K}_c256_x8", topology(512, [8, 2, 2], [K]), f"mrf_pair_k{K}_c256", 3, ("bf16",), pair_stride(K, 256), dense=True)
    add("pair_k7_k11_c128", topology(256, [2, 2], [7, 11]), "mrf_pair_k11_c128", 3, ("bf16",), pair_stride(11, 128), dense=True)
    add("pair_k3_k7_c256", topology(512, [2, 2, 2], [3, 7]), "mrf_pair_k7_c256", 3, ("bf16",), pair_stride(7, 256), dense=True)
    # a 128-channel pair stage behind a quiet 256-channel one (second stage under test)
    add("pair_k7_c128_stage1", topology(512, [2, 2, 2], [7]), "mrf_pair_k7_c128", 3, ("bf16",), pair_stride(7, 128),
        stage=1, dense=True)
    # bf16 activation planes under the narrow pairs (first factor 8)
    add("pair_k7_c32_x8", topology(64, [8], [7]), "mrf_pair_k7_c32", 3, ("bf16",), pair_stride(7, 32), dense=True)
    add("pair_post_k11_c64_x8", topology(128, [8], [3, 11]), "mrf_pair_post_k11_c64", 1, ("bf16",),
        pair_stride(11, 64, True), dense=True)

    # ---- ResBlock1 whole block
    for C in (32, 64):
        C0, fac = _wide(C)
        add(f"block_k3_c{C}", topology(C0, fac, [3]), f"mrf_block_k3_c{C}", 1, MODES3, block1_stride(3, C))
        for K in (7, 11):
            add(f"block_k{K}_c{C}", topology(C0, fac, [K]), f"mrf_block_k{K}_c{C}", 1, MODES3, block1_stride(K, C),
                env=[("TTS_MI355X_RB1_WHOLE_K", "7,11")])
    add("block_k3_c128", topology(256, [2, 2], [3]), "mrf_block_k3_c128", 1, ("f16x3", "bf16"), block1_stride(3, 128), dense=True)
    add("block_k3_c128_x8", topology(256, [8, 2], [3]), "mrf_block_k3_c128", 1, ("bf16",), block1_stride(3, 128), dense=True)
    # two whole blocks per stage: zmode 1 and zmode 3
    add("block_k3_k3_c128", topology(256, [2, 2], [3, 3]), "mrf_block_k3_c128", 2, ("f16x3", "bf16"), block1_stride(3, 128),
        dense=True)
    add("block_k3_k7_c64", topology(128, [2], [3, 7]), "mrf_block_k7_c64", 1, MODES3, block1_stride(7, 64),
        env=[("TTS_MI355X_RB1_WHOLE_K", "7,11")])
    add("block_k3_c64_x8", topology(128, [8], [3]), "mrf_block_k3_c64", 1, ("bf16",), block1_stride(3, 64), dense=True)

    # ---- ResBlock2 whole block: four kernels per stage (zmodes 1, 2, 2, 3), dilations [1, 3]
    ALL = ("TTS_MI355X_RB2_ALL", "1")
    K4 = [3, 5, 7, 11]
    for K in K4:
        add(f"block2_k{K}_c32", topology(64, [2], K4, "2"), f"mrf_block2_k{K}_c32", 1, MODES3, block2_stride(K, 32, 0), env=[ALL])
        for geo in (0, 1):
            add(f"block2_k{K}_c64_geo{geo}", topology(128, [2], K4, "2"), f"mrf_block2_k{K}_c64", 1, MODES3,
                block2_stride(K, 64, geo), env=[ALL, ("TTS_MI355X_RB2_GEO64", str(geo))])
        # the 192-column tiles on bf16 planes
        add(f"block2_k{K}_c64_geo1_x8", topology(128, [8], K4, "2"), f"mrf_block2_k{K}_c64", 1, ("bf16",),
            block2_stride(K, 64, 1), env=[ALL, ("TTS_MI355X_RB2_GEO64", "1")], dense=True)
    for K in (3, 5):
        add(f"block2_k{K}_c128", topology(256, [2, 2], [3, 5], "2"), f"mrf_block2_k{K}_c128", 1, ("f16x3", "bf16"),
            block2_stride(K, 128, 0), env=[ALL])
    add("block2_k5_c128_x8", topology(256, [8, 2], [3, 5], "2"), "mrf_block2_k5_c128", 1, ("bf16",),
        block2_stride(5, 128, 0), env=[ALL], dense=True)
    # HiFiGAN-v3's second branch: kernel 5, dilations [2, 6]
    add("block2_k5_c64_d26", topology(128, [2], [3, 5], "2", dil=[[1, 2], [2, 6]]), "mrf_block2_k5_c64", 1, MODES3,
        block2_stride(5, 64, 0), env=[ALL, ("TTS_MI355X_RB2_GEO64", "0")])
    return fs


FORMS: List[Form] = _forms()
FORM = {f.name: f for f in FORMS}
assert len(FORM) == len(FORMS)

# (form name, stage length) of every case; the exact arm runs each in every mode of the form
CASES: List[Tuple[str, int]] = [(f.name, n) for f in FORMS for n in f.lengths()]
DENSE_CASES: List[Tuple[str, int]] = [(f.name, n) for f in FORMS if f.dense for n in f.lengths()]


# ---------------------------------------------------------------------------------------------
# Exact-integer weights and inputs
# ---------------------------------------------------------------------------------------------
UPS_NONZEROS = 16  # per output row and phase of the upsampler that feeds the stage under test


def _block_conv(C: int, K: int, seed: int, tag: int) -> np.ndarray:
    """[C][C][K] 0 / 1 weights of one conv of the block under test, one nonzero per output row,
    placed by the rule of the module docstring."""
    G = C // 16
    perm = np.random.default_rng(10007 * tag + 31 * C + K).permutation(G * K)
    w = np.zeros((C, C, K), np.float32)
    for r in range(C):
        rb, i = divmod(r, 32)
        g, k = divmod(int(perm[(i + 32 * seed + 5 * rb) % (G * K)]), K)
        w[r, 16 * g + (7 * i + 3 * rb + seed + tag) % 16, k] = 1.0
    return w


def _quiet_conv(C: int, K: int, rng) -> np.ndarray:
    w = np.zeros((C, C, K), np.float32)
    w[rng.integers(C), rng.integers(C), rng.integers(K)] = 1.0
    return w


def exact_state_dict(cfg: dict, stage: int, seed: int) -> "OrderedDict[str, torch.Tensor]":
    """0 / 1 state dict (folded weights, no weight norm) of a ``HifiganGenerator(**cfg)`` in which
    only MRF stage ``stage`` computes at full strength."""
    rng = np.random.default_rng(977 * seed + 13)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()

    def put(name, w):
        sd[f"{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        sd[f"{name}.bias"] = torch.zeros(w.shape[1] if name.startswith("ups.") else w.shape[0])

    C0 = cfg["upsample_initial_channel"]
    w = np.zeros((C0, cfg["in_channels"], 7), np.float32)
    # one mel bin per row, at the centre tap (a one-frame mel reaches no other)
    w[np.arange(C0), rng.integers(cfg["in_channels"], size=C0), 3] = 1.0
    put("conv_pre", w)
    for i, u in enumerate(cfg["upsample_factors"]):
        cin, cout = C0 >> i, C0 >> (i + 1)
        w = np.zeros((cin, cout, 2 * u), np.float32)
        # output phase r reads taps r and r + u.  In front of the stage under test: UPS_NONZEROS
        # per (output row, phase).  Everywhere else a selection, one nonzero per (output row, phase):
        # the u * cout >= cin picks walk through permutations of the input channels, so every
        # channel of the stage in front is read and nothing grows.  Of the two taps the one in
        # [u / 2, u + u / 2) is taken: input sample m then lands on output m u + tap - u / 2, inside
        # [m u, m u + u), so the first and last samples are not cut off by the transposed conv's
        # padding and every element of the stage under test reaches conv_post
        if i == stage:
            for co in range(cout):
                for r in range(u):
                    ci = rng.choice(cin, size=UPS_NONZEROS, replace=False)
                    w[ci, co, r + u * rng.integers(2, size=UPS_NONZEROS)] = 1.0
        else:
            assert u * cout >= cin
            picks = np.concatenate([rng.permutation(cin) for _ in range(-(-u * cout // cin))])[: u * cout]
            for n, ci in enumerate(picks):
                co, r = divmod(n, u)
                w[ci, co, r if r >= u // 2 else r + u] = 1.0
        put(f"ups.{i}", w)
    nk = len(cfg["resblock_kernel_sizes"])
    assert nk in (1, 2, 4), "the MRF mean must divide by a power of two"
    for i in range(len(cfg["upsample_factors"])):
        ch = C0 >> (i + 1)
        for j, k in enumerate(cfg["resblock_kernel_sizes"]):
            names = ([f"convs1.{m}" for m in range(3)] + [f"convs2.{m}" for m in range(3)]
                     if cfg["resblock_type"] == "1" else [f"convs.{m}" for m in range(2)])
            for c, nm in enumerate(names):
                w = _block_conv(ch, k, seed, 8 * j + c) if i == stage else _quiet_conv(ch, k, rng)
                put(f"resblocks.{i * nk + j}.{nm}", w)
    cl = C0 >> len(cfg["upsample_factors"])
    sd["conv_post.weight"] = torch.full((1, cl, 7), 2.0 ** -16)
    sd["conv_post.bias"] = torch.zeros(1)
    return sd


def block_conv_names(cfg: dict, stage: int) -> List[str]:
    nk = len(cfg["resblock_kernel_sizes"])
    sub = ([f"convs1.{m}" for m in range(3)] + [f"convs2.{m}" for m in range(3)]
           if cfg["resblock_type"] == "1" else [f"convs.{m}" for m in range(2)])
    return [f"resblocks.{stage * nk + j}.{s}" for j in range(nk) for s in sub]


def coverage_union(cfg: dict, stage: int, seeds: Sequence[int]) -> Dict[str, np.ndarray]:
    """Per conv of the block under test: [C / 32][C / 16][K] booleans, true where some seed's weights
    hold a nonzero in that (32-row block, 16-channel group, tap)."""
    out: Dict[str, np.ndarray] = {}
    for s in seeds:
        sd = exact_state_dict(cfg, stage, s)
        for nm in block_conv_names(cfg, stage):
            w = sd[nm + ".weight"].numpy()
            C, _, K = w.shape
            m = (w != 0).reshape(C // 32, 32, C // 16, 16, K).any(axis=(1, 3))
            out[nm] = m if nm not in out else (out[nm] | m)
    return out


def exact_mel(batch: int, frames: int, seed: int) -> torch.Tensor:
    """0 / 1 mel [batch][80][frames], no utterance all zero.  One bin in ten is set; mels of fewer
    than four frames are denser (most of so short a stage's taps fall into the zero padding)."""
    rng = np.random.default_rng(7907 * seed + frames)
    p = 0.1 if frames >= 4 else 0.5
    m = (rng.random((batch, 80, frames)) < p).astype(np.float32)
    for b in range(batch):
        if not m[b].any():
            m[b, rng.integers(80), rng.integers(frames)] = 1.0
    return torch.from_numpy(m)


# ---------------------------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------------------------
def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def emulated_forward(cfg: dict, sd, mel: torch.Tensor, rnd=_bf16, z_at=None):
    """``oracle.hifigan_ref.hifigan_forward`` (fp64, pad 0) restated with ``rnd`` applied to the input
    of every conv and transposed conv; returns (waveform, conv_post's argument).  With the identity
    for ``rnd`` it is the oracle itself, which a CPU test asserts bit for bit.  ``z_at = (stage, z)``
    runs only what follows that stage's MRF, from ``z`` in its place (``mel`` is unused)."""
    w = {k: v.double() for k, v in sd.items()}
    lrelu = F.leaky_relu
    o = None if z_at else F.conv1d(rnd(mel.double()), w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    kernels, dils = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    nk = len(kernels)
    for i, (u, k) in enumerate(zip(cfg["upsample_factors"], cfg["upsample_kernel_sizes"])):
        if z_at and i <= z_at[0]:
            o = z_at[1]
            continue
        o = F.conv_transpose1d(rnd(lrelu(o, 0.1)), w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        z = None
        for j, (kk, dil) in enumerate(zip(kernels, dils)):
            r = f"resblocks.{i * nk + j}"
            x = o
            if cfg["resblock_type"] == "1":
                for m in range(3):
                    t = F.conv1d(rnd(lrelu(x, 0.1)), w[f"{r}.convs1.{m}.weight"], w[f"{r}.convs1.{m}.bias"],
                                 dilation=dil[m], padding=hifigan_ref.get_padding(kk, dil[m]))
                    t = F.conv1d(rnd(lrelu(t, 0.1)), w[f"{r}.convs2.{m}.weight"], w[f"{r}.convs2.{m}.bias"],
                                 padding=hifigan_ref.get_padding(kk, 1))
                    x = t + x
            else:
                for m in range(2):
                    t = F.conv1d(rnd(lrelu(x, 0.1)), w[f"{r}.convs.{m}.weight"], w[f"{r}.convs.{m}.bias"],
                                 dilation=dil[m], padding=hifigan_ref.get_padding(kk, dil[m]))
                    x = t + x
            z = x if z is None else z + x
        o = z / nk
    arg = F.conv1d(rnd(lrelu(o)), w["conv_post.weight"], w["conv_post.bias"], padding=3)
    return torch.tanh(arg), arg


def reference(cfg: dict, sd, mel: torch.Tensor):
    """(fp64 oracle output, bf16-emulated oracle output, the oracle's stages, conv_post's argument)."""
    with torch.no_grad():
        ref, stages = hifigan_ref.hifigan_forward(sd, mel, pad=0, dtype=torch.float64, return_stages=True, **cfg)
        emu, arg = emulated_forward(cfg, sd, mel)
    return ref, emu, stages, arg


def reach(cfg: dict, sd, stage: int, stage_len: int) -> torch.Tensor:
    """d sum(conv_post's argument) / d z for z = the MRF output of ``stage``, [C][stage_len], at
    z = 1: what follows is linear on non-negative values, so this is the weight with which each
    element of the stage under test reaches the waveform (0: an error there is invisible)."""
    C = cfg["upsample_initial_channel"] >> (stage + 1)
    z = torch.ones(1, C, stage_len, dtype=torch.float64, requires_grad=True)
    _, arg = emulated_forward(cfg, sd, None, rnd=lambda t: t, z_at=(stage, z))
    arg.sum().backward()
    return z.grad[0]


def mel_frames(form: Form, stage_len: int) -> int:
    assert stage_len % form.step == 0
    return stage_len // form.step


@functools.lru_cache(maxsize=None)
def exact_sd(name: str, seed: int):
    f = FORM[name]
    return exact_state_dict(f.cfg, f.stage, seed)


@functools.lru_cache(maxsize=None)
def exact_input(name: str, stage_len: int, seed: int) -> torch.Tensor:
    return exact_mel(B, mel_frames(FORM[name], stage_len), seed + 17 * stage_len)


@functools.lru_cache(maxsize=None)
def exact_oracle(name: str, stage_len: int, seed: int) -> torch.Tensor:
    """fp64 oracle of one exact case, computed once and shared."""
    f = FORM[name]
    with torch.no_grad():
        return hifigan_ref.hifigan_forward(exact_sd(name, seed), exact_input(name, stage_len, seed), pad=0,
                                           dtype=torch.float64, **f.cfg)


# the dense arm: ordinary synthetic weights and a Gaussian mel on the same topologies and lengths
@functools.lru_cache(maxsize=None)
def dense_sd(name: str):
    return synthetic.hifigan_state_dict(**FORM[name].cfg, seed=300 + len(name), weight_norm=False)


@functools.lru_cache(maxsize=None)
def dense_input(name: str, stage_len: int) -> torch.Tensor:
    return synthetic.mel(B, mel_frames(FORM[name], stage_len), seed=stage_len)


@functools.lru_cache(maxsize=None)
def dense_oracle(name: str, stage_len: int) -> torch.Tensor:
    with torch.no_grad():
        return hifigan_ref.hifigan_forward(dense_sd(name), dense_input(name, stage_len), pad=0, dtype=torch.float64,
                                           **FORM[name].cfg)
