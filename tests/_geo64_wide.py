"""Forms, strides and inputs for the tests of the 64-channel f16x3 kernels' 256-column tiles.

f16x3 at 64 channels takes, by default, the pair kernel's GEO 0 tile and the kernel-3 whole block's
GEO 0 tile on swizzled 64-byte LDS rows (``TTS_MI355X_GEO64_WIDE=0`` at create time restores the
192- and 128-column tiles).  The tile strides, restated from the library's source
(``SOURCE_LINES`` quotes the lines; the CPU test asserts they stand there):

* pair: ``RP_W = 256`` at GEO 0, ``RP_BN = RP_W - 2 * LEAD`` with ``LEAD = (K - 1) / 2``:
  S = 254 / 250 / 246 at kernels 3 / 7 / 11, and ``STRIDE = RP_BN - 2 * kPostHalo`` = 240 for the
  kernel-11 pair with ``conv_post`` in its epilogue;
* block: ``RP_W = 256`` at GEO 0, ``RP_BN = RP_W - 2 * r3_lead(3)`` = 232 (kept columns [12, 244)).

Everything else (0 / 1 weights, ``conv_post`` = 2^-16, the gate, the reach check, the references)
is ``_mrf_exact``'s, imported.  B = 2.  Stage lengths: 4, S - 2, S, S + 2, 2 S and 3 S + 6, all even
(the stage follows a x2 layer); at S and 2 S the last workgroup of a block with the upsampling tail
keeps no column of its own and emits only the x2 layer's last one.
"""
from __future__ import annotations

import contextlib
import functools
import os
from typing import List, Tuple

import torch

import _mrf_exact as X
from oracle import hifigan_ref
from tts_amd import synthetic

B = 2
MODE = "f16x3"
SWITCH = "TTS_MI355X_GEO64_WIDE"

SOURCE_LINES = X.SOURCE_LINES[:7] + (  # PairCfg's RP_W, LEAD, RP_BN, STRIDE, kPostHalo and the two grids
    # the pair: GEO 0 (256 columns) with the swizzled rows, in front of the 192-column fallback
    ("kernels_resblock.hip", "if (C == 64 && (wide64 & kWide64Pair) && pair_geo64() == 1 && a.c1.planes == 0) {"),
    ("kernels_resblock.hip", "launch_pair_t<S, K, 64, 0, true>(a, B, s);"),
    ("kernels_resblock.hip", "using P = PairCfg<S, K, C, PD, GEO, AX, true, SWZ>;"),
    ("kernels_resblock.hip", "using P = PairCfg<S, K, C, PD, GEO, AX, false, SWZ>;"),
    # the block: GEO 0 (256 columns) with the swizzled rows, plain and with the upsampling tail
    ("kernels_resblock.hip", "if (C == 64 && (wide64 & kWide64Block) && a.planes == 0) {"),
    ("kernels_resblock.hip", "launch_res3_wide64<S, false>(a, B, s);"),
    ("kernels_resblock.hip", "else if (wide64 & kWide64Block) launch_res3_wide64<SchemeH3, true>(a, B, s);"),
    ("kernels_resblock.hip", "using P = Res3Cfg<S, 64, 0, 3, 6, r3_xoff(3), r3_lead(3), UP, true>;"),
    ("kernels_resblock.hip", "static_assert(P::RP_BN == 232, \"kept columns [12, 244)\");"),
    ("kernels_resblock.hip", "const int rp_w = C == 64 && (wide64 & kWide64Block) ? 256 : 128;"),
    ("kernels_resblock.hip", "return e && e[0] == '0' ? 0 : (kWide64Block | kWide64Pair);"),
    ("resblock_block.hpp", "static constexpr int RP_W = GEO == 0 ? 256 : (GEO == 1 ? 192 : 128);"),
    ("resblock_block.hpp", "static constexpr int RP_BN = RP_W - 2 * LEAD;"),
    ("resblock_block.hpp", "constexpr int R3_LEAD = 12;"),
    ("resblock_block.hpp", "constexpr int r3_lead(int K) { return R3_LEAD * ((K - 1) / 2); }"),
)


def pair_stride(K: int, post: bool = False) -> Tuple[int, int]:
    rp_bn = 256 - 2 * ((K - 1) // 2)
    return (rp_bn - 6, (K - 1) // 2 + 3) if post else (rp_bn, (K - 1) // 2)


def block_stride() -> Tuple[int, int]:
    return 256 - 2 * 12, 12


R3OFF = ("TTS_MI355X_RESBLOCK3", "0")


def _forms() -> List[X.Form]:
    fs = []

    def add(name, cfg, launch, count, S_lead, env=()):
        fs.append(X.Form(name, cfg, 0, tuple(env), launch, count, (MODE,), S_lead[0], S_lead[1]))

    for K in (3, 7, 11):
        add(f"pair_k{K}", X.topology(128, [2], [K]), f"mrf_pair_k{K}_c64", 3, pair_stride(K), env=[R3OFF] if K == 3 else [])
    add("pair_post_k11", X.topology(128, [2], [3, 11]), "mrf_pair_post_k11_c64", 1, pair_stride(11, True))
    add("block", X.topology(128, [2], [3]), "mrf_block_k3_c64", 1, block_stride())
    # the block as its stage's last launch, the next stage's x2 upsampler in its tail
    add("block_up", X.topology(128, [2, 2], [3]), "mrf_block_k3_c64", 1, block_stride())
    add("block_up_k7", X.topology(128, [2, 2], [3, 7]), "mrf_block_k3_c64", 1, block_stride())
    return fs


FORMS = _forms()
FORM = {f.name: f for f in FORMS}
# a form with the upsampling tail launches no upsampler for its second stage
TAIL = {"block_up": "ups_u2_c32", "block_up_k7": "ups_u2_c32"}


def lengths(f: X.Form) -> List[int]:
    S = f.S
    return [4, S - 2, S, S + 2, 2 * S, 3 * S + 6]


def dense_lengths(f: X.Form) -> List[int]:
    return [f.S + 2, 3 * f.S + 6]


CASES = [(f.name, n) for f in FORMS for n in lengths(f)]
DENSE_CASES = [(f.name, n) for f in FORMS for n in dense_lengths(f)]


@functools.lru_cache(maxsize=None)
def exact_sd(name: str, seed: int):
    return X.exact_state_dict(FORM[name].cfg, 0, seed)


@functools.lru_cache(maxsize=None)
def exact_input(name: str, stage_len: int, seed: int) -> torch.Tensor:
    return X.exact_mel(B, X.mel_frames(FORM[name], stage_len), seed + 17 * stage_len)


@functools.lru_cache(maxsize=None)
def exact_oracle(name: str, stage_len: int, seed: int) -> torch.Tensor:
    with torch.no_grad():
        return hifigan_ref.hifigan_forward(exact_sd(name, seed), exact_input(name, stage_len, seed), pad=0,
                                           dtype=torch.float64, **FORM[name].cfg)


@functools.lru_cache(maxsize=None)
def dense_sd(name: str):
    return synthetic.hifigan_state_dict(**FORM[name].cfg, seed=640 + len(name), weight_norm=False)


@functools.lru_cache(maxsize=None)
def dense_input(name: str, stage_len: int) -> torch.Tensor:
    return synthetic.mel(B, X.mel_frames(FORM[name], stage_len), seed=stage_len)


@functools.lru_cache(maxsize=None)
def dense_oracle(name: str, stage_len: int) -> torch.Tensor:
    with torch.no_grad():
        return hifigan_ref.hifigan_forward(dense_sd(name), dense_input(name, stage_len), pad=0, dtype=torch.float64,
                                           **FORM[name].cfg)


@contextlib.contextmanager
def env(form: X.Form, wide: bool):
    """The form's switches and the geometry switch, none of the others: they are read when a
    generator's first forward creates its native handle."""
    keys = X.ENV_SWITCHES + (SWITCH,)
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(dict(form.env))
    if not wide:
        os.environ[SWITCH] = "0"
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
