"""Forms, strides and inputs for the tests of the 32-channel f16x3 whole block on 512-column tiles.

f16x3 at 32 channels runs, by default, a kernel-7 branch that a later branch follows in its stage as
one whole-block launch on a 512-column tile of swizzled 64-byte LDS rows (``Res3Cfg`` GEO 5); a
kernel-7 branch that is its stage's last MRF writer keeps the pair launches, whose last one carries
``conv_post``, and the kernel-3 block keeps its 256-column tile.  Under ``TTS_MI355X_RB1_WHOLE_K``
the kernel-7 / 11 blocks take the same 512-column tile.  ``TTS_MI355X_GEO32_WIDE=0`` at create time
restores the kernel-7 pairs and the 256-column blocks.  The tile strides, restated from the
library's source (``SOURCE_LINES`` quotes the lines; the CPU test asserts they stand there):

* ``RP_W = 512`` at GEO 5, ``RP_BN = RP_W - 2 * LEAD`` with ``LEAD = r3_lead(K) = 12 (K - 1) / 2``:
  S = 440 / 392 at kernels 7 / 11 (kept columns [LEAD, 512 - LEAD)).

Everything else (0 / 1 weights, ``conv_post`` = 2^-16, the gate, the reach check, the references)
is ``_mrf_exact``'s, imported.  B = 2.  Stage lengths: 4, S - 2, S, S + 2, 2 S and 3 S + 6, all even
(the stage follows a x2 layer), at most 1,326 columns.
"""
from __future__ import annotations

import contextlib
import functools
import os
from typing import Dict, List, Tuple

import torch

import _mrf_exact as X
from oracle import hifigan_ref
from tts_amd import synthetic

B = 2
MODE = "f16x3"
SWITCH = "TTS_MI355X_GEO32_WIDE"

# (file under tts-3_amd/csrc, text): the tile, its selection and the switch
SOURCE_LINES = (
    ("resblock_block.hpp", "struct Res3Cfg<S, C, 5, K, NCV, XO, LEAD, UP, SW> {"),
    ("resblock_block.hpp", "static constexpr int RP_W = 512;"),
    ("resblock_block.hpp", "static constexpr int RP_BN = RP_W - 2 * LEAD;"),
    ("resblock_block.hpp", "constexpr int R3_LEAD = 12;"),
    ("resblock_block.hpp", "constexpr int r3_lead(int K) { return R3_LEAD * ((K - 1) / 2); }"),
    ("kernels_resblock.hip", "using P = Res3Cfg<S, C, GEO, K, 6, r3_xoff(K), r3_lead(K)>;"),
    ("kernels_resblock.hip", "if (C == 32 && (K == 7 || K == 11) && (wide64 & kWide32Block) && a.planes == 0) {"),
    ("kernels_resblock.hip", "if (K == 7) launch_res3_t<S, 32, 5, 7>(a, B, s);"),
    ("kernels_resblock.hip", "else launch_res3_t<S, 32, 5, 11>(a, B, s);"),
    ("kernels_resblock.hip", "return e && e[0] == '0' ? 0 : kWide32Block;"),
    ("common.hpp", "constexpr int kWide32Block = 4;"),
    ("hifigan.cpp", "geo32_wide_ = mrf_geo32_wide(mode);"),
    ("hifigan.cpp", "const bool k7_block = k == 7 && ch == 32 && (geo32_wide_ & kWide32Block) != 0 && j + 1 < cfg_.num_kernels;"),
    ("hifigan.cpp", "[&] { launch_resblock3(L1.mode, ra, B, L1.Cout, L1.K, geo64_wide_ | geo32_wide_, sj); });"),
    ("hifigan.cpp", "const bool k_ok = k == 3 || k7_block || wk.find(std::to_string(k)) != std::string::npos;"),
)


def block_stride(K: int) -> Tuple[int, int]:
    lead = 12 * ((K - 1) // 2)
    return 512 - 2 * lead, lead


WHOLE = ("TTS_MI355X_RB1_WHOLE_K", "7,11")


def _forms() -> List[X.Form]:
    fs = []

    def add(name, kernels, K, env=()):
        S, lead = block_stride(K)
        fs.append(X.Form(name, X.topology(64, [2], kernels), 0, tuple(env), f"mrf_block_k{K}_c32", 1, (MODE,), S, lead))

    add("block_k7_first", [7, 3], 7)       # the kernel-7 block writes the MRF sum (zmode 1)
    add("block_k7_mid", [3, 7, 11, 3], 7)  # and adds to it (zmode 2), its position in HiFiGAN-v1
    add("block_k11", [11], 11, env=[WHOLE])
    return fs


FORMS = _forms()
FORM = {f.name: f for f in FORMS}
# launch counts of one forward beside the form's own launch: (default, with the switch at 0)
LAUNCHES: Dict[str, Tuple[Dict[str, int], Dict[str, int]]] = {
    "block_k7_first": ({"mrf_block_k7_c32": 1, "mrf_pair_k7_c32": 0, "mrf_block_k3_c32": 1},
                       {"mrf_block_k7_c32": 0, "mrf_pair_k7_c32": 3, "mrf_block_k3_c32": 1}),
    "block_k7_mid": ({"mrf_block_k7_c32": 1, "mrf_pair_k7_c32": 0, "mrf_pair_k11_c32": 3, "mrf_block_k3_c32": 2},
                     {"mrf_block_k7_c32": 0, "mrf_pair_k7_c32": 3, "mrf_pair_k11_c32": 3, "mrf_block_k3_c32": 2}),
    "block_k11": ({"mrf_block_k11_c32": 1, "mrf_pair_k11_c32": 0}, {"mrf_block_k11_c32": 1, "mrf_pair_k11_c32": 0}),
}
# the dispatch case: a kernel-7 branch that is its stage's last MRF writer keeps the pairs
LAST_K7 = X.Form("last_k7", X.topology(64, [2], [3, 7]), 0, (), "mrf_pair_post_k7_c32", 1, (MODE,), *block_stride(7))
LAST_K7_LAUNCHES = {"mrf_pair_post_k7_c32": 1, "mrf_pair_k7_c32": 2, "mrf_block_k7_c32": 0, "mrf_block_k3_c32": 1}
ALL_FORM = dict(FORM, last_k7=LAST_K7)


def lengths(f: X.Form) -> List[int]:
    S = f.S
    return [4, S - 2, S, S + 2, 2 * S, 3 * S + 6]


def dense_lengths(f: X.Form) -> List[int]:
    return [f.S + 2, 3 * f.S + 6]


CASES = [(f.name, n) for f in FORMS for n in lengths(f)]
DENSE_CASES = [(f.name, n) for f in FORMS for n in dense_lengths(f)]
LAST_K7_LENGTHS = [LAST_K7.S + 2, 3 * LAST_K7.S + 6]


@functools.lru_cache(maxsize=None)
def exact_sd(name: str, seed: int):
    return X.exact_state_dict(ALL_FORM[name].cfg, 0, seed)


@functools.lru_cache(maxsize=None)
def exact_input(name: str, stage_len: int, seed: int) -> torch.Tensor:
    return X.exact_mel(B, X.mel_frames(ALL_FORM[name], stage_len), seed + 17 * stage_len)


@functools.lru_cache(maxsize=None)
def exact_oracle(name: str, stage_len: int, seed: int) -> torch.Tensor:
    with torch.no_grad():
        return hifigan_ref.hifigan_forward(exact_sd(name, seed), exact_input(name, stage_len, seed), pad=0,
                                           dtype=torch.float64, **ALL_FORM[name].cfg)


@functools.lru_cache(maxsize=None)
def dense_sd(name: str):
    return synthetic.hifigan_state_dict(**FORM[name].cfg, seed=320 + len(name), weight_norm=False)


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
    keys = X.ENV_SWITCHES + (SWITCH, "TTS_MI355X_GEO64_WIDE")
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
