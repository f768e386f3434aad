"""Exact-integer inputs, cases and the fp64 reference for the base conv kernels.

``conv1d_mfma_kernel`` (``kernels_conv.hip``, the fp32 math mode) and ``conv1d_split_kernel``
(``split_kernel.hpp``: fp32x6, f16x3, bf16) are reached through ``tts_op_conv1d_bench``, which takes
a tile index; the ConvTranspose1d forms through ``tts_op_conv_transpose1d``.  The inputs are built so
that every math mode must reproduce the fp64 reference bit for bit:

* ``x`` holds integers in [-4, 4], the weights integers in [-2, 2], ``bias`` / ``res`` / ``z0``
  integers in [-3, 3]; ``in_slope`` and ``out_slope`` are 1, 0.5 or 0.25 and ``zdiv`` is 4;
* after the leaky-ReLU every operand has at most 3 significant bits, so the bf16 operand, the
  three-piece bf16 split and the scaled fp16 hi / lo split are exact (the low pieces are zero);
* every product and partial sum is a multiple of 2^-2, the value after ``out_slope`` a multiple of
  2^-4 and the one after ``/ zdiv`` a multiple of 2^-6, all far below 2^24 of those steps: exact in
  fp32 in any summation order.  ``test_conv_exact_cpu.py`` asserts the bounds for every case.

B = 3 and batch item 1 is all zero: in f16x3 that item's max-abs slot is 0, the ``m == 0`` branch of
``amax_exp`` (``split_device.hpp``).

``FP32_TILES`` / ``SPLIT_TILES`` mirror the two tile tables as (BM, BN, CK, wide); the source lines
are quoted beside them and the CPU test parses the sources and compares.  Per (mode, tile):

* channels ``(Cin, Cout)`` = ``(CK + 3, BM + 1)`` (a second row block of one row, a second channel
  chunk of three channels) and ``(5, 31)``;
* ``(K, dil)`` = (1, 1), (3, 1), (3, 5), (5, 2), (7, 5), (11, 5) - the last two at the narrow halo
  limit ``(K - 1) * 5`` - and on the wide tiles (7, 16) (halo 96, the wide limit) and (11, 9);
* with ``pad = dil * (K - 1) / 2``: T in {1, pad, pad + 1, BN - pad, BN - 1, BN, BN + 1, BN + pad,
  2 BN + 1};
* the epilogues ``EPILOGUES`` rotate over (channels, (K, dil), T), so each meets every tile and
  every K; the ``rep_pad`` one is K = 7, dil = 1, ``rep_pad`` = 5 with the edges placed on
  ``Tout = T + 10``, plus T = 1 and 2.

``CONVT_SHAPES`` / ``CONVT_WINDOW_SHAPES`` list the ConvTranspose1d shapes and ``convT_form`` names the
form the entry point dispatches each to (see ``test_conv_exact_gpu.py``).

Out of scope:

* the Winograd tile 21: its transforms are inexact, and ``test_op_conv1d_winograd`` sweeps its edges;
* the gate tile 20 and the ``cvec`` / ``mask`` / ``wn_rows`` / bf16-plane epilogues: the op entry
  cannot reach them.  They are held bitwise to the unfused kernels in ``test_glow_gpu.py`` and
  ``test_vits_gpu.py``, and those unfused kernels are the ones tested here.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

B = 3
ZDIV = 4.0
MODES = ("fp32", "fp32x6", "f16x3", "bf16")
SPLIT_MODES = MODES[1:]
SLOPES = (1.0, 0.5, 0.25)
NARROW_DMAX = 5   # kernels_conv.hip ``constexpr int DMAX = 5;``, split_kernel.hpp ``(K - 1) * 5``
HALO_WIDE = 96    # kernels_conv.hip ``constexpr int HALO_WIDE = 96;``, split_kernel.hpp ``halo <= 96``

# ---------------------------------------------------------------------------------------------
# Tile tables: index -> (BM, BN, CK, wide)
# ---------------------------------------------------------------------------------------------
# kernels_conv.hip kConvTiles ``{BM, BN, TM, TN, CK = 8*G, PD}`` and launch_conv1d_k
# ``case N: launch_conv1d_t<K, BM, BN, TM, TN, G, PD, WIDE>``:
#   {128, 128, 2, 2, 16, 1},  // 0     case 0: launch_conv1d_t<K, 128, 128, 2, 2, 2, 1, true>
#   {64, 256, 2, 2, 16, 1},   // 1     case 1: launch_conv1d_t<K, 64, 256, 2, 2, 2, 1, true>
#   {32, 512, 1, 4, 8, 1},    // 2     case 2: launch_conv1d_t<K, 32, 512, 1, 4, 1, 1, true>
#   {128, 128, 2, 2, 32, 1},  // 3     case 3: launch_conv1d_t<K, 128, 128, 2, 2, 4, 1, false>
#   {128, 128, 2, 2, 16, 2},  // 4     case 4: launch_conv1d_t<K, 128, 128, 2, 2, 2, 2, false>
#   {32, 256, 1, 2, 16, 1},   // 8     case 8: launch_conv1d_t<K, 32, 256, 1, 2, 2, 1, false>
#   {64, 128, 2, 1, 16, 1},   // 10    case 10: launch_conv1d_t<K, 64, 128, 2, 1, 2, 1, false>
#   {128, 128, 2, 2, 32, 2},  // 11    case 11: launch_conv1d_t<K, 128, 128, 2, 2, 4, 2, false>
# 5, 6, 7, 9, 12, 13 stand behind ``#ifdef TTS_TUNING_TILES`` and are not built.
FP32_TILES: Dict[int, Tuple[int, int, int, bool]] = {
    0: (128, 128, 16, True),
    1: (64, 256, 16, True),
    2: (32, 512, 8, True),
    3: (128, 128, 32, False),
    4: (128, 128, 16, False),
    8: (32, 256, 16, False),
    10: (64, 128, 16, False),
    11: (128, 128, 32, False),
}
FP32_UNBUILT = (5, 6, 7, 9, 12, 13)
FP32_TABLE_SIZE = 14

# kernels_conv_split.hip kSplitTiles ``{BM, BN, TM, TN, CK = 16*G, PD}`` and split_kernel.hpp
# launch_split_k ``case N: launch_split_t<S, K, BM, BN, TM, TN, G, PD, WIDE, ...>``:
#   {128, 128, 2, 2, 16, 1},  // 0     case 0: launch_split_t<S, K, 128, 128, 2, 2, 1, 1, true, ...>
#   {64, 256, 2, 2, 16, 1},   // 1     case 1: launch_split_t<S, K, 64, 256, 2, 2, 1, 1, true, ...>
#   {32, 512, 1, 4, 16, 1},   // 2     case 2: launch_split_t<S, K, 32, 512, 1, 4, 1, 1, true, ...>
#   {128, 128, 2, 2, 32, 1},  // 3     ... 3-19: WIDE = false
#   {64, 128, 2, 1, 32, 1},   // 4
#   {32, 256, 1, 2, 32, 1},   // 5
#   {64, 256, 2, 2, 32, 1},   // 6
#   {128, 128, 2, 2, 16, 2},  // 7
#   {64, 128, 2, 1, 32, 2},   // 8
#   {64, 256, 2, 2, 32, 2},   // 9
#   {64, 256, 2, 2, 16, 2},   // 10
#   {32, 256, 1, 2, 32, 2},   // 11
#   {64, 128, 2, 1, 32, 3},   // 12
#   {128, 128, 2, 2, 32, 2},  // 13
#   {32, 256, 1, 2, 16, 1},   // 14
#   {32, 256, 1, 2, 16, 2},   // 15
#   {32, 128, 1, 1, 16, 2},   // 16
#   {64, 128, 2, 1, 16, 1},   // 17
#   {64, 128, 2, 1, 16, 2},   // 18
#   {32, 512, 1, 4, 16, 2},   // 19
# 20 is the gate tile and 21 the Winograd tile (module docstring).
SPLIT_TILES: Dict[int, Tuple[int, int, int, bool]] = {
    0: (128, 128, 16, True),
    1: (64, 256, 16, True),
    2: (32, 512, 16, True),
    3: (128, 128, 32, False),
    4: (64, 128, 32, False),
    5: (32, 256, 32, False),
    6: (64, 256, 32, False),
    7: (128, 128, 16, False),
    8: (64, 128, 32, False),
    9: (64, 256, 32, False),
    10: (64, 256, 16, False),
    11: (32, 256, 32, False),
    12: (64, 128, 32, False),
    13: (128, 128, 32, False),
    14: (32, 256, 16, False),
    15: (32, 256, 16, False),
    16: (32, 128, 16, False),
    17: (64, 128, 16, False),
    18: (64, 128, 16, False),
    19: (32, 512, 16, False),
}
SPLIT_TABLE_SIZE = 22  # with the gate and Winograd tiles


def tiles_of(mode: str) -> Dict[int, Tuple[int, int, int, bool]]:
    return FP32_TILES if mode == "fp32" else SPLIT_TILES


# the 8 + 3 x 20 (mode, tile) pairs, tiles of one geometry next to each other: the cases of a
# geometry are shared, so their cached references are reused by the tests that follow
MODE_TILES: List[Tuple[str, int]] = sorted(((m, t) for m in MODES for t in tiles_of(m)),
                                           key=lambda mt: (tiles_of(mt[0])[mt[1]][:3], mt[1], MODES.index(mt[0])))
assert len(MODE_TILES) == 8 + 3 * 20


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
KD_ALL = ((1, 1), (3, 1), (3, 5), (5, 2), (7, 5), (11, 5))
KD_WIDE = ((7, 16), (11, 9))
KS = (1, 3, 5, 7, 11)
# name -> (fixed (in_slope, out_slope) or None: drawn per case, res, zmode)
EPILOGUES = {
    "plain": (None, False, 0),
    "slopes_res": ((0.5, 0.25), True, 0),
    "zmode1": (None, False, 1),
    "zmode2_res": (None, True, 2),
    "zmode3": (None, False, 3),
}
ROTATED = tuple(EPILOGUES)
REP_PAD = 5
ALL_EPILOGUES = ROTATED + ("rep_pad",)


@dataclass(frozen=True)
class Case:
    BM: int
    BN: int
    CK: int
    Cin: int
    Cout: int
    K: int
    dil: int
    T: int
    rep: int
    epi: str
    in_slope: float
    out_slope: float
    res: bool
    zmode: int

    @property
    def pad(self) -> int:
        return self.dil * (self.K - 1) // 2

    @property
    def Tout(self) -> int:
        return self.T + 2 * self.rep

    @property
    def seed(self) -> int:
        return zlib.crc32(repr((self.Cin, self.Cout, self.K, self.dil, self.T, self.rep, self.epi)).encode())

    def __str__(self) -> str:
        return (f"Cin={self.Cin} Cout={self.Cout} K={self.K} dil={self.dil} T={self.T} epilogue={self.epi} "
                f"(slopes {self.in_slope}/{self.out_slope}, res={self.res}, zmode={self.zmode}, rep_pad={self.rep})")


def lengths(BN: int, pad: int) -> List[int]:
    return sorted({t for t in (1, pad, pad + 1, BN - pad, BN - 1, BN, BN + 1, BN + pad, 2 * BN + 1) if t > 0})


def channel_shapes(BM: int, CK: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    return ((CK + 3, BM + 1), (5, 31))


@functools.lru_cache(maxsize=None)
def cases(BM: int, BN: int, CK: int, wide: bool) -> Tuple[Case, ...]:
    out: List[Case] = []
    kds = KD_ALL + (KD_WIDE if wide else ())
    for i, (Cin, Cout) in enumerate(channel_shapes(BM, CK)):
        for j, (K, dil) in enumerate(kds):
            for n, T in enumerate(lengths(BN, dil * (K - 1) // 2)):
                epi = ROTATED[(i + j + n) % len(ROTATED)]
                fixed, res, zmode = EPILOGUES[epi]
                s_in, s_out = fixed or (SLOPES[(i + 2 * j + n) % 3], SLOPES[(j + n // 3) % 3])
                out.append(Case(BM, BN, CK, Cin, Cout, K, dil, T, 0, epi, s_in, s_out, res, zmode))
        # replicate padding (conv_pre's form): the edges of lengths() on Tout = T + 2 * REP_PAD
        pad = 3
        touts = [t for t in lengths(BN, pad) if t > 2 * REP_PAD]
        for n, T in enumerate([1, 2] + [t - 2 * REP_PAD for t in touts]):
            out.append(Case(BM, BN, CK, Cin, Cout, 7, 1, T, REP_PAD, "rep_pad", SLOPES[(i + n) % 3], SLOPES[(n // 2) % 3],
                            (i + n) % 2 == 1, 0))
    return tuple(out)


def cases_of(mode: str, tile: int) -> Tuple[Case, ...]:
    return cases(*tiles_of(mode)[tile])


def length_classes(c: Case) -> List[str]:
    """The classes of T (Tout under replicate padding) the coverage test counts."""
    n, out = c.Tout, []
    if n < c.pad:
        out.append("<pad")
    for name, v in (("BN-1", c.BN - 1), ("BN", c.BN), ("BN+1", c.BN + 1)):
        if n == v:
            out.append(name)
    if n > 2 * c.BN:
        out.append(">2BN")
    return out


# ---------------------------------------------------------------------------------------------
# Inputs and references
# ---------------------------------------------------------------------------------------------
def _ints(g: torch.Generator, lo: int, hi: int, *shape: int) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def cover_weights(w: torch.Tensor, group: int = 8) -> torch.Tensor:
    """Put a nonzero into every all-zero (32-row block, ``group``-channel group, tap) of [Cout][Cin][K]
    weights and into every all-zero row, in place.  8-channel groups are the fp32 kernel's staging
    unit; they nest in the split kernels' 16-channel groups and in every tile's CK-channel chunk."""
    Cout, Cin, K = w.shape
    for r0 in range(0, Cout, 32):
        for c0 in range(0, Cin, group):
            for k in range(K):
                blk = w[r0:r0 + 32, c0:c0 + group, k]
                if not blk.any():
                    blk[(r0 // 32 + k) % blk.shape[0], (c0 // group + k) % blk.shape[1]] = 1.0 if (r0 + c0 + k) % 2 else -2.0
    for r in range(Cout):
        if not w[r].any():
            w[r, r % Cin, r % K] = 1.0
    return w


def inputs(c: Case):
    """(x [B][Cin][T], w [Cout][Cin][K], bias [Cout], res or None, z0) as fp32 tensors of integers."""
    g = torch.Generator().manual_seed(c.seed)
    x = _ints(g, -4, 4, B, c.Cin, c.T)
    x[1] = 0.0
    w = cover_weights(_ints(g, -2, 2, c.Cout, c.Cin, c.K))
    bias = _ints(g, -3, 3, c.Cout)
    res = _ints(g, -3, 3, B, c.Cout, c.Tout) if c.res else None
    z0 = _ints(g, -3, 3, B, c.Cout, c.Tout)
    return x, w, bias, res, z0


def conv_reference(x, w, bias, res, z0, *, dil, rep, in_slope, out_slope, zmode, zdiv=ZDIV) -> torch.Tensor:
    """fp64 ``F.conv1d`` with the op's prologue and epilogue (conv_device.hpp conv_epilogue_impl)."""
    K = w.shape[2]
    xp = F.pad(x.double(), (rep, rep), "replicate") if rep else x.double()
    v = F.conv1d(F.leaky_relu(xp, in_slope), w.double(), bias.double(), dilation=dil, padding=dil * (K - 1) // 2)
    v = F.leaky_relu(v, out_slope)
    if res is not None:
        v = v + res.double()
    if zmode == 2:
        v = z0.double() + v
    elif zmode == 3:
        v = (z0.double() + v) / zdiv
    return v


# bounded: the tests of one tile geometry follow each other (MODE_TILES) and share these
@functools.lru_cache(maxsize=400)
def reference(c: Case) -> torch.Tensor:
    x, w, bias, res, z0 = inputs(c)
    return conv_reference(x, w, bias, res, z0, dil=c.dil, rep=c.rep, in_slope=c.in_slope, out_slope=c.out_slope,
                          zmode=c.zmode)


def numpy_reference(x, w, bias, res, z0, *, dil, rep, in_slope, out_slope, zmode, zdiv=ZDIV, zero_pad=False,
                    drop_tap=None, shift=0) -> np.ndarray:
    """The same operation written out tap by tap in numpy fp64, with the three deliberate mistakes
    the sensitivity test applies: ``drop_tap`` leaves a tap out, ``shift`` reads the input that many
    columns to the right, ``zero_pad`` pads with zeros where the op replicates."""
    x, w, bias = (np.asarray(a, np.float64) for a in (x, w, bias))
    Cout, Cin, K = w.shape
    pad = dil * (K - 1) // 2
    if rep:
        x = np.pad(x, ((0, 0), (0, 0), (rep, rep)), mode="constant" if zero_pad else "edge")
    To = x.shape[2]
    a = np.where(x > 0, x, x * in_slope)
    ap = np.pad(a, ((0, 0), (0, 0), (pad + abs(shift), pad + abs(shift))))
    v = np.zeros((x.shape[0], Cout, To)) + bias[None, :, None]
    for k in range(K):
        if k == drop_tap:
            continue
        o = abs(shift) + shift + k * dil
        v += np.einsum("oc,bct->bot", w[:, :, k], ap[:, :, o:o + To])
    v = np.where(v > 0, v, v * out_slope)
    if res is not None:
        v = v + np.asarray(res, np.float64)
    if zmode == 2:
        v = np.asarray(z0, np.float64) + v
    elif zmode == 3:
        v = (np.asarray(z0, np.float64) + v) / zdiv
    return v


# ---------------------------------------------------------------------------------------------
# ConvTranspose1d (kernel 2U, stride U, padding U / 2)
# ---------------------------------------------------------------------------------------------
CONVT_SLOPE = 0.5
# kernels_conv.hip ConvTTiles<U>::t[convT_tile_for(Cout, U)] with ``convT_tile_for``:
# ``return Cout > 32 ? 0 : 1;``  (BM, BN; CK = 8)
#   ConvTTiles<8>: {{64, 64, 1, 1, 8}, {32, 128, 1, 1, 8}}
#   ConvTTiles<4>: {{64, 128, 1, 2, 8}, {32, 256, 1, 2, 8}}
#   ConvTTiles<2>: {{64, 256, 2, 2, 8}, {32, 512, 1, 4, 8}}
CONVT_FP32_TILES = {8: ((64, 64), (32, 128)), 4: ((64, 128), (32, 256)), 2: ((64, 256), (32, 512))}
CONVT_RES_BN = 64  # kernels_convT_res.hip ConvTResCfg: BN = WC * TN * 32 with WR = 8 (WC = 1), TN = 2


def split_tile_for(mode: str, Cout: int, K: int, Cin: int, dil: int) -> int:
    """kernels_conv_split.hip conv1d_split_tile_for (without ``TTS_MI355X_B1_TILES``)."""
    if (K - 1) * dil > (K - 1) * 5:
        return 0 if Cout > 64 else (1 if Cout > 32 else 2)
    if mode == "f16x3":
        return 13 if Cout > 64 else (10 if Cout > 32 else 14)
    if Cout > 64:
        return 7 if (K >= 11 or Cin % 32 != 0) else 3
    if Cout > 32:
        return 10 if K <= 3 else 1
    return 2


def convT_res_supported(mode: str, Cin: int, Cout: int, U: int) -> bool:
    """kernels_convT_res.hip convT_res_supported, for the op entry's arguments (rows = U * Cout)."""
    rows = U * Cout
    return mode in ("f16x3", "bf16") and U == 8 and rows % 256 == 0 and (Cin in (128, 256) or (Cin == 512 and rows >= 1024))


def convT_form(mode: str, Cin: int, Cout: int, U: int) -> Tuple[str, int]:
    """(form, BN: frames per workgroup) ``tts_op_conv_transpose1d`` dispatches the shape to."""
    if mode == "fp32":
        cls = 0 if Cout > 32 else 1
        return f"fp32_poly_u{U}_t{cls}", CONVT_FP32_TILES[U][cls][1]
    if convT_res_supported(mode, Cin, Cout, U):
        return f"window_x8_c{Cin}", CONVT_RES_BN
    tile = split_tile_for(mode, U * Cout, 2, Cin, 1)
    return f"split_ups_u{U}_t{tile}", SPLIT_TILES[tile][1]


# (Cin, Cout, U): generic shapes (two row blocks and a second channel chunk, ragged Cout 24 / 20 / 12) ...
CONVT_SHAPES = [(Cin, Cout, U) for U in (2, 4, 8) for Cin, Cout in ((19, 65), (32, 24), (5, 12), (40, 20))]
# ... few enough rows for the 64- and 32-row tile choices at U = 4 and 8 (32 / 64 / 32 rows)
CONVT_SHAPES += [(5, 8, 4), (5, 8, 8), (5, 4, 8)]
# ... and the window-resident x8 form's (f16x3 / bf16; the other modes take their generic form)
CONVT_WINDOW_SHAPES = [(128, 32, 8), (128, 64, 8), (256, 32, 8), (256, 64, 8), (512, 128, 8)]
WINDOW_FRAMES = (63, 64, 65, 127, 128, 129, 257)


def convT_frames(mode: str, Cin: int, Cout: int, U: int) -> List[int]:
    """Input lengths: the columns are frames m in [0, Tin], so the tile's last column is Tin = BN - 1."""
    form, BN = convT_form(mode, Cin, Cout, U)
    t = {1, 2, BN - 2, BN - 1, BN, BN + 1}
    if (Cin, Cout, U) in CONVT_WINDOW_SHAPES:
        t |= set(WINDOW_FRAMES) if Cin < 512 else {64, 65, 129}
    return sorted(t)


def convT_inputs(Cin: int, Cout: int, U: int, Tin: int):
    g = torch.Generator().manual_seed(Cin * 7919 + Cout * 104729 + U * 1299709 + Tin)
    x = _ints(g, -4, 4, B, Cin, Tin)
    x[1] = 0.0
    w = _ints(g, -2, 2, Cin, Cout, 2 * U)
    bias = _ints(g, -3, 3, Cout)
    return x, w, bias


@functools.lru_cache(maxsize=64)
def convT_reference(Cin: int, Cout: int, U: int, Tin: int) -> torch.Tensor:
    x, w, bias = convT_inputs(Cin, Cout, U, Tin)
    return F.conv_transpose1d(F.leaky_relu(x.double(), CONVT_SLOPE), w.double(), bias.double(), stride=U, padding=U // 2)


# ---------------------------------------------------------------------------------------------
# The lines of the library the mirrors above restate, (file under tts-3_amd/csrc, text); the CPU
# test asserts that each still stands there word for word
# ---------------------------------------------------------------------------------------------
SOURCE_LINES = (
    ("kernels_conv.hip", "constexpr int DMAX = 5;"),
    ("kernels_conv.hip", "constexpr int HALO_WIDE = 96;"),
    ("kernels_conv.hip", "if (halo <= (K - 1) * DMAX) {"),
    ("kernels_conv.hip", "} else if (WIDE && halo <= HALO_WIDE) {"),
    ("kernels_conv.hip", "int convT_tile_for(int Cout, int /*U*/) { return Cout > 32 ? 0 : 1; }"),
    ("kernels_conv.hip", "static constexpr ConvTile t[] = {{64, 64, 1, 1, 8}, {32, 128, 1, 1, 8}};"),
    ("kernels_conv.hip", "static constexpr ConvTile t[] = {{64, 128, 1, 2, 8}, {32, 256, 1, 2, 8}};"),
    ("kernels_conv.hip", "static constexpr ConvTile t[] = {{64, 256, 2, 2, 8}, {32, 512, 1, 4, 8}};"),
    ("kernels_conv.hip", "dim3 grid(ceil_div(a.Tin + 1, BN), ceil_div(a.Cout, BM), B);"),
    ("split_kernel.hpp", "if (halo <= (K - 1) * 5) {"),
    ("split_kernel.hpp", "} else if (WIDE && halo <= 96) {"),
    ("kernels_conv_split.hip", "if ((K - 1) * dil > (K - 1) * 5) return Cout > 64 ? 0 : (Cout > 32 ? 1 : 2);  // wide-halo tiles"),
    ("kernels_conv_split.hip", "if (mode == MATH_FP32_F16X3 || (mode == MATH_BF16 && b1_h3_tiles)) {"),
    ("kernels_conv_split.hip", "if (Cout > 64) return 13;"),
    ("kernels_conv_split.hip", "if (Cout > 32) return 10;"),
    ("kernels_conv_split.hip", "return 14;  // one 16-channel group, 42 KB of LDS: 3 workgroups per CU"),
    ("kernels_conv_split.hip", "if (Cout > 64) return (K >= 11 || Cin % 32 != 0) ? 7 : 3;"),
    ("kernels_conv_split.hip", "if (Cout > 32) return K <= 3 ? 10 : 1;"),
    ("kernels_conv_split.hip", "if (a.ups > 0 && convT_res_supported(mode, a)) {"),
    ("kernels_convT_res.hip", "const bool shape = a.ups == 8 && a.Cout % 256 == 0 && (a.Cin == 128 || a.Cin == 256 || (a.Cin == 512 && a.Cout >= 1024));"),
    ("kernels_convT_res.hip", "return (mode == MATH_FP32_F16X3 || mode == MATH_BF16) && shape && a.Tout == a.Tin + 1 && a.pad == 1 &&"),
    ("kernels_convT_res.hip", "static constexpr int BN = WC * TN * 32;      // frames per workgroup"),
    ("kernels_convT_res.hip", "if (a.Cin == 512) launch_res_t<S, 32, 8, 2, 4>(a, B, s);"),
    ("kernels_convT_res.hip", "else if (a.Cin == 256) launch_res_t<S, 16, 8, 2>(a, B, s);"),
    ("kernels_convT_res.hip", "else launch_res_t<S, 8, 8, 2>(a, B, s);"),
    ("abi.cpp", "const int tile = tts::conv_tile_for(math_mode, stride * Cout, 2, Cin, 1, false);"),
    ("abi.cpp", "const int tile = tts::convT_tile_for(Cout, stride);"),
)
