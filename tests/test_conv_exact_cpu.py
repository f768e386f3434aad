"""The cases of ``test_conv_exact_gpu.py`` are what that test's argument needs them to be.

Nothing here runs a kernel:

* the tile mirrors of ``_conv_exact`` are compared with ``kConvTiles`` / ``kSplitTiles`` and with the
  ``case N:`` lists of ``launch_conv1d_k`` / ``launch_split_k`` parsed from the sources (which fp32
  indices are built, which tiles are ``WIDE``), and the dispatch lines the ConvTranspose1d forms
  are derived from still stand word for word;
* for every case: every operand (after the leaky-ReLU) has at most 8 significant bits,
  ``sum |w| |lrelu(x)| + |bias| + |res| + |z0|`` stays below 2^24 of the smallest step (2^-6: the
  value after ``out_slope`` 0.25 and ``/ 4``), and the fp64 reference round-trips through fp32;
* every (32-row block, CK-channel group, tap) of every weight tensor holds a nonzero, and no output
  row is all zero;
* every (mode, tile) meets every epilogue, every K, and a length from each of the classes
  ``< pad``, ``BN - 1``, ``BN``, ``BN + 1``, ``> 2 BN``;
* a dropped tap, an input shifted by one column and zero padding in place of replication each move
  an output of the numpy reference in the last kept column of a tile, so the GPU test would see them.
"""
import os
import re

import numpy as np
import pytest
import torch

import _conv_exact as X

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd", "csrc")
STEP = 2.0 ** -6
GEOMETRIES = sorted({t for m in X.MODES for t in X.tiles_of(m).values()})


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _table(text, name):
    """[(BM, BN, TM, TN, CK, PD), ...] of ``constexpr ConvTile <name>[] = {...};``."""
    body = re.search(r"constexpr ConvTile %s\[\] = \{\n(.*?)\n\};" % name, text, re.S).group(1)
    rows = []
    for i, line in enumerate(body.split("\n")):
        m = re.match(r"\s*\{([0-9, ]+)\},\s*// (\d+)", line)
        assert m and int(m.group(2)) == i, f"{name}: row {i} is {line!r}"
        v = [int(s) for s in m.group(1).split(",")]
        rows.append(tuple(v[:5]) + (v[5] if len(v) > 5 else 1,))
    return rows


def _cases(text, fn, extra):
    """{tile: (BM, BN, TM, TN, G, PD, wide)} of the ``case N: <fn><...>`` lines, in two parts: the ones
    that are always built and the ones behind ``#ifdef TTS_TUNING_TILES``."""
    pat = re.compile(r"case (\d+): %s<%sK, (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false)[,>]" % (fn, extra))
    built, tuning, guarded = {}, {}, False
    for line in text.split("\n"):
        if line.startswith("#ifdef TTS_TUNING_TILES"):
            guarded = True
        elif line.startswith("#endif"):
            guarded = False
        m = pat.search(line)
        if m:
            v = m.groups()
            (tuning if guarded else built)[int(v[0])] = tuple(int(s) for s in v[1:7]) + (v[7] == "true",)
    return built, tuning


def test_fp32_tile_mirror():
    text = _read("kernels_conv.hip")
    table = _table(text, "kConvTiles")
    built, tuning = _cases(text, "launch_conv1d_t", "")
    assert len(table) == X.FP32_TABLE_SIZE
    assert sorted(built) == sorted(X.FP32_TILES) and sorted(tuning) == sorted(X.FP32_UNBUILT)
    assert sorted(list(built) + list(tuning)) == list(range(len(table)))
    with open(os.path.join(os.path.dirname(CSRC), "Makefile")) as fh:
        assert "TTS_TUNING_TILES" not in fh.read(), "the tuning tiles are built: add them to _conv_exact.FP32_TILES"
    for idx, (BM, BN, TM, TN, G, PD, wide) in {**built, **tuning}.items():
        assert table[idx] == (BM, BN, TM, TN, 8 * G, PD), f"kConvTiles[{idx}] against its launch case"
    for idx, mirror in X.FP32_TILES.items():
        BM, BN, TM, TN, G, PD, wide = built[idx]
        assert mirror == (BM, BN, 8 * G, wide), f"fp32 tile {idx}"


def test_split_tile_mirror():
    table = _table(_read("kernels_conv_split.hip"), "kSplitTiles")
    built, tuning = _cases(_read("split_kernel.hpp"), "launch_split_t", "S, ")
    assert len(table) == X.SPLIT_TABLE_SIZE and not tuning
    assert sorted(built) == sorted(X.SPLIT_TILES) == list(range(20))
    for idx, mirror in X.SPLIT_TILES.items():
        BM, BN, TM, TN, G, PD, wide = built[idx]
        assert table[idx] == (BM, BN, TM, TN, 16 * G, PD), f"kSplitTiles[{idx}] against its launch case"
        assert mirror == (BM, BN, 16 * G, wide), f"split tile {idx}"
    assert "static_assert(kSplitGateTile == 20 && kSplitWinoTile == 21" in _read("kernels_conv_split.hip")


def test_source_lines():
    text = {}
    for fname, line in X.SOURCE_LINES:
        if fname not in text:
            text[fname] = _read(fname)
        assert line in text[fname], f"{fname} no longer holds {line!r}: re-derive the mirror in _conv_exact.py"


def _sig_bits(a: np.ndarray) -> int:
    """Most significant bits any element of ``a`` needs (0 for an all-zero array)."""
    a = np.abs(np.asarray(a, np.float64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 0
    m, _ = np.frexp(a)            # m in [0.5, 1)
    n = (m * 2.0 ** 53).astype(np.int64)
    low = n & -n                  # lowest set bit
    return int(np.max(53 - np.log2(low.astype(np.float64)).astype(np.int64)))


def _lrelu(a, slope):
    return np.where(a > 0, a, a * slope)


@pytest.mark.parametrize("geo", GEOMETRIES, ids=[f"{g[0]}x{g[1]}x{g[2]}{'w' if g[3] else ''}" for g in GEOMETRIES])
def test_cases_are_exact_and_cover_the_weights(geo):
    BM, BN, CK, wide = geo
    worst = 0.0
    for c in X.cases(*geo):
        x, w, bias, res, z0 = (None if t is None else t.numpy() for t in X.inputs(c))
        assert x.shape == (X.B, c.Cin, c.T) and not x[1].any() and x[0].any() and x[2].any(), str(c)
        a = _lrelu(x.astype(np.float64), c.in_slope)
        for name, v in (("lrelu(x)", a), ("w", w), ("bias", bias), ("res", res), ("z0", z0)):
            if v is not None:
                assert _sig_bits(v) <= 8, f"{c}: {name} needs {_sig_bits(v)} bits"
        # a bound on every partial sum, in units of the smallest step
        bound = np.abs(w).sum(axis=(1, 2)).max() * np.abs(a).max() + np.abs(bias).max() + 3.0 + 3.0
        worst = max(worst, bound / STEP)
        assert bound / STEP < 2.0 ** 24, str(c)
        ref = X.reference(c)
        assert ref.shape == (X.B, c.Cout, c.Tout), str(c)
        assert torch.equal(ref.float().double(), ref), f"{c}: the reference does not round-trip through fp32"
        assert torch.equal(ref / STEP, torch.round(ref / STEP)), f"{c}: the reference is no multiple of 2^-6"
        # weights: every (32-row block, CK-channel group, tap) and every row
        wz = w != 0
        for r0 in range(0, c.Cout, 32):
            for c0 in range(0, c.Cin, CK):
                assert wz[r0:r0 + 32, c0:c0 + CK].any(axis=(0, 1)).all(), f"{c}: empty block at row {r0}, channel {c0}"
        assert wz.any(axis=(1, 2)).all(), f"{c}: an all-zero output row"
    assert worst < 2.0 ** 24


def test_reference_matches_numpy():
    """torch's fp64 conv against the tap-by-tap numpy form, on the smallest geometry."""
    for c in X.cases(32, 128, 16, False):
        x, w, bias, res, z0 = X.inputs(c)
        v = X.numpy_reference(x, w, bias, res, z0, dil=c.dil, rep=c.rep, in_slope=c.in_slope, out_slope=c.out_slope,
                              zmode=c.zmode)
        assert np.array_equal(v, X.reference(c).numpy()), str(c)


@pytest.mark.parametrize("mode,tile", X.MODE_TILES, ids=[f"{m}-{t}" for m, t in X.MODE_TILES])
def test_case_coverage(mode, tile):
    BM, BN, CK, wide = X.tiles_of(mode)[tile]
    cs = X.cases_of(mode, tile)
    assert {c.epi for c in cs} == set(X.ALL_EPILOGUES)
    assert {c.K for c in cs} == set(X.KS)
    for K in X.KS:
        want = set(X.ROTATED) | ({"rep_pad"} if K == 7 else set())
        assert {c.epi for c in cs if c.K == K} == want, f"K={K}"
    assert {n for c in cs for n in X.length_classes(c)} == {"<pad", "BN-1", "BN", "BN+1", ">2BN"}
    for K in X.KS[1:]:  # and per kernel size with a halo
        assert {n for c in cs if c.K == K for n in X.length_classes(c)} == {"<pad", "BN-1", "BN", "BN+1", ">2BN"}, K
    halos = {(c.K - 1) * c.dil for c in cs}
    assert {(K - 1) * X.NARROW_DMAX for K in (3, 7, 11)} <= halos
    assert (X.HALO_WIDE in halos and 90 in halos) == wide and max(halos) == (X.HALO_WIDE if wide else 50)
    shapes = {(c.Cin, c.Cout) for c in cs}
    assert shapes == {(CK + 3, BM + 1), (5, 31)}
    assert {c.in_slope for c in cs} == {c.out_slope for c in cs} == set(X.SLOPES)
    assert all(c.rep == (X.REP_PAD if c.epi == "rep_pad" else 0) for c in cs)
    assert {c.T for c in cs if c.epi == "rep_pad"} >= {1, 2, BN - 10, BN - 11, BN - 9}
    # at most about 130 x 48 x 1100 floats per tensor
    assert max(max(c.Cin, c.Cout) * c.Tout for c in cs) <= 130 * 1100


def test_case_counts():
    n = {m: sum(len(X.cases_of(m, t)) for t in X.tiles_of(m)) for m in X.MODES}
    assert n["fp32x6"] == n["f16x3"] == n["bf16"]
    assert n == {"fp32": 3 * 146 + 5 * 110, "fp32x6": 3 * 146 + 17 * 110, "f16x3": 3 * 146 + 17 * 110,
                 "bf16": 3 * 146 + 17 * 110}


@pytest.mark.parametrize("epi,tiles", [("zmode2_res", 2), ("rep_pad", 1)])
def test_sensitivity(epi, tiles):
    """Three mistakes a kernel could make, applied to the numpy reference of one case (two tiles and
    a column; under replicate padding exactly one tile, so that the padded margin holds the tile's
    last column): each moves outputs, among them one in every tile's last kept column."""
    BM, BN, CK = 32, 128, 16
    c = next(c for c in X.cases(BM, BN, CK, False) if c.epi == epi and c.Tout == tiles * BN + (tiles > 1)
             and c.Cout == BM + 1 and c.K > 1)
    x, w, bias, res, z0 = X.inputs(c)
    kw = dict(dil=c.dil, rep=c.rep, in_slope=c.in_slope, out_slope=c.out_slope, zmode=c.zmode)
    good = X.numpy_reference(x, w, bias, res, z0, **kw)
    assert np.array_equal(good, X.reference(c).numpy())
    last = [n * BN - 1 for n in range(1, tiles + 1)]
    # the centre tap: the outer ones read the zero padding at a tile's last column near the end
    mistakes = {"dropped tap": dict(drop_tap=c.K // 2), "shifted input": dict(shift=1)}
    if c.rep:
        mistakes["zero padding"] = dict(zero_pad=True)
    for name, m in mistakes.items():
        bad = X.numpy_reference(x, w, bias, res, z0, **kw, **m)
        diff = bad != good
        n = int(diff.sum())
        print(f"{c.epi} {name}: {n} of {diff.size} outputs differ")
        assert n > 0, name
        if name == "zero padding":
            # only the replicated margins and the taps that reach them: both ends, nothing between
            cols = np.nonzero(diff.any(axis=(0, 1)))[0]
            assert cols.min() < c.rep + c.pad and cols.max() >= c.Tout - c.rep - c.pad, name
            assert not diff[:, :, c.rep + c.pad:c.Tout - c.rep - c.pad].any(), name
        else:
            assert n > diff.size // 3, name
        assert all(diff[:, :, t].any() for t in last), f"{name}: no output moves in columns {last}"


def test_convT_forms():
    """Every form ``tts_op_conv_transpose1d`` dispatches to is reached, and the shapes are exact."""
    forms = {m: {} for m in X.MODES}
    for m in X.MODES:
        for s in X.CONVT_SHAPES + X.CONVT_WINDOW_SHAPES:
            forms[m].setdefault(X.convT_form(m, *s)[0], []).append(s)
    assert {f"fp32_poly_u{U}_t{t}" for U in (2, 4, 8) for t in (0, 1)} <= set(forms["fp32"])
    for m, tiles in (("f16x3", (13, 10, 14)), ("fp32x6", (7, 3, 10, 2)), ("bf16", (7, 3, 10, 2))):
        got = {f for f in forms[m] if f.startswith("split_ups")}
        assert {int(f.rsplit("t", 1)[1]) for f in got} == set(tiles), (m, got)
        assert got == {f"split_ups_u{U}_t{t}" for U in (2, 4, 8) for t in tiles if (U, t) != (2, 3)}, (m, got)
    for m in ("f16x3", "bf16"):
        assert {"window_x8_c128", "window_x8_c256", "window_x8_c512"} <= set(forms[m])
        assert sorted(forms[m]["window_x8_c128"] + forms[m]["window_x8_c256"] + forms[m]["window_x8_c512"]) == sorted(X.CONVT_WINDOW_SHAPES)
    assert not any(f.startswith("window") for m in ("fp32", "fp32x6") for f in forms[m])
    for Cin, Cout, U in X.CONVT_SHAPES + X.CONVT_WINDOW_SHAPES:
        for m in X.MODES:
            _, BN = X.convT_form(m, Cin, Cout, U)
            assert {1, 2, BN - 2, BN - 1, BN, BN + 1} <= set(X.convT_frames(m, Cin, Cout, U))
        Tin = max(X.convT_frames("f16x3", Cin, Cout, U))
        x, w, bias = X.convT_inputs(Cin, Cout, U, Tin)
        assert not x[1].any() and _sig_bits(_lrelu(x.numpy().astype(np.float64), X.CONVT_SLOPE)) <= 8
        assert (2 * Cin * 2 * 4 + 3) * 2 < 2.0 ** 24  # in halves
        ref = X.convT_reference(Cin, Cout, U, Tin)
        assert ref.shape == (X.B, Cout, U * Tin) and torch.equal(ref.float().double(), ref)
    assert any(Cout in (24, 20) for _, Cout, _ in X.CONVT_SHAPES)
