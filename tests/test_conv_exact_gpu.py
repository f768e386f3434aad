"""Exact-integer edge tests of the base conv kernels on MI355X (cases: ``_conv_exact.py``).

a. ``test_conv1d_exact[mode-tile]``: every case of the (mode, tile) pair through
   ``tts_op_conv1d_bench(..., tile, reps = 0)`` into a NaN-filled output, bitwise against the fp64
   reference.  fp32 tiles {0, 1, 2, 3, 4, 8, 10, 11}, split tiles 0-19 in fp32x6, f16x3 and bf16.
b. ``test_refusals``: a halo past the tile's limit, an fp32 tile that is not built and a split tile
   past the table return ``TTS_ERR_UNSUPPORTED``, name the limit and leave the output untouched.
c. ``test_conv_transpose1d_exact``: the same integer recipe (``in_slope`` 0.5) through
   ``tts_op_conv_transpose1d`` in all four modes, bitwise against fp64 ``F.conv_transpose1d``.
   Which shape reaches which form (``_conv_exact.convT_form``, from ``convT_tile_for``,
   ``conv_tile_for(mode, U * Cout, 2, Cin, 1, false)``, ``convT_res_supported`` and the ``ups`` path
   of ``launch_conv1d_split``), with the frames per workgroup BN:

   * fp32, polyphase ``convT_mfma_kernel``: Cout 65 -> tile 0 (BN 64 / 128 / 256 at U = 8 / 4 / 2),
     Cout 24, 12, 20 (ragged), 8, 4 -> tile 1 (BN 128 / 256 / 512); the window shapes Cout 32 -> tile 1,
     Cout 64, 128 -> tile 0;
   * split ``ups`` form (``conv1d_split_kernel<K = 2>``) on the default tile of U * Cout rows:
     f16x3 -> 13 (> 64 rows, BN 128), 10 (> 32, BN 256), 14 (BN 256); fp32x6 and bf16 -> 7 (> 64 rows,
     Cin % 32 != 0), 3 (> 64 rows, Cin 32), 10 (> 32 rows), 2 (BN 512).  (Cin, Cout) = (19, 65) gives
     130 / 260 / 520 rows, (32, 24) 48 / 96 / 192, (5, 12) 24 / 48 / 96, (40, 20) 40 / 80 / 160, and
     (5, 8) at U = 4 / 8 and (5, 4) at U = 8 the 32- and 64-row classes there;
   * window-resident x8 form (``convT_res_kernel``, 64-frame windows; f16x3 and bf16): Cin 128 and 256
     with Cout 32 (one 256-row pass) and 64 (two), Cin 512 with Cout 128 (four passes split over four
     workgroups per window).  In fp32x6 the same shapes take the ``ups`` form on tile 3.

   Frame counts: the columns are frames m in [0, Tin], so Tin in {1, 2, BN - 2, BN - 1, BN, BN + 1}, and
   for the window shapes also {63, 64, 65, 127, 128, 129, 257} (Cin 512: {64, 65, 129}).
d. ``test_conv1d_random[mode-tile]``: the integer data leaves the low split pieces at zero, so one
   random case per (mode, tile) at the suite's ``tol(mode, op=True)`` gates.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_exact as X
from _util import assert_close_fp32, tol
from tts_amd import _native as N

pytestmark = pytest.mark.gpu
MT_IDS = [f"{m}-{t}" for m, t in X.MODE_TILES]


def first_difference(out: torch.Tensor, ref: torch.Tensor) -> str:
    bad = torch.nonzero(out.double() != ref)  # NaN != x holds, so an unwritten element counts
    b, r, t = bad[0].tolist()
    return (f"{len(bad)} of {ref.numel()} differ, first at (b={b}, row={r}, column={t}): got {out[b, r, t].item()!r}, "
            f"want {ref[b, r, t].item()!r}")


def run_conv(dev, mode, tile, c, x, w, bias, res, z0):
    """One launch into a NaN-filled output; returns (status, the output on the host)."""
    d = N.TtsConv1dDesc(x.shape[0], c.Cin, c.Cout, c.T, c.K, c.dil, c.rep, c.in_slope, c.out_slope, c.zmode, X.ZDIV,
                        N.MATH_MODES[mode])
    shape = (x.shape[0], c.Cout, c.Tout)
    y = torch.full(shape, float("nan"), device=dev) if c.zmode == 0 else None
    z = None if c.zmode == 0 else (z0.to(dev) if c.zmode >= 2 else torch.full(shape, float("nan"), device=dev))
    resd = res.to(dev) if res is not None else None
    wn, bn, xd = w.numpy(), bias.numpy(), x.to(dev)
    st = N.lib().tts_op_conv1d_bench(ctypes.byref(d), N.ptr(xd), N.ptr(wn), N.ptr(bn), N.ptr(resd), N.ptr(y),
                                     N.ptr(z), tile, 0, None, N.stream_ptr(dev))
    return st, (y if c.zmode == 0 else z).cpu()


# ----------------------------------------------------------------------------- a. exact conv1d
@pytest.mark.parametrize("mode,tile", X.MODE_TILES, ids=MT_IDS)
def test_conv1d_exact(cuda_device, mode, tile):
    for c in X.cases_of(mode, tile):
        ref = X.reference(c)
        st, out = run_conv(cuda_device, mode, tile, c, *X.inputs(c))
        N.check(f"tts_op_conv1d_bench ({mode} tile {tile}: {c})", st)
        assert out.shape == ref.shape
        assert torch.equal(out.double(), ref), f"{mode} tile {tile} {c}: {first_difference(out, ref)}"


# ----------------------------------------------------------------------------- b. refusals
def _narrow_and_wide(mode):
    tiles = X.tiles_of(mode)
    return [t for t, v in tiles.items() if not v[3]], [t for t, v in tiles.items() if v[3]]


@pytest.mark.parametrize("mode", X.MODES)
def test_refusals(cuda_device, mode):
    narrow, wide = _narrow_and_wide(mode)
    unbuilt = X.FP32_UNBUILT[0] if mode == "fp32" else X.SPLIT_TABLE_SIZE
    assert unbuilt == (5 if mode == "fp32" else 22)
    cases = [(t, 3, 6, ("= 12 ", "exceeds 10 ")) for t in narrow]
    cases += [(t, 3, 49, ("= 98 ", "exceeds 96 ")) for t in wide]
    cases += [(unbuilt, 3, 1, ("bad tile index",))]
    for tile, K, dil, words in cases:
        BM, BN, CK = X.tiles_of(mode).get(tile, (32, 128, 16, False))[:3]
        c = X.Case(BM, BN, CK, 5, 31, K, dil, BN + 1, 0, "plain", 1.0, 1.0, False, 0)
        x, w, bias, _, _ = X.inputs(c)
        d = N.TtsConv1dDesc(X.B, c.Cin, c.Cout, c.T, K, dil, 0, 1.0, 1.0, 0, X.ZDIV, N.MATH_MODES[mode])
        y, xd = torch.full((X.B, c.Cout, c.T), 12345.0, device=cuda_device), x.to(cuda_device)
        st = N.lib().tts_op_conv1d_bench(ctypes.byref(d), N.ptr(xd), N.ptr(w.numpy()), N.ptr(bias.numpy()),
                                         None, N.ptr(y), None, tile, 0, None, N.stream_ptr(cuda_device))
        msg = N.lib().tts_last_error().decode()
        what = f"{mode} tile {tile} K={K} dil={dil}"
        assert st == N.TTS_ERR_UNSUPPORTED, f"{what}: status {st} ({msg})"
        assert all(s in msg for s in words), f"{what}: {msg!r}"
        torch.cuda.synchronize(cuda_device)
        assert bool((y == 12345.0).all()), f"{what}: a refused launch wrote to its output"
    # the halo just inside the limit is taken (the wide one: K = 3, dil = 48 is halo 96)
    for tile, dil in [(narrow[0], 5), (wide[0], 48)]:
        BM, BN, CK = X.tiles_of(mode)[tile][:3]
        c = X.Case(BM, BN, CK, 5, 31, 3, dil, BN + 1, 0, "plain", 1.0, 1.0, False, 0)
        x, w, bias, res, z0 = X.inputs(c)
        st, out = run_conv(cuda_device, mode, tile, c, x, w, bias, res, z0)
        N.check(f"{mode} tile {tile} dil={dil}", st)
        ref = X.conv_reference(x, w, bias, None, z0, dil=dil, rep=0, in_slope=1.0, out_slope=1.0, zmode=0)
        assert torch.equal(out.double(), ref), f"{mode} tile {tile} K=3 dil={dil}: {first_difference(out, ref)}"


# ----------------------------------------------------------------------------- c. exact ConvTranspose1d
CONVT = [(m, s) for s in X.CONVT_SHAPES + X.CONVT_WINDOW_SHAPES for m in X.MODES]  # a shape's modes share references


@pytest.mark.parametrize("mode,shape", CONVT, ids=[f"{m}-{X.convT_form(m, *s)[0]}-c{s[0]}x{s[1]}" for m, s in CONVT])
def test_conv_transpose1d_exact(cuda_device, mode, shape):
    Cin, Cout, U = shape
    form, BN = X.convT_form(mode, Cin, Cout, U)
    for Tin in X.convT_frames(mode, Cin, Cout, U):
        x, w, bias = X.convT_inputs(Cin, Cout, U, Tin)
        ref = X.convT_reference(Cin, Cout, U, Tin)
        y, xd = torch.full((X.B, Cout, U * Tin), float("nan"), device=cuda_device), x.to(cuda_device)
        N.call("tts_op_conv_transpose1d", N.ptr(xd), X.B, Cin, Tin, N.ptr(w.numpy()), N.ptr(bias.numpy()),
               Cout, 2 * U, U, X.CONVT_SLOPE, N.MATH_MODES[mode], N.ptr(y), N.stream_ptr(cuda_device))
        out = y.cpu()
        assert torch.equal(out.double(), ref), \
            f"{mode} {form} (BN {BN}) Cin={Cin} Cout={Cout} U={U} Tin={Tin}: {first_difference(out, ref)}"


# ----------------------------------------------------------------------------- d. random complement
@pytest.mark.parametrize("mode,tile", X.MODE_TILES, ids=MT_IDS)
def test_conv1d_random(cuda_device, mode, tile):
    """Gaussian data (every split piece in use) on every tile: two row blocks, six, three or two channel
    chunks (the last one half full at CK = 32), two column tiles, residual."""
    BM, BN, CK, _ = X.tiles_of(mode)[tile]
    c = X.Case(BM, BN, CK, 48, BM + 1, 5, 2, BN + 7, 0, "random", 0.1, 1.0, True, 0)
    g = torch.Generator().manual_seed(100 * tile + BN)
    x = torch.randn(2, c.Cin, c.T, generator=g)
    w = torch.randn(c.Cout, c.Cin, c.K, generator=g) / np.sqrt(c.Cin * c.K)
    bias = torch.randn(c.Cout, generator=g) * 0.1
    res = torch.randn(2, c.Cout, c.T, generator=g)
    v = F.conv1d(F.leaky_relu(x.double(), c.in_slope), w.double(), bias.double(), dilation=c.dil, padding=c.pad)
    ref = v + res.double()
    st, out = run_conv(cuda_device, mode, tile, c, x, w, bias, res, None)
    N.check(f"tts_op_conv1d_bench ({mode} tile {tile})", st)
    assert_close_fp32(out, ref, f"conv_exact random {mode} tile {tile}", **tol(mode, op=True))
