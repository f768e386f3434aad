"""The epilogue of the 8-wave Winograd conv (wino8_kernel.hpp) at op level, f16x3, B = 2.

The epilogue takes one of several compiled paths, chosen per workgroup: the pair exchange of one
point group or the other; then, per (residual, zmode), the whole-tile path (16-byte vectors only,
with or without the output activation) or, for the last column tile, the per-sample path; and the
direct stores of dilation 1 or the LDS transpose of dilations 3 and 5.  The cases cross what
selects a path:

* dilation 1 / 3 / 5 (workgroups of TW = 256 / 252 / 240 samples);
* lengths 4, TW - 4, TW, TW + 4 and 2 TW + 8: a lone partial tile, a lone whole tile, and a 1- or
  2-vector last tile behind one or two whole ones (all multiples of 4: the 8-wave kernel runs);
* the epilogue forms: convs1 (no residual, out_slope 0.1), convs2 (residual, out_slope 1) with
  zmode 0 / 2 / 3, zmode 1 without a residual, and a conditioning vector.

Channels (128: one 128-row tile, 256: two) and kernel size (7, 11) do not select an epilogue path;
their four combinations rotate over the cases so that each meets every dilation, every length
class and every form.

Gate: the fp64 reference of _conv_exact.conv_reference under the fp32 op gates of _util.py (the
gate of test_op_conv1d_winograd).  Bitwise: item 1 of the batch equals the same item run alone,
and a second run equals the first.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _conv_exact import conv_reference
from _util import assert_close_fp32
from tts_amd import _native as N

pytestmark = pytest.mark.gpu

WINO_TILE = 21  # kSplitWinoTile (common.hpp)
ZDIV = 3.0
B = 2
TW = {1: 256, 3: 252, 5: 240}  # Wino8Cfg::TW
SHAPES = ((128, 7), (256, 11), (128, 11), (256, 7))  # (channels, kernel size)
FORMS = {
    # name: in_slope, out_slope, residual, zmode, cvec
    "convs1": (0.1, 0.1, False, 0, False),
    "convs2_z0": (1.0, 1.0, True, 0, False),
    "convs2_z2": (1.0, 1.0, True, 2, False),
    "convs2_z3": (1.0, 1.0, True, 3, False),
    "zinit": (0.1, 0.1, False, 1, False),
    "cvec": (0.1, 0.1, False, 0, True),
}


def lengths(dil):
    tw = TW[dil]
    return (4, tw - 4, tw, tw + 4, 2 * tw + 8)


CASES = []
for _i, _dil in enumerate((1, 3, 5)):
    for _j, _T in enumerate(lengths(_dil)):
        for _k, _form in enumerate(FORMS):
            _C, _K = SHAPES[(_i + _j + _k) % 4]
            CASES.append((_C, _K, _dil, _T, _form))


def test_case_table():
    """Every (channels, kernel size) meets every dilation, every length class and every form."""
    for shape in SHAPES:
        mine = [c for c in CASES if (c[0], c[1]) == shape]
        assert {c[2] for c in mine} == {1, 3, 5}
        assert {lengths(c[2]).index(c[3]) for c in mine} == set(range(5))
        assert {c[4] for c in mine} == set(FORMS)
    assert len(set(CASES)) == len(CASES) == 3 * 5 * len(FORMS)
    assert all(c[3] % 4 == 0 for c in CASES)


@functools.lru_cache(maxsize=None)
def _weights(C, K):
    g = torch.Generator().manual_seed(100 * C + K)
    w = torch.randn(C, C, K, generator=g) / np.sqrt(C * K)
    b = torch.randn(C, generator=g) * 0.1
    return w, b


def _run(dev, x, w, b, res, z0, cvec, dil, s_in, s_out, zmode):
    nb, C, T = x.shape
    d = N.TtsConv1dDesc(nb, C, C, T, w.shape[2], dil, 0, s_in, s_out, zmode, ZDIV, N.MATH_MODES["f16x3"])
    y = torch.full((nb, C, T), float("nan"), device=dev)
    z = z0.to(dev)
    resd = res.to(dev) if res is not None else None
    wn, bn = w.numpy().copy(), b.numpy().copy()
    if cvec is None:
        N.call("tts_op_conv1d_bench", ctypes.byref(d), N.ptr(x.to(dev)), N.ptr(wn), N.ptr(bn), N.ptr(resd), N.ptr(y),
               N.ptr(z), WINO_TILE, 0, None, N.stream_ptr(dev))
    else:
        cv = cvec.to(dev)
        N.call("tts_op_conv1d_cvec", ctypes.byref(d), N.ptr(x.to(dev)), N.ptr(wn), N.ptr(bn), N.ptr(cv), N.ptr(resd),
               N.ptr(y), N.ptr(z), WINO_TILE, N.stream_ptr(dev))
    return (y if zmode == 0 else z).cpu()


@pytest.mark.parametrize("case", CASES, ids=[f"c{c[0]}k{c[1]}d{c[2]}t{c[3]}-{c[4]}" for c in CASES])
def test_wino_epilogue(cuda_device, case):
    C, K, dil, T, form = case
    s_in, s_out, use_res, zmode, use_cvec = FORMS[form]
    w, b = _weights(C, K)
    g = torch.Generator().manual_seed(hash(case[:4]) & 0xFFFF)
    x = torch.randn(B, C, T, generator=g) * 2
    res = torch.randn(B, C, T, generator=g) if use_res else None
    z0 = torch.randn(B, C, T, generator=g)
    cvec = torch.randn(B, C, generator=g) * 0.5 if use_cvec else None
    kw = dict(dil=dil, rep=0, in_slope=s_in, out_slope=s_out, zmode=zmode, zdiv=ZDIV)
    if cvec is None:
        ref = conv_reference(x, w, b, res, z0, **kw)
    else:  # the vector joins the bias of its batch item
        ref = torch.cat([conv_reference(x[i:i + 1], w, b + cvec[i], None, z0[i:i + 1], **kw) for i in range(B)])
    out = _run(cuda_device, x, w, b, res, z0, cvec, dil, s_in, s_out, zmode)
    assert_close_fp32(out, ref, f"winograd epilogue {case}")
    again = _run(cuda_device, x, w, b, res, z0, cvec, dil, s_in, s_out, zmode)
    assert torch.equal(again, out), "run-to-run"
    alone = _run(cuda_device, x[1:], w, b, res[1:] if use_res else None, z0[1:], cvec[1:] if use_cvec else None, dil,
                 s_in, s_out, zmode)
    assert torch.equal(alone[0], out[1]), "batch invariance"
