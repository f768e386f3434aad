"""Single ops of the speaker encoder through the C-ABI (``tts_op_conv2d_3x3``)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _native as N


def _host(t, n: int, what: str) -> Optional[np.ndarray]:
    if t is None:
        return None
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
    if a.shape != (n,):
        raise ValueError(f"{what} must have shape ({n},), got {a.shape}")
    return a


def conv2d_tile() -> int:
    """Output columns one workgroup of the Conv2d kernel computes."""
    return N.lib().tts_op_conv2d_3x3_tile()


def conv2d_3x3(x: torch.Tensor, w: torch.Tensor, bias=None, stride: int = 1, relu: bool = False, scale=None,
               shift=None, math_mode: Optional[str] = None) -> torch.Tensor:
    """``scale * act(F.conv2d(x, w, bias, stride, padding=(k - 1) // 2)) + shift`` in one launch, with
    ``act`` = ReLU (``relu``) or the identity and ``scale`` / ``shift`` per output channel (an
    eval-mode BatchNorm after the ReLU).  ``x`` [B, Cin, F, T] is a device tensor; ``w``
    [Cout, Cin, k, k] with k = 3 (pad 1) or 1 (pad 0, the ``downsample`` conv) and the per-channel
    vectors may live anywhere (they are packed on the host).  ``math_mode``: ``"bf16"``, or any
    fp32-faithful name (all of them run the fp32x6 kernel)."""
    N.require_device_tensor(x, "conv2d_3x3 input")
    if x.dim() != 4 or w.dim() != 4 or w.shape[2] != w.shape[3] or w.shape[1] != x.shape[1]:
        raise ValueError(f"conv2d_3x3: x {tuple(x.shape)} and w {tuple(w.shape)} do not form a square-kernel Conv2d")
    mode = math_mode if math_mode is not None else N.default_math_mode()
    if mode not in N.MATH_MODES:
        raise ValueError(f"math_mode={mode!r}: must be one of {sorted(N.MATH_MODES)}")
    B, Cin, F, T = x.shape
    Cout, _, k, _ = w.shape
    stride = int(stride)
    xd = x.to(torch.float32).contiguous()
    hw = np.ascontiguousarray(w.detach().cpu().numpy(), dtype=np.float32)
    hb, hs, ht = _host(bias, Cout, "bias"), _host(scale, Cout, "scale"), _host(shift, Cout, "shift")
    Fo, To = (-(-F // stride), -(-T // stride)) if stride >= 1 else (0, 0)
    out = torch.empty((B, Cout, Fo, To), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        N.call("tts_op_conv2d_3x3", N.ptr(xd), B, Cin, F, T, N.ptr(hw), Cout, k, stride, N.ptr(hb), int(bool(relu)),
               N.ptr(hs), N.ptr(ht), N.MATH_MODES[mode], N.ptr(out), N.stream_ptr(x.device))
    return out
