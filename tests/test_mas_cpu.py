"""Glow-TTS alignment surface without a GPU: the new C-ABI entry points validate their arguments
before any HIP call, the size limit is reported with its documented message, and the Python drop-ins
exist, do their host arithmetic right and refuse CPU tensors."""
import ctypes

import pytest
import torch

from tts_amd import _native as N
from tts_amd.tts import GlowTTS


def _buf(n=64):
    """Host memory standing in for a device pointer: never dereferenced on the paths under test."""
    b = ctypes.create_string_buffer(n)
    return b, ctypes.c_void_p(ctypes.addressof(b))


def _status(name, *args):
    st = getattr(N.lib(), name)(*args)
    return st, N.lib().tts_last_error().decode()


def test_mas_logp_rejects_null_and_bad_sizes():
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    good = [p, null, p, 1, 80, 5, 7, p, null]  # o_log_scale may be NULL (mean_only)
    for i in (0, 2, 7):
        a = list(good)
        a[i] = null
        st, msg = _status("tts_glow_mas_logp", *a)
        assert st == N.TTS_ERR_INVALID and "NULL" in msg
    for i in (3, 4, 5, 6):
        for bad in (0, -3):
            a = list(good)
            a[i] = bad
            st, msg = _status("tts_glow_mas_logp", *a)
            assert st == N.TTS_ERR_INVALID and "shape" in msg
    del keep


def test_maximum_path_rejects_null_and_bad_sizes():
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    # value, mask (optional), t_x, t_y, B, T_en, T_de, workspace, path / durations / log_dur (optional), stream
    good = [p, null, p, p, 1, 5, 7, p, null, null, null, null]
    for i in (0, 2, 3, 7):
        a = list(good)
        a[i] = null
        st, msg = _status("tts_maximum_path", *a)
        assert st == N.TTS_ERR_INVALID and "NULL" in msg
    for i in (4, 5, 6):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            st, msg = _status("tts_maximum_path", *a)
            assert st == N.TTS_ERR_INVALID and "shape" in msg
    del keep


def test_maximum_path_limits():
    keep, p = _buf()
    null = ctypes.c_void_p(0)
    st, msg = _status("tts_maximum_path", p, null, p, p, 1, 1025, 7, p, null, null, null, null)
    assert st == N.TTS_ERR_UNSUPPORTED and "more than 1024 tokens" in msg
    st, msg = _status("tts_maximum_path", p, null, p, p, 1, 1024, 1 << 19, p, null, null, null, null)
    assert st == N.TTS_ERR_UNSUPPORTED and "2 GiB" in msg
    lib = N.lib()
    assert lib.tts_maximum_path_workspace_bytes(1, 1025, 7) == -1
    assert lib.tts_maximum_path_workspace_bytes(0, 5, 7) == -1
    # row starts [B][T_en + 1] int32, rounded up to 256 bytes; the decision bits live in LDS up to 96 KiB
    assert lib.tts_maximum_path_workspace_bytes(3, 5, 7) == 256
    assert lib.tts_maximum_path_workspace_bytes(16, 128, 882) == (16 * 129 * 4 + 255) // 256 * 256
    # T_en = 257 runs 8 tokens per lane: 512 words per 32-column chunk, 48 chunks fit
    assert lib.tts_maximum_path_workspace_bytes(1, 257, 1536) == (258 * 4 + 255) // 256 * 256
    assert lib.tts_maximum_path_workspace_bytes(2, 257, 1537) == (2 * 258 * 4 + 255) // 256 * 256 + 2 * 49 * 512 * 4
    del keep


def test_maximum_path_refuses_cpu_tensors():
    from tts_amd.tts import maximum_path
    from tts_amd.tts.helpers import maximum_path as mp2

    assert maximum_path is mp2
    with pytest.raises(RuntimeError, match="runs only on a ROCm device"):
        maximum_path(torch.zeros(1, 3, 4), torch.ones(1, 3, 4))


def test_glow_tts_exposes_the_alignment_entry_points():
    for name in ("forward", "inference_with_MAS", "preprocess"):
        assert callable(getattr(GlowTTS, name)), name
    assert GlowTTS.forward is not torch.nn.Module.forward
    m = GlowTTS(dict(num_chars=20))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.forward(torch.zeros(1, 4, dtype=torch.int64), torch.tensor([4]), torch.zeros(1, 8, 80))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.inference_with_MAS(torch.zeros(1, 4, dtype=torch.int64), torch.tensor([4]), torch.zeros(1, 8, 80))


@pytest.mark.parametrize("T,lens,want_T,want_lens", [
    (117, [117, 116, 1, 0, 33], 116, [116, 116, 0, 0, 32]),   # odd: one frame dropped
    (116, [116, 115, 2, 3, 64], 116, [116, 114, 2, 2, 64]),   # even: kept
])
def test_preprocess_arithmetic(T, lens, want_T, want_lens):
    m = GlowTTS(dict(num_chars=20))
    assert m.num_squeeze == 2
    y = torch.arange(2 * 3 * T, dtype=torch.float32).reshape(2, 3, T)
    attn = torch.arange(2 * 5 * T, dtype=torch.float32).reshape(2, 1, 5, T)
    y2, l2, T2, a2 = m.preprocess(y, torch.tensor(lens), T, attn)
    assert T2 == want_T
    assert torch.equal(y2, y[:, :, :want_T]) and torch.equal(a2, attn[:, :, :, :want_T])
    assert l2.tolist() == want_lens
    y3, l3, T3, a3 = m.preprocess(y, torch.tensor(lens), None)
    assert T3 is None and a3 is None and y3.shape[2] == T and l3.tolist() == want_lens


def test_preprocess_other_squeeze():
    m = GlowTTS(dict(num_chars=20, num_squeeze=1))
    y = torch.zeros(1, 3, 7)
    y2, l2, T2, _ = m.preprocess(y, torch.tensor([7]), 7)
    assert T2 == 7 and y2.shape[2] == 7 and l2.tolist() == [7]
