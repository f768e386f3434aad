"""The LSTM / skinny-product packer of Tacotron2 (tts-3_amd/csrc/pack.cpp: pack_lstm, pack_lstm_bias,
pack_skinny_rows) under AddressSanitizer + UBSan: `make -C tts-3_amd asan-check-tacotron2` builds
csrc/pack.cpp with the stand-alone tests_native/lstm_pack_check.cpp (host code only), packs (H, I) =
(8, 5), (40, 24), (96, 160), (256, 512), (1024, 1792), fp32 and bf16, with and without padded columns,
into buffers of exactly the advertised size and decodes them back against the torch weights."""
import os
import shutil
import subprocess

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd")


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/llvm/bin/clang++"),
                    reason="needs make and the ROCm clang++")
def test_lstm_packer_clean_under_asan_ubsan():
    r = subprocess.run(["make", "-C", PKG, "asan-check-tacotron2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "LSTM packer OK" in r.stdout
