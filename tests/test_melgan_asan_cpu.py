"""The MelGAN residual-block packer (tts-3_amd/csrc/pack.cpp, pack_melgan_block) under
AddressSanitizer + UBSan: `make -C tts-3_amd asan-check-melgan` builds csrc/pack.cpp with the
stand-alone tests_native/melgan_check.cpp (host code only), packs [W1], [W2 | Ws] and the biases
for channel counts with and without padded rows / columns (1, 32, 40, 48, 96, 192, 256) into
buffers of exactly the advertised size and decodes them back against the torch weights."""
import os
import shutil
import subprocess

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd")


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/llvm/bin/clang++"),
                    reason="needs make and the ROCm clang++")
def test_melgan_packer_clean_under_asan_ubsan():
    r = subprocess.run(["make", "-C", PKG, "asan-check-melgan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "residual-block packer OK" in r.stdout
