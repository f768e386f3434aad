"""The Conv2d packer of the speaker encoder (tts-3_amd/csrc/pack.cpp, pack_conv2d and
pack_conv2d_epilogue) under AddressSanitizer + UBSan: `make -C tts-3_amd asan-check-conv2d` builds
csrc/pack.cpp with the stand-alone tests_native/conv2d_pack_check.cpp (host code only), packs 3x3 and
1x1 weights with and without padded rows / channels, and past one 256-row group, into buffers of
exactly the advertised size and decodes them back against the torch-layout weights."""
import os
import shutil
import subprocess

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-3_amd")


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/llvm/bin/clang++"),
                    reason="needs make and the ROCm clang++")
def test_conv2d_packer_clean_under_asan_ubsan():
    r = subprocess.run(["make", "-C", PKG, "asan-check-conv2d"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "conv2d packer OK" in r.stdout
