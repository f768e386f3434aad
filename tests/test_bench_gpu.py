"""A plain ``bench.py`` run on the device, at a toy shape: it reports the headline fields and none of
``--full``'s side measurements, and ``--dump-outputs`` holds exactly what the timed path returns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "hbm_roofline_step", "kernel_breakdown_ms", "cpu_baseline", "alt_math_mode", "glow_decoder",
             "glow_tts_e2e", "xtts_decoder", "vits_waveform", "vits_tts_e2e", "resblock2_decoder",
             "accuracy_vs_fp64_oracle")


def test_plain_run_is_lean_and_dumps_the_timed_output(tmp_path, cuda_device):
    import bench
    from tts_amd import synthetic

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "3", "--frames", "21", "--dump-outputs", str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["metric"] == bench.METRIC and rec["unit"] == "samples/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == bench.DTYPE["f16x3"] and rec["steps"] == 2 and rec["n_gpus"] == 1
    assert rec["value"] == pytest.approx(3 * 256 * (21 + 10) / (rec["ms_per_step"] / 1e3), rel=1e-9)
    assert rec["build"]["target"] == "gfx950"
    assert not [k for k in FULL_ONLY if k in rec]

    wav = np.load(tmp_path / "waveform.npy")
    assert wav.dtype == np.float32 and wav.shape == (3, 1, 256 * (21 + 10))
    g = bench.build_generator("f16x3", cuda_device)
    want = g.inference(synthetic.mel(3, 21, seed=0).to(cuda_device)).cpu().numpy()
    assert np.array_equal(wav, want)
