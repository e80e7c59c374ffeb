"""A plain `bench.py` run on the GPU: the headline line alone (nothing of --full), and what --dump-outputs writes -- the generator output of the
last timed step -- against the fp32 CPU oracle on the same seeded images.  bench.py runs as a CHILD process (the pytest process has initialised the GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gandtr_amd.tools import synth
from oracle import gandtr_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_output(cuda_device, tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GANDTR_BENCH_FORCE_DIST"):
        env.pop(k, None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--gen-batch", "4",
                           "--dump-outputs", str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, check=False)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-2000:]
    lines = [ln for ln in proc.stdout.decode(errors="replace").splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"] == "f16c" and rec["full"] is False
    assert all(rec[k] is None for k in ("roofline", "fast_mode", "exact_mode", "secondary", "parity_measured")) and "cpu_baseline" not in rec
    assert sorted(os.listdir(tmp_path)) == ["generator_output.npy"]
    got = np.load(tmp_path / "generator_output.npy")
    assert got.shape == (4, 3, 256, 256) and got.dtype == np.float32
    # rank 0's batch of 4 is the CPU baseline's sample (bench.CPU_SAMPLE_GEN); the gate is north_star's 1e-3 of the pre-tanh range, which tanh
    # (1-Lipschitz) carries over to the image
    x = synth.synth_input(100, (4, 3, 256, 256), 1.0)
    ref = O.resnet_generator(x, synth.generator_state(0, "instance", gain=0.02), "instance", 9, pre_tanh=True)
    d = float((torch.from_numpy(got) - torch.tanh(ref)).abs().max())
    assert d <= 1e-3 * float(ref.abs().max()), d
