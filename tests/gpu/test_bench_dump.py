"""bench.py --dump-outputs on the GPU paths the CPU rehearsal cannot
reach: the ConvNet config and --mode pool.  Tiny populations; each case is
one short benchmark process."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))


def _bench(out, *extra):
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--horizon", "4",
         "--dump-outputs", str(out)] + list(extra),
        capture_output=True, text=True, timeout=240, cwd=ROOT,
    )
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    dumped = {p.name: np.load(p) for p in out.iterdir()}
    for name, arr in dumped.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert np.isfinite(arr).all(), name
    assert sum(a.nbytes for a in dumped.values()) <= 64 << 20
    return json.loads(lines[0]), dumped


@requires_gpu
class TestBenchDumpGPU:
    def test_conv_engine_dump(self, tmp_path):
        d, dumped = _bench(tmp_path / "conv", "--model", "conv",
                           "--pop-per-gpu", "32")
        assert d["config"]["model"] == "es-conv-84x84x4-dqn-act6"
        assert {"theta.npy", "adam_m.npy", "adam_v.npy",
                "stats.npy"} <= set(dumped)
        assert np.abs(dumped["adam_m.npy"]).max() > 0
        assert dumped["stats.npy"][3] == 32 * 16  # rollouts per step

    def test_pool_mode_dump(self, tmp_path):
        d, dumped = _bench(tmp_path / "pool", "--mode", "pool",
                           "--pop-per-gpu", "64")
        assert d["config"]["parallelism"] == "pool-dp1"
        # one row per rank: the stats dict run_on_all returned, and theta's
        # checksum as printed in the result line
        assert dumped["stats.npy"].shape == (1, 5)
        assert dumped["stats.npy"][0, 3] == 64 * 64
        assert dumped["theta_sum.npy"].shape == (1,)
        assert dumped["theta_sum.npy"][0] == d["config"]["theta_sum"]
