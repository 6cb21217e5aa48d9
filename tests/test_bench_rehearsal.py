"""Dress rehearsal of the driver's SCALE invocation (VERDICT r1 #3:
"when the driver gets an 8-GPU node, the curve exists on the first
try").  Runs the EXACT torchrun command shape the driver uses — nnodes
1, nproc-per-node N, master-addr 127.0.0.1 — against bench.py with
FAM_BENCH_CPU=1 (HIP kernels stubbed, gloo collectives), and validates
the emitted JSON contract."""

import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class TestBenchRehearsal:
    def test_driver_invocation_world2(self):
        env = dict(os.environ)
        env["FAM_BENCH_CPU"] = "1"
        env["FAM_PG_TIMEOUT"] = "60"
        proc = subprocess.run(
            [
                sys.executable, "-m", "torch.distributed.run",
                "--nnodes=1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1",
                "--master-port", str(_free_port()),
                os.path.join(ROOT, "bench.py"),
                "--gpus", "2", "--steps", "2", "--warmup", "1",
                "--pop-per-gpu", "8", "--horizon", "4",
            ],
            capture_output=True, text=True, timeout=420, cwd=ROOT, env=env,
        )
        assert proc.returncode == 0, proc.stderr[-3000:]
        # exactly ONE JSON line, from rank 0
        lines = [ln for ln in proc.stdout.splitlines()
                 if ln.startswith("{")]
        assert len(lines) == 1, proc.stdout
        d = json.loads(lines[0])
        assert d["metric"] == "es_rollouts_per_sec"
        assert d["n_gpus"] == 2
        assert d["steps"] == 2 and d["warmup"] == 1
        assert d["config"]["parallelism"] == "dp2"
        assert d["config"]["global_batch"] == 8 * 2 * 64
        assert d["value"] > 0 and d["ms_per_step"] > 0
        assert d["scaling"] == "weak"

    def test_single_rank_default_contract(self):
        env = dict(os.environ)
        env["FAM_BENCH_CPU"] = "1"
        proc = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"),
             "--steps", "2", "--warmup", "1",
             "--pop-per-gpu", "8", "--horizon", "4"],
            capture_output=True, text=True, timeout=300, cwd=ROOT, env=env,
        )
        assert proc.returncode == 0, proc.stderr[-3000:]
        d = json.loads([ln for ln in proc.stdout.splitlines()
                        if ln.startswith("{")][0])
        assert d["n_gpus"] == 1
        assert d["higher_is_better"] is True



_DUMP_CACHE = {}


def _bench_dump(tmp_path_factory, steps, warmup, *extra):
    """Run the CPU-rehearsal benchmark with --dump-outputs; returns
    (result line, {file name: array}).  Each argument set runs once and is
    shared by the tests below."""
    import numpy as np

    key = (steps, warmup) + extra
    if key not in _DUMP_CACHE:
        env = dict(os.environ)
        env["FAM_BENCH_CPU"] = "1"
        out = tmp_path_factory.mktemp("dump")
        proc = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"),
             "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
             "--pop-per-gpu", "8", "--horizon", "4",
             "--dump-outputs", str(out)] + list(extra),
            capture_output=True, text=True, timeout=300, cwd=ROOT, env=env,
        )
        assert proc.returncode == 0, proc.stderr[-3000:]
        lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, proc.stdout
        _DUMP_CACHE[key] = (json.loads(lines[0]),
                            {p.name: np.load(p) for p in out.iterdir()})
    return _DUMP_CACHE[key]


class TestBenchDumpOutputs:
    def test_files_dtypes_and_size(self, tmp_path_factory):
        import numpy as np

        d, dumped = _bench_dump(tmp_path_factory, 3, 1)
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert {"theta.npy", "adam_m.npy", "adam_v.npy",
                "stats.npy"} <= set(dumped)
        for name, arr in dumped.items():
            assert arr.dtype in (np.float32, np.float64), name
            assert np.isfinite(arr).all(), name
        assert dumped["theta.npy"].shape == dumped["adam_m.npy"].shape
        assert np.abs(dumped["adam_m.npy"]).max() > 0
        assert sum(a.nbytes for a in dumped.values()) <= 64 << 20

    def test_same_arguments_same_outputs_and_full_exits_zero(
            self, tmp_path_factory):
        """A second run with the same arguments dumps equal arrays; it is
        given --full, which must exit 0 and leave the headline run as it
        is."""
        import numpy as np

        _d, first = _bench_dump(tmp_path_factory, 3, 1)
        d, second = _bench_dump(tmp_path_factory, 3, 1, "--full")
        assert d["metric"] == "es_rollouts_per_sec" and d["steps"] == 3
        assert set(first) == set(second)
        for name in first:
            assert np.array_equal(first[name], second[name]), name

    def test_dump_is_the_last_timed_step(self, tmp_path_factory):
        """Iterations are numbered warmup + i, so 1 warm-up + 3 timed steps
        and 2 + 2 end on the same iteration 3 and must dump the same stats
        and state; one more timed step must move them."""
        import numpy as np

        _d, a = _bench_dump(tmp_path_factory, 3, 1)
        _d, b = _bench_dump(tmp_path_factory, 2, 2)
        _d, c = _bench_dump(tmp_path_factory, 4, 1)
        for name in a:
            assert np.array_equal(a[name], b[name]), name
        # stats layout: fitness_mean, fitness_max, grad_norm, rollouts,
        # env_steps
        assert a["stats.npy"][3] == 8 * 64
        assert a["stats.npy"][4] == 8 * 64 * 4
        assert not np.array_equal(a["theta.npy"], c["theta.npy"])
        assert not np.array_equal(a["stats.npy"][:3], c["stats.npy"][:3])
