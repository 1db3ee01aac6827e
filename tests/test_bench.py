"""bench.py's plain run: the headline line only, `--steps` timed steps, and --dump-outputs of the last one (-m gpu);
the options it refuses before touching a GPU (CPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"pos": 2, "vel": 2, "rho": 1, "p": 1, "drho_dt": 1, "force": 2, "force_prior": 2, "Vol": 1, "B": 4}


def _bench(*argv, timeout=300):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TORCHELASTIC_RUN_ID"):
        e.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=e, cwd=ROOT, capture_output=True,
                          text=True, timeout=timeout)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    r = _bench("--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == line["unit"] == "particle-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert not {"aux", "accuracy", "cpu_baseline"} & set(line) and line["roofline"] is None and line["kernels_ms"] == {}
    assert np.load(tmp_path / "sim.npy")[0] == 3 + 7  # the state of the last timed step
    n_total = int(line["config"]["workload"].split("n_total=")[1].split(",")[0])
    for name, cols in FIELDS.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float64 and a.reshape(n_total, -1).shape[1] == cols and np.isfinite(a).all(), name
    assert not (tmp_path / "rows.npy").exists()  # 5 760 particles: every row, no sample
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20


@pytest.mark.parametrize("argv", [("--profile-steps", "20"), ("--gpus", "2", "--dump-outputs", "out")],
                         ids=["profile-steps-without-full", "dump-outputs-on-two-gpus"])
def test_bench_refuses_options_it_cannot_honour(argv):
    r = _bench(*argv, "--check-launch", timeout=120)
    assert r.returncode == 2 and "{" not in r.stdout, (r.returncode, r.stdout, r.stderr)
