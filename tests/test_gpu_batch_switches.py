"""-m gpu: the three schedules of a batch's step -- the fused E|A launch, the clock in pass E's tail workgroup, a clock launch
of its own -- bit for bit the standalone contexts', flow statistics included.

The default schedule of a small channel is the first; SPHX_DEBUG_SWITCHES=no_fuse_ea / no_tail_clock select the others.  The
library reads the switches once per process, so every set runs tests/batch_switch_worker.py as a fresh child under its own
time limit.  Each test asserts, from a standalone context in the child, that the schedule it means was in fact chosen.  After a
child that ends by a signal, an abort or its time limit no further child is started: that end is to be diagnosed from what the
child printed, not run again."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "batch_switch_worker.py")
CHILD_SECONDS = 240
_abnormal = []  # what ended abnormally, if anything did

# (switches, lanes per particle, then fuse_ea, tail_clock of the schedule)
SETS = [("", 16, 1, 1), ("", 32, 1, 1), ("no_fuse_ea", 16, 0, 1), ("no_fuse_ea", 32, 0, 1), ("no_tail_clock", 16, 0, 0)]


@pytest.mark.parametrize("switches,lpp,fuse_ea,tail_clock", SETS, ids=[f"{s or 'none'}-lpp{l}" for s, l, *_ in SETS])
def test_batch_switch_set_bit_identical_to_standalone(switches, lpp, fuse_ea, tail_clock):
    _run_set(switches, lpp, fuse_ea, tail_clock, [])


def test_batch_own_clock_launch_in_four_regimes():
    """The clock launch of its own (no_tail_clock), whose dt limits are per member: the members of
    test_gpu_regimes.regime_members -- default physics (acoustic dt), flow to the left, c_f = 0.3 and mu = 2 (both limited by
    their viscous dt, five times and a quarter of the default's) -- with K = 4 and a skin of 1.6 h, so that no member outruns
    the skin (a forced re-binning re-bins all members of a batch, which the standalone contexts would not do)."""
    _run_set("no_tail_clock", 16, 0, 0, ["--case", "regimes", "--rebuild-every", "4", "--skin-h", "1.6"])


def _run_set(switches, lpp, fuse_ea, tail_clock, extra):
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=switches)
    cmd = [sys.executable, WORKER, "--lpp", str(lpp)] + extra
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(f"[{switches}] lpp {lpp}: time limit of {CHILD_SECONDS} s")
        pytest.fail(f"{_abnormal[0]}\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
    if r.returncode != 0:
        _abnormal.append(f"[{switches}] lpp {lpp}: exit code {r.returncode}")
        pytest.fail(f"{_abnormal[0]}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["switches"] == switches and out["lpp"] == lpp and out["info"]["lanes_per_particle"] == lpp
    assert (out["schedule"]["fuse_ea"], out["schedule"]["tail_clock"], out["schedule"]["dynamic"]) == (fuse_ea, tail_clock, 0), out["schedule"]
    assert out["steps"] == 2 * out["info"]["rebuild_every"] + 3 and out["steps_taken"] == [out["steps"]] * 4, out
    assert out["n_samples"] == [out["steps"]] * 4, out
    assert out["info"]["realignments"] == 0, out["info"]
    assert min(out["rebins"]) >= 2, out  # 2K+3 steps: re-binned at least twice
    assert not out["differs"], out["differs"]
