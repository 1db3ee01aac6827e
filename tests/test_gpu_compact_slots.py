"""-m gpu: the compact step kernels (16 and 32 lanes per particle) compute what they computed before their own-record loads
and their minimum-image fold were rewritten to issue fewer instructions (own_slot, pair_dx, csrc/sphx_kernels.hpp) -- to the bit.

tests/golden/compact_slots_<case>_lpp<lanes>.npz were recorded once on an MI355X with the library of the commit before that
change (tests/golden/make_compact_slots.py, beside them).  tests/compact_slots_worker.py runs the same cases with this build,
once per block size in a fresh child under its own time limit (SPHX_DEBUG_SWITCHES is read once per process), and the tests
compare what the children wrote against the fixtures as bytes: the nine downloaded fields, t, dt, max |v|, the pair count and
both wall shears after 35 steps.

  channel     dp = 1/21, DL = 23/21: 483 fluid + 184 wall particles, five cell columns -- the folded re-binning step applies,
              483 is no multiple of 8, 10, 16 or 20 (the particles of a workgroup of 256 or 320 threads at 32 or 16 lanes), so the
              last workgroup of every pass is partly filled and reaches beyond the population, and the periodic seam lies inside
              every pass;
  developed   the benchmark's start (analytic parabola, jitter 0.05 dp), two scheduled re-binnings in the 35 steps;
  rest        the lattice at rest.

After a child that ends by a signal, an abort or its time limit no further child is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "compact_slots_worker.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHILD_SECONDS = 240
SIZES = (256, 320)
CASES = ("developed", "rest")
LANES = (16, 32)
ARRAYS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B", "t", "dt_last", "vmax", "pairs", "tau_bottom",
          "tau_top")


@pytest.fixture(scope="module")
def golden():
    out = {}
    for case in CASES:
        for lpp in LANES:
            with np.load(os.path.join(GOLDEN, f"compact_slots_{case}_lpp{lpp}.npz")) as z:
                out[case, lpp] = {k: z[k].copy() for k in ARRAYS + ("rebins",)}
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{block size: (the child's facts per run, {(case, lanes): {name: array}})}; a child that ended abnormally ends the series."""
    out = {}
    for blk in SIZES:
        d = str(tmp_path_factory.mktemp(f"block_{blk}"))
        env = dict(os.environ, SPHX_DEBUG_SWITCHES=f"block_{blk}")
        try:
            r = subprocess.run([sys.executable, WORKER, d], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"block_{blk}: time limit of {CHILD_SECONDS} s; nothing more is started\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
        if r.returncode != 0:
            pytest.fail(f"block_{blk}: exit code {r.returncode}; nothing more is started\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
        facts = json.loads(lines[0])
        assert facts["switches"] == f"block_{blk}"
        data = {}
        for case in CASES:
            for lpp in LANES:
                with np.load(os.path.join(d, f"{case}_lpp{lpp}.npz")) as z:
                    data[case, lpp] = {k: z[k].copy() for k in ARRAYS}
        out[blk] = (facts["runs"], data)
    return out


@pytest.mark.parametrize("lpp", LANES)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("blk", SIZES)
def test_children_ran_the_kernels_in_question(runs, golden, blk, case, lpp):
    f = runs[blk][0][f"{case}_lpp{lpp}"]
    print(f"[block {blk}] {case} at {lpp} lanes: {f}")
    assert f["block_size"] == blk and f["lanes"] == lpp, f
    assert f["n_fluid"] == 483 and f["n_wall"] == 184 and f["n_cell_x"] == 5, f
    # the three-launch step with the folded re-binning and the clock in the tail workgroup
    assert f["fuse_ea"] == 1 and f["tail_clock"] == 1 and f["dynamic"] == 0, f
    assert f["steps"] == 35 and f["finite"] and f["rebins"] == int(golden[case, lpp]["rebins"]), f
    if case == "developed":
        assert f["rebins"] == 2, f


@pytest.mark.parametrize("lpp", LANES)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("blk", SIZES)
def test_results_are_the_recorded_ones_to_the_bit(runs, golden, blk, case, lpp):
    got, want = runs[blk][1][case, lpp], golden[case, lpp]
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (blk, case, lpp, k)
        assert got[k].tobytes() == want[k].tobytes(), \
            f"block_{blk}, {case} at {lpp} lanes: {k} differs from the recording, largest difference {np.max(np.abs(got[k] - want[k]))!r}"
