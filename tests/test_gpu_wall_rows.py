"""-m gpu: the compact step kernels (16 and 32 lanes per particle) compute what they computed before pass CD stopped building
the pair of a prefetched wall row twice (forces_pass, wall_pressure_from; csrc/sphx_kernels.hpp, csrc/sphx_device.hpp) -- to the
bit, in waves with wall rows, in waves without, and where both kinds share a launch.

tests/golden/wall_rows_<case>_lpp<lanes>.npz were recorded once on an MI355X with the library of the commit before that change
(tests/golden/make_wall_rows.py, beside them).  tests/wall_rows_worker.py (its docstring says what each case is for) runs the
same cases with this build, once per block size in a fresh child under its own time limit (SPHX_DEBUG_SWITCHES is read once
per process), and a third child runs the first case with no_wall_paths.  The tests compare what the children wrote against the
fixtures as bytes: the nine downloaded fields, t, dt, max |v|, the pair count and both wall shears after 20 steps -- of every
member for the batch.  The worker itself asserts on the device's neighbour list that the waves a case is there for exist
(check_census) and compares the batch members with contexts of their own.

After a child that ends by a signal, an abort or its time limit no further child is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wall_rows_worker as worker

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "wall_rows_worker.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHILD_SECONDS = 240
# (child: its switches, its cases)
CHILDREN = {"block_256": ("block_256", tuple(worker.CASES)), "block_320": ("block_320", tuple(worker.CASES)),
            "no_wall_paths": ("block_320,no_wall_paths", ("slots_developed",))}
RUNS = [(child, case, lpp) for child, (_, cases) in CHILDREN.items() for case in cases for lpp in worker.LANES]


@pytest.fixture(scope="module")
def golden():
    out = {}
    for case in worker.CASES:
        for lpp in worker.LANES:
            with np.load(os.path.join(GOLDEN, f"wall_rows_{case}_lpp{lpp}.npz")) as z:
                out[case, lpp] = {k: z[k].copy() for k in worker.ARRAYS + ("rebins",)}
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{child: (the child's facts per run, {(case, lanes): {name: array}})}; a child that ended abnormally ends the series."""
    out = {}
    for child, (switches, cases) in CHILDREN.items():
        d = str(tmp_path_factory.mktemp(child))
        env = dict(os.environ, SPHX_DEBUG_SWITCHES=switches)
        try:
            r = subprocess.run([sys.executable, WORKER, d, *cases], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{child}: time limit of {CHILD_SECONDS} s; nothing more is started\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
        if r.returncode != 0:
            pytest.fail(f"{child}: exit code {r.returncode}; nothing more is started\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
        facts = json.loads(lines[0])
        assert facts["switches"] == switches
        data = {}
        for case in cases:
            for lpp in worker.LANES:
                with np.load(os.path.join(d, f"{case}_lpp{lpp}.npz")) as z:
                    data[case, lpp] = {k: z[k].copy() for k in worker.ARRAYS}
        out[child] = (facts["runs"], data)
    return out


@pytest.mark.parametrize("child,case,lpp", RUNS)
def test_children_ran_the_kernels_in_question(runs, golden, child, case, lpp):
    f = runs[child][0][f"{case}_lpp{lpp}"]
    print(f"[{child}] {case} at {lpp} lanes: {f}")
    blk = 256 if case in worker.ALWAYS_256 else int(CHILDREN[child][0].split(",")[0].split("_")[1])
    assert f["block_size"] == blk and f["lanes"] == lpp, f
    # the three-launch step with the folded re-binning and the clock in the tail workgroup, across one re-binning at least
    assert f["fuse_ea"] == 1 and f["tail_clock"] == 1 and f["dynamic"] == 0 and f["finite"], f
    assert f["rebins"] == int(golden[case, lpp]["rebins"]) and f["rebins"] >= 1, f
    if case == "batch4":
        assert f["members"] == worker.MEMBERS and f["steps"] == [worker.STEPS] * worker.MEMBERS and f["members_equal_contexts"], f
    else:
        assert f["steps"] == worker.STEPS and f["substeps"] == (3 if case == "dual_rate" else 1), f
        worker.check_census(case, f["census"])
    if case.startswith("slots") or case == "batch4":
        assert f["n_fluid"] == 483 and f["n_wall"] == 184 and f["n_cell_x"] == 5, f


@pytest.mark.parametrize("child,case,lpp", RUNS)
def test_results_are_the_recorded_ones_to_the_bit(runs, golden, child, case, lpp):
    got, want = runs[child][1][case, lpp], golden[case, lpp]
    for k in worker.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (child, case, lpp, k)
        assert got[k].tobytes() == want[k].tobytes(), \
            f"{child}, {case} at {lpp} lanes: {k} differs from the recording, largest difference {np.max(np.abs(got[k] - want[k]))!r}"


@pytest.mark.parametrize("lpp", worker.LANES)
def test_no_wall_paths_gives_the_bytes_of_the_default(runs, lpp):
    a, b = runs["block_320"][1]["slots_developed", lpp], runs["no_wall_paths"][1]["slots_developed", lpp]
    for k in worker.ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), (lpp, k)
