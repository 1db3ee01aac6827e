"""-m gpu: the block size of the compact step kernels does not change a bit of what a caller sees.

Sums run over the 16 or 32 lanes of a particle, maxima are exact, the neighbour lists are indexed by global lane and xcd_block
only renumbers workgroups, so 64, 128, 256, 512 and 1 024 threads per workgroup (SPHX_DEBUG_SWITCHES=block_64 ... block_1024)
have to agree bit for bit.  The library reads the switches once per process: tests/block_size_worker.py runs every case once per
size in a fresh child under its own time limit, and the tests compare what the children wrote, as bytes, against the 256-thread
child: the nine downloaded fields, t, dt, vmax, the pair count and both wall shears, after 35 steps across two re-binnings (whose
kernels stay at 256 threads; the per-workgroup maxima are kept per 64, 128 or 256 lanes, and a workgroup of more lanes than
that fills every entry it covers) of

  odd         597 fluid particles (dp 0.05, DL 1.5, three removed): no multiple of the 4, 8, 16, 32 or 64 particles of a workgroup,
              so the last workgroup is partly filled and partly beyond the population;
  c1, c2      the benchmark's small channels, 32 and 16 lanes per particle; c2 runs 1 200 workgroups of 64 threads and 600 of
              128 per pass: more than 256, and the clock's tail workgroup collects nineteen and five entries per thread;
  c2_chunked  the same 35 steps as calls of 1 + 7 + 27, which must also equal c2's single call;
  dense       dense_cases.C, lists of up to 106 entries: the loops behind the rows a lane asks for ahead.

After a child that ends by a signal, an abort or its time limit no further child is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "block_size_worker.py")
CHILD_SECONDS = 240
SIZES = (256, 64, 128, 320, 384, 512, 1024)
CASES = ("odd", "c1", "c2", "c2_chunked", "dense")
ARRAYS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B", "t", "dt_last", "vmax", "pairs", "tau_bottom",
          "tau_top")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{block size: (the child's JSON line, {case: {name: array}})}; a child that ended abnormally ends the series."""
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
            with np.load(os.path.join(d, case + ".npz")) as z:
                data[case] = {k: z[k].copy() for k in ARRAYS}
        out[blk] = (facts["cases"], data)
    return out


def _same_bytes(a, b, what):
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs, largest difference {np.max(np.abs(a[k] - b[k]))!r}"


@pytest.mark.parametrize("blk", SIZES)
def test_children_ran_the_size_they_were_asked_for(runs, blk):
    facts = runs[blk][0]
    lanes = dict(odd=16, c1=32, c2=16, c2_chunked=16, dense=16)
    for case in CASES:
        f = facts[case]
        print(f"[block {blk}] {case}: {f}")
        assert f["block_size"] == blk and f["lanes"] == lanes[case], f
        assert f["fuse_ea"] == 1 and f["tail_clock"] == 1, f   # the three-launch step with the clock in the tail workgroup
        # (two scheduled re-binnings in 35 steps; the dense state outruns its cell skin and re-bins far more often)
        assert f["steps"] == 35 and f["finite"] and (f["rebins"] == 2 or (case == "dense" and f["rebins"] > 2)), f
        assert f["rebins"] == runs[256][0][case]["rebins"], f
    assert facts["odd"]["n_fluid"] == 597 and facts["c2"]["n_fluid"] == 4800 and facts["c1"]["n_fluid"] == 1875


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("blk", (64, 128, 320, 384, 512, 1024))
def test_block_size_changes_no_bit(runs, blk, case):
    _same_bytes(runs[blk][1][case], runs[256][1][case], f"block_{blk} against block_256, {case}")


@pytest.mark.parametrize("blk", SIZES)
def test_chunked_calls_equal_one_call(runs, blk):
    _same_bytes(runs[blk][1]["c2_chunked"], runs[blk][1]["c2"], f"block_{blk}: 1 + 7 + 27 steps against 35")


def test_launch_names_and_counts_are_unchanged(runs):
    """16 profiled steps of c2 from step 35 -- one full re-binning cycle: the cell sweep once, pass B sixteen times, the fused E|A
    launch fifteen times, the two kernels of the re-binning step once -- whatever the block size."""
    want = {"k_density_build": 1, "k_kgc": 16, "k_forces": 15, "k_continuity_density": 15, "k_forces_hist": 1, "k_continuity_rebin": 1}
    for blk in SIZES:
        got = runs[blk][0]["c2"]["launches"]
        print(f"[block {blk}] launches of 16 steps: {got}")
        assert got == want, (blk, got)
