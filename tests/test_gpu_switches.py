"""-m gpu: both sides of every A/B behind SPHX_DEBUG_SWITCHES, against the oracle, on a small channel.

The kernel forms behind the headline number (LDS tiles in passes A, B and E, slot-coded lists) start at 10^6 resident
particles; `tiles_be_from_1` brings them down to any size, and no_lds_tiles, no_coded_lists, no_fuse_ea, no_tail_clock,
no_lazy_out and full_copyback select the other side of an A/B.  A small channel is a legal input of the tile forms: the layout
of a workgroup's tile (tile_ranges) is three index ranges cut from the cell starts and capped at the tile size, worked out
for every workgroup of every walk-kernel context whatever its size (the force pass stages its tile at every size already), and
a neighbour outside the staged ranges is read from global memory; the 10^6 is a speed threshold.

The library reads the switches once per process, so every set runs tests/switch_worker.py as a fresh child under its own time
limit: 35 steps of the moving-wall variant across its re-binnings, every field against the oracle at the tolerances of
test_gpu_resident.py.  Each test asserts that the forms it means were in fact chosen (Context.kernel_forms / schedule).
kernel_forms has no entry for lazy_out: for no_lazy_out only its precondition (walk kernels) can be asserted.  After a child
that ends by a signal, an abort or its time limit no further child is started: that end is to be diagnosed from what the child
printed, not run again.

The default state flows to the right, stays two decades below the cap of the Riemann dissipation and is limited by the
acoustic dt on every step, so a wrong folded constant of the cap, a wrong wrap at x < 0 or a wrong viscous limit in one of the
force-pass, list or clock forms selected here would change nothing above.  test_switch_set_matches_oracle_left_capped runs the
sets that change the force pass, the lists or the clock once more on regime_cases.left_capped at the worker's size (--case):
the same variant mirrored, c_f = 0.3.  Over its 35 steps the oracle counts 266 to 531 fluid pairs on the cap, 130 crossings of
the seam to the left and the viscous limit on every step (tests/test_regime_cases.py asserts it); the flow outruns the cell
skin, so drift-forced re-binnings and their cool-down are on the way as well.

Both states load every cell column alike and keep their lists at a quarter of the capacity.
test_switch_set_matches_oracle_dense runs the tile forms, both list codings, the compact kernels and the device-decided
re-binning on dense_cases.A at the worker's size: long lists, uneven columns, voids."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "switch_worker.py")
CHILD_SECONDS = 240
_abnormal = []  # what ended abnormally, if anything did

WALK = dict(walk_kernels=True, lds_tiles=True, tiles_abe=False, coded_lists=False)
COMPACT = dict(walk_kernels=False, lds_tiles=False, tiles_abe=False, coded_lists=False)
# (switches, lanes per particle, dynamic re-binning, kernel forms, then fuse_ea, tail_clock of the schedule)
SETS = [
    ("", 2, False, WALK, 1, 1),
    ("", 16, False, COMPACT, 1, 1),
    ("tiles_be_from_1", 2, False, dict(WALK, tiles_abe=True, coded_lists=True), 0, 1),
    ("tiles_be_from_1,no_coded_lists", 2, False, dict(WALK, tiles_abe=True), 0, 1),
    ("no_lds_tiles", 2, False, dict(WALK, lds_tiles=False), 1, 1),
    ("no_fuse_ea", 2, False, WALK, 0, 1),
    ("no_fuse_ea", 16, False, COMPACT, 0, 1),
    ("no_tail_clock", 2, False, WALK, 0, 0),
    ("no_tail_clock", 16, False, COMPACT, 0, 0),
    ("no_lazy_out", 2, False, WALK, 1, 1),
    ("", 2, True, WALK, 0, 0),
    ("full_copyback", 2, True, WALK, 0, 0),
]


# the sets that change the force pass, the lists or the clock
REGIME_SETS = [s for s in SETS if (s[0], s[1], s[2]) in {
    ("", 2, False), ("", 16, False), ("tiles_be_from_1", 2, False), ("tiles_be_from_1,no_coded_lists", 2, False),
    ("no_lds_tiles", 2, False), ("no_tail_clock", 2, False), ("no_tail_clock", 16, False), ("", 2, True)}]
assert len(REGIME_SETS) == 8


@pytest.mark.parametrize("switches,lpp,dynamic,forms,fuse_ea,tail_clock", SETS,
                         ids=[f"{s or 'none'}-lpp{l}{'-dyn' if d else ''}" for s, l, d, *_ in SETS])
def test_switch_set_matches_oracle(switches, lpp, dynamic, forms, fuse_ea, tail_clock):
    _run_set(switches, lpp, dynamic, forms, fuse_ea, tail_clock, "")


@pytest.mark.parametrize("switches,lpp,dynamic,forms,fuse_ea,tail_clock", REGIME_SETS,
                         ids=[f"{s or 'none'}-lpp{l}{'-dyn' if d else ''}" for s, l, d, *_ in REGIME_SETS])
def test_switch_set_matches_oracle_left_capped(switches, lpp, dynamic, forms, fuse_ea, tail_clock):
    _run_set(switches, lpp, dynamic, forms, fuse_ea, tail_clock, "left_capped")


# the tile forms and both list codings, the compact kernels and the device-decided re-binning
DENSE_SETS = [s for s in SETS if (s[0], s[1], s[2]) in {
    ("", 2, False), ("tiles_be_from_1", 2, False), ("tiles_be_from_1,no_coded_lists", 2, False), ("no_lds_tiles", 2, False),
    ("", 16, False), ("", 2, True)}]
assert len(DENSE_SETS) == 6


@pytest.mark.parametrize("switches,lpp,dynamic,forms,fuse_ea,tail_clock", DENSE_SETS,
                         ids=[f"{s or 'none'}-lpp{l}{'-dyn' if d else ''}" for s, l, d, *_ in DENSE_SETS])
def test_switch_set_matches_oracle_dense(switches, lpp, dynamic, forms, fuse_ea, tail_clock):
    """dense_cases.A at the worker's size: the variant pulled towards mid-channel and towards the seam next to the bottom
    wall.  Lists of up to 69 entries and a superset of up to 141 (of 96 and 144 at 2 lanes per particle); the fullest cell
    column holds 219 particles and the fullest three adjacent ones 560 where every column of the variant holds 160 and 480,
    so a workgroup's tile layout (three ranges capped at 480 or 464 slots) overflows, entries go out as far codes or index
    differences, and the columns next to the cores run empty within a few steps (tests/test_dense_cases.py asserts the
    census)."""
    _run_set(switches, lpp, dynamic, forms, fuse_ea, tail_clock, "A")


def _run_set(switches, lpp, dynamic, forms, fuse_ea, tail_clock, case):
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=switches)
    cmd = [sys.executable, WORKER, "--lpp", str(lpp), "--steps", "35"] + (["--dynamic"] if dynamic else [])
    cmd += ["--case", case] if case else []
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
    assert out["switches"] == switches and out["steps"] == 35 and out["case"] == case
    print(f"[switches] {case or 'variant'} [{switches}] lpp {lpp}{' dynamic' if dynamic else ''}: rebins {out['rebins']} forced "
          f"{out['forced_rebuilds']} worst {max(out['errors'].values()):.1e} {out['errors']}")
    assert out["forms"] == forms, out["forms"]
    assert (out["schedule"]["fuse_ea"], out["schedule"]["tail_clock"], out["schedule"]["dynamic"]) == (fuse_ea, tail_clock, int(dynamic)), out["schedule"]
    assert out["rebins"] + out["forced_rebuilds"] >= 2, out      # 35 steps: re-binned at least twice on every schedule
    assert not out["failures"], (out["failures"], out["errors"])
