"""-m gpu: the folded re-binning step against the chain it replaces, bit for bit.

Small channels on the compact kernels re-bin in three launches: pass CD takes the cell histogram (k_forces_hist) and pass E
scans it, ranks every particle inside its new cell by id and stores the new ordering itself, with the clock in its tail
workgroup (k_continuity_rebin).  SPHX_DEBUG_SWITCHES=no_fold_rebin brings back k_continuity -> k_clock_scan -> k_scatter ->
k_reorder.  The new ordering is canonical (new cell, then ascending id), so the two must agree in every bit: every array of
download() with np.array_equal, and step, t, dt_last, vmax and the re-binnings counted by the schedule exactly.

The library reads the switches once per process, so each side runs tests/rebin_fold_worker.py as a fresh child under its own
time limit.  Every case holds at least three scheduled re-binnings (K = 16, 50 steps or more), and each child reports the
launches of a profiled stretch: the test asserts which chain ran.  After a child that ends by a signal, an abort or its time
limit no further child is started: that end is to be diagnosed from what the child printed, not run again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "rebin_fold_worker.py")
CHILD_SECONDS = 240
_abnormal = []  # what ended abnormally, if anything did

CHAIN = ("k_clock_scan", "k_scatter", "k_reorder")
FOLD = ("k_forces_hist", "k_continuity_rebin")
FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")


def run_child(case, mode, switches, out):
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=switches)
    cmd = [sys.executable, WORKER, "--case", case, "--mode", mode, "--out", str(out)]
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(f"[{switches}] {case}/{mode}: time limit of {CHILD_SECONDS} s")
        pytest.fail(f"{_abnormal[0]}\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
    if r.returncode != 0:
        _abnormal.append(f"[{switches}] {case}/{mode}: exit code {r.returncode}")
        pytest.fail(f"{_abnormal[0]}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(lines[0])
    assert res["switches"] == switches
    with np.load(str(out)) as z:
        arrays = {k: z[k] for k in FIELDS}
    print(f"[{switches or 'default'}] {case}/{mode}: step {res['step']} t {res['t']!r} dt_last {res['dt_last']!r} vmax {res['vmax']!r} "
          f"rebins {res['rebins']} forced {res['forced_rebuilds']} columns {res['n_cell_x']} K {res['rebuild_every']} "
          f"lanes {res['lanes']} graphs {res['graphs']} launches {res['launches']} "
          f"avg_us { {k: round(v, 2) for k, v in res['avg_us'].items()} }")
    return res, arrays


def both_sides(case, mode, tmp_path):
    new, a_new = run_child(case, mode, "", tmp_path / "fold.npz")
    old, a_old = run_child(case, mode, "no_fold_rebin", tmp_path / "chain.npz")
    return new, a_new, old, a_old


def assert_identical(new, a_new, old, a_old):
    assert new["device_status"] == 0 and old["device_status"] == 0, (new["device_status"], old["device_status"])
    for k in ("step", "t", "dt_last", "vmax", "rebins", "forced_rebuilds"):
        assert new[k] == old[k], (k, new[k], old[k])
    for k in FIELDS:
        assert a_new[k].shape == a_old[k].shape and np.all(np.isfinite(a_new[k])), k
        if not np.array_equal(a_new[k], a_old[k]):
            bad = np.argwhere(a_new[k] != a_old[k])
            pytest.fail(f"{k}: {len(bad)} of {a_new[k].size} entries differ, first at {bad[:3].tolist()}, "
                        f"max |diff| {np.max(np.abs(a_new[k] - a_old[k])):.3e}")


def assert_chain(res, folded):
    names = set(res["launches"])
    want, never = (FOLD, CHAIN) if folded else (CHAIN, FOLD)
    assert all(n in names for n in want) and not any(n in names for n in never), (folded, sorted(names))


@pytest.mark.parametrize("case,lanes", [("c2", 16), ("c1", 32)])
def test_headline_channels_are_bit_identical(case, lanes, tmp_path):
    """C2 (16 lanes per particle) and C1 (32) from the benchmark's start state: 56 steps, re-binnings at steps 16, 32, 48."""
    new, a_new, old, a_old = both_sides(case, "advance", tmp_path)
    assert new["lanes"] == lanes and new["schedule"]["fuse_ea"] == 1 and new["rebuild_every"] == 16, new
    assert new["step"] == 56 and new["rebins"] >= 3, new
    assert_chain(new, True)
    assert_chain(old, False)
    assert_identical(new, a_new, old, a_old)


def test_moving_walls_uneven_mass_rho0_are_bit_identical(tmp_path):
    """helpers.make_variant: moving walls, uneven mass, rho0 = 2.5 -- the mass and the id travel through the new pass E."""
    new, a_new, old, a_old = both_sides("variant", "advance", tmp_path)
    assert new["step"] == 50 and new["rebins"] >= 3 and new["schedule"]["fuse_ea"] == 1, new
    assert_chain(new, True)
    assert_chain(old, False)
    assert_identical(new, a_new, old, a_old)


def test_three_column_channel_is_bit_identical(tmp_path):
    """Three cell columns: every +-1 column of every cell is reached through the periodic wrap."""
    new, a_new, old, a_old = both_sides("three", "advance", tmp_path)
    assert new["n_cell_x"] == 3 and new["rebuild_every"] == 16 and new["step"] == 50 and new["rebins"] >= 3, new
    assert_chain(new, True)
    assert_chain(old, False)
    assert_identical(new, a_new, old, a_old)


def test_two_column_channel_keeps_the_chain(tmp_path):
    """Two cell columns (dp = 0.1, DL = 0.7): the +-1 columns coincide.  Such a channel re-bins on every step and has no skin, so
    it does not run the fused launches the fold builds on: both sides run today's chain, and agree."""
    new, a_new, old, a_old = both_sides("two", "advance", tmp_path)
    assert new["n_cell_x"] == 2 and new["rebuild_every"] == 1 and new["schedule"]["fuse_ea"] == 0, new
    assert_chain(new, False)
    assert_chain(old, False)
    assert_identical(new, a_new, old, a_old)


def test_benchmark_cadence_graph_replay_is_bit_identical(tmp_path):
    """C2 as the benchmark drives it: 5 steps of warm-up, then prepare_steps(20) / enqueue_steps(20) / sync() five times."""
    new, a_new, old, a_old = both_sides("c2", "graph", tmp_path)
    assert new["step"] == 105 and new["rebins"] >= 6, new
    assert new["graphs"]["slots_replayed"] >= 100 and old["graphs"]["slots_replayed"] >= 100, (new["graphs"], old["graphs"])
    assert_chain(new, True)
    assert_chain(old, False)
    assert_identical(new, a_new, old, a_old)


def test_eager_profiled_run_lists_the_new_launches(tmp_path):
    """C2 stepped eagerly with profiling on: the compared run itself lists k_continuity_rebin and none of k_scatter, k_reorder,
    k_clock_scan; with no_fold_rebin it is the other way round."""
    new, a_new, old, a_old = both_sides("c2", "profile", tmp_path)
    assert new["step"] == 56 and new["rebins"] >= 3, new
    assert_chain(new, True)
    assert_chain(old, False)
    assert new["launches"]["k_continuity_rebin"] == new["rebins"] == old["launches"]["k_reorder"], (new["launches"], old["launches"])
    assert_identical(new, a_new, old, a_old)
