"""Child process of tests/test_gpu_wall_rows.py and tests/golden/make_wall_rows.py: SPHX_DEBUG_SWITCHES is read once per process, so
each block size of the compact step kernels (block_256, block_320) and the switch no_wall_paths run in a fresh one.  Runs the
cases named on the command line (default: all of CASES) at 16 and at 32 lanes per particle and writes what a caller can see of
each -- the nine downloaded fields, t, dt_last, vmax, the pair count, both wall shears -- to OUT/<case>_lpp<lanes>.npz, and
prints ONE JSON line with the facts of every run: block size, lanes, schedule, steps, re-binnings, the grid, and the census of
wave classes taken from the device's own neighbour list.

    SPHX_DEBUG_SWITCHES=block_320 python tests/wall_rows_worker.py OUT [case ...]

What the cases are for (pass CD at 16 / 32 lanes per particle keeps the pair of a prefetched wall row for its second loop,
csrc/sphx_kernels.hpp, forces_pass; the census counts the waves of 64 lanes in which some lane owns a row of wall neighbours):

  slots_developed, slots_rest   the 483-particle channel of tests/compact_slots_worker.py, 20 steps across one folded re-binning
                                (k_forces_hist, k_continuity_rebin); wall rows sit in most waves
  mixed                         dp 0.05, DL 1.5, DH 1: 600 particles, waves with and without a wall row in one launch
  moving_left                   the same channel flowing leftward between moving walls with uneven mass: the mirrored wall
                                velocity of pass E, the viscous wall term of pass CD
  dual_rate                     the dual-rate loop with three inner sub-steps: the inner ones leave the wall terms of the first
                                loop of pass CD out, the second loop still needs the pair
  dense_wall                    tests/dense_cases.py's case C, pulled towards the seam next to the bottom wall: lanes whose third
                                and later rows hold wall entries (the loops behind the two prefetched rows)
  batch4                        four members (four seeds of slots_developed) through the batch kernels; the worker also runs
                                each member as a context of its own and reports whether the bytes agree"""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    sys.path.insert(0, p)

import compact_slots_worker as slots  # noqa: E402
import dense_cases  # noqa: E402
from helpers import make_case, make_variant  # noqa: E402

FIELDS = slots.FIELDS
SCALARS = slots.SCALARS
ARRAYS = FIELDS + SCALARS
LANES = (16, 32)
STEPS = 20
MEMBERS = 4
MIXED = dict(dp=0.05, DL=1.5)


def slots_developed(cfg, geo):
    prm, parts, start = slots.developed(cfg, geo)
    return prm, dict(parts, **start), {}


def slots_rest(cfg, geo):
    prm, parts, _ = slots.rest(cfg, geo)
    return prm, parts, {}


def mixed(cfg, geo):
    prm, parts = make_case(cfg, geo, seed=77, jitter=0.2, **MIXED)
    return prm, parts, {}


def moving_left(cfg, geo):
    prm, parts = make_variant(cfg, geo, seed=78, jitter=0.2, U_bulk=-0.666667, top_ux=-0.8, bottom_ux=0.3, rho0=2.5,
                              transport_coeff=0.1, **MIXED)
    return prm, parts, {}


def dual_rate(cfg, geo):
    prm, parts = make_case(cfg, geo, seed=79, jitter=0.2, **MIXED)
    return prm, parts, dict(dual_rate=3)


def dense_wall(cfg, geo):
    prm, parts = dense_cases.C(cfg, geo, "small")
    return prm, parts, {}


def batch4(cfg, geo):
    """-> prm, [parts of member k], {}: the benchmark's start of the 483-particle channel at four seeds"""
    prm, parts = slots.channel(cfg, geo)
    members = []
    for k in range(MEMBERS):
        pos, vel = geo.developed_state(prm, parts, jitter=0.05, seed=12345 + k)
        members.append(dict(parts, pos=pos, vel=vel))
    return prm, members, {}


CASES = {"slots_developed": slots_developed, "slots_rest": slots_rest, "mixed": mixed, "moving_left": moving_left,
         "dual_rate": dual_rate, "dense_wall": dense_wall, "batch4": batch4}
# what the census of a case must show, per lane count (asserted by the worker on the device's list, by the CPU test on the oracle's)
BOTH_CLASSES = ("slots_developed", "slots_rest", "mixed", "moving_left", "dual_rate", "dense_wall")
INTERIOR_MAJORITY = ("mixed", "moving_left", "dual_rate")   # a channel high enough: most waves have no wall row
THIRD_WALL_ROW = ("dense_wall",)
ALWAYS_256 = ("dual_rate",)   # (the dual-rate loop keeps workgroups of 256 threads whatever block_N says)


def census(pair_i, pair_j, pos, nf, lanes, DL, ncx, ncy, y0, cs):
    """Wave classes of the compact passes from a pair list (1-based indices, fluid rows first, as the oracle and the device
    return it) at the positions the list was built from.  The device keeps the fluid sorted by cell (cx * ncy + cy, columns of
    DL / ncx, rows of cs from y0), then by index; a wave holds 64 / lanes consecutive particles.  A lane owns entries sub,
    sub + lanes, ... of its particle's list, fluid entries first: a particle with n entries of which n_wall > 0 are wall ones has
    wall entries in rows (n - n_wall) // lanes .. (n - 1) // lanes.
    -> dict(waves, wall_waves, interior_waves, wall_particles, third_row_walls: particles with a wall entry in row >= 2)"""
    i, j = np.asarray(pair_i).astype(np.int64) - 1, np.asarray(pair_j).astype(np.int64) - 1
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    assert np.all(lo < nf)
    n_wall = np.bincount(lo[hi >= nf], minlength=nf)[:nf]
    n_all = n_wall + np.bincount(np.concatenate([lo[hi < nf], hi[hi < nf]]), minlength=nf)[:nf]
    cx = np.clip(np.floor(pos[:nf, 0] * (ncx / DL)).astype(np.int64), 0, ncx - 1)
    cy = np.clip(np.floor((pos[:nf, 1] - y0) / cs).astype(np.int64), 0, ncy - 1)
    order = np.lexsort((np.arange(nf), cx * ncy + cy))
    per_wave = 64 // lanes
    n_waves = -(-nf // per_wave)
    has = np.zeros(n_waves * per_wave, dtype=bool)
    has[:nf] = n_wall[order] > 0
    wall_waves = int(np.count_nonzero(has.reshape(n_waves, per_wave).any(axis=1)))
    third = int(np.count_nonzero((n_wall > 0) & ((n_all - 1) // lanes >= 2)))
    return dict(waves=int(n_waves), wall_waves=wall_waves, interior_waves=int(n_waves - wall_waves),
                wall_particles=int(np.count_nonzero(n_wall)), third_row_walls=third, list_max=int(n_all.max()))


def check_census(case, c):
    """The classes the case is there for are present (c: census())."""
    if case in BOTH_CLASSES:
        assert c["wall_waves"] > 0 and c["interior_waves"] > 0, (case, c)
    if case in INTERIOR_MAJORITY:
        assert c["interior_waves"] > c["wall_waves"], (case, c)
    if case in THIRD_WALL_ROW:
        assert c["third_row_walls"] > 0, (case, c)


def _scalars(st, mon):
    tb, tt, npairs = mon
    return dict(t=st["t"], dt_last=st["dt_last"], vmax=st["vmax"], pairs=npairs, tau_bottom=tb, tau_top=tt)


def _run_context(capi, prm, parts, lpp, kw, want_census=True):
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=lpp, **kw) as ctx:
        info, tuning, sched, policy = ctx.info(), ctx.tuning(), ctx.schedule(), ctx.grid_policy()
        c = None
        if want_census:
            nl = ctx.neighbor_list()
            y0 = float(np.min(parts["pos"][:, 1]))
            c = census(nl[0], nl[1], parts["pos"], parts["n_fluid"], lpp, prm.DL, info["n_cell_x"], info["n_cell_y"], y0,
                       2.0 * prm.h + policy["skin"])
        st = ctx.advance(1e9, max_steps=STEPS)
        got = ctx.download()
        mon = ctx.monitor(tau=True, pairs=True)
        after = ctx.schedule()
        facts = dict(block_size=tuning["block_size"], lanes=tuning["lanes_per_particle"], fuse_ea=sched["fuse_ea"],
                     tail_clock=sched["tail_clock"], dynamic=sched["dynamic"], steps=int(st["step"]), substeps=ctx.substeps(),
                     rebins=int(after["rebins"] - sched["rebins"]), n_fluid=int(info["n_fluid"]), n_wall=int(info["n_wall"]),
                     n_cell_x=int(info["n_cell_x"]), n_cell_y=int(info["n_cell_y"]), skin=policy["skin"], census=c,
                     finite=bool(all(np.all(np.isfinite(got[k])) for k in FIELDS)))
    return {**{k: got[k] for k in FIELDS}, **{k: np.asarray(v) for k, v in _scalars(st, mon).items()}}, facts


def _run_batch(capi, prm, members, lpp):
    with capi.Batch.from_parts([prm] * len(members), members, t_end=1e9, lanes_per_particle=lpp) as b:
        sts = b.advance(1e9, max_steps=STEPS)
        outs = [{**b.download(m), **{k: np.asarray(v) for k, v in _scalars(sts[m], b.monitor(m, tau=True, pairs=True)).items()}}
                for m in range(len(members))]
        info = b.info()
    alone = [_run_context(capi, prm, pa, lpp, {}, want_census=False) for pa in members]
    same = all(outs[m][k].tobytes() == alone[m][0][k].tobytes() for m in range(len(members)) for k in ARRAYS)
    facts = dict(alone[0][1], members=int(info["n_members"]), lanes=int(info["lanes_per_particle"]),
                 steps=[int(s["step"]) for s in sts], members_equal_contexts=bool(same),
                 finite=bool(all(np.all(np.isfinite(o[k])) for o in outs for k in FIELDS)))
    return {k: np.stack([o[k] for o in outs]) for k in ARRAYS}, facts


def main():
    out_dir, names = sys.argv[1], sys.argv[2:] or list(CASES)
    os.makedirs(out_dir, exist_ok=True)
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    facts = {}
    for name in names:
        for lpp in LANES:
            prm, parts, kw = CASES[name](pkg.config, pkg.geometry)
            if name == "batch4":
                arrays, f = _run_batch(pkg.capi, prm, parts, lpp)
            else:
                arrays, f = _run_context(pkg.capi, prm, parts, lpp, kw)
                check_census(name, f["census"])
            np.savez(os.path.join(out_dir, f"{name}_lpp{lpp}.npz"), **arrays)
            facts[f"{name}_lpp{lpp}"] = f
    print(json.dumps(dict(switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), runs=facts)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
