"""-m gpu: the opt-in dual-rate loop (sphx_params.dual_rate = 2..4), particle by particle against a reference of the same
operation.

Reference: tests/dual_rate_reference.py -- one outer step of the oracle's neighbour search, density / KGC, viscous force and
transport shift, then n_in times the oracle's integration_verlet on the carried state with the pair list, Vol, B and
force_prior of the outer step's start.  tests/test_dual_rate_reference.py shows on the CPU that it is oracle.run to the bit
at n_in = 1, that it tells a stale drho_dt, the wrong velocity buffer, or pairs / viscous force refreshed in an inner sub-step
from the right loop by >= 1e-3, and that every start below is conditioned to <= 1e-12 for a 1e-15 perturbation.

Channel: dp = 0.05, DL = 1.5, DH = 1 -- 600 fluid particles, at most 20 acoustic sub-steps per case.  What each case reaches
in the kernels (forces_pass with later = 1, continuity_body with next_half = 1, inner_substeps in the launch layer):

  A  plain, 32 lanes, n_in 2, 10 outer   one row or none per lane; lanes that prefetch their own record
  B  plain, 16 lanes, n_in 2, 10 outer   one to two rows
  C  plain, 16 lanes, n_in 3,  6 outer   odd sub-step count: the vel2 / output ping-pong of inner_substeps
  D  plain, 32 lanes, n_in 4,  5 outer   the maximum
  E  squeezed at the bottom wall, 16 lanes, n_in 2, 6 outer   more than two rows with wall rows behind the prefetched ones:
     `continue` in the `later` remainder loop, the second wall loop reading again; max |v| grows from 1 to 7, so dt changes
     by a quarter from one outer step to the next (the limit is still the acoustic one: the advective one needs
     max |v| > c_f / (n_in - 1) = 15)
  F  squeezed at the periodic seam, 16 lanes, n_in 2, 6 outer   the same across the minimum image
  G  squeezed at the top wall, 16 lanes, n_in 3, 4 outer   top wall, odd count
  H  moving walls, uneven mass, rho0 = 2.5, 16 and 32 lanes, n_in 2, 10 outer   per-particle wall velocity in the inner
     continuity pass
  I  plain, 16 lanes, n_in 2, rebuild_every 4, 10 outer   re-binning between outer steps (fold_rebin is off for n_in > 1)
  J  plain, 16 lanes, n_in 2, advance(2.5 Dt_first) then advance(1e9, max_steps = 2)   the last outer step clipped to the
     target, then resumed; compared after each call
  K  squeezed at the bottom wall, 16 lanes, n_in 4, 3 outer   max |v| ~ 9 > c_f / 3: the advective limit of next_dt sets Dt
  L  plain with U_bulk < 0, 16 lanes, n_in 2, 10 outer   the flow to the left: the periodic wrap xo < 0 in the inner sub-steps

Bound: RTOL = 1e-10 in max|a - b| / max|b| per field and for dt and max |v| -- tests/test_gpu_headline_parity.py's bound for up
to 35 steps of the same formulas in another summation order; t to 1e-12 relative; the step count exactly.  Every case runs
twice and must repeat to the bit.
"""
import numpy as np
import pytest

import dual_rate_reference as drr

pytestmark = pytest.mark.gpu

RTOL = 1e-10  # tests/test_gpu_headline_parity.py, RTOL[20] and RTOL[35]


def _gpu(capi, prm, parts, calls, **kw):
    """calls: [(t_target, max_steps), ...] -> context facts, [(status, download) after each call]."""
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        info = dict(tuning=ctx.tuning(), policy=ctx.grid_policy(), sched=ctx.schedule(), substeps=ctx.substeps())
        outs = []
        for t_target, max_steps in calls:
            st = ctx.advance(t_target, max_steps=max_steps)
            outs.append((st, ctx.download()))
        info["sched_after"], info["policy_after"] = ctx.schedule(), ctx.grid_policy()
    return info, outs


def _check(name, capi, capsys, prm, parts, lanes, n_in, calls, **kw):
    kw = dict(kw, lanes_per_particle=lanes, dual_rate=n_in)
    info, outs = _gpu(capi, prm, parts, calls, **kw)
    _, outs2 = _gpu(capi, prm, parts, calls, **kw)
    assert info["substeps"] == n_in == drr.substeps(prm, n_in), info
    assert info["tuning"]["lanes_per_particle"] == lanes, info
    ref, steps = None, 0
    for n, ((st, got), (st2, got2), (t_target, max_steps)) in enumerate(zip(outs, outs2, calls)):
        assert st == st2
        for k, v in got.items():
            assert np.array_equal(v, got2[k]), f"{name}: {k} differs between two runs (call {n})"
        ref = drr.run(prm, parts, n_in, t_target=t_target, max_outer=max_steps, state=ref)
        assert ref["steps"] > steps  # (every call of a case takes steps)
        steps = ref["steps"]
        err = drr.errors(got, ref)
        e_t, e_dt = abs(st["t"] - ref["t"]) / ref["t"], abs(st["dt_last"] - ref["dt_last"]) / ref["dt_last"]
        e_v = abs(st["vmax"] - ref["vmax"]) / ref["vmax"]
        with capsys.disabled():
            print(f"\n[dual-rate parity] {name} call {n}: {st['step']} outer x {n_in}, vmax {ref['vmax']:.3g}: max rel err "
                  + " ".join(f"{k}={v:.1e}" for k, v in err.items()) + f" | t {e_t:.1e} dt {e_dt:.1e} vmax {e_v:.1e}")
        assert st["step"] == ref["steps"], (st, ref["steps"])
        assert e_t <= 1e-12 and e_dt <= RTOL and e_v <= RTOL, (e_t, e_dt, e_v)
        for k, e in err.items():
            assert e <= RTOL, f"{name}:{k} (call {n}): {e:.3e} > {RTOL:.0e}"
    return info, outs


# cases A to H, K and L of drr.GPU_CASES (the table whose starts and lengths the CPU tests check for conditioning), one per lane count
STEPPED = [(k if len(lanes) == 1 else f"{k}{l}", start, l, n_in, n_outer)
           for k, (start, lanes, n_in, n_outer) in drr.GPU_CASES.items() if k not in ("I", "J") for l in lanes]


@pytest.mark.parametrize("case,start,lanes,n_in,n_outer", STEPPED, ids=[c[0] for c in STEPPED])
def test_dual_rate_matches_the_reference(case, start, lanes, n_in, n_outer, cfgmod, geom, capi, oracle, capsys):
    prm, parts = drr.start(cfgmod, geom, start)
    n_all, n_wall = drr.counts_within(prm, parts, 2.0 * prm.h)
    if start in ("bottom", "top", "seam"):  # more than two rows of 16, wall rows behind the prefetched ones
        assert np.any((n_all > 32) & (n_wall > 0))
    elif start in ("plain", "left"):
        assert 16 < n_all.max() <= 32
    _, outs = _check(f"{case} {start} {lanes} lanes", capi, capsys, prm, parts, lanes, n_in, [(1e9, n_outer)])
    st = outs[0][0]
    if case == "E":
        assert st["vmax"] > 5.0, st
    if case == "K":  # the advective limit is the smaller one (tests/test_dual_rate_reference.py shows it on the reference)
        assert st["vmax"] * (n_in - 1) > prm.c_f, st


def test_dual_rate_rebinning_between_outer_steps(cfgmod, geom, capi, oracle, capsys):
    prm, parts = drr.start(cfgmod, geom, "plain")
    info, _ = _check("I plain 16 lanes K=4", capi, capsys, prm, parts, 16, 2, [(1e9, 10)], rebuild_every=4)
    assert info["policy"]["rebuild_every"] == 4, info
    rebins = info["sched_after"]["rebins"] - info["sched"]["rebins"]
    forced = info["policy_after"]["forced_rebuilds"] - info["policy"]["forced_rebuilds"]
    assert rebins + forced >= 2, info


def test_dual_rate_clipped_to_a_target_then_resumed(cfgmod, geom, capi, oracle, capsys):
    prm, parts = drr.start(cfgmod, geom, "plain")
    t1 = 2.5 * drr.first_outer_step(prm, parts, 2)
    _, outs = _check("J plain 16 lanes", capi, capsys, prm, parts, 16, 2, [(t1, 0), (1e9, 2)])
    (st1, _), (st2, _) = outs
    assert st1["step"] == 3 and abs(st1["t"] - t1) <= 1e-12  # two full outer steps and a clipped one
    assert st1["dt_last"] < 0.75 * drr.first_outer_step(prm, parts, 2) / 2
    assert st2["step"] == 5 and st2["dt_last"] > st1["dt_last"]
