"""-m gpu: the resident step loop in the regimes the suite's default states never enter (tests/regime_cases.py): flow to the
left (the periodic wrap at x < 0, re-binning of a particle that re-enters in the last column), c_f = 0.3 (hundreds of pairs on
the cap and on the linear part of the Riemann dissipation fmin(3 max(du, 0), c_f), and a flow that outruns the cell skin, so
the drift bound forces re-binnings), mu = 2 (the viscous dt binds on every step), g = -100 from rest (the body dt binds, then
the acoustic one) and the density floor of the half step.  tests/test_regime_cases.py proves on the CPU, with the oracle
alone, that each case enters its branch; here every kernel family (lanes per particle 0 = the library's choice, 2 and 4: the
walk forms, 16 and 32: the compact ones) steps each case against the oracle.

The comparison is test_gpu_resident._steps_match_oracle's, tolerances unchanged: the nine fields to rtol 1e-9 + 1e-10 of the
field's largest magnitude, t to 1e-13, dt to 1e-12, max |v| to 1e-9, the pair count exactly, both tau to 1e-8.  Two summation
orders of the reference arithmetic (serial against OpenMP oracle) differ by at most 9e-14 of a field's magnitude after 35
steps of any of these cases -- no more than on the default states -- so the tolerances keep three decades of margin."""
import numpy as np
import pytest

import regime_cases as rc
from helpers import assert_close, full_state
from test_gpu_resident import _steps_match_oracle

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
LANES = [0, 2, 4, 16, 32]
STEPPED = [(name, lanes, n) for name in ("leftward", "capped", "left_capped", "viscous", "body") for lanes in LANES
           for n in ((3, 12) if name == "body" else (3, 35))]
_built = {}


def _case(cfgmod, geom, name, size="small"):
    if (name, size) not in _built:
        _built[name, size] = rc.CASES[name](cfgmod, geom, size) if name in rc.CASES else getattr(rc, name)(cfgmod, geom, size)
    return _built[name, size]


def _rel(a, b):
    return abs(a - b) / abs(b)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lanes,n_steps", STEPPED, ids=[f"{c}-lpp{l}-{n}" for c, l, n in STEPPED])
def test_every_kernel_family_in_every_regime(name, lanes, n_steps, cfgmod, geom, capi, oracle, capsys):
    prm, parts = _case(cfgmod, geom, name)
    nf = parts["n_fluid"]
    _steps_match_oracle((prm, parts, lanes), capi, oracle, n_steps)
    # once more for what that comparison does not look at: the schedule, the first dt, the errors as figures
    ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n_steps, enable_sort=False)
    with capi.Context.from_parts(prm, parts, lanes_per_particle=lanes, t_end=1e9) as ctx:
        forms, before = ctx.kernel_forms(), ctx.schedule()
        first = ctx.advance(1e9, max_steps=1)
        st = ctx.advance(1e9, max_steps=n_steps - 1)
        got = ctx.download()
        after, policy = ctx.schedule(), ctx.grid_policy()
    assert st["step"] == n_steps
    if lanes:
        assert forms["walk_kernels"] == (lanes < 16), forms
    err = {k: float(np.max(np.abs(got[k] - ref[k])) / max(np.max(np.abs(ref[k])), 1e-300)) for k in FIELDS}
    with capsys.disabled():
        print(f"\n[regimes] {name} lanes {lanes} ({'walk' if forms['walk_kernels'] else 'compact'}) {n_steps} steps: rebins "
              f"{after['rebins'] - before['rebins']} forced {policy['forced_rebuilds']} worst {max(err.values()):.1e} | "
              + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    for k in FIELDS:    # one advance or 1 + (n - 1): the same steps
        assert_close(got[k], ref[k], rtol=1e-9, atol_scale=1e-10, name=f"{k}@1+{n_steps - 1}")
    x = got["pos"][:nf, 0]
    assert np.all(x >= 0.0) and np.all(x <= prm.DL)
    if n_steps >= 35:
        assert after["rebins"] > before["rebins"], (before, after, policy)     # crossers have been re-binned
    if name == "viscous":
        assert _rel(first["dt_last"], rc.dt_viscous(prm)) <= 1e-12 and _rel(st["dt_last"], rc.dt_viscous(prm)) <= 1e-12
    if name == "body":
        assert _rel(first["dt_last"], rc.dt_body(prm)) <= 1e-12, (first["dt_last"], rc.dt_body(prm))
        if n_steps == 12:                                                      # by then the acoustic limit has taken over
            assert st["dt_last"] < 0.9 * rc.dt_body(prm)
            assert _rel(st["dt_last"], ref["stats"]["dt_last"]) <= 1e-12
    if name in ("leftward", "left_capped", "body"):
        assert np.mean(got["vel"][:nf, 0]) < 0.0


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 3, 10])
@pytest.mark.parametrize("lanes", [2, 16])
def test_density_floor_on_the_device(lanes, n_steps, cfgmod, geom, capi, oracle):
    """The half-step floor `rho_half < 1e-10 -> rho0` of pass A / pass E.  A step ends with rho = rho_half + drho_dt dt / 2 and
    p = p0 (rho / rho0 - 1), so p is not 0 after the step (the oracle: 0.41 and -0.37 on the two rows, against -85 and 9.5
    without the floor); what shows the floor is rho == rho0 + drho_dt dt / 2 with the constant rho0 (regime_cases.floored_rows)
    -- exactly on the oracle, to 2 ulp of rho0 on the device, whose closing update may be a fused multiply-add -- and p, rho
    and every other field of those rows matching the oracle at the file's tolerances."""
    prm, parts = _case(cfgmod, geom, "floor")
    nf = parts["n_fluid"]
    _steps_match_oracle((prm, parts, lanes), capi, oracle, n_steps)
    if n_steps == 1:
        ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=1, enable_sort=False)
        with capi.Context.from_parts(prm, parts, lanes_per_particle=lanes, t_end=1e9) as ctx:
            st = ctx.advance(1e9, max_steps=1)
            got = ctx.download(fields=("rho", "p", "drho_dt"))
        rows = list(rc.FLOOR_ROWS)
        assert rc.floored_rows(prm, ref, nf) == rows
        assert rc.floored_rows(prm, dict(got, dt_last=st["dt_last"]), nf, ulps=2) == rows
        assert_close(got["p"][rows], ref["p"][rows], rtol=1e-9, atol=1e-10 * np.max(np.abs(ref["p"])), name="p of the floored rows")
        assert np.all(np.abs(got["p"][rows]) < 0.01 * prm.p0)        # (without the floor: -34 p0 and more)


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 16])
@pytest.mark.parametrize("name", ["left_capped", "body"])
def test_call_patterns_agree_to_the_bit(name, lanes, cfgmod, geom, capi):
    """N steps as one advance, as graph replays of four steps, and as single-step calls: identical bits (as
    test_gpu_resident.test_graph_and_eager_agree).  left_capped outruns the cell skin, so the device stops the loop for forced
    re-binnings on the way: they, too, must not depend on how the host chunks its calls."""
    prm, parts = _case(cfgmod, geom, name)
    n = 13
    outs = []
    for kw, single in ((dict(), False), (dict(steps_per_graph=4), False), (dict(steps_per_graph=4), True)):
        with capi.Context.from_parts(prm, parts, lanes_per_particle=lanes, t_end=1e9, **kw) as ctx:
            if single:
                for _ in range(n):
                    st = ctx.advance(1e9, max_steps=1)
            else:
                st = ctx.advance(1e9, max_steps=n)
            assert st["step"] == n
            outs.append(dict(ctx.download(), t=st["t"], dt_last=st["dt_last"], vmax=st["vmax"]))
    for what, other in (("graph replays", outs[1]), ("single steps", outs[2])):
        for k, v in outs[0].items():
            assert np.array_equal(np.asarray(v), np.asarray(other[k])), f"{name} lanes {lanes}: {k} differs between one advance and {what}"


@pytest.mark.parametrize("lanes", [2, 16])
@pytest.mark.parametrize("name", ["left_capped", "body"])
def test_target_time_clipping(name, lanes, cfgmod, geom, capi, oracle):
    """advance(t_target) lands on the target with a last dt clipped by `remain` (SPH_Poiseuille.m:252), as the oracle's loop
    (test_gpu_resident.test_target_time_clipping); for `body` the clipped step follows body- and acoustic-limited ones."""
    prm, parts = _case(cfgmod, geom, name)
    nf = parts["n_fluid"]
    dt0 = rc.dt_body(prm) if name == "body" else 0.25 * prm.h / (prm.c_f + 1.0)
    target = 7.3 * dt0
    ref = oracle.run(prm, parts, t_end=target, output_interval=target, enable_sort=False)
    n_ref = ref["stats"]["steps"]
    before = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n_ref - 1, enable_sort=False)["stats"]["dt_last"]
    assert n_ref >= 8 and ref["stats"]["dt_last"] < 0.9 * before                      # the last step was clipped
    with capi.Context.from_parts(prm, parts, lanes_per_particle=lanes, t_end=1e9) as ctx:
        st = ctx.advance(target)
        assert st["done"] == 1 and abs(st["t"] - target) < 1e-12
        assert st["step"] == ref["stats"]["steps"]
        assert abs(st["dt_last"] - ref["stats"]["dt_last"]) <= 2e-13 * target      # target - t, with t to 1e-13 on either side
        st2 = ctx.advance(target)
        assert st2["step"] == st["step"]
        got = ctx.download()
    for k in FIELDS:
        assert_close(got[k], ref[k], rtol=1e-9, atol_scale=1e-10, name=k)
    assert np.all(got["pos"][:nf, 0] >= 0) and np.all(got["pos"][:nf, 0] <= prm.DL)


# 4 ---------------------------------------------------------------------------------------------------------------
MEMBERS = ("default", "leftward_plain", "capped", "viscous_plain")    # fixed walls, even mass: what a batch shares


def regime_members(cfgmod, geom, size="small"):
    """Four channels on one geometry that differ in mu, c_f, p0, gravity_g and their state: today's default physics, the flow
    to the left, c_f = 0.3 and mu = 2 (the plain make_case forms of the regime cases, so that the walls can be shared)."""
    members = [getattr(rc, name)(cfgmod, geom, size) for name in MEMBERS]
    for prm, parts in members[1:]:
        assert np.array_equal(parts["mass"], members[0][1]["mass"]) and np.array_equal(parts["wall_vel"], members[0][1]["wall_vel"])
        assert np.array_equal(parts["pos"][parts["n_fluid"]:], members[0][1]["pos"][parts["n_fluid"]:])
    return members


@pytest.mark.parametrize("lanes", [16, 32])
def test_batch_of_four_regimes_is_bit_identical_to_standalone(lanes, cfgmod, geom, capi):
    """enqueue_steps(20) on the batch and on four standalone contexts.  A member that never fell out of step is bit for bit its
    standalone context; a drift-forced re-binning re-bins ALL members of a batch, which a standalone context would not do at
    that step, so the interval and the skin are given: K = 4 with a skin of 1.6 h.  Measured on the oracle over these 20 steps,
    the largest distance a particle covers in three steps is 0.39 h in the fastest member (c_f = 0.3, whose dt is the viscous
    one, five times the default's) and 0.23 h or less in the others: well inside the half skin of 0.8 h; that no re-binning was
    forced and no member realigned is asserted."""
    members = regime_members(cfgmod, geom)
    kw = dict(t_end=1e9, lanes_per_particle=lanes, rebuild_every=4, skin_h=1.6)
    n = 20
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        assert b.info()["lanes_per_particle"] == lanes and b.info()["rebuild_every"] == 4
        b.enqueue_steps(n)
        sts = b.sync()
        got = [full_state(b.download(m), sts[m], b.monitor(m, tau=True, pairs=True)) for m in range(len(members))]
        info = b.info()
    assert info["realignments"] == 0 and info["forced_rebuilds"] == 0, info
    for m, (prm, parts) in enumerate(members):
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.enqueue_steps(n)
            st = ctx.sync()
            ref = full_state(ctx.download(), st, ctx.monitor(tau=True, pairs=True))
            assert ctx.grid_policy()["forced_rebuilds"] == 0
        assert got[m]["step"] == n
        for k in ref:
            assert np.array_equal(np.asarray(got[m][k]), np.asarray(ref[k])), f"member {m} ({MEMBERS[m]}) lanes {lanes}: {k} differs"
    dts = [g["dt_last"] for g in got]
    assert dts[3] < 0.3 * dts[0] and dts[2] > 3.0 * dts[0] and got[1]["tau"][0] < 0 < got[0]["tau"][0]   # four physics indeed


@pytest.mark.parametrize("lanes", [16, 32])
def test_batch_of_four_regimes_reaches_one_time_in_different_step_counts(lanes, cfgmod, geom, capi, oracle):
    """advance(t_target) with the library's own interval and skin: the viscous member needs about four times the steps of the
    default one, the capped one a fifth; the batch realigns them, and each member matches the oracle's loop to the same time."""
    members = regime_members(cfgmod, geom)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    t1 = 10.3 * dt0
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=lanes) as b:
        sts = b.advance(t1)
        got = [b.download(m) for m in range(len(members))]
        taus = [b.monitor(m, tau=True, pairs=True) for m in range(len(members))]
        info = b.info()
    steps = [s["step"] for s in sts]
    assert all(s["done"] == 1 and abs(s["t"] - t1) < 1e-12 for s in sts), sts
    assert steps[3] >= 3 * steps[0] and 3 * steps[2] < steps[0] and info["realignments"] >= 1, (steps, info)
    for m, (prm, parts) in enumerate(members):
        ref = oracle.run(prm, parts, t_end=t1, output_interval=t1, enable_sort=False)
        assert steps[m] == ref["stats"]["steps"], (MEMBERS[m], steps, ref["stats"]["steps"])
        for k in FIELDS:
            assert_close(got[m][k], ref[k], rtol=1e-9, atol_scale=1e-10, name=f"{MEMBERS[m]}.{k}")
        assert_close(np.array(taus[m][:2]), np.array([ref["stats"]["tau_bottom"], ref["stats"]["tau_top"]]), rtol=1e-8,
                     atol_scale=1e-9, name=f"{MEMBERS[m]}.tau")
        assert taus[m][2] == ref["stats"]["n_pairs_last"]
