"""-m gpu: the profile series of a batch (include/sphx.h section 2k) -- k_profile_series_b records every member's series in
one launch per step slot.  Members that fall out of step keep their own step / t series and record counts and are bit for bit
standalone contexts; a member that overflows counts its own dropped records; with several workgroups per member the ticket
and the int64 sums are per member; driver.run_sweep hands every member its series and the table its figures."""
import ctypes as C

import numpy as np
import pytest

import profile_series_cases as sc
from helpers import err_id, make_case

pytestmark = pytest.mark.gpu

MU = (0.05, 0.1, 0.2, 0.1)


def _members(cfgmod, geom):
    """Four members of dp05 with mu in MU; the last shares its mu with member 1 and has a perturbed initial state (its own
    jitter and noise).  Every member's dt is acoustic (0.25 h / (c_f + max|v|) = 1.0e-3 against 0.125 h^2 / nu >= 2.6e-3), so
    the clocks differ by the members' max|v| alone: out of step in t within a step, and by a step at a target time chosen
    between the members' times after 25 steps."""
    return [make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=21 if m < 3 else 99, developed=True, mu=mu)
            for m, mu in enumerate(MU)]


def _standalone(capi, members, target, cfg, **kw):
    refs, steps = [], []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.profile_series_enable(**cfg)
            steps.append(ctx.advance(target)["step"])
            refs.append(ctx.profile_series_sums())
    return refs, steps


def _target(capi, members, n=25, **kw):
    """a time between the members' times after n steps: some reach it in n steps, the others need one more"""
    t_n = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            t_n.append(ctx.advance(1e9, max_steps=n)["t"])
    ts = sorted(t_n)
    assert len(set(ts)) == len(ts), ts
    return 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])


# 1, 2 ------------------------------------------------------------------------------------------------------------
def test_members_out_of_step_equal_standalone_contexts(cfgmod, geom, capi, profmod):
    members = _members(cfgmod, geom)
    bands = sc.bands(members[0][0])
    target = _target(capi, members)
    cfg = dict(every=1, capacity=64, bands=bands)
    refs, steps = _standalone(capi, members, target, cfg)
    assert len(set(steps)) > 1 and all(24 <= s <= 27 for s in steps), steps
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.profile_series_enable(**cfg)
        sts = b.advance(target)
        got = b.profile_series_sums()
        prof = b.profile_series()
    assert [s["step"] for s in sts] == steps
    for m in range(4):
        assert len(got[m]["step"]) == steps[m] and got[m]["count"].shape == (steps[m], 3, 20)
        sc.assert_series_identical(got[m], refs[m], f"member {m}")
        assert np.array_equal(prof[m]["u_mean"], profmod.profile_series_profiles(members[m][0].DH, refs[m])["u_mean"], equal_nan=True)
    assert len({len(g["step"]) for g in got}) > 1                       # record counts differ between members
    assert len({g["t"][:20].tobytes() for g in got}) == 4               # each on its own clock
    # a member that overflows: capacity = the smallest member's count
    cap = min(steps)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.profile_series_enable(**dict(cfg, capacity=cap))
        b.advance(target)
        full = b.profile_series_sums()
    assert [f["n_dropped"] for f in full] == [s - cap for s in steps] and any(f["n_dropped"] == 0 for f in full)
    for m in range(4):
        sc.assert_series_identical(full[m], {k: refs[m][k][:cap] for k in sc.SERIES}, f"member {m}, capacity {cap}", counters=False)


# 3 ---------------------------------------------------------------------------------------------------------------
def test_several_workgroups_per_member(cfgmod, geom, capi):
    """30 k fluid particles a member: eight workgroups per grid row of k_profile_series_b, a ticket and int64 sums per member"""
    members = [make_case(cfgmod, geom, dp=0.01, DL=3.0, jitter=0.2, seed=31 + m, developed=True, mu=mu) for m, mu in enumerate((0.1, 0.15))]
    assert members[0][1]["n_fluid"] > 2 * 4096
    bands = sc.bands(members[0][0])
    cfg = dict(every=2, capacity=16, bands=bands)
    kw = dict(lanes_per_particle=16)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.profile_series_enable(**cfg)
            ctx.advance(1e9, max_steps=12)
            refs.append(ctx.profile_series_sums())
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, **kw) as b:
        b.profile_series_enable(**cfg)
        b.advance(1e9, max_steps=12)
        b.profile_series_sample()
        got = b.profile_series_sums()
    for m in range(2):
        assert got[m]["step"].tolist() == [2, 4, 6, 8, 10, 12, 12] and got[m]["n_dropped"] == 0
        sc.assert_series_identical({k: got[m][k][:6] for k in sc.SERIES}, refs[m], f"member {m}", counters=False)
        for f in sc.FIELDS:
            assert np.array_equal(got[m][f][6], got[m][f][5]), f      # the sample of the state now: the last step's again
    assert not np.array_equal(got[0]["sum_ux"], got[1]["sum_ux"])


def test_batch_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = _members(cfgmod, geom)[:3]
    M = 3
    ok = capi.SphxProfileSeriesConfig(n_bins=0, every=1, capacity=16, t_from=0.0, n_bands=0)
    nothing = (None, None, None, None, None, None, 0)
    for fn, args in ((L.sphx_batch_profile_series_enable, (C.byref(ok),)), (L.sphx_batch_profile_series_disable, ()),
                     (L.sphx_batch_profile_series_sample, ()), (L.sphx_batch_profile_series_read, (0, *nothing))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    n, dropped = np.full(M, -1, dtype=np.int32), np.full(M, -1, dtype=np.int64)
    pn, pd = n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64))
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        assert err_id(capi, L.sphx_batch_profile_series_read, h, 0, *nothing) == ("SPHX:ProfileSeries:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_batch_profile_series_sample, h) == ("SPHX:ProfileSeries:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_batch_profile_series_disable(h) == capi.SPHX_OK       # no-op when off
        assert L.sphx_batch_profile_series_enable(h, C.byref(ok)) == capi.SPHX_OK
        b.advance(1e9, max_steps=5)
        # (20 bins x 1 band x 5 = 100 doubles a record: the cap of 1 << 27 doubles is taken over the members)
        for bad in (dict(every=0), dict(capacity=0), dict(n_bins=1537), dict(capacity=(1 << 27) // (100 * M) + 1)):
            c2 = capi.SphxProfileSeriesConfig(**dict(dict(n_bins=0, every=1, capacity=16, t_from=0.0, n_bands=0), **bad))
            assert err_id(capi, L.sphx_batch_profile_series_enable, h, C.byref(c2)) == ("SPHX:ProfileSeries:config", capi.SPHX_ERR_ARG), bad
        with pytest.raises(capi.SphxError) as e:
            b.profile_series_enable(capacity=(1 << 27) // (100 * M) + 1)
        assert e.value.identifier == "SPHX:ProfileSeries:config"
        assert L.sphx_batch_profile_series_read(h, 0, None, None, None, None, pn, pd, 0) == capi.SPHX_OK   # counts only
        assert list(n) == [5] * M and list(dropped) == [0] * M                # the refused enables left the series running
        times, records = np.full((M, 4, 2), -1.0), np.full((M, 4, 1, 20, 5), -1.0)
        assert err_id(capi, L.sphx_batch_profile_series_read, h, 4, capi.ptr(times), capi.ptr(records), None, None, None, None, 1) == \
            ("SPHX:ProfileSeries:capacity", capi.SPHX_ERR_ARG)
        assert np.all(times == -1.0) and np.all(records == -1.0)
        times, records = np.full((M, 7, 2), -1.0), np.full((M, 7, 1, 20, 5), -1.0)   # nothing was drained; rows beyond n_records stay
        assert L.sphx_batch_profile_series_read(h, 7, capi.ptr(times), capi.ptr(records), None, None, pn, None, 0) == capi.SPHX_OK
        for m in range(M):
            assert list(times[m, :5, 0]) == [1.0, 2.0, 3.0, 4.0, 5.0] and np.all(times[m, 5:] == -1.0) and np.all(records[m, 5:] == -1.0), m
            held = records[m, :5, 0, :, 0].sum(axis=1)                      # (a particle outside [0, DH] is not binned)
            assert np.all(held <= members[m][1]["n_fluid"]) and np.all(held >= members[m][1]["n_fluid"] - 2)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_run_sweep_sets_the_members_series(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, mu=mu, end_time=0.3, output_interval=0.1) for mu in (0.1, 0.15, 0.2)]
    res = driver.run_sweep(prms, history_capacity=1024, profiles_every=2)
    assert res.table["t_developed"].shape == (3,) and res.table["tau_fit"].shape == (3,)
    for m, r in enumerate(res.members):
        s = r.profile_series
        assert s["n_dropped"] == 0 and s["step"].tolist() == list(range(2, r.steps + 1, 2)), m   # no gap across the drains
        assert np.array_equal(s["t"], r.history["t"][1::2]) and s["u_mean"].shape == (r.steps // 2, 2, 20)
        alone = driver.run(prms[m], profiles_every=2).profile_series
        assert np.array_equal(s["step"], alone["step"]) and np.array_equal(s["count"], alone["count"]), m
        if res.grid_policy["realignments"] == 0:
            for k in sc.SERIES + ("u_mean", "u_std", "uy_mean", "uy_std"):
                assert np.array_equal(s[k], alone[k], equal_nan=True), (m, k)
        else:
            # the members reach an output point in different step counts and are then re-binned into one layout (include/sphx.h
            # section 2b, "realignment"): the summation order of the steps that follow differs from a standalone context's, so
            # the states agree to rounding carried through ~300 steps, not to the bit -- and the series, exact sums of the state,
            # with them.  1e-9 of U_max is five orders above that and four below the first digit a figure shows.
            u_max = prms[m].gravity_g * prms[m].DH ** 2 / (8.0 * prms[m].nu)
            assert np.max(np.abs(s["t"] - alone["t"])) <= 1e-12
            for k in ("u_mean", "uy_mean"):
                assert np.array_equal(np.isnan(s[k]), np.isnan(alone[k])), (m, k)
                assert np.nanmax(np.abs(s[k] - alone[k])) <= 1e-9 * abs(u_max), (m, k, float(np.nanmax(np.abs(s[k] - alone[k]))))
        fig = driver.profile_series_figures(prms[m], s)
        for k in ("t_developed", "tau_fit"):
            assert np.array_equal(res.table[k][m], fig[k], equal_nan=True), (m, k)
    assert len({r.profile_series["sum_ux"].tobytes() for r in res.members}) == 3
    assert all(r.profile_series is None for r in driver.run_sweep(prms, history_capacity=1024).members)
    with pytest.raises(RuntimeError, match=r"member 0.*profiles_capacity >= \d+ \(it is 4\)"):
        driver.run_sweep(prms, history_capacity=1024, profiles_every=2, profiles_capacity=4)
