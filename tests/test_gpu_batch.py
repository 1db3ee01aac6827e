"""-m gpu: batched contexts (sphx_batch_*, capi.Batch) -- M channels of one geometry stepped by the same launches.

Members that never fell out of step must be bit for bit standalone contexts with the same parameters; members that reach
one target time in different step counts are realigned (re-binned into one layout) and then match the oracle within the
tolerances of test_gpu_resident.py.
"""
import numpy as np
import pytest

from helpers import assert_close, batch_members, full_state, make_variant

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
# members differ in mu, c_f, transport_coeff and the seed of their initial state
VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=17.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=13.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]


def _assert_identical(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("lpp", [16, 32])
@pytest.mark.parametrize("dp,DL", [(0.05, 3.0), (0.025, 1.5)])
def test_bit_identical_to_standalone(cfgmod, geom, capi, dp, DL, lpp):
    members = batch_members(cfgmod, geom, dp, DL, VARIANTS)
    kw = dict(t_end=1e9, lanes_per_particle=lpp)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
        assert b.info()["lanes_per_particle"] == lpp and K > 1
    n = 3 * K + 1  # crosses at least two scheduled re-binnings
    for eager in (False, True):
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            if eager:  # one-step calls: every slot launched eagerly
                for _ in range(n):
                    sts = b.advance(1e9, max_steps=1)
                assert b.graph_stats()["slots_eager"] >= n
            else:
                sts = b.advance(1e9, max_steps=n)
                assert b.graph_stats()["slots_replayed"] > 0
            got = [full_state(b.download(m), sts[m], b.monitor(m, tau=True, pairs=True)) for m in range(len(members))]
            assert b.info()["realignments"] == 0
        for m, (prm, parts) in enumerate(members):
            with capi.Context.from_parts(prm, parts, **kw) as ctx:
                st = ctx.advance(1e9, max_steps=n)
                ref = full_state(ctx.download(), st, ctx.monitor(tau=True, pairs=True))
            assert got[m]["step"] == n
            _assert_identical(got[m], ref, f"member {m} eager={eager} dp={dp} lpp={lpp}")


def test_shared_moving_walls_and_uneven_mass(cfgmod, geom, capi, oracle):
    """One batch whose shared walls move and whose shared mass is uneven (helpers.make_variant, rho0 = 2.5); members differ in
    mu, c_f, transport_coeff and their state as above.  Bit for bit the standalone contexts; member 1 against the oracle."""
    members = []
    for v in VARIANTS:
        prm, parts = make_variant(cfgmod, geom, dp=0.05, DL=1.5, jitter=0.2, seed=v["seed"], developed=True, rho0=2.5, mu=v["mu"],
                                  c_f=v["c_f"], transport_coeff=v["transport_coeff"])
        if members:  # walls and masses are the batch's, not the member's
            parts.update(mass=members[0][1]["mass"], wall_vel=members[0][1]["wall_vel"])
        members.append((prm, parts))
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        n = 2 * b.info()["rebuild_every"] + 3
        sts = b.advance(1e9, max_steps=n)
        got = [full_state(b.download(m), sts[m], b.monitor(m, tau=True, pairs=True)) for m in range(len(members))]
        assert b.info()["realignments"] == 0
    for m, (prm, parts) in enumerate(members):
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            st = ctx.advance(1e9, max_steps=n)
            ref = full_state(ctx.download(), st, ctx.monitor(tau=True, pairs=True))
        _assert_identical(got[m], ref, f"member {m}, moving walls")
    prm, parts = members[1]
    ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n, enable_sort=False)
    _oracle_check(got[1], ref)
    assert_close(got[1]["tau"][0], ref["stats"]["tau_bottom"], rtol=1e-8, atol_scale=1e-9, name="tau_bottom")
    assert_close(got[1]["tau"][1], ref["stats"]["tau_top"], rtol=1e-8, atol_scale=1e-9, name="tau_top")
    assert got[1]["pairs"] == ref["stats"]["n_pairs_last"]


def test_rebuild_every_one_bit_identical_to_standalone(cfgmod, geom, capi):
    """No skin: every slot re-bins and the clock is a launch of its own (k_clock_scan with the cell scan), as one call and
    as one-step calls."""
    members = batch_members(cfgmod, geom, 0.05, 1.5, VARIANTS[:3])
    kw = dict(t_end=1e9, lanes_per_particle=16, rebuild_every=1)
    n = 9
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            st = ctx.advance(1e9, max_steps=n)
            refs.append(full_state(ctx.download(), st, ctx.monitor(tau=True, pairs=True)))
    for eager in (False, True):
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            assert b.info()["rebuild_every"] == 1
            if eager:
                for _ in range(n):
                    sts = b.advance(1e9, max_steps=1)
            else:
                sts = b.advance(1e9, max_steps=n)
            got = [full_state(b.download(m), sts[m], b.monitor(m, tau=True, pairs=True)) for m in range(len(members))]
            assert b.info()["realignments"] == 0
        for m in range(len(members)):
            assert got[m]["step"] == n
            _assert_identical(got[m], refs[m], f"member {m} eager={eager}, rebuild_every=1")


def test_single_member_equals_standalone(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.025, 1.5, VARIANTS[1:2])
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        st = b.advance(1e9, max_steps=37)[0]
        got = full_state(b.download(0), st, b.monitor(0, tau=True, pairs=True))
    with capi.Context.from_parts(*members[0], t_end=1e9) as ctx:
        st = ctx.advance(1e9, max_steps=37)
        ref = full_state(ctx.download(), st, ctx.monitor(tau=True, pairs=True))
    _assert_identical(got, ref, "M = 1")


def test_no_cross_talk(cfgmod, geom, capi):
    variants = [dict(VARIANTS[k % 4], seed=100 + k) for k in range(64)]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    kw = dict(t_end=1e9, lanes_per_particle=16)

    def run(mem):
        with capi.Batch.from_parts(*zip(*mem), **kw) as b:
            b.advance(1e9, max_steps=20)
            return {m: b.download(m) for m in (0, 5, 31, 63)}

    base = run(members)
    prm5, parts5 = members[5]
    pert = dict(parts5, vel=parts5["vel"].copy(order="F"))
    pert["vel"][: parts5["n_fluid"], 1] += 1e-3
    other = run(members[:5] + [(prm5, pert)] + members[6:])
    for m in (0, 31, 63):
        _assert_identical(other[m], base[m], f"member {m} after perturbing member 5")
    assert not np.array_equal(other[5]["vel"], base[5]["vel"])


def _oracle_check(got, ref):
    for k in FIELDS:
        assert_close(got[k], ref[k], rtol=1e-9, atol_scale=1e-10, name=k)


def test_time_target_realigns_and_matches_oracle(cfgmod, geom, capi, oracle):
    # different c_f: one target time in different step counts
    variants = [dict(VARIANTS[0], c_f=15.0), dict(VARIANTS[1], c_f=21.0), dict(VARIANTS[2], c_f=11.0)]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    t1, t2 = 10.3 * dt0, 17.9 * dt0
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
        sts = b.advance(t1)
        steps = [s["step"] for s in sts]
        assert len(set(steps)) > 1, steps
        assert all(s["done"] == 1 and abs(s["t"] - t1) < 1e-12 for s in sts)
        assert b.info()["realignments"] >= 1
        first = [b.download(m) for m in range(3)]
        sts2 = b.advance(t2)
        second = [b.download(m) for m in range(3)]
        taus = [b.monitor(m, tau=True) for m in range(3)]
    for m, (prm, parts) in enumerate(members):
        ref = oracle.run(prm, parts, t_end=t1, output_interval=t1, enable_sort=False)
        assert steps[m] == ref["stats"]["steps"]
        _oracle_check(first[m], ref)
        ref2 = oracle.run(prm, parts, t_end=t2, output_interval=t1, enable_sort=False)
        assert sts2[m]["step"] == ref2["stats"]["steps"]
        _oracle_check(second[m], ref2)
        assert_close(np.array(taus[m][:2]), np.array([ref2["stats"]["tau_bottom"], ref2["stats"]["tau_top"]]), rtol=1e-8,
                     atol_scale=1e-9, name="tau")


def test_drift_forced_rebinning_matches_oracle(cfgmod, geom, capi, oracle):
    """A skin far too thin for K (as test_gpu_grid_skin.py): the device stops the members, the batch re-bins all of them."""
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:3], jitter=0.3)
    n = 24
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16, rebuild_every=8, skin_h=0.03) as b:
        sts = b.advance(1e9, max_steps=n)
        got = [b.download(m) for m in range(3)]
        info = b.info()
    assert info["forced_rebuilds"] > 0 and info["realignments"] >= info["forced_rebuilds"]
    for m, (prm, parts) in enumerate(members):
        assert sts[m]["step"] == n
        ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n, enable_sort=False)
        _oracle_check(got[m], ref)


def test_diverging_member_is_named(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.05, 1.5, VARIANTS[:3], jitter=0.1)
    prm2, parts2 = members[2]
    bad = dict(parts2, vel=parts2["vel"].copy(order="F"))
    bad["vel"][3, 0] = np.nan
    members[2] = (prm2, bad)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        with pytest.raises(capi.SphxError) as e:
            b.advance(1e9, max_steps=4)
    assert e.value.code == capi.SPHX_ERR_DIVERGED
    assert "member 2" in e.value.message


def test_batch_of_only_diverging_members_raises(cfgmod, geom, capi):
    """A NaN in EVERY member: the host's step estimate has no finite max |v| to go by.  It used to come out as zero slots --
    advance() took no step and raised nothing.  Now one slot is enqueued and arming the clocks raises the status."""
    members = batch_members(cfgmod, geom, 0.05, 1.5, VARIANTS[:3], jitter=0.1)
    for m, (prm, parts) in enumerate(members):
        bad = dict(parts, vel=parts["vel"].copy(order="F"))
        bad["vel"][3, 0] = np.nan
        members[m] = (prm, bad)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        with pytest.raises(capi.SphxError) as e:
            b.advance(1e9, max_steps=4)
    assert e.value.code == capi.SPHX_ERR_DIVERGED
    assert "member 0" in e.value.message


def test_run_batch_matches_run(cfgmod, geom, driver):
    prms = [cfgmod.params_from_values(dp=0.025, DL=1.5, mu=mu, end_time=0.004, output_interval=0.002)
            for mu in (0.1, 0.15, 0.2)]
    res = driver.run_batch(prms)
    assert len(res) == 3
    for prm, r in zip(prms, res):
        one = driver.run(prm)
        assert r.steps == one.steps and abs(r.t - one.t) < 1e-12
        if r.grid_policy["realignments"] == 0:
            assert r.L2_error == one.L2_error
            assert np.array_equal(r.u_mean, one.u_mean, equal_nan=True)
        else:
            assert abs(r.L2_error - one.L2_error) <= 1e-9
            assert np.allclose(r.u_mean, one.u_mean, rtol=0, atol=1e-9, equal_nan=True)
        assert len(r.full_profile_u) == len(one.full_profile_u)
