"""-m gpu: flow statistics of batches (include/sphx.h section 2c, k_flow_stats_b) -- every member's time-averaged profile
accumulated inside the batch's step loop.  A member's sums must be bit for bit those of a standalone context with the same
config; in-loop samples equal samples taken between steps; idle members are not sampled; the physics is untouched;
driver.run_ensemble follows run_batch's trajectories and meets the acceptance bar of the single-context statistics."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_sums_identical, batch_members, err_id, stats_bands

pytestmark = pytest.mark.gpu

VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=17.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=13.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]
# (dp, DL): k_flow_stats_b runs ceil(n_fluid / 4096) workgroups per member (as k_flow_stats per context)
SIZES = {
    "one_workgroup": (0.05, 3.0),   # 1 200 fluid particles: one workgroup finishes a member's sample (no ticket)
    "two_workgroups": (0.025, 3.0),  # 4 800 (C2): two workgroups per member, global sums + ticket, last one out finishes
}


def _batch_sums(b, n_bands=3):
    """[member][band] sums dicts"""
    per_band = [b.flow_stats_sums(k) for k in range(n_bands)]
    return [[per_band[k][m] for k in range(n_bands)] for m in range(b.n_members)]


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpp", [16, 32])
@pytest.mark.parametrize("size", list(SIZES))
def test_members_equal_standalone_contexts(cfgmod, geom, capi, size, lpp):
    dp, DL = SIZES[size]
    members = batch_members(cfgmod, geom, dp, DL, VARIANTS)
    kw = dict(t_end=1e9, lanes_per_particle=lpp)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
        assert b.info()["lanes_per_particle"] == lpp and K > 1
    n = 3 * K + 1  # crosses re-binnings
    with capi.Context.from_parts(*members[0], **kw) as ctx:
        t_mid = ctx.advance(1e9, max_steps=n // 2)["t"]
    cfg = dict(every=3, t_from=t_mid, bands=stats_bands(members[0][0]))
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.flow_stats_enable(**cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            refs.append([ctx.flow_stats_sums(k) for k in range(3)])
    assert all(0 < r[0]["n_samples"] < n // 3 for r in refs)
    for eager in (False, True):
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            b.flow_stats_enable(**cfg)
            if eager:
                for _ in range(n):
                    sts = b.advance(1e9, max_steps=1)
                assert b.graph_stats()["slots_eager"] >= n
            else:
                sts = b.advance(1e9, max_steps=n)
                assert b.graph_stats()["slots_replayed"] > 0
            got = _batch_sums(b)
            assert b.info()["realignments"] == 0
        for m in range(len(members)):
            assert sts[m]["step"] == n
            assert_sums_identical(got[m], refs[m], f"{size} lpp={lpp} eager={eager} member {m}")


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_in_loop_equals_sampling_between_steps(cfgmod, geom, capi, size):
    dp, DL = SIZES[size]
    members = batch_members(cfgmod, geom, dp, DL, VARIANTS[:3])
    bands = stats_bands(members[0][0])
    N = 40
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.flow_stats_enable(every=1, bands=bands)
        b.advance(1e9, max_steps=N)
        in_loop = _batch_sums(b)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.flow_stats_enable(every=10 ** 9, bands=bands)
        for _ in range(N):
            b.advance(1e9, max_steps=1)
            b.flow_stats_sample()
        between = _batch_sums(b)
    for m in range(len(members)):
        assert in_loop[m][0]["n_samples"] == N
        assert_sums_identical(in_loop[m], between[m], f"{size} member {m}: in-loop vs between steps")


# 3 ---------------------------------------------------------------------------------------------------------------
def _dt_members(cfgmod, geom):
    variants = [dict(VARIANTS[0], c_f=15.0), dict(VARIANTS[1], c_f=21.0), dict(VARIANTS[2], c_f=11.0)]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    return members, 10.3 * dt0, 17.9 * dt0


@pytest.mark.parametrize("chunks", [False, True])
def test_idle_members_are_not_sampled(cfgmod, geom, capi, chunks):
    members, t1, t2 = _dt_members(cfgmod, geom)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
        b.flow_stats_enable(every=1, t_from=0.0, bands=stats_bands(members[0][0]))
        if chunks:
            b.advance(t1)
        sts = b.advance(t2)
        assert b.info()["realignments"] >= 1
        got = _batch_sums(b)
    steps = [s["step"] for s in sts]
    assert len(set(steps)) > 1, steps
    for m, s in enumerate(sts):
        assert abs(s["t"] - t2) < 1e-12
        for band in got[m]:
            assert band["n_samples"] == s["step"] and band["t_last"] == s["t"], (m, band["n_samples"], s)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_no_effect_on_the_physics(cfgmod, geom, capi):
    members, t1, t2 = _dt_members(cfgmod, geom)
    outs = []
    for on in (False, True):
        with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
            if on:
                b.flow_stats_enable(every=1, bands=stats_bands(members[0][0]))
            b.advance(t1)
            sts = b.advance(t2)
            assert b.info()["realignments"] >= 1
            outs.append((sts, [b.download(m) for m in range(len(members))]))
    assert outs[0][0] == outs[1][0]
    for m in range(len(members)):
        for k, v in outs[0][1][m].items():
            assert np.array_equal(v, outs[1][1][m][k]), (m, k)


def test_toggling_recaptures_graphs_and_keeps_the_states(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:3])
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.advance(1e9, max_steps=96)
        plain = [b.download(m, fields=("pos", "vel", "drho_dt")) for m in range(3)]
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.advance(1e9, max_steps=32)                       # graphs without the sampling kernel
        g0 = b.graph_stats()["graphs_captured"]
        b.flow_stats_enable(every=1)
        b.advance(1e9, max_steps=32)
        g1 = b.graph_stats()["graphs_captured"]
        assert g1 > g0
        assert [s["n_samples"] for s in b.flow_stats_sums(0)] == [32] * 3
        b.flow_stats_disable()
        b.advance(1e9, max_steps=32)
        assert b.graph_stats()["graphs_captured"] > g1
        with pytest.raises(capi.SphxError) as e:
            b.flow_stats(0)
        assert e.value.identifier == "SPHX:Stats:disabled"
        toggled = [b.download(m, fields=("pos", "vel", "drho_dt")) for m in range(3)]
        b.flow_stats_enable(every=2)
        b.flow_stats_sample()
        assert [s["n_samples"] for s in b.flow_stats_sums(0)] == [1] * 3
        b.flow_stats_reset()
        assert all(s["n_samples"] == 0 and not s["count"].any() for s in b.flow_stats_sums(0))
    for m in range(3):
        for k in plain[m]:
            assert np.array_equal(plain[m][k], toggled[m][k]), (m, k)


# 5 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:2])
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        none8 = (None, *[None] * 5, None, None, None)
        assert err_id(capi, L.sphx_batch_flow_stats_read, h, 0, 0, *none8) == ("SPHX:Stats:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_batch_flow_stats_sample, h)[0] == "SPHX:Stats:disabled"
        assert err_id(capi, L.sphx_batch_flow_stats_reset, h)[0] == "SPHX:Stats:disabled"
        assert L.sphx_batch_flow_stats_disable(h) == capi.SPHX_OK  # (off already: no-op)
        for bad in (dict(every=0), dict(every=-1), dict(n_bands=3), dict(n_bins=-1), dict(n_bins=1000)):
            c2 = capi.SphxFlowStatsConfig(n_bins=0, every=1, t_from=0.0, n_bands=1)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert err_id(capi, L.sphx_batch_flow_stats_enable, h, C.byref(c2)) == ("SPHX:Stats:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_batch_flow_stats_enable, h, None)[0] == "SPHX:Stats:config"
        assert err_id(capi, L.sphx_batch_flow_stats_read, h, 0, 0, *none8)[0] == "SPHX:Stats:disabled"  # still off
        cfg = capi.SphxFlowStatsConfig(n_bins=0, every=1, t_from=0.0, n_bands=1)
        assert L.sphx_batch_flow_stats_enable(h, C.byref(cfg)) == capi.SPHX_OK
        buf = [np.zeros(2 * 64) for _ in range(5)]
        args = [capi.ptr(x) for x in buf]
        assert err_id(capi, L.sphx_batch_flow_stats_read, h, 2, 64, None, *args, None, None, None)[0] == "SPHX:Stats:band"
        assert err_id(capi, L.sphx_batch_flow_stats_read, h, -1, 64, None, *args, None, None, None)[0] == "SPHX:Stats:band"
        n = C.c_int(0)
        assert L.sphx_batch_flow_stats_read(h, 0, 0, C.byref(n), *none8[1:]) == capi.SPHX_OK
        assert n.value == 20
        assert err_id(capi, L.sphx_batch_flow_stats_read, h, 0, n.value - 1, None, *args, None, None, None)[0] == "SPHX:Stats:capacity"
        ns = np.zeros(2, dtype=np.int64)
        assert L.sphx_batch_flow_stats_read(h, 1, 64, None, *args, ns.ctypes.data_as(C.POINTER(C.c_int64)), None, None) == capi.SPHX_OK
        assert list(ns) == [0, 0]


# 6 ---------------------------------------------------------------------------------------------------------------
def test_run_ensemble_follows_run_batch(cfgmod, geom, driver):
    prms = [cfgmod.params_from_values(dp=0.025, DL=1.5, mu=mu, end_time=0.004, output_interval=0.002)
            for mu in (0.1, 0.15, 0.2)]
    ref = driver.run_batch(prms)
    ens = driver.run_ensemble(prms, average_from=0.0)
    late = driver.run_ensemble(prms, average_from=0.0025, average_every=2)
    assert ens.pooled is None and len(ens.members) == 3  # (a sweep: nothing to pool)
    for m, (r, e, l) in enumerate(zip(ref, ens.members, late.members)):
        assert (e.steps, e.t) == (r.steps, r.t) and (l.steps, l.t) == (r.steps, r.t), m
        for k in ("pos", "vel"):
            assert np.array_equal(getattr(e, k), getattr(r, k)) and np.array_equal(getattr(l, k), getattr(r, k)), (m, k)
        assert e.L2_error == r.L2_error
        ta = e.time_avg
        assert ta["n_samples"] == r.steps and ta["t_last"] == r.t and 0.0 < ta["t_first"] < 0.002
        assert 0 < l.time_avg["n_samples"] < r.steps // 2 + 1 and l.time_avg["t_first"] >= 0.0025
    assert ens.grid_policy["realignments"] == ref[0].grid_policy["realignments"]


# 7 ---------------------------------------------------------------------------------------------------------------
def test_ensemble_meets_the_acceptance_bar(cfgmod, geom, driver):
    prm = cfgmod.params_from_values(dp=0.025, DL=3.0, end_time=20.0, output_interval=1.0)
    parts = [geom.init_particles(prm)] + [geom.perturbed_particles(prm, 0.01, k) for k in (1, 2, 3)]
    res = driver.run_ensemble([prm] * 4, average_from=16.0, parts_list=parts)
    pooled = res.pooled
    L2s = [r.time_avg["L2"] for r in res.members]
    print("members' time-averaged L2 = " + ", ".join(f"{v:.5f}" for v in L2s)
          + f"; pooled L2 = {pooled['L2']:.5f} (mean {pooled['L2_mean']:.5f}, std {pooled['L2_std']:.5f})"
          + f"; u_mean_se / U_max: max {np.nanmax(pooled['u_mean_se']) / pooled['U_max']:.2e}, "
            f"median {np.nanmedian(pooled['u_mean_se']) / pooled['U_max']:.2e}; wall {res.wall_seconds:.1f} s")
    print("u_mean_se = " + np.array2string(pooled["u_mean_se"], precision=4, max_line_width=200))
    for r in res.members:
        ta = r.time_avg
        assert ta["n_samples"] > 1000 and ta["t_first"] >= 16.0 and ta["t_last"] == r.t
        assert ta["L2"] <= 0.01
    assert pooled["L2"] <= 0.01
