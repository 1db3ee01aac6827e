"""-m gpu: the pair statistics of a batch (include/sphx.h section 2m) -- k_pair_dist_b counts every member's pairs in one
launch per step slot.  Integer sums: a member's equal a standalone context's count for count, members that fall out of step are
sampled on their own clocks, a member that stops early keeps its sums; driver.run_sweep gives the table its columns and
driver.run_ensemble pools the members."""
import ctypes as C

import numpy as np
import pytest

import pair_dist_cases as pc
from helpers import batch_members, err_id

pytestmark = pytest.mark.gpu

VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=21.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=11.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]
SETTING = dict(n_bins=64, with_walls=True)


def _members(cfgmod, geom):
    return batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)


# 1 ---------------------------------------------------------------------------------------------------------------
def test_members_equal_standalone_contexts(cfgmod, geom, capi, profmod):
    """Every member takes the same number of steps (no realignment): its state, and so every count, is a standalone context's."""
    members = _members(cfgmod, geom)
    xbands = pc.bands(members[0][0])
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
    n = 2 * K + 3  # crosses re-binnings
    with capi.Context.from_parts(*members[0], **kw) as ctx:
        t_mid = ctx.advance(1e9, max_steps=n // 2)["t"]
    cfg = dict(every=3, t_from=t_mid, bands=xbands, y_margin=members[0][0].h, **SETTING)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.pair_dist_enable(**cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            refs.append(ctx.pair_dist_sums())
    assert all(0 < r[0]["n_samples"] < n // 3 + 1 for r in refs)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.pair_dist_enable(**cfg)
        sts = b.advance(1e9, max_steps=n)
        got = b.pair_dist_sums()
        one = b.pair_dist(1)
        assert b.info()["realignments"] == 0
        b.pair_dist_sample()                          # the state now: what download() returns, every member
        again = b.pair_dist_sums()
        states = [b.download(m, fields=("pos",))["pos"] for m in range(4)]
        b.pair_dist_reset()
        assert all(s["n_samples"] == 0 and s["ff"].sum() == 0 and s["r2_min"] == np.inf for mem in b.pair_dist_sums() for s in mem)
    assert len(got) == 4 and all(len(g) == 3 for g in got)
    for m in range(4):
        assert sts[m]["step"] == n
        pc.assert_counts_equal(got[m], refs[m], f"member {m}", head=True)
        assert np.array_equal(one[m]["ff"], refs[m][1]["ff"]) and one[m]["n_neigh"] == refs[m][1]["ff"].sum() / refs[m][1]["centres"]
        prm, parts = members[m]
        now = pc.numpy_sums(profmod, prm, parts, states[m], 64, 2.0 * prm.h, prm.h, True, xbands)
        pc.assert_counts_equal(again[m], pc.add_counts(refs[m], now), f"member {m}: one more sample of the state now")
        assert again[m][0]["n_samples"] == refs[m][0]["n_samples"] + 1 and again[m][0]["t_last"] == sts[m]["t"]
    assert len({g[0]["ff"].tobytes() for g in got}) == 4   # the members really differ


# 2 ---------------------------------------------------------------------------------------------------------------
def test_members_are_sampled_on_their_own_clocks(cfgmod, geom, capi):
    """The members' dt differ (c_f): they reach the target in different step counts, the fast ones stop early and sit out the
    slots that remain.  Each is sampled once per step it takes, the last time at the time it stopped."""
    members = _members(cfgmod, geom)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
        b.pair_dist_enable(every=1, bands=pc.bands(members[0][0]), **SETTING)
        b.advance(6.3 * dt0)
        sts = b.advance(13.9 * dt0)
        got = b.pair_dist_sums()
    steps = [s["step"] for s in sts]
    assert len(set(steps)) > 1 and min(steps) < max(steps), steps
    for m, s in enumerate(sts):
        for band in got[m]:
            assert band["n_samples"] == s["step"] and band["t_last"] == s["t"], (m, band["n_samples"], s)
        assert 0 < got[m][0]["centres"] <= s["step"] * members[m][1]["n_fluid"]   # (a particle outside [0, DH] is no centre)


def test_a_member_that_stops_early_equals_a_standalone_context(cfgmod, geom, capi):
    """One advance to a target: the members take their own numbers of steps with no realignment in between, so each member's
    state -- and its sums -- are those of a context advanced to the same target."""
    members = _members(cfgmod, geom)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    target = 9.4 * dt0
    cfg = dict(every=2, bands=pc.bands(members[0][0]), **SETTING)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    refs, steps = [], []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.pair_dist_enable(**cfg)
            steps.append(ctx.advance(target)["step"])
            refs.append(ctx.pair_dist_sums())
    assert len(set(steps)) > 1, steps
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.pair_dist_enable(**cfg)
        sts = b.advance(target)
        got = b.pair_dist_sums()
    assert [s["step"] for s in sts] == steps
    for m in range(4):
        pc.assert_counts_equal(got[m], refs[m], f"member {m} ({steps[m]} steps)", head=True)
        assert got[m][0]["n_samples"] == steps[m] // 2


def test_several_workgroups_per_member(cfgmod, geom, capi):
    """30 k fluid particles a member: 938 workgroups per grid row of k_pair_dist_b, each member its own block of sums"""
    members = batch_members(cfgmod, geom, 0.01, 3.0, VARIANTS[:2])
    cfg = dict(every=2, bands=pc.bands(members[0][0]), **SETTING)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.pair_dist_enable(**cfg)
            ctx.advance(1e9, max_steps=6)
            refs.append(ctx.pair_dist_sums())
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.pair_dist_enable(**cfg)
        b.advance(1e9, max_steps=6)
        got = b.pair_dist_sums()
    for m in range(2):
        pc.assert_counts_equal(got[m], refs[m], f"member {m}", head=True)
        assert got[m][0]["n_samples"] == 3 and 0 < got[m][0]["centres"] <= 3 * members[m][1]["n_fluid"]
    assert not np.array_equal(got[0][0]["ff"], got[1][0]["ff"])


# 3 ---------------------------------------------------------------------------------------------------------------
def test_batch_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = _members(cfgmod, geom)[:3]
    M = 3
    ok = capi.SphxPairDistConfig(n_bins=16, every=1)
    nothing = (None,) * 8
    for fn, args in ((L.sphx_batch_pair_dist_enable, (C.byref(ok),)), (L.sphx_batch_pair_dist_disable, ()), (L.sphx_batch_pair_dist_reset, ()),
                     (L.sphx_batch_pair_dist_sample, ()), (L.sphx_batch_pair_dist_read, (0, 0, *nothing))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        for fn, args in ((L.sphx_batch_pair_dist_read, (0, 0, *nothing)), (L.sphx_batch_pair_dist_sample, ()), (L.sphx_batch_pair_dist_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:PairDist:disabled", capi.SPHX_ERR_STATE)
        with pytest.raises(capi.SphxError) as e:
            b.pair_dist_sums()
        assert e.value.identifier == "SPHX:PairDist:disabled" and "batch" in e.value.message
        assert L.sphx_batch_pair_dist_disable(h) == capi.SPHX_OK       # no-op when off
        b.pair_dist_enable(n_bins=16)
        b.advance(1e9, max_steps=5)
        for bad in (dict(every=0), dict(n_bins=0), dict(n_bins=1025), dict(r_max=1.0), dict(n_bands=3)):
            c2 = capi.SphxPairDistConfig(**dict(dict(n_bins=16, every=1), **bad))
            assert err_id(capi, L.sphx_batch_pair_dist_enable, h, C.byref(c2)) == ("SPHX:PairDist:config", capi.SPHX_ERR_ARG), bad
        ns = np.full(M, -1, dtype=np.int64)
        assert L.sphx_batch_pair_dist_read(h, 0, 0, None, None, None, None, None, i64(ns), None, None) == capi.SPHX_OK
        assert list(ns) == [5] * M                                      # the refused enables left the sampler running
        assert err_id(capi, L.sphx_batch_pair_dist_read, h, 1, 0, *nothing) == ("SPHX:PairDist:band", capi.SPHX_ERR_ARG)
        ff = np.full((M, 20), -7, dtype=np.int64)
        assert err_id(capi, L.sphx_batch_pair_dist_read, h, 0, 15, None, i64(ff), *nothing[2:]) == ("SPHX:PairDist:capacity", capi.SPHX_ERR_ARG)
        assert np.all(ff == -7)
        cen = np.zeros(M, dtype=np.int64)
        assert L.sphx_batch_pair_dist_read(h, 0, 20, None, i64(ff), None, i64(cen), *nothing[4:]) == capi.SPHX_OK  # member m's bins at m * capacity
        want = b.pair_dist_sums()
        for m in range(M):
            assert np.array_equal(ff[m, :16], want[m][0]["ff"]) and np.all(ff[m, 16:] == -7) and cen[m] == want[m][0]["centres"] > 0


# 4 ---------------------------------------------------------------------------------------------------------------
def test_run_sweep_adds_the_pair_columns(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, transport_coeff=tc, end_time=0.1, output_interval=0.05) for tc in (0.0, 0.15, 0.3)]
    res = driver.run_sweep(prms, history_capacity=1024, pairs_from=0.0, pairs_every=2, pairs_walls=True)
    for k in ("r_min_dp", "n_neigh", "sigma1_dp"):
        assert res.table[k].shape == (3,) and np.all(np.isfinite(res.table[k])), k
    for m, r in enumerate(res.members):
        pd = r.pair_dist
        assert len(pd) == 3 and pd[0]["n_samples"] == r.steps // 2 and pd[0]["ff"].dtype == np.int64
        fig = driver.pair_dist_figures(prms[m], pd)
        for k in ("r_min_dp", "n_neigh", "sigma1_dp"):
            assert res.table[k][m] == fig[k], (m, k)
        if res.grid_policy["realignments"] == 0:  # (a realignment changes the summation order of the steps behind it: the state
            alone = driver.run(prms[m], pairs_from=0.0, pairs_every=2, pairs_walls=True).pair_dist   # agrees to rounding only)
            pc.assert_counts_equal(pd, alone, f"member {m} against driver.run", head=True)
    plain = driver.run_sweep(prms, history_capacity=1024)
    assert not {"r_min_dp", "n_neigh", "sigma1_dp"} & set(plain.table) and all(r.pair_dist is None for r in plain.members)


def test_run_ensemble_pools_the_members(cfgmod, geom, driver, profmod):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.1, output_interval=0.05) for _ in range(3)]
    parts_list = [geom.perturbed_particles(p, 0.1, 40 + m) for m, p in enumerate(prms)]
    res = driver.run_ensemble(prms, average_from=0.05, parts_list=parts_list, pairs_from=0.05, pairs_every=3)
    pooled = res.pooled_pairs
    assert len(pooled) == 3 and all(r.pair_dist is not None for r in res.members)
    for b in range(3):
        mine = [r.pair_dist[b] for r in res.members]
        assert np.array_equal(pooled[b]["ff"], sum(s["ff"] for s in mine)) and pooled[b]["ff"].dtype == np.int64
        assert pooled[b]["centres"] == sum(s["centres"] for s in mine) and pooled[b]["n_samples"] == sum(s["n_samples"] for s in mine)
        assert pooled[b]["r2_min"] == min(s["r2_min"] for s in mine)
        assert np.array_equal(pooled[b]["g"], profmod.pair_dist_profiles(pooled[b], prms[0].dp)["g"], equal_nan=True)
    assert len({r.pair_dist[0]["ff"].tobytes() for r in res.members}) == 3
    assert driver.run_ensemble(prms, average_from=0.05, parts_list=parts_list).pooled_pairs is None
