"""-m gpu: the density statistics of a batch (include/sphx.h section 2s) -- k_dens_stats_b samples every member in one launch per
step slot.  A member that was never realigned has a standalone context's sums byte for byte; one that fell out of step and was
realigned agrees with numpy within the bound of tests/dens_stats_cases.py; a member whose gate is closed is not touched; the
read takes a member index; driver.run_sweep gives the table its columns and driver.run_ensemble pools the members."""
import ctypes as C

import numpy as np
import pytest

import dens_stats_cases as dc
from helpers import batch_members, err_id

pytestmark = pytest.mark.gpu

# four members differing in mu, c_f, transport_coeff and seed; c_f differs, so they fall out of step when advanced to a time
VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=21.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=11.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]
SETTING = dict(n_bins=20, hist_range=0.25)


def _members(cfgmod, geom):
    return batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)


def _batch_sums(b, n_bands=3):
    per_band = [b.dens_stats_sums(k) for k in range(n_bands)]      # [band][member]
    return [[per_band[k][m] for k in range(n_bands)] for m in range(b.n_members)]


def _ctx_sums(ctx, n_bands=3):
    return [ctx.dens_stats_sums(k) for k in range(n_bands)]


# 1 ---------------------------------------------------------------------------------------------------------------
def test_members_equal_standalone_contexts_to_the_byte(cfgmod, geom, capi, profmod):
    """Every member takes the same number of steps (no realignment): its slots are a standalone context's, and so is every bit."""
    members = _members(cfgmod, geom)
    xbands = dc.bands(members[0][0])
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
    n = 2 * K + 3  # crosses re-binnings
    with capi.Context.from_parts(*members[0], **kw) as ctx:
        t_mid = ctx.advance(1e9, max_steps=n // 2)["t"]
    cfg = dict(every=3, t_from=t_mid, bands=xbands, **SETTING)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.dens_stats_enable(**cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            refs.append(_ctx_sums(ctx))
    assert all(0 < r[0]["n_samples"] < n // 3 + 1 for r in refs)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.dens_stats_enable(**cfg)
        sts = b.advance(1e9, max_steps=n)
        got = _batch_sums(b)
        prof = b.dens_stats(1)
        assert b.info()["realignments"] == 0
        b.dens_stats_sample()                          # the state now: what download() returns, every member
        again = _batch_sums(b)
        states = [b.download(m, fields=("pos",))["pos"] for m in range(4)]
        b.dens_stats_reset()
        for mem in _batch_sums(b):
            for s in mem:
                assert s["n_samples"] == 0 and not np.any(s["count"]) and not np.any(s["sum_d"]) and not np.any(s["hist"])
                assert np.all(s["d_min"] == np.inf) and np.all(s["d_max"] == -np.inf)
    for m in range(4):
        prm, parts = members[m]
        assert sts[m]["step"] == n
        dc.assert_identical(got[m], refs[m], f"member {m}")
        # one more sample, of the state now: the sums so far plus numpy's sample of the download
        dens = dc.density(profmod, prm, parts, states[m])
        near = int(dc.near_edges(dens[0] / prm.rho0 - 1.0, 64, 0.25, 0.5).sum())
        assert near <= 2, near
        one = dc.numpy_sums(profmod, prm, parts, states[m], 20, xbands, dens, hist_range=0.25)
        sc = profmod.dens_scales(0.5, parts["n_fluid"])
        dc.assert_sums_match(again[m], dc.add_sums(profmod, refs[m], one), dc.quantisation(one, sc), f"member {m}: one more sample of the state now",
                             loose=near)
        assert again[m][0]["n_samples"] == refs[m][0]["n_samples"] + 1 and again[m][0]["t_last"] == sts[m]["t"]
        want = profmod.dens_stats_profiles(prm.DH, prm.p0, refs[m][1])
        assert np.array_equal(prof[m]["p_mean"], want["p_mean"], equal_nan=True) and np.array_equal(prof[m]["count"], refs[m][1]["count"])
    assert len({g[0]["sum_d"].tobytes() for g in got}) == 4   # the members really differ


# 2 ---------------------------------------------------------------------------------------------------------------
def test_members_out_of_step_are_sampled_on_their_own_clocks(cfgmod, geom, capi, profmod):
    """The members' dt differ (c_f): advanced to a time in two calls they take different step counts, the fast ones stop early
    and sit out the slots that remain (their gate is closed: nothing of theirs is touched), and the second call realigns, after
    which a member's layout differs from a standalone context's.  Each is sampled once per step it takes.  Compared with numpy:
    the sums of a standalone context stepped one step at a time to the same two targets, with a download after every step; the
    batch member's trajectory is that context's (test_gpu_batch.py), its sums numpy's within the bound."""
    members = _members(cfgmod, geom)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    t1, t2 = 6.3 * dt0, 13.9 * dt0
    xbands = dc.bands(members[0][0])
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.dens_stats_enable(every=1, bands=xbands, **SETTING)
        b.advance(t1)
        sts = b.advance(t2)
        got = _batch_sums(b)
        realigned = b.info()["realignments"]
    steps = [s["step"] for s in sts]
    assert len(set(steps)) > 1 and realigned >= 1, (steps, realigned)
    for m, (prm, parts) in enumerate(members):
        sc = profmod.dens_scales(0.5, parts["n_fluid"])
        total = quant = None
        loose = 0
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            targets = [t1, t2]     # the batch's two calls: the last step before each target is clipped to it
            for _ in range(steps[m]):
                st = ctx.advance(targets[0], max_steps=1)
                if st["t"] >= targets[0] and len(targets) > 1:
                    targets.pop(0)
                pos = ctx.download(fields=("pos",))["pos"]
                dens = dc.density(profmod, prm, parts, pos)
                near = int(dc.near_edges(dens[0] / prm.rho0 - 1.0, 64, 0.25, 0.5).sum())
                assert near <= 2, near
                loose += near
                one = dc.numpy_sums(profmod, prm, parts, pos, 20, xbands, dens, hist_range=0.25)
                q = dc.quantisation(one, sc)
                total = one if total is None else dc.add_sums(profmod, total, one)
                quant = q if quant is None else dc.add_quantisation(quant, q)
        # the same steps to the same target (a realigned member sums its forces in another order: the last bits of t may differ)
        assert st["step"] == steps[m] and abs(st["t"] - sts[m]["t"]) <= 1e-12 * t2, (m, st, sts[m])
        for band in got[m]:
            assert band["n_samples"] == steps[m] and band["t_last"] == sts[m]["t"], (m, band["n_samples"], sts[m])
        dc.assert_sums_match(got[m], total, quant, f"member {m} ({steps[m]} steps)", loose=loose)


def test_a_member_that_stops_early_equals_a_standalone_context(cfgmod, geom, capi):
    """One advance to a target: the members take their own numbers of steps with no realignment in between, so each member's
    slots -- and its sums, to the byte -- are those of a context advanced to the same target.  A member that has stopped sits
    out the slots that remain: its gate is closed and it is not sampled in them."""
    members = _members(cfgmod, geom)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    target = 9.4 * dt0
    cfg = dict(every=2, bands=dc.bands(members[0][0]), **SETTING)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    refs, steps = [], []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.dens_stats_enable(**cfg)
            steps.append(ctx.advance(target)["step"])
            refs.append(_ctx_sums(ctx))
    assert len(set(steps)) > 1, steps
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.dens_stats_enable(**cfg)
        sts = b.advance(target)
        got = _batch_sums(b)
    assert [s["step"] for s in sts] == steps
    for m in range(4):
        dc.assert_identical(got[m], refs[m], f"member {m} ({steps[m]} steps)")
        assert got[m][0]["n_samples"] == steps[m] // 2


def test_several_workgroups_per_member(cfgmod, geom, capi):
    """30 k fluid particles a member: 469 workgroups per grid row of k_dens_stats_b, each member its own blocks of sums and keys
    and its own ticket"""
    members = batch_members(cfgmod, geom, 0.01, 3.0, VARIANTS[:2])
    cfg = dict(every=2, bands=dc.bands(members[0][0]), **SETTING)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.dens_stats_enable(**cfg)
            ctx.advance(1e9, max_steps=6)
            refs.append(_ctx_sums(ctx))
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.dens_stats_enable(**cfg)
        b.advance(1e9, max_steps=6)
        got = _batch_sums(b)
    for m in range(2):
        dc.assert_identical(got[m], refs[m], f"member {m}")
        assert got[m][0]["n_samples"] == 3 and 0 < got[m][0]["count"].sum() <= 3 * members[m][1]["n_fluid"]
    assert not np.array_equal(got[0][0]["sum_d"], got[1][0]["sum_d"])


# 3 ---------------------------------------------------------------------------------------------------------------
def test_batch_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = _members(cfgmod, geom)[:3]
    M = 3
    ok = capi.SphxDensStatsConfig(n_bins=16, every=1, n_hist=64, hist_range=0.05, delta_bound=0.5)
    nothing = (None,) * 9
    for fn, args in ((L.sphx_batch_dens_stats_enable, (C.byref(ok),)), (L.sphx_batch_dens_stats_disable, ()), (L.sphx_batch_dens_stats_reset, ()),
                     (L.sphx_batch_dens_stats_sample, ()), (L.sphx_batch_dens_stats_read, (0, 0, 0, 0, *nothing))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        for fn, args in ((L.sphx_batch_dens_stats_read, (0, 0, 0, 0, *nothing)), (L.sphx_batch_dens_stats_sample, ()),
                         (L.sphx_batch_dens_stats_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:DensStats:disabled", capi.SPHX_ERR_STATE)
        with pytest.raises(capi.SphxError) as e:
            b.dens_stats_sums()
        assert e.value.identifier == "SPHX:DensStats:disabled" and "batch" in e.value.message
        assert L.sphx_batch_dens_stats_disable(h) == capi.SPHX_OK       # no-op when off
        b.dens_stats_enable(n_bins=16)
        b.advance(1e9, max_steps=5)
        for bad in (dict(every=0), dict(n_bins=-1), dict(n_bins=952), dict(n_hist=0), dict(hist_range=0.6), dict(delta_bound=0.7), dict(n_bands=3)):
            c2 = capi.SphxDensStatsConfig(**dict(dict(n_bins=16, every=1, n_hist=64, hist_range=0.05, delta_bound=0.5), **bad))
            assert err_id(capi, L.sphx_batch_dens_stats_enable, h, C.byref(c2)) == ("SPHX:DensStats:config", capi.SPHX_ERR_ARG), bad
        for m in range(M):
            ns = C.c_int64(-1)
            assert L.sphx_batch_dens_stats_read(h, m, 0, 0, 0, *(None,) * 6, C.byref(ns), None, None) == capi.SPHX_OK
            assert ns.value == 5                                        # the refused enables left the sampler running
        for m in (-1, M):
            assert err_id(capi, L.sphx_batch_dens_stats_read, h, m, 0, 0, 0, *nothing) == ("SPHX:Batch:member", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_batch_dens_stats_read, h, 0, 1, 0, 0, *nothing) == ("SPHX:DensStats:band", capi.SPHX_ERR_ARG)
        sums = np.full((8, 20), -7.0)
        assert err_id(capi, L.sphx_batch_dens_stats_read, h, 0, 0, 15, 0, None, None, capi.ptr(sums), *(None,) * 6) == \
            ("SPHX:DensStats:capacity", capi.SPHX_ERR_ARG)
        assert np.all(sums == -7.0)
        want = b.dens_stats_sums(0)
        for m in range(M):
            assert L.sphx_batch_dens_stats_read(h, m, 0, 20, 0, None, None, capi.ptr(sums), *(None,) * 6) == capi.SPHX_OK  # [field][capacity]
            for j, f in enumerate(dc.FIELDS):
                assert np.array_equal(sums[j, :16], want[m][f]) and np.all(sums[j, 16:] == -7.0), (m, f)
            assert want[m]["count"].sum() > 0


# 4 ---------------------------------------------------------------------------------------------------------------
def test_run_sweep_adds_the_density_columns(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, mu=mu, end_time=0.1, output_interval=0.05) for mu in (0.08, 0.1, 0.15)]
    res = driver.run_sweep(prms, history_capacity=1024, density_from=0.0, density_every=2)
    for k in ("delta_rms", "delta_max", "p_spread"):
        assert res.table[k].shape == (3,) and np.all(np.isfinite(res.table[k])), k
    for m, r in enumerate(res.members):
        ds = r.dens_stats
        assert len(ds) == 2 and ds[0]["n_samples"] == r.steps // 2 and len(ds[0]["count"]) == 20
        fig = driver.density_figures(prms[m], ds)
        assert res.table["delta_rms"][m] == fig["delta_rms"] and res.table["p_spread"][m] == fig["p_spread"]
    plain = driver.run_sweep(prms, history_capacity=1024)
    assert not {"delta_rms", "delta_max", "p_spread"} & set(plain.table) and all(r.dens_stats is None for r in plain.members)


def test_run_ensemble_pools_the_members(cfgmod, geom, driver, profmod):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.1, output_interval=0.05) for _ in range(3)]
    parts_list = [geom.perturbed_particles(p, 0.1, 40 + m) for m, p in enumerate(prms)]
    res = driver.run_ensemble(prms, average_from=0.05, parts_list=parts_list, density_from=0.05, density_every=3)
    pooled = res.pooled_density
    assert len(pooled) == 2 and all(r.dens_stats is not None for r in res.members)
    for b in range(2):
        mine = [r.dens_stats[b] for r in res.members]
        want = profmod.pool_dens_stats(prms[0].DH, prms[0].p0, mine)
        for f in dc.COUNTS + dc.SUMMED:
            assert np.array_equal(pooled[b][f], mine[0][f] + mine[1][f] + mine[2][f]), (b, f)
        assert np.array_equal(pooled[b]["d_min"], np.minimum(np.minimum(mine[0]["d_min"], mine[1]["d_min"]), mine[2]["d_min"]))
        assert np.array_equal(pooled[b]["hist"], mine[0]["hist"] + mine[1]["hist"] + mine[2]["hist"])
        assert pooled[b]["n_samples"] == sum(s["n_samples"] for s in mine) and pooled[b]["n_members"] == 3
        assert np.array_equal(pooled[b]["d_mean"], want["d_mean"], equal_nan=True) and np.array_equal(pooled[b]["hist_density"], want["hist_density"])
    assert len({r.dens_stats[0]["sum_d"].tobytes() for r in res.members}) == 3
    assert driver.run_ensemble(prms, average_from=0.05, parts_list=parts_list).pooled_density is None
