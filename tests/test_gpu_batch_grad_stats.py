"""-m gpu: the gradient statistics of a batch (include/sphx.h section 2o) -- k_grad_stats_b samples every member in one launch
per step slot.  A member that was never realigned has a standalone context's sums byte for byte; one that fell out of step and
was realigned agrees within the bound of tests/grad_stats_cases.py, its counts exactly; a member whose gate is closed is not
touched; driver.run_sweep gives the table its columns and driver.run_ensemble pools the members."""
import ctypes as C

import numpy as np
import pytest

import grad_stats_cases as gc
from helpers import batch_members, err_id

pytestmark = pytest.mark.gpu

# four members differing in mu; c_f differs too, so they fall out of step when advanced to a time
VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=21.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=11.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]
SETTING = dict(n_bins=20, with_walls=True)


def _members(cfgmod, geom):
    return batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)


def _batch_sums(b, n_bands=3):
    per_band = [b.grad_stats_sums(k) for k in range(n_bands)]      # [band][member]
    return [[per_band[k][m] for k in range(n_bands)] for m in range(b.n_members)]


def _ctx_sums(ctx, n_bands=3):
    return [ctx.grad_stats_sums(k) for k in range(n_bands)]


# 1 ---------------------------------------------------------------------------------------------------------------
def test_members_equal_standalone_contexts_to_the_byte(cfgmod, geom, capi, profmod):
    """Every member takes the same number of steps (no realignment): its slots are a standalone context's, and so is every bit."""
    members = _members(cfgmod, geom)
    xbands = gc.bands(members[0][0])
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
    n = 2 * K + 3  # crosses re-binnings
    with capi.Context.from_parts(*members[0], **kw) as ctx:
        t_mid = ctx.advance(1e9, max_steps=n // 2)["t"]
    cfg = dict(every=3, t_from=t_mid, bands=xbands, **SETTING)
    refs, again_refs = [], []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.grad_stats_enable(**cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            refs.append(_ctx_sums(ctx))
            ctx.grad_stats_sample()
            again_refs.append(_ctx_sums(ctx))
    assert all(0 < r[0]["n_samples"] < n // 3 + 1 for r in refs)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.grad_stats_enable(**cfg)
        sts = b.advance(1e9, max_steps=n)
        got = _batch_sums(b)
        prof = b.grad_stats(1)
        assert b.info()["realignments"] == 0
        b.grad_stats_sample()                          # the state now: what download() returns, every member
        again = _batch_sums(b)
        b.grad_stats_reset()
        assert all(s["n_samples"] == 0 and not np.any(s["count"]) and not np.any(s["sum_gxy"]) for mem in _batch_sums(b) for s in mem)
    for m in range(4):
        assert sts[m]["step"] == n
        gc.assert_identical(got[m], refs[m], f"member {m}")
        # (the sample of the state now may see another layout than the context's: both on the fixed-point grid, within the bound)
        sc = profmod.grad_scales(sts[m]["vmax"], members[m][0].h, members[m][1]["n_fluid"])
        quant = [{f: 2.0 * q[f] for f in gc.SUMMED} for q in gc.quantisation(again_refs[m], sc)]
        gc.assert_sums_match(again[m], again_refs[m], quant, f"member {m}: one more sample of the state now")
        assert again[m][0]["n_samples"] == refs[m][0]["n_samples"] + 1 and again[m][0]["t_last"] == sts[m]["t"]
        want = profmod.grad_stats_profiles(members[m][0].DH, refs[m][1])
        assert np.array_equal(prof[m]["gxy_mean"], want["gxy_mean"], equal_nan=True) and np.array_equal(prof[m]["count"], refs[m][1]["count"])
    assert len({g[0]["sum_gxy"].tobytes() for g in got}) == 4   # the members really differ


# 2 ---------------------------------------------------------------------------------------------------------------
def test_members_out_of_step_are_sampled_on_their_own_clocks(cfgmod, geom, capi, profmod):
    """The members' dt differ (c_f): advanced to a time in two calls they take different step counts, the fast ones stop early
    and sit out the slots that remain (their gate is closed: nothing of theirs is touched), and the second call realigns.  Each
    is sampled once per step it takes.  Against a standalone context advanced to the same targets: the counts exactly; the sums
    within the bound, because a realignment reorders a member's slots and with them the order its partners are added in.  Both
    sides are on the fixed-point grid, so the quantisation term counts twice; its scale is the coarsest of the run (the
    largest max |v| the step history recorded)."""
    members = _members(cfgmod, geom)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    t1, t2 = 6.3 * dt0, 13.9 * dt0
    xbands = gc.bands(members[0][0])
    kw = dict(t_end=1e9, lanes_per_particle=16)
    refs, steps, vmax = [], [], []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.grad_stats_enable(every=1, bands=xbands, **SETTING)
            ctx.history_enable(every=1, capacity=256)
            ctx.advance(t1)
            steps.append(ctx.advance(t2)["step"])
            refs.append(_ctx_sums(ctx))
            vmax.append(float(np.max(ctx.history()["vmax"])))
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.grad_stats_enable(every=1, bands=xbands, **SETTING)
        b.advance(t1)
        sts = b.advance(t2)
        got = _batch_sums(b)
        realigned = b.info()["realignments"]
    assert len(set(steps)) > 1 and [s["step"] for s in sts] == steps and realigned >= 1, (steps, realigned)
    for m, s in enumerate(sts):
        prm, parts = members[m]
        for band in got[m]:
            assert band["n_samples"] == s["step"] and band["t_last"] == s["t"], (m, band["n_samples"], s)
        sc = profmod.grad_scales(vmax[m], prm.h, parts["n_fluid"])
        quant = [{f: 2.0 * q[f] for f in gc.SUMMED} for q in gc.quantisation(refs[m], sc)]
        gc.assert_sums_match(got[m], refs[m], quant, f"member {m} ({steps[m]} steps)")


def test_a_member_that_stops_early_equals_a_standalone_context(cfgmod, geom, capi):
    """One advance to a target: the members take their own numbers of steps with no realignment in between, so each member's
    slots -- and its sums, to the byte -- are those of a context advanced to the same target."""
    members = _members(cfgmod, geom)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    target = 9.4 * dt0
    cfg = dict(every=2, bands=gc.bands(members[0][0]), **SETTING)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    refs, steps = [], []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.grad_stats_enable(**cfg)
            steps.append(ctx.advance(target)["step"])
            refs.append(_ctx_sums(ctx))
    assert len(set(steps)) > 1, steps
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.grad_stats_enable(**cfg)
        sts = b.advance(target)
        got = _batch_sums(b)
    assert [s["step"] for s in sts] == steps
    for m in range(4):
        gc.assert_identical(got[m], refs[m], f"member {m} ({steps[m]} steps)")
        assert got[m][0]["n_samples"] == steps[m] // 2


def test_several_workgroups_per_member(cfgmod, geom, capi):
    """30 k fluid particles a member: 469 workgroups per grid row of k_grad_stats_b, each member its own block of sums and its
    own ticket"""
    members = batch_members(cfgmod, geom, 0.01, 3.0, VARIANTS[:2])
    cfg = dict(every=2, bands=gc.bands(members[0][0]), **SETTING)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.grad_stats_enable(**cfg)
            ctx.advance(1e9, max_steps=6)
            refs.append(_ctx_sums(ctx))
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.grad_stats_enable(**cfg)
        b.advance(1e9, max_steps=6)
        got = _batch_sums(b)
    for m in range(2):
        gc.assert_identical(got[m], refs[m], f"member {m}")
        assert got[m][0]["n_samples"] == 3 and 0 < got[m][0]["count"].sum() <= 3 * members[m][1]["n_fluid"]
    assert not np.array_equal(got[0][0]["sum_gxy"], got[1][0]["sum_gxy"])


# 3 ---------------------------------------------------------------------------------------------------------------
def test_batch_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = _members(cfgmod, geom)[:3]
    M = 3
    ok = capi.SphxGradStatsConfig(n_bins=16, every=1, det_min=0.05)
    nothing = (None,) * 5
    for fn, args in ((L.sphx_batch_grad_stats_enable, (C.byref(ok),)), (L.sphx_batch_grad_stats_disable, ()), (L.sphx_batch_grad_stats_reset, ()),
                     (L.sphx_batch_grad_stats_sample, ()), (L.sphx_batch_grad_stats_read, (0, 0, *nothing))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        for fn, args in ((L.sphx_batch_grad_stats_read, (0, 0, *nothing)), (L.sphx_batch_grad_stats_sample, ()), (L.sphx_batch_grad_stats_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:GradStats:disabled", capi.SPHX_ERR_STATE)
        with pytest.raises(capi.SphxError) as e:
            b.grad_stats_sums()
        assert e.value.identifier == "SPHX:GradStats:disabled" and "batch" in e.value.message
        assert L.sphx_batch_grad_stats_disable(h) == capi.SPHX_OK       # no-op when off
        b.grad_stats_enable(n_bins=16)
        b.advance(1e9, max_steps=5)
        for bad in (dict(every=0), dict(n_bins=-1), dict(n_bins=641), dict(det_min=-1.0), dict(n_bands=3)):
            c2 = capi.SphxGradStatsConfig(**dict(dict(n_bins=16, every=1, det_min=0.05), **bad))
            assert err_id(capi, L.sphx_batch_grad_stats_enable, h, C.byref(c2)) == ("SPHX:GradStats:config", capi.SPHX_ERR_ARG), bad
        ns = np.full(M, -1, dtype=np.int64)
        assert L.sphx_batch_grad_stats_read(h, 0, 0, None, None, i64(ns), None, None) == capi.SPHX_OK
        assert list(ns) == [5] * M                                      # the refused enables left the sampler running
        assert err_id(capi, L.sphx_batch_grad_stats_read, h, 1, 0, *nothing) == ("SPHX:GradStats:band", capi.SPHX_ERR_ARG)
        sums = np.full((M, 12, 20), -7.0)
        assert err_id(capi, L.sphx_batch_grad_stats_read, h, 0, 15, None, capi.ptr(sums), None, None, None) == ("SPHX:GradStats:capacity", capi.SPHX_ERR_ARG)
        assert np.all(sums == -7.0)
        assert L.sphx_batch_grad_stats_read(h, 0, 20, None, capi.ptr(sums), None, None, None) == capi.SPHX_OK  # [member][field][capacity]
        want = b.grad_stats_sums(0)
        for m in range(M):
            for j, f in enumerate(gc.FIELDS):
                assert np.array_equal(sums[m, j, :16], want[m][f]) and np.all(sums[m, j, 16:] == -7.0), (m, f)
            assert want[m]["count"].sum() > 0


# 4 ---------------------------------------------------------------------------------------------------------------
def test_run_sweep_adds_the_gradient_columns(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, mu=mu, end_time=0.1, output_interval=0.05) for mu in (0.08, 0.1, 0.15)]
    res = driver.run_sweep(prms, history_capacity=1024, gradients_from=0.0, gradients_every=2)
    for k in ("L2_shear", "tau_wall_dev", "div_rms"):
        assert res.table[k].shape == (3,) and np.all(np.isfinite(res.table[k])), k
    for m, r in enumerate(res.members):
        gs = r.grad_stats
        assert len(gs) == 2 and gs[0]["n_samples"] == r.steps // 2 and len(gs[0]["count"]) == 20
        fig = driver.grad_figures(prms[m], gs)
        assert res.table["L2_shear"][m] == fig["L2_shear"] and res.table["div_rms"][m] == fig["div_rms"]
    plain = driver.run_sweep(prms, history_capacity=1024)
    assert not {"L2_shear", "tau_wall_dev", "div_rms"} & set(plain.table) and all(r.grad_stats is None for r in plain.members)


def test_run_ensemble_pools_the_members(cfgmod, geom, driver, profmod):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.1, output_interval=0.05) for _ in range(3)]
    parts_list = [geom.perturbed_particles(p, 0.1, 40 + m) for m, p in enumerate(prms)]
    res = driver.run_ensemble(prms, average_from=0.05, parts_list=parts_list, gradients_from=0.05, gradients_every=3)
    pooled = res.pooled_grad
    assert len(pooled) == 2 and all(r.grad_stats is not None for r in res.members)
    for b in range(2):
        mine = [r.grad_stats[b] for r in res.members]
        for f in gc.FIELDS:
            assert np.array_equal(pooled[b][f], mine[0][f] + mine[1][f] + mine[2][f]), (b, f)
        assert pooled[b]["n_samples"] == sum(s["n_samples"] for s in mine) and pooled[b]["n_members"] == 3
        assert np.array_equal(pooled[b]["gxy_mean"], profmod.grad_stats_profiles(prms[0].DH, pooled[b])["gxy_mean"], equal_nan=True)
    assert len({r.grad_stats[0]["sum_gxy"].tobytes() for r in res.members}) == 3
    assert driver.run_ensemble(prms, average_from=0.05, parts_list=parts_list).pooled_grad is None
