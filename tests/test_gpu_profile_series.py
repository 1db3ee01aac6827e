"""-m gpu: the device-side profile series (include/sphx.h section 2j) -- the flow statistics' sample of every sampled step,
recorded by k_profile_series inside the step loop.  Checked against numpy binning of download() record by record, against the
flow statistics' running sums (to the bit: the records added in order ARE those sums), against sampling between steps from
the host, for its gate, its record buffer (capacity, drain, no stale contents), its limits and error identifiers, for
leaving the physics, the launches and the other four samplers untouched, for repeatability, through driver.run against the
output-point profiles, against the start-up solution of plane Poiseuille flow, and through the MATLAB context gateway."""
import ctypes as C

import numpy as np
import pytest

import mex_mock
import profile_series_cases as sc
from helpers import HISTORY_FIELDS, check_kernel_form, err_id, gateway_cfg, make_case, profiled_launches

pytestmark = pytest.mark.gpu


def _ctx(capi, cfgmod, geom, name, **more):
    prm, parts, kw = sc.case(make_case, cfgmod, geom, name)
    return prm, parts, capi.Context.from_parts(prm, parts, t_end=1e9, **dict(kw, **more))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_every_record_matches_numpy(cfgmod, geom, capi, profmod, name):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    nf = parts["n_fluid"]
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    bands = sc.bands(prm)
    states, status = [], []
    with ctx:
        check_kernel_form(ctx, name)
        ctx.profile_series_enable(every=1, capacity=16, bands=bands)
        for _ in range(7):
            ctx.advance(1e9, max_steps=1)
            states.append(ctx.download(fields=("pos", "vel")))
            status.append(ctx.sync())
        got = ctx.profile_series_sums()
        prof = ctx.profile_series()
    assert got["count"].shape == (7, 3, n_bins) and got["n_dropped"] == 0
    assert got["step"].tolist() == [s["step"] for s in status] == list(range(1, 8))
    assert got["t"].tolist() == [s["t"] for s in status]
    for r, d in enumerate(states):
        pos, vel = d["pos"][:nf], d["vel"][:nf]
        for b, band in enumerate([None] + bands):
            sc.assert_record_matches(got, r, b, sc.numpy_sums(pos, vel, prm, n_bins, band), f"{name} record {r} band {b}")
        _, u_mid = profmod.compute_mid_channel_profile(pos, vel[:, 0], prm.DL, prm.DH, bands[0][0], bands[0][1], n_bins)
        assert np.array_equal(np.isnan(prof["u_mean"][r, 1]), np.isnan(u_mid))
        ok = ~np.isnan(u_mid)
        np.testing.assert_allclose(prof["u_mean"][r, 1][ok], u_mid[ok], rtol=1e-12, atol=1e-14)
    assert got["count"][:, 0].sum(axis=1).tolist() == [float(np.sum((d["pos"][:nf, 1] >= 0) & (d["pos"][:nf, 1] <= prm.DH))) for d in states]
    if name == "leftward":
        assert prm.gravity_g < 0 and np.all(got["sum_ux"][:, 0, n_bins // 2] < 0)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("name", list(sc.CASES))
def test_records_add_up_to_the_flow_statistics_bit_for_bit(cfgmod, geom, capi, name, every):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    bands = sc.bands(prm)
    with ctx:
        t_from = 0.0
        ctx.flow_stats_enable(every=every, t_from=t_from, bands=bands)
        ctx.profile_series_enable(every=every, t_from=t_from, bands=bands, capacity=32)
        st = ctx.advance(1e9, max_steps=23)
        assert st["step"] == 23
        series = ctx.profile_series_sums()
        stats = [ctx.flow_stats_sums(b) for b in range(3)]
    n = 23 // every
    assert len(series["step"]) == n and series["n_dropped"] == 0
    for b in range(3):
        assert stats[b]["n_samples"] == n
        assert (stats[b]["t_first"], stats[b]["t_last"]) == (series["t"][0], series["t"][-1])
        total = sc.running_sums(series, b)
        for f in sc.FIELDS:
            assert np.array_equal(total[f], stats[b][f]), f"{name} every {every} band {b}: {f}"


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_in_loop_equals_sampling_between_single_steps(cfgmod, geom, capi, name):
    N = 20  # (past the static schedule's re-binning interval of 16)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    bands = sc.bands(prm)
    with ctx:
        ctx.profile_series_enable(every=1, bands=bands, capacity=32)
        st = ctx.advance(1e9, max_steps=N)
        rebins = ctx.schedule()["rebins"]
        in_loop = ctx.profile_series_sums()
    assert st["step"] == N and rebins >= 1, f"{name}: {rebins} re-binnings in {N} steps"
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    with ctx:
        ctx.profile_series_enable(every=10 ** 9, bands=bands, capacity=32)
        for _ in range(N):
            ctx.advance(1e9, max_steps=1)
            ctx.profile_series_sample()
        by_hand = ctx.profile_series_sums()
    assert len(in_loop["step"]) == N
    sc.assert_series_identical(in_loop, by_hand, name)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_gate(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.profile_series_enable(every=1, capacity=32)
        ctx.advance(1e9, max_steps=20)
        every_step = ctx.profile_series_sums()
    t = every_step["t"]
    t_from = 0.5 * (t[3] + t[4])  # between step 4 and step 5
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.profile_series_enable(every=3, t_from=t_from, capacity=32)
        ctx.advance(1e9, max_steps=20)
        gated = ctx.profile_series_sums()
        ctx.profile_series_enable(every=10 ** 9)
        ctx.advance(1e9, max_steps=5)
        assert len(ctx.profile_series_sums()["step"]) == 0
        ctx.profile_series_sample()
        one = ctx.profile_series_sums()
        st = ctx.sync()
    want = [s for s in range(1, 21) if s % 3 == 0 and t[s - 1] >= t_from]
    assert want == [6, 9, 12, 15, 18] and gated["step"].tolist() == want
    rows = [s - 1 for s in want]
    sc.assert_series_identical(gated, {k: every_step[k][rows] for k in sc.SERIES}, "gated", counters=False)
    assert one["step"].tolist() == [25] and one["t"].tolist() == [st["t"]] and one["n_dropped"] == 0


# 5 ---------------------------------------------------------------------------------------------------------------
def test_record_buffer_capacity_and_drain(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    bands = sc.bands(prm)
    with ctx:
        ctx.profile_series_enable(every=1, bands=bands, capacity=64)
        ctx.advance(1e9, max_steps=10)
        whole = ctx.profile_series_sums()
    assert len(whole["step"]) == 10
    for cap in (1, 2, 3):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
        with ctx:
            ctx.profile_series_enable(every=1, bands=bands, capacity=cap)
            ctx.advance(1e9, max_steps=7)
            full = ctx.profile_series_sums()
            again = ctx.profile_series_sums(drain=True)
            empty = ctx.profile_series_sums()
            ctx.advance(1e9, max_steps=3)
            resumed = ctx.profile_series_sums()
        assert full["step"].tolist() == list(range(1, cap + 1)) and full["n_dropped"] == 7 - cap
        sc.assert_series_identical(full, {k: whole[k][:cap] for k in sc.SERIES}, f"capacity {cap}", counters=False)
        sc.assert_series_identical(full, again, "read twice")
        assert len(empty["step"]) == 0 and empty["n_dropped"] == 0 and empty["count"].shape == (0, 3, whole["count"].shape[2])
        # after the drain the next records land at slot 0 and n_dropped restarts
        assert resumed["step"].tolist() == list(range(8, 8 + min(cap, 3))) and resumed["n_dropped"] == 3 - min(cap, 3)
        sc.assert_series_identical(resumed, {k: whole[k][7:7 + cap] for k in sc.SERIES}, f"capacity {cap} resumed", counters=False)


def test_stale_contents_never_show(cfgmod, geom, capi):
    """The record buffer is never cleared: a record is complete because every counter of it is stored, zeros included.  The old
    buffer goes back to the pool at disable and is filled with NaN words there, so whatever block the new buffer gets, a
    counter that was not written would show."""
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    bands = sc.bands(prm)
    with ctx:
        ctx.profile_series_enable(every=1, n_bins=200, bands=bands, capacity=4)
        ctx.advance(1e9, max_steps=4)
        assert len(ctx.profile_series_sums()["step"]) == 4
        ctx.profile_series_disable()
        assert capi.pool_scrub(0xFFFFFFFF) >= 1
        ctx.profile_series_enable(every=1, n_bins=100, bands=bands, capacity=4)
        ctx.advance(1e9, max_steps=2)
        got = ctx.profile_series_sums()
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.advance(1e9, max_steps=4)
        ctx.profile_series_enable(every=1, n_bins=100, bands=bands, capacity=64)
        ctx.advance(1e9, max_steps=2)
        want = ctx.profile_series_sums()
    assert got["step"].tolist() == [5, 6] and got["count"].shape == (2, 3, 100)
    assert all(np.all(np.isfinite(got[f])) for f in sc.FIELDS)
    assert np.any(got["count"][:, 1:] == 0)  # (a band of about 50 particles in 100 bins: zeros that had to be stored)
    sc.assert_series_identical(got, want, "after re-enabling with fewer bins")


# 6 ---------------------------------------------------------------------------------------------------------------
def test_limits(cfgmod, geom, capi, profmod):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    nf = parts["n_fluid"]
    bands = sc.bands(prm)
    L = capi.lib()
    with ctx:
        ctx.profile_series_enable(every=10 ** 9, n_bins=512, bands=bands, capacity=2)  # 3 x 512 = 1536 counters: all of the LDS
        ctx.advance(1e9, max_steps=3)
        ctx.profile_series_sample()
        d = ctx.download(fields=("pos", "vel"))
        got = ctx.profile_series_sums()
        assert got["count"].shape == (1, 3, 512)
        for b, band in enumerate([None] + bands):
            sc.assert_record_matches(got, 0, b, sc.numpy_sums(d["pos"][:nf], d["vel"][:nf], prm, 512, band), f"1536 counters, band {b}")
        for n_bins, n_bands in ((1537, 0), (769, 1), (513, 2)):
            cfg = capi.SphxProfileSeriesConfig(n_bins=n_bins, every=1, capacity=2, t_from=0.0, n_bands=n_bands)
            assert err_id(capi, L.sphx_ctx_profile_series_enable, ctx._h, C.byref(cfg)) == ("SPHX:ProfileSeries:config", capi.SPHX_ERR_ARG)
        sc.assert_series_identical(ctx.profile_series_sums(), got, "a refused enable leaves the records as they were")
        ctx.profile_series_sample()
        assert ctx.profile_series_sums()["step"].tolist() == [3, 3]       # ... and the series running


def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    nothing = (None, None, None, None, None, None, 0)

    def config(**kw):
        c = capi.SphxProfileSeriesConfig(n_bins=0, every=1, capacity=16, t_from=0.0, n_bands=0)
        for k, v in kw.items():
            if k in ("band_x", "band_hw"):
                for j, x in enumerate(v):
                    getattr(c, k)[j] = x
            else:
                setattr(c, k, v)
        return c

    with ctx:
        h = ctx._h
        assert err_id(capi, L.sphx_ctx_profile_series_read, h, 0, *nothing) == ("SPHX:ProfileSeries:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_ctx_profile_series_sample, h) == ("SPHX:ProfileSeries:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_profile_series_disable(h) == capi.SPHX_OK       # a no-op when off
        for call in (ctx.profile_series, ctx.profile_series_sums, ctx.profile_series_sample):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:ProfileSeries:disabled"
        ctx.profile_series_enable(every=1, capacity=16)
        ctx.advance(1e9, max_steps=5)
        before = ctx.profile_series_sums()
        assert len(before["step"]) == 5
        nan, inf = float("nan"), float("inf")
        refused = [dict(n_bins=-1), dict(every=0), dict(every=-1), dict(capacity=0), dict(capacity=-5), dict(t_from=nan),
                   dict(n_bands=-1), dict(n_bands=3), dict(n_bands=1, band_x=[nan], band_hw=[0.1]), dict(n_bands=1, band_x=[inf], band_hw=[0.1]),
                   dict(n_bands=2, band_x=[0.5, 0.5], band_hw=[0.1, -0.1]), dict(n_bands=1, band_x=[0.5], band_hw=[inf]),
                   dict(n_bins=1537), dict(capacity=(1 << 27) // 100 + 1)]   # (20 bins x 1 band x 5: 100 doubles a record)
        for bad in refused:
            c2 = config(**bad)
            assert err_id(capi, L.sphx_ctx_profile_series_enable, h, C.byref(c2)) == ("SPHX:ProfileSeries:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_profile_series_enable, h, None) == ("SPHX:ProfileSeries:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.profile_series_enable(every=0)
        assert e.value.identifier == "SPHX:ProfileSeries:config"
        sc.assert_series_identical(ctx.profile_series_sums(), before, "a refused enable leaves the records as they were")
        ctx.advance(1e9, max_steps=2)
        assert ctx.profile_series_sums()["step"].tolist() == list(range(1, 8))         # ... and the series running
        n, nb, nbd = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.sphx_ctx_profile_series_read(h, 0, None, None, C.byref(nb), C.byref(nbd), C.byref(n), None, 0) == capi.SPHX_OK
        assert (nb.value, nbd.value, n.value) == (20, 1, 7)
        times, records = np.zeros((7, 2)), np.zeros((7, 1, 20, 5))
        assert err_id(capi, L.sphx_ctx_profile_series_read, h, 6, capi.ptr(times), None, None, None, None, None, 0)[0] == "SPHX:ProfileSeries:capacity"
        assert err_id(capi, L.sphx_ctx_profile_series_read, h, 6, None, capi.ptr(records), None, None, None, None, 1)[0] == "SPHX:ProfileSeries:capacity"
        assert np.all(times == 0) and np.all(records == 0)
        assert L.sphx_ctx_profile_series_read(h, 7, capi.ptr(times), capi.ptr(records), None, None, None, None, 0) == capi.SPHX_OK
        assert times[:, 0].tolist() == list(range(1, 8)) and np.array_equal(records[:, 0, :, 1], ctx.profile_series_sums()["sum_ux"][:, 0])
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = config()
        for fn, args in ((L.sphx_ctx_profile_series_enable, (C.byref(cfg),)), (L.sphx_ctx_profile_series_disable, ()),
                         (L.sphx_ctx_profile_series_sample, ()), (L.sphx_ctx_profile_series_read, (0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:ProfileSeries:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


def test_a_non_finite_velocity_raises_the_range_flag(cfgmod, geom, capi):
    """Nothing is stepped: the sample of the initial state, of which one particle's u_y is NaN."""
    prm, parts, kw = sc.case(make_case, cfgmod, geom, "dp05_auto")
    vel = parts["vel"].copy(order="F")
    vel[5, 1] = float("nan")
    with capi.Context.from_parts(prm, dict(parts, vel=vel), t_end=1e9) as ctx:
        ctx.profile_series_enable(every=1, capacity=4)
        ctx.profile_series_sample()
        with pytest.raises(capi.SphxError) as e:
            ctx.profile_series_sums()
        assert e.value.identifier == "SPHX:ProfileSeries:range" and e.value.code == capi.SPHX_ERR_STATE


# 7 ---------------------------------------------------------------------------------------------------------------
SAMPLERS = ("series", "stats", "history", "field", "probes")
KERNELS = ("k_flow_stats", "k_step_history", "k_field_map", "k_point_probes", "k_profile_series")


def _on(ctx, prm, which):
    if "stats" in which:
        ctx.flow_stats_enable(every=1)
    if "history" in which:
        ctx.history_enable(every=1, capacity=64)
    if "field" in which:
        ctx.field_map_enable(nx=31, ny=17, every=1, with_walls=True)
    if "probes" in which:
        ctx.probes_enable([(0.3 * prm.DL, 0.5 * prm.DH), (0.0, 0.1 * prm.DH)], every=1, with_walls=True)
    if "series" in which:
        ctx.profile_series_enable(every=1, bands=sc.bands(prm), capacity=64)


def _read(ctx, which):
    out = {}
    if "stats" in which:
        out["stats"] = ctx.flow_stats_sums(0)
    if "history" in which:
        out["history"] = ctx.history()
    if "field" in which:
        out["field"] = ctx.field_map_sums()
    if "probes" in which:
        out["probes"] = ctx.probes()
    if "series" in which:
        out["series"] = ctx.profile_series_sums()
    return out


@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic"])
def test_no_feedback_on_the_physics_or_the_other_samplers(cfgmod, geom, capi, name):
    outs, reads = {}, {}
    for which in ((),) + tuple((s,) for s in SAMPLERS) + (SAMPLERS,):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            _on(ctx, prm, which)
            st = ctx.advance(1e9, max_steps=20)
            outs[which] = (st, ctx.download(fields=("pos", "vel", "drho_dt")))
            reads[which] = _read(ctx, which)
    for which, (st, d) in outs.items():
        assert st == outs[()][0], which            # the clock
        for k in ("pos", "vel", "drho_dt"):
            assert np.array_equal(d[k], outs[()][1][k]), (which, k)
    both = reads[SAMPLERS]
    assert len(both["series"]["step"]) == 20 == both["stats"]["n_samples"] == both["field"]["n_samples"] == len(both["history"]["t"]) == len(both["probes"]["t"])
    sc.assert_series_identical(reads[("series",)]["series"], both["series"], f"{name}: series alone vs all five")
    for k in sc.FIELDS:
        assert np.array_equal(reads[("stats",)]["stats"][k], both["stats"][k]), k
    for k in HISTORY_FIELDS:
        assert np.array_equal(reads[("history",)]["history"][k], both["history"][k]), k
    for k in ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2"):
        assert np.array_equal(reads[("field",)]["field"][k], both["field"][k]), k
    for k in ("step", "t", "weight", "u_x", "u_y", "rho"):
        assert np.array_equal(reads[("probes",)]["probes"][k], both["probes"][k], equal_nan=True), k


def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.profile_series_enable(every=1)
        on = profiled_launches(ctx, 20)
        ctx.profile_series_disable()
        off = profiled_launches(ctx, 20)
    assert all("k_profile_series" not in d for d in (never, never2, off))
    assert on.pop("k_profile_series") == 20
    assert on == never and off == never2
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # behind the other four, one launch each
        _on(ctx, prm, SAMPLERS)
        five = profiled_launches(ctx, 20)
    assert [five.pop(k) for k in KERNELS] == [20] * 5 and five == never


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.profile_series_enable(every=1, capacity=100)
        ctx.advance(1e9, max_steps=64)
        assert ctx.profile_series_sums()["step"].tolist() == list(range(65, 129))
        ctx.profile_series_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.profile_series_sums()
        assert e.value.identifier == "SPHX:ProfileSeries:disabled"
        ctx.profile_series_enable(every=2, n_bins=7)
        got = ctx.profile_series_sums()
        assert len(got["step"]) == 0 and got["count"].shape == (0, 1, 7) and got["n_dropped"] == 0
        ctx.prepare_steps(24)
        g0 = ctx.graph_stats()["graphs_captured"]
        st = ctx.advance(1e9, max_steps=24)
        assert ctx.graph_stats()["graphs_captured"] == g0
        got = ctx.profile_series_sums()
        assert got["step"].tolist() == list(range(194, 217, 2)) and got["t"][-1] == st["t"]
        ctx.prepare_steps(8)                               # prepared with the series on: disabling takes effect all the same
        ctx.profile_series_disable()
        ctx.advance(1e9, max_steps=8)
        ctx.profile_series_enable(every=1, n_bins=7)
        ctx.advance(1e9, max_steps=2)
        assert ctx.profile_series_sums()["step"].tolist() == [225, 226]


# 8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp01_multi", "dp05_auto"])
def test_repeatable(cfgmod, geom, capi, name):
    runs = []
    for _ in range(2):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            ctx.profile_series_enable(every=1, bands=sc.bands(prm), capacity=32)
            ctx.advance(1e9, max_steps=20)
            runs.append(ctx.profile_series_sums())
    assert len(runs[0]["step"]) == 20
    for k in sc.SERIES:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), f"{name}: {k}"


# 9 ---------------------------------------------------------------------------------------------------------------
def test_driver_series_holds_the_output_point_profiles(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.3, output_interval=0.1)
    res = driver.run(prm, profiles_every=1)
    s = res.profile_series
    assert len(s["step"]) == res.steps and s["n_dropped"] == 0 and s["step"].tolist() == list(range(1, res.steps + 1))
    assert s["u_mean"].shape == (res.steps, 2, len(res.y_mid)) and np.array_equal(s["y_mid"], res.y_mid)
    assert len(res.profile_times) == 4 and len(res.full_profile_u) == 3
    for k in range(1, len(res.profile_times)):
        (r,) = np.flatnonzero(s["t"] == res.profile_times[k])     # it exists, once
        for got, want in ((s["u_mean"][r, 1], res.mid_profile_u[k]), (s["u_mean"][r, 0], res.full_profile_u[k - 1])):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=1e-14)
    assert driver.run(prm).profile_series is None
    need = int(np.searchsorted(s["t"], 0.1 + 1e-12))              # the records of the first output interval
    assert need > 8
    with pytest.raises(RuntimeError, match=rf"profiles_capacity >= {need} \(it is 8\)"):
        driver.run(prm, profiles_every=1, profiles_capacity=8)


# 10 --------------------------------------------------------------------------------------------------------------
def test_the_series_follows_the_startup_transient(cfgmod, driver, profmod):
    """One run from rest: dp = 0.05, DL = 1.0, t_end = 1.0, every 5th step.  At the records nearest t = 0.25, 0.5 and 1.0 the
    mid-band profile is closer to the start-up solution than half the distance between that solution and the steady parabola
    (both relative L2 by profile.l2_error's rule, the parabola in the denominator): the series follows the transient, not the
    parabola.  A condition, not a measured bar.
    The reference physics meets it: the oracle's stepper (oracle/) on the same case, binned with
    profile.compute_mid_channel_profile at t = 0.25, 0.5, 1.0, gives L2_startup = 0.00810, 0.00499, 0.01273 where half the
    distance is 0.390, 0.305, 0.186 (233, 468, 945 steps)."""
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=1.0, output_interval=0.25)
    res = driver.run(prm, profiles_every=5)
    s = res.profile_series
    assert len(s["step"]) == res.steps // 5 and s["n_dropped"] == 0
    fig = driver.profile_series_figures(prm, s, band=1)
    y = s["y_mid"]
    u_exact = prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y)
    print(f"steps {res.steps}, records {len(s['step'])}, tau_fit / tau_exact = {fig['tau_fit'] / fig['tau_exact']:.4f}, "
          f"t_developed = {fig['t_developed']}")
    for t_want in (0.25, 0.5, 1.0):
        r = int(np.argmin(np.abs(s["t"] - t_want)))
        start = profmod.poiseuille_startup(y, np.array([s["t"][r]]), prm.gravity_g, prm.nu, prm.DH)[:, 0]
        gap = profmod.l2_error(start, u_exact)
        print(f"t = {s['t'][r]:.6f} (step {s['step'][r]}): L2_startup = {fig['L2_startup'][r]:.5f}, L2_steady = {fig['L2_steady'][r]:.5f}, "
              f"half the distance to the parabola = {0.5 * gap:.5f}")
        assert abs(s["t"][r] - t_want) < 0.01
        assert fig["L2_startup"][r] < 0.5 * gap


# 11 --------------------------------------------------------------------------------------------------------------
def test_matlab_gateway_pseries_commands(cfgmod, geom, capi):
    prm, parts, kw = sc.case(make_case, cfgmod, geom, "dp05_auto")
    bands = np.asfortranarray(np.array(sc.bands(prm)))
    gw = mex_mock.Gateway("sphx_ctx_mex.c")
    nf, nt = parts["n_fluid"], parts["n_total"]
    state = (parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"])
    (h,) = gw(1, "create", gateway_cfg(prm, 1e9), nf, nt, *state, 0.0, 0)
    try:
        with pytest.raises(mex_mock.MexError) as e:
            gw(10, "pseries_read", h, 0)
        assert e.value.identifier == "SPHX:ProfileSeries:disabled"
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "pseries_enable", h, 0, 1, 16, 0.0, np.zeros((3, 2), order="F"))
        assert e.value.identifier == "SPHX:ProfileSeries:config"
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "pseries_enable", h, 0, 0, 16, 0.0, bands)
        assert e.value.identifier == "SPHX:ProfileSeries:config"
        gw(0, "pseries_enable", h, 0, 2, 64, 0.0, bands)
        gw(1, "advance", h, 1e9, 30)
        gw(0, "pseries_sample", h)
        got = gw(10, "pseries_read", h, 1)
        gw(0, "pseries_sample", h)                             # the drained buffer starts again
        after = gw(10, "pseries_read", h, 0)
        gw(0, "pseries_disable", h)
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "pseries_sample", h)
        assert e.value.identifier == "SPHX:ProfileSeries:disabled"
    finally:
        gw(0, "destroy", h)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.profile_series_enable(every=2, capacity=64, bands=sc.bands(prm))
        ctx.advance(1e9, max_steps=30)
        ctx.profile_series_sample()
        want = ctx.profile_series_sums()
    assert len(want["step"]) == 16
    assert np.array_equal(np.ravel(got[0]), want["step"]) and np.array_equal(np.ravel(got[1]), want["t"])
    assert (got[7], got[8], got[9]) == (20, 3, 0)
    for k, f in enumerate(sc.FIELDS):
        assert got[2 + k].shape == (16, 60) and np.array_equal(got[2 + k], want[f].reshape(16, 60)), f
    assert (after[0], after[1]) == (30.0, want["t"][-1]) and after[9] == 0
    for k, f in enumerate(sc.FIELDS):
        assert after[2 + k].shape == (1, 60) and np.array_equal(after[2 + k][0], want[f][-1].ravel()), f
