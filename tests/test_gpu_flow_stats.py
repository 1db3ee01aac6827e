"""-m gpu: device-side flow statistics (include/sphx.h section 2a) -- time-averaged velocity profiles accumulated by
k_flow_stats inside the step loop.  Checked against numpy sums over download() (bins, bands, edges), against sampling
between steps from the host (bit for bit: the sample sits at the end of the step, on every schedule), for gating,
for leaving the physics and the launches untouched, for repeatability, for its error identifiers, against the
analytic profile over a long window, and through the MATLAB context gateway."""
import ctypes as C

import numpy as np
import pytest

import mex_mock
from helpers import assert_sums_identical, check_kernel_form, err_id, gateway_cfg, make_case, profiled_launches, stats_bands

pytestmark = pytest.mark.gpu

# (dp, DL, context options, make_case options): compact kernels at both sizes and several lane counts, the large-channel ("walk") kernels,
# a device-decided (dynamic) schedule and the dual-rate loop
CASES = {
    "dp05_auto": (0.05, 3.0, dict(), dict()),
    "dp05_lpp32": (0.05, 3.0, dict(lanes_per_particle=32), dict()),
    "dp025_lpp16": (0.025, 1.5, dict(lanes_per_particle=16), dict()),
    "dp025_walk": (0.025, 1.5, dict(lanes_per_particle=4), dict()),
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1), dict()),
    "dp025_dual": (0.025, 1.5, dict(lanes_per_particle=16, dual_rate=2), dict()),
    "dp01_multi": (0.01, 3.0, dict(), dict()),  # 30 k fluid particles: several workgroups per sample (global sums + ticket)
    "leftward": (0.05, 3.0, dict(), dict(U_bulk=-0.666667)),  # g < 0: u_x, its sums and means negative, the wrap at x < 0
}
FIELDS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2")


def _case(cfgmod, geom, name, seed=11):
    dp, DL, kw, mk = CASES[name]
    prm, parts = make_case(cfgmod, geom, **dict(dict(dp=dp, DL=DL, jitter=0.2, seed=seed, developed=True), **mk))
    return prm, parts, kw


def _numpy_sums(pos, vel, prm, n_bins, band=None):
    x, y, ux, uy = pos[:, 0], pos[:, 1], vel[:, 0], vel[:, 1]
    if band is not None:
        xw = np.mod(x, prm.DL)
        d = np.abs(xw - band[0])
        d = np.minimum(d, prm.DL - d)
        sel = d <= band[1]
        y, ux, uy = y[sel], ux[sel], uy[sel]
    edges = np.linspace(0.0, prm.DH, n_bins + 1)
    inside = (y >= edges[0]) & (y <= edges[-1])
    k = np.minimum(np.searchsorted(edges, y[inside], side="right") - 1, n_bins - 1)
    ux, uy = ux[inside], uy[inside]
    return dict(zip(FIELDS, [np.bincount(k, weights=w, minlength=n_bins).astype(np.float64)
                             for w in (np.ones_like(ux), ux, ux * ux, uy, uy * uy)]))


def _assert_sums_match(got, want, what):
    assert np.array_equal(got["count"], want["count"]), what + ": counts"
    # (the device sums exactly in fixed point with a quantum set by max|v|, numpy in floating point: both are compared to
    #  the largest |sum| of the band)
    scale = max(max(float(np.max(np.abs(want[f]))) for f in FIELDS[1:]), 1e-300)
    for f in FIELDS[1:]:
        err = float(np.max(np.abs(got[f] - want[f])))
        assert err <= 1e-12 * scale, f"{what}: {f} off by {err / scale:.3e} of the largest |sum|"


def _all_sums(ctx, n_bands=3):
    return [ctx.flow_stats_sums(b) for b in range(n_bands)]


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_sample_now_matches_numpy(cfgmod, geom, capi, profmod, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    nf = parts["n_fluid"]
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    bands = stats_bands(prm)
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        check_kernel_form(ctx, name)
        ctx.flow_stats_enable(every=10 ** 9, bands=bands)
        ctx.advance(1e9, max_steps=7)
        ctx.flow_stats_sample()
        d = ctx.download(fields=("pos", "vel"))
        st = ctx.sync()
        got = _all_sums(ctx)
        mid = ctx.flow_stats(1)
    pos, vel = d["pos"][:nf], d["vel"][:nf]
    for b, band in enumerate([None] + bands):
        _assert_sums_match(got[b], _numpy_sums(pos, vel, prm, n_bins, band), f"{name} band {b}")
        assert got[b]["n_samples"] == 1 and got[b]["t_first"] == got[b]["t_last"] == st["t"]
    _, u_mid = profmod.compute_mid_channel_profile(pos, vel[:, 0], prm.DL, prm.DH, bands[0][0], bands[0][1], n_bins)
    assert np.array_equal(np.isnan(mid["u_mean"]), np.isnan(u_mid))
    ok = ~np.isnan(u_mid)
    np.testing.assert_allclose(mid["u_mean"][ok], u_mid[ok], rtol=1e-12, atol=1e-14)
    if name == "leftward":
        # (bins at least 2h from the walls: next to them a jittered particle with y < 0 carries the parabola's other sign)
        inner = (mid["y_mid"] >= 2.0 * prm.h) & (mid["y_mid"] <= prm.DH - 2.0 * prm.h)
        assert prm.gravity_g < 0 and inner.sum() >= n_bins - 8 and np.all(mid["u_mean"][inner & ok] < 0) and (inner & ok).sum() >= inner.sum() - 1
        for b in range(3):
            assert np.all(got[b]["sum_ux"][inner & (got[b]["count"] > 0)] < 0)


# 2 ---------------------------------------------------------------------------------------------------------------
def test_particles_on_edges_and_outside(cfgmod, geom, capi, profmod):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=5, developed=True)
    nf = parts["n_fluid"]
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    edges = np.linspace(0.0, prm.DH, n_bins + 1)
    pos = parts["pos"].copy(order="F")
    specials = list(edges) + [0.0, prm.DH, -1e-12, prm.DH + 1e-12, np.nextafter(edges[3], 0.0), np.nextafter(edges[7], 1.0)]
    idx = np.arange(0, len(specials) * 37, 37)[: len(specials)]
    assert idx[-1] < nf
    pos[idx, 1] = specials
    parts = dict(parts, pos=pos)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.flow_stats_enable(n_bins=n_bins, every=10 ** 9)
        ctx.flow_stats_sample()
        d = ctx.download(fields=("pos", "vel"))
        got = ctx.flow_stats_sums(0)
        prof = ctx.flow_stats(0)
    assert np.array_equal(d["pos"][idx, 1], np.asarray(specials))
    want = _numpy_sums(d["pos"][:nf], d["vel"][:nf], prm, n_bins)
    _assert_sums_match(got, want, "edges")
    assert got["count"].sum() == nf - 2  # the two particles just outside [0, DH] are dropped
    _, u_ref = profmod.compute_binned_profile_mean(d["pos"][:nf, 1], d["vel"][:nf, 0], 0.0, prm.DH, n_bins)
    np.testing.assert_allclose(prof["u_mean"], u_ref, rtol=1e-12, atol=1e-14)


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_lpp16", "dp025_walk", "dp05_dynamic", "dp025_dual", "dp01_multi"])
def test_in_loop_equals_sampling_between_steps(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    bands = stats_bands(prm)
    N = 48
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:  # in the loop, one advance call (graph replays)
        ctx.flow_stats_enable(every=1, bands=bands)
        st = ctx.advance(1e9, max_steps=N)
        assert st["step"] == N
        rebins = ctx.schedule()["rebins"]
        in_loop = _all_sums(ctx)
    assert rebins >= 2, f"{name}: only {rebins} re-binnings in {N} steps"
    assert in_loop[0]["n_samples"] == N
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:  # from the host, after every single step
        ctx.flow_stats_enable(every=10 ** 9, bands=bands)
        for _ in range(N):
            ctx.advance(1e9, max_steps=1)
            ctx.flow_stats_sample()
        between = _all_sums(ctx)
    assert_sums_identical(in_loop, between, f"{name}: in-loop vs between steps")
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:  # in the loop, chunked calls (eager slots and short graphs)
        ctx.flow_stats_enable(every=1, bands=bands)
        for n in (1, 3, 5, 11, 28):
            ctx.advance(1e9, max_steps=n)
        chunked = _all_sums(ctx)
    assert_sums_identical(in_loop, chunked, f"{name}: one call vs chunked")


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_gating_every_and_t_from(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    N, every = 40, 3
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        statuses = [ctx.advance(1e9, max_steps=1) for _ in range(N)]
    t_from = 0.5 * (statuses[N // 2]["t"] + statuses[N // 2 + 1]["t"])
    want = [s for s in statuses if s["step"] % every == 0 and s["t"] >= t_from]
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        ctx.flow_stats_enable(every=every, t_from=t_from)
        ctx.advance(1e9, max_steps=N)
        got = ctx.flow_stats(0)
    assert got["n_samples"] == len(want) > 0
    assert got["t_first"] == want[0]["t"] and got["t_last"] == want[-1]["t"]


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp05_dynamic"])
def test_no_feedback_on_the_physics(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    outs = []
    for on in (False, True):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            if on:
                ctx.flow_stats_enable(every=1, bands=stats_bands(prm))
            st = ctx.advance(1e9, max_steps=45)
            outs.append((st, ctx.download(fields=("pos", "vel", "drho_dt"))))
    assert outs[0][0] == outs[1][0]
    for k in ("pos", "vel", "drho_dt"):
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.flow_stats_enable(every=1)
        on = profiled_launches(ctx, 20)
        ctx.flow_stats_disable()
        off = profiled_launches(ctx, 20)
    assert "k_flow_stats" not in never and "k_flow_stats" not in never2 and "k_flow_stats" not in off
    assert on.pop("k_flow_stats") == 20
    assert on == never and off == never2


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.flow_stats_enable(every=1)
        ctx.advance(1e9, max_steps=64)
        assert ctx.flow_stats(0)["n_samples"] == 64
        ctx.flow_stats_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.flow_stats(0)
        assert e.value.identifier == "SPHX:Stats:disabled"
        ctx.flow_stats_enable(every=2)
        assert ctx.flow_stats(0)["n_samples"] == 0
        ctx.prepare_steps(24)
        g0 = ctx.graph_stats()["graphs_captured"]
        st = ctx.advance(1e9, max_steps=24)
        assert ctx.graph_stats()["graphs_captured"] == g0
        got = ctx.flow_stats(0)
        assert got["n_samples"] == 12 and got["t_last"] == st["t"]
        ctx.flow_stats_reset()
        assert ctx.flow_stats(0)["n_samples"] == 0 and np.all(ctx.flow_stats_sums(0)["count"] == 0)


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp01_multi"])
def test_repeatable(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    runs = []
    for _ in range(2):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.flow_stats_enable(every=1, bands=stats_bands(prm))
            ctx.advance(1e9, max_steps=60)
            runs.append(_all_sums(ctx))
    assert_sums_identical(runs[0], runs[1], name)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        h = ctx._h
        cfg = capi.SphxFlowStatsConfig(n_bins=0, every=1, t_from=0.0, n_bands=1)
        assert err_id(capi, L.sphx_ctx_flow_stats_read, h, 0, 0, None, *[None] * 5, None, None, None)[0] == "SPHX:Stats:disabled"
        assert err_id(capi, L.sphx_ctx_flow_stats_sample, h)[0] == "SPHX:Stats:disabled"
        for bad in (dict(every=0), dict(every=-1), dict(n_bands=3), dict(n_bins=-1), dict(n_bins=1000)):
            c2 = capi.SphxFlowStatsConfig(n_bins=0, every=1, t_from=0.0, n_bands=1)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert err_id(capi, L.sphx_ctx_flow_stats_enable, h, C.byref(c2)) == ("SPHX:Stats:config", capi.SPHX_ERR_ARG), bad
        with pytest.raises(capi.SphxError) as e:
            ctx.flow_stats_enable(every=0)
        assert e.value.identifier == "SPHX:Stats:config"
        assert L.sphx_ctx_flow_stats_enable(h, C.byref(cfg)) == capi.SPHX_OK
        n = C.c_int(0)
        buf = [np.zeros(64) for _ in range(5)]
        assert err_id(capi, L.sphx_ctx_flow_stats_read, h, 2, 64, None, *[capi.ptr(b) for b in buf], None, None, None)[0] == "SPHX:Stats:band"
        assert err_id(capi, L.sphx_ctx_flow_stats_read, h, -1, 64, None, *[capi.ptr(b) for b in buf], None, None, None)[0] == "SPHX:Stats:band"
        assert L.sphx_ctx_flow_stats_read(h, 0, 0, C.byref(n), *[None] * 5, None, None, None) == capi.SPHX_OK
        assert n.value == 20
        assert err_id(capi, L.sphx_ctx_flow_stats_read, h, 0, n.value - 1, None, *[capi.ptr(b) for b in buf], None, None, None)[0] == "SPHX:Stats:capacity"
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = capi.SphxFlowStatsConfig(n_bins=0, every=1, t_from=0.0, n_bands=0)
        for fn, args in ((L.sphx_ctx_flow_stats_enable, (C.byref(cfg),)), (L.sphx_ctx_flow_stats_disable, ()),
                         (L.sphx_ctx_flow_stats_reset, ()), (L.sphx_ctx_flow_stats_sample, ()),
                         (L.sphx_ctx_flow_stats_read, (0, 0, None, *[None] * 5, None, None, None))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:Stats:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


# 8 ---------------------------------------------------------------------------------------------------------------
def test_time_averaged_profile_meets_the_acceptance_bar(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.025, DL=3.0, end_time=20.0, output_interval=1.0)
    res = driver.run(prm, average_from=16.0)
    ta = res.time_avg
    print(f"time-averaged L2 = {ta['L2']:.5f} over {ta['n_samples']} samples in [{ta['t_first']:.4f}, {ta['t_last']:.4f}]; "
          f"five-snapshot L2 = {res.L2_time_mean():.5f}; uy_rms/Umax = {ta['uy_rms_over_umax']:.5f}; "
          f"ux_std_centre/Umax = {ta['ux_std_centre_over_umax']:.5f}")
    assert ta["n_samples"] > 1000 and ta["t_first"] >= 16.0 and ta["t_last"] == res.t
    assert ta["L2"] <= 0.01


# 9 ---------------------------------------------------------------------------------------------------------------
def test_matlab_gateway_stats_commands(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    gw = mex_mock.Gateway("sphx_ctx_mex.c")
    nf, nt = parts["n_fluid"], parts["n_total"]
    state = (parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"])
    bands = np.array(stats_bands(prm))
    (h,) = gw(1, "create", gateway_cfg(prm, 1e9), nf, nt, *state, 0.0, 0)
    try:
        gw(0, "stats_enable", h, 0, 2, 0.0, bands)
        gw(1, "advance", h, 1e9, 30)
        gw(0, "stats_sample", h)
        got = [gw(8, "stats_read", h, b) for b in range(3)]
        with pytest.raises(mex_mock.MexError) as e:
            gw(8, "stats_read", h, 3)
        assert e.value.identifier == "SPHX:Stats:band"
    finally:
        gw(0, "destroy", h)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.flow_stats_enable(every=2, bands=[tuple(b) for b in bands])
        ctx.advance(1e9, max_steps=30)
        ctx.flow_stats_sample()
        want = _all_sums(ctx)
    for b in range(3):
        for k, f in enumerate(FIELDS):
            assert np.array_equal(got[b][k], want[b][f]), (b, f)
        assert (got[b][5], got[b][6], got[b][7]) == (want[b]["n_samples"], want[b]["t_first"], want[b]["t_last"])
