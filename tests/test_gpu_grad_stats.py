"""-m gpu: the device-side gradient statistics (include/sphx.h section 2n) -- the velocity gradient at every fluid particle,
estimated by k_grad_stats inside the step loop and binned.  count and skipped are compared exactly, the summed fields within the
bound of tests/grad_stats_cases.py.  Checked against profile.grad_stats_sums (numpy) of download() on every form of the step,
with and without walls, over the bin counts up to the LDS limit; on a linear field (exact); on the lattice at rest (exact
zeros); in the loop against numpy sums of the state after every step, across scheduled and drift-forced re-binnings; for its
gate (the pair statistics'), for repeatability to the byte, for its limits and error identifiers, for leaving the launches and
the other six samplers untouched, and for a particle without partners (skipped, not NaN)."""
import ctypes as C

import numpy as np
import pytest

import grad_stats_cases as gc
import probe_cases
from helpers import HISTORY_FIELDS, STATS_FIELDS, check_kernel_form, err_id, make_case, profiled_launches

pytestmark = pytest.mark.gpu

NEVER = 10 ** 9  # an `every` no test reaches: the sampler is on and only samples when asked


def _ctx(capi, cfgmod, geom, name, **more):
    prm, parts, kw = probe_cases.case(make_case, cfgmod, geom, name)
    return prm, parts, capi.Context.from_parts(prm, parts, t_end=1e9, **dict(kw, **more))


def _all_sums(ctx, n_bands=3):
    return [ctx.grad_stats_sums(b) for b in range(n_bands)]


def _scales(profmod, prm, parts, vmax):
    return profmod.grad_scales(vmax, prm.h, parts["n_fluid"])


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.CASES))
def test_sample_now_matches_numpy(cfgmod, geom, capi, profmod, name):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    xbands = gc.bands(prm)
    with ctx:
        check_kernel_form(ctx, name)
        st = ctx.advance(1e9, max_steps=7)
        state = ctx.download(fields=("pos", "vel"))
        sc = _scales(profmod, prm, parts, st["vmax"])
        for walls in (False, True):
            grads = gc.gradients(profmod, prm, parts, state, walls)
            for n_bins in gc.BINS:
                what = f"{name}: n_bins {n_bins} walls {walls}"
                ctx.grad_stats_enable(n_bins=n_bins, every=NEVER, with_walls=walls, bands=xbands)
                ctx.grad_stats_sample()
                got = _all_sums(ctx)
                want = gc.numpy_sums(profmod, prm, parts, state, n_bins, xbands, grads, vmax=st["vmax"])
                gc.assert_sums_match(got, want, gc.quantisation(want, sc), what)
                assert all(g["n_samples"] == 1 and g["t_first"] == g["t_last"] == st["t"] for g in got), what
                assert got[0]["count"].sum() >= got[1]["count"].sum() > 0 and got[2]["count"].sum() > 0, what
                assert got[0]["count"].sum() + got[0]["skipped"].sum() <= parts["n_fluid"] and got[0]["skipped"].sum() == 0, what
    assert st["step"] == 7


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", [False, True])
def test_linear_field_as_uploaded(cfgmod, geom, capi, profmod, walls):
    """u = (a + b y, c y), walls included: G = (0, b, 0, c) at every particle, whatever the arrangement.  No step is taken: the
    clock's max |v| is the one the context computed from the uploaded state."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=11, developed=True)
    lin, (_, b, _, c) = gc.linear_field(prm, parts)
    with capi.Context.from_parts(prm, lin, t_end=1e9) as ctx:
        vmax = ctx.sync()["vmax"]
        ctx.grad_stats_enable(every=NEVER, with_walls=walls, bands=gc.bands(prm))
        ctx.grad_stats_sample()
        profs = [ctx.grad_stats(k) for k in range(3)]
    assert abs(vmax - gc.vmax_of(lin, lin)) <= 1e-14 * vmax and vmax > 0
    sc = _scales(profmod, prm, parts, vmax)
    big = max(abs(b), abs(c))
    tol1 = 1e-12 * big + 2.0 ** -(sc["s1"] + 1)                 # a mean of values each rounded to 2^-s1
    tol3 = 2.0 ** -(sc["s3"] + 1)                               # ... of squares each rounded to 2^-s3
    for k, p in enumerate(profs):
        ok = p["count"] > 0
        assert ok.sum() >= 15 and np.all(p["skipped"] == 0), k
        for comp, want in (("gxx", 0.0), ("gxy", b), ("gyx", 0.0), ("gyy", c)):
            err = float(np.max(np.abs(p[comp + "_mean"][ok] - want)))
            print(f"linear field, walls {walls}, band {k}: {comp} off by {err:.3e} (allowed {tol1:.3e})")
            assert err <= tol1, (k, comp)
        # sqrt(c^2 + d) - |c| <= |d| / |c|
        assert float(np.max(np.abs(p["div_rms"][ok] - abs(c)))) <= 1e-12 * big + (tol3 + 2 * abs(c) * tol1) / abs(c), k
        assert float(np.max(np.abs(p["vort_mean"][ok] + b))) <= 2 * tol1, k


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", [False, True])
def test_lattice_at_rest_sums_to_exact_zeros(cfgmod, geom, capi, walls):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.0, developed=False)
    assert parts["n_fluid"] == 1200 and not np.any(parts["vel"])
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.grad_stats_enable(n_bins=20, every=NEVER, with_walls=walls)
        ctx.grad_stats_sample()
        s = ctx.grad_stats_sums(0)
    assert np.all(s["count"] == 1200 / 20) and np.all(s["skipped"] == 0) and s["n_samples"] == 1
    for f in gc.SUMMED:
        assert np.all(s[f] == 0.0) and not np.any(np.signbit(s[f])), f


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, more", [("dp05_auto", dict(rebuild_every=4)), ("dp05_dynamic", dict()),
                                        ("dp05_auto", dict(rebuild_every=8, skin_h=0.05))])   # (a skin far too thin: the drift bound)
def test_in_loop_equals_numpy_sums_of_every_step(cfgmod, geom, capi, profmod, name, more):
    N = 24
    setting = dict(n_bins=20, with_walls=False)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name, **more)
    xbands = gc.bands(prm)
    with ctx:   # in the loop, one advance call (graph replays); the step history records this run's own clock
        ctx.grad_stats_enable(every=1, bands=xbands, **setting)
        ctx.history_enable(every=1, capacity=64)
        st = ctx.advance(1e9, max_steps=N)
        in_loop = _all_sums(ctx)
        clock = ctx.history()["t"]
        rebins, forced_a = ctx.schedule()["rebins"], ctx.grid_policy()["forced_rebuilds"]
    assert st["step"] == N and len(clock) == N and clock[-1] == st["t"]
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name, **more)
    total = quant = None
    statuses = []
    with ctx:   # step by step, with a download and numpy's sums after every step; sampled in the loop as well
        ctx.grad_stats_enable(every=1, bands=xbands, **setting)
        for _ in range(N):
            s1 = ctx.advance(1e9, max_steps=1)
            statuses.append(s1)
            state = ctx.download(fields=("pos", "vel"))
            one = gc.numpy_sums(profmod, prm, parts, state, 20, xbands, gc.gradients(profmod, prm, parts, state, False), vmax=s1["vmax"])
            q = gc.quantisation(one, _scales(profmod, prm, parts, s1["vmax"]))
            total = one if total is None else gc.add_sums(total, one)
            quant = q if quant is None else gc.add_quantisation(quant, q)
        stepped = _all_sums(ctx)
        forced_b = ctx.grid_policy()["forced_rebuilds"]
    print(f"{name} {more}: {rebins} re-binnings, forced {forced_a} / {forced_b}")
    assert rebins + forced_a >= (2 if more else 1)   # (the dynamic schedule re-bins when the device decides: once in these steps)
    if "skin_h" in more:
        assert forced_a >= 1 and forced_b >= 1
    gc.assert_sums_match(stepped, total, quant, f"{name} {more}: step by step")
    gc.assert_sums_match(in_loop, total, quant, f"{name} {more}: one call")
    # The re-binning schedule is a function of the step count and of device-side events alone (test_gpu_grid_skin.py:
    # test_call_pattern_does_not_change_the_bits), a stop on the drift bound included: both runs take the same steps from the same
    # layouts, so their clocks and their sums are the same bits.
    for how, band in (("one call", in_loop[0]), ("step by step", stepped[0])):
        print(f"{name} {more}: {how}: n_samples {band['n_samples']} t_first {band['t_first']!r} t_last {band['t_last']!r}; the one call's "
              f"history {float(clock[0])!r} {float(clock[-1])!r}, the single steps' status {statuses[0]['t']!r} {statuses[-1]['t']!r}")
    assert forced_a == forced_b
    for band in in_loop:
        assert (band["n_samples"], band["t_first"], band["t_last"]) == (N, clock[0], clock[-1])   # its own clock ...
    for band in in_loop + stepped:
        assert (band["n_samples"], band["t_first"], band["t_last"]) == (N, statuses[0]["t"], statuses[-1]["t"])   # ... and the other run's
    gc.assert_identical(in_loop, stepped, f"{name} {more}: one call against single steps")


def test_gate_is_the_pair_statistics_gate(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        times = [ctx.advance(1e9, max_steps=1)["t"] for _ in range(24)]
    t_from = 0.5 * (times[6] + times[7])   # between step 7 and step 8
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.grad_stats_enable(every=5, t_from=t_from)
        ctx.pair_dist_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=24)
        g, p = ctx.grad_stats_sums(0), ctx.pair_dist_sums()[0]
        ctx.grad_stats_enable(every=NEVER)
        ctx.advance(1e9, max_steps=5)
        idle = ctx.grad_stats_sums(0)
    assert (g["n_samples"], g["t_first"], g["t_last"]) == (p["n_samples"], p["t_first"], p["t_last"]) == (3, times[9], times[19])
    assert 0 < g["count"].sum() + g["skipped"].sum() <= 3 * parts["n_fluid"]   # (a particle outside [0, DH] is dropped)
    assert idle["n_samples"] == 0 and np.isnan(idle["t_first"]) and all(not np.any(idle[f]) for f in gc.FIELDS)


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp01_multi"])   # one workgroup row of 19, and the 469 of 30 k particles
def test_repeatable_to_the_byte(cfgmod, geom, capi, name):
    runs = []
    for _ in range(2):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            ctx.grad_stats_enable(every=1, with_walls=True, bands=gc.bands(prm))
            ctx.advance(1e9, max_steps=10)
            runs.append(_all_sums(ctx))
    assert runs[0][0]["n_samples"] == 10 and runs[0][0]["count"].sum() > 0 and np.any(runs[0][0]["sum_gxy"] != 0.0)
    gc.assert_identical(runs[0], runs[1], f"{name}: two identical runs")


# 7 ---------------------------------------------------------------------------------------------------------------
def test_limits(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    L = capi.lib()
    with ctx:
        ctx.grad_stats_enable(n_bins=213, every=NEVER, bands=gc.bands(prm))   # 3 x 213 = 639 of 640
        ctx.grad_stats_sample()
        got = _all_sums(ctx)
        assert got[0]["count"].shape == (213,) and got[0]["count"].sum() == parts["n_fluid"]
        for n_bins, n_bands in ((641, 0), (321, 1), (214, 2), (-1, 0)):
            cfg = capi.SphxGradStatsConfig(n_bins=n_bins, every=1, det_min=0.05, n_bands=n_bands)
            for k in range(n_bands):
                cfg.band_x[k], cfg.band_hw[k] = 0.5, 0.1
            assert err_id(capi, L.sphx_ctx_grad_stats_enable, ctx._h, C.byref(cfg)) == ("SPHX:GradStats:config", capi.SPHX_ERR_ARG), n_bins
        gc.assert_identical(_all_sums(ctx), got, "a refused enable leaves the sums as they were")
        ctx.grad_stats_sample()
        assert ctx.grad_stats_sums(0)["n_samples"] == 2   # ... and the sampler running
        ctx.grad_stats_enable(n_bins=640, every=NEVER)
        ctx.grad_stats_sample()
        assert ctx.grad_stats_sums(0)["count"].sum() == parts["n_fluid"]


def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    nothing = (None,) * 5

    def config(**kw):
        c = capi.SphxGradStatsConfig(n_bins=20, every=1, t_from=0.0, det_min=0.05, with_walls=0, n_bands=0)
        for k, v in kw.items():
            if k in ("band_x", "band_hw"):
                for j, x in enumerate(v):
                    getattr(c, k)[j] = x
            else:
                setattr(c, k, v)
        return c

    with ctx:
        h = ctx._h
        for fn, args in ((L.sphx_ctx_grad_stats_read, (0, 0, *nothing)), (L.sphx_ctx_grad_stats_sample, ()), (L.sphx_ctx_grad_stats_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:GradStats:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_grad_stats_disable(h) == capi.SPHX_OK       # a no-op when off
        for call in (ctx.grad_stats, ctx.grad_stats_sums, ctx.grad_stats_sample, ctx.grad_stats_reset):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:GradStats:disabled"
        ctx.grad_stats_enable(every=1, bands=gc.bands(prm))
        ctx.advance(1e9, max_steps=5)
        before = _all_sums(ctx)
        assert before[0]["n_samples"] == 5
        nan, inf = float("nan"), float("inf")
        refused = [dict(n_bins=-1), dict(n_bins=641), dict(every=0), dict(every=-1), dict(t_from=nan), dict(det_min=-0.01), dict(det_min=nan),
                   dict(det_min=inf), dict(with_walls=2), dict(with_walls=-1), dict(n_bands=-1), dict(n_bands=3),
                   dict(n_bands=1, band_x=[nan], band_hw=[0.1]), dict(n_bands=1, band_x=[inf], band_hw=[0.1]),
                   dict(n_bands=2, band_x=[0.5, 0.5], band_hw=[0.1, -0.1]), dict(n_bands=1, band_x=[0.5], band_hw=[inf])]
        for bad in refused:
            c2 = config(**bad)
            assert err_id(capi, L.sphx_ctx_grad_stats_enable, h, C.byref(c2)) == ("SPHX:GradStats:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_grad_stats_enable, h, None) == ("SPHX:GradStats:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.grad_stats_enable(det_min=-1.0)
        assert e.value.identifier == "SPHX:GradStats:config"
        gc.assert_identical(_all_sums(ctx), before, "a refused enable leaves the sums as they were")
        ctx.advance(1e9, max_steps=2)
        assert ctx.grad_stats_sums(0)["n_samples"] == 7                  # ... and the sampler running
        for band in (-1, 3):
            assert err_id(capi, L.sphx_ctx_grad_stats_read, h, band, 0, *nothing) == ("SPHX:GradStats:band", capi.SPHX_ERR_ARG)
            with pytest.raises(capi.SphxError) as e:
                ctx.grad_stats(band)
            assert e.value.identifier == "SPHX:GradStats:band"
        sums = np.full((12, 20), -7.0)
        assert err_id(capi, L.sphx_ctx_grad_stats_read, h, 0, 19, None, capi.ptr(sums), None, None, None)[0] == "SPHX:GradStats:capacity"
        assert np.all(sums == -7.0)
        nb, ns = C.c_int(0), C.c_int64(0)
        assert L.sphx_ctx_grad_stats_read(h, 2, 0, C.byref(nb), None, C.byref(ns), None, None) == capi.SPHX_OK   # no array: no capacity
        assert (nb.value, ns.value) == (20, 7)
        wide = np.full((12, 25), -7.0)
        assert L.sphx_ctx_grad_stats_read(h, 1, 25, None, capi.ptr(wide), None, None, None) == capi.SPHX_OK   # field f of bin k at f * capacity + k
        want = ctx.grad_stats_sums(1)
        for j, f in enumerate(gc.FIELDS):
            assert np.array_equal(wide[j, :20], want[f]) and np.all(wide[j, 20:] == -7.0), f
        ctx.grad_stats_reset()
        assert all(s["n_samples"] == 0 and not np.any(s["count"]) and not np.any(s["sum_gxy"]) for s in _all_sums(ctx))
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = config()
        for fn, args in ((L.sphx_ctx_grad_stats_enable, (C.byref(cfg),)), (L.sphx_ctx_grad_stats_disable, ()), (L.sphx_ctx_grad_stats_reset, ()),
                         (L.sphx_ctx_grad_stats_sample, ()), (L.sphx_ctx_grad_stats_read, (0, 0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:GradStats:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.grad_stats_enable(every=1)
        ctx.advance(1e9, max_steps=64)
        assert ctx.grad_stats_sums(0)["n_samples"] == 64
        ctx.grad_stats_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.grad_stats_sums(0)
        assert e.value.identifier == "SPHX:GradStats:disabled"
        ctx.grad_stats_enable(every=2, n_bins=7)
        ctx.advance(1e9, max_steps=24)
        got = ctx.grad_stats_sums(0)
        assert got["n_samples"] == 12 and got["count"].shape == (7,) and 0 < got["count"].sum() + got["skipped"].sum() <= 12 * parts["n_fluid"]


def _six_on(ctx, prm):
    ctx.flow_stats_enable(every=1)
    ctx.history_enable(every=1, capacity=64)
    ctx.field_map_enable(nx=31, ny=17, every=1, with_walls=True)
    ctx.probes_enable([(0.3 * prm.DL, 0.5 * prm.DH), (0.0, 0.1 * prm.DH)], every=1, with_walls=True)
    ctx.profile_series_enable(every=1, bands=gc.bands(prm), capacity=64)
    ctx.pair_dist_enable(every=1, with_walls=True, bands=gc.bands(prm))


def _six_read(ctx):
    return dict(stats=ctx.flow_stats_sums(0), history=ctx.history(), field=ctx.field_map_sums(), probes=ctx.probes(),
                series=ctx.profile_series_sums(), pairs=ctx.pair_dist_sums())


@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic"])
def test_no_feedback_on_the_physics_or_the_other_six_samplers(cfgmod, geom, capi, name):
    runs = {}
    for grads, others in ((False, False), (True, False), (False, True), (True, True)):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            if others:
                _six_on(ctx, prm)
            if grads:
                ctx.grad_stats_enable(every=1, with_walls=True, bands=gc.bands(prm))
            st = ctx.advance(1e9, max_steps=20)
            runs[grads, others] = (st, ctx.download(fields=("pos", "vel", "drho_dt")), _six_read(ctx) if others else None,
                                   _all_sums(ctx) if grads else None)
    st0, d0 = runs[False, False][:2]
    for key, (st, d, _, _) in runs.items():
        assert st == st0, key
        for k in ("pos", "vel", "drho_dt"):
            assert np.array_equal(d[k], d0[k]), (key, k)
    gc.assert_identical(runs[True, False][3], runs[True, True][3], f"{name}: alone against all seven")
    assert runs[True, True][3][0]["n_samples"] == 20
    a, b = runs[False, True][2], runs[True, True][2]
    for k in STATS_FIELDS:
        assert np.array_equal(a["stats"][k], b["stats"][k]), k
        assert np.array_equal(a["series"][k], b["series"][k]), k
    for k in HISTORY_FIELDS:
        assert np.array_equal(a["history"][k], b["history"][k]), k
    for k in ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2"):
        assert np.array_equal(a["field"][k], b["field"][k]), k
    for k in ("step", "t", "weight", "u_x", "u_y", "rho"):
        assert np.array_equal(a["probes"][k], b["probes"][k], equal_nan=True), k
    for x, y in zip(a["pairs"], b["pairs"]):
        assert np.array_equal(x["ff"], y["ff"]) and np.array_equal(x["fw"], y["fw"]) and x["centres"] == y["centres"] and x["r2_min"] == y["r2_min"]


# 8 ---------------------------------------------------------------------------------------------------------------
def test_a_particle_without_partners_is_skipped(cfgmod, geom, capi, profmod):
    """The channel is full of fluid: a hole is made around one particle by moving every other fluid particle within 2.3 h of it
    half a channel length along x, on top of the fluid there.  Sampled as uploaded, walls off."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=11, developed=True)
    nf = parts["n_fluid"]
    pos = parts["pos"].copy(order="F")
    lone = int(np.argmin(np.hypot(pos[:nf, 0] - 1.0, pos[:nf, 1] - 0.5)))
    dx = pos[:nf, 0] - pos[lone, 0]
    near = (np.hypot(dx, pos[:nf, 1] - pos[lone, 1]) < 2.3 * prm.h) & (np.arange(nf) != lone)
    assert 15 < near.sum() < 40
    pos[:nf][near, 0] += 0.5 * prm.DL
    holed = dict(parts, pos=pos)
    n_bins = 20
    with capi.Context.from_parts(prm, holed, t_end=1e9) as ctx:
        vmax = ctx.sync()["vmax"]
        ctx.grad_stats_enable(n_bins=n_bins, every=NEVER, bands=gc.bands(prm))
        ctx.grad_stats_sample()
        got = _all_sums(ctx)
    k = int(pos[lone, 1] / (prm.DH / n_bins))
    want_skipped = np.zeros(n_bins)
    want_skipped[k] = 1.0
    assert np.array_equal(got[0]["skipped"], want_skipped) and got[0]["count"].sum() == nf - 1
    assert all(np.all(np.isfinite(got[b][f])) for b in range(3) for f in gc.FIELDS)
    want = gc.numpy_sums(profmod, prm, holed, holed, n_bins, gc.bands(prm), gc.gradients(profmod, prm, holed, holed, False), vmax=vmax)
    assert np.array_equal(want[0]["skipped"], want_skipped)
    gc.assert_sums_match(got, want, gc.quantisation(want, _scales(profmod, prm, parts, vmax)), "a hole around one particle")


# 9 ---------------------------------------------------------------------------------------------------------------
def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.grad_stats_enable(every=1)
        on = profiled_launches(ctx, 20)
        ctx.grad_stats_disable()
        off = profiled_launches(ctx, 20)
    assert all("k_grad_stats" not in d for d in (never, never2, off))
    assert on.pop("k_grad_stats") == 20
    assert on == never and off == never2
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # behind the other six, one launch each
        _six_on(ctx, prm)
        ctx.grad_stats_enable(every=4)
        seven = profiled_launches(ctx, 20)
    kernels = ("k_flow_stats", "k_step_history", "k_field_map", "k_point_probes", "k_profile_series", "k_pair_dist", "k_grad_stats")
    assert [seven.pop(k) for k in kernels] == [20] * 7 and seven == never   # (gated out, the launch skips itself)


# 10 --------------------------------------------------------------------------------------------------------------
def test_driver_run_and_its_figures(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.1, output_interval=0.05)
    res = driver.run(prm, gradients_from=0.05, gradients_every=2)
    gs = res.grad_stats
    assert len(gs) == 2 and all(len(b["count"]) == 20 for b in gs)       # the whole channel and the mid-channel band
    assert 0 < gs[0]["n_samples"] <= res.steps // 2 and gs[0]["t_first"] >= 0.05 and gs[0]["t_last"] <= res.t
    assert gs[0]["count"].sum() + gs[0]["skipped"].sum() <= gs[0]["n_samples"] * res.n_fluid and gs[0]["count"].sum() > gs[1]["count"].sum() > 0
    fig = driver.grad_figures(prm, gs)
    print(f"driver.run: {gs[0]['n_samples']} samples, L2_shear {fig['L2_shear']:.4f} / {fig['L2_shear_all']:.4f}, tau_wall "
          f"{fig['tau_wall_bottom']:.4f} {fig['tau_wall_top']:.4f} target {fig['tau_target']:.4f}, div_rms {fig['div_rms']:.3e}")
    assert np.array_equal(fig["shear"], gs[0]["gxy_mean"], equal_nan=True) and np.isfinite(fig["div_rms"]) and np.isfinite(fig["L2_shear"])
    assert driver.run(prm).grad_stats is None
