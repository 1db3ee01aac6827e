"""-m gpu: the device-side density statistics (include/sphx.h section 2r) -- the density the next step starts from, re-summed
at every fluid particle by k_dens_stats inside the step loop and binned.  The integers (count, outliers, histogram, below,
above) are compared exactly, the summed fields and the extremes within the bound of tests/dens_stats_cases.py.  Checked against
profile.dens_stats_sums (numpy) of the uploaded state on every form of the step, over the bin counts up to the LDS limit and
both histograms; against the step kernels' own density (mass / Vol of a download); on the lattice at rest; in the loop against
numpy sums of the state after every step, across scheduled and drift-forced re-binnings; for its gate (the pair statistics'),
for repeatability to the byte -- also on scrubbed pool memory --, for its limits and error identifiers, for leaving the launches,
the physics and the other eight samplers untouched, and for outliers."""
import ctypes as C

import numpy as np
import pytest

import dens_stats_cases as dc
import probe_cases
from helpers import check_kernel_form, err_id, make_case, profiled_launches

pytestmark = pytest.mark.gpu

NEVER = 10 ** 9  # an `every` no test reaches: the sampler is on and only samples when asked


def _ctx(capi, cfgmod, geom, name, **more):
    prm, parts, kw = probe_cases.case(make_case, cfgmod, geom, name)
    return prm, parts, capi.Context.from_parts(prm, parts, t_end=1e9, **dict(kw, **more))


def _all_sums(ctx, n_bands=3):
    return [ctx.dens_stats_sums(b) for b in range(n_bands)]


def _scales(profmod, parts, delta_bound=0.5):
    return profmod.dens_scales(delta_bound, parts["n_fluid"])


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_sample_now_as_uploaded_matches_numpy(cfgmod, geom, capi, profmod, name):
    """No step is taken: the state is the uploaded one, which tests/test_dens_stats_host.py shows to hold no particle within
    dc.EDGE of a histogram edge or of the bound, so every integer is compared exactly."""
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    xbands = dc.bands(prm)
    dens = dc.density(profmod, prm, parts, parts["pos"])
    sc = _scales(profmod, parts)
    with ctx:
        check_kernel_form(ctx, name)
        t0 = ctx.sync()["t"]
        for n_hist, hist_range in dc.HIST:
            for n_bins in dc.BINS:
                what = f"{name}: n_bins {n_bins} hist {n_hist} x {hist_range}"
                ctx.dens_stats_enable(n_bins=n_bins, every=NEVER, n_hist=n_hist, hist_range=hist_range, bands=xbands)
                ctx.dens_stats_sample()
                got = _all_sums(ctx)
                want = dc.numpy_sums(profmod, prm, parts, parts["pos"], n_bins, xbands, dens, n_hist=n_hist, hist_range=hist_range)
                dc.assert_sums_match(got, want, dc.quantisation(want, sc), what)
                assert all(g["n_samples"] == 1 and g["t_first"] == g["t_last"] == t0 for g in got), what
                assert got[0]["count"].sum() >= got[1]["count"].sum() > 0 and got[2]["count"].sum() > 0, what
                assert got[0]["count"].sum() == parts["n_fluid"] and got[0]["outliers"].sum() == 0, what


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in dc.CASES if n != "dp025_dual"])
def test_the_sample_is_the_step_kernels_own_density(cfgmod, geom, capi, profmod, name):
    """Pass A's density of the same state, reached by a different route: sampled as uploaded, then one step and a download, whose
    Vol = mass / rho is what pass A of that step summed from the uploaded positions.  (dp025_dual is left to the other tests: an
    outer step of the dual-rate loop ends with the Vol of its last inner step, which is not the uploaded state's.)  The walls'
    share is not among the step's outputs and comes from numpy."""
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    nf = parts["n_fluid"]
    xbands = dc.bands(prm)
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    with ctx:
        assert ctx.substeps() == 1
        ctx.dens_stats_enable(n_bins=n_bins, every=NEVER, hist_range=0.25, bands=xbands)
        ctx.dens_stats_sample()
        got = _all_sums(ctx)
        ctx.advance(1e9, max_steps=1)
        d = ctx.download(fields=("Vol",))
    rho = parts["mass"][:nf] / d["Vol"][:nf]
    delta = rho / prm.rho0 - 1.0
    near = int(dc.near_edges(delta, 64, 0.25, 0.5).sum())
    assert near <= 2, near
    _, wall = dc.density(profmod, prm, parts, parts["pos"])
    want = dc.numpy_sums(profmod, prm, parts, parts["pos"], n_bins, xbands, (rho, wall), hist_range=0.25)
    dc.assert_sums_match(got, want, dc.quantisation(want, _scales(profmod, parts)), f"{name}: against mass / Vol of the next step", loose=near)
    assert got[0]["count"].sum() == nf


# 3 ---------------------------------------------------------------------------------------------------------------
def test_lattice_at_rest(cfgmod, geom, capi, profmod):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.0, developed=False)
    nf = parts["n_fluid"]
    assert nf == 1200
    dens = dc.density(profmod, prm, parts, parts["pos"])
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        for n_hist, hist_range in dc.HIST:
            ctx.dens_stats_enable(n_bins=20, every=NEVER, n_hist=n_hist, hist_range=hist_range)
            ctx.dens_stats_sample()
            s = ctx.dens_stats_sums(0)
            assert np.all(s["count"] == nf / 20) and np.all(s["outliers"] == 0) and s["n_samples"] == 1
            assert np.all(np.abs(s["d_min"] - dc.LATTICE_DELTA) <= 1e-13) and np.all(np.abs(s["d_max"] - dc.LATTICE_DELTA) <= 1e-13)
            assert s["d_max"].max() - s["d_min"].min() <= 1e-13
            assert s["hist"][31] == nf and s["hist"].sum() == nf and (s["below"], s["above"]) == (0, 0)
            # a mean of 60 values each within 1e-13 and rounded to 2^-s_d
            assert np.all(np.abs(s["sum_d"] / s["count"] - dc.LATTICE_DELTA) <= 1e-13 + 2.0 ** -(_scales(profmod, parts)["s_d"] + 1))
    (want,) = dc.numpy_sums(profmod, prm, parts, parts["pos"], 20, [], dens)
    assert np.array_equal(s["sum_wall"] != 0.0, want["sum_wall"] != 0.0) and 0 < np.count_nonzero(s["sum_wall"]) < 20
    dc.assert_sums_match([s], [want], dc.quantisation([want], _scales(profmod, parts)), "lattice at rest",
                         bound=16 * dc.LATTICE_FP_DEVIATION)   # (sums of -5e-05 with rho's rounding error: the lattice's own figure, see dc)


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, more", [("dp05_auto", dict(rebuild_every=4)), ("dp05_dynamic", dict()), ("dp05_wide_skin", dict()),
                                        ("dp05_auto", dict(rebuild_every=8, skin_h=0.05))])   # (a skin far too thin: the drift bound)
def test_in_loop_equals_numpy_sums_of_every_step(cfgmod, geom, capi, profmod, name, more):
    N = 24
    setting = dict(n_bins=20, hist_range=0.25)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name, **more)
    xbands = dc.bands(prm)
    sc = _scales(profmod, parts)
    with ctx:   # in the loop, one advance call (graph replays)
        ctx.dens_stats_enable(every=1, bands=xbands, **setting)
        st = ctx.advance(1e9, max_steps=N)
        in_loop = _all_sums(ctx)
        rebins, forced_a = ctx.schedule()["rebins"], ctx.grid_policy()["forced_rebuilds"]
    assert st["step"] == N
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name, **more)
    total = quant = None
    statuses, loose = [], 0
    with ctx:   # step by step, with a download and numpy's sums after every step; sampled in the loop as well
        ctx.dens_stats_enable(every=1, bands=xbands, **setting)
        for _ in range(N):
            statuses.append(ctx.advance(1e9, max_steps=1))
            pos = ctx.download(fields=("pos",))["pos"]
            dens = dc.density(profmod, prm, parts, pos)
            near = int(dc.near_edges(dens[0] / prm.rho0 - 1.0, 64, 0.25, 0.5).sum())
            assert near <= 2, near     # (more than two particles on an edge in one sample: not chance)
            loose += near
            one = dc.numpy_sums(profmod, prm, parts, pos, 20, xbands, dens, hist_range=0.25)
            q = dc.quantisation(one, sc)
            total = one if total is None else dc.add_sums(profmod, total, one)
            quant = q if quant is None else dc.add_quantisation(quant, q)
        stepped = _all_sums(ctx)
        forced_b = ctx.grid_policy()["forced_rebuilds"]
    print(f"{name} {more}: {rebins} re-binnings, forced {forced_a} / {forced_b}; particles on an edge: {loose}")
    assert rebins + forced_a >= (2 if more else 1)   # (the dynamic schedule re-bins when the device decides: once in these steps)
    if "skin_h" in more:
        assert forced_a >= 1 and forced_b >= 1
    dc.assert_sums_match(stepped, total, quant, f"{name} {more}: step by step", loose=loose)
    dc.assert_sums_match(in_loop, total, quant, f"{name} {more}: one call", loose=loose)
    assert forced_a == forced_b
    for band in in_loop + stepped:
        assert (band["n_samples"], band["t_first"], band["t_last"]) == (N, statuses[0]["t"], statuses[-1]["t"])
    # both runs take the same steps from the same layouts (test_gpu_grid_skin.py): the same bits
    dc.assert_identical(in_loop, stepped, f"{name} {more}: one call against single steps")


def test_gate_is_the_pair_statistics_gate(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        times = [ctx.advance(1e9, max_steps=1)["t"] for _ in range(24)]
    t_from = 0.5 * (times[6] + times[7])   # between step 7 and step 8
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.dens_stats_enable(every=5, t_from=t_from)
        ctx.pair_dist_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=24)
        g, p = ctx.dens_stats_sums(0), ctx.pair_dist_sums()[0]
        ctx.dens_stats_enable(every=NEVER)
        ctx.advance(1e9, max_steps=5)
        idle = ctx.dens_stats_sums(0)
    assert (g["n_samples"], g["t_first"], g["t_last"]) == (p["n_samples"], p["t_first"], p["t_last"]) == (3, times[9], times[19])
    assert 0 < g["count"].sum() + g["outliers"].sum() <= 3 * parts["n_fluid"]   # (a particle outside [0, DH] is dropped)
    assert g["hist"].sum() + g["below"] + g["above"] == g["count"].sum()
    assert idle["n_samples"] == 0 and np.isnan(idle["t_first"]) and all(not np.any(idle[f]) for f in dc.COUNTS + dc.SUMMED)
    assert np.all(idle["d_min"] == np.inf) and np.all(idle["d_max"] == -np.inf) and not np.any(idle["hist"]) and (idle["below"], idle["above"]) == (0, 0)


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp01_multi"])   # one workgroup row of 19, and the 469 of 30 k particles
def test_repeatable_to_the_byte_also_on_scrubbed_memory(cfgmod, geom, capi, name):
    runs = []
    for how in ("first", "second", "scrubbed"):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            if how == "scrubbed":   # every cached free block reads 3, 3, 3, ...: a word the sampler did not write would show
                assert capi.pool_scrub(3) >= 1
            ctx.dens_stats_enable(every=1, hist_range=0.25, bands=dc.bands(prm))
            ctx.advance(1e9, max_steps=10)
            runs.append(_all_sums(ctx))
    assert runs[0][0]["n_samples"] == 10 and runs[0][0]["count"].sum() > 0 and np.any(runs[0][0]["sum_d"] != 0.0)
    assert runs[0][0]["hist"].sum() + runs[0][0]["below"] + runs[0][0]["above"] == runs[0][0]["count"].sum()
    dc.assert_identical(runs[0], runs[1], f"{name}: two identical runs")
    dc.assert_identical(runs[0], runs[2], f"{name}: on scrubbed pool memory")


# 6 ---------------------------------------------------------------------------------------------------------------
def test_limits(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    L = capi.lib()
    with ctx:
        ctx.dens_stats_enable(n_bins=311, every=NEVER, bands=dc.bands(prm))   # 3 x (8 x 311 + 66) = 7662 of 7680 words
        ctx.dens_stats_sample()
        got = _all_sums(ctx)
        assert got[0]["count"].shape == (311,) and got[0]["count"].sum() == parts["n_fluid"]
        for n_bins, n_bands, n_hist in ((952, 0, 64), (472, 1, 64), (312, 2, 64), (832, 0, 1024), (-1, 0, 64), (20, 0, 0), (20, 0, 1025)):
            cfg = capi.SphxDensStatsConfig(n_bins=n_bins, every=1, n_hist=n_hist, hist_range=0.05, delta_bound=0.5, n_bands=n_bands)
            for k in range(n_bands):
                cfg.band_x[k], cfg.band_hw[k] = 0.5, 0.1
            assert err_id(capi, L.sphx_ctx_dens_stats_enable, ctx._h, C.byref(cfg)) == ("SPHX:DensStats:config", capi.SPHX_ERR_ARG), n_bins
        dc.assert_identical(_all_sums(ctx), got, "a refused enable leaves the sums as they were")
        ctx.dens_stats_sample()
        assert ctx.dens_stats_sums(0)["n_samples"] == 2   # ... and the sampler running
        for kw in (dict(n_bins=951), dict(n_bins=831, n_hist=1024, hist_range=0.5), dict(n_bins=1, n_hist=1, hist_range=1e-3, delta_bound=1e-3)):
            ctx.dens_stats_enable(every=NEVER, **kw)
            ctx.dens_stats_sample()
            s = ctx.dens_stats_sums(0)
            assert s["count"].sum() + s["outliers"].sum() == parts["n_fluid"] and s["hist"].sum() + s["below"] + s["above"] == s["count"].sum(), kw


def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    nothing = (None,) * 9

    def config(**kw):
        c = capi.SphxDensStatsConfig(n_bins=20, every=1, t_from=0.0, n_hist=64, hist_range=0.05, delta_bound=0.5, n_bands=0)
        for k, v in kw.items():
            if k in ("band_x", "band_hw"):
                for j, x in enumerate(v):
                    getattr(c, k)[j] = x
            else:
                setattr(c, k, v)
        return c

    with ctx:
        h = ctx._h
        for fn, args in ((L.sphx_ctx_dens_stats_read, (0, 0, 0, *nothing)), (L.sphx_ctx_dens_stats_sample, ()), (L.sphx_ctx_dens_stats_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:DensStats:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_dens_stats_disable(h) == capi.SPHX_OK       # a no-op when off
        for call in (ctx.dens_stats, ctx.dens_stats_sums, ctx.dens_stats_sample, ctx.dens_stats_reset):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:DensStats:disabled"
        ctx.dens_stats_enable(every=1, bands=dc.bands(prm))
        ctx.advance(1e9, max_steps=5)
        before = _all_sums(ctx)
        assert before[0]["n_samples"] == 5
        nan, inf = float("nan"), float("inf")
        refused = [dict(n_bins=-1), dict(n_bins=952), dict(every=0), dict(every=-1), dict(t_from=nan), dict(n_hist=0), dict(n_hist=-3),
                   dict(n_hist=1025), dict(hist_range=0.0), dict(hist_range=-0.05), dict(hist_range=nan), dict(hist_range=0.50001),
                   dict(hist_range=0.2, delta_bound=0.1), dict(delta_bound=0.0), dict(delta_bound=-0.5), dict(delta_bound=nan),
                   dict(delta_bound=inf), dict(delta_bound=0.5000001), dict(n_bands=-1), dict(n_bands=3),
                   dict(n_bands=1, band_x=[nan], band_hw=[0.1]), dict(n_bands=1, band_x=[inf], band_hw=[0.1]),
                   dict(n_bands=2, band_x=[0.5, 0.5], band_hw=[0.1, -0.1]), dict(n_bands=1, band_x=[0.5], band_hw=[inf])]
        for bad in refused:
            c2 = config(**bad)
            assert err_id(capi, L.sphx_ctx_dens_stats_enable, h, C.byref(c2)) == ("SPHX:DensStats:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_dens_stats_enable, h, None) == ("SPHX:DensStats:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.dens_stats_enable(delta_bound=0.6)
        assert e.value.identifier == "SPHX:DensStats:config"
        dc.assert_identical(_all_sums(ctx), before, "a refused enable leaves the sums as they were")
        ctx.advance(1e9, max_steps=2)
        assert ctx.dens_stats_sums(0)["n_samples"] == 7                  # ... and the sampler running
        for band in (-1, 3):
            assert err_id(capi, L.sphx_ctx_dens_stats_read, h, band, 0, 0, *nothing) == ("SPHX:DensStats:band", capi.SPHX_ERR_ARG)
            with pytest.raises(capi.SphxError) as e:
                ctx.dens_stats(band)
            assert e.value.identifier == "SPHX:DensStats:band"
        sums = np.full((8, 20), -7.0)
        hist = np.full(64, -7, dtype=np.int64)
        hp = hist.ctypes.data_as(C.POINTER(C.c_int64))
        assert err_id(capi, L.sphx_ctx_dens_stats_read, h, 0, 19, 0, None, None, capi.ptr(sums), *(None,) * 6)[0] == "SPHX:DensStats:capacity"
        assert err_id(capi, L.sphx_ctx_dens_stats_read, h, 0, 0, 63, None, None, None, hp, *(None,) * 5)[0] == "SPHX:DensStats:capacity"
        assert np.all(sums == -7.0) and np.all(hist == -7)
        nb, nh, ns = C.c_int(0), C.c_int(0), C.c_int64(0)
        assert L.sphx_ctx_dens_stats_read(h, 2, 0, 0, C.byref(nb), C.byref(nh), None, None, None, None, C.byref(ns), None, None) == capi.SPHX_OK
        assert (nb.value, nh.value, ns.value) == (20, 64, 7)                # no array: no capacity
        wide = np.full((8, 25), -7.0)
        assert L.sphx_ctx_dens_stats_read(h, 1, 25, 0, *(None,) * 2, capi.ptr(wide), *(None,) * 6) == capi.SPHX_OK   # field f of bin k at f * capacity + k
        want = ctx.dens_stats_sums(1)
        for j, f in enumerate(dc.FIELDS):
            assert np.array_equal(wide[j, :20], want[f]) and np.all(wide[j, 20:] == -7.0), f
        ctx.dens_stats_reset()
        for s in _all_sums(ctx):
            assert s["n_samples"] == 0 and not np.any(s["count"]) and not np.any(s["sum_d2"]) and not np.any(s["hist"])
            assert np.all(s["d_min"] == np.inf) and np.all(s["d_max"] == -np.inf)
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = config()
        for fn, args in ((L.sphx_ctx_dens_stats_enable, (C.byref(cfg),)), (L.sphx_ctx_dens_stats_disable, ()), (L.sphx_ctx_dens_stats_reset, ()),
                         (L.sphx_ctx_dens_stats_sample, ()), (L.sphx_ctx_dens_stats_read, (0, 0, 0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:DensStats:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.dens_stats_enable(every=1)
        ctx.advance(1e9, max_steps=64)
        assert ctx.dens_stats_sums(0)["n_samples"] == 64
        ctx.dens_stats_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.dens_stats_sums(0)
        assert e.value.identifier == "SPHX:DensStats:disabled"
        ctx.dens_stats_enable(every=2, n_bins=7)
        ctx.advance(1e9, max_steps=24)
        got = ctx.dens_stats_sums(0)
        assert got["n_samples"] == 12 and got["count"].shape == (7,) and 0 < got["count"].sum() + got["outliers"].sum() <= 12 * parts["n_fluid"]


# 7 ---------------------------------------------------------------------------------------------------------------
_OTHERS = ("stats", "history", "field", "probes", "series", "pairs", "grads", "tracers")


def _other_on(ctx, prm, parts, which):
    if which == "stats":
        ctx.flow_stats_enable(every=1)
    elif which == "history":
        ctx.history_enable(every=1, capacity=64)
    elif which == "field":
        ctx.field_map_enable(nx=31, ny=17, every=1, with_walls=True)
    elif which == "probes":
        ctx.probes_enable([(0.3 * prm.DL, 0.5 * prm.DH), (0.0, 0.1 * prm.DH)], every=1, with_walls=True)
    elif which == "series":
        ctx.profile_series_enable(every=1, bands=dc.bands(prm), capacity=64)
    elif which == "pairs":
        ctx.pair_dist_enable(every=1, with_walls=True, bands=dc.bands(prm))
    elif which == "grads":
        ctx.grad_stats_enable(every=1, with_walls=True, bands=dc.bands(prm))
    elif which == "tracers":
        ctx.tracers_enable(np.arange(0, parts["n_fluid"], 7, dtype=np.int32), every=1, capacity=32)


def _other_read(ctx, which):
    if which == "stats":
        return ctx.flow_stats_sums(0)
    if which == "history":
        rec, dropped = ctx.history_records()
        return dict(records=rec, n_dropped=dropped)
    if which == "field":
        return ctx.field_map_sums()
    if which == "probes":
        return ctx.probes()
    if which == "series":
        return ctx.profile_series_sums()
    if which == "pairs":
        return {f"{b}.{k}": v for b, band in enumerate(ctx.pair_dist_sums()) for k, v in band.items()}
    if which == "grads":
        return {f"{b}.{k}": v for b in range(3) for k, v in ctx.grad_stats_sums(b).items()}
    return ctx.tracers()


def _same(a, b, what):
    n = 0
    for k, v in a.items():
        assert np.asarray(v).tobytes() == np.asarray(b[k]).tobytes(), (what, k)
        n += 1
    return n


@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic"])
def test_no_feedback_on_the_physics_or_the_other_eight_samplers(cfgmod, geom, capi, name):
    """All nine on against each alone, byte for byte -- the eight others' records and the density statistics' own -- and the
    physics with and without the samplers."""
    def run(on):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            for which in _OTHERS:
                if which in on:
                    _other_on(ctx, prm, parts, which)
            if "dens" in on:
                ctx.dens_stats_enable(every=1, hist_range=0.25, bands=dc.bands(prm))
            st = ctx.advance(1e9, max_steps=20)
            state = ctx.download(fields=("pos", "vel", "drho_dt"))
            reads = {which: _other_read(ctx, which) for which in _OTHERS if which in on}
            if "dens" in on:
                reads["dens"] = _all_sums(ctx)
        return st, state, reads

    st0, d0, _ = run(())
    st9, d9, all_on = run(_OTHERS + ("dens",))
    assert st9 == st0 and all(np.array_equal(d9[k], d0[k]) for k in ("pos", "vel", "drho_dt"))
    assert all_on["dens"][0]["n_samples"] == 20
    n = 0
    for which in _OTHERS:
        st, d, alone = run((which,))
        assert st == st0 and all(np.array_equal(d[k], d0[k]) for k in ("pos", "vel", "drho_dt")), which
        n += _same(alone[which], all_on[which], f"{name}: {which} alone against all nine")
    assert n > 60, n
    st, d, alone = run(("dens",))
    assert st == st0 and all(np.array_equal(d[k], d0[k]) for k in ("pos", "vel", "drho_dt"))
    dc.assert_identical(alone["dens"], all_on["dens"], f"{name}: alone against all nine")


# 8 ---------------------------------------------------------------------------------------------------------------
def test_outliers_are_counted_and_summed_nowhere(cfgmod, geom, capi, profmod):
    """Three fluid particles from different places within 0.2 dp of one another: each has two partners at almost no distance,
    2 W(0) dp^2 = 0.54 of rho0 on top of a full neighbourhood, and lands beyond delta_bound = 0.5.  Sampled as uploaded; how many exceed the bound is numpy's count."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=11, developed=True)
    nf = parts["n_fluid"]
    pos = parts["pos"].copy(order="F")
    first = int(np.argmin(np.hypot(pos[:nf, 0] - 1.0, pos[:nf, 1] - 0.5)))
    # (two from far away, mid-channel: the first keeps every partner it had and gains two)
    a = int(np.argmin(np.hypot(pos[:nf, 0] - 2.0, pos[:nf, 1] - 0.5)))
    b = int(np.argmin(np.hypot(pos[:nf, 0] - 2.5, pos[:nf, 1] - 0.5)))
    pos[a] = pos[first] + np.array([0.1 * prm.dp, 0.0])
    pos[b] = pos[first] + np.array([0.0, 0.1 * prm.dp])
    close = dict(parts, pos=pos)
    rho, wall = dc.density(profmod, prm, close, pos)
    delta = rho / prm.rho0 - 1.0
    out = np.abs(delta) > 0.5
    print(f"delta of the three: {delta[[first, a, b]]}; outliers {int(out.sum())}")
    assert 1 <= out.sum() <= 3 and set(np.flatnonzero(out)) <= {first, a, b} and np.all(delta[[first, a, b]] > 0.4)
    assert not dc.near_edges(delta, 64, 0.25, 0.5).any()
    n_bins = 20
    with capi.Context.from_parts(prm, close, t_end=1e9) as ctx:
        ctx.dens_stats_enable(n_bins=n_bins, every=NEVER, hist_range=0.25, bands=dc.bands(prm))
        ctx.dens_stats_sample()
        got = _all_sums(ctx)
    want = dc.numpy_sums(profmod, prm, close, pos, n_bins, dc.bands(prm), (rho, wall), hist_range=0.25)
    assert got[0]["outliers"].sum() == out.sum() == want[0]["outliers"].sum() and got[0]["count"].sum() == nf - out.sum()
    assert got[0]["hist"].sum() + got[0]["below"] + got[0]["above"] == nf - out.sum()
    assert got[0]["d_max"].max() <= 0.5 and all(np.all(np.isfinite(got[k][f])) for k in range(3) for f in dc.SUMMED)
    dc.assert_sums_match(got, want, dc.quantisation(want, _scales(profmod, parts)), "three particles on top of one another")


# 9 ---------------------------------------------------------------------------------------------------------------
def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.dens_stats_enable(every=1)
        on = profiled_launches(ctx, 20)
        ctx.dens_stats_disable()
        off = profiled_launches(ctx, 20)
    assert all("k_dens_stats" not in d for d in (never, never2, off))
    assert on.pop("k_dens_stats") == 20
    assert on == never and off == never2
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # behind the other eight, one launch each
        for which in _OTHERS:
            _other_on(ctx, prm, parts, which)
        ctx.dens_stats_enable(every=4)
        nine = profiled_launches(ctx, 20)
    kernels = ("k_flow_stats", "k_step_history", "k_field_map", "k_point_probes", "k_profile_series", "k_pair_dist", "k_grad_stats", "k_tracers",
               "k_dens_stats")
    assert [nine.pop(k) for k in kernels] == [20] * 9 and nine == never   # (gated out, the launch skips itself)


# 10 --------------------------------------------------------------------------------------------------------------
def test_driver_run_and_its_figures(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.1, output_interval=0.05)
    res = driver.run(prm, density_from=0.05, density_every=2)
    ds = res.dens_stats
    assert len(ds) == 2 and all(len(b["count"]) == 20 and len(b["hist"]) == 64 for b in ds)   # the whole channel and the mid-channel band
    assert 0 < ds[0]["n_samples"] <= res.steps // 2 and ds[0]["t_first"] >= 0.05 and ds[0]["t_last"] <= res.t
    assert ds[0]["count"].sum() + ds[0]["outliers"].sum() <= ds[0]["n_samples"] * res.n_fluid and ds[0]["count"].sum() > ds[1]["count"].sum() > 0
    for k in ("y_mid", "d_mean", "d_std", "d_min", "d_max", "p_mean", "p_std", "wall_mean", "packing"):
        assert ds[0][k].shape == (20,) and np.all(np.isfinite(ds[0][k])), k
    assert ds[0]["hist_density"].shape == ds[0]["hist_centres"].shape == (64,)
    fig = driver.density_figures(prm, ds)
    print("driver.run: " + ", ".join(f"{k} {v:.4e}" for k, v in fig.items()))
    assert set(fig) == {"delta_rms", "delta_mean", "delta_max", "outliers", "ma2", "p_spread", "wall_bias", "packing"}
    assert all(np.isfinite(v) for v in fig.values()) and fig["delta_rms"] <= fig["delta_max"] <= 0.5 and fig["outliers"] == 0
    assert driver.run(prm).dens_stats is None
