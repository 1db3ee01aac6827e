"""-m gpu: the device-side pair statistics (include/sphx.h section 2l) -- the pair-distance histogram of the fluid particles,
counted by k_pair_dist inside the step loop.  Integer work: every comparison is np.array_equal, r2_min bit for bit.  Checked
against profile.pair_histogram (numpy) of download() over bins, ranges, margins, walls and bands on every form of the step, on
the lattice's known table, on hand-placed pairs exactly on bin edges and on a clump; in the loop against sampling between single
steps, for its gate, for independence of the layout, for leaving the physics, the launches and the other samplers untouched,
for its limits and error identifiers, through driver.run and through the MATLAB context gateway."""
import ctypes as C

import numpy as np
import pytest

import mex_mock
import pair_dist_cases as pc
import probe_cases
from helpers import HISTORY_FIELDS, STATS_FIELDS, check_kernel_form, err_id, gateway_cfg, make_case, profiled_launches

pytestmark = pytest.mark.gpu

NEVER = 10 ** 9  # an `every` no test reaches: the sampler is on and only samples when asked


def _ctx(capi, cfgmod, geom, name, **more):
    prm, parts, kw = probe_cases.case(make_case, cfgmod, geom, name)
    return prm, parts, capi.Context.from_parts(prm, parts, t_end=1e9, **dict(kw, **more))


def _moved(parts, rows, where):
    pos = parts["pos"].copy(order="F")
    pos[list(rows)] = where
    return dict(parts, pos=pos)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.CASES))
def test_sample_now_matches_numpy(cfgmod, geom, capi, profmod, name):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    xbands = pc.bands(prm)
    with ctx:
        check_kernel_form(ctx, name)
        st = ctx.advance(1e9, max_steps=7)
        pos = ctx.download(fields=("pos",))["pos"]
        sep = pc.separations(profmod, prm, parts, pos)
        for n_bins, r_max, y_margin, walls in pc.settings(prm):
            what = f"{name}: n_bins {n_bins} r_max {r_max:.4f} y_margin {y_margin:.4f} walls {walls}"
            ctx.pair_dist_enable(n_bins=n_bins, every=NEVER, r_max=r_max, y_margin=y_margin, with_walls=walls, bands=xbands)
            ctx.pair_dist_sample()
            got = ctx.pair_dist_sums()
            want = pc.numpy_sums(profmod, prm, parts, pos, n_bins, r_max, y_margin, walls, xbands, sep)
            pc.assert_counts_equal(got, want, what)
            assert all(g["n_samples"] == 1 and g["t_first"] == g["t_last"] == st["t"] for g in got), what
            # (a centre 2h from both walls has no wall particle within 2h)
            assert got[0]["ff"].sum() > 0 and (got[0]["fw"].sum() > 0) == (walls and y_margin == 0.0), what
            assert got[0]["centres"] >= got[1]["centres"] > 0 and got[2]["centres"] > 0, what
    assert st["step"] == 7


def test_r_max_zero_means_two_h(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.pair_dist_enable(every=NEVER)
        ctx.pair_dist_sample()
        a = ctx.pair_dist_sums()
        ctx.pair_dist_enable(every=NEVER, r_max=2.0 * prm.h)
        ctx.pair_dist_sample()
        b = ctx.pair_dist_sums()
    pc.assert_counts_equal(a, b, "r_max = 0 against 2h", head=True)
    assert a[0]["r_edges"][-1] == 2.0 * prm.h and len(a) == 1 and len(a[0]["ff"]) == 64


# 2 ---------------------------------------------------------------------------------------------------------------
def test_lattice_table(cfgmod, geom, capi):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.0, seed=11, developed=True)
    assert (parts["n_fluid"], parts["n_total"] - parts["n_fluid"]) == (1200, 480)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.pair_dist_enable(n_bins=64, every=NEVER, with_walls=True)
        ctx.pair_dist_sample()
        (whole,) = ctx.pair_dist_sums()
        ctx.pair_dist_enable(n_bins=64, every=NEVER, y_margin=2.0 * prm.h)
        ctx.pair_dist_sample()
        bulk = ctx.pair_dist(0)
    want = np.zeros(64, dtype=np.int64)
    for k, v in pc.LATTICE_FF.items():
        want[k] = v
    assert np.array_equal(whole["ff"], want) and whole["ff"].sum() == 22680 and whole["centres"] == 1200
    assert whole["fw"].sum() == pc.LATTICE_FW_TOTAL
    assert (bulk["centres"], bulk["n_neigh"]) == pc.LATTICE_BULK
    assert abs(whole["r_min"] / prm.dp - 1.0) <= 1e-14 and whole["r2_min"] == bulk["r2_min"]


def _with_edge_pairs(parts):
    nf = parts["n_fluid"]
    pairs = pc.edge_pairs()
    rows = [nf // 2 + 3 * i for i in range(2 * len(pairs))]   # any fluid slots: the sums do not depend on them
    return _moved(parts, rows, [p for ab in pairs for p in ab]), rows


def test_pairs_exactly_on_bin_edges(cfgmod, geom, capi, profmod):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=11, developed=True)
    assert pc.EDGE_R_MAX <= 2.0 * prm.h
    placed, rows = _with_edge_pairs(parts)
    nf = parts["n_fluid"]
    with capi.Context.from_parts(prm, placed, t_end=1e9) as ctx:
        ctx.pair_dist_enable(n_bins=pc.EDGE_BINS, every=NEVER, r_max=pc.EDGE_R_MAX, with_walls=True)
        ctx.pair_dist_sample()
        got = ctx.pair_dist_sums()
        assert np.array_equal(ctx.download(fields=("pos",))["pos"][rows], placed["pos"][rows])  # (the upload left them where they are)
    want = pc.numpy_sums(profmod, prm, placed, placed["pos"], pc.EDGE_BINS, pc.EDGE_R_MAX, 0.0, True, [])
    pc.assert_counts_equal(got, want, "pairs on bin edges")
    # what the placed pairs contribute by the rule: the placed particles alone
    alone = profmod.pair_histogram(placed["pos"][rows], prm.DL, prm.DH, pc.EDGE_R_MAX, pc.EDGE_BINS)[0]
    assert np.array_equal(alone["ff"], pc.edge_bins()) and alone["r2_min"] == 0.0
    assert got[0]["r2_min"] == 0.0 and got[0]["ff"][0] >= 2


def test_clump(cfgmod, geom, capi, profmod):
    """40 fluid particles within 0.01 dp of one point, sampled as uploaded: no step is taken."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=11, developed=True)
    rng = np.random.default_rng(5)
    rows = list(range(100, 140))
    ang, rad = rng.random(40) * 2 * np.pi, 0.01 * prm.dp * np.sqrt(rng.random(40))
    centre = np.array([1.7, 0.45])
    clumped = _moved(parts, rows, centre + np.column_stack([rad * np.cos(ang), rad * np.sin(ang)]))
    with capi.Context.from_parts(prm, clumped, t_end=1e9) as ctx:
        ctx.pair_dist_enable(n_bins=64, every=NEVER, with_walls=True, bands=pc.bands(prm))
        ctx.pair_dist_sample()
        got = ctx.pair_dist_sums()
    want = pc.numpy_sums(profmod, prm, clumped, clumped["pos"], 64, 2.0 * prm.h, 0.0, True, pc.bands(prm))
    pc.assert_counts_equal(got, want, "clump")
    assert 2.0 * 0.01 * prm.dp < got[0]["r_edges"][1]        # the clump's diameter is inside bin 0
    assert got[0]["ff"][0] >= 40 * 39 and got[0]["r_min"] < 0.02 * prm.dp


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, more", [("dp05_auto", dict(rebuild_every=4)), ("dp05_dynamic", dict())])
def test_in_loop_equals_sampling_between_single_steps(cfgmod, geom, capi, name, more):
    N = 12
    setting = dict(n_bins=64, with_walls=True)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name, **more)
    with ctx:
        ctx.pair_dist_enable(every=1, bands=pc.bands(prm), **setting)
        st = ctx.advance(1e9, max_steps=N)
        in_loop = ctx.pair_dist_sums()
        if more:
            assert ctx.grid_policy()["rebuild_every"] == 4
    assert st["step"] == N
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name, **more)
    with ctx:
        ctx.pair_dist_enable(every=NEVER, bands=pc.bands(prm), **setting)
        total = None
        for _ in range(N):
            ctx.advance(1e9, max_steps=1)
            ctx.pair_dist_sample()
            one = ctx.pair_dist_sums()
            ctx.pair_dist_reset()
            assert all(o["n_samples"] == 1 for o in one)
            total = one if total is None else pc.add_counts(total, one)
        assert all(s["n_samples"] == 0 and s["ff"].sum() == 0 and s["centres"] == 0 and s["r2_min"] == np.inf
                   for s in ctx.pair_dist_sums())  # (after the reset)
    assert all(s["n_samples"] == N for s in in_loop)
    pc.assert_counts_equal(in_loop, total, f"{name}: in-loop sums against the samples between single steps added up")


def test_gate(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    singles, times = [], []
    with ctx:
        ctx.pair_dist_enable(every=NEVER)
        for _ in range(20):
            times.append(ctx.advance(1e9, max_steps=1)["t"])
            ctx.pair_dist_sample()
            singles.append(ctx.pair_dist_sums())
            ctx.pair_dist_reset()
    t_from = 0.5 * (times[3] + times[4])  # between step 4 and step 5
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.pair_dist_enable(every=3, t_from=t_from)
        ctx.advance(1e9, max_steps=20)
        gated = ctx.pair_dist_sums()
        ctx.pair_dist_enable(every=NEVER)
        ctx.advance(1e9, max_steps=5)
        idle = ctx.pair_dist_sums()
    want_steps = [s for s in range(1, 21) if s % 3 == 0 and times[s - 1] >= t_from]
    assert want_steps == [6, 9, 12, 15, 18]
    total = singles[want_steps[0] - 1]
    for s in want_steps[1:]:
        total = pc.add_counts(total, singles[s - 1])
    pc.assert_counts_equal(gated, total, "every = 3 from t_from")
    assert (gated[0]["n_samples"], gated[0]["t_first"], gated[0]["t_last"]) == (5, times[5], times[17])
    assert idle[0]["n_samples"] == 0 and np.isnan(idle[0]["t_first"]) and idle[0]["r2_min"] == np.inf and idle[0]["ff"].sum() == 0


# 4 ---------------------------------------------------------------------------------------------------------------
LAYOUTS = [dict(), dict(lanes_per_particle=4), dict(lanes_per_particle=32), dict(rebuild_every=16, skin_h=2.0),
           dict(rebuild_every=1), dict(dynamic_rebin=1)]


def test_sums_do_not_depend_on_the_layout(cfgmod, geom, capi):
    prm, parts = make_case(cfgmod, geom, dp=0.025, DL=1.5, jitter=0.2, seed=11, developed=True)
    sums, grids = [], []
    for kw in LAYOUTS:
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.pair_dist_enable(n_bins=64, every=NEVER, with_walls=True, bands=pc.bands(prm), y_margin=prm.h)
            ctx.pair_dist_sample()
            sums.append(ctx.pair_dist_sums())
            grids.append((ctx.info()["n_cell_x"], ctx.grid_policy()["skin"], ctx.schedule()["dynamic"]))
    assert len(set(grids)) >= 3, grids   # the contexts really differ in their cells
    for kw, s in zip(LAYOUTS[1:], sums[1:]):
        pc.assert_counts_equal(s, sums[0], f"layout {kw}", head=True)


# 5 ---------------------------------------------------------------------------------------------------------------
def _others_on(ctx, prm):
    ctx.flow_stats_enable(every=1)
    ctx.history_enable(every=1, capacity=64)
    ctx.field_map_enable(nx=31, ny=17, every=1, with_walls=True)
    ctx.probes_enable([(0.3 * prm.DL, 0.5 * prm.DH), (0.0, 0.1 * prm.DH)], every=1, with_walls=True)
    ctx.profile_series_enable(every=1, bands=pc.bands(prm), capacity=64)


def _others_read(ctx):
    return dict(stats=ctx.flow_stats_sums(0), history=ctx.history(), field=ctx.field_map_sums(), probes=ctx.probes(),
                series=ctx.profile_series_sums())


@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic"])
def test_no_feedback_on_the_physics_or_the_other_samplers(cfgmod, geom, capi, name):
    runs = {}
    for pairs, others in ((False, False), (True, False), (False, True), (True, True)):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            if others:
                _others_on(ctx, prm)
            if pairs:
                ctx.pair_dist_enable(every=1, with_walls=True, bands=pc.bands(prm))
            st = ctx.advance(1e9, max_steps=20)
            runs[pairs, others] = (st, ctx.download(fields=("pos", "vel", "drho_dt")), _others_read(ctx) if others else None,
                                   ctx.pair_dist_sums() if pairs else None)
    st0, d0 = runs[False, False][:2]
    for key, (st, d, _, _) in runs.items():
        assert st == st0, key
        for k in ("pos", "vel", "drho_dt"):
            assert np.array_equal(d[k], d0[k]), (key, k)
    pc.assert_counts_equal(runs[True, False][3], runs[True, True][3], f"{name}: alone against all six", head=True)
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


def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.pair_dist_enable(every=1)
        on = profiled_launches(ctx, 20)
        ctx.pair_dist_disable()
        off = profiled_launches(ctx, 20)
    assert all("k_pair_dist" not in d for d in (never, never2, off))
    assert on.pop("k_pair_dist") == 20
    assert on == never and off == never2
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # behind the other five, one launch each
        _others_on(ctx, prm)
        ctx.pair_dist_enable(every=4)
        six = profiled_launches(ctx, 20)
    kernels = ("k_flow_stats", "k_step_history", "k_field_map", "k_point_probes", "k_profile_series", "k_pair_dist")
    assert [six.pop(k) for k in kernels] == [20] * 6 and six == never   # (gated out, the launch skips itself)


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.pair_dist_enable(every=1)
        ctx.advance(1e9, max_steps=64)
        assert ctx.pair_dist_sums()[0]["n_samples"] == 64
        ctx.pair_dist_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.pair_dist_sums()
        assert e.value.identifier == "SPHX:PairDist:disabled"
        ctx.pair_dist_enable(every=2, n_bins=7)
        ctx.advance(1e9, max_steps=24)
        got = ctx.pair_dist_sums()
        assert got[0]["n_samples"] == 12 and got[0]["ff"].shape == (7,)


def test_repeatable(cfgmod, geom, capi):
    runs = []
    for _ in range(2):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp01_multi")
        with ctx:
            ctx.pair_dist_enable(every=1, with_walls=True, bands=pc.bands(prm))
            ctx.advance(1e9, max_steps=10)
            runs.append(ctx.pair_dist_sums())
    assert runs[0][0]["n_samples"] == 10 and 0 < runs[0][0]["centres"] <= 10 * parts["n_fluid"]
    pc.assert_counts_equal(runs[0], runs[1], "two identical runs", head=True)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_limits(cfgmod, geom, capi, profmod):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    L = capi.lib()
    with ctx:
        ctx.pair_dist_enable(n_bins=1024, every=NEVER, with_walls=True, bands=pc.bands(prm))  # 3 x 2 x 1024 = 6144 counters: all of the LDS
        ctx.pair_dist_sample()
        got = ctx.pair_dist_sums()
        want = pc.numpy_sums(profmod, prm, parts, parts["pos"], 1024, 2.0 * prm.h, 0.0, True, pc.bands(prm))
        pc.assert_counts_equal(got, want, "6144 counters")
        for n_bins in (1025, 0, -1):
            cfg = capi.SphxPairDistConfig(n_bins=n_bins, every=1)
            assert err_id(capi, L.sphx_ctx_pair_dist_enable, ctx._h, C.byref(cfg)) == ("SPHX:PairDist:config", capi.SPHX_ERR_ARG)
        pc.assert_counts_equal(ctx.pair_dist_sums(), got, "a refused enable leaves the sums as they were", head=True)
        ctx.pair_dist_sample()
        assert ctx.pair_dist_sums()[0]["n_samples"] == 2  # ... and the sampler running


def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    nothing = (None,) * 8

    def config(**kw):
        c = capi.SphxPairDistConfig(n_bins=64, every=1, t_from=0.0, r_max=0.0, y_margin=0.0, with_walls=0, n_bands=0)
        for k, v in kw.items():
            if k in ("band_x", "band_hw"):
                for j, x in enumerate(v):
                    getattr(c, k)[j] = x
            else:
                setattr(c, k, v)
        return c

    with ctx:
        h = ctx._h
        for fn, args in ((L.sphx_ctx_pair_dist_read, (0, 0, *nothing)), (L.sphx_ctx_pair_dist_sample, ()), (L.sphx_ctx_pair_dist_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:PairDist:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_pair_dist_disable(h) == capi.SPHX_OK       # a no-op when off
        for call in (ctx.pair_dist, ctx.pair_dist_sums, ctx.pair_dist_sample, ctx.pair_dist_reset):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:PairDist:disabled"
        ctx.pair_dist_enable(every=1, bands=pc.bands(prm))
        ctx.advance(1e9, max_steps=5)
        before = ctx.pair_dist_sums()
        assert before[0]["n_samples"] == 5
        nan, inf = float("nan"), float("inf")
        two_h = 2.0 * prm.h
        refused = [dict(n_bins=0), dict(n_bins=-1), dict(n_bins=1025), dict(every=0), dict(every=-1), dict(t_from=nan),
                   dict(r_max=-0.01), dict(r_max=np.nextafter(two_h, 1.0)), dict(r_max=nan), dict(r_max=inf), dict(y_margin=-0.1),
                   dict(y_margin=nan), dict(with_walls=2), dict(with_walls=-1), dict(n_bands=-1), dict(n_bands=3),
                   dict(n_bands=1, band_x=[nan], band_hw=[0.1]), dict(n_bands=1, band_x=[inf], band_hw=[0.1]),
                   dict(n_bands=2, band_x=[0.5, 0.5], band_hw=[0.1, -0.1]), dict(n_bands=1, band_x=[0.5], band_hw=[inf])]
        for bad in refused:
            c2 = config(**bad)
            assert err_id(capi, L.sphx_ctx_pair_dist_enable, h, C.byref(c2)) == ("SPHX:PairDist:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_pair_dist_enable, h, None) == ("SPHX:PairDist:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.pair_dist_enable(r_max=2.5 * prm.h)
        assert e.value.identifier == "SPHX:PairDist:config"
        pc.assert_counts_equal(ctx.pair_dist_sums(), before, "a refused enable leaves the sums as they were", head=True)
        ctx.advance(1e9, max_steps=2)
        assert ctx.pair_dist_sums()[0]["n_samples"] == 7                  # ... and the sampler running
        for band in (-1, 3):
            assert err_id(capi, L.sphx_ctx_pair_dist_read, h, band, 0, *nothing) == ("SPHX:PairDist:band", capi.SPHX_ERR_ARG)
            with pytest.raises(capi.SphxError) as e:
                ctx.pair_dist(band)
            assert e.value.identifier == "SPHX:PairDist:band"
        ff, fw = np.full(64, -7, dtype=np.int64), np.full(64, -7, dtype=np.int64)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        assert err_id(capi, L.sphx_ctx_pair_dist_read, h, 0, 63, None, i64(ff), *nothing[2:])[0] == "SPHX:PairDist:capacity"
        assert err_id(capi, L.sphx_ctx_pair_dist_read, h, 0, 63, None, None, i64(fw), *nothing[3:])[0] == "SPHX:PairDist:capacity"
        assert np.all(ff == -7) and np.all(fw == -7)
        nb, cen = C.c_int(0), C.c_int64(0)
        assert L.sphx_ctx_pair_dist_read(h, 2, 0, C.byref(nb), None, None, C.byref(cen), *nothing[4:]) == capi.SPHX_OK  # no array: no capacity
        assert (nb.value, cen.value) == (64, ctx.pair_dist_sums()[2]["centres"])
        assert L.sphx_ctx_pair_dist_read(h, 0, 64, None, i64(ff), i64(fw), *nothing[3:]) == capi.SPHX_OK
        assert np.array_equal(ff, ctx.pair_dist_sums()[0]["ff"]) and np.all(fw == 0)   # (no wall histogram: zeros)
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = config()
        for fn, args in ((L.sphx_ctx_pair_dist_enable, (C.byref(cfg),)), (L.sphx_ctx_pair_dist_disable, ()), (L.sphx_ctx_pair_dist_reset, ()),
                         (L.sphx_ctx_pair_dist_sample, ()), (L.sphx_ctx_pair_dist_read, (0, 0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:PairDist:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_driver_run_and_its_figures(cfgmod, driver, profmod):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.1, output_interval=0.05)
    res = driver.run(prm, pairs_from=0.05, pairs_every=2, pairs_walls=True)
    pd = res.pair_dist
    steps = [s for s in range(2, res.steps + 1, 2)]
    assert len(pd) == 3 and all(len(b["ff"]) == 64 and b["ff"].dtype == np.int64 for b in pd)
    assert 0 < pd[0]["n_samples"] < len(steps) and pd[0]["t_first"] >= 0.05 and pd[0]["t_last"] <= res.t
    assert pd[0]["r_edges"][-1] == 2.0 * prm.h and pd[0]["fw"].sum() == 0   # (centres 2h from the walls meet no wall particle)
    assert pd[0]["centres"] >= pd[1]["centres"] > 0 and pd[2]["centres"] > 0
    fig = driver.pair_dist_figures(prm, pd)
    print(f"driver.run: {pd[0]['n_samples']} samples, figures {fig}")
    assert set(fig) == {"r_min_dp", "n_neigh", "sigma1_dp", "seam_dev"}
    assert fig["r_min_dp"] == pd[0]["r_min"] / prm.dp and fig["n_neigh"] == pd[0]["ff"].sum() / pd[0]["centres"]
    # sanity, not a measured bar: a disc of radius 2h = 2.6 dp holds pi 2.6^2 - 1 = 20.2 lattice neighbours; nothing has paired
    assert 15.0 < fig["n_neigh"] < 25.0 and 0.5 < fig["r_min_dp"] < 1.207
    assert fig["sigma1_dp"] >= 0.0 and 0.0 <= fig["seam_dev"] <= 1.0
    assert np.array_equal(pd[1]["g"], profmod.pair_dist_profiles(pd[1], prm.dp)["g"])
    assert driver.run(prm).pair_dist is None
    with pytest.raises(ValueError, match="pairs_from needs the resident engine"):
        driver.run(prm, engine="mex", pairs_from=0.0)


# 8 ---------------------------------------------------------------------------------------------------------------
def test_matlab_gateway_pairs_commands(cfgmod, geom, capi):
    prm, parts, kw = probe_cases.case(make_case, cfgmod, geom, "dp05_auto")
    xbands = np.asfortranarray(np.array(pc.bands(prm)))
    gw = mex_mock.Gateway("sphx_ctx_mex.c")
    nf, nt = parts["n_fluid"], parts["n_total"]
    state = (parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"])
    (h,) = gw(1, "create", gateway_cfg(prm, 1e9), nf, nt, *state, 0.0, 0)
    try:
        with pytest.raises(mex_mock.MexError) as e:
            gw(7, "pairs_read", h, 0)
        assert e.value.identifier == "SPHX:PairDist:disabled"
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "pairs_enable", h, 64, 1, 0.0, 0.0, 0.0, 0, np.zeros((3, 2), order="F"))
        assert e.value.identifier == "SPHX:PairDist:config"
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "pairs_enable", h, 64, 0, 0.0, 0.0, 0.0, 0, xbands)
        assert e.value.identifier == "SPHX:PairDist:config"
        gw(0, "pairs_enable", h, 32, 2, 0.0, 1.5 * prm.h, prm.h, 1, xbands)
        gw(1, "advance", h, 1e9, 30)
        gw(0, "pairs_sample", h)
        got = [gw(7, "pairs_read", h, b) for b in range(3)]
        with pytest.raises(mex_mock.MexError) as e:
            gw(7, "pairs_read", h, 3)
        assert e.value.identifier == "SPHX:PairDist:band"
        gw(0, "pairs_disable", h)
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "pairs_sample", h)
        assert e.value.identifier == "SPHX:PairDist:disabled"
    finally:
        gw(0, "destroy", h)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.pair_dist_enable(n_bins=32, every=2, r_max=1.5 * prm.h, y_margin=prm.h, with_walls=True, bands=pc.bands(prm))
        ctx.advance(1e9, max_steps=30)
        ctx.pair_dist_sample()
        want = ctx.pair_dist_sums()
    for b in range(3):
        ff, fw, centres, r2_min, ns, t0, t1 = got[b]
        assert np.size(ff) == np.size(fw) == 32 and np.asarray(ff).dtype == np.float64
        assert np.array_equal(np.ravel(ff), want[b]["ff"]) and np.array_equal(np.ravel(fw), want[b]["fw"])
        assert (centres, ns, t0, t1) == (want[b]["centres"], 16, want[b]["t_first"], want[b]["t_last"])
        assert pc.same_bits(r2_min, want[b]["r2_min"])
    assert want[0]["fw"].sum() > 0
