"""-m gpu: device-side point probes (include/sphx.h section 2h) -- the flow at fixed points, one record per sampled step, by
k_point_probes (one wave per probe) inside the step loop.  Checked against profile.shepard_points (the same definition in
numpy) of the downloaded state on every small case and point set, with and without moving walls, against the field map on
map nodes, against sampling between steps from the host, for gating and the record buffer, for leaving the physics, the
launches and the other samplers untouched, for repeatability, for its error identifiers, through driver.run and through
the MATLAB context gateway.

The bound of the comparisons with numpy (probe_cases.BOUND): a probe sums up to about 150 non-negative weights, each product
rounded to 1.1e-16, then divides once -- about 1e-13 of the largest |value| of a column; the tests allow 1e-12."""
import ctypes as C

import numpy as np
import pytest

import mex_mock
import probe_cases as pc
from field_map_cases import void_case
from helpers import HISTORY_FIELDS, STATS_FIELDS, check_kernel_form, err_id, gateway_cfg, make_case, make_variant, profiled_launches

pytestmark = pytest.mark.gpu
SMALL = ("dp05_auto", "dp025_walk", "dp05_dynamic", "dp025_dual", "two_cols", "one_col", "dp01_multi")


def _run_of(prm, parts, grid, state, point):
    """fluid particles in the three cell columns' rows around `point`'s cell, by the positions `state` was binned at"""
    ncx, ncy, csx, csy, y_min = grid
    nf = parts["n_fluid"]
    cx = np.minimum((state["pos"][:nf, 0] / csx).astype(int), ncx - 1)
    cy = np.minimum(((state["pos"][:nf, 1] - y_min) / csy).astype(int), ncy - 1)
    px, py = min(int(point[0] / csx), ncx - 1), min(int((point[1] - y_min) / csy), ncy - 1)
    return max(int(np.count_nonzero((cx == c % ncx) & (np.abs(cy - py) <= 1))) for c in (px - 1, px, px + 1))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_sample_now_matches_numpy(cfgmod, geom, capi, profmod, name):
    prm, parts, kw = pc.case(make_variant, cfgmod, geom, name)
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        check_kernel_form(ctx, name)
        ctx.advance(1e9, max_steps=7)
        d = ctx.download(fields=("pos", "vel"))
        st = ctx.sync()
        assert st["step"] == 7
        grid = pc.cell_geometry(prm, parts, ctx)
        sets = pc.point_sets(prm, grid, d["pos"][:parts["n_fluid"]])
        assert [len(p) for p in sets.values()] == [1, pc.WAVES - 1, pc.WAVES, pc.WAVES + 1, 300]
        for label, pts in sets.items():
            for walls in (False, True):
                ctx.probes_enable(pts, every=10 ** 9, with_walls=walls)
                ctx.probes_sample()
                got = ctx.probes()
                what = f"{name} P={label} walls={walls}"
                assert got["step"].tolist() == [st["step"]] and got["t"].tolist() == [st["t"]] and got["n_dropped"] == 0, what
                want = pc.numpy_probes(profmod, prm, parts, d, pts, with_walls=walls)
                assert np.array_equal(got["points"], want["points"]), what
                assert np.all((got["points"][:, 0] >= 0.0) & (got["points"][:, 0] < prm.DL)), what
                pc.assert_values_match(got, want, what, row=0)
                if walls and label == "300":   # the wall rows did enter: on the wall lines the weight is a full neighbourhood's
                    on_wall = (pts[:, 1] == 0.0) | (pts[:, 1] == prm.DH)
                    assert on_wall.sum() >= 5 and np.all(got["weight"][0][on_wall] > 0.8), what


def test_void_is_no_value(cfgmod, geom, capi, profmod):
    prm, parts = void_case(cfgmod, geom)
    pts = np.array([(0.5 * prm.DL, 0.5 * prm.DH), (0.25 * prm.DL, 0.5 * prm.DH), (0.5 * prm.DL + 0.5 * prm.h, 0.5 * prm.DH),
                    (0.5 * prm.DL, 0.5 * prm.DH - 0.5 * prm.h)])
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.probes_enable(pts)
        ctx.probes_sample()                                   # no step taken: the state as uploaded
        d = ctx.download(fields=("pos", "vel"))
        got = ctx.probes()
    want = pc.numpy_probes(profmod, prm, parts, d, pts)
    void = np.isnan(want["u_x"])
    assert void.tolist() == [True, False, True, True]
    pc.assert_values_match(got, want, "void", row=0)
    assert np.all(got["weight"][0][void] == 0.0) and np.all(got["rho"][0][void] == 0.0)
    assert np.all(np.isnan(got["u_x"][0][void])) and np.all(np.isnan(got["u_y"][0][void]))


def test_a_run_longer_than_a_wave(cfgmod, geom, capi, profmod):
    """A lane takes a second candidate of a column only where the column's run of three cells holds more than 64 particles.  On
    the one-column case (dp 0.1, DL 0.4: a column of 0.4 x 3 * 0.26 holds about 31) it never does; a skin of 2 h makes the
    cells 5.2 dp wide and the runs about 80 long."""
    prm, parts, kw = pc.case(make_variant, cfgmod, geom, "dp05_wide_skin")
    pts = np.concatenate([pc.random_points(prm, 40, 12), [(0.0, 0.5 * prm.DH), (prm.DL, 0.0)]])
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        grid = pc.cell_geometry(prm, parts, ctx)
        longest = max(_run_of(prm, parts, grid, parts, p) for p in pts[:40])
        assert longest > 64, longest
        for steps in (0, 7):
            if steps:
                ctx.advance(1e9, max_steps=steps)
            d = ctx.download(fields=("pos", "vel"))
            for walls in (False, True):
                ctx.probes_enable(pts, with_walls=walls)
                ctx.probes_sample()
                pc.assert_values_match(ctx.probes(), pc.numpy_probes(profmod, prm, parts, d, pts, with_walls=walls),
                                       f"wide skin after {steps} steps walls={walls}", row=0)
    prm, parts, kw = pc.case(make_variant, cfgmod, geom, "one_col")
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        print("one_col: longest run", _run_of(prm, parts, pc.cell_geometry(prm, parts, ctx), parts, (0.2, 0.5)))


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "one_col"])
def test_agrees_with_the_field_map_on_its_nodes(cfgmod, geom, capi, profmod, name):
    prm, parts, kw = pc.case(make_variant, cfgmod, geom, name)
    nx, ny = capi.field_map_shape(prm)
    rng = np.random.default_rng(3)
    nodes = np.unique(np.concatenate([np.arange(ny), (nx - 1) * ny + np.arange(ny), rng.choice(nx * ny, size=min(200, nx * ny), replace=False)]))
    xs, ys = profmod.field_map_nodes(prm.DL, prm.DH, nx, ny)
    pts = np.column_stack([xs[nodes // ny], ys[nodes % ny]])
    for walls in (False, True):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.field_map_enable(every=10 ** 9, with_walls=walls)
            ctx.probes_enable(pts, every=10 ** 9, with_walls=walls)
            ctx.advance(1e9, max_steps=7)
            ctx.probes_sample()
            ctx.field_map_sample()
            got, fm = ctx.probes(), ctx.field_map_sums()
        assert fm["n_samples"] == 1 and len(got["step"]) == 1
        want = {k: fm[p].T.ravel()[nodes] for k, p in (("weight", "sum_w"), ("u_x", "sum_ux"), ("u_y", "sum_uy"))}
        assert np.all(fm["count"].T.ravel()[nodes] == 1)
        pc.assert_values_match(dict(got, rho=got["rho"] * 0), dict(want, rho=np.zeros(len(pts))), f"{name} walls={walls}: probes vs map", row=0)


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk"])
@pytest.mark.parametrize("P", ["one", "300"])
def test_in_loop_equals_sampling_between_steps(cfgmod, geom, capi, name, P):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, name)
    N = 12
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        pts = pc.point_sets(prm, pc.cell_geometry(prm, parts, ctx), parts["pos"][:parts["n_fluid"]])[P]
    runs, forced = {}, {}
    for how in ("replayed", "eager", "between"):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.probes_enable(pts, every=10 ** 9 if how == "between" else 1, with_walls=True)
            if how == "replayed":
                assert ctx.advance(1e9, max_steps=N)["step"] == N
                assert ctx.graph_stats()["slots_replayed"] == N
            else:
                for _ in range(N):
                    ctx.advance(1e9, max_steps=1)
                    if how == "between":
                        ctx.probes_sample()
                assert ctx.graph_stats()["slots_eager"] == N
            forced[how] = ctx.grid_policy()["forced_rebuilds"]
            runs[how] = ctx.probes()
    assert runs["replayed"]["step"].tolist() == list(range(1, N + 1)) and np.all(np.diff(runs["replayed"]["t"]) > 0)
    pc.assert_series_identical(runs["replayed"], runs["eager"], f"{name} P={P}: replayed vs eager")
    # (a stop on the drift bound changes the re-binning phase, and with it the order a lane sums its candidates in)
    same = pc.assert_series_identical if forced["replayed"] == 0 and forced["between"] == 0 else pc.assert_series_close
    same(runs["replayed"], runs["between"], f"{name} P={P}: in-loop vs between steps")


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_gating_every_and_t_from(cfgmod, geom, capi, name):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, name)
    N, every = 26, 3
    pts = pc.random_points(prm, pc.WAVES + 1, 6)
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        statuses = [ctx.advance(1e9, max_steps=1) for _ in range(N)]
    t_from = statuses[4]["t"]                                  # t after step 5
    want = [s for s in statuses if s["step"] % every == 0 and s["t"] >= t_from]
    assert [s["step"] for s in want] == list(range(6, N + 1, 3))
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        ctx.probes_enable(pts, every=every, t_from=t_from)
        ctx.history_enable(every=every, t_from=t_from)
        ctx.advance(1e9, max_steps=N)
        got, hist = ctx.probes(), ctx.history()
    assert got["step"].tolist() == [s["step"] for s in want] and got["t"].tolist() == [s["t"] for s in want]
    assert np.array_equal(got["step"], hist["step"]) and np.array_equal(got["t"], hist["t"]) and got["n_dropped"] == 0
    assert got["u_x"].shape == (len(want), len(pts)) and not np.any(np.isnan(got["u_x"]))


@pytest.mark.parametrize("P", [1, 40])
def test_full_buffer_drops_and_drain_resumes(cfgmod, geom, capi, P):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, "dp05_auto")
    pts = pc.random_points(prm, P, 7)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.probes_enable(pts, every=1, capacity=64)
        ctx.advance(1e9, max_steps=7)
        whole = ctx.probes()
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.probes_enable(pts, every=1, capacity=3)
        st = ctx.advance(1e9, max_steps=7)
        full = ctx.probes()
        again = ctx.probes()                                   # reading without drain changes nothing
        drained = ctx.probes(drain=True)
        empty = ctx.probes()
        st2 = ctx.advance(1e9, max_steps=2)
        ctx.probes_sample()                                    # ungated: the state of the last step once more
        resumed = ctx.probes()
    assert st["step"] == 7 and full["step"].tolist() == [1, 2, 3] and full["n_dropped"] == 4
    for k in pc.SERIES:
        assert np.array_equal(full[k], whole[k][:3]), k        # the first three rows intact
    pc.assert_series_identical(full, again, "read twice")
    pc.assert_series_identical(full, drained, "read with drain")
    assert len(empty["step"]) == 0 and empty["n_dropped"] == 0 and empty["u_x"].shape == (0, P)
    assert resumed["step"].tolist() == [8, 9, 9] and resumed["n_dropped"] == 0 and resumed["t"][-1] == st2["t"]
    for k in pc.FIELDS:
        assert np.array_equal(resumed[k][1], resumed[k][2]), k


# 5 ---------------------------------------------------------------------------------------------------------------
def _all_on(ctx, pts, which=("probes", "stats", "history", "field")):
    if "stats" in which:
        ctx.flow_stats_enable(every=1)
    if "history" in which:
        ctx.history_enable(every=1, capacity=64)
    if "field" in which:
        ctx.field_map_enable(nx=31, ny=17, every=1, with_walls=True)
    if "probes" in which:
        ctx.probes_enable(pts, every=1, with_walls=True)


def _read_all(ctx, which):
    out = {}
    if "stats" in which:
        out["stats"] = ctx.flow_stats_sums(0)
    if "history" in which:
        out["history"] = ctx.history()
    if "field" in which:
        out["field"] = ctx.field_map_sums()
    if "probes" in which:
        out["probes"] = ctx.probes()
    return out


@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp05_dynamic"])
def test_no_feedback_on_the_physics_or_the_other_samplers(cfgmod, geom, capi, name):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, name)
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        pts = pc.point_sets(prm, pc.cell_geometry(prm, parts, ctx), parts["pos"][:parts["n_fluid"]])["300"]
    outs, reads = {}, {}
    for which in ((), ("probes",), ("stats",), ("history",), ("field",), ("probes", "stats", "history", "field")):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            _all_on(ctx, pts, which)
            st = ctx.advance(1e9, max_steps=20)
            outs[which] = (st, ctx.download(fields=("pos", "vel", "drho_dt")))
            reads[which] = _read_all(ctx, which)
    for which, (st, d) in outs.items():
        assert st == outs[()][0], which
        for k in ("pos", "vel", "drho_dt"):
            assert np.array_equal(d[k], outs[()][1][k]), (which, k)
    both = reads[("probes", "stats", "history", "field")]
    assert len(both["probes"]["step"]) == 20 == both["stats"]["n_samples"] == both["field"]["n_samples"] == len(both["history"]["t"])
    pc.assert_series_identical(reads[("probes",)]["probes"], both["probes"], f"{name}: probes alone vs all four")
    for k in STATS_FIELDS:
        assert np.array_equal(reads[("stats",)]["stats"][k], both["stats"][k]), k
    for k in HISTORY_FIELDS:
        assert np.array_equal(reads[("history",)]["history"][k], both["history"][k]), k
    for k in ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2"):
        assert np.array_equal(reads[("field",)]["field"][k], both["field"][k]), k


def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, "dp05_auto")
    pts = pc.random_points(prm, 40, 8)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.probes_enable(pts, every=1)
        on = profiled_launches(ctx, 20)
        ctx.probes_disable()
        off = profiled_launches(ctx, 20)
    assert "k_point_probes" not in never and "k_point_probes" not in never2 and "k_point_probes" not in off
    assert on.pop("k_point_probes") == 20
    assert on == never and off == never2
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:  # behind the other three, one launch each
        _all_on(ctx, pts)
        four = profiled_launches(ctx, 20)
    assert [four.pop(k) for k in ("k_flow_stats", "k_step_history", "k_field_map", "k_point_probes")] == [20] * 4 and four == never


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, "dp05_auto")
    pts = pc.random_points(prm, 40, 8)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.probes_enable(pts, every=1, capacity=100)
        ctx.advance(1e9, max_steps=64)
        assert ctx.probes()["step"].tolist() == list(range(65, 129))
        ctx.probes_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.probes()
        assert e.value.identifier == "SPHX:Probe:disabled"
        ctx.probes_enable(pts[:3], every=2)
        got = ctx.probes()
        assert len(got["step"]) == 0 and got["u_x"].shape == (0, 3) and got["n_dropped"] == 0
        ctx.prepare_steps(24)
        g0 = ctx.graph_stats()["graphs_captured"]
        st = ctx.advance(1e9, max_steps=24)
        assert ctx.graph_stats()["graphs_captured"] == g0
        got = ctx.probes()
        assert got["step"].tolist() == list(range(194, 217, 2)) and got["t"][-1] == st["t"]


@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp01_multi"])
def test_repeatable(cfgmod, geom, capi, name):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, name)
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        pts = pc.point_sets(prm, pc.cell_geometry(prm, parts, ctx), parts["pos"][:parts["n_fluid"]])["300"]
    runs = []
    for _ in range(2):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.probes_enable(pts, every=1, with_walls=True)
            ctx.advance(1e9, max_steps=20)
            runs.append(ctx.probes())
    assert len(runs[0]["step"]) == 20
    pc.assert_series_identical(runs[0], runs[1], name)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, kw = pc.case(make_case, cfgmod, geom, "dp05_auto")
    nothing = (None, None, None, None, None, 0)
    good = np.array([[0.5, 0.5], [1.0, 0.25]])

    def config(points=good, **kw):
        pts = None if points is None else np.ascontiguousarray(points, dtype=np.float64)
        c = capi.SphxProbesConfig(n_points=0 if pts is None else len(pts), every=1, capacity=16, with_walls=0, t_from=0.0,
                                  points=capi.ptr(pts))
        for k, v in kw.items():
            setattr(c, k, v)
        return c, pts

    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        h = ctx._h
        assert err_id(capi, L.sphx_ctx_probes_read, h, 0, *nothing) == ("SPHX:Probe:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_ctx_probes_sample, h) == ("SPHX:Probe:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_probes_disable(h) == capi.SPHX_OK       # a no-op when off
        with pytest.raises(capi.SphxError) as e:
            ctx.probes()
        assert e.value.identifier == "SPHX:Probe:disabled"
        ctx.probes_enable(good, every=1, capacity=16)
        ctx.advance(1e9, max_steps=5)
        before = ctx.probes()
        assert len(before["step"]) == 5
        nan, inf = float("nan"), float("inf")
        refused = [dict(points=None, n_points=2), dict(n_points=0), dict(n_points=-1), dict(n_points=4097),
                   dict(points=[[nan, 0.5]]), dict(points=[[0.5, inf]]), dict(points=[[-inf, 0.5]]), dict(points=[[0.5, -1e-9]]),
                   dict(points=[[0.5, prm.DH * (1 + 1e-12)]]), dict(every=0), dict(every=-1), dict(capacity=0), dict(capacity=-5),
                   dict(capacity=(1 << 24) + 1), dict(t_from=nan), dict(t_from=inf), dict(with_walls=2), dict(with_walls=-1)]
        for bad in refused:
            c2, keep = config(**bad)
            assert err_id(capi, L.sphx_ctx_probes_enable, h, C.byref(c2)) == ("SPHX:Probe:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_probes_enable, h, None) == ("SPHX:Probe:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.probes_enable(good, every=0)
        assert e.value.identifier == "SPHX:Probe:config"
        pc.assert_series_identical(ctx.probes(), before, "a refused enable leaves the records as they were")
        ctx.advance(1e9, max_steps=2)
        assert ctx.probes()["step"].tolist() == list(range(1, 8))         # ... and the sampler running
        n, npts = C.c_int(0), C.c_int(0)
        assert L.sphx_ctx_probes_read(h, 0, None, None, C.byref(npts), C.byref(n), None, 0) == capi.SPHX_OK
        assert (npts.value, n.value) == (2, 7)
        times, values = np.zeros((7, 2)), np.zeros((7, 2, 4))
        assert err_id(capi, L.sphx_ctx_probes_read, h, 6, capi.ptr(times), None, None, None, None, 0)[0] == "SPHX:Probe:capacity"
        assert err_id(capi, L.sphx_ctx_probes_read, h, 6, None, capi.ptr(values), None, None, None, 1)[0] == "SPHX:Probe:capacity"
        assert np.all(times == 0) and np.all(values == 0)
        assert L.sphx_ctx_probes_read(h, 7, capi.ptr(times), capi.ptr(values), None, None, None, 0) == capi.SPHX_OK
        assert times[:, 0].tolist() == list(range(1, 8)) and np.array_equal(values[:, :, 1], ctx.probes()["u_x"])   # nothing was drained
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg, keep = config()
        for fn, args in ((L.sphx_ctx_probes_enable, (C.byref(cfg),)), (L.sphx_ctx_probes_disable, ()), (L.sphx_ctx_probes_sample, ()),
                         (L.sphx_ctx_probes_read, (0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:Probe:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_driver_fills_probes(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.02, output_interval=0.01)
    pts = [(0.0, 0.5), (1.5, 0.5), (prm.DL, 0.1), (2.0, 0.0)]
    every = 3
    res = driver.run(prm, probe_points=pts, probe_every=every, probe_walls=True)
    p = res.probes
    assert res.steps > 2 * every and len(p["step"]) == res.steps // every and p["n_dropped"] == 0
    assert p["step"].tolist() == list(range(every, res.steps + 1, every)) and np.all(np.diff(p["t"]) > 0) and p["t"][-1] <= res.t
    assert p["u_x"].shape == (len(p["step"]), 4) and np.array_equal(p["points"][:, 0], [0.0, 1.5, 0.0, 2.0])
    assert np.all(p["weight"] > 0.8) and np.all(p["rho"][:, :2] > 0.9 * prm.rho0)
    fig = driver.probe_figures(prm, p)
    assert fig["n_records"] == len(p["step"]) and np.all(np.isfinite(fig["u_x_mean"])) and np.all(np.isfinite(fig["f_peak_uy"]))
    assert driver.run(prm).probes is None
    need = int(np.searchsorted(p["t"], 0.01 + 1e-12))            # the records of the first output interval
    assert need > 2
    with pytest.raises(RuntimeError, match=rf"probe_capacity >= {need} \(it is 2\)"):
        driver.run(prm, probe_points=pts, probe_every=every, probe_capacity=2)


def test_matlab_gateway_probe_commands(cfgmod, geom, capi):
    prm, parts, kw = pc.case(make_case, cfgmod, geom, "dp05_auto")
    pts = np.asfortranarray(np.concatenate([pc.random_points(prm, 5, 9), [(prm.DL, 0.5), (-0.5, 1.0)]]))
    gw = mex_mock.Gateway("sphx_ctx_mex.c")
    nf, nt = parts["n_fluid"], parts["n_total"]
    state = (parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"])
    (h,) = gw(1, "create", gateway_cfg(prm, 1e9), nf, nt, *state, 0.0, 0)
    try:
        with pytest.raises(mex_mock.MexError) as e:
            gw(7, "probe_read", h, 0)
        assert e.value.identifier == "SPHX:Probe:disabled"
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "probe_enable", h, np.zeros((3, 3), order="F"), 1, 16, 0.0, 0)
        assert e.value.identifier == "SPHX:Probe:config"
        gw(0, "probe_enable", h, pts, 2, 64, 0.0, 1)
        gw(1, "advance", h, 1e9, 30)
        gw(0, "probe_sample", h)
        got = gw(7, "probe_read", h, 1)
        gw(0, "probe_sample", h)                               # the drained buffer starts again
        after = gw(7, "probe_read", h, 0)
        gw(0, "probe_disable", h)
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "probe_sample", h)
        assert e.value.identifier == "SPHX:Probe:disabled"
    finally:
        gw(0, "destroy", h)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.probes_enable(pts, every=2, capacity=64, with_walls=True)
        ctx.advance(1e9, max_steps=30)
        ctx.probes_sample()
        want = ctx.probes()
    assert len(want["step"]) == 16
    assert np.array_equal(np.ravel(got[0]), want["step"]) and np.array_equal(np.ravel(got[1]), want["t"])
    for k, f in enumerate(pc.FIELDS):
        assert got[2 + k].shape == (16, 7) and np.array_equal(got[2 + k], want[f]), f
    assert got[6] == 0 and (after[0], after[1]) == (30.0, want["t"][-1]) and after[6] == 0
    for k, f in enumerate(pc.FIELDS):
        assert after[2 + k].shape == (1, 7) and np.array_equal(after[2 + k][0], want[f][-1]), f
