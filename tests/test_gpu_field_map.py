"""-m gpu: device-side velocity-field maps (include/sphx.h section 2e) -- the flow sampled on a regular grid in x and y by
k_field_map inside the step loop.  Checked against profile.shepard_field (the same definition in numpy) of the downloaded
state, with wall particles, over a void, against sampling between steps from the host, for gating, for leaving the physics
and the launches untouched, for repeatability, for its error identifiers, through driver.run and through the MATLAB
context gateway.

The bound of the comparisons with numpy: a node sums up to about 150 non-negative weights, each product rounded to
1.1e-16, then divides once -- about 1e-13 of the largest |value| of a plane; the tests allow 1e-12."""
import ctypes as C

import numpy as np
import pytest

import mex_mock
from field_map_cases import void_case
from helpers import assert_sums_identical, check_kernel_form, err_id, gateway_cfg, make_case, make_variant, profiled_launches

pytestmark = pytest.mark.gpu

# name: (dp, DL, context options, make_case options)
CASES = {
    "dp05_auto": (0.05, 3.0, dict(), dict()),                          # 1 200 particles, 4 800 nodes
    "dp025_walk": (0.025, 1.5, dict(lanes_per_particle=4), dict()),
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1), dict()),
    "dp025_dual": (0.025, 1.5, dict(lanes_per_particle=16, dual_rate=2), dict()),
    "two_cols_07": (0.1, 0.7, dict(), dict()),                         # two cell columns
    "two_cols_06": (0.1, 0.6, dict(), dict()),
    "one_col": (0.1, 0.4, dict(), dict(developed=False)),              # one column, two images within 2h
    "dp01_multi": (0.01, 3.0, dict(), dict()),                         # 30 k particles, 120 k nodes: many workgroups
    "leftward": (0.05, 3.0, dict(), dict(U_bulk=-0.666667)),           # g < 0: u_x negative at every node
}
PLANES = ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")
BOUND = 1e-12


def _case(cfgmod, geom, name, seed=11):
    dp, DL, kw, mk = CASES[name]
    prm, parts = make_case(cfgmod, geom, **dict(dict(dp=dp, DL=DL, jitter=0.2, seed=seed, developed=True), **mk))
    return prm, parts, kw


def _numpy_planes(profmod, prm, f):
    """One sample's six planes from shepard_field's sums (whole grid [ny, nx] or picked nodes)."""
    hit = f["S0"] > 0.0
    z = lambda v: np.where(hit, v, 0.0)
    return dict(count=hit.astype(np.float64), sum_w=z(f["S0"] * prm.dp ** 2), sum_ux=z(f["u_x"]), sum_uy=z(f["u_y"]),
                sum_ux2=z(f["u_x"] ** 2), sum_uy2=z(f["u_y"] ** 2))


def _assert_planes_match(got, want, what):
    assert np.array_equal(got["count"], want["count"]), what + ": count"
    for k in PLANES[1:]:
        scale = max(float(np.max(np.abs(want[k]))), 1e-300)
        err = float(np.max(np.abs(got[k] - want[k])))
        print(f"{what}: {k} off by {err / scale:.3e} of the largest |value|")
        assert err <= BOUND * scale, f"{what}: {k} off by {err / scale:.3e} of the largest |value|"


def _assert_map_identical(a, b, what):
    assert_sums_identical([a], [b], what, PLANES)


def _assert_close(a, b, what):
    assert np.array_equal(a["count"], b["count"]), what + ": count"
    for k in PLANES[1:]:
        scale = max(float(np.max(np.abs(b[k]))), 1e-300)
        assert float(np.max(np.abs(a[k] - b[k]))) <= BOUND * scale, f"{what}: {k}"
    assert (a["n_samples"], a["t_first"], a["t_last"]) == (b["n_samples"], b["t_first"], b["t_last"]), what


def _picked_nodes(nx, ny, n=2000, seed=5):
    """A seeded sample of nodes with the four corners and both end columns."""
    rng = np.random.default_rng(seed)
    ends = np.concatenate([np.arange(ny), (nx - 1) * ny + np.arange(ny)])
    rest = rng.choice(nx * ny, size=n - len(ends), replace=False)
    return np.unique(np.concatenate([ends, rest]))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_sample_now_matches_numpy(cfgmod, geom, capi, profmod, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    nf = parts["n_fluid"]
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        check_kernel_form(ctx, name)
        ctx.field_map_enable(every=10 ** 9)
        ctx.advance(1e9, max_steps=7)
        ctx.field_map_sample()
        d = ctx.download(fields=("pos", "vel"))
        st = ctx.sync()
        got = ctx.field_map_sums()
    nx, ny = capi.field_map_shape(prm)
    assert got["count"].shape == (ny, nx)
    assert got["n_samples"] == 1 and got["t_first"] == got["t_last"] == st["t"]
    assert np.all(got["count"] == got["n_samples"])          # every node has a contributor
    pos, vel = d["pos"][:nf], d["vel"][:nf]
    if name == "dp01_multi":
        nodes = _picked_nodes(nx, ny)
        f = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny, nodes=nodes)
        got = {k: got[k].T.ravel()[nodes] for k in PLANES}
    else:
        f = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny)
    print(f"{name}: min S0 dp^2 = {np.min(f['S0']) * prm.dp ** 2:.3f}")
    _assert_planes_match(got, _numpy_planes(profmod, prm, f), name)
    if name == "leftward":
        # (at least 2h from the walls: next to them a jittered particle with y < 0 carries the parabola's other sign)
        inner = (f["y"] >= 2.0 * prm.h) & (f["y"] <= prm.DH - 2.0 * prm.h)
        assert prm.gravity_g < 0 and inner.sum() >= ny - 14 and np.all(got["sum_ux"][inner] < 0) and np.all(f["u_x"][inner] < 0)


# 2 ---------------------------------------------------------------------------------------------------------------
def test_walls_enter_with_their_velocity(cfgmod, geom, capi, profmod):
    prm, parts = make_variant(cfgmod, geom, dp=0.05, DL=1.5, jitter=0.2, seed=11, developed=True)
    nf = parts["n_fluid"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.field_map_enable(every=10 ** 9, with_walls=True)
        ctx.advance(1e9, max_steps=7)
        ctx.field_map_sample()
        d = ctx.download(fields=("pos", "vel"))
        got = ctx.field_map_sums()
    nx, ny = capi.field_map_shape(prm)
    f = profmod.shepard_field(d["pos"][:nf], d["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny, wall_pos=parts["pos"][nf:],
                              wall_vel=parts["wall_vel"][nf:])
    _assert_planes_match(got, _numpy_planes(profmod, prm, f), "walls")
    fluid_only = profmod.shepard_field(d["pos"][:nf], d["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny)
    assert np.all(got["sum_w"][0] > 1.5 * fluid_only["S0"][0] * prm.dp ** 2)   # the wall rows did enter


# 3 ---------------------------------------------------------------------------------------------------------------
def test_void_nodes_are_skipped(cfgmod, geom, capi, profmod):
    prm, parts = void_case(cfgmod, geom)
    nf = parts["n_fluid"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.field_map_enable()
        ctx.field_map_sample()                               # no step taken: the state as uploaded
        d = ctx.download(fields=("pos", "vel"))
        got = ctx.field_map_sums()
        m = ctx.field_map()
    nx, ny = capi.field_map_shape(prm)
    f = profmod.shepard_field(d["pos"][:nf], d["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny)
    void = f["S0"] == 0.0
    assert void.sum() >= 5
    assert np.array_equal(got["count"] == 0.0, void)
    _assert_planes_match(got, _numpy_planes(profmod, prm, f), "void")
    for k in ("weight", "u_x", "u_y", "u_x_std", "u_y_std"):
        assert np.array_equal(np.isnan(m[k]), void), k
    assert np.array_equal(m["x"], f["x"]) and np.array_equal(m["y"], f["y"])


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp05_dynamic", "dp025_dual", "dp01_multi"])
def test_in_loop_equals_sampling_between_steps(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    N = 48
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:  # in the loop, one advance call (graph replays)
        ctx.field_map_enable(every=1)
        st = ctx.advance(1e9, max_steps=N)
        assert st["step"] == N
        rebins = ctx.schedule()["rebins"]
        forced_a = ctx.grid_policy()["forced_rebuilds"]
        in_loop = ctx.field_map_sums()
    assert rebins >= 2, f"{name}: only {rebins} re-binnings in {N} steps"
    assert in_loop["n_samples"] == N and np.all(in_loop["count"] == N)
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:  # from the host, after every single step
        ctx.field_map_enable(every=10 ** 9)
        for _ in range(N):
            ctx.advance(1e9, max_steps=1)
            ctx.field_map_sample()
        forced_b = ctx.grid_policy()["forced_rebuilds"]
        between = ctx.field_map_sums()
    # (a stop on the drift bound changes the re-binning phase, and with it the order a node sums its candidates in)
    same = _assert_map_identical if forced_a == 0 and forced_b == 0 else _assert_close
    same(in_loop, between, f"{name}: in-loop vs between steps")
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:  # in the loop, chunked calls (eager slots and short graphs)
        ctx.field_map_enable(every=1)
        for n in (1, 3, 5, 11, 28):
            ctx.advance(1e9, max_steps=n)
        forced_c = ctx.grid_policy()["forced_rebuilds"]
        chunked = ctx.field_map_sums()
    same = _assert_map_identical if forced_a == 0 and forced_c == 0 else _assert_close
    same(in_loop, chunked, f"{name}: one call vs chunked")


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_gating_every_and_t_from(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    N, every = 40, 3
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        statuses = [ctx.advance(1e9, max_steps=1) for _ in range(N)]
    t_from = 0.5 * (statuses[N // 2]["t"] + statuses[N // 2 + 1]["t"])
    want = [s for s in statuses if s["step"] % every == 0 and s["t"] >= t_from]
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        ctx.field_map_enable(every=every, t_from=t_from)
        ctx.advance(1e9, max_steps=N)
        got = ctx.field_map()
    assert got["n_samples"] == len(want) > 0
    assert got["t_first"] == want[0]["t"] and got["t_last"] == want[-1]["t"]
    assert np.all(got["count"] == len(want))


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp05_dynamic"])
def test_no_feedback_on_the_physics(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    outs = []
    for on in (False, True):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            if on:
                ctx.field_map_enable(every=1, with_walls=True)
                ctx.flow_stats_enable(every=1)
                ctx.history_enable(every=1, capacity=64)
            st = ctx.advance(1e9, max_steps=40)
            outs.append((st, ctx.download(fields=("pos", "vel", "drho_dt"))))
            if on:
                assert ctx.field_map_sums()["n_samples"] == ctx.flow_stats(0)["n_samples"] == len(ctx.history()["t"]) == 40
    assert outs[0][0] == outs[1][0]
    for k in ("pos", "vel", "drho_dt"):
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


# 7 ---------------------------------------------------------------------------------------------------------------
def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.field_map_enable(every=1)
        on = profiled_launches(ctx, 20)
        ctx.field_map_disable()
        off = profiled_launches(ctx, 20)
    assert "k_field_map" not in never and "k_field_map" not in never2 and "k_field_map" not in off
    assert on.pop("k_field_map") == 20
    assert on == never and off == never2


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.field_map_enable(every=1)
        ctx.advance(1e9, max_steps=64)
        assert ctx.field_map_sums()["n_samples"] == 64
        ctx.field_map_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.field_map()
        assert e.value.identifier == "SPHX:Field:disabled"
        ctx.field_map_enable(nx=31, ny=17, every=2)
        got = ctx.field_map_sums()
        assert got["n_samples"] == 0 and got["count"].shape == (17, 31) and np.isnan(got["t_first"]) and np.isnan(got["t_last"])
        ctx.prepare_steps(24)
        g0 = ctx.graph_stats()["graphs_captured"]
        st = ctx.advance(1e9, max_steps=24)
        assert ctx.graph_stats()["graphs_captured"] == g0
        got = ctx.field_map_sums()
        assert got["n_samples"] == 12 and got["t_last"] == st["t"] and np.all(got["count"] == 12)
        ctx.field_map_reset()
        got = ctx.field_map_sums()
        assert got["n_samples"] == 0 and all(np.all(got[k] == 0) for k in PLANES)


# 8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp01_multi"])
def test_repeatable(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    runs = []
    for _ in range(2):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.field_map_enable(every=1)
            ctx.advance(1e9, max_steps=40)
            runs.append(ctx.field_map_sums())
    _assert_map_identical(runs[0], runs[1], name)


# 9 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    nothing = (None, None, *[None] * 6, None, None, None)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        h = ctx._h
        assert err_id(capi, L.sphx_ctx_field_map_read, h, 0, *nothing) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_ctx_field_map_sample, h) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_ctx_field_map_reset, h) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_field_map_disable(h) == capi.SPHX_OK       # a no-op when off
        for bad in (dict(nx=1), dict(ny=1), dict(nx=-2), dict(ny=-1), dict(nx=1 << 13, ny=(1 << 12) + 1), dict(every=0),
                    dict(every=-1), dict(t_from=float("nan")), dict(with_walls=2), dict(with_walls=-1)):
            c2 = capi.SphxFieldMapConfig(nx=0, ny=0, every=1, with_walls=0, t_from=0.0)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert err_id(capi, L.sphx_ctx_field_map_enable, h, C.byref(c2)) == ("SPHX:Field:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_field_map_enable, h, None) == ("SPHX:Field:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.field_map_enable(every=0)
        assert e.value.identifier == "SPHX:Field:config"
        cfg = capi.SphxFieldMapConfig(nx=0, ny=0, every=1, with_walls=0, t_from=0.0)
        assert L.sphx_ctx_field_map_enable(h, C.byref(cfg)) == capi.SPHX_OK
        gx, gy = C.c_int(0), C.c_int(0)
        assert L.sphx_ctx_field_map_read(h, 0, C.byref(gx), C.byref(gy), *[None] * 6, None, None, None) == capi.SPHX_OK
        assert (gx.value, gy.value) == (120, 40)
        buf = np.zeros(4800)
        for slot in range(6):
            arrs = [capi.ptr(buf) if k == slot else None for k in range(6)]
            assert err_id(capi, L.sphx_ctx_field_map_read, h, 4799, None, None, *arrs, None, None, None)[0] == "SPHX:Field:capacity"
        assert L.sphx_ctx_field_map_read(h, 4800, None, None, capi.ptr(buf), *[None] * 5, None, None, None) == capi.SPHX_OK
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = capi.SphxFieldMapConfig(nx=0, ny=0, every=1, with_walls=0, t_from=0.0)
        for fn, args in ((L.sphx_ctx_field_map_enable, (C.byref(cfg),)), (L.sphx_ctx_field_map_disable, ()),
                         (L.sphx_ctx_field_map_reset, ()), (L.sphx_ctx_field_map_sample, ()),
                         (L.sphx_ctx_field_map_read, (0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:Field:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


# 10 --------------------------------------------------------------------------------------------------------------
def test_driver_fills_field_avg(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.02, output_interval=0.01)
    res = driver.run(prm, field_from=0.0)
    fa = res.field_avg
    assert fa["n_samples"] == res.steps > 0 and fa["t_last"] == res.t
    assert fa["u_x"].shape == (40, 120) and np.all(fa["count"] == res.steps)
    fig = driver.field_figures(prm, fa)
    assert np.isfinite(fig["L2"]) and np.isfinite(fig["x_spread"]) and 0 <= fig["ix"] < 120
    assert driver.run(prm).field_avg is None


# 11 --------------------------------------------------------------------------------------------------------------
def test_matlab_gateway_field_commands(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    gw = mex_mock.Gateway("sphx_ctx_mex.c")
    nf, nt = parts["n_fluid"], parts["n_total"]
    state = (parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"])
    (h,) = gw(1, "create", gateway_cfg(prm, 1e9), nf, nt, *state, 0.0, 0)
    try:
        with pytest.raises(mex_mock.MexError) as e:
            gw(9, "field_read", h)
        assert e.value.identifier == "SPHX:Field:disabled"
        gw(0, "field_enable", h, 0, 0, 2, 0.0, 1)
        gw(1, "advance", h, 1e9, 30)
        gw(0, "field_sample", h)
        got = gw(9, "field_read", h)
        gw(0, "field_reset", h)
        cleared = gw(9, "field_read", h)
        gw(0, "field_disable", h)
        with pytest.raises(mex_mock.MexError) as e:
            gw(0, "field_sample", h)
        assert e.value.identifier == "SPHX:Field:disabled"
    finally:
        gw(0, "destroy", h)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.field_map_enable(every=2, with_walls=True)
        ctx.advance(1e9, max_steps=30)
        ctx.field_map_sample()
        want = ctx.field_map_sums()
    for k, f in enumerate(PLANES):
        assert got[k].shape == (40, 120) and np.array_equal(got[k], want[f]), f
    assert (got[6], got[7], got[8]) == (want["n_samples"], want["t_first"], want["t_last"]) and want["n_samples"] == 16
    assert cleared[6] == 0 and np.all(cleared[0] == 0) and np.isnan(cleared[7])
