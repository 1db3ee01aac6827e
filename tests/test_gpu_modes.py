"""-m gpu: the device-side mode amplitudes (include/sphx.h section 2t) -- the count, u_x and u_y of the fluid particles projected
on the channel's modes by k_modes inside the step loop.  Checked against the numpy definition (profile.mode_sums) of the sampled
state, with the exact identities to the bit; across the particle counts at which the grid changes shape; for records that do not
depend on the particle order or the lanes per particle; in the loop across re-binnings against sampling between single steps,
with its gate, its record buffer and its lifecycle; for leaving the physics and the launches untouched; under poison-at-free;
for its error identifiers; through driver.run; and against the oracle's own trajectory of the start-up of plane Poiseuille flow."""
import ctypes as C

import numpy as np
import pytest

import mode_cases as mc
from helpers import check_kernel_form, err_id, make_case, profiled_launches

pytestmark = pytest.mark.gpu


def _ctx(capi, cfgmod, geom, name, **more):
    prm, parts, kw = mc.case(make_case, cfgmod, geom, name)
    return prm, parts, capi.Context.from_parts(prm, parts, t_end=1e9, **dict(kw, **more))


def _check(profmod, prm, rec, pos, vel, vmax, mx, ny, what):
    want = mc.numpy_modes(profmod, prm, pos, vel, mx, ny)
    mc.assert_record_matches(rec, want, profmod.mode_scales(vmax, len(pos)), len(pos), what)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modes", mc.MODES)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_sample_now_matches_numpy(cfgmod, geom, capi, profmod, name, modes):
    mx, ny = modes
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    nf = parts["n_fluid"]
    with ctx:
        check_kernel_form(ctx, name)
        ctx.modes_enable(mx=mx, ny=ny, every=10 ** 9, capacity=4)
        v0 = ctx.sync()["vmax"]
        ctx.modes_sample()                                   # the state as uploaded
        st = ctx.advance(1e9, max_steps=3)
        ctx.modes_sample()                                   # ... and what three steps left
        d = ctx.download(fields=("pos", "vel"))
        got = ctx.modes()
    assert got["n"].shape == got["ux"].shape == got["uy"].shape == (2, mx + 1, ny + 1, 4) and got["n_dropped"] == 0
    assert got["step"].tolist() == [0, 3] and got["t"].tolist() == [0.0, st["t"]]
    _check(profmod, prm, mc.record(got, 0), parts["pos"][:nf], parts["vel"][:nf], v0, mx, ny, f"{name} {modes} as uploaded")
    _check(profmod, prm, mc.record(got, 1), d["pos"][:nf], d["vel"][:nf], st["vmax"], mx, ny, f"{name} {modes} after 3 steps")


# 2 ---------------------------------------------------------------------------------------------------------------
COUNTS = (50, 63, 64, 65, mc.BLOCK - 1, mc.BLOCK, mc.BLOCK + 1, 1000, mc.CHUNK - 1, mc.CHUNK, mc.CHUNK + 1, 2400)


@pytest.mark.parametrize("modes", [(0, 0), (0, mc.RUN - 1), (1, mc.RUN), (4, 8)])
def test_particle_counts(cfgmod, geom, capi, profmod, modes):
    """The first N fluid rows of a 2 400-particle state with all of its walls (nothing is stepped): N below a wave, not a multiple
    of 64, around a workgroup's threads and around mc.CHUNK -- up to which modes (0, 0), one group, are ONE workgroup that
    finishes alone; one more particle makes two chunks with global sums and a ticket.  (0, RUN - 1): the largest ny in one
    group; (1, RUN): two groups per m, the second one mode wide."""
    mx, ny = modes
    prm, parts = make_case(cfgmod, geom, dp=0.025, DL=1.5, jitter=0.2, seed=11, developed=True)
    nf, nt = parts["n_fluid"], parts["n_total"]
    assert nf == COUNTS[-1] and mc.CHUNK + 1 < nf
    for n in COUNTS:
        rows = np.r_[0:n, nf:nt]
        sub = {k: np.asfortranarray(parts[k][rows]) for k in ("pos", "vel", "drho_dt", "mass", "wall_vel")}
        with capi.Context(prm, n, len(rows), sub["pos"], sub["vel"], sub["drho_dt"], sub["mass"], sub["wall_vel"], t_end=1e9) as ctx:
            ctx.modes_enable(mx=mx, ny=ny, every=10 ** 9, capacity=2)
            vmax = ctx.sync()["vmax"]
            ctx.modes_sample()
            ctx.modes_sample()
            got = ctx.modes()
        assert got["step"].tolist() == [0, 0]
        _check(profmod, prm, mc.record(got, 0), sub["pos"][:n], sub["vel"][:n], vmax, mx, ny, f"{modes} N = {n}")
        for f in mc.FIELDS:  # the second sample: the global sums were put back to zero
            assert got[f][0].tobytes() == got[f][1].tobytes(), (n, f)


# 3 ---------------------------------------------------------------------------------------------------------------
def test_records_do_not_depend_on_row_order_or_lanes(cfgmod, geom, capi):
    prm, parts = make_case(cfgmod, geom, dp=0.025, DL=1.5, jitter=0.2, seed=11, developed=True)
    nf, nt = parts["n_fluid"], parts["n_total"]
    perm = np.r_[np.random.default_rng(5).permutation(nf), nf:nt]
    shuffled = dict(parts, **{k: np.asfortranarray(parts[k][perm]) for k in ("pos", "vel", "drho_dt", "mass", "wall_vel")})
    runs = {}
    for what, pa, kw in (("as built", parts, {}), ("shuffled", shuffled, {}), ("16 lanes", parts, dict(lanes_per_particle=16)),
                         ("32 lanes", parts, dict(lanes_per_particle=32)), ("shuffled, 4 lanes", shuffled, dict(lanes_per_particle=4))):
        with capi.Context.from_parts(prm, pa, t_end=1e9, **kw) as ctx:
            if kw:
                assert ctx.tuning()["lanes_per_particle"] == kw["lanes_per_particle"]
            ctx.modes_enable(mx=16, ny=16, every=10 ** 9, capacity=2)
            ctx.modes_sample()
            runs[what] = ctx.modes()
    assert runs["as built"]["n"][0, 0, 0, 0] == nf and np.any(runs["as built"]["uy"] != 0.0)
    for what, got in runs.items():
        mc.assert_series_identical(got, runs["as built"], what)


# 4 ---------------------------------------------------------------------------------------------------------------
N_LOOP = 40


@pytest.fixture(scope="module")
def in_loop(cfgmod, geom, capi):
    """forty in-loop records of dp05_auto, every step; the re-binnings of the run"""
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.modes_enable(every=1, capacity=64)
        st = ctx.advance(1e9, max_steps=N_LOOP)
        rebins = ctx.schedule()["rebins"]
        got = ctx.modes()
    assert st["step"] == N_LOOP
    return got, rebins


@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_forty_in_loop_records_equal_sampling_between_single_steps(cfgmod, geom, capi, profmod, name, in_loop):
    if name == "dp05_auto":
        loop, rebins = in_loop
    else:
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            ctx.modes_enable(every=1, capacity=64)
            ctx.advance(1e9, max_steps=N_LOOP)
            rebins = ctx.schedule()["rebins"]
            loop = ctx.modes()
    # (the static schedule re-bins every 16th step: two in forty; the other forms decide on the device: at least one)
    assert rebins >= (2 if name == "dp05_auto" else 1), f"{name}: {rebins} re-binnings in {N_LOOP} steps"
    prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
    nf = parts["n_fluid"]
    states = []
    with ctx:
        ctx.modes_enable(every=10 ** 9, capacity=64)
        for _ in range(N_LOOP):
            st = ctx.advance(1e9, max_steps=1)
            ctx.modes_sample()
            states.append((ctx.download(fields=("pos", "vel")), st["vmax"]))
        by_hand = ctx.modes()
    assert loop["step"].tolist() == list(range(1, N_LOOP + 1)) and loop["n_dropped"] == 0
    mc.assert_series_identical(loop, by_hand, name)
    for r in (0, 15, 16, 31, 32, N_LOOP - 1):  # around the static schedule's re-binnings
        d, vmax = states[r]
        _check(profmod, prm, mc.record(loop, r), d["pos"][:nf], d["vel"][:nf], vmax, 4, 8, f"{name} record {r}")


def test_repeatable_and_gated(cfgmod, geom, capi, in_loop):
    every_step, _ = in_loop
    t = every_step["t"]
    t_from = 0.5 * (t[3] + t[4])  # between step 4 and step 5
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.modes_enable(every=1, capacity=64)
        ctx.advance(1e9, max_steps=N_LOOP)
        again = ctx.modes()
        ctx.modes_enable(every=3, t_from=t_from + t[-1], capacity=64)      # (re-enabled: empty, and the clock runs on)
        assert len(ctx.modes()["step"]) == 0
    mc.assert_series_identical(again, every_step, "two runs")
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.modes_enable(every=3, t_from=t_from, capacity=64)
        ctx.advance(1e9, max_steps=20)
        gated = ctx.modes()
        ctx.modes_enable(every=10 ** 9)
        ctx.advance(1e9, max_steps=5)
        assert len(ctx.modes()["step"]) == 0
        ctx.modes_sample()
        one = ctx.modes()
        st = ctx.sync()
    want = [s for s in range(1, 21) if s % 3 == 0 and t[s - 1] >= t_from]
    assert want == [6, 9, 12, 15, 18] and gated["step"].tolist() == want
    mc.assert_series_identical(gated, {k: every_step[k][[s - 1 for s in want]] for k in mc.SERIES}, "gated", counters=False)
    assert one["step"].tolist() == [25] and one["t"].tolist() == [st["t"]] and one["n_dropped"] == 0


def test_record_buffer_capacity_drain_and_lifecycle(cfgmod, geom, capi, in_loop):
    whole, _ = in_loop
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    cap = 3
    with ctx:
        ctx.modes_enable(every=1, capacity=cap)
        ctx.advance(1e9, max_steps=7)
        full = ctx.modes()
        again = ctx.modes(drain=True)
        empty = ctx.modes()
        ctx.advance(1e9, max_steps=5)
        resumed = ctx.modes()
        ctx.modes_disable()
        ctx.modes_disable()                                  # a no-op when off
        for call in (ctx.modes, ctx.modes_sample):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:Modes:disabled" and e.value.code == capi.SPHX_ERR_STATE
        ctx.advance(1e9, max_steps=4)                        # steps 13-16, not recorded
        ctx.modes_enable(mx=2, ny=3, every=2, capacity=8)
        fresh = ctx.modes()
        ctx.advance(1e9, max_steps=6)
        back = ctx.modes()
    assert full["step"].tolist() == [1, 2, 3] and full["n_dropped"] == 7 - cap
    mc.assert_series_identical(full, {k: whole[k][:cap] for k in mc.SERIES}, "capacity 3", counters=False)
    mc.assert_series_identical(full, again, "read twice")
    assert len(empty["step"]) == 0 and empty["n_dropped"] == 0 and empty["ux"].shape == (0, 5, 9, 4)
    # after the drain the next records land at slot 0 and n_dropped restarts
    assert resumed["step"].tolist() == [8, 9, 10] and resumed["n_dropped"] == 2
    mc.assert_series_identical(resumed, {k: whole[k][7:10] for k in mc.SERIES}, "resumed", counters=False)
    assert len(fresh["step"]) == 0 and fresh["n"].shape == (0, 3, 4, 4) and fresh["n_dropped"] == 0
    assert back["step"].tolist() == [18, 20, 22] and back["n_dropped"] == 0
    for f in mc.FIELDS:  # the smaller set of modes is the corner of the larger one, to the bit
        assert np.array_equal(back[f], whole[f][[17, 19, 21], :3, :4]), f


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic"])
def test_sampler_on_and_never_on_leave_the_same_state(cfgmod, geom, capi, name):
    outs = []
    for on in (False, True):
        prm, parts, ctx = _ctx(capi, cfgmod, geom, name)
        with ctx:
            if on:
                ctx.modes_enable(mx=16, ny=16, every=1, capacity=64)
            st = ctx.advance(1e9, max_steps=N_LOOP)
            outs.append((st, ctx.download(fields=("pos", "vel", "drho_dt"))))
            if on:
                assert len(ctx.modes()["step"]) == N_LOOP
    assert outs[0][0] == outs[1][0]
    for k in ("pos", "vel", "drho_dt"):
        assert outs[0][1][k].tobytes() == outs[1][1][k].tobytes(), k


def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.modes_enable(every=1)
        on = profiled_launches(ctx, 20)
        ctx.modes_disable()
        off = profiled_launches(ctx, 20)
    assert all("k_modes" not in d for d in (never, never2, off))
    assert on.pop("k_modes") == 20
    assert on == never and off == never2


def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    with ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the sampling kernel
        ctx.modes_enable(every=1, capacity=100)
        ctx.advance(1e9, max_steps=64)
        assert ctx.modes()["step"].tolist() == list(range(65, 129))
        ctx.modes_disable()
        ctx.advance(1e9, max_steps=64)
        ctx.modes_enable(every=2, mx=1, ny=1)
        ctx.prepare_steps(24)
        g0 = ctx.graph_stats()["graphs_captured"]
        st = ctx.advance(1e9, max_steps=24)
        assert ctx.graph_stats()["graphs_captured"] == g0
        got = ctx.modes()
        assert got["step"].tolist() == list(range(194, 217, 2)) and got["t"][-1] == st["t"]
        ctx.prepare_steps(8)                               # prepared with the sampler on: disabling takes effect all the same
        ctx.modes_disable()
        ctx.advance(1e9, max_steps=8)
        ctx.modes_enable(every=1, mx=1, ny=1)
        ctx.advance(1e9, max_steps=2)
        assert ctx.modes()["step"].tolist() == [225, 226]


# 6 ---------------------------------------------------------------------------------------------------------------
def test_poison_at_free_gives_the_same_bytes(cfgmod, geom, capi, in_loop):
    want, _ = in_loop
    capi.pool_poison_on_free(True)
    try:
        prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
        with ctx:
            ctx.modes_enable(mx=16, ny=16, every=1, capacity=4)   # a larger buffer first: its blocks go back poisoned
            ctx.advance(1e9, max_steps=2)
            ctx.modes_disable()
        prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
        with ctx:
            ctx.modes_enable(every=1, capacity=64)
            ctx.advance(1e9, max_steps=N_LOOP)
            got = ctx.modes()
    finally:
        capi.pool_poison_on_free(False)
    mc.assert_series_identical(got, want, "poison at free")
    assert all(np.all(np.isfinite(got[f])) for f in mc.FIELDS)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, ctx = _ctx(capi, cfgmod, geom, "dp05_auto")
    nothing = (None, None, None, None, None, None, 0)

    def config(**kw):
        c = capi.SphxModesConfig(mx=4, ny=8, every=1, capacity=16, t_from=0.0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    with ctx:
        h = ctx._h
        assert err_id(capi, L.sphx_ctx_modes_read, h, 0, *nothing) == ("SPHX:Modes:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_ctx_modes_sample, h) == ("SPHX:Modes:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_modes_disable(h) == capi.SPHX_OK           # a no-op when off
        ctx.modes_enable(every=1, capacity=16)
        ctx.advance(1e9, max_steps=5)
        before = ctx.modes()
        assert len(before["step"]) == 5
        refused = [dict(mx=-1), dict(mx=17), dict(ny=-1), dict(ny=17), dict(every=0), dict(every=-1), dict(capacity=0), dict(capacity=-5),
                   dict(t_from=float("nan")), dict(capacity=(1 << 27) // 540 + 1)]   # (45 modes x 12: 540 doubles a record)
        for bad in refused:
            c2 = config(**bad)
            assert err_id(capi, L.sphx_ctx_modes_enable, h, C.byref(c2)) == ("SPHX:Modes:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_modes_enable, h, None) == ("SPHX:Modes:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.modes_enable(every=0)
        assert e.value.identifier == "SPHX:Modes:config"
        mc.assert_series_identical(ctx.modes(), before, "a refused enable leaves the records as they were")
        ctx.advance(1e9, max_steps=2)
        assert ctx.modes()["step"].tolist() == list(range(1, 8))      # ... and the sampler running
        n, gx, gy = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.sphx_ctx_modes_read(h, 0, None, None, C.byref(gx), C.byref(gy), C.byref(n), None, 0) == capi.SPHX_OK
        assert (gx.value, gy.value, n.value) == (4, 8, 7)
        times, records = np.zeros((7, 2)), np.zeros((7, 5, 9, 3, 4))
        assert err_id(capi, L.sphx_ctx_modes_read, h, 6, capi.ptr(times), None, None, None, None, None, 0)[0] == "SPHX:Modes:capacity"
        assert err_id(capi, L.sphx_ctx_modes_read, h, 6, None, capi.ptr(records), None, None, None, None, 1)[0] == "SPHX:Modes:capacity"
        assert np.all(times == 0) and np.all(records == 0)
        assert L.sphx_ctx_modes_read(h, 7, capi.ptr(times), capi.ptr(records), None, None, None, None, 0) == capi.SPHX_OK
        assert times[:, 0].tolist() == list(range(1, 8)) and np.array_equal(records[:, :, :, 1, :], ctx.modes()["ux"])
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = config()
        for fn, args in ((L.sphx_ctx_modes_enable, (C.byref(cfg),)), (L.sphx_ctx_modes_disable, ()), (L.sphx_ctx_modes_sample, ()),
                         (L.sphx_ctx_modes_read, (0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:Modes:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


def test_a_non_finite_velocity_raises_the_range_flag(cfgmod, geom, capi):
    """Nothing is stepped: the sample of the initial state, of which one particle's u_y is NaN."""
    prm, parts, kw = mc.case(make_case, cfgmod, geom, "dp05_auto")
    vel = parts["vel"].copy(order="F")
    vel[5, 1] = float("nan")
    with capi.Context.from_parts(prm, dict(parts, vel=vel), t_end=1e9) as ctx:
        ctx.modes_enable(every=1, capacity=4)
        ctx.modes_sample()
        with pytest.raises(capi.SphxError) as e:
            ctx.modes()
        assert e.value.identifier == "SPHX:Modes:range" and e.value.code == capi.SPHX_ERR_STATE


# 8 ---------------------------------------------------------------------------------------------------------------
def test_driver_run_collects_the_whole_series(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0, end_time=0.03, output_interval=0.01)
    res = driver.run(prm, modes_every=1, modes=(2, 3))
    s = res.modes
    assert s["step"].tolist() == list(range(1, res.steps + 1)) and s["n_dropped"] == 0 and s["t"][-1] == res.t
    assert s["n"].shape == s["ux"].shape == (res.steps, 3, 4, 4) and np.all(s["n"][:, 0, 0, 0] == res.n_fluid)
    assert driver.run(prm).modes is None
    need = int(np.searchsorted(s["t"], 0.01 + 1e-12))              # the records of the first output interval
    assert need > 4
    with pytest.raises(RuntimeError, match=rf"modes_capacity >= {need} \(it is 4\)"):
        driver.run(prm, modes_every=1, modes_capacity=4)
    fig = driver.mode_figures(prm, s)
    assert fig["b"].shape == (res.steps, 4) and np.all(fig["b"][:, 1] > 0.0)


# 9 ---------------------------------------------------------------------------------------------------------------
def test_startup_follows_the_oracle_mode_by_mode(cfgmod, geom, capi, profmod, oracle):
    """From rest, dp = 0.05, DL = 3, to t = 0.4 (374 steps), every step recorded.  b_1(t) and b_3(t) = (2 / N) ux[0, n, cs] of the
    device's records against profile.mode_sums of the oracle's own trajectory, step by step, within mc.PARITY of the series'
    largest |b_n| (the suite's parity tolerance: 1e-10 of a field's scale); and their largest distance from the closed form
    b_n(inf) (1 - exp(-t / tau_n)) within 1.5 x what the oracle's trajectory shows (mc.STARTUP_DISTANCE, measured on the CPU by
    tests/test_modes_host.py; the margin is for summation order only)."""
    s = mc.STARTUP
    prm = cfgmod.params_from_values(dp=s["dp"], DL=s["DL"], end_time=s["t_end"], output_interval=s["t_end"])
    parts = geom.init_particles(prm)
    nf = parts["n_fluid"]
    with capi.Context.from_parts(prm, parts, t_end=s["t_end"]) as ctx:
        ctx.modes_enable(mx=0, ny=3, every=1, capacity=1024)
        st = ctx.sync()
        while st["t"] < s["t_end"] - 1e-12:
            st = ctx.advance(s["t_end"])
        got = ctx.modes()
    t, pos, vel = mc.oracle_trajectory(oracle, prm, parts, s["t_end"])
    want = mc.b_series(profmod, prm, pos, vel)
    assert st["t"] == s["t_end"] and got["n_dropped"] == 0 and len(got["t"]) == len(t) == st["step"]
    assert np.all(np.abs(got["t"] - t) <= 1e-13 * t)
    assert np.all(got["n"][:, 0, 0, 0] == nf)
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    for n in (1, 3):
        b = 2.0 / nf * got["ux"][:, 0, n, 2]
        scale = float(np.max(np.abs(want[n])))
        parity = float(np.max(np.abs(b - want[n]))) / scale
        dist = float(np.max(np.abs(b - profmod.mode_b_exact(n, got["t"], prm.gravity_g, prm.nu, prm.DH)))) / u_max
        print(f"b_{n}: {len(t)} steps, off the oracle's by {parity:.3e} of its largest value; at most {dist:.5e} U_max from the closed "
              f"form (the oracle: {mc.STARTUP_DISTANCE[n]:.5e})")
        assert parity <= mc.PARITY, n
        assert dist <= mc.STARTUP_MARGIN * mc.STARTUP_DISTANCE[n], n
