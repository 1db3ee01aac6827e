"""-m gpu: the device-side step history (include/sphx.h section 2d) -- one record per step (step, t, dt, vmax, tau_bottom,
tau_top, kinetic_energy, u_bulk) written by k_step_history inside the step loop.  Checked step by step against the oracle's
loop (restarted for every row), against the host path it replaces (status / monitor() / numpy over download()) on every
kernel form and schedule, for independence of host chunking, for gating and the buffer's bounds, for leaving the physics and
the launches untouched, with captured graphs, for repeatability, for its error identifiers, through the MATLAB context
gateway and through driver.run."""
import ctypes as C

import numpy as np
import pytest

import mex_mock
from helpers import assert_close, make_case, make_variant

pytestmark = pytest.mark.gpu

# the shapes of tests/test_gpu_flow_stats.py: the smallest that reach each kernel form and schedule
CASES = {
    "dp05_auto": (0.05, 3.0, dict()),                                  # 1 200 fluid particles: one workgroup, no ticket
    "dp025_lpp16": (0.025, 1.5, dict(lanes_per_particle=16)),
    "dp025_walk": (0.025, 1.5, dict(lanes_per_particle=4)),            # the "_w" forms
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1)),
    "dp025_dual": (0.025, 1.5, dict(lanes_per_particle=16, dual_rate=2)),
    "dp01_multi": (0.01, 3.0, dict()),                                 # 30 k particles: several workgroups, partials + ticket
}
FIELDS = ("step", "t", "dt", "vmax", "tau_bottom", "tau_top", "kinetic_energy", "u_bulk")
CLOCK, SUMS = FIELDS[:4], FIELDS[4:]


def _case(cfgmod, geom, name, seed=11):
    dp, DL, kw = CASES[name]
    prm, parts = make_case(cfgmod, geom, dp=dp, DL=DL, jitter=0.2, seed=seed, developed=True)
    return prm, parts, kw


def _ctx(capi, prm, parts, **kw):
    nf, nt = parts["n_fluid"], parts["n_total"]
    return capi.Context(prm, nf, nt, parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"],
                        t_end=1e9, **kw)


def _check_form(ctx, name):
    if name == "dp025_walk":
        assert ctx.kernel_forms()["walk_kernels"]
    if name == "dp05_dynamic":
        assert ctx.schedule()["dynamic"]
    if name == "dp025_dual":
        assert ctx.substeps() > 1


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def _host_sums(parts, d):
    """kinetic energy and bulk velocity of a downloaded state, as the header defines them"""
    nf = parts["n_fluid"]
    v, m = d["vel"][:nf], parts["mass"][:nf]
    return float(np.sum(0.5 * m * (v[:, 0] ** 2 + v[:, 1] ** 2))), float(np.mean(v[:, 0]))


# 1 ---------------------------------------------------------------------------------------------------------------
def _oracle_rows(oracle, prm, parts, n_steps):
    """row k-1 = what the oracle's loop leaves after k steps (restarted from the initial state for every row)"""
    nf = parts["n_fluid"]
    rows = np.zeros((n_steps, 8))
    for k in range(1, n_steps + 1):
        ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=k, enable_sort=False)
        s, v, m = ref["stats"], ref["vel"][:nf], ref["mass"][:nf]
        assert s["steps"] == k
        rows[k - 1] = (k, s["t"], s["dt_last"], s["vmax"], s["tau_bottom"], s["tau_top"],
                       np.sum(0.5 * m * (v[:, 0] ** 2 + v[:, 1] ** 2)), np.mean(v[:, 0]))
    return rows


@pytest.fixture(scope="module")
def plain_series(cfgmod, geom, oracle):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0)
    return prm, parts, _oracle_rows(oracle, prm, parts, 36)


@pytest.fixture(scope="module")
def left_series(cfgmod, geom, oracle):
    # plain_series mirrored: U_bulk < 0, so g, u_bulk and both tau are negative
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, U_bulk=-0.666667)
    return prm, parts, _oracle_rows(oracle, prm, parts, 36)


@pytest.fixture(scope="module")
def variant_series(cfgmod, geom, oracle):
    # moving walls (top and bottom differ in size and sign), uneven mass, rho0 != 1
    prm, parts = make_variant(cfgmod, geom, seed=7, developed=True, dp=0.05, DL=1.5, jitter=0.2, rho0=2.5, transport_coeff=0.1)
    return prm, parts, _oracle_rows(oracle, prm, parts, 12)


def _assert_series_matches_oracle(hist, want, what):
    n = len(want)
    assert list(hist["step"]) == list(range(1, n + 1)) and hist["n_dropped"] == 0, what
    got = {k: hist[k] for k in FIELDS}
    ref = {k: want[:, j] for j, k in enumerate(FIELDS)}
    tau_got = np.column_stack([got["tau_bottom"], got["tau_top"]])
    tau_ref = np.column_stack([ref["tau_bottom"], ref["tau_top"]])
    tau_scale = np.max(np.abs(tau_ref), axis=1, keepdims=True)
    print(f"{what}: max rel err t {_rel(got['t'], ref['t']).max():.2e} dt {_rel(got['dt'], ref['dt']).max():.2e} "
          f"vmax {_rel(got['vmax'], ref['vmax']).max():.2e} tau (of the pair's larger) "
          f"{(np.abs(tau_got - tau_ref) / tau_scale).max():.2e} kinetic_energy "
          f"{_rel(got['kinetic_energy'], ref['kinetic_energy']).max():.2e} u_bulk {_rel(got['u_bulk'], ref['u_bulk']).max():.2e}")
    assert np.all(np.abs(got["t"] - ref["t"]) <= 1e-13 * ref["t"]), what
    assert np.all(np.abs(got["dt"] - ref["dt"]) <= 1e-12 * ref["dt"]), what
    assert np.all(np.abs(got["vmax"] - ref["vmax"]) <= 1e-9 * ref["vmax"]), what
    for k in range(n):  # the pair of one step together, as tests/test_gpu_resident.py compares monitor() with the oracle
        assert_close(tau_got[k], tau_ref[k], rtol=1e-8, atol_scale=1e-9, name=f"{what}: tau of step {k + 1}")
    assert np.all(_rel(got["kinetic_energy"], ref["kinetic_energy"]) <= 1e-8), what
    assert np.all(_rel(got["u_bulk"], ref["u_bulk"]) <= 1e-8), what


def test_series_matches_the_oracle_step_by_step(capi, plain_series):
    _series_matches_the_oracle_step_by_step(capi, plain_series, "dp05")


def test_series_matches_the_oracle_step_by_step_leftward(capi, left_series):
    prm, parts, want = left_series
    assert prm.gravity_g < 0 and np.all(want[:, 4:6] < 0) and np.all(want[:, 7] < 0)    # both tau and u_bulk of the oracle
    hist = _series_matches_the_oracle_step_by_step(capi, left_series, "dp05 leftward")
    assert np.all(hist["tau_bottom"] < 0) and np.all(hist["tau_top"] < 0) and np.all(hist["u_bulk"] < 0)


def _series_matches_the_oracle_step_by_step(capi, series, what):
    prm, parts, want = series
    # from one step to the next every field moves by far more than the tolerances: a record taken a step early or late fails
    assert np.all(np.abs(np.diff(want[:, 1:], axis=0)) >= 1e-6 * np.abs(want[1:, 1:]))
    with _ctx(capi, prm, parts) as ctx:
        ctx.history_enable(every=1)
        assert ctx.advance(1e9, max_steps=len(want))["step"] == len(want)
        rebins = ctx.schedule()["rebins"]
        hist = ctx.history()
    assert rebins >= 2, f"only {rebins} re-binnings: both Vol / B lookups must be exercised"
    _assert_series_matches_oracle(hist, want, what)
    return hist


@pytest.mark.parametrize("lpp", [16, 4])
def test_series_matches_the_oracle_with_moving_walls_and_uneven_mass(capi, variant_series, lpp):
    prm, parts, want = variant_series
    assert np.all(want[:, 4] * want[:, 5] < 0) and np.all(_rel(want[:, 4], -want[:, 5]) > 0.1)  # tau_bottom != tau_top
    with _ctx(capi, prm, parts, lanes_per_particle=lpp, rebuild_every=4) as ctx:
        assert ctx.kernel_forms()["walk_kernels"] == (lpp == 4)
        ctx.history_enable(every=1)
        assert ctx.advance(1e9, max_steps=len(want))["step"] == len(want)
        rebins = ctx.schedule()["rebins"]
        hist = ctx.history()
    assert rebins >= 2
    _assert_series_matches_oracle(hist, want, f"variant lpp {lpp}")


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_last_record_is_what_the_host_path_reports(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    with _ctx(capi, prm, parts, **kw) as ctx:
        _check_form(ctx, name)
        ctx.history_enable(every=1)
        st = ctx.advance(1e9, max_steps=45)
        hist = ctx.history()
        tb, tt, _ = ctx.monitor(tau=True)
        ke, ub = _host_sums(parts, ctx.download(fields=("vel",)))
    assert len(hist["step"]) == 45 and hist["n_dropped"] == 0
    assert (hist["step"][-1], hist["t"][-1], hist["dt"][-1], hist["vmax"][-1]) == (st["step"], st["t"], st["dt_last"], st["vmax"])
    err = dict(tau_bottom=_rel(hist["tau_bottom"][-1], tb), tau_top=_rel(hist["tau_top"][-1], tt),
               kinetic_energy=_rel(hist["kinetic_energy"][-1], ke), u_bulk=_rel(hist["u_bulk"][-1], ub))
    print(name, {k: f"{float(v):.2e}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= 1e-12, f"{name}: {k} off by {float(v):.3e} (summation order only)"


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_chunked_calls_record_the_same_series(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    runs = []
    for chunks in ((45,), (7, 13, 25)):
        with _ctx(capi, prm, parts, **kw) as ctx:
            ctx.history_enable(every=1)
            for n in chunks:
                ctx.advance(1e9, max_steps=n)
            runs.append(ctx.history())
    one, chunked = runs
    assert list(one["step"]) == list(range(1, 46))
    for k in CLOCK:
        assert np.array_equal(one[k], chunked[k]), f"{name}: {k}"
    for k in SUMS:
        err = _rel(chunked[k], one[k]).max()
        assert err <= 1e-12, f"{name}: {k} off by {err:.3e}"


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_gating_every_and_t_from(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    N, every = 40, 3
    with _ctx(capi, prm, parts, **kw) as ctx:
        statuses = [ctx.advance(1e9, max_steps=1) for _ in range(N)]
    t_from = 0.5 * (statuses[N // 2]["t"] + statuses[N // 2 + 1]["t"])
    want = [s for s in statuses if s["step"] % every == 0 and s["t"] >= t_from]
    with _ctx(capi, prm, parts, **kw) as ctx:
        ctx.history_enable(every=every, t_from=t_from)
        ctx.advance(1e9, max_steps=N)
        hist = ctx.history()
    assert len(want) > 0 and list(hist["step"]) == [s["step"] for s in want]
    assert list(hist["t"]) == [s["t"] for s in want] and list(hist["dt"]) == [s["dt_last"] for s in want]
    assert list(hist["vmax"]) == [s["vmax"] for s in want]


def test_full_buffer_drops_and_drain_resumes(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with _ctx(capi, prm, parts) as ctx:
        ctx.history_enable(every=1, capacity=10)
        ctx.advance(1e9, max_steps=25)
        full = ctx.history()
        again = ctx.history()                    # reading without drain changes nothing
        drained = ctx.history(drain=True)
        empty = ctx.history()
        st = ctx.advance(1e9, max_steps=5)
        resumed = ctx.history()
        ctx.history_enable(every=1, capacity=10)  # re-enabling empties the buffer
        assert len(ctx.history()["step"]) == 0
    assert list(full["step"]) == list(range(1, 11)) and full["n_dropped"] == 15
    for k in FIELDS + ("n_dropped",):
        assert np.array_equal(full[k], again[k]) and np.array_equal(full[k], drained[k]), k
    assert len(empty["step"]) == 0 and empty["n_dropped"] == 0
    assert list(resumed["step"]) == list(range(26, 31)) and resumed["n_dropped"] == 0 and resumed["t"][-1] == st["t"]


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp05_dynamic"])
def test_no_feedback_on_the_physics(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    outs = []
    for on in (False, True):
        with _ctx(capi, prm, parts, **kw) as ctx:
            if on:
                ctx.history_enable(every=1)
            st = ctx.advance(1e9, max_steps=45)
            outs.append((st, ctx.download(fields=("pos", "vel", "drho_dt"))))
    assert outs[0][0] == outs[1][0]
    for k in ("pos", "vel", "drho_dt"):
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k


def _profiled_launches(ctx, n):
    ctx.profile_enable(True)
    ctx.advance(1e9, max_steps=n)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {k: v["launches"] for k, v in prof.items() if v["launches"] > 0}  # (names seen earlier stay listed with 0)


def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with _ctx(capi, prm, parts) as ctx:                   # steps 1-20 and 21-40: the same re-binning phases as below
        never = _profiled_launches(ctx, 20)
        never2 = _profiled_launches(ctx, 20)
    with _ctx(capi, prm, parts) as ctx:
        ctx.history_enable(every=4)                       # one launch per slot whatever the stride: it skips itself
        on = _profiled_launches(ctx, 20)
        assert list(ctx.history()["step"]) == [4, 8, 12, 16, 20]
        ctx.history_disable()
        off = _profiled_launches(ctx, 20)
    assert "k_step_history" not in never and "k_step_history" not in never2 and "k_step_history" not in off
    assert on.pop("k_step_history") == 20
    assert on == never and off == never2


def test_independent_of_the_flow_statistics(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with _ctx(capi, prm, parts) as ctx:
        ctx.history_enable(every=2)
        ctx.advance(1e9, max_steps=30)
        alone = ctx.history()
    with _ctx(capi, prm, parts) as ctx:
        ctx.flow_stats_enable(every=3)
        ctx.history_enable(every=2)
        ctx.advance(1e9, max_steps=30)
        both = ctx.history()
        assert ctx.flow_stats(0)["n_samples"] == 10
        ctx.flow_stats_disable()
        ctx.advance(1e9, max_steps=4)
        assert list(ctx.history()["step"]) == list(range(2, 35, 2))
    assert list(alone["step"]) == list(range(2, 31, 2))
    for k in FIELDS:
        assert np.array_equal(alone[k], both[k]), k


# 6 ---------------------------------------------------------------------------------------------------------------
def test_enable_disable_take_effect_on_existing_graphs(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with _ctx(capi, prm, parts) as ctx:
        ctx.advance(1e9, max_steps=64)                    # graphs exist without the history kernel
        ctx.history_enable(every=1)
        ctx.advance(1e9, max_steps=64)
        assert list(ctx.history()["step"]) == list(range(65, 129))
        ctx.history_disable()
        ctx.advance(1e9, max_steps=64)
        with pytest.raises(capi.SphxError) as e:
            ctx.history()
        assert e.value.identifier == "SPHX:History:disabled"
        ctx.history_enable(every=2)
        assert len(ctx.history()["step"]) == 0
        ctx.prepare_steps(24)
        g0 = ctx.graph_stats()["graphs_captured"]
        st = ctx.advance(1e9, max_steps=24)
        assert ctx.graph_stats()["graphs_captured"] == g0
        hist = ctx.history()
        assert list(hist["step"]) == list(range(194, 217, 2)) and hist["t"][-1] == st["t"]


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp01_multi"])
def test_repeatable(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    runs = []
    for _ in range(2):
        with _ctx(capi, prm, parts, **kw) as ctx:
            ctx.history_enable(every=1)
            ctx.advance(1e9, max_steps=60)
            runs.append(ctx.history_records())
    assert runs[0][0].shape == (60, 8) and runs[0][1] == runs[1][1] == 0
    assert runs[0][0].tobytes() == runs[1][0].tobytes(), name


# 8 ---------------------------------------------------------------------------------------------------------------
def _err(capi, fn, *args):
    rc = fn(*args)
    assert rc != capi.SPHX_OK
    return capi.lib().sphx_last_error_id().decode(), rc


def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    n, dropped = C.c_int(-1), C.c_int64(-1)
    with _ctx(capi, prm, parts) as ctx:
        h = ctx._h
        assert _err(capi, L.sphx_ctx_history_read, h, 0, None, C.byref(n), C.byref(dropped), 0) == \
            ("SPHX:History:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_history_disable(h) == capi.SPHX_OK       # no-op when off
        for bad in (dict(every=0), dict(every=-1), dict(capacity=0), dict(capacity=-5), dict(capacity=(1 << 22) + 1),
                    dict(t_from=float("nan")), dict(t_from=float("inf")), dict(t_from=-float("inf"))):
            c2 = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert _err(capi, L.sphx_ctx_history_enable, h, C.byref(c2)) == ("SPHX:History:config", capi.SPHX_ERR_ARG), bad
        assert _err(capi, L.sphx_ctx_history_enable, h, None) == ("SPHX:History:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.history_enable(every=0)
        assert e.value.identifier == "SPHX:History:config"
        # a refused config leaves the context without a history, and stepping
        assert _err(capi, L.sphx_ctx_history_read, h, 0, None, None, None, 0)[0] == "SPHX:History:disabled"
        assert ctx.advance(1e9, max_steps=3)["step"] == 3
        cfg = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
        assert L.sphx_ctx_history_enable(h, C.byref(cfg)) == capi.SPHX_OK
        ctx.advance(1e9, max_steps=5)
        assert L.sphx_ctx_history_read(h, 0, None, C.byref(n), C.byref(dropped), 0) == capi.SPHX_OK   # counts only
        assert (n.value, dropped.value) == (5, 0)
        buf = np.full((5, 8), -1.0)
        assert _err(capi, L.sphx_ctx_history_read, h, 4, capi.ptr(buf), None, None, 1) == \
            ("SPHX:History:capacity", capi.SPHX_ERR_ARG)
        assert np.all(buf == -1.0)
        assert L.sphx_ctx_history_read(h, 5, capi.ptr(buf), C.byref(n), None, 0) == capi.SPHX_OK      # ... and nothing was drained
        assert n.value == 5 and list(buf[:, 0]) == [4.0, 5.0, 6.0, 7.0, 8.0]
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
        for fn, args in ((L.sphx_ctx_history_enable, (C.byref(cfg),)), (L.sphx_ctx_history_disable, ()),
                         (L.sphx_ctx_history_read, (0, None, None, None, 0))):
            assert _err(capi, fn, eng._h, *args) == ("SPHX:History:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


# 9 ---------------------------------------------------------------------------------------------------------------
def _cfg(prm, t_end):
    return dict(DL=prm.DL, DH=prm.DH, dp=prm.dp, h=prm.h, rho0=prm.rho0, mu=prm.mu, c_f=prm.c_f, p0=prm.p0,
                inv_sigma0=prm.inv_sigma0, gravity_g=prm.gravity_g, transport_coeff=prm.transport_coeff,
                t_end=t_end, sort_interval=prm.sort_interval)


def test_matlab_gateway_history_commands(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    gw = mex_mock.Gateway("sphx_ctx_mex.c")
    nf, nt = parts["n_fluid"], parts["n_total"]
    state = (parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"])
    (h,) = gw(1, "create", _cfg(prm, 1e9), nf, nt, *state, 0.0, 0)
    try:
        with pytest.raises(mex_mock.MexError) as e:
            gw(2, "history_read", h, 0)
        assert e.value.identifier == "SPHX:History:disabled"
        gw(0, "history_enable", h, 2, 12, 0.0)
        gw(1, "advance", h, 1e9, 30)
        rec, dropped = gw(2, "history_read", h, 1)
        rec2, dropped2 = gw(2, "history_read", h, 0)       # drained
        gw(0, "history_disable", h)
    finally:
        gw(0, "destroy", h)
    with _ctx(capi, prm, parts) as ctx:
        ctx.history_enable(every=2, capacity=12)
        ctx.advance(1e9, max_steps=30)
        want, want_dropped = ctx.history_records()
    assert rec.shape == (12, 8) and dropped == want_dropped == 3
    assert np.array_equal(rec, want)
    assert np.asarray(rec2).size == 0 and dropped2 == 0


# 10 --------------------------------------------------------------------------------------------------------------
def test_driver_returns_the_history_of_the_whole_run(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.2, output_interval=0.05)
    res = driver.run(prm, history_every=2, history_capacity=4096)
    hist = res.history
    assert res.steps > 8 and hist["n_dropped"] == 0
    assert list(hist["step"]) == list(range(2, res.steps + 1, 2))   # no gap and no repeat across the four output points
    assert np.all(np.diff(hist["t"]) > 0) and hist["t"][-1] <= res.t
    if res.steps % 2 == 0:
        assert hist["t"][-1] == res.t
    # the run's last tau is the monitor's of the last step; the history's last record is that step when it is even
    last = driver.run(prm, history_every=1, history_capacity=4096)
    assert last.steps == res.steps and last.history["step"][-1] == last.steps
    assert _rel(last.history["tau_bottom"][-1], last.tau_bottom) <= 1e-12
    assert _rel(last.history["tau_top"][-1], last.tau_top) <= 1e-12
    for k in FIELDS:                                                 # every second record of the full series, bit for bit
        assert np.array_equal(last.history[k][1::2], hist[k]), k
    fig = driver.history_figures(prm, last.history, t_from=0.1)
    assert fig["n_records"] == int(np.count_nonzero(last.history["t"] >= 0.1)) > 0
    assert min(last.history["u_bulk"][last.history["t"] >= 0.1]) <= fig["u_bulk_mean"] <= max(last.history["u_bulk"])
