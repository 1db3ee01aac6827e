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
from helpers import (assert_history_matches_oracle, check_kernel_form, err_id, gateway_cfg, make_case, make_variant,
                     oracle_history_rows, profiled_launches, rel_err)

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


def _host_sums(parts, d):
    """kinetic energy and bulk velocity of a downloaded state, as the header defines them"""
    nf = parts["n_fluid"]
    v, m = d["vel"][:nf], parts["mass"][:nf]
    return float(np.sum(0.5 * m * (v[:, 0] ** 2 + v[:, 1] ** 2))), float(np.mean(v[:, 0]))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_series(cfgmod, geom, oracle):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0)
    return prm, parts, oracle_history_rows(oracle, prm, parts, 36)


@pytest.fixture(scope="module")
def left_series(cfgmod, geom, oracle):
    # plain_series mirrored: U_bulk < 0, so g, u_bulk and both tau are negative
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, U_bulk=-0.666667)
    return prm, parts, oracle_history_rows(oracle, prm, parts, 36)


@pytest.fixture(scope="module")
def variant_series(cfgmod, geom, oracle):
    # moving walls (top and bottom differ in size and sign), uneven mass, rho0 != 1
    prm, parts = make_variant(cfgmod, geom, seed=7, developed=True, dp=0.05, DL=1.5, jitter=0.2, rho0=2.5, transport_coeff=0.1)
    return prm, parts, oracle_history_rows(oracle, prm, parts, 12)


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
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.history_enable(every=1)
        assert ctx.advance(1e9, max_steps=len(want))["step"] == len(want)
        rebins = ctx.schedule()["rebins"]
        hist = ctx.history()
    assert rebins >= 2, f"only {rebins} re-binnings: both Vol / B lookups must be exercised"
    assert_history_matches_oracle(hist, want, what)
    return hist


@pytest.mark.parametrize("lpp", [16, 4])
def test_series_matches_the_oracle_with_moving_walls_and_uneven_mass(capi, variant_series, lpp):
    prm, parts, want = variant_series
    assert np.all(want[:, 4] * want[:, 5] < 0) and np.all(rel_err(want[:, 4], -want[:, 5]) > 0.1)  # tau_bottom != tau_top
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=lpp, rebuild_every=4) as ctx:
        assert ctx.kernel_forms()["walk_kernels"] == (lpp == 4)
        ctx.history_enable(every=1)
        assert ctx.advance(1e9, max_steps=len(want))["step"] == len(want)
        rebins = ctx.schedule()["rebins"]
        hist = ctx.history()
    assert rebins >= 2
    assert_history_matches_oracle(hist, want, f"variant lpp {lpp}")


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_last_record_is_what_the_host_path_reports(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        check_kernel_form(ctx, name)
        ctx.history_enable(every=1)
        st = ctx.advance(1e9, max_steps=45)
        hist = ctx.history()
        tb, tt, _ = ctx.monitor(tau=True)
        ke, ub = _host_sums(parts, ctx.download(fields=("vel",)))
    assert len(hist["step"]) == 45 and hist["n_dropped"] == 0
    assert (hist["step"][-1], hist["t"][-1], hist["dt"][-1], hist["vmax"][-1]) == (st["step"], st["t"], st["dt_last"], st["vmax"])
    err = dict(tau_bottom=rel_err(hist["tau_bottom"][-1], tb), tau_top=rel_err(hist["tau_top"][-1], tt),
               kinetic_energy=rel_err(hist["kinetic_energy"][-1], ke), u_bulk=rel_err(hist["u_bulk"][-1], ub))
    print(name, {k: f"{float(v):.2e}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= 1e-12, f"{name}: {k} off by {float(v):.3e} (summation order only)"


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_chunked_calls_record_the_same_series(cfgmod, geom, capi, name):
    prm, parts, kw = _case(cfgmod, geom, name)
    runs = []
    for chunks in ((45,), (7, 13, 25)):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.history_enable(every=1)
            for n in chunks:
                ctx.advance(1e9, max_steps=n)
            runs.append(ctx.history())
    one, chunked = runs
    assert list(one["step"]) == list(range(1, 46))
    for k in CLOCK:
        assert np.array_equal(one[k], chunked[k]), f"{name}: {k}"
    for k in SUMS:
        err = rel_err(chunked[k], one[k]).max()
        assert err <= 1e-12, f"{name}: {k} off by {err:.3e}"


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
        ctx.history_enable(every=every, t_from=t_from)
        ctx.advance(1e9, max_steps=N)
        hist = ctx.history()
    assert len(want) > 0 and list(hist["step"]) == [s["step"] for s in want]
    assert list(hist["t"]) == [s["t"] for s in want] and list(hist["dt"]) == [s["dt_last"] for s in want]
    assert list(hist["vmax"]) == [s["vmax"] for s in want]


def test_full_buffer_drops_and_drain_resumes(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
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
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            if on:
                ctx.history_enable(every=1)
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
        ctx.history_enable(every=4)                       # one launch per slot whatever the stride: it skips itself
        on = profiled_launches(ctx, 20)
        assert list(ctx.history()["step"]) == [4, 8, 12, 16, 20]
        ctx.history_disable()
        off = profiled_launches(ctx, 20)
    assert "k_step_history" not in never and "k_step_history" not in never2 and "k_step_history" not in off
    assert on.pop("k_step_history") == 20
    assert on == never and off == never2


def test_independent_of_the_flow_statistics(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.history_enable(every=2)
        ctx.advance(1e9, max_steps=30)
        alone = ctx.history()
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
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
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
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
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.history_enable(every=1)
            ctx.advance(1e9, max_steps=60)
            runs.append(ctx.history_records())
    assert runs[0][0].shape == (60, 8) and runs[0][1] == runs[1][1] == 0
    assert runs[0][0].tobytes() == runs[1][0].tobytes(), name


# 8 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    n, dropped = C.c_int(-1), C.c_int64(-1)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        h = ctx._h
        assert err_id(capi, L.sphx_ctx_history_read, h, 0, None, C.byref(n), C.byref(dropped), 0) == \
            ("SPHX:History:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_history_disable(h) == capi.SPHX_OK       # no-op when off
        for bad in (dict(every=0), dict(every=-1), dict(capacity=0), dict(capacity=-5), dict(capacity=(1 << 22) + 1),
                    dict(t_from=float("nan")), dict(t_from=float("inf")), dict(t_from=-float("inf"))):
            c2 = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert err_id(capi, L.sphx_ctx_history_enable, h, C.byref(c2)) == ("SPHX:History:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_history_enable, h, None) == ("SPHX:History:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            ctx.history_enable(every=0)
        assert e.value.identifier == "SPHX:History:config"
        # a refused config leaves the context without a history, and stepping
        assert err_id(capi, L.sphx_ctx_history_read, h, 0, None, None, None, 0)[0] == "SPHX:History:disabled"
        assert ctx.advance(1e9, max_steps=3)["step"] == 3
        cfg = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
        assert L.sphx_ctx_history_enable(h, C.byref(cfg)) == capi.SPHX_OK
        ctx.advance(1e9, max_steps=5)
        assert L.sphx_ctx_history_read(h, 0, None, C.byref(n), C.byref(dropped), 0) == capi.SPHX_OK   # counts only
        assert (n.value, dropped.value) == (5, 0)
        buf = np.full((5, 8), -1.0)
        assert err_id(capi, L.sphx_ctx_history_read, h, 4, capi.ptr(buf), None, None, 1) == \
            ("SPHX:History:capacity", capi.SPHX_ERR_ARG)
        assert np.all(buf == -1.0)
        assert L.sphx_ctx_history_read(h, 5, capi.ptr(buf), C.byref(n), None, 0) == capi.SPHX_OK      # ... and nothing was drained
        assert n.value == 5 and list(buf[:, 0]) == [4.0, 5.0, 6.0, 7.0, 8.0]
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
        for fn, args in ((L.sphx_ctx_history_enable, (C.byref(cfg),)), (L.sphx_ctx_history_disable, ()),
                         (L.sphx_ctx_history_read, (0, None, None, None, 0))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:History:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()


# 9 ---------------------------------------------------------------------------------------------------------------
def test_matlab_gateway_history_commands(cfgmod, geom, capi):
    prm, parts, kw = _case(cfgmod, geom, "dp05_auto")
    gw = mex_mock.Gateway("sphx_ctx_mex.c")
    nf, nt = parts["n_fluid"], parts["n_total"]
    state = (parts["pos"], parts["vel"], parts["drho_dt"], parts["mass"], parts["wall_vel"])
    (h,) = gw(1, "create", gateway_cfg(prm, 1e9), nf, nt, *state, 0.0, 0)
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
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
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
    assert rel_err(last.history["tau_bottom"][-1], last.tau_bottom) <= 1e-12
    assert rel_err(last.history["tau_top"][-1], last.tau_top) <= 1e-12
    for k in FIELDS:                                                 # every second record of the full series, bit for bit
        assert np.array_equal(last.history[k][1::2], hist[k]), k
    fig = driver.history_figures(prm, last.history, t_from=0.1)
    assert fig["n_records"] == int(np.count_nonzero(last.history["t"] >= 0.1)) > 0
    assert min(last.history["u_bulk"][last.history["t"] >= 0.1]) <= fig["u_bulk_mean"] <= max(last.history["u_bulk"])
