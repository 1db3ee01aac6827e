"""-m gpu: device-side particle tracers (include/sphx.h section 2p) -- chosen fluid rows followed step by step, one record per
sampled step, by k_tracers (a scan of the population against a table id -> column) inside the step loop.

A tracer record is what download() returns in the tracked rows, so every comparison here is np.array_equal on the float64
arrays: no tolerance.  That makes the records a check of the id bookkeeping (FluidSet::id through the fold-rebin path, the
scatter / reorder chain and the in-place dynamic path): a record taken inside the loop after every step must equal the
download taken after that step, across re-binnings and in both layouts.  n_missing -- tracers no slot of the population held
-- is 0 throughout."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import regime_cases
import tracer_cases as tc
from helpers import check_kernel_form, err_id, make_case, make_variant, profiled_launches
from test_gpu_switches import CHILD_SECONDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.SMALL)
def test_sample_now_equals_download(cfgmod, geom, capi, profmod, name):
    prm, parts, kw = tc.case(make_variant, cfgmod, geom, name)
    nf = parts["n_fluid"]
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        check_kernel_form(ctx, name)
        st = ctx.advance(1e9, max_steps=7)
        d = ctx.download(fields=("pos", "vel"))
        assert st["step"] == 7
        sets = tc.id_sets(nf)
        assert [len(v) for v in sets.values()] == [min(n, nf) for n in (1, 63, 64, 65, 300)] + [nf]
        assert all(0 in v and nf - 1 in v for k, v in sets.items() if k != "1")
        for label, ids in sets.items():
            ctx.tracers_enable(ids, every=10 ** 9, capacity=2)
            ctx.tracers_sample()
            got = ctx.tracers()
            what = f"{name} T={label}"
            assert got["step"].tolist() == [7] and got["t"].tolist() == [st["t"]], what
            assert got["n_dropped"] == 0 and got["n_missing"] == 0, what
            assert np.array_equal(got["ids"], ids) and got["x"].shape == (1, len(ids)), what
            tc.assert_record_is_state(got, 0, tc.state_rows(profmod, d, ids), what)
            assert np.all((got["x"] >= 0.0) & (got["x"] < prm.DL)), what


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.SMALL)
def test_in_loop_records_equal_a_download_after_every_step(cfgmod, geom, capi, profmod, name):
    prm, parts, kw = tc.case(make_case, cfgmod, geom, name)
    nf, N = parts["n_fluid"], 40
    ids = tc.id_sets(nf)["300"]
    runs, states = {}, []
    for how in ("replayed", "eager", "between"):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.tracers_enable(ids, every=10 ** 9 if how == "between" else 1, capacity=N)
            if how == "replayed":
                assert ctx.advance(1e9, max_steps=N)["step"] == N
                assert ctx.graph_stats()["slots_replayed"] >= N    # (more where the loop stopped on the drift bound and resumed)
            else:
                for _ in range(N):
                    ctx.advance(1e9, max_steps=1)
                    if how == "between":
                        ctx.tracers_sample()
                    else:
                        states.append(ctx.download(fields=("pos", "vel")))
                assert ctx.graph_stats()["slots_eager"] >= N
            sched, policy = ctx.schedule(), ctx.grid_policy()
            print(f"{name} {how}: schedule {sched} policy {policy}")
            # the run crossed re-binnings: on the static schedule two of them use both layouts (0 -> 1 -> 0)
            assert sched["rebins"] >= 2, (name, how, sched)
            runs[how] = ctx.tracers()
    for how, tr in runs.items():
        assert tr["step"].tolist() == list(range(1, N + 1)) and np.all(np.diff(tr["t"]) > 0), how
        assert tr["n_dropped"] == 0 and tr["n_missing"] == 0, (how, tr["n_missing"])
    tc.assert_series_identical(runs["replayed"], runs["eager"], f"{name}: replayed vs eager")
    tc.assert_series_identical(runs["replayed"], runs["between"], f"{name}: in-loop vs sampled between steps")
    assert len(states) == N
    for r, d in enumerate(states):
        tc.assert_record_is_state(runs["eager"], r, tc.state_rows(profmod, d, ids), f"{name}: record {r} vs the download after step {r + 1}")


# 3 ---------------------------------------------------------------------------------------------------------------
def _seam_case(cfgmod, geom, which):
    if which == "rightward":
        prm, parts = make_case(cfgmod, geom, dp=0.05, DL=1.5, jitter=0.2, seed=7, developed=True)
        return prm, parts, 1.0
    prm, parts = regime_cases.leftward_plain(cfgmod, geom, "small")
    return prm, parts, -1.0


def _seam_run(cfgmod, geom, capi, profmod, which, N=40):
    """The tracers of `which` case that the uploaded state and the first dt predict to cross the seam within N steps, by a factor
    of two in the travelled distance (x0 + u_x0 N dt0 / 2 beyond x = DL, leftward: below x = 0; computed on the CPU), recorded at
    the upload and after each of N steps, and the series unwrapped.  N = 40, the run length of the in-loop tests: a
    few rows either way on these states, in the core of the channel.  transport_coeff = 0: the transport shift moves a particle
    without a velocity (pass CD: x += shift + dt / 2 u_prev + dt / 2 u), so with it on a path is not the integral of the recorded
    velocity, and on a freshly jittered lattice the shift of a step can exceed u dt."""
    prm, parts, sign = _seam_case(cfgmod, geom, which)
    nf = parts["n_fluid"]
    kw = dict(t_end=1e9, transport_coeff=0.0)
    with capi.Context.from_parts(prm, parts, **kw) as ctx:
        dt0 = ctx.advance(1e9, max_steps=1)["dt_last"]
    x0, u0 = parts["pos"][:nf, 0], parts["vel"][:nf, 0]
    travel = u0 * N * dt0
    if sign > 0:
        ids = np.flatnonzero((u0 > 0) & (x0 + 0.5 * travel > prm.DL))
    else:
        ids = np.flatnonzero((u0 < 0) & (x0 + 0.5 * travel < 0.0))
    assert len(ids) >= 1, (which, len(ids))
    with capi.Context.from_parts(prm, parts, **kw) as ctx:
        ctx.tracers_enable(ids, every=1, capacity=N + 1)
        ctx.tracers_sample()                                   # record 0: the state as uploaded
        ctx.advance(1e9, max_steps=N)
        tr = ctx.tracers()
    assert len(tr["step"]) == N + 1 and tr["n_missing"] == 0 and tr["n_dropped"] == 0
    return prm, sign, ids, tr, profmod.unwrap_tracers(tr, prm.DL)


@pytest.mark.parametrize("which", ["rightward", "leftward"])
def test_the_seam(cfgmod, geom, capi, profmod, which):
    """Tracers that cross x = DL (leftward: x = 0) within the run: the recorded x drops (jumps up) by more than DL / 2, and the
    increments of unwrap_tracers' path are the trapezoid of the recorded velocities: a wrong image would be off by DL.

    The bound on |increment - 0.5 (u_prev + u) dt|: the drift of one step's acceleration, |u - u_prev| dt, from the recorded
    velocities, plus a rounding floor of 8 ulp of 2 DL (the step adds three terms to x, the unwrapping one more; a tracer whose
    velocity did not change has no other allowance)."""
    prm, sign, ids, tr, un = _seam_run(cfgmod, geom, capi, profmod, which)
    jump = np.diff(tr["x"], axis=0)
    crossed = np.any(-sign * jump > 0.5 * prm.DL, axis=0)
    print(f"{which}: {len(ids)} tracers, {int(crossed.sum())} crossed the seam")
    assert crossed.any()
    inc = np.diff(un["x_unwrapped"], axis=0)
    dt = np.diff(tr["t"])[:, None]
    trapezoid = 0.5 * (tr["u_x"][1:] + tr["u_x"][:-1]) * dt
    bound = np.abs(np.diff(tr["u_x"], axis=0)) * dt + 8 * np.spacing(2.0 * prm.DL)
    worst = float(np.max(np.abs(inc - trapezoid) / bound))
    print(f"{which}: worst |increment - trapezoid| / bound = {worst:.3e}")
    assert np.all(np.abs(inc - trapezoid) <= bound)
    assert np.array_equal(un["x_unwrapped"][0], tr["x"][0])
    images = (un["x_unwrapped"] - tr["x"]) / prm.DL
    assert np.all(np.abs(images - np.round(images)) < 1e-12) and set(np.unique(np.round(images))) <= {0.0, sign}


@pytest.mark.parametrize("which", ["rightward", "leftward"])
def test_the_seam_unwrapped_path_is_monotone(cfgmod, geom, capi, profmod, which):
    """The unwrapped x of every tracked tracer moves one way throughout.  (Not a property of every particle of these states:
    the jittered start rings acoustically, and over 80 steps a particle near the wall -- row 3 of the leftward state, y = 0.18 --
    was measured to have its velocity reversed, -0.60 at the upload and +0.217 after step 7, its path following its recorded
    velocity back and forth.  The rows the rule selects for 40 steps lie in the core.)"""
    prm, sign, ids, tr, un = _seam_run(cfgmod, geom, capi, profmod, which)
    inc = np.diff(un["x_unwrapped"], axis=0)
    for r, k in np.argwhere(~(sign * inc > 0.0))[:12]:
        print(f"{which}: not monotone at record {r + 1} tracer {k} (row {ids[k]}): x {tr['x'][r, k]!r} -> {tr['x'][r + 1, k]!r}, "
              f"u_x {tr['u_x'][r, k]!r} -> {tr['u_x'][r + 1, k]!r} (at the upload {tr['u_x'][0, k]!r}), y {tr['y'][r + 1, k]!r}")
    print(f"{which}: {int(np.count_nonzero(~(sign * inc > 0.0)))} of {inc.size} increments against the flow, in "
          f"{int(np.count_nonzero(np.any(~(sign * inc > 0.0), axis=0)))} of {len(ids)} tracers")
    assert np.all(sign * inc > 0.0), "x_unwrapped is not monotone"


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dp05_auto", "dp05_dynamic", "dp025_dual"])
def test_gating_every_and_t_from(cfgmod, geom, capi, name):
    prm, parts, kw = tc.case(make_case, cfgmod, geom, name)
    N, every = 26, 3
    ids = tc.id_sets(parts["n_fluid"])["65"]
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        statuses = [ctx.advance(1e9, max_steps=1) for _ in range(N)]
    t_from = statuses[4]["t"]                                  # t after step 5
    want = [s for s in statuses if s["step"] % every == 0 and s["t"] >= t_from]
    assert [s["step"] for s in want] == list(range(6, N + 1, 3))
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        check_kernel_form(ctx, name)
        ctx.tracers_enable(ids, every=every, t_from=t_from)
        ctx.history_enable(every=every, t_from=t_from)
        ctx.advance(1e9, max_steps=N)
        got, hist = ctx.tracers(), ctx.history()
    # (dual-rate: one record per outer step, the history's)
    assert got["step"].tolist() == [s["step"] for s in want] and got["t"].tolist() == [s["t"] for s in want]
    assert np.array_equal(got["step"], hist["step"]) and np.array_equal(got["t"], hist["t"])
    assert got["n_dropped"] == 0 and got["n_missing"] == 0 and got["u_x"].shape == (len(want), len(ids))


@pytest.mark.parametrize("T", ["1", "65"])
def test_full_buffer_drops_and_drain_resumes(cfgmod, geom, capi, T):
    prm, parts, kw = tc.case(make_case, cfgmod, geom, "dp05_auto")
    ids = tc.id_sets(parts["n_fluid"])[T]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.tracers_enable(ids, every=1, capacity=64)
        ctx.advance(1e9, max_steps=7)
        whole = ctx.tracers()
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.tracers_enable(ids, every=1, capacity=3)
        st = ctx.advance(1e9, max_steps=7)
        full = ctx.tracers()
        again = ctx.tracers()                                  # reading without drain changes nothing
        drained = ctx.tracers(drain=True)
        empty = ctx.tracers()
        st2 = ctx.advance(1e9, max_steps=2)
        ctx.tracers_sample()                                   # ungated: the state of the last step once more
        resumed = ctx.tracers()
        ctx.tracers_enable(ids[::-1].copy(), every=1, capacity=3)  # re-enable empties the buffer
        fresh = ctx.tracers()
    assert st["step"] == 7 and full["step"].tolist() == [1, 2, 3] and full["n_dropped"] == 4 and full["n_missing"] == 0
    for k in tc.SERIES:
        assert np.array_equal(full[k], whole[k][:3]), k        # the records below the capacity untouched by the dropped ones
    tc.assert_series_identical(full, again, "read twice")
    tc.assert_series_identical(full, drained, "read with drain")
    assert len(empty["step"]) == 0 and empty["n_dropped"] == 0 and empty["u_x"].shape == (0, len(ids))
    assert resumed["step"].tolist() == [8, 9, 9] and resumed["n_dropped"] == 0 and resumed["t"][-1] == st2["t"]
    for k in tc.FIELDS:
        assert np.array_equal(resumed[k][1], resumed[k][2]), k
    assert len(fresh["step"]) == 0 and fresh["n_dropped"] == 0 and np.array_equal(fresh["ids"], ids[::-1])


# 5 ---------------------------------------------------------------------------------------------------------------
def test_off_means_no_extra_launch(cfgmod, geom, capi):
    prm, parts, kw = tc.case(make_case, cfgmod, geom, "dp05_auto")
    ids = tc.id_sets(parts["n_fluid"])["65"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:  # steps 1-20 and 21-40: the same re-binning phases as below
        never = profiled_launches(ctx, 20)
        never2 = profiled_launches(ctx, 20)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.tracers_enable(ids, every=1)
        on = profiled_launches(ctx, 20)
        ctx.tracers_disable()
        off = profiled_launches(ctx, 20)
    assert "k_tracers" not in never and "k_tracers" not in never2 and "k_tracers" not in off
    assert on.pop("k_tracers") == 20
    assert on == never and off == never2


@pytest.mark.parametrize("name", ["dp05_auto", "dp025_walk", "dp05_dynamic"])
def test_no_feedback_on_the_physics(cfgmod, geom, capi, name):
    prm, parts, kw = tc.case(make_case, cfgmod, geom, name)
    ids = tc.id_sets(parts["n_fluid"])["all"]
    outs = {}
    for on in (False, True):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            if on:
                ctx.tracers_enable(ids, every=1, capacity=32)
            st = ctx.advance(1e9, max_steps=30)
            outs[on] = (st, ctx.download(fields=("pos", "vel", "drho_dt")))
            if on:
                tr = ctx.tracers()
                assert len(tr["step"]) == 30 and tr["n_missing"] == 0
    assert outs[True][0] == outs[False][0]
    for k in ("pos", "vel", "drho_dt"):
        assert np.array_equal(outs[True][1][k], outs[False][1][k]), k


def _others_on(ctx, prm):
    pts = np.array([(0.0, 0.5 * prm.DH), (0.5 * prm.DL, 0.25 * prm.DH), (0.7 * prm.DL, prm.DH)])
    ctx.flow_stats_enable(every=1)
    ctx.history_enable(every=1, capacity=64)
    ctx.field_map_enable(nx=31, ny=17, every=1, with_walls=True)
    ctx.probes_enable(pts, every=1, with_walls=True)
    ctx.profile_series_enable(every=1, capacity=64)
    ctx.pair_dist_enable(every=1)
    ctx.grad_stats_enable(every=1)


def _others_read(ctx):
    rec, dropped = ctx.history_records()
    out = dict(stats=ctx.flow_stats_sums(0), history=dict(records=rec, n_dropped=dropped), field=ctx.field_map_sums(), probes=ctx.probes(),
               series=ctx.profile_series_sums(), grads=ctx.grad_stats_sums(0))
    for b, band in enumerate(ctx.pair_dist_sums()):
        out[f"pairs{b}"] = band
    return out


def test_the_other_seven_samplers_are_unchanged(cfgmod, geom, capi):
    prm, parts, kw = tc.case(make_case, cfgmod, geom, "dp05_auto")
    ids = tc.id_sets(parts["n_fluid"])["300"]
    reads = {}
    for on in (False, True):
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            _others_on(ctx, prm)
            if on:
                ctx.tracers_enable(ids, every=1, capacity=32)
            ctx.advance(1e9, max_steps=20)
            reads[on] = _others_read(ctx)
            if on:
                assert len(ctx.tracers()["step"]) == 20
    n = 0
    for name, a in reads[False].items():
        for k, v in a.items():
            w = reads[True][name][k]
            assert np.asarray(v).tobytes() == np.asarray(w).tobytes(), (name, k)
            n += 1
    assert n > 40, n


# 6 ---------------------------------------------------------------------------------------------------------------
def test_repeatable(cfgmod, geom, capi):
    prm, parts, kw = tc.case(make_case, cfgmod, geom, "dp01_multi")
    ids = tc.id_sets(parts["n_fluid"])["all"]
    runs = []
    for _ in range(2):
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.tracers_enable(ids, every=4, capacity=8)
            ctx.advance(1e9, max_steps=20)
            runs.append(ctx.tracers())
    assert runs[0]["step"].tolist() == [4, 8, 12, 16, 20] and runs[0]["n_missing"] == 0
    tc.assert_series_identical(runs[0], runs[1], "dp01_multi")


def test_records_do_not_depend_on_recycled_memory():
    """tests/tracer_pool_worker.py in a fresh process of its own: a context and a batch of four, every fluid row tracked, observed
    as the first device work, after a foreign predecessor, after the pool was scrubbed and after a predecessor that ran into
    NaN -- the same bytes four times, every block of the later runs a recycled one.  A column nobody wrote would show here."""
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tracer_pool_worker.py")], cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"time limit of {CHILD_SECONDS} s\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
    assert r.returncode == 0, f"exit code {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    print(f"[tracer pool history] {out['n_arrays']} arrays, scrubbed {out['scrubbed']} blocks, hits / misses {out['deltas']}")
    assert out["n_arrays"] >= 9 * 5 and out["scrubbed"] > 0, out
    for h in ("foreign", "scrub3", "nan"):                        # not vacuous: every block of a later run had a previous owner
        assert out["deltas"][h]["misses"] == 0 and out["deltas"][h]["hits"] > 0, (h, out["deltas"])
    assert not any(out["differing"].values()), out["differing"]
    assert not out["failures"], out["failures"]


# 7 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, pkg):
    L = capi.lib()
    prm, parts, kw = tc.case(make_case, cfgmod, geom, "dp05_auto")
    nf, nt = parts["n_fluid"], parts["n_total"]
    nothing = (None, None, None, None, None, None, None, 0)
    good = [5, 0, nf - 1]

    def config(ids=good, **kw):
        arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        c = capi.SphxTracersConfig(n_tracers=0 if arr is None else len(arr), every=1, capacity=16, t_from=0.0,
                                   ids=None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int32)))
        for k, v in kw.items():
            setattr(c, k, v)
        return c, arr

    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        h = ctx._h
        assert err_id(capi, L.sphx_ctx_tracers_read, h, 0, *nothing) == ("SPHX:Tracers:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_ctx_tracers_sample, h) == ("SPHX:Tracers:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_ctx_tracers_disable(h) == capi.SPHX_OK      # a no-op when off
        with pytest.raises(capi.SphxError) as e:
            ctx.tracers()
        assert e.value.identifier == "SPHX:Tracers:disabled"
        ctx.tracers_enable(good, every=1, capacity=16)
        ctx.advance(1e9, max_steps=5)
        before = ctx.tracers()
        assert len(before["step"]) == 5
        nan, inf = float("nan"), float("inf")
        refused = [dict(ids=None, n_tracers=2), dict(n_tracers=0), dict(n_tracers=-1), dict(ids=[3, 7, 3]), dict(ids=[-1]), dict(ids=[nf]),
                   dict(ids=[nt - 1]), dict(ids=[nt]), dict(ids=[2 ** 31 - 1]), dict(every=0), dict(every=-1), dict(capacity=0),
                   dict(capacity=-5), dict(capacity=(1 << 27) // (3 * 4) + 1), dict(t_from=nan), dict(t_from=inf)]
        for bad in refused:
            c2, keep = config(**bad)
            assert err_id(capi, L.sphx_ctx_tracers_enable, h, C.byref(c2)) == ("SPHX:Tracers:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_ctx_tracers_enable, h, None) == ("SPHX:Tracers:config", capi.SPHX_ERR_ARG)
        for bad in (dict(ids=[1, 1]), dict(ids=[nf]), dict(ids=[nt - 1]), dict(ids=[]), dict(ids=good, every=0),
                    dict(ids=good, capacity=(1 << 27) // (3 * 4) + 1), dict(ids=[0.5])):
            with pytest.raises(capi.SphxError) as e:
                ctx.tracers_enable(**bad)
            assert e.value.identifier == "SPHX:Tracers:config", bad
        tc.assert_series_identical(ctx.tracers(), before, "a refused enable leaves the records as they were")
        ctx.advance(1e9, max_steps=2)
        assert ctx.tracers()["step"].tolist() == list(range(1, 8))         # ... and the sampler running
        n, nT, ids = C.c_int(0), C.c_int(0), np.full(3, -7, dtype=np.int32)
        assert L.sphx_ctx_tracers_read(h, 0, None, None, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nT), C.byref(n), None, None, 0) == capi.SPHX_OK
        assert (nT.value, n.value, ids.tolist()) == (3, 7, good)
        times, values = np.zeros((7, 2)), np.zeros((7, 3, 4))
        assert err_id(capi, L.sphx_ctx_tracers_read, h, 6, capi.ptr(times), None, None, None, None, None, None, 0)[0] == "SPHX:Tracers:capacity"
        assert err_id(capi, L.sphx_ctx_tracers_read, h, 6, None, capi.ptr(values), None, None, None, None, None, 1)[0] == "SPHX:Tracers:capacity"
        assert np.all(times == 0) and np.all(values == 0)
        assert L.sphx_ctx_tracers_read(h, 7, capi.ptr(times), capi.ptr(values), None, None, None, None, None, 0) == capi.SPHX_OK
        assert times[:, 0].tolist() == list(range(1, 8)) and np.array_equal(values[:, :, 2], ctx.tracers()["u_x"])   # nothing was drained
    eng = pkg.slab.HipSlabEngine(prm, parts, 0, 2, 0, t_end=1e9, native=True)
    try:
        cfg, keep = config()
        for fn, args in ((L.sphx_ctx_tracers_enable, (C.byref(cfg),)), (L.sphx_ctx_tracers_disable, ()), (L.sphx_ctx_tracers_sample, ()),
                         (L.sphx_ctx_tracers_read, (0, *nothing))):
            assert err_id(capi, fn, eng._h, *args) == ("SPHX:Tracers:slab", capi.SPHX_ERR_ARG)
    finally:
        eng.close()
