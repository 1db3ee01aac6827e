"""-m gpu: flow statistics and step history of a slab ring (include/sphx.h section 3a; k_flow_stats_s, k_step_history_s), on
in-process rings (sphx_slab_group_run) on device 0.  A slab samples the particles it owns and keeps partial sums; the ring's
value is their sum.  Checked against numpy's binning of the owned particles of the snapshots (one sample, exact), against a
single context of the same state sampling every step (sums, counts bin for bin, every field of the history), for the gating,
for leaving the ring's state bit for bit as it is without them -- in the chain, the two-stream and the replayed-graph form of
the step -- and for the error identifiers."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from helpers import HISTORY_FIELDS, STATS_FIELDS, err_id, make_case, make_variant, stats_bands

pytestmark = pytest.mark.gpu

# every ring: developed=True, jitter=0.2, seed=11, as tests/test_slab.py::test_slab_native_ring_in_one_process -- but case e, seed
# 12: with seed 11 one of its 60 000 particles passes within 1e-7 DL of a band edge at steps 10, 12 and 22, which the guard of
# the count comparison (_guard) does not allow; seeds 12, 14 and 17 keep clear, 13, 15 and 16 do not
CASES = {
    "a": dict(world=2, dp=0.05, DL=3.0, calls=[27]),                            # crosses the scheduled re-binning at K = 24
    "b": dict(world=3, dp=0.05, DL=4.5, calls=[23], leftward=True, kw=dict(rebuild_every=4)),  # ownership migrates left, x < 0
    "c": dict(world=2, dp=0.05, DL=3.0, calls=[5, 18, 1, 1, 2], overlap="always"),  # the two-stream form of the step
    "d": dict(world=2, dp=0.05, DL=3.0, calls=[3, 25, 19], graph_after=0),      # replays of the step graph carry the samplers
    "e": dict(world=4, dp=0.01, DL=6.0, calls=[26], seed=12),                   # ~15 k fluid particles per slab: several workgroups
}


@pytest.fixture(scope="module")
def slab(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".slab")


_made = {}


def _case(cfgmod, geom, name):
    if name not in _made:
        c = CASES[name]
        common = dict(dp=c["dp"], DL=c["DL"], jitter=0.2, seed=c.get("seed", 11), developed=True, end_time=1e9)
        if c.get("leftward"):
            prm, parts = make_variant(cfgmod, geom, U_bulk=-0.666667, top_ux=-0.8, bottom_ux=0.3, rho0=2.5, transport_coeff=0.1,
                                      **common)
            assert prm.gravity_g < 0
        else:
            prm, parts = make_case(cfgmod, geom, **common)
        _made[name] = (prm, parts)
    return _made[name]


@contextlib.contextmanager
def _ring(slab, prm, parts, name):
    """The engines of case `name`'s ring; SPHX_SLAB_OVERLAP is read when a slab's buffers are made (the first group_run)."""
    c = CASES[name]
    env_before = os.environ.pop("SPHX_SLAB_OVERLAP", None)
    if c.get("overlap"):
        os.environ["SPHX_SLAB_OVERLAP"] = c["overlap"]
    engines = []
    try:
        engines = [slab.HipSlabEngine(prm, parts, r, c["world"], 0, t_end=1e9, native=True, **c.get("kw", {}))
                   for r in range(c["world"])]
        yield engines
    finally:
        for e in engines:
            e.close()
        os.environ.pop("SPHX_SLAB_OVERLAP", None)
        if env_before is not None:
            os.environ["SPHX_SLAB_OVERLAP"] = env_before


def _run(slab, engines, name, calls=None):
    c = CASES[name]
    for k, n in enumerate(c["calls"] if calls is None else calls):
        slab.HipSlabEngine.group_run(engines, n)
        if calls is None and c.get("graph_after") == k:
            slab.HipSlabEngine.graph_prepare(engines)
    return [e.sync() for e in engines]


def _steps(name):
    return sum(CASES[name]["calls"])


def _last_step_rebinned(capi, eng):
    """The clock's drift is exactly zero behind a step that ended with a re-binning (read by sync())."""
    d = C.c_double(-1.0)
    capi.check(capi.lib().sphx_ctx_grid_policy(eng._h, None, None, None, C.byref(d)))
    return d.value == 0.0


def _numpy_sums(pos, vel, prm, n_bins, band=None):  # (tests/test_gpu_flow_stats.py)
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
    return dict(zip(STATS_FIELDS, [np.bincount(k, weights=w, minlength=n_bins).astype(np.float64)
                                   for w in (np.ones_like(ux), ux, ux * ux, uy, uy * uy)]))


def _sums_deviation(got, want):
    """max |got - want| over the four velocity sums, as a fraction of the largest |sum| of the band"""
    scale = max(max(float(np.max(np.abs(want[f]))) for f in STATS_FIELDS[1:]), 1e-300)
    return max(float(np.max(np.abs(got[f] - want[f]))) for f in STATS_FIELDS[1:]) / scale


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_one_sample_is_numpys_binning_of_the_owned_particles(cfgmod, geom, capi, profmod, slab, name):
    prm, parts = _case(cfgmod, geom, name)
    nf, steps = parts["n_fluid"], _steps(name)
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    bands = stats_bands(prm)
    with _ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.flow_stats_enable(every=steps, bands=bands)  # only the last step is sampled
        sts = _run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        per_rank = [[e.flow_stats_sums(b) for b in range(3)] for e in engines]
        rebinned = _last_step_rebinned(capi, engines[0])
    owned = [(np.column_stack([s["x"][s["owned"]], s["y"][s["owned"]]]), np.column_stack([s["vx"][s["owned"]], s["vy"][s["owned"]]]))
             for s in snaps]
    pos, vel = np.vstack([o[0] for o in owned]), np.vstack([o[1] for o in owned])
    assert len(pos) == nf
    inside = (pos[:, 1] >= 0.0) & (pos[:, 1] <= prm.DH)
    for b, band in enumerate([None] + bands):
        got = slab.pool_ring_sums([r[b] for r in per_rank])
        want = _numpy_sums(pos, vel, prm, n_bins, band)  # (x taken mod DL in there)
        assert np.array_equal(got["count"], want["count"]), f"{name} band {b}: counts"
        dev = _sums_deviation(got, want)
        print(f"{name} band {b}: sums off by {dev:.3e} of the largest |sum|")
        assert dev <= 1e-12, f"{name} band {b}"
        for r in per_rank:
            assert r[b]["n_samples"] == 1 and r[b]["t_first"] == r[b]["t_last"] == sts[0]["t"]
    assert sum(r[0]["count"].sum() for r in per_rank) == nf - int((~inside).sum())
    if not rebinned:  # (a re-binning in the last step hands particles over behind the sample: the snapshot then shows the new owners)
        for r, (p, _) in zip(per_rank, owned):
            assert r[0]["count"].sum() == int(((p[:, 1] >= 0.0) & (p[:, 1] <= prm.DH)).sum())


# 2, 3: one ring and one reference context per case, both samplers on every step ----------------------------------------
_every_step = {}


def _guard(prm, pos, bands, n_bins, what):
    """No fluid particle within 1e-7 DH of a bin edge or within 1e-7 DL of a band edge: the ring's state agrees with the context's
    to 1e-9 per particle, so every particle falls into the same bin and band on both."""
    bw = prm.DH / n_bins
    r = pos[:, 1] / bw
    k = np.round(r)
    near = (k >= 0) & (k <= n_bins) & (np.abs(r - k) * bw < 1e-7 * prm.DH)
    assert not near.any(), f"{what}: {int(near.sum())} particles within 1e-7 DH of a bin edge"
    for xc, hw in bands:
        d = np.abs(np.mod(pos[:, 0], prm.DL) - xc)
        d = np.minimum(d, prm.DL - d)
        near = np.abs(d - hw) < 1e-7 * prm.DL
        assert not near.any(), f"{what}: {int(near.sum())} particles within 1e-7 DL of a band edge"


def _reference(cfgmod, geom, capi, profmod, name):
    """The single context of case `name`: flow statistics and history of every step, and (a second pass, step by step) the guard."""
    prm, parts = _case(cfgmod, geom, name)
    nf, steps = parts["n_fluid"], _steps(name)
    bands = stats_bands(prm)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.flow_stats_enable(every=1, bands=bands)
        ctx.history_enable(every=1)
        ctx.advance(1e9, max_steps=steps)
        out = dict(sums=[ctx.flow_stats_sums(b) for b in range(3)], hist=ctx.history())
    guard = None
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
        try:
            for k in range(steps):
                ctx.advance(1e9, max_steps=1)
                _guard(prm, ctx.download(fields=("pos",))["pos"][:nf], bands, n_bins, f"{name} step {k + 1}")
        except AssertionError as e:
            guard = str(e)
    out["guard"] = guard
    return out


def _both(cfgmod, geom, capi, profmod, slab, name):
    if name not in _every_step:
        prm, parts = _case(cfgmod, geom, name)
        with _ring(slab, prm, parts, name) as engines:
            for e in engines:  # (before the first call: the replays of case d carry the samplers)
                e.flow_stats_enable(every=1, bands=stats_bands(prm))
                e.history_enable(every=1)
            sts = _run(slab, engines, name)
            ring = dict(sums=[slab.pool_ring_sums([e.flow_stats_sums(b) for e in engines]) for b in range(3)],
                        records=[e.history_records() for e in engines], status=sts)
            ring["hist"] = slab.pool_ring_history(ring["records"])
            ring["profile"] = slab.ring_flow_stats(engines, band=1)
            ring["drained"] = slab.ring_history(engines, drain=True)
            ring["after_drain"] = [e.history_records() for e in engines]
            slab.HipSlabEngine.group_run(engines, 2)  # (eagerly: two more records, from index 0 of the emptied buffers)
            for e in engines:
                e.sync()
            ring["two_more"] = [e.history_records() for e in engines]
        _every_step[name] = (ring, _reference(cfgmod, geom, capi, profmod, name))
    return _every_step[name]


@pytest.mark.parametrize("name", list(CASES))
def test_sums_of_every_step_match_a_single_context(cfgmod, geom, capi, profmod, slab, name):
    ring, ref = _both(cfgmod, geom, capi, profmod, slab, name)
    prm, _ = _case(cfgmod, geom, name)
    steps = _steps(name)
    assert ref["guard"] is None, ref["guard"]  # (the case's seed keeps every particle clear of the edges at every sampled step)
    for b in range(3):
        got, want = ring["sums"][b], ref["sums"][b]
        assert got["n_samples"] == want["n_samples"] == steps
        assert abs(got["t_first"] - want["t_first"]) <= 1e-12 * want["t_first"]
        assert abs(got["t_last"] - want["t_last"]) <= 1e-12 * want["t_last"]
        dev = _sums_deviation(got, want)
        print(f"{name} band {b}: ring against context, sums off by {dev:.3e} of the largest |sum|")
        assert np.array_equal(got["count"], want["count"]), f"{name} band {b}: counts"
        assert dev <= 1e-8, f"{name} band {b}"
    prof = ring["profile"]
    ok = ring["sums"][1]["count"] > 0
    assert np.array_equal(prof["count"], ring["sums"][1]["count"])
    np.testing.assert_allclose(prof["u_mean"][ok], ring["sums"][1]["sum_ux"][ok] / ring["sums"][1]["count"][ok], rtol=1e-14)


@pytest.mark.parametrize("name", list(CASES))
def test_history_of_every_step_matches_a_single_context(cfgmod, geom, capi, profmod, slab, name):
    ring, ref = _both(cfgmod, geom, capi, profmod, slab, name)
    steps = _steps(name)
    got, want = ring["hist"], ref["hist"]
    for rec, dropped in ring["records"]:
        assert len(rec) == steps and dropped == 0
        assert np.array_equal(rec[:, :4], ring["records"][0][0][:, :4])  # the clock's fields: the same on every rank
    assert np.array_equal(got["step"], want["step"]) and np.array_equal(got["step"], np.arange(1, steps + 1))
    assert np.max(np.abs(got["t"] - want["t"]) / want["t"]) <= 1e-12
    for k in ("dt", "vmax"):
        assert np.max(np.abs(got[k] - want[k]) / np.abs(want[k])) <= 1e-9, k
    dev = {k: float(np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k]))) for k in HISTORY_FIELDS[4:]}
    print(f"{name}: ring against context, largest deviation by the series' largest magnitude: "
          + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    for k in ("kinetic_energy", "u_bulk"):
        assert dev[k] <= 1e-8, k
    tau_scale = max(np.max(np.abs(want["tau_bottom"])), np.max(np.abs(want["tau_top"])))
    for k in ("tau_bottom", "tau_top"):
        assert np.max(np.abs(got[k] - want[k])) <= 1e-7 * tau_scale, k
    # drain=True handed out the same records and emptied every slab's buffer; later records start at index 0
    assert all(np.array_equal(ring["drained"][k], got[k]) for k in HISTORY_FIELDS)
    for (rec, dropped), (more, _) in zip(ring["after_drain"], ring["two_more"]):
        assert len(rec) == 0 and dropped == 0
        assert np.array_equal(more[:, 0], [steps + 1, steps + 2])


def test_history_capacity_and_drops_are_per_slab(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.history_enable(every=1, capacity=10)
        _run(slab, engines, "a")
        recs = [e.history_records() for e in engines]
    for rec, dropped in recs:
        assert len(rec) == 10 and dropped == 17
        assert np.array_equal(rec[:, 0], np.arange(1, 11))


# 4 ---------------------------------------------------------------------------------------------------------------
def test_gating_samples_the_steps_a_context_samples(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    steps = _steps("a")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.flow_stats_enable(every=5, t_from=t_from)
        ctx.history_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        want, want_h = ctx.flow_stats_sums(0), ctx.history()
    assert want["n_samples"] == 3  # steps 15, 20, 25
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.flow_stats_enable(every=5, t_from=t_from)
            e.history_enable(every=5, t_from=t_from)
        _run(slab, engines, "a")
        got, got_h = slab.ring_flow_stats(engines), slab.ring_history(engines)
    assert got["n_samples"] == want["n_samples"]
    assert abs(got["t_first"] - want["t_first"]) <= 1e-12 * want["t_first"] and abs(got["t_last"] - want["t_last"]) <= 1e-12 * want["t_last"]
    assert np.array_equal(got_h["step"], want_h["step"]) and np.array_equal(got_h["step"], [15, 20, 25])


def _state_bits(snaps):
    return [tuple(s[k].tobytes() for k in ("x", "y", "vx", "vy", "drho", "id", "owned")) for s in snaps]


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_samplers_leave_the_ring_bit_for_bit(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form."""
    prm, parts = _case(cfgmod, geom, name)
    bits = []
    for on in (False, True):
        with _ring(slab, prm, parts, name) as engines:
            if on:
                for e in engines:
                    e.flow_stats_enable(every=1, bands=stats_bands(prm))
                    e.history_enable(every=1)
            _run(slab, engines, name)
            bits.append(_state_bits([e.snapshot() for e in engines]))
    assert bits[0] == bits[1]


def test_captured_and_eager_forms_give_the_same_bits(cfgmod, geom, capi, profmod, slab):
    """Case d (replays of the step graph) against the same calls without graph_prepare: sums and records bit for bit."""
    ring, _ = _both(cfgmod, geom, capi, profmod, slab, "d")
    prm, parts = _case(cfgmod, geom, "d")
    with _ring(slab, prm, parts, "d") as engines:
        for e in engines:
            e.flow_stats_enable(every=1, bands=stats_bands(prm))
            e.history_enable(every=1)
        _run(slab, engines, "d", calls=CASES["d"]["calls"])  # (explicit calls: no graph)
        sums = [slab.pool_ring_sums([e.flow_stats_sums(b) for e in engines]) for b in range(3)]
        records = [e.history_records() for e in engines]
    for b in range(3):
        for k in STATS_FIELDS + ("n_samples", "t_first", "t_last"):
            assert np.array_equal(sums[b][k], ring["sums"][b][k]), (b, k)
    for (rec, _), (want, _) in zip(records, ring["records"]):
        assert np.array_equal(rec, want)


def test_disable_run_enable_starts_from_zero(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.flow_stats_enable(every=1)
            e.history_enable(every=1)
        slab.HipSlabEngine.group_run(engines, 5)
        for e in engines:  # (no sync in between: disable waits for the slab's streams itself)
            e.flow_stats_disable()
            e.history_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.flow_stats_enable(every=1)
            e.history_enable(every=1)
        slab.HipSlabEngine.group_run(engines, 3)
        first = slab.pool_ring_sums([e.flow_stats_sums() for e in engines])  # (no sync either: the read waits)
        hist = slab.ring_history(engines)
        for e in engines:
            e.flow_stats_reset()
        empty = slab.pool_ring_sums([e.flow_stats_sums() for e in engines])
        for e in engines:
            e.sync()
    assert first["n_samples"] == 3 and first["count"].sum() > 0
    assert np.array_equal(hist["step"], [10, 11, 12])
    assert empty["n_samples"] == 0 and empty["count"].sum() == 0 and np.isnan(empty["t_first"])


# 5 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    L = capi.lib()
    scfg, hcfg = capi.flow_stats_config(), capi.history_config()
    n, nb, dr = C.c_int(0), C.c_int(0), C.c_int64(0)

    def calls(h):
        return [(L.sphx_slab_flow_stats_enable, h, C.byref(scfg)), (L.sphx_slab_flow_stats_disable, h), (L.sphx_slab_flow_stats_reset, h),
                (L.sphx_slab_flow_stats_read, h, 0, 0, C.byref(nb), None, None, None, None, None, None, None, None),
                (L.sphx_slab_history_enable, h, C.byref(hcfg)), (L.sphx_slab_history_disable, h),
                (L.sphx_slab_history_read, h, 0, None, C.byref(n), C.byref(dr), 0)]

    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        for call in calls(ctx._h):
            assert err_id(capi, *call) == ("SPHX:Slab:ctx", capi.SPHX_ERR_ARG), call[0].__name__
    # a slab of the caller-driven protocol (rebuild_every = 1), on a stream of the library's own
    h, f = C.c_void_p(), capi.f64
    params = capi.make_params(prm, 1e9, None, 0, 0, 1, 0.0)
    capi.check(L.sphx_slab_create(C.byref(h), C.byref(params), C.c_int(parts["n_fluid"]), C.c_int(parts["n_total"]),
                                  *[capi.ptr(f(parts[k])) for k in ("pos", "vel", "drho_dt", "mass", "wall_vel")], C.c_double(0.0),
                                  C.c_int64(0), C.c_int(0), C.c_int(2), C.c_int(slab.HALO_COLS), None))
    try:
        for call in calls(h):
            assert err_id(capi, *call) == ("SPHX:Slab:protocol", capi.SPHX_ERR_ARG), call[0].__name__
    finally:
        L.sphx_ctx_destroy(h)
    with _ring(slab, prm, parts, "a") as engines:
        e = engines[0]
        h = e._h
        assert err_id(capi, L.sphx_slab_flow_stats_read, h, 0, 0, C.byref(nb), None, None, None, None, None, None, None, None) == \
            ("SPHX:Stats:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_slab_flow_stats_reset, h) == ("SPHX:Stats:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_slab_history_read, h, 0, None, C.byref(n), C.byref(dr), 0) == ("SPHX:History:disabled", capi.SPHX_ERR_STATE)
        for fn, want in ((e.flow_stats_sums, "SPHX:Stats:disabled"), (e.flow_stats_reset, "SPHX:Stats:disabled"),
                         (e.history_records, "SPHX:History:disabled")):
            with pytest.raises(capi.SphxError) as ei:
                fn()
            assert ei.value.identifier == want
        assert L.sphx_slab_flow_stats_disable(h) == capi.SPHX_OK and L.sphx_slab_history_disable(h) == capi.SPHX_OK  # (off already)
        # a bad config, band or capacity: the identifiers of sections 2a / 2d, from the library and from the binding's own checks
        bad = capi.SphxFlowStatsConfig(n_bins=0, every=0, t_from=0.0, n_bands=0)
        assert err_id(capi, L.sphx_slab_flow_stats_enable, h, C.byref(bad)) == ("SPHX:Stats:config", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_slab_flow_stats_enable, h, None) == ("SPHX:Stats:config", capi.SPHX_ERR_ARG)
        badh = capi.SphxHistoryConfig(every=1, capacity=0, t_from=0.0)
        assert err_id(capi, L.sphx_slab_history_enable, h, C.byref(badh)) == ("SPHX:History:config", capi.SPHX_ERR_ARG)
        for fn, kw, want in ((e.flow_stats_enable, dict(every=0), "SPHX:Stats:config"), (e.flow_stats_enable, dict(n_bins=800, bands=[(1.0, 0.1)]), "SPHX:Stats:config"),
                             (e.history_enable, dict(capacity=0), "SPHX:History:config"), (e.history_enable, dict(t_from=float("inf")), "SPHX:History:config")):
            with pytest.raises(capi.SphxError) as ei:
                fn(**kw)
            assert ei.value.identifier == want
        e.flow_stats_enable(bands=[(1.0, 0.1)])
        e.history_enable()
        slab.HipSlabEngine.group_run(engines, 3)
        assert err_id(capi, L.sphx_slab_flow_stats_read, h, 2, 0, C.byref(nb), None, None, None, None, None, None, None, None) == \
            ("SPHX:Stats:band", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as ei:
            e.flow_stats_sums(2)
        assert ei.value.identifier == "SPHX:Stats:band"
        small = np.zeros(4)
        assert err_id(capi, L.sphx_slab_flow_stats_read, h, 0, 4, C.byref(nb), capi.ptr(small), None, None, None, None, None, None, None) == \
            ("SPHX:Stats:capacity", capi.SPHX_ERR_ARG)
        rec = np.zeros((2, 8))
        assert err_id(capi, L.sphx_slab_history_read, h, 2, capi.ptr(rec), C.byref(n), C.byref(dr), 0) == ("SPHX:History:capacity", capi.SPHX_ERR_ARG)
        # the context's calls keep refusing a slab
        assert err_id(capi, L.sphx_ctx_flow_stats_enable, h, C.byref(scfg)) == ("SPHX:Stats:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_flow_stats_read, h, 0, 0, C.byref(nb), None, None, None, None, None, None, None, None) == \
            ("SPHX:Stats:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_history_enable, h, C.byref(hcfg)) == ("SPHX:History:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_history_read, h, 0, None, C.byref(n), C.byref(dr), 0) == ("SPHX:History:slab", capi.SPHX_ERR_ARG)
        for x in engines:
            x.sync()
        assert e.flow_stats_sums(1)["n_samples"] == 3 and len(e.history_records()[0]) == 3
