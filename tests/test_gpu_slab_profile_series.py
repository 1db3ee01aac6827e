"""-m gpu: the profile series of a slab ring (include/sphx.h section 3a; k_profile_series_s, sphx_slab_pseries_*), on in-process
rings (sphx_slab_group_run) on device 0, over the ring cases of tests/test_gpu_slab_samplers.py.  A slab records the sample of
the particles it owns, a PARTIAL record; the ring's record is the slabs' added up.  Checked against numpy's binning of the owned
particles of the snapshots (one record, counts exact), against a single context of the same state recording every step,
against the slab's own flow statistics (the records added in order ARE its sums, to the bit), for the gating, for leaving the
ring and the other samplers bit for bit as they are -- in the chain, the two-stream and the replayed-graph form of the step --
for the record buffer (capacity, drain, no stale contents, disable / enable), the error identifiers, and against the start-up
of plane Poiseuille flow from rest with a band on the cut between two slabs."""
import ctypes as C

import numpy as np
import pytest

import profile_series_cases as sc
import test_gpu_slab_samplers as rings  # the ring cases, their engines and calls, the guard: used as they are
from helpers import HISTORY_FIELDS, STATS_FIELDS, err_id, stats_bands

pytestmark = pytest.mark.gpu

CASES = rings.CASES


@pytest.fixture(scope="module")
def slab(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".slab")


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_one_record_is_numpys_binning_of_the_owned_particles(cfgmod, geom, profmod, slab, name):
    prm, parts = rings._case(cfgmod, geom, name)
    nf, steps = parts["n_fluid"], rings._steps(name)
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    bands = stats_bands(prm)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.profile_series_enable(every=steps, bands=bands)  # only the last step is recorded
        sts = rings._run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        per_rank = [e.profile_series_sums() for e in engines]
    for s in per_rank:  # every slab: exactly one record, of the last step
        assert s["count"].shape == (1, 3, n_bins) and s["n_dropped"] == 0
        assert s["step"].tolist() == [steps] and s["t"].tolist() == [sts[0]["t"]]
    pos = np.vstack([np.column_stack([s["x"][s["owned"]], s["y"][s["owned"]]]) for s in snaps])
    vel = np.vstack([np.column_stack([s["vx"][s["owned"]], s["vy"][s["owned"]]]) for s in snaps])
    assert len(pos) == nf
    got = slab.pool_ring_profile_series(per_rank)
    for b, band in enumerate([None] + bands):
        sc.assert_record_matches(got, 0, b, sc.numpy_sums(pos, vel, prm, n_bins, band), f"{name} band {b}")  # (x taken mod DL in there)
    inside = (pos[:, 1] >= 0.0) & (pos[:, 1] <= prm.DH)
    assert got["count"][0, 0].sum() == int(inside.sum())


# 2, 6: one ring and one reference context per case, the series of every step -------------------------------------------
_rings, _refs = {}, {}


def _reference(cfgmod, geom, capi, profmod, name):
    """The single context of case `name`'s state: its series of every step and (a second pass, step by step) the guard."""
    c = CASES[name]
    steps = rings._steps(name)
    key = (c["dp"], c["DL"], c.get("seed", 11), bool(c.get("leftward")), steps)  # (cases a and c: one state, one reference)
    if key not in _refs:
        prm, parts = rings._case(cfgmod, geom, name)
        nf, bands = parts["n_fluid"], stats_bands(prm)
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.profile_series_enable(every=1, bands=bands, capacity=steps)
            ctx.advance(1e9, max_steps=steps)
            out = dict(series=ctx.profile_series_sums())
        guard = None
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
            try:
                for k in range(steps):
                    ctx.advance(1e9, max_steps=1)
                    rings._guard(prm, ctx.download(fields=("pos",))["pos"][:nf], bands, n_bins, f"{name} step {k + 1}")
            except AssertionError as e:
                guard = str(e)
        out["guard"] = guard
        _refs[key] = out
    return _refs[key]


def _every_step(cfgmod, geom, slab, name):
    if name not in _rings:
        prm, parts = rings._case(cfgmod, geom, name)
        with rings._ring(slab, prm, parts, name) as engines:
            for e in engines:  # (before the first call: the replays of case d carry the launch)
                e.profile_series_enable(every=1, bands=stats_bands(prm), capacity=rings._steps(name))
            sts = rings._run(slab, engines, name)
            per_rank = [e.profile_series_sums() for e in engines]
            _rings[name] = dict(status=sts, per_rank=per_rank, pooled=slab.ring_profile_series_sums(engines))
    return _rings[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_record_matches_a_single_context(cfgmod, geom, capi, profmod, slab, name):
    ring, ref = _every_step(cfgmod, geom, slab, name), _reference(cfgmod, geom, capi, profmod, name)
    steps = rings._steps(name)
    for s in ring["per_rank"]:  # every slab: all the steps, none dropped, the clock's columns bit for bit
        assert len(s["step"]) == steps and s["n_dropped"] == 0
        assert np.array_equal(s["step"], ring["per_rank"][0]["step"]) and np.array_equal(s["t"], ring["per_rank"][0]["t"])
    got, want = ring["pooled"], ref["series"]
    sc.assert_series_identical(got, slab.pool_ring_profile_series(ring["per_rank"]), f"{name}: ring_profile_series_sums")
    assert np.array_equal(got["step"], want["step"]) and np.array_equal(got["step"], np.arange(1, steps + 1))
    assert np.max(np.abs(got["t"] - want["t"]) / want["t"]) <= 1e-12 and got["t"][-1] == ring["status"][0]["t"]
    assert ref["guard"] is None, ref["guard"]  # (the case's seed keeps every particle clear of the edges at every step)
    assert np.array_equal(got["count"], want["count"]), f"{name}: counts"
    for b in range(3):
        scale = max(max(float(np.max(np.abs(want[f][:, b]))) for f in STATS_FIELDS[1:]), 1e-300)
        dev = max(float(np.max(np.abs(got[f][:, b] - want[f][:, b]))) for f in STATS_FIELDS[1:]) / scale
        print(f"{name} band {b}: ring against context, records off by {dev:.3e} of the largest |sum| of the series")
        assert dev <= 1e-8, f"{name} band {b}"


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("name", ["a", "e"])
def test_records_of_a_slab_add_up_to_its_flow_statistics_bit_for_bit(cfgmod, geom, slab, name, every):
    prm, parts = rings._case(cfgmod, geom, name)
    bands, steps = stats_bands(prm), rings._steps(name)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.flow_stats_enable(every=every, bands=bands)
            e.profile_series_enable(every=every, bands=bands, capacity=steps)
        rings._run(slab, engines, name)
        series = [e.profile_series_sums() for e in engines]
        stats = [[e.flow_stats_sums(b) for b in range(3)] for e in engines]
    for r, (s, st) in enumerate(zip(series, stats)):
        assert len(s["step"]) == steps // every and s["n_dropped"] == 0
        for b in range(3):
            assert st[b]["n_samples"] == steps // every
            assert (st[b]["t_first"], st[b]["t_last"]) == (s["t"][0], s["t"][-1])
            total = sc.running_sums(s, b)
            for f in sc.FIELDS:
                assert np.array_equal(total[f], st[b][f]), f"{name} every {every} rank {r} band {b}: {f}"


# 4 ---------------------------------------------------------------------------------------------------------------
def test_gating_records_the_steps_a_context_records(cfgmod, geom, capi, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    steps = rings._steps("a")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.profile_series_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        want = ctx.profile_series_sums()
    assert want["step"].tolist() == [15, 20, 25]
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.profile_series_enable(every=5, t_from=t_from)
        rings._run(slab, engines, "a")
        got = [e.profile_series_sums() for e in engines]
    for s in got:
        assert s["step"].tolist() == [15, 20, 25] and s["n_dropped"] == 0
        assert np.max(np.abs(s["t"] - want["t"]) / want["t"]) <= 1e-12


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_the_ring_and_the_other_samplers_do_not_feel_it(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form; flow
    statistics and history are on in both runs."""
    prm, parts = rings._case(cfgmod, geom, name)
    bands, steps = stats_bands(prm), rings._steps(name)
    runs = []
    for on in (False, True):
        with rings._ring(slab, prm, parts, name) as engines:
            for e in engines:
                e.flow_stats_enable(every=1, bands=bands)
                e.history_enable(every=1)
                if on:
                    e.profile_series_enable(every=1, bands=bands, capacity=steps)
            rings._run(slab, engines, name)
            runs.append(dict(bits=rings._state_bits([e.snapshot() for e in engines]),
                             sums=[[e.flow_stats_sums(b) for b in range(3)] for e in engines],
                             hist=[e.history_records() for e in engines]))
            if on:
                assert all(len(e.profile_series_sums()["step"]) == steps for e in engines)
    off, on = runs
    assert off["bits"] == on["bits"]
    for r in range(len(off["sums"])):
        for b in range(3):
            for k in STATS_FIELDS + ("n_samples", "t_first", "t_last"):
                assert np.array_equal(off["sums"][r][b][k], on["sums"][r][b][k]), (r, b, k)
        assert off["hist"][r][1] == on["hist"][r][1] == 0 and off["hist"][r][0].shape == (steps, len(HISTORY_FIELDS))
        assert np.array_equal(off["hist"][r][0], on["hist"][r][0]), r


# 6 ---------------------------------------------------------------------------------------------------------------
def test_replayed_graph_and_eager_form_give_the_same_bits(cfgmod, geom, slab):
    """Case d (replays of the step graph) against the same calls without graph_prepare: every slab's series and the pooled one."""
    ring = _every_step(cfgmod, geom, slab, "d")
    prm, parts = rings._case(cfgmod, geom, "d")
    with rings._ring(slab, prm, parts, "d") as engines:
        for e in engines:
            e.profile_series_enable(every=1, bands=stats_bands(prm), capacity=rings._steps("d"))
        rings._run(slab, engines, "d", calls=CASES["d"]["calls"])  # (explicit calls: no graph)
        per_rank = [e.profile_series_sums() for e in engines]
        pooled = slab.ring_profile_series_sums(engines)
    assert len(pooled["step"]) == rings._steps("d")
    sc.assert_series_identical(pooled, ring["pooled"], "pooled")
    for r, (got, want) in enumerate(zip(per_rank, ring["per_rank"])):
        sc.assert_series_identical(got, want, f"rank {r}")


# 7 ---------------------------------------------------------------------------------------------------------------
def test_capacity_drops_and_drain_are_per_slab(cfgmod, geom, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.profile_series_enable(every=1, bands=stats_bands(prm), capacity=10)
        rings._run(slab, engines, "a")  # 27 steps
        full = [e.profile_series_sums() for e in engines]
        again = [e.profile_series_sums(drain=True) for e in engines]
        empty = [e.profile_series_sums() for e in engines]
        slab.HipSlabEngine.group_run(engines, 2)
        more = [e.profile_series_sums() for e in engines]
        for e in engines:
            e.sync()
    for r, (f, a, em, m) in enumerate(zip(full, again, empty, more)):
        assert f["step"].tolist() == list(range(1, 11)) and f["n_dropped"] == 17
        sc.assert_series_identical(f, a, f"rank {r}: drain=True hands out the same records")
        assert len(em["step"]) == 0 and em["n_dropped"] == 0 and em["count"].shape == (0, 3, f["count"].shape[2])
        assert m["step"].tolist() == [28, 29] and m["n_dropped"] == 0  # (from index 0 of the emptied buffer)


def test_stale_contents_never_show(cfgmod, geom, capi, slab):
    """tests/test_gpu_profile_series.py::test_stale_contents_never_show on a ring: the record buffer is never cleared, the old one
    goes back to the pool at disable and is filled with NaN words there, so a counter that was not written would show."""
    prm, parts = rings._case(cfgmod, geom, "a")
    bands = stats_bands(prm)
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.profile_series_enable(every=1, n_bins=200, bands=bands, capacity=4)
        slab.HipSlabEngine.group_run(engines, 4)
        assert all(len(e.profile_series_sums()["step"]) == 4 for e in engines)
        for e in engines:
            e.profile_series_disable()
        assert capi.pool_scrub(0xFFFFFFFF) >= 1
        for e in engines:
            e.profile_series_enable(every=1, n_bins=100, bands=bands, capacity=4)
        slab.HipSlabEngine.group_run(engines, 2)
        got = [e.profile_series_sums() for e in engines]
    with rings._ring(slab, prm, parts, "a") as engines:  # a ring that enabled late
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.profile_series_enable(every=1, n_bins=100, bands=bands, capacity=64)
        slab.HipSlabEngine.group_run(engines, 2)
        want = [e.profile_series_sums() for e in engines]
    for r, (g, w) in enumerate(zip(got, want)):
        assert g["step"].tolist() == [5, 6] and g["count"].shape == (2, 3, 100)
        assert all(np.all(np.isfinite(g[f])) for f in sc.FIELDS)
        assert np.any(g["count"] == 0)  # (zeros that had to be stored)
        sc.assert_series_identical(g, w, f"rank {r}: after re-enabling with fewer bins")


def test_disable_run_enable_starts_from_the_current_step(cfgmod, geom, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.profile_series_enable(every=1)
        slab.HipSlabEngine.group_run(engines, 5)
        for e in engines:  # (no sync in between: disable waits for the slab's streams itself)
            e.profile_series_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.profile_series_enable(every=1)
        before = [e.profile_series_sums() for e in engines]
        slab.HipSlabEngine.group_run(engines, 3)
        after = [e.profile_series_sums() for e in engines]  # (no sync either: the read waits)
        for e in engines:
            e.sync()
    for b, a in zip(before, after):
        assert len(b["step"]) == 0 and b["n_dropped"] == 0
        assert a["step"].tolist() == [10, 11, 12] and a["n_dropped"] == 0 and a["count"][:, 0].sum() > 0


# 8 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    L = capi.lib()
    cfg = capi.SphxProfileSeriesConfig(n_bins=0, every=1, capacity=16, t_from=0.0, n_bands=0)
    n, nb, nbd, dr = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    nothing = (None, None, None, None, None, None, 0)

    def calls(h):
        return [(L.sphx_slab_pseries_enable, h, C.byref(cfg)), (L.sphx_slab_pseries_disable, h), (L.sphx_slab_pseries_read, h, 0, *nothing)]

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
    with rings._ring(slab, prm, parts, "a") as engines:
        e = engines[0]
        h = e._h
        assert err_id(capi, L.sphx_slab_pseries_read, h, 0, *nothing) == ("SPHX:ProfileSeries:disabled", capi.SPHX_ERR_STATE)
        with pytest.raises(capi.SphxError) as ei:
            e.profile_series_sums()
        assert ei.value.identifier == "SPHX:ProfileSeries:disabled"
        assert L.sphx_slab_pseries_disable(h) == capi.SPHX_OK  # (off already)
        e.profile_series_disable()
        # a bad config: the identifiers of section 2j, from the library and from the binding's own checks
        assert err_id(capi, L.sphx_slab_pseries_enable, h, None) == ("SPHX:ProfileSeries:config", capi.SPHX_ERR_ARG)
        for bad in (dict(every=0), dict(capacity=0)):
            c2 = capi.SphxProfileSeriesConfig(**dict(dict(n_bins=0, every=1, capacity=16, t_from=0.0, n_bands=0), **bad))
            assert err_id(capi, L.sphx_slab_pseries_enable, h, C.byref(c2)) == ("SPHX:ProfileSeries:config", capi.SPHX_ERR_ARG), bad
        for kw in (dict(every=0), dict(capacity=0), dict(n_bins=800, bands=[(1.0, 0.1)])):
            with pytest.raises(capi.SphxError) as ei:
                e.profile_series_enable(**kw)
            assert ei.value.identifier == "SPHX:ProfileSeries:config"
        for x in engines:
            x.profile_series_enable(every=1, capacity=16)
        slab.HipSlabEngine.group_run(engines, 7)
        before = e.profile_series_sums()
        bad = capi.SphxProfileSeriesConfig(n_bins=0, every=0, capacity=16, t_from=0.0, n_bands=0)
        assert err_id(capi, L.sphx_slab_pseries_enable, h, C.byref(bad)) == ("SPHX:ProfileSeries:config", capi.SPHX_ERR_ARG)
        sc.assert_series_identical(e.profile_series_sums(), before, "a refused enable leaves the records as they were")
        # the shape-only read, and arrays that are too small
        assert L.sphx_slab_pseries_read(h, 0, None, None, C.byref(nb), C.byref(nbd), C.byref(n), C.byref(dr), 0) == capi.SPHX_OK
        assert (nb.value, nbd.value, n.value, dr.value) == (20, 1, 7, 0)
        times, records = np.zeros((7, 2)), np.zeros((7, 1, 20, 5))
        assert err_id(capi, L.sphx_slab_pseries_read, h, 6, capi.ptr(times), None, None, None, None, None, 0) == \
            ("SPHX:ProfileSeries:capacity", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_slab_pseries_read, h, 6, None, capi.ptr(records), None, None, None, None, 1) == \
            ("SPHX:ProfileSeries:capacity", capi.SPHX_ERR_ARG)
        assert np.all(times == 0) and np.all(records == 0)
        assert L.sphx_slab_pseries_read(h, 7, capi.ptr(times), capi.ptr(records), None, None, None, None, 0) == capi.SPHX_OK
        assert times[:, 0].tolist() == list(range(1, 8)) and np.array_equal(records[:, 0, :, 1], before["sum_ux"][:, 0])
        # the context's calls keep refusing a slab
        assert err_id(capi, L.sphx_ctx_profile_series_enable, h, C.byref(cfg)) == ("SPHX:ProfileSeries:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_profile_series_read, h, 0, *nothing) == ("SPHX:ProfileSeries:slab", capi.SPHX_ERR_ARG)
        for x in engines:
            x.sync()
        assert len(e.profile_series_sums()["step"]) == 7


# 9 ---------------------------------------------------------------------------------------------------------------
def _advance_ring(slab, engines, prm, t_target):
    """group_run to t_target: whole batches while at least that many steps certainly remain (no dt exceeds dt_upper_bound),
    then singly -- a step enqueued behind the target would be an overrun."""
    hint = slab.dt_upper_bound(prm)
    st = engines[0].sync()
    while st["t"] < t_target - 1e-12:
        n = max(1, min(int((t_target - st["t"]) / hint) - 1, 256))
        slab.HipSlabEngine.group_run(engines, n, t_target)
        st = [e.sync() for e in engines][0]
    return st


def test_the_ring_follows_the_startup_transient(cfgmod, geom, profmod, driver, slab):
    """One ring of two slabs from rest: dp = 0.05, DL = 3.0, to t = 1.0, every 5th step, band 1 centred on the cut between the
    slabs (the left edge of rank 1's first cell column, half-width max(dp, h)), so both slabs fill it.  The condition is
    tests/test_gpu_profile_series.py::test_the_series_follows_the_startup_transient's, for band 0 and band 1: at the records
    nearest t = 0.25, 0.5 and 1.0 the pooled profile is closer to the start-up solution than half the distance between that
    solution and the steady parabola (both relative L2 by profile.l2_error's rule).  A condition, not a measured bar.
    The reference physics meets it: the oracle's stepper (oracle/) on the same case, DL = 3.0 (the ring's 20 cell columns put
    the cut at x = 1.5; half-width 0.065), binned with profile.compute_binned_profile_mean / compute_mid_channel_profile at
    t = 0.25, 0.5, 1.0 (233, 468, 945 steps), gives L2_startup = 0.00810, 0.00499, 0.01030 over the whole channel and 0.00810,
    0.00499, 0.02065 in the band, where half the distance is 0.390, 0.305, 0.186.  Up to t = 0.5 these are the figures of DL = 1
    (0.0081, 0.0050: the flow from rest is x-invariant); at t = 1.0 the lattice has begun to break up, and the band's few
    particles per bin scatter more than the whole channel's 60."""
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=1.0)
    parts = geom.init_particles(prm)
    engines = []
    try:
        engines = [slab.HipSlabEngine(prm, parts, r, 2, 0, t_end=1e9, native=True) for r in range(2)]
        # the cut: the left edge of rank 1's first cell column, by slab.partition's arithmetic on the ring's own cell columns --
        # a skinned slab's columns are 2h + skin wide, so there are fewer of them than slab.n_cell_columns(prm) (20, not 23)
        lay = engines[1].layout()
        ncx = lay["col1"]
        assert ncx <= slab.n_cell_columns(prm) and slab.partition(ncx, 2)[1] == (lay["col0"], ncx)
        x_cut = lay["col0"] * (prm.DL / ncx)
        bands = [(x_cut, max(prm.dp, prm.h))]
        print(f"{ncx} cell columns, x_cut = {x_cut}, half-width {bands[0][1]}")
        for e in engines:
            e.profile_series_enable(every=5, bands=bands)
        st = _advance_ring(slab, engines, prm, 1.0)
        per_rank = [e.profile_series_sums() for e in engines]
        s = slab.ring_profile_series(engines)
    finally:
        for e in engines:
            e.close()
    assert abs(st["t"] - 1.0) <= 1e-12
    assert len(s["step"]) == st["step"] // 5 and s["n_dropped"] == 0 and np.array_equal(s["step"], 5 * np.arange(1, len(s["step"]) + 1))
    for p in per_rank:  # both slabs hold particles of the band on their cut, at every record
        assert np.all(p["count"][:, 1].sum(axis=1) > 0)
    y = s["y_mid"]
    u_exact = prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y)
    for band in (0, 1):
        fig = driver.profile_series_figures(prm, s, band=band)
        print(f"band {band}: steps {st['step']}, records {len(s['step'])}, tau_fit / tau_exact = {fig['tau_fit'] / fig['tau_exact']:.4f}, "
              f"t_developed = {fig['t_developed']}")
        for t_want in (0.25, 0.5, 1.0):
            r = int(np.argmin(np.abs(s["t"] - t_want)))
            start = profmod.poiseuille_startup(y, np.array([s["t"][r]]), prm.gravity_g, prm.nu, prm.DH)[:, 0]
            gap = profmod.l2_error(start, u_exact)
            print(f"band {band}, t = {s['t'][r]:.6f} (step {s['step'][r]}): L2_startup = {fig['L2_startup'][r]:.5f}, "
                  f"L2_steady = {fig['L2_steady'][r]:.5f}, half the distance to the parabola = {0.5 * gap:.5f}")
            assert abs(s["t"][r] - t_want) < 0.01
            assert fig["L2_startup"][r] < 0.5 * gap
