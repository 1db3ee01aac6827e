"""-m gpu: point probes of a batch (include/sphx.h section 2i) -- k_point_probes_b records every member's series in one
launch per step slot.  Every member's times and values are bit for bit a standalone context's with the same config, eager
and replayed, with one probe and with 300; members that fall out of step carry their own step / t series and their own
n_dropped; after a realignment the records agree up to summation order; the error identifiers; driver.run_sweep."""
import ctypes as C

import numpy as np
import pytest

import probe_cases as pc
from helpers import batch_members, err_id

pytestmark = pytest.mark.gpu

VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=17.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=13.0, transport_coeff=0.30, seed=9)]
SIZES = {"dp05": (0.05, 3.0, dict()), "dp025_lpp16": (0.025, 1.5, dict(lanes_per_particle=16))}


def _points(capi, prm, parts, P, kw):
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        return pc.point_sets(prm, pc.cell_geometry(prm, parts, ctx), parts["pos"][:parts["n_fluid"]])[P]


def _dt_members(cfgmod, geom):
    """members whose dt differ (c_f 15 / 21 / 11): they need different step counts to one target time"""
    variants = [dict(VARIANTS[0], c_f=15.0), dict(VARIANTS[1], c_f=21.0), dict(VARIANTS[2], c_f=11.0)]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    return members, 10.3 * dt0, 17.9 * dt0


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ["one", "300"])
@pytest.mark.parametrize("size", list(SIZES))
def test_members_equal_standalone_contexts(cfgmod, geom, capi, size, P):
    dp, DL, opts = SIZES[size]
    members = batch_members(cfgmod, geom, dp, DL, VARIANTS)
    kw = dict(t_end=1e9, **opts)
    pts = _points(capi, *members[0], P, opts)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
        assert K > 1
    n = 2 * K + 1  # crosses re-binnings
    with capi.Context.from_parts(*members[0], **kw) as ctx:
        t_early = ctx.advance(1e9, max_steps=4)["t"]
    cfg = dict(every=2, capacity=64, t_from=t_early, with_walls=True)   # (3 members x 300 points: the default 65 536 is over the total)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.probes_enable(pts, **cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            assert ctx.schedule()["rebins"] >= 2
            refs.append(ctx.probes())
    assert refs[0]["step"].tolist() == list(range(4, n + 1, 2))      # (the other members reach t_from at steps of their own)
    assert all(0 < len(r["step"]) < n // 2 + 1 and np.all(r["step"] % 2 == 0) and r["n_dropped"] == 0 for r in refs)
    # a read from another member's block cannot pass: the members' series are far apart
    for a in range(3):
        for c in range(a + 1, 3):
            k = min(len(refs[a]["step"]), len(refs[c]["step"]))
            assert np.all(np.abs(refs[a]["u_x"][-k:] - refs[c]["u_x"][-k:]) > 1e-6 * np.abs(refs[c]["u_x"][-k:]) + 1e-12), (a, c)
    for eager in (False, True):
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            b.probes_enable(pts, **cfg)
            if eager:
                for _ in range(n):
                    sts = b.advance(1e9, max_steps=1)
                assert b.graph_stats()["slots_eager"] >= n
            else:
                sts = b.advance(1e9, max_steps=n)
                assert b.graph_stats()["slots_replayed"] > 0
            got = b.probes()
            assert b.info()["realignments"] == 0
        for m in range(3):
            assert sts[m]["step"] == n
            pc.assert_series_identical(got[m], refs[m], f"{size} P={P} eager={eager} member {m}")


# 2 ---------------------------------------------------------------------------------------------------------------
def test_members_out_of_step_keep_their_own_series(cfgmod, geom, capi):
    members, t1, t2 = _dt_members(cfgmod, geom)
    pts = pc.random_points(members[0][0], 40, 3)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.probes_enable(pts, every=1, capacity=5)
        b.history_enable(every=1)
        sts = b.advance(t2)
        assert b.info()["realignments"] >= 1
        steps = [s["step"] for s in sts]
        full, hist = b.probes(), b.history()
        drained = b.probes(drain=True)
        empty = b.probes()
        sts2 = b.advance(1e9, max_steps=3)
        resumed = b.probes()
    assert len(set(steps)) == 3 and min(steps) > 5, steps
    for m in range(3):
        assert full[m]["step"].tolist() == [1, 2, 3, 4, 5] and full[m]["n_dropped"] == steps[m] - 5, (m, steps)
        assert np.array_equal(full[m]["t"], hist[m]["t"][:5])          # its own clock
        pc.assert_series_identical(full[m], drained[m], f"member {m}: read with drain")
        assert len(empty[m]["step"]) == 0 and empty[m]["n_dropped"] == 0
        assert resumed[m]["step"].tolist() == [steps[m] + 1, steps[m] + 2, steps[m] + 3] and resumed[m]["n_dropped"] == 0
        assert resumed[m]["t"][-1] == sts2[m]["t"]
    assert len({full[m]["t"].tobytes() for m in range(3)}) == 3


def test_after_a_realignment_the_records_agree(cfgmod, geom, capi):
    members, t1, t2 = _dt_members(cfgmod, geom)
    pts = _points(capi, *members[0], "300", dict(lanes_per_particle=16))
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.probes_enable(pts, every=1, capacity=256, with_walls=True)
        b.advance(t1)
        sts = b.advance(t2)
        assert b.info()["realignments"] >= 1
        got = b.probes()
    for m, (prm, parts) in enumerate(members):
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.probes_enable(pts, every=1, capacity=256, with_walls=True)
            ctx.advance(t1)
            st = ctx.advance(t2)
            want = ctx.probes()
        assert st["step"] == sts[m]["step"] == len(want["step"])
        pc.assert_series_close(got[m], want, f"member {m}")


# 3 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)
    M = 3
    good = np.array([[0.5, 0.5], [1.0, 0.25]])
    n, dropped = np.full(M, -1, dtype=np.int32), np.full(M, -1, dtype=np.int64)
    pn, pd = n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64))

    def config(points=good, **kw):
        pts = None if points is None else np.ascontiguousarray(points, dtype=np.float64)
        c = capi.SphxProbesConfig(n_points=0 if pts is None else len(pts), every=1, capacity=16, with_walls=0, t_from=0.0,
                                  points=capi.ptr(pts))
        for k, v in kw.items():
            setattr(c, k, v)
        return c, pts

    ok, keep = config()
    for fn, args in ((L.sphx_batch_probes_enable, (C.byref(ok),)), (L.sphx_batch_probes_disable, ()), (L.sphx_batch_probes_sample, ()),
                     (L.sphx_batch_probes_read, (0, None, None, None, None, None, 0))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    refused = [dict(points=None, n_points=2), dict(n_points=0), dict(n_points=4097), dict(points=[[float("nan"), 0.5]]),
               dict(points=[[0.5, 1.5]]), dict(every=0), dict(capacity=0), dict(capacity=(1 << 24) // M + 1),  # (the total over the members)
               dict(t_from=float("inf")), dict(with_walls=2)]
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        assert err_id(capi, L.sphx_batch_probes_read, h, 0, None, None, None, pn, pd, 0) == ("SPHX:Probe:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_batch_probes_sample, h) == ("SPHX:Probe:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_batch_probes_disable(h) == capi.SPHX_OK       # no-op when off
        assert L.sphx_batch_probes_enable(h, C.byref(ok)) == capi.SPHX_OK
        b.advance(1e9, max_steps=5)
        for bad in refused:                                       # a refused enable leaves the running probes and their records
            c2, keep2 = config(**bad)
            assert err_id(capi, L.sphx_batch_probes_enable, h, C.byref(c2)) == ("SPHX:Probe:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_batch_probes_enable, h, None) == ("SPHX:Probe:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            b.probes_enable(good, capacity=(1 << 24) // M + 1)
        assert e.value.identifier == "SPHX:Probe:config"
        assert L.sphx_batch_probes_read(h, 0, None, None, None, pn, pd, 0) == capi.SPHX_OK   # counts only: capacity is not checked
        assert list(n) == [5] * M and list(dropped) == [0] * M
        times, values = np.full((M, 4, 2), -1.0), np.full((M, 4, 2, 4), -1.0)
        assert err_id(capi, L.sphx_batch_probes_read, h, 4, capi.ptr(times), capi.ptr(values), None, None, None, 1) == \
            ("SPHX:Probe:capacity", capi.SPHX_ERR_ARG)
        assert np.all(times == -1.0) and np.all(values == -1.0)
        times, values = np.full((M, 7, 2), -1.0), np.full((M, 7, 2, 4), -1.0)      # nothing was drained; rows beyond n_records stay
        assert L.sphx_batch_probes_read(h, 7, capi.ptr(times), capi.ptr(values), None, pn, None, 0) == capi.SPHX_OK
        for m in range(M):
            assert list(times[m, :5, 0]) == [1.0, 2.0, 3.0, 4.0, 5.0] and np.all(times[m, 5:] == -1.0) and np.all(values[m, 5:] == -1.0), m
            assert np.all(values[m, :5, :, 0] > 0.8)
        assert len({values[m, :5, :, 1].tobytes() for m in range(M)}) == M  # each member's own u_x


# 4 ---------------------------------------------------------------------------------------------------------------
def test_run_sweep_sets_the_members_probes(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.04, output_interval=0.02) for mu in (0.1, 0.15, 0.2)]
    pts = [(0.0, 0.5), (1.5, 0.25), (prms[0].DL, 1.0)]
    res = driver.run_sweep(prms, history_capacity=256, probe_points=pts, probe_every=2, probe_capacity=256)
    for m, r in enumerate(res.members):
        p, h = r.probes, r.history
        assert p["n_dropped"] == 0 and p["step"].tolist() == list(range(2, r.steps + 1, 2)), m   # no gap across the drains
        assert np.array_equal(p["t"], h["t"][1::2]) and p["u_x"].shape == (r.steps // 2, 3)
        assert np.array_equal(p["points"][:, 0], [0.0, 1.5, 0.0])
        fig = driver.probe_figures(prms[m], p)
        assert fig["n_records"] == r.steps // 2 and np.all(np.isfinite(fig["u_x_mean"]))
    assert len({r.probes["u_x"].tobytes() for r in res.members}) == 3
    assert all(r.probes is None for r in driver.run_sweep(prms, history_capacity=256).members)
    with pytest.raises(RuntimeError, match=r"member 0.*probe_capacity >= \d+ \(it is 4\)"):
        driver.run_sweep(prms, history_capacity=256, probe_points=pts, probe_capacity=4)
