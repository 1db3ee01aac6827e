"""-m gpu: particle tracers of a batch (include/sphx.h section 2q) -- k_tracers_b records every member's series in one launch
per step slot.  Every member's series is bit for bit a standalone context's with the same config over the same steps, eager
and replayed (a tracer record is a copy: the layout decides which thread copies a particle, not what is copied), also for
members that fell out of step and were realigned, where both sides take the same steps (rebuild_every = 1, see
test_realigned_members_equal_standalone_contexts); on the default schedule realigned members record their own state -- a sample
equals the member's download byte for byte, the records up to the realignment equal a standalone context's; n_missing is 0 for
every member throughout; the error identifiers; driver.run_sweep's table columns and driver.run's drained
series."""
import ctypes as C

import numpy as np
import pytest

import tracer_cases as tc
from helpers import batch_members, err_id

pytestmark = pytest.mark.gpu

# four members that differ in mu (and in their seeds: every member follows its own particles)
VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=15.0, transport_coeff=0.30, seed=8),
            dict(mu=0.08, c_f=15.0, transport_coeff=0.30, seed=9), dict(mu=0.2, c_f=15.0, transport_coeff=0.30, seed=10)]


def _dt_members(cfgmod, geom):
    """four members in mu whose dt differ as well (c_f 15 / 21 / 11 / 18): they need different step counts to one target time,
    fall out of step and are realigned (tests/test_gpu_batch_probes.py)"""
    variants = [dict(v, c_f=c) for v, c in zip(VARIANTS, (15.0, 21.0, 11.0, 18.0))]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    return members, 10.3 * dt0, 17.9 * dt0


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ["1", "300", "all"])
def test_members_equal_standalone_contexts(cfgmod, geom, capi, T):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)
    kw = dict(t_end=1e9)
    ids = tc.id_sets(members[0][1]["n_fluid"])[T]
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
        assert K > 1
    n = 2 * K + 1  # crosses re-binnings
    cfg = dict(every=2, capacity=n)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.tracers_enable(ids, **cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            assert ctx.schedule()["rebins"] >= 2
            refs.append(ctx.tracers())
    assert all(r["step"].tolist() == list(range(2, n + 1, 2)) and r["n_dropped"] == 0 and r["n_missing"] == 0 for r in refs)
    assert len({r["x"].tobytes() for r in refs}) == len(members)     # a read from another member's block cannot pass
    for eager in (False, True):
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            b.tracers_enable(ids, **cfg)
            if eager:
                for _ in range(n):
                    sts = b.advance(1e9, max_steps=1)
                assert b.graph_stats()["slots_eager"] >= n
            else:
                sts = b.advance(1e9, max_steps=n)
                assert b.graph_stats()["slots_replayed"] > 0
            got = b.tracers()
            assert b.info()["realignments"] == 0
        for m in range(len(members)):
            assert sts[m]["step"] == n
            tc.assert_series_identical(got[m], refs[m], f"T={T} eager={eager} member {m}")


# 2 ---------------------------------------------------------------------------------------------------------------
def _realigned_run(cfgmod, geom, capi, rebuild_every=0):
    """the batch of _dt_members advanced to t1 and t2 with 300 tracers recorded at every step, sampled once more at the end, and
    every member's download; and the same calls on standalone contexts"""
    members, t1, t2 = _dt_members(cfgmod, geom)
    ids = tc.id_sets(members[0][1]["n_fluid"])["300"]
    kw = dict(t_end=1e9, lanes_per_particle=16, rebuild_every=rebuild_every)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.tracers_enable(ids, every=1, capacity=64)
        first = b.advance(t1)
        sts = b.advance(t2)
        assert b.info()["realignments"] >= 1
        got = b.tracers()
        b.tracers_sample()
        after = b.tracers()
        downs = [b.download(m, fields=("pos", "vel")) for m in range(len(members))]
    steps = [s["step"] for s in sts]
    assert len(set(steps)) == len(members), steps                    # every member on its own clock
    alone = []
    for m, (prm, parts) in enumerate(members):
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.tracers_enable(ids, every=1, capacity=64)
            ctx.advance(t1)
            st = ctx.advance(t2)
            alone.append(ctx.tracers())
        assert st["step"] == steps[m] == len(alone[m]["step"])
    return ids, [s["step"] for s in first], steps, got, after, downs, alone


def test_realigned_members_record_their_own_state(cfgmod, geom, capi, profmod):
    """The default schedule (re-binning every 16th step).  After the members fell out of step and were realigned every id is
    still met in exactly one slot (n_missing == 0), a sample equals the member's download byte for byte, and the records up to
    the first realignment are a standalone context's byte for byte.  Not the records after it: a realignment is a re-binning the
    standalone context never takes, it changes the order the member's neighbour sums are taken in, and from the next step on the
    member's STATE differs from the standalone's within rounding (include/sphx.h section 2b; tests/test_gpu_batch.py compares
    realigned members with the oracle at rtol 1e-9 for that reason).  Measured: the records after the realignment -- 8 of 19,
    11 of 26, 6 of 14, 9 of 22 -- differ by at most 8.9e-16 in x, 3.3e-16 in y, 3.1e-14 in u_x and 2.6e-14 in u_y."""
    ids, first, steps, got, after, downs, alone = _realigned_run(cfgmod, geom, capi)
    for m in range(len(steps)):
        assert got[m]["n_missing"] == 0 and after[m]["n_missing"] == 0 and got[m]["n_dropped"] == 0, m
        assert got[m]["step"].tolist() == list(range(1, steps[m] + 1)) and np.array_equal(got[m]["t"], alone[m]["t"]), m
        assert after[m]["step"].tolist() == got[m]["step"].tolist() + [steps[m]]
        tc.assert_record_is_state(after[m], -1, tc.state_rows(profmod, downs[m], ids), f"member {m}: sample after the realignment")
        for k in tc.FIELDS:                                            # the steps to t1: before any realignment
            assert np.array_equal(got[m][k][:first[m]], alone[m][k][:first[m]]), (m, k)


def test_realigned_members_equal_standalone_contexts(cfgmod, geom, capi, profmod):
    """Four members in mu that fall out of step and are realigned: each member's series equals a standalone context's over the
    same steps byte for byte, and n_missing == 0 for each member after the realignments.

    "The same steps" is the condition: a realignment re-bins every member at once, a step the standalone context does not have
    on a schedule that re-bins every K-th step (test_realigned_members_record_their_own_state has that case and its figures).
    With rebuild_every = 1 every step of either side ends with a re-binning, so a realignment re-bins a layout that is already
    binned -- the same slot order again -- and member and context do take the same steps.  The members still end the calls at
    different state parities, so the batch realigns them; the test asserts that it did."""
    ids, first, steps, got, after, downs, alone = _realigned_run(cfgmod, geom, capi, rebuild_every=1)
    for m in range(len(steps)):
        for k in tc.FIELDS:
            d = np.abs(got[m][k] - alone[m][k])
            rows = np.flatnonzero(np.any(d != 0.0, axis=1))
            print(f"member {m} {k}: {len(rows)} of {steps[m]} records differ" +
                  (f", the first is record {rows[0]} (the first realignment came after step {first[m]}), largest difference {d.max():.3e} "
                   f"of a largest |value| {np.abs(alone[m][k]).max():.3e}" if len(rows) else ""))
    for m in range(len(steps)):
        tc.assert_series_identical(got[m], alone[m], f"member {m}")
        assert after[m]["n_missing"] == 0 and after[m]["step"].tolist() == got[m]["step"].tolist() + [steps[m]], m
        tc.assert_record_is_state(after[m], -1, tc.state_rows(profmod, downs[m], ids), f"member {m}: sample after the realignments")


def test_members_out_of_step_keep_their_own_buffers(cfgmod, geom, capi):
    members, t1, t2 = _dt_members(cfgmod, geom)
    ids = tc.id_sets(members[0][1]["n_fluid"])["65"]
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
        b.tracers_enable(ids, every=1, capacity=5)
        b.history_enable(every=1)
        sts = b.advance(t2)
        steps = [s["step"] for s in sts]
        full, hist = b.tracers(), b.history()
        drained = b.tracers(drain=True)
        empty = b.tracers()
        sts2 = b.advance(1e9, max_steps=3)
        resumed = b.tracers()
    assert len(set(steps)) == len(members) and min(steps) > 5, steps
    for m in range(len(members)):
        assert full[m]["step"].tolist() == [1, 2, 3, 4, 5] and full[m]["n_dropped"] == steps[m] - 5 and full[m]["n_missing"] == 0, (m, steps)
        assert np.array_equal(full[m]["t"], hist[m]["t"][:5])          # its own clock
        tc.assert_series_identical(full[m], drained[m], f"member {m}: read with drain")
        assert len(empty[m]["step"]) == 0 and empty[m]["n_dropped"] == 0
        assert resumed[m]["step"].tolist() == [steps[m] + 1, steps[m] + 2, steps[m] + 3] and resumed[m]["n_dropped"] == 0
        assert resumed[m]["t"][-1] == sts2[m]["t"] and resumed[m]["n_missing"] == 0
    assert len({full[m]["t"].tobytes() for m in range(len(members))}) == len(members)


# 3 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:3])
    M = 3
    nf, nt = members[0][1]["n_fluid"], members[0][1]["n_total"]
    good = [5, 0, nf - 1]
    n, dropped, missing = np.full(M, -1, dtype=np.int32), np.full(M, -1, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    pn, pd, pm = n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64)), missing.ctypes.data_as(C.POINTER(C.c_int64))

    def config(ids=good, **kw):
        arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        c = capi.SphxTracersConfig(n_tracers=0 if arr is None else len(arr), every=1, capacity=16, t_from=0.0,
                                   ids=None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int32)))
        for k, v in kw.items():
            setattr(c, k, v)
        return c, arr

    ok, keep = config()
    for fn, args in ((L.sphx_batch_tracers_enable, (C.byref(ok),)), (L.sphx_batch_tracers_disable, ()), (L.sphx_batch_tracers_sample, ()),
                     (L.sphx_batch_tracers_read, (0, None, None, None, None, None, None, None, 0))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    cap_over = (1 << 27) // (M * 3 * 4) + 1                            # (the total over the members)
    refused = [dict(ids=None, n_tracers=2), dict(n_tracers=0), dict(ids=[3, 3]), dict(ids=[nf]), dict(ids=[nt - 1]), dict(ids=[-1]),
               dict(every=0), dict(capacity=0), dict(capacity=cap_over), dict(t_from=float("inf"))]
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        assert err_id(capi, L.sphx_batch_tracers_read, h, 0, None, None, None, None, pn, pd, pm, 0) == ("SPHX:Tracers:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_batch_tracers_sample, h) == ("SPHX:Tracers:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_batch_tracers_disable(h) == capi.SPHX_OK      # no-op when off
        assert L.sphx_batch_tracers_enable(h, C.byref(ok)) == capi.SPHX_OK
        b.advance(1e9, max_steps=5)
        for bad in refused:                                       # a refused enable leaves the running tracers and their records
            c2, keep2 = config(**bad)
            assert err_id(capi, L.sphx_batch_tracers_enable, h, C.byref(c2)) == ("SPHX:Tracers:config", capi.SPHX_ERR_ARG), bad
        with pytest.raises(capi.SphxError) as e:
            b.tracers_enable(good, capacity=cap_over)
        assert e.value.identifier == "SPHX:Tracers:config"
        assert L.sphx_batch_tracers_read(h, 0, None, None, None, None, pn, pd, pm, 0) == capi.SPHX_OK   # counts only: capacity is not checked
        assert list(n) == [5] * M and list(dropped) == [0] * M and list(missing) == [0] * M
        times, values = np.full((M, 4, 2), -1.0), np.full((M, 4, 3, 4), -1.0)
        assert err_id(capi, L.sphx_batch_tracers_read, h, 4, capi.ptr(times), capi.ptr(values), None, None, None, None, None, 1) == \
            ("SPHX:Tracers:capacity", capi.SPHX_ERR_ARG)
        assert np.all(times == -1.0) and np.all(values == -1.0)
        times, values = np.full((M, 7, 2), -1.0), np.full((M, 7, 3, 4), -1.0)      # nothing was drained; rows beyond n_records stay
        assert L.sphx_batch_tracers_read(h, 7, capi.ptr(times), capi.ptr(values), None, None, pn, None, None, 0) == capi.SPHX_OK
        for m in range(M):
            assert list(times[m, :5, 0]) == [1.0, 2.0, 3.0, 4.0, 5.0] and np.all(times[m, 5:] == -1.0) and np.all(values[m, 5:] == -1.0), m
        assert len({values[m, :5].tobytes() for m in range(M)}) == M  # each member's own particles


# 4 ---------------------------------------------------------------------------------------------------------------
def test_run_sweep_fills_the_tracer_columns(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, transport_coeff=tc_, end_time=0.04, output_interval=0.02) for tc_ in (0.1, 0.2)]
    res = driver.run_sweep(prms, history_capacity=256, tracers=64, tracers_every=2, tracers_capacity=256)
    for m, r in enumerate(res.members):
        p, h = r.tracers, r.history
        assert p["n_dropped"] == 0 and p["n_missing"] == 0 and p["step"].tolist() == list(range(2, r.steps + 1, 2)), m   # no gap across the drains
        assert np.array_equal(p["t"], h["t"][1::2]) and p["x"].shape == (r.steps // 2, 64)
        assert np.array_equal(p["ids"], driver.tracer_ids(64, r.n_fluid))
    for k in ("D_y_nu", "y_drift", "u_dev_rms"):
        assert res.table[k].shape == (2,) and np.all(np.isfinite(res.table[k])), (k, res.table[k])
    print({k: res.table[k].tolist() for k in ("transport_coeff", "D_y_nu", "y_drift", "u_dev_rms")})
    assert len({r.tracers["y"].tobytes() for r in res.members}) == 2
    none = driver.run_sweep(prms, history_capacity=256)
    assert all(r.tracers is None for r in none.members) and "D_y_nu" not in none.table
    with pytest.raises(RuntimeError, match=r"member 0.*tracers_capacity >= \d+ \(it is 4\)"):
        driver.run_sweep(prms, history_capacity=256, tracers=64, tracers_capacity=4)


def test_driver_run_returns_one_contiguous_series(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.02, output_interval=0.01)
    every = 3
    res = driver.run(prm, tracers=16, tracers_every=every)
    p = res.tracers
    assert res.steps > 2 * every and len(p["step"]) == res.steps // every and p["n_dropped"] == 0 and p["n_missing"] == 0
    assert p["step"].tolist() == list(range(every, res.steps + 1, every)) and np.all(np.diff(p["t"]) > 0) and p["t"][-1] <= res.t
    assert p["x"].shape == (len(p["step"]), 16) and np.array_equal(p["ids"], driver.tracer_ids(16, res.n_fluid))
    assert np.all((p["x"] >= 0.0) & (p["x"] < prm.DL)) and np.all((p["y"] > 0.0) & (p["y"] < prm.DH))
    if res.steps % every == 0:                                    # the last record is the final state's rows
        assert np.array_equal(p["x"][-1], res.pos[p["ids"], 0]) and np.array_equal(p["u_y"][-1], res.vel[p["ids"], 1])
    fig = driver.tracer_figures(prm, p, y_margin=0.0)
    assert fig["n_records"] == len(p["step"]) and np.isfinite(fig["D_y_nu"]) and np.isfinite(fig["u_dev_rms"])
    assert driver.run(prm).tracers is None
    need = int(np.searchsorted(p["t"], 0.01 + 1e-12))            # the records of the first output interval
    assert need > 2
    with pytest.raises(RuntimeError, match=rf"tracers_capacity >= {need} \(it is 2\)"):
        driver.run(prm, tracers=16, tracers_every=every, tracers_capacity=2)
