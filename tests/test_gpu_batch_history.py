"""-m gpu: the step history of batches (include/sphx.h section 2f, k_step_history_b) -- one record per member and step
(step, t, dt, vmax, tau_bottom, tau_top, kinetic_energy, u_bulk) written inside the batch's step loop.  A member's records
must be bit for bit those of a standalone context with the same config; they are checked step by step against the oracle's
loop and against the host path they replace (status / monitor() / numpy over download()); idle members record nothing; every
member has its own buffer bounds; the physics is untouched; toggling re-captures the graphs; the history and the batch's flow
statistics do not see each other; two runs give the same bits; the C ABI names its errors; the debug switches that move the
Vol / B buffers and the clock update (fresh child processes, tests/batch_history_worker.py); driver.run_sweep."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_history_matches_oracle, batch_members, err_id, make_case, oracle_history_rows, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("step", "t", "dt", "vmax", "tau_bottom", "tau_top", "kinetic_energy", "u_bulk")
STATS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2")
VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=17.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=13.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]
# (dp, DL): k_step_history_b runs ceil(n_fluid / 2048) workgroups per member (as k_step_history per context)
SIZES = {
    "one_workgroup": (0.05, 3.0),      # 1 200 fluid particles: one workgroup writes a member's record (no ticket)
    "three_workgroups": (0.025, 3.0),  # 4 800 (C2): three workgroups per member, partials + a ticket per member
}


def _dt_members(cfgmod, geom):
    """members whose dt differ (c_f 15 / 21 / 11): they need different step counts to one target time"""
    variants = [dict(VARIANTS[0], c_f=15.0), dict(VARIANTS[1], c_f=21.0), dict(VARIANTS[2], c_f=11.0)]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    return members, 10.3 * dt0, 17.9 * dt0


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpp", [16, 32])
@pytest.mark.parametrize("size", list(SIZES))
def test_members_equal_standalone_contexts(cfgmod, geom, capi, size, lpp):
    dp, DL = SIZES[size]
    members = batch_members(cfgmod, geom, dp, DL, VARIANTS)
    nf = members[0][1]["n_fluid"]
    assert -(-nf // 2048) == (1 if size == "one_workgroup" else 3)
    kw = dict(t_end=1e9, lanes_per_particle=lpp)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
        assert b.info()["lanes_per_particle"] == lpp and K > 1
    n = 3 * K + 1  # crosses re-binnings
    with capi.Context.from_parts(*members[0], **kw) as ctx:
        t_mid = ctx.advance(1e9, max_steps=n // 2)["t"]
    cfg = dict(every=3, t_from=t_mid)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.history_enable(**cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            assert ctx.schedule()["rebins"] >= 2
            refs.append(ctx.history())
    assert all(0 < len(r["step"]) < n // 3 + 1 and r["n_dropped"] == 0 for r in refs)
    # a read from another member's block cannot pass: the members' series are far apart
    for a in range(len(members)):
        for c in range(a + 1, len(members)):
            k = min(len(refs[a]["step"]), len(refs[c]["step"]))
            assert k > 0 and np.all(rel_err(refs[a]["tau_bottom"][:k], refs[c]["tau_bottom"][:k]) > 1e-3), (a, c)
    for eager in (False, True):
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            b.history_enable(**cfg)
            if eager:
                for _ in range(n):
                    sts = b.advance(1e9, max_steps=1)
                assert b.graph_stats()["slots_eager"] >= n
            else:
                sts = b.advance(1e9, max_steps=n)
                assert b.graph_stats()["slots_replayed"] > 0
            got = b.history()
            assert b.info()["realignments"] == 0
        for m in range(len(members)):
            what = f"{size} lpp={lpp} eager={eager} member {m}"
            assert sts[m]["step"] == n and got[m]["n_dropped"] == 0, what
            for k in FIELDS:
                assert np.array_equal(got[m][k], refs[m][k]), f"{what}: {k}"


# 2 ---------------------------------------------------------------------------------------------------------------
def test_series_match_the_oracle_step_by_step(cfgmod, geom, capi, oracle):
    n = 12
    members = [make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=21, developed=True, mu=0.1),
               make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=22, developed=True, mu=0.15, U_bulk=-0.666667),
               make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=23, developed=True, mu=0.07)]
    assert members[1][0].gravity_g < 0
    want = [oracle_history_rows(oracle, prm, parts, n) for prm, parts in members]
    for w in want:
        # from one step to the next every field moves by far more than the tolerances: a record taken a step early or late fails
        assert np.all(np.abs(np.diff(w[:, 1:], axis=0)) >= 1e-6 * np.abs(w[1:, 1:]))
    assert np.all(want[1][:, 4:6] < 0) and np.all(want[1][:, 7] < 0)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, rebuild_every=4) as b:
        assert b.info()["rebuild_every"] == 4
        b.history_enable(every=1)
        sts = b.advance(1e9, max_steps=n)
        got = b.history()
        info, gs = b.info(), b.graph_stats()
        print("batch:", info, gs)
    # every K-th slot of the batch's schedule re-bins, and a realignment only starts the count again with a re-binning of
    # its own: the slots the batch took hold at least two re-binning slots, so both Vol / B lookups are reached
    slots = gs["slots_replayed"] + gs["slots_eager"]
    assert slots >= n and (slots - 1) // info["rebuild_every"] >= 2, (slots, info)
    for m in range(3):
        assert sts[m]["step"] == n
        assert_history_matches_oracle(got[m], want[m], f"member {m}")
    assert np.all(got[1]["tau_bottom"] < 0) and np.all(got[1]["tau_top"] < 0) and np.all(got[1]["u_bulk"] < 0)


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_last_record_is_what_the_host_path_reports(cfgmod, geom, capi, size):
    dp, DL = SIZES[size]
    members = batch_members(cfgmod, geom, dp, DL, VARIANTS[:3])
    nf = members[0][1]["n_fluid"]
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.history_enable(every=1)
        sts = b.advance(1e9, max_steps=45)
        got = b.history()
        mons = [b.monitor(m, tau=True) for m in range(3)]
        vels = [b.download(m, fields=("vel",))["vel"][:nf] for m in range(3)]
    for m, (st, h) in enumerate(zip(sts, got)):
        assert len(h["step"]) == 45 and h["n_dropped"] == 0
        assert (h["step"][-1], h["t"][-1], h["dt"][-1], h["vmax"][-1]) == (st["step"], st["t"], st["dt_last"], st["vmax"])
        mass = members[m][1]["mass"][:nf]
        ke = float(np.sum(0.5 * mass * (vels[m][:, 0] ** 2 + vels[m][:, 1] ** 2)))
        ub = float(np.mean(vels[m][:, 0]))
        err = dict(tau_bottom=rel_err(h["tau_bottom"][-1], mons[m][0]), tau_top=rel_err(h["tau_top"][-1], mons[m][1]),
                   kinetic_energy=rel_err(h["kinetic_energy"][-1], ke), u_bulk=rel_err(h["u_bulk"][-1], ub))
        print(size, m, {k: f"{float(v):.2e}" for k, v in err.items()})
        for k, v in err.items():
            assert v <= 1e-12, f"{size} member {m}: {k} off by {float(v):.3e} (summation order only)"


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [False, True])
def test_idle_members_record_nothing(cfgmod, geom, capi, chunks):
    members, t1, t2 = _dt_members(cfgmod, geom)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
        b.history_enable(every=1)
        if chunks:
            b.advance(t1)
        sts = b.advance(t2)
        assert b.info()["realignments"] >= 1
        got = b.history()
    steps = [s["step"] for s in sts]
    assert len(set(steps)) > 1, steps
    for m, (s, h) in enumerate(zip(sts, got)):
        assert abs(s["t"] - t2) < 1e-12
        assert len(h["step"]) == s["step"] and h["n_dropped"] == 0, (m, len(h["step"]), s)
        assert list(h["step"]) == list(range(1, s["step"] + 1)), m
        assert h["t"][-1] == s["t"] and np.all(np.diff(h["t"]) > 0), m


# 5 ---------------------------------------------------------------------------------------------------------------
def test_full_buffers_are_per_member(cfgmod, geom, capi):
    members, _, t2 = _dt_members(cfgmod, geom)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
        b.history_enable(every=1, capacity=5)
        sts = b.advance(t2)
        steps = [s["step"] for s in sts]
        full = b.history()
        again = b.history()                    # reading without drain changes nothing
        drained = b.history(drain=True)
        empty = b.history()
        sts2 = b.advance(1e9, max_steps=3)
        resumed = b.history()
    assert len(set(steps)) == 3 and min(steps) > 5, steps
    for m in range(3):
        assert list(full[m]["step"]) == [1, 2, 3, 4, 5] and full[m]["n_dropped"] == steps[m] - 5, (m, steps)
        for k in FIELDS + ("n_dropped",):
            assert np.array_equal(full[m][k], again[m][k]) and np.array_equal(full[m][k], drained[m][k]), (m, k)
        assert len(empty[m]["step"]) == 0 and empty[m]["n_dropped"] == 0
        assert list(resumed[m]["step"]) == [steps[m] + 1, steps[m] + 2, steps[m] + 3] and resumed[m]["n_dropped"] == 0
        assert resumed[m]["t"][-1] == sts2[m]["t"]


# 6 ---------------------------------------------------------------------------------------------------------------
def test_no_feedback_on_the_physics(cfgmod, geom, capi):
    members, t1, t2 = _dt_members(cfgmod, geom)
    outs = []
    for on in (False, True):
        with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
            if on:
                b.history_enable(every=1)
            b.advance(t1)
            sts = b.advance(t2)
            assert b.info()["realignments"] >= 1
            outs.append((sts, [b.download(m) for m in range(len(members))]))
    assert outs[0][0] == outs[1][0]
    for m in range(len(members)):
        for k, v in outs[0][1][m].items():
            assert v.tobytes() == outs[1][1][m][k].tobytes(), (m, k)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_toggling_recaptures_graphs_and_keeps_the_states(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:3])
    kw = dict(t_end=1e9, lanes_per_particle=16)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.advance(1e9, max_steps=96)
        plain = [b.download(m, fields=("pos", "vel", "drho_dt")) for m in range(3)]
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.advance(1e9, max_steps=32)                       # graphs without the history kernel
        g0 = b.graph_stats()["graphs_captured"]
        b.history_enable(every=1)
        b.advance(1e9, max_steps=32)
        g1 = b.graph_stats()["graphs_captured"]
        assert g1 > g0
        assert [list(h["step"]) for h in b.history()] == [list(range(33, 65))] * 3
        b.history_disable()
        b.advance(1e9, max_steps=32)
        assert b.graph_stats()["graphs_captured"] > g1
        with pytest.raises(capi.SphxError) as e:
            b.history()
        assert e.value.identifier == "SPHX:History:disabled"
        toggled = [b.download(m, fields=("pos", "vel", "drho_dt")) for m in range(3)]
        b.history_enable(every=2)                          # re-enabling starts from empty buffers
        assert all(len(h["step"]) == 0 for h in b.history())
    for m in range(3):
        for k in plain[m]:
            assert plain[m][k].tobytes() == toggled[m][k].tobytes(), (m, k)


# 8 ---------------------------------------------------------------------------------------------------------------
def test_independent_of_the_batch_flow_statistics(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:3])
    runs = {}
    for hist, stats in ((True, False), (False, True), (True, True)):
        with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
            if stats:
                b.flow_stats_enable(every=3)
            if hist:
                b.history_enable(every=2)
            b.advance(1e9, max_steps=30)
            runs[(hist, stats)] = (b.history_records() if hist else None, b.flow_stats_sums(0) if stats else None)
    for m in range(3):
        alone, both = runs[(True, False)][0][m], runs[(True, True)][0][m]
        assert list(alone[0][:, 0]) == list(range(2, 31, 2)) and alone[1] == both[1] == 0
        assert alone[0].tobytes() == both[0].tobytes(), m
        s_alone, s_both = runs[(False, True)][1][m], runs[(True, True)][1][m]
        assert s_alone["n_samples"] == s_both["n_samples"] == 10
        for k in STATS:
            assert s_alone[k].tobytes() == s_both[k].tobytes(), (m, k)
        assert (s_alone["t_first"], s_alone["t_last"]) == (s_both["t_first"], s_both["t_last"])


# 9 ---------------------------------------------------------------------------------------------------------------
def test_repeatable(cfgmod, geom, capi):
    dp, DL = SIZES["three_workgroups"]
    members = batch_members(cfgmod, geom, dp, DL, VARIANTS[:3])
    runs = []
    for _ in range(2):
        with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
            b.history_enable(every=1)
            b.advance(1e9, max_steps=60)
            runs.append(b.history_records())
    for m in range(3):
        assert runs[0][m][0].shape == (60, 8) and runs[0][m][1] == runs[1][m][1] == 0
        assert runs[0][m][0].tobytes() == runs[1][m][0].tobytes(), m


# 10 --------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    M = 5  # 5 * (1 << 22) records exceed the cap on n_members * capacity, 1 << 24
    members = batch_members(cfgmod, geom, 0.05, 3.0, (VARIANTS + VARIANTS[:1])[:M])
    n = np.full(M, -1, dtype=np.int32)
    dropped = np.full(M, -1, dtype=np.int64)
    pn, pd = n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64))
    ok = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
    for fn, args in ((L.sphx_batch_history_enable, (C.byref(ok),)), (L.sphx_batch_history_disable, ()),
                     (L.sphx_batch_history_read, (0, None, None, None, 0))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    bad_configs = (dict(every=0), dict(every=-1), dict(capacity=0), dict(capacity=-5), dict(capacity=(1 << 22) + 1),
                   dict(capacity=1 << 22), dict(capacity=(1 << 24) // M + 1),  # (the last two: n_members * capacity > 1 << 24)
                   dict(t_from=float("nan")), dict(t_from=float("inf")), dict(t_from=-float("inf")))
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        assert err_id(capi, L.sphx_batch_history_read, h, 0, None, pn, pd, 0) == ("SPHX:History:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_batch_history_disable(h) == capi.SPHX_OK       # no-op when off
        for bad in bad_configs:
            c2 = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert err_id(capi, L.sphx_batch_history_enable, h, C.byref(c2)) == ("SPHX:History:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_batch_history_enable, h, None) == ("SPHX:History:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as e:
            b.history_enable(capacity=1 << 22)
        assert e.value.identifier == "SPHX:History:config"
        # a refused config leaves the batch without a history, and stepping
        assert err_id(capi, L.sphx_batch_history_read, h, 0, None, None, None, 0)[0] == "SPHX:History:disabled"
        assert [s["step"] for s in b.advance(1e9, max_steps=3)] == [3] * M
        assert L.sphx_batch_history_enable(h, C.byref(ok)) == capi.SPHX_OK
        b.advance(1e9, max_steps=5)
        assert L.sphx_batch_history_read(h, 0, None, pn, pd, 0) == capi.SPHX_OK   # counts only: capacity is not checked
        assert list(n) == [5] * M and list(dropped) == [0] * M
        # a refused enable leaves the running history and its records as they are
        for bad in bad_configs:
            c2 = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert err_id(capi, L.sphx_batch_history_enable, h, C.byref(c2))[0] == "SPHX:History:config", bad
        buf = np.full((M, 5, 8), -1.0)
        assert err_id(capi, L.sphx_batch_history_read, h, 4, capi.ptr(buf), None, None, 1) == \
            ("SPHX:History:capacity", capi.SPHX_ERR_ARG)
        assert np.all(buf == -1.0)
        wide = np.full((M, 7, 8), -1.0)                                # ... and nothing was drained; rows beyond n_records stay
        assert L.sphx_batch_history_read(h, 7, capi.ptr(wide), pn, None, 0) == capi.SPHX_OK
        assert list(n) == [5] * M
        for m in range(M):
            assert list(wide[m, :5, 0]) == [4.0, 5.0, 6.0, 7.0, 8.0] and np.all(wide[m, 5:] == -1.0), m
        assert len({wide[m, :5, 4].tobytes() for m in range(4)}) == 4  # each member's own tau_bottom


# 11 --------------------------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, "tests", "batch_history_worker.py")
CHILD_SECONDS = 240
_abnormal = []  # what ended abnormally, if anything did
# (switches, then fuse_ea, tail_clock of the schedule they select)
SWITCH_SETS = [("no_fuse_ea", 0, 1), ("no_fold_rebin", 1, 1), ("no_tail_clock", 0, 0), ("no_fuse_ea,no_fold_rebin,no_tail_clock", 0, 0)]


@pytest.mark.parametrize("switches,fuse_ea,tail_clock", SWITCH_SETS, ids=[s.replace(",", "+") for s, *_ in SWITCH_SETS])
def test_debug_switches_bit_identical_to_standalone(switches, fuse_ea, tail_clock):
    """SPHX_DEBUG_SWITCHES is read once per process: every set runs the worker as a fresh child under its own time limit.
    After a child that ends by a signal, an abort or its time limit no further child is started."""
    if _abnormal:
        pytest.fail(f"not started: an earlier child ended abnormally ({_abnormal[0]})")
    env = dict(os.environ, SPHX_DEBUG_SWITCHES=switches)
    try:
        r = subprocess.run([sys.executable, WORKER], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(f"[{switches}]: time limit of {CHILD_SECONDS} s")
        pytest.fail(f"{_abnormal[0]}\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-3000:]}")
    if r.returncode != 0:
        _abnormal.append(f"[{switches}]: exit code {r.returncode}")
        pytest.fail(f"{_abnormal[0]}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(lines[0])
    assert out["switches"] == switches
    assert (out["schedule"]["fuse_ea"], out["schedule"]["tail_clock"], out["schedule"]["dynamic"]) == (fuse_ea, tail_clock, 0), out["schedule"]
    assert out["steps_taken"] == [out["steps"]] * 3 and out["n_records"] == [out["steps"]] * 3 and out["n_dropped"] == [0] * 3, out
    assert out["info"]["realignments"] == 0 and min(out["rebins"]) >= 2, out
    assert not out["differs"], out["differs"]


# 12 --------------------------------------------------------------------------------------------------------------
def test_run_sweep(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.06, output_interval=0.02) for mu in (0.1, 0.15, 0.2)]
    res = driver.run_sweep(prms, history_capacity=256, history_from=0.03, settle_tol=0.5)
    assert len(res.members) == 3 and res.wall_seconds > 0 and res.grid_policy["rebuild_every"] >= 1
    for m, r in enumerate(res.members):
        h = r.history
        assert r.steps > 30 and h["n_dropped"] == 0 and r.time_avg is None
        assert list(h["step"]) == list(range(1, r.steps + 1)), m      # no gap and no repeat across the three drains
        assert h["t"][-1] == r.t and np.all(np.diff(h["t"]) > 0)
        assert rel_err(h["tau_bottom"][-1], r.tau_bottom) <= 1e-12 and rel_err(h["tau_top"][-1], r.tau_top) <= 1e-12
        fig = driver.history_figures(prms[m], h, t_from=0.03, tol=0.5)
        assert 0 < fig["n_records"] < r.steps
        for k, v in fig.items():
            assert np.array_equal(res.table[k][m], v, equal_nan=True), (m, k)
        assert res.table["steps"][m] == r.steps and res.table["n_dropped"][m] == 0
        for k in ("mu", "c_f", "p0", "gravity_g", "transport_coeff"):
            assert res.table[k][m] == getattr(prms[m], k)
    assert all(len(v) == 3 for v in res.table.values())
    # with average_from: the batch's flow statistics as well, the members' time averages are run_ensemble's
    avg = driver.run_sweep(prms, history_every=2, history_capacity=256, average_from=0.03, average_every=2)
    ens = driver.run_ensemble(prms, average_from=0.03, average_every=2)
    for m, (a, e) in enumerate(zip(avg.members, ens.members)):
        assert (a.steps, a.t) == (e.steps, e.t) == (res.members[m].steps, res.members[m].t)
        assert a.pos.tobytes() == e.pos.tobytes() and a.vel.tobytes() == e.vel.tobytes()
        assert list(a.history["step"]) == list(range(2, a.steps + 1, 2))
        ta, te = a.time_avg, e.time_avg
        assert ta["n_samples"] == te["n_samples"] > 0 and (ta["t_first"], ta["t_last"]) == (te["t_first"], te["t_last"])
        for k in ("u_mean", "mid_u_mean", "u_exact"):
            assert np.array_equal(ta[k], te[k], equal_nan=True), (m, k)
        for k in ("L2", "uy_rms_over_umax", "ux_std_centre_over_umax"):
            assert ta[k] == te[k] or (np.isnan(ta[k]) and np.isnan(te[k])), (m, k)
        for k in STATS:
            assert ta["profile"][k].tobytes() == te["profile"][k].tobytes(), (m, k)
    # one output interval takes more than 8 steps: the capacity is too small, and the error names the member
    with pytest.raises(RuntimeError, match=r"member 0.*history_capacity >= \d+"):
        driver.run_sweep(prms, history_capacity=8)
