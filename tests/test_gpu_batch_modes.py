"""-m gpu: the mode amplitudes of a batch (include/sphx.h section 2u) -- k_modes_b records every member's amplitudes in one launch
per step slot.  Members that differ in mu fall out of step, keep their own step / t series and record counts and are byte for
byte standalone contexts; a member that sits out a slot touches nothing; a member that overflows counts its own dropped records;
with several chunks per member the ticket and the int64 sums are per member; driver.run_sweep hands every member its records
and the table the decay times of the first two start-up modes."""
import ctypes as C

import numpy as np
import pytest

import mode_cases as mc
from helpers import err_id, make_case

pytestmark = pytest.mark.gpu

MU = (0.05, 0.1, 0.2, 0.1)


def _members(cfgmod, geom):
    """Four members of dp05 with mu in MU; the last shares its mu with member 1 and has a perturbed initial state (its own
    jitter and noise).  Every member's dt is acoustic, so the clocks differ by the members' max |v| alone: out of step in t
    within a step, and by a step at a target time chosen between the members' times after 25 steps."""
    return [make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=21 if m < 3 else 99, developed=True, mu=mu)
            for m, mu in enumerate(MU)]


def _target(capi, members, n=25):
    """a time between the members' times after n steps: some reach it in n steps, the others need one more"""
    t_n = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            t_n.append(ctx.advance(1e9, max_steps=n)["t"])
    ts = sorted(t_n)
    assert len(set(ts)) == len(ts), ts
    return 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])


def test_members_out_of_step_equal_standalone_contexts(cfgmod, geom, capi):
    members = _members(cfgmod, geom)
    target = _target(capi, members)
    cfg = dict(mx=4, ny=8, every=1, capacity=64)
    refs, steps = [], []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.modes_enable(**cfg)
            steps.append(ctx.advance(target)["step"])
            refs.append(ctx.modes())
    assert len(set(steps)) > 1 and all(24 <= s <= 27 for s in steps), steps
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.modes_enable(**cfg)
        sts = b.advance(target)
        got = b.modes()
    assert [s["step"] for s in sts] == steps
    for m in range(4):
        # a member that had reached the target sat out the batch's last slots: no record of them, nothing dropped
        assert len(got[m]["step"]) == steps[m] and got[m]["ux"].shape == (steps[m], 5, 9, 4) and got[m]["n_dropped"] == 0
        mc.assert_series_identical(got[m], refs[m], f"member {m}")
    assert len({len(g["step"]) for g in got}) > 1                       # record counts differ between members
    assert len({g["t"][:20].tobytes() for g in got}) == 4               # each on its own clock
    assert len({g["ux"][:20].tobytes() for g in got}) == 4
    # a member that overflows: capacity = the smallest member's count
    cap = min(steps)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.modes_enable(**dict(cfg, capacity=cap))
        b.advance(target)
        full = b.modes()
    assert [f["n_dropped"] for f in full] == [s - cap for s in steps] and any(f["n_dropped"] == 0 for f in full)
    for m in range(4):
        mc.assert_series_identical(full[m], {k: refs[m][k][:cap] for k in mc.SERIES}, f"member {m}, capacity {cap}", counters=False)


def test_a_member_gated_out_touches_nothing(cfgmod, geom, capi):
    """t_from between the members' clocks: after ten steps the members whose t has passed it have records, the others none --
    no record, no dropped record, and the rows of the caller's arrays that belong to them stay as they were."""
    members = _members(cfgmod, geom)
    L = capi.lib()
    M = 4
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        sts = b.advance(1e9, max_steps=10)
    ts = sorted(s["t"] for s in sts)
    t_from = 0.5 * (ts[1] + ts[2])
    late = [m for m in range(M) if sts[m]["t"] >= t_from]
    assert len(late) == 2
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.modes_enable(mx=1, ny=2, every=10, capacity=4, t_from=t_from)
        b.advance(1e9, max_steps=10)
        got = b.modes()
        n, dropped = np.full(M, -1, dtype=np.int32), np.full(M, -1, dtype=np.int64)
        times, records = np.full((M, 2, 2), -1.0), np.full((M, 2, 2, 3, 3, 4), -1.0)
        assert L.sphx_batch_modes_read(b._h, 2, capi.ptr(times), capi.ptr(records), None, None, n.ctypes.data_as(C.POINTER(C.c_int)),
                                       dropped.ctypes.data_as(C.POINTER(C.c_int64)), 0) == capi.SPHX_OK
    for m in range(M):
        assert got[m]["step"].tolist() == ([10] if m in late else []) and got[m]["n_dropped"] == 0, m
        assert n[m] == (1 if m in late else 0) and dropped[m] == 0
        assert np.all(times[m, n[m]:] == -1.0) and np.all(records[m, n[m]:] == -1.0), m
        if m in late:
            assert times[m, 0].tolist() == [10.0, sts[m]["t"]] and records[m, 0, 0, 0, 0, 0] == members[m][1]["n_fluid"]


def test_several_chunks_per_member(cfgmod, geom, capi):
    """30 k fluid particles a member: 15 chunks x 15 groups per grid row of k_modes_b, a ticket and int64 sums per member"""
    members = [make_case(cfgmod, geom, dp=0.01, DL=3.0, jitter=0.2, seed=31 + m, developed=True, mu=mu) for m, mu in enumerate((0.1, 0.15))]
    assert members[0][1]["n_fluid"] > 2 * mc.CHUNK
    cfg = dict(every=2, capacity=16)
    kw = dict(lanes_per_particle=16)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.modes_enable(**cfg)
            ctx.advance(1e9, max_steps=12)
            refs.append(ctx.modes())
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, **kw) as b:
        b.modes_enable(**cfg)
        b.advance(1e9, max_steps=12)
        b.modes_sample()
        got = b.modes()
    for m in range(2):
        assert got[m]["step"].tolist() == [2, 4, 6, 8, 10, 12, 12] and got[m]["n_dropped"] == 0
        mc.assert_series_identical({k: got[m][k][:6] for k in mc.SERIES}, refs[m], f"member {m}", counters=False)
        for f in mc.FIELDS:
            assert got[m][f][6].tobytes() == got[m][f][5].tobytes(), f      # the sample of the state now: the last step's again
        mc.assert_exact_identities(mc.record(got[m], 6), members[m][1]["n_fluid"], f"member {m}")
    assert not np.array_equal(got[0]["ux"], got[1]["ux"])


def test_batch_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = _members(cfgmod, geom)[:3]
    M = 3
    ok = capi.SphxModesConfig(mx=4, ny=8, every=1, capacity=16, t_from=0.0)
    nothing = (None, None, None, None, None, None, 0)
    for fn, args in ((L.sphx_batch_modes_enable, (C.byref(ok),)), (L.sphx_batch_modes_disable, ()), (L.sphx_batch_modes_sample, ()),
                     (L.sphx_batch_modes_read, (0, *nothing))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        assert err_id(capi, L.sphx_batch_modes_read, h, 0, *nothing) == ("SPHX:Modes:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_batch_modes_sample, h) == ("SPHX:Modes:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_batch_modes_disable(h) == capi.SPHX_OK       # no-op when off
        for call in (b.modes, b.modes_sample):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:Modes:disabled"
        b.modes_enable(every=1, capacity=16)
        b.advance(1e9, max_steps=5)
        # (45 modes x 12 = 540 doubles a record: the cap of 1 << 27 doubles is taken over the members)
        for bad in (dict(every=0), dict(capacity=0), dict(mx=17), dict(ny=-1), dict(capacity=(1 << 27) // (540 * M) + 1)):
            c2 = capi.SphxModesConfig(**dict(dict(mx=4, ny=8, every=1, capacity=16, t_from=0.0), **bad))
            assert err_id(capi, L.sphx_batch_modes_enable, h, C.byref(c2)) == ("SPHX:Modes:config", capi.SPHX_ERR_ARG), bad
        with pytest.raises(capi.SphxError) as e:
            b.modes_enable(capacity=(1 << 27) // (540 * M) + 1)
        assert e.value.identifier == "SPHX:Modes:config"
        got = b.modes()
        assert [g["step"].tolist() for g in got] == [[1, 2, 3, 4, 5]] * M  # the refused enables left the sampler running
        times = np.full((M, 4, 2), -1.0)
        assert err_id(capi, L.sphx_batch_modes_read, h, 4, capi.ptr(times), None, None, None, None, None, 1) == \
            ("SPHX:Modes:capacity", capi.SPHX_ERR_ARG)
        assert np.all(times == -1.0)


def test_run_sweep_fills_the_decay_times(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=1.0, mu=mu, end_time=0.1, output_interval=0.05) for mu in (0.1, 0.15, 0.2)]
    res = driver.run_sweep(prms, history_capacity=1024, modes_every=2)
    assert res.table["tau1_fit"].shape == res.table["tau3_fit"].shape == (3,)
    for m, r in enumerate(res.members):
        s = r.modes
        assert s["n_dropped"] == 0 and s["step"].tolist() == list(range(2, r.steps + 1, 2)), m   # no gap across the drains
        assert np.array_equal(s["t"], r.history["t"][1::2]) and s["ux"].shape == (r.steps // 2, 5, 9, 4)
        fig = driver.mode_figures(prms[m], s)
        assert res.table["tau1_fit"][m] == fig["tau_fit"][1] and res.table["tau3_fit"][m] == fig["tau_fit"][3]
        print(f"member {m}: tau1_fit / tau_exact = {fig['tau_fit'][1] / fig['tau_exact'][1]:.4f}, tau3_fit / tau_exact = "
              f"{fig['tau_fit'][3] / fig['tau_exact'][3]:.4f}")
        assert np.isfinite(fig["tau_fit"][1]) and fig["tau_fit"][1] > 0.0 and np.isfinite(fig["tau_fit"][3]) and fig["tau_fit"][3] > 0.0
        if res.grid_policy["realignments"] == 0:
            alone = driver.run(prms[m], modes_every=2).modes
            mc.assert_series_identical(s, alone, f"member {m} against a standalone run")
    # a larger viscosity decays faster: the table responds to what the sweep varies
    assert res.table["tau1_fit"][0] > res.table["tau1_fit"][1] > res.table["tau1_fit"][2]
    assert all(r.modes is None for r in driver.run_sweep(prms, history_capacity=1024).members)
    with pytest.raises(RuntimeError, match=r"member 0.*modes_capacity >= \d+ \(it is 4\)"):
        driver.run_sweep(prms, history_capacity=1024, modes_every=2, modes_capacity=4)
