"""The ten slot samplers -- flow statistics, step history, field map, point probes, profile series, pair statistics, gradient
statistics, particle tracers, density statistics, mode amplitudes (include/sphx.h sections 2a, 2d, 2e, 2h, 2j, 2l, 2n, 2p, 2r,
2t) -- beside each other on one context: what they share on the device (the gate, the fenced ticket, the head update:
csrc/sphx_slot_sample.hpp) and on the host (one lifecycle, one view of the state a slot leaves, one record-ring read:
csrc/sphx_samplers.hpp) must keep them independent of each other.  Everything here is bit-equality between runs of the same
device code on the same state: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from helpers import batch_members, make_case

pytestmark = pytest.mark.gpu

# main: 4 800 fluid particles -- k_flow_stats runs two workgroups and k_step_history three, both through the fenced ticket; the
# default map has 240 x 80 nodes.  dynamic: the device decides when to re-bin, the samplers find out from the clock.
CASES = {
    "dp025_lpp16": (0.025, 3.0, dict(lanes_per_particle=16)),
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1)),
}
STATE = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
CLOCK = ("t", "dt_last", "vmax")
ALL = ("stats", "history", "field", "probes", "series", "pairs", "grads", "tracers", "dens", "modes")
RECORD = ("history", "probes", "series", "tracers", "modes")  # the samplers that keep a ring of records
CAPACITY = 64


@pytest.fixture(scope="module", params=list(CASES))
def case(request, cfgmod, geom):
    dp, DL, kw = CASES[request.param]
    prm, parts = make_case(cfgmod, geom, dp=dp, DL=DL, jitter=0.2, seed=11, developed=True)
    return request.param, prm, parts, kw


def _points(prm):
    """8 probes: across the channel, on both walls' side, one on the periodic seam and one left of it"""
    DL, DH = prm.DL, prm.DH
    return np.array([[0.0, 0.5 * DH], [0.13 * DL, 0.1 * DH], [0.31 * DL, 0.9 * DH], [0.5 * DL, 0.5 * DH], [0.77 * DL, 0.0],
                     [0.9 * DL, DH], [-0.2 * DL, 0.3 * DH], [1.4 * DL, 0.7 * DH]])


def _ids(n_fluid):
    """8 fluid rows, first and last included, not in order"""
    return np.array([n_fluid - 1, 0, n_fluid // 2, 7, n_fluid // 3, 1, n_fluid - 2, n_fluid // 5], dtype=np.int32)


def _enable(x, prm, which):
    """the samplers named in `which` on the context or batch x of channels with parameters prm"""
    bands = ((0.5 * prm.DL, 0.1 * prm.DL),)
    if "stats" in which:
        x.flow_stats_enable(bands=bands)
    if "history" in which:
        x.history_enable(capacity=CAPACITY)
    if "field" in which:
        x.field_map_enable()
    if "probes" in which:
        x.probes_enable(_points(prm), capacity=CAPACITY)
    if "series" in which:
        x.profile_series_enable(capacity=CAPACITY, bands=bands)
    if "pairs" in which:
        x.pair_dist_enable(n_bins=32, with_walls=True, bands=bands)
    if "grads" in which:
        x.grad_stats_enable(bands=bands)
    if "tracers" in which:
        x.tracers_enable(_ids(x.n_fluid), capacity=CAPACITY)
    if "dens" in which:
        x.dens_stats_enable(bands=bands)
    if "modes" in which:
        x.modes_enable(mx=2, ny=2, capacity=CAPACITY)


def _flat(prefix, d):
    return {f"{prefix}/{k}": np.asarray(v) for k, v in d.items()}


def _outputs(ctx, which):
    """Everything the samplers named in `which` hold, as {name: array}."""
    out = {}
    if "stats" in which:
        for band in (0, 1):
            out.update(_flat(f"stats{band}", ctx.flow_stats_sums(band)))
    if "history" in which:
        rec, dropped = ctx.history_records()
        out.update({"history/records": rec, "history/n_dropped": np.asarray(dropped)})
    if "field" in which:
        out.update(_flat("field", ctx.field_map_sums()))
    if "probes" in which:
        out.update(_flat("probes", ctx.probes()))
    if "series" in which:
        out.update(_flat("series", ctx.profile_series_sums()))
    if "pairs" in which:
        for band, d in enumerate(ctx.pair_dist_sums()):
            out.update(_flat(f"pairs{band}", d))
    if "grads" in which:
        for band in (0, 1):
            out.update(_flat(f"grads{band}", ctx.grad_stats_sums(band)))
    if "tracers" in which:
        out.update(_flat("tracers", ctx.tracers()))
    if "dens" in which:
        for band in (0, 1):
            out.update(_flat(f"dens{band}", ctx.dens_stats_sums(band)))
    if "modes" in which:
        out.update(_flat("modes", ctx.modes()))
    return out


def _samples(outputs):
    """how many samples each sampler of `outputs` has taken, by its own count"""
    n = {}
    for key, name in (("stats0/n_samples", "stats"), ("field/n_samples", "field"), ("pairs0/n_samples", "pairs"),
                      ("grads0/n_samples", "grads"), ("dens0/n_samples", "dens")):
        if key in outputs:
            n[name] = int(outputs[key])
    for key, name in (("history/records", "history"), ("probes/step", "probes"), ("series/step", "series"),
                      ("tracers/step", "tracers"), ("modes/step", "modes")):
        if key in outputs:
            n[name] = len(outputs[key])
    return n


def _steps(outputs):
    """the step numbers of the records each record sampler of `outputs` holds"""
    s = {name: list(outputs[f"{name}/step"]) for name in ("probes", "series", "tracers", "modes") if f"{name}/step" in outputs}
    if "history/records" in outputs:
        s["history"] = list(outputs["history/records"][:, 0])
    return s


def _assert_same_bits(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: {k} differs"


def _only(outputs, name):
    return {k: v for k, v in outputs.items() if k.split("/")[0].rstrip("0123456789") == name}


# (a) ---------------------------------------------------------------------------------------------------------------
def test_each_sampler_alone_and_all_ten_together_give_the_same_bits(capi, case):
    name, prm = case[0], case[1]
    runs, tails = {}, {}
    for which in [(s,) for s in ALL] + [ALL]:
        with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
            _enable(ctx, prm, which)
            st = ctx.advance(1e9, max_steps=40)
            assert st["step"] == 40
            state = dict(ctx.download(STATE), **{k: np.asarray(st[k]) for k in CLOCK})
            runs[which] = (_outputs(ctx, which), state, ctx.graph_stats(), ctx.schedule())
            # An advance of 40 slots is replayed whole (a graph of 32 or 40 slots and one of the 8 left: only fewer than 4 are
            # launched eagerly), so 3 more slots follow for the eager launches.
            assert ctx.advance(1e9, max_steps=3)["step"] == 43
            tails[which] = (_outputs(ctx, which), ctx.graph_stats())
    together, state0, graphs, sched = runs[ALL]
    print(f"{name}: after 40 slots {graphs} {sched}; after 43 {tails[ALL][1]}")
    # replayed graphs, eager slots, and (static schedule, K = 16) two scheduled re-binnings
    assert graphs["slots_replayed"] > 0 and tails[ALL][1]["slots_eager"] > 0
    if name == "dp05_dynamic":
        assert sched["dynamic"]
    else:
        assert sched["rebins"] >= 2
    assert _samples(together) == {s: 40 for s in ALL}
    assert _steps(together) == {s: list(range(1, 41)) for s in RECORD} and together["history/n_dropped"] == 0
    assert _samples(tails[ALL][0]) == {s: 43 for s in ALL}
    for s in ALL:
        alone, state, _, _ = runs[(s,)]
        _assert_same_bits(alone, _only(together, s), f"{name}: {s} alone against all ten on")
        _assert_same_bits(state, state0, f"{name}: the state with {s} alone against all ten on")
        _assert_same_bits(tails[(s,)][0], _only(tails[ALL][0], s), f"{name}: {s} alone, 3 eager slots on")


# (b) ---------------------------------------------------------------------------------------------------------------
def test_enabling_and_disabling_one_sampler_leaves_the_others_alone(capi, case):
    name, prm = case[0], case[1]
    rest = tuple(s for s in ALL if s not in ("history", "field"))
    with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, prm, rest + ("history",))
        ctx.advance(1e9, max_steps=10)
        _enable(ctx, prm, ("field",))
        ctx.advance(1e9, max_steps=10)
        history = _outputs(ctx, ("history",))  # (disabling releases the records)
        ctx.history_disable()
        assert ctx.advance(1e9, max_steps=10)["step"] == 30
        others, field = _outputs(ctx, rest), _outputs(ctx, ("field",))
        with pytest.raises(capi.SphxError) as e:
            ctx.history_records()
        assert e.value.identifier == "SPHX:History:disabled"
    # the same 30 steps, in the same three calls, with one sampler each
    for s in rest:
        with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
            _enable(ctx, prm, (s,))
            for _ in range(3):
                ctx.advance(1e9, max_steps=10)
            _assert_same_bits(_only(others, s), _outputs(ctx, (s,)), f"{name}: {s} of 30 steps")
    assert _samples(others) == {s: 30 for s in rest}
    with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, prm, ("history",))
        for _ in range(2):
            ctx.advance(1e9, max_steps=10)
        _assert_same_bits(history, _outputs(ctx, ("history",)), f"{name}: history of steps 1..20")
    assert list(history["history/records"][:, 0]) == list(range(1, 21)) and history["history/n_dropped"] == 0
    with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
        t10 = ctx.advance(1e9, max_steps=10)["t"]
        _enable(ctx, prm, ("field",))
        for _ in range(2):
            ctx.advance(1e9, max_steps=10)
        _assert_same_bits(field, _outputs(ctx, ("field",)), f"{name}: map of steps 11..30")
    assert field["field/n_samples"] == 20 and field["field/t_first"] > t10


# (c) ---------------------------------------------------------------------------------------------------------------
def test_a_refused_enable_leaves_a_running_sampler_as_it_was(capi, case):
    name, prm = case[0], case[1]
    L = capi.lib()
    pts, ids = _points(prm), _ids(case[2]["n_fluid"])
    p_pts, p_ids = pts.ctypes.data_as(C.POINTER(C.c_double)), ids.ctypes.data_as(C.POINTER(C.c_int32))
    # each through the raw C call: capi's own validators would refuse these first
    refused = (
        ("SPHX:Stats:config", L.sphx_ctx_flow_stats_enable, capi.SphxFlowStatsConfig(n_bins=0, every=0, t_from=0.0, n_bands=0)),
        ("SPHX:History:config", L.sphx_ctx_history_enable, capi.SphxHistoryConfig(every=1, capacity=0, t_from=0.0)),
        ("SPHX:Field:config", L.sphx_ctx_field_map_enable, capi.SphxFieldMapConfig(nx=1, ny=0, every=1, with_walls=0, t_from=0.0)),
        ("SPHX:Probe:config", L.sphx_ctx_probes_enable,
         capi.SphxProbesConfig(n_points=0, every=1, capacity=CAPACITY, with_walls=0, t_from=0.0, points=p_pts)),
        ("SPHX:ProfileSeries:config", L.sphx_ctx_profile_series_enable,
         capi.SphxProfileSeriesConfig(n_bins=0, every=1, capacity=0, t_from=0.0, n_bands=0)),
        ("SPHX:PairDist:config", L.sphx_ctx_pair_dist_enable,
         capi.SphxPairDistConfig(n_bins=0, every=1, t_from=0.0, r_max=0.0, y_margin=0.0, with_walls=0, n_bands=0)),
        ("SPHX:GradStats:config", L.sphx_ctx_grad_stats_enable,
         capi.SphxGradStatsConfig(n_bins=0, every=1, t_from=0.0, det_min=0.05, with_walls=0, n_bands=3)),
        ("SPHX:Tracers:config", L.sphx_ctx_tracers_enable,
         capi.SphxTracersConfig(n_tracers=0, every=1, capacity=CAPACITY, t_from=0.0, ids=p_ids)),
        ("SPHX:DensStats:config", L.sphx_ctx_dens_stats_enable,
         capi.SphxDensStatsConfig(n_bins=0, every=1, t_from=0.0, n_hist=0, n_bands=0, hist_range=0.05, delta_bound=0.5)),
        ("SPHX:Modes:config", L.sphx_ctx_modes_enable, capi.SphxModesConfig(mx=17, ny=2, every=1, capacity=CAPACITY, t_from=0.0)),
    )
    with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, prm, ALL)
        ctx.advance(1e9, max_steps=10)
        before = _outputs(ctx, ALL)
        for ident, enable, cfg in refused:
            assert enable(ctx._h, C.byref(cfg)) == capi.SPHX_ERR_ARG
            assert L.sphx_last_error_id().decode() == ident
            _assert_same_bits(_outputs(ctx, ALL), before, f"{name}: after the refused {ident}")
        assert ctx.advance(1e9, max_steps=5)["step"] == 15
        after = _outputs(ctx, ALL)
    assert _samples(before) == {s: 10 for s in ALL}
    assert _samples(after) == {s: 15 for s in ALL}
    assert _steps(after) == {s: list(range(1, 16)) for s in RECORD}
    # ... and they are the samples of an undisturbed run of the same calls
    with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, prm, ALL)
        ctx.advance(1e9, max_steps=10)
        ctx.advance(1e9, max_steps=5)
        _assert_same_bits(after, _outputs(ctx, ALL), f"{name}: 15 steps, against a run without refused enables")


# (d) ---------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25  # (no record holds it: steps and counts are >= 0, and the arrays are compared whole)


def _refused_read(capi, x, s, m, cap):
    """The raw read of record sampler s of the context or batch x (m channels) into sentinel-filled arrays of `cap` records per
    channel, draining: -> (return code, identifier, whether every array and count still holds its sentinel)."""
    L = capi.lib()
    width = {"history": len(capi.HISTORY_FIELDS), "probes": 8 * len(capi.PROBE_FIELDS), "tracers": 8 * len(capi.TRACER_FIELDS),
             "modes": 3 * 3 * len(capi.MODE_FIELDS) * len(capi.MODE_BASES)}
    if s == "series":
        n_bins, n_bands = x._profile_series
        width["series"] = n_bins * n_bands * 5
    times, values = np.full((m, cap, 2), SENTINEL), np.full((m, cap, width[s]), SENTINEL)
    n, dropped, missing = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int64), np.full(m, -1, dtype=np.int64)
    a, b = C.c_int(-1), C.c_int(-1)
    ids = np.full(8, -1, dtype=np.int32)
    pd = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_double))
    pn, pdrop = n.ctypes.data_as(C.POINTER(C.c_int)), dropped.ctypes.data_as(C.POINTER(C.c_int64))
    stem = x._stem
    if s == "history":
        rc = getattr(L, stem + "history_read")(x._h, C.c_int(cap), pd(values), pn, pdrop, C.c_int(1))
    elif s == "probes":
        rc = getattr(L, stem + "probes_read")(x._h, C.c_int(cap), pd(times), pd(values), C.byref(a), pn, pdrop, C.c_int(1))
    elif s == "tracers":
        rc = getattr(L, stem + "tracers_read")(x._h, C.c_int(cap), pd(times), pd(values), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                               C.byref(a), pn, pdrop, missing.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(1))
    elif s == "series":
        rc = getattr(L, stem + "profile_series_read")(x._h, C.c_int(cap), pd(times), pd(values), C.byref(a), C.byref(b), pn, pdrop,
                                                      C.c_int(1))
    else:
        rc = getattr(L, stem + "modes_read")(x._h, C.c_int(cap), pd(times), pd(values), C.byref(a), C.byref(b), pn, pdrop, C.c_int(1))
    untouched = (np.all(times == SENTINEL) and np.all(values == SENTINEL) and np.all(n == -1) and np.all(dropped == -1)
                 and np.all(missing == -1) and np.all(ids == -1) and a.value == -1 and b.value == -1)
    return rc, L.sphx_last_error_id().decode(), bool(untouched)


READERS = {"history": lambda x, drain: x.history(drain), "probes": lambda x, drain: x.probes(drain),
           "series": lambda x, drain: x.profile_series_sums(drain), "tracers": lambda x, drain: x.tracers(drain),
           "modes": lambda x, drain: x.modes(drain)}
STEMS = {"history": "History", "probes": "Probe", "series": "ProfileSeries", "tracers": "Tracers", "modes": "Modes"}


def _check_refused_reads(capi, x, m, what):
    """every record sampler of x: a read one record short is refused whole, the next one returns every record, once"""
    for s in RECORD:
        want = READERS[s](x, False)
        per = want if m > 1 else [want]
        counts = [len(d["step"]) for d in per]
        rc, ident, untouched = _refused_read(capi, x, s, m, max(counts) - 1)
        assert rc == capi.SPHX_ERR_ARG and ident == f"SPHX:{STEMS[s]}:capacity", f"{what}: {s}: {rc} {ident}"
        assert untouched, f"{what}: {s}: the refused read wrote into the caller's arrays"
        got = READERS[s](x, True)  # (nothing was drained: every record is still there; this read drains)
        for k, (g, w) in enumerate(zip(got if m > 1 else [got], per)):
            _assert_same_bits(_flat(s, g), _flat(s, w), f"{what}: {s} member {k} after the refused read")
        after = READERS[s](x, False)
        assert [len(d["step"]) for d in (after if m > 1 else [after])] == [0] * m, f"{what}: {s}: the draining read left records"
    return counts


def test_a_read_one_record_short_copies_and_drains_nothing_on_a_context(capi, case):
    name, prm = case[0], case[1]
    with capi.Context.from_parts(prm, case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, prm, RECORD)
        assert ctx.advance(1e9, max_steps=10)["step"] == 10
        assert _check_refused_reads(capi, ctx, 1, name) == [10]


def test_a_read_one_record_short_copies_and_drains_nothing_on_a_batch_with_unequal_counts(cfgmod, geom, capi):
    # members whose dt differ (c_f 15 / 21): they need different step counts to one target time, so their rings fill unequally
    variants = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=21.0, transport_coeff=0.20, seed=8)]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    prm = members[0][0]
    t_target = 10.3 * 0.25 * prm.h / (15.0 + 1.5)
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        _enable(b, prm, RECORD)
        sts = b.advance(t_target)
        steps = [int(st["step"]) for st in sts]
        assert steps[0] != steps[1] and min(steps) >= 2 and max(steps) <= CAPACITY, steps
        counts = [len(d["step"]) for d in b.history()]
        assert counts == steps
        _check_refused_reads(capi, b, 2, "batch")
