"""The three slot samplers -- flow statistics, step history, field map (include/sphx.h sections 2a, 2d, 2e) -- beside each
other on one context: what they share on the device (the gate, the fenced ticket, the head update: csrc/sphx_slot_sample.hpp)
and on the host (one lifecycle, one view of the state a slot leaves: csrc/sphx_samplers.hpp) must keep them independent of
each other.  Everything here is bit-equality between runs of the same device code on the same state: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_case

pytestmark = pytest.mark.gpu

# main: 4 800 fluid particles -- k_flow_stats runs two workgroups and k_step_history three, both through the fenced ticket; the
# default map has 240 x 80 nodes.  dynamic: the device decides when to re-bin, the samplers find out from the clock.
CASES = {
    "dp025_lpp16": (0.025, 3.0, dict(lanes_per_particle=16)),
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1)),
}
STATE = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
CLOCK = ("t", "dt_last", "vmax")


@pytest.fixture(scope="module", params=list(CASES))
def case(request, cfgmod, geom):
    dp, DL, kw = CASES[request.param]
    prm, parts = make_case(cfgmod, geom, dp=dp, DL=DL, jitter=0.2, seed=11, developed=True)
    return request.param, prm, parts, kw


def _enable(ctx, case, which):
    DL = case[1].DL
    if "stats" in which:
        ctx.flow_stats_enable(bands=((0.5 * DL, 0.1 * DL),))
    if "history" in which:
        ctx.history_enable(capacity=64)
    if "field" in which:
        ctx.field_map_enable()


def _outputs(ctx, which):
    """Everything the samplers named in `which` hold, as {name: array}."""
    out = {}
    if "stats" in which:
        for band in (0, 1):
            out.update({f"stats{band}/{k}": np.asarray(v) for k, v in ctx.flow_stats_sums(band).items()})
    if "history" in which:
        rec, dropped = ctx.history_records()
        out.update({"history/records": rec, "history/n_dropped": np.asarray(dropped)})
    if "field" in which:
        out.update({f"field/{k}": np.asarray(v) for k, v in ctx.field_map_sums().items()})
    return out


def _assert_same_bits(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: {k} differs"


def _only(outputs, prefix):
    return {k: v for k, v in outputs.items() if k.startswith(prefix)}


# (a) ---------------------------------------------------------------------------------------------------------------
def test_each_sampler_alone_and_all_three_together_give_the_same_bits(capi, case):
    name = case[0]
    all3 = ("stats", "history", "field")
    runs, tails = {}, {}
    for which in (("stats",), ("history",), ("field",), all3):
        with capi.Context.from_parts(case[1], case[2], t_end=1e9, **case[3]) as ctx:
            _enable(ctx, case, which)
            st = ctx.advance(1e9, max_steps=40)
            assert st["step"] == 40
            state = dict(ctx.download(STATE), **{k: np.asarray(st[k]) for k in CLOCK})
            runs[which] = (_outputs(ctx, which), state, ctx.graph_stats(), ctx.schedule())
            # An advance of 40 slots is replayed whole (a graph of 32 or 40 slots and one of the 8 left: only fewer than 4 are
            # launched eagerly), so 3 more slots follow for the eager launches.
            assert ctx.advance(1e9, max_steps=3)["step"] == 43
            tails[which] = (_outputs(ctx, which), ctx.graph_stats())
    together, state0, graphs, sched = runs[all3]
    print(f"{name}: after 40 slots {graphs} {sched}; after 43 {tails[all3][1]}")
    # replayed graphs, eager slots, and (static schedule, K = 16) two scheduled re-binnings
    assert graphs["slots_replayed"] > 0 and tails[all3][1]["slots_eager"] > 0
    if name == "dp05_dynamic":
        assert sched["dynamic"]
    else:
        assert sched["rebins"] >= 2
    assert together["stats0/n_samples"] == 40 and together["field/n_samples"] == 40
    assert list(together["history/records"][:, 0]) == list(range(1, 41)) and together["history/n_dropped"] == 0
    assert tails[all3][0]["stats0/n_samples"] == 43 and len(tails[all3][0]["history/records"]) == 43
    for which in (("stats",), ("history",), ("field",)):
        alone, state, _, _ = runs[which]
        _assert_same_bits(alone, _only(together, which[0]), f"{name}: {which[0]} alone against all three on")
        _assert_same_bits(state, state0, f"{name}: the state with {which[0]} alone against all three on")
        _assert_same_bits(tails[which][0], _only(tails[all3][0], which[0]), f"{name}: {which[0]} alone, 3 eager slots on")


# (b) ---------------------------------------------------------------------------------------------------------------
def test_enabling_and_disabling_one_sampler_leaves_the_others_alone(capi, case):
    name = case[0]
    with capi.Context.from_parts(case[1], case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, case, ("stats", "history"))
        ctx.advance(1e9, max_steps=10)
        _enable(ctx, case, ("field",))
        ctx.advance(1e9, max_steps=10)
        history = _outputs(ctx, ("history",))  # (disabling releases the records)
        ctx.history_disable()
        assert ctx.advance(1e9, max_steps=10)["step"] == 30
        stats, field = _outputs(ctx, ("stats",)), _outputs(ctx, ("field",))
        with pytest.raises(capi.SphxError) as e:
            ctx.history_records()
        assert e.value.identifier == "SPHX:History:disabled"
    # the same 30 steps, in the same three calls, with one sampler each
    with capi.Context.from_parts(case[1], case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, case, ("stats",))
        for _ in range(3):
            ctx.advance(1e9, max_steps=10)
        _assert_same_bits(stats, _outputs(ctx, ("stats",)), f"{name}: statistics of 30 steps")
    assert stats["stats0/n_samples"] == 30
    with capi.Context.from_parts(case[1], case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, case, ("history",))
        for _ in range(2):
            ctx.advance(1e9, max_steps=10)
        _assert_same_bits(history, _outputs(ctx, ("history",)), f"{name}: history of steps 1..20")
    assert list(history["history/records"][:, 0]) == list(range(1, 21)) and history["history/n_dropped"] == 0
    with capi.Context.from_parts(case[1], case[2], t_end=1e9, **case[3]) as ctx:
        t10 = ctx.advance(1e9, max_steps=10)["t"]
        _enable(ctx, case, ("field",))
        for _ in range(2):
            ctx.advance(1e9, max_steps=10)
        _assert_same_bits(field, _outputs(ctx, ("field",)), f"{name}: map of steps 11..30")
    assert field["field/n_samples"] == 20 and field["field/t_first"] > t10


# (c) ---------------------------------------------------------------------------------------------------------------
def test_a_refused_enable_leaves_a_running_sampler_as_it_was(capi, case):
    name = case[0]
    L = capi.lib()
    all3 = ("stats", "history", "field")
    # each through the raw C call: capi's own validators would refuse these first
    refused = (
        ("SPHX:Stats:config", L.sphx_ctx_flow_stats_enable, capi.SphxFlowStatsConfig(n_bins=0, every=0, t_from=0.0, n_bands=0)),
        ("SPHX:History:config", L.sphx_ctx_history_enable, capi.SphxHistoryConfig(every=1, capacity=0, t_from=0.0)),
        ("SPHX:Field:config", L.sphx_ctx_field_map_enable, capi.SphxFieldMapConfig(nx=1, ny=0, every=1, with_walls=0, t_from=0.0)),
    )
    with capi.Context.from_parts(case[1], case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, case, all3)
        ctx.advance(1e9, max_steps=10)
        before = _outputs(ctx, all3)
        for ident, enable, cfg in refused:
            assert enable(ctx._h, C.byref(cfg)) == capi.SPHX_ERR_ARG
            assert L.sphx_last_error_id().decode() == ident
            _assert_same_bits(_outputs(ctx, all3), before, f"{name}: after the refused {ident}")
        assert ctx.advance(1e9, max_steps=5)["step"] == 15
        after = _outputs(ctx, all3)
    assert before["stats0/n_samples"] == 10 and before["field/n_samples"] == 10 and len(before["history/records"]) == 10
    assert after["stats0/n_samples"] == 15 and after["field/n_samples"] == 15
    assert list(after["history/records"][:, 0]) == list(range(1, 16))
    # ... and they are the samples of an undisturbed run of the same calls
    with capi.Context.from_parts(case[1], case[2], t_end=1e9, **case[3]) as ctx:
        _enable(ctx, case, all3)
        ctx.advance(1e9, max_steps=10)
        ctx.advance(1e9, max_steps=5)
        _assert_same_bits(after, _outputs(ctx, all3), f"{name}: 15 steps, against a run without refused enables")
