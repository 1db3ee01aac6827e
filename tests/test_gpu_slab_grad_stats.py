"""-m gpu: the gradient statistics of a slab ring (include/sphx.h section 3a; k_grad_stats_s, sphx_slab_gstats_*), on in-process
rings (sphx_slab_group_run) on device 0, over the ring cases of tests/test_gpu_slab_samplers.py used as they are.  A slab bins
the estimates of the particles it OWNS, their partners taken from everything it holds, halo copies included -- positions,
velocities and masses at once, differentiated: the sampler that checks the halo exchange hardest.  The ring's sums are the
slabs' added up.  count and skipped are compared exactly, the summed fields within the bounds of
tests/slab_grad_stats_cases.py (derived from the measured SENSITIVITY; no figure of the code under test went into them).
Checked against numpy over the owned rows of the snapshots (pooled and per slab), against the flow statistics' count, against a
single context stepped one step at a time, at the LDS limit, for the gating, for leaving the ring and the other six samplers
bit for bit as they are -- chain, two-stream and replayed-graph form --, for determinism, the lifecycle and the error
identifiers.  The bands are grad_stats_cases.bands: mid-channel, which lies ON the cut of the two-slab rings, and the periodic
seam, whose partners are the copies at x - DL / x + DL."""
import ctypes as C

import numpy as np
import pytest

import grad_stats_cases as gc
import pair_dist_cases as pc
import slab_grad_stats_cases as sc
import test_gpu_slab_samplers as rings  # the ring cases, their engines and calls, the guard: used as they are
from helpers import err_id, stats_bands

pytestmark = pytest.mark.gpu

CASES = rings.CASES


@pytest.fixture(scope="module")
def slab(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".slab")


def _per_rank(engines, n_bands=3):
    return [[e.grads_part_sums(b) for b in range(n_bands)] for e in engines]


def _bits(per_rank):
    """every field and the head of every rank's sums, for comparisons to the last bit"""
    return [[tuple(np.asarray(d[f]).tobytes() for f in gc.FIELDS) + (d["n_samples"], np.float64(d["t_first"]).tobytes(),
                                                                       np.float64(d["t_last"]).tobytes()) for d in bands] for bands in per_rank]


def _blob(x):
    """anything a sampler's read returns, as something == compares to the last bit"""
    if isinstance(x, dict):
        return tuple((k, _blob(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_blob(v) for v in x)
    if x is None or isinstance(x, (str, bool, int)):
        return x
    return np.asarray(x).tobytes()


def _owned_rows(prm, parts, snaps):
    """the owned rows of the snapshots, pooled in rank order: pos, vel, vol (the masses go by id), the rank of every row"""
    pos = np.vstack([np.column_stack([s["x"][s["owned"]], s["y"][s["owned"]]]) for s in snaps])
    vel = np.vstack([np.column_stack([s["vx"][s["owned"]], s["vy"][s["owned"]]]) for s in snaps])
    ids = np.concatenate([s["id"][s["owned"]] for s in snaps])
    rank = np.concatenate([np.full(int(s["owned"].sum()), r) for r, s in enumerate(snaps)])
    assert sorted(ids.tolist()) == list(range(parts["n_fluid"]))
    return pos, vel, parts["mass"][ids] / prm.rho0, rank, ids


def _d_copy(prm, snaps, pos, vel, ids):
    """the largest deviation of a copy's position or velocity, as the snapshots show it, from its owner's row"""
    row_of = np.empty(len(ids), dtype=np.int64)
    row_of[ids] = np.arange(len(ids))
    worst = 0.0
    for s in snaps:
        c = ~s["owned"]
        o = row_of[s["id"][c]]
        dx = s["x"][c] - pos[o, 0]
        dx -= prm.DL * np.round(dx / prm.DL)
        for d in (dx, s["y"][c] - pos[o, 1], s["vx"][c] - vel[o, 0], s["vy"][c] - vel[o, 1]):
            worst = max(worst, float(np.max(np.abs(d))) if len(d) else 0.0)
    return worst


def _conditions(g, det_min, bound, what):
    """not tolerances: a state that meets one needs another seed"""
    near = int(np.count_nonzero(np.abs(g["det"] - det_min) < sc.EDGE))
    assert near == 0, f"{what}: {near} particles with det M within 1e-6 of det_min: another seed"
    near = int(np.count_nonzero(np.abs(np.abs(g["G"]) - bound) < sc.EDGE))
    assert near == 0, f"{what}: {near} components within 1e-6 of the bound: another seed"


def _subset(profmod, prm, pos, vel, vol, g, rows, n_bins, xbands, det_min, vmax):
    """the reference's per-particle estimates binned over `rows` alone"""
    return profmod.grad_stats_sums(pos[rows], vel[rows], vol[rows], prm.DL, prm.DH, prm.h, n_bins, bands=xbands, det_min=det_min, vmax=vmax,
                                   gradients=dict(G=g["G"][rows], det=g["det"][rows]))


def _walls(prm, parts, with_walls):
    return gc.walls_of(prm, parts) if with_walls else {}


# 1 ---------------------------------------------------------------------------------------------------------------
def _one_sample(cfgmod, geom, capi, profmod, slab, name, with_walls, det_min, n_bins=0):
    prm, parts = rings._case(cfgmod, geom, name)
    nf, steps, xbands = parts["n_fluid"], rings._steps(name), gc.bands(prm)
    what = f"{name} walls={with_walls} det_min={det_min:.6g}"
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.grads_part_enable(n_bins=n_bins, every=steps, det_min=det_min, with_walls=with_walls, bands=xbands)  # only the last step
        sts = rings._run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        per_rank = _per_rank(engines)
        got = slab.ring_grad_stats_sums(engines)
        figures = slab.ring_grad_stats(engines)
        rebinned = rings._last_step_rebinned(capi, engines[0])
    n_bins = n_bins or profmod.n_profile_bins(prm.DH, prm.dp)
    vmax = sts[0]["vmax"]
    assert all(st["vmax"] == vmax and st["t"] == sts[0]["t"] for st in sts)
    for sums in per_rank:  # every slab stamps the sample, whatever it owns
        for d in sums:
            assert d["n_samples"] == 1 and d["t_first"] == d["t_last"] == sts[0]["t"]
    gc.assert_identical(got, [slab.pool_ring_grad_stats([p[b] for p in per_rank]) for b in range(3)], f"{what}: ring_grad_stats_sums")
    assert np.array_equal(figures[0]["count"], got[0]["count"]) and figures[0]["gxy_mean"].shape == (n_bins,)

    pos, vel, vol, rank, ids = _owned_rows(prm, parts, snaps)
    d_copy = _d_copy(prm, snaps, pos, vel, ids)
    print(f"{what}: d_copy as the snapshots show it (behind phase 3, the copies refreshed) {d_copy:.3e}; assumed for the sampling point "
          f"{sc.D_COPY:.1e} (profiles/r25_slab_point_probes.txt)")
    assert d_copy <= sc.D_COPY
    rings._guard(prm, pos, xbands, n_bins, what)
    g = profmod.velocity_gradients(pos, vel, vol, prm.DL, prm.h, **_walls(prm, parts, with_walls))
    bound = profmod.grad_scales(vmax, prm.h, nf)["bound"]
    _conditions(g, det_min, bound, what)
    want = profmod.grad_stats_sums(pos, vel, vol, prm.DL, prm.DH, prm.h, n_bins, bands=xbands, det_min=det_min, vmax=vmax, gradients=g)
    # per slab: the reference's estimates over the rows that slab owns, the quantisation term of that slab's own scales
    quant = None
    for r, (sums, s) in enumerate(zip(per_rank, snaps)):
        want_r = _subset(profmod, prm, pos, vel, vol, g, rank == r, n_bins, xbands, det_min, vmax)
        scales = profmod.grad_scales(vmax, prm.h, len(s["id"]))  # (the count the slab holds)
        assert scales["bound"] == bound
        q_r = gc.quantisation(want_r, scales)
        quant = q_r if quant is None else gc.add_quantisation(quant, q_r)
        if not rebinned:  # (a re-binning in the last step hands particles over behind the sample: the snapshot shows the new owners)
            gc.assert_sums_match(sums, want_r, q_r, f"{what} rank {r}", bound=sc.BOUND_ONE_SAMPLE)
            y = s["y"][s["owned"]]
            assert sums[0]["count"].sum() + sums[0]["skipped"].sum() == int(np.count_nonzero((y >= 0.0) & (y <= prm.DH))), r
    gc.assert_sums_match(got, want, quant, f"{what} pooled", bound=sc.BOUND_ONE_SAMPLE)
    dev = gc.deviation(got, want)
    print(f"{what}: pooled sums off by {dev[0]:.3e} ({dev[1]}, band {dev[2]}); rebinned in the last step: {rebinned}")
    assert got[0]["count"].sum() + got[0]["skipped"].sum() == nf and got[1]["count"].sum() > 0 and got[2]["count"].sum() > 0
    return got, per_rank


@pytest.mark.parametrize("name, with_walls", [("a", True), ("a", False), ("b", True), ("e", False)])
def test_one_sample_is_numpys_over_what_the_ring_holds(cfgmod, geom, capi, profmod, slab, name, with_walls):
    """(b: leftward flow, x < 0, three slabs; e: several workgroups per slab)"""
    got, _ = _one_sample(cfgmod, geom, capi, profmod, slab, name, with_walls, 0.05)
    assert got[0]["skipped"].sum() == 0


def test_one_sample_with_particles_skipped(cfgmod, geom, capi, profmod, slab):
    """det_min from a CPU census (numpy) of det M of the very state that is sampled -- the ring is run once without the sampler
    to learn it; a second run is the same state to the bit --, in the first gap of at least 1e-4 with 20 or more particles
    below it: the wall-adjacent particles, whose one-sided support leaves the smallest det M without wall partners, ARE skipped,
    on both slabs."""
    prm, parts = rings._case(cfgmod, geom, "a")
    with rings._ring(slab, prm, parts, "a") as engines:
        rings._run(slab, engines, "a")
        snaps = [e.snapshot() for e in engines]
    pos, vel, vol, _, _ = _owned_rows(prm, parts, snaps)
    det = profmod.velocity_gradients(pos, vel, vol, prm.DL, prm.h)["det"]
    det_min, below = sc.det_min_that_skips(det)
    near_wall = np.minimum(pos[:, 1], prm.DH - pos[:, 1]) < 2.0 * prm.h
    assert np.all(near_wall[det < det_min])
    print(f"det_min {det_min:.6f}: {below} particles of the sampled state below it, all within 2h of a wall; min det M {det.min():.4f}")
    got, per_rank = _one_sample(cfgmod, geom, capi, profmod, slab, "a", False, det_min)
    assert got[0]["skipped"].sum() == below >= 20 and got[0]["count"].sum() > got[0]["skipped"].sum()
    assert all(p[0]["skipped"].sum() > 0 for p in per_rank)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_count_plus_skipped_is_the_flow_statistics_count(cfgmod, geom, slab, name):
    prm, parts = rings._case(cfgmod, geom, name)
    steps = rings._steps(name)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.flow_stats_enable(every=1, bands=gc.bands(prm))
            e.grads_part_enable(every=1, bands=gc.bands(prm))
        rings._run(slab, engines, name)
        grads = _per_rank(engines)
        stats = [[e.flow_stats_sums(b) for b in range(3)] for e in engines]
    for r, (g, f) in enumerate(zip(grads, stats)):
        for b in range(3):
            assert g[b]["n_samples"] == f[b]["n_samples"] == steps
            assert np.array_equal(g[b]["count"] + g[b]["skipped"], f[b]["count"]), (name, r, b)
    assert sum(g[0]["count"].sum() for g in grads) > 0.9 * steps * parts["n_fluid"]


# 3 ---------------------------------------------------------------------------------------------------------------
_refs = {}


def _reference(cfgmod, geom, capi, profmod, name):
    """The single context of case `name`'s state stepped one step at a time: its sums, the quantisation terms of its samples, the
    guard and the conditions on every step's state."""
    c = CASES[name]
    steps = rings._steps(name)
    key = (c["dp"], c["DL"], c.get("seed", 11), bool(c.get("leftward")), steps)  # (cases a and c: one state)
    if key not in _refs:
        prm, parts = rings._case(cfgmod, geom, name)
        nf, xbands = parts["n_fluid"], gc.bands(prm)
        n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
        vol = parts["mass"][:nf] / prm.rho0
        quant, trouble = None, None
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.grad_stats_enable(every=1, with_walls=True, bands=xbands)
            for k in range(steps):
                st = ctx.advance(1e9, max_steps=1)
                state = ctx.download(fields=("pos", "vel"))
                pos, vel = state["pos"][:nf], state["vel"][:nf]
                g = profmod.velocity_gradients(pos, vel, vol, prm.DL, prm.h, **gc.walls_of(prm, parts))
                scales = profmod.grad_scales(st["vmax"], prm.h, nf)
                one = profmod.grad_stats_sums(pos, vel, vol, prm.DL, prm.DH, prm.h, n_bins, bands=xbands, vmax=st["vmax"], gradients=g)
                q = gc.quantisation(one, scales)
                quant = q if quant is None else gc.add_quantisation(quant, q)
                if trouble is None:
                    try:
                        rings._guard(prm, pos, xbands, n_bins, f"{name} step {k + 1}")
                        _conditions(g, 0.05, scales["bound"], f"{name} step {k + 1}")
                    except AssertionError as e:
                        trouble = str(e)
            sums = [ctx.grad_stats_sums(b) for b in range(3)]
        _refs[key] = dict(sums=sums, quant=quant, trouble=trouble)
    return _refs[key]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_sums_of_every_step_match_a_single_context(cfgmod, geom, capi, profmod, slab, name):
    """The runs cross the scheduled re-binning (a, c), include leftward flow with x < 0 (b) and the two-stream form (c).  The
    quantisation term is the context's samples' plus as much again for the slabs': a slab holds fewer particles than the channel,
    so its quantum is no coarser than the context's."""
    prm, parts = rings._case(cfgmod, geom, name)
    steps = rings._steps(name)
    ref = _reference(cfgmod, geom, capi, profmod, name)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.grads_part_enable(every=1, with_walls=True, bands=gc.bands(prm))
        rings._run(slab, engines, name)
        per_rank = _per_rank(engines)
        got = slab.ring_grad_stats_sums(engines)
        if name == "b":
            assert min(float(np.min(e.snapshot()["x"])) for e in engines) < 0.0
    want = ref["sums"]
    for b in range(3):
        assert got[b]["n_samples"] == want[b]["n_samples"] == steps
        assert all(p[b]["n_samples"] == steps for p in per_rank)
        assert abs(got[b]["t_first"] - want[b]["t_first"]) <= 1e-12 * want[b]["t_first"]
        assert abs(got[b]["t_last"] - want[b]["t_last"]) <= 1e-12 * want[b]["t_last"]
        assert all(pc.same_bits(p[b]["t_last"], per_rank[0][b]["t_last"]) for p in per_rank)
    assert ref["trouble"] is None, ref["trouble"]
    quant = gc.add_quantisation(ref["quant"], ref["quant"])
    gc.assert_sums_match(got, want, quant, f"{name}: ring against context", bound=sc.BOUND_EVERY_STEP)
    dev = gc.deviation(got, want)
    print(f"{name}: ring against context over {steps} steps off by {dev[0]:.3e} ({dev[1]}, band {dev[2]})")


# 4 ---------------------------------------------------------------------------------------------------------------
def test_the_lds_limit_on_a_ring(cfgmod, geom, capi, profmod, slab):
    """213 bins in three bands: 639 of the 640 counters, 61 344 B of dynamic LDS for k_grad_stats_s.  Counts against numpy over the
    owned rows of the snapshots; every step of a few is sampled, the last is compared through `every`."""
    prm, parts = rings._case(cfgmod, geom, "a")
    xbands, n_bins = gc.bands(prm), gc.BINS[-1]
    assert 3 * n_bins == profmod.GRAD_MAX_BINS - 1
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.grads_part_enable(n_bins=n_bins, every=4, bands=xbands)
        slab.HipSlabEngine.group_run(engines, 4)
        sts = [e.sync() for e in engines]
        snaps = [e.snapshot() for e in engines]
        got = slab.ring_grad_stats_sums(engines)
        with pytest.raises(capi.SphxError) as ei:  # one bin more does not fit
            engines[0].grads_part_enable(n_bins=n_bins + 1, every=4, bands=xbands)
        assert ei.value.identifier == "SPHX:GradStats:config"
        assert engines[0].grads_part_sums(0)["n_samples"] == 1
    pos, vel, vol, _, _ = _owned_rows(prm, parts, snaps)
    rings._guard(prm, pos, xbands, n_bins, "the LDS limit")
    want = profmod.grad_stats_sums(pos, vel, vol, prm.DL, prm.DH, prm.h, n_bins, bands=xbands, vmax=sts[0]["vmax"])
    for b in range(3):
        assert got[b]["count"].shape == (n_bins,) and got[b]["n_samples"] == 1
        for f in gc.COUNTS:
            assert np.array_equal(got[b][f], want[b][f]), (b, f)
    assert got[0]["count"].sum() == parts["n_fluid"] and np.count_nonzero(got[0]["count"]) > 50


# 5 ---------------------------------------------------------------------------------------------------------------
def test_gating_samples_the_steps_a_context_samples(cfgmod, geom, capi, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    steps = rings._steps("a")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.grad_stats_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        want = ctx.grad_stats_sums(0)
    assert want["n_samples"] == 3  # steps 15, 20, 25
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.grads_part_enable(every=5, t_from=t_from)
        rings._run(slab, engines, "a")
        got = [e.grads_part_sums(0) for e in engines]
    for g in got:
        assert g["n_samples"] == want["n_samples"]
        assert abs(g["t_first"] - want["t_first"]) <= 1e-12 * want["t_first"] and abs(g["t_last"] - want["t_last"]) <= 1e-12 * want["t_last"]
        assert pc.same_bits(g["t_first"], got[0]["t_first"]) and pc.same_bits(g["t_last"], got[0]["t_last"])
    assert sum(g["count"].sum() + g["skipped"].sum() for g in got) == want["count"].sum() + want["skipped"].sum() > 0


# 6 ---------------------------------------------------------------------------------------------------------------
def _others_on(prm, e):
    """the other six samplers, every step"""
    e.flow_stats_enable(every=1, bands=stats_bands(prm))
    e.history_enable(every=1)
    e.field_part_enable(nx=24, ny=9, every=1, with_walls=True)
    pts = np.array([[0.25 * prm.DL, 0.5 * prm.DH], [0.5 * prm.DL, 0.1 * prm.DH], [0.0, 0.5 * prm.DH], [0.9 * prm.DL, 0.8 * prm.DH]])
    e.probes_part_enable(pts, every=1, with_walls=True)
    e.profile_series_enable(every=1, bands=stats_bands(prm))
    e.pairs_part_enable(every=1, with_walls=True, bands=pc.bands(prm))


def _others_read(e):
    return _blob([[e.flow_stats_sums(b) for b in range(3)], e.history_records()[0], e.field_part_sums(), e.probes_part_records(),
                  e.profile_series_sums(), e.pairs_part_sums()])


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_the_ring_and_the_other_samplers_do_not_feel_it(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form; the other
    six samplers are on in both runs."""
    prm, parts = rings._case(cfgmod, geom, name)
    steps = rings._steps(name)
    runs = []
    for on in (False, True):
        with rings._ring(slab, prm, parts, name) as engines:
            for e in engines:
                _others_on(prm, e)
                if on:
                    e.grads_part_enable(every=1, with_walls=True, bands=gc.bands(prm))
            rings._run(slab, engines, name)
            runs.append(dict(bits=rings._state_bits([e.snapshot() for e in engines]), others=[_others_read(e) for e in engines]))
            if on:
                assert all(e.grads_part_sums(0)["n_samples"] == steps and e.grads_part_sums(0)["count"].sum() > 0 for e in engines)
    off, on = runs
    assert off["bits"] == on["bits"]
    for r in range(len(off["others"])):
        assert off["others"][r] == on["others"][r], r


# 6, 7 ------------------------------------------------------------------------------------------------------------
def test_replayed_graph_eager_form_and_a_second_run_give_the_same_bytes(cfgmod, geom, slab):
    """Case d: replays of the step graph, the same calls without graph_prepare, and those once more: every rank's bytes."""
    prm, parts = rings._case(cfgmod, geom, "d")
    steps = rings._steps("d")
    runs = []
    for calls in (None, CASES["d"]["calls"], CASES["d"]["calls"]):  # (explicit calls: no graph)
        with rings._ring(slab, prm, parts, "d") as engines:
            for e in engines:
                e.grads_part_enable(every=1, with_walls=True, bands=gc.bands(prm))
            rings._run(slab, engines, "d", calls=calls)
            runs.append(_per_rank(engines))
    assert all(p[0]["n_samples"] == steps and p[0]["count"].sum() > 0 for p in runs[0])
    assert _bits(runs[0]) == _bits(runs[1]), "replayed graph against eager form"
    assert _bits(runs[1]) == _bits(runs[2]), "two identical runs"


def test_enabling_after_graph_prepare_drops_the_graph_and_samples(cfgmod, geom, slab):
    """A graph prepared without the sampler carries no launch for it: enabling drops it, the loop runs eagerly and samples every
    step -- the bytes of a ring that never had a graph."""
    prm, parts = rings._case(cfgmod, geom, "d")
    runs = []
    for graph in (True, False):
        with rings._ring(slab, prm, parts, "d") as engines:
            slab.HipSlabEngine.group_run(engines, 3)
            if graph:
                slab.HipSlabEngine.graph_prepare(engines)
            for e in engines:
                e.grads_part_enable(every=1, bands=gc.bands(prm))
            slab.HipSlabEngine.group_run(engines, 25)
            for e in engines:
                e.sync()
            runs.append(_per_rank(engines))
    assert all(p[0]["n_samples"] == 25 for p in runs[0])
    assert _bits(runs[0]) == _bits(runs[1])


# 8 ---------------------------------------------------------------------------------------------------------------
def _empty(d):
    return (d["n_samples"] == 0 and all(not np.any(d[f]) for f in gc.FIELDS) and np.isnan(d["t_first"]) and np.isnan(d["t_last"]))


def test_reset_and_disable_run_enable_start_from_zero(cfgmod, geom, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.grads_part_enable(every=1, with_walls=True, bands=gc.bands(prm))
        slab.HipSlabEngine.group_run(engines, 5)
        first = slab.ring_grad_stats_sums(engines)  # (no sync: the read waits for the slab's streams itself)
        slab.HipSlabEngine.group_run(engines, 2)
        for e in engines:  # (no sync: the samples of everything enqueued land before the sums are cleared)
            e.grads_part_reset()
        cleared = _per_rank(engines)
        slab.HipSlabEngine.group_run(engines, 2)
        resumed = slab.ring_grad_stats_sums(engines)
        for e in engines:  # (no sync in between: disable waits too)
            e.grads_part_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.grads_part_enable(every=1, n_bins=7)
        before = _per_rank(engines, 1)
        slab.HipSlabEngine.group_run(engines, 3)
        after = slab.ring_grad_stats_sums(engines)
        sts = [e.sync() for e in engines]
    nf = parts["n_fluid"]
    assert sts[0]["step"] == 16
    assert first[0]["n_samples"] == 5 and first[0]["count"].sum() + first[0]["skipped"].sum() == 5 * nf
    assert all(_empty(d) for p in cleared for d in p) and all(len(p) == 3 for p in cleared)
    assert resumed[0]["n_samples"] == 2 and resumed[0]["count"].sum() + resumed[0]["skipped"].sum() == 2 * nf
    assert resumed[0]["t_first"] > first[0]["t_last"]
    assert all(_empty(p[0]) and p[0]["count"].shape == (7,) for p in before)
    assert len(after) == 1 and after[0]["n_samples"] == 3 and after[0]["count"].sum() + after[0]["skipped"].sum() == 3 * nf
    assert after[0]["t_last"] == sts[0]["t"]


# 9 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    L = capi.lib()
    nothing = (None,) * 5

    def config(**kw):
        return capi.SphxGradStatsConfig(**dict(dict(n_bins=0, every=1, t_from=0.0, det_min=0.05, with_walls=0, n_bands=0), **kw))

    cfg = config()

    def calls(h):
        return [(L.sphx_slab_gstats_enable, h, C.byref(cfg)), (L.sphx_slab_gstats_disable, h), (L.sphx_slab_gstats_reset, h),
                (L.sphx_slab_gstats_read, h, 0, 0, *nothing)]

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
        for fn, args in ((L.sphx_slab_gstats_read, (0, 0, *nothing)), (L.sphx_slab_gstats_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:GradStats:disabled", capi.SPHX_ERR_STATE)
        for call in (e.grads_part_sums, e.grads_part_reset):
            with pytest.raises(capi.SphxError) as ei:
                call()
            assert ei.value.identifier == "SPHX:GradStats:disabled"
        assert L.sphx_slab_gstats_disable(h) == capi.SPHX_OK  # (off already)
        e.grads_part_disable()
        for x in engines:
            x.grads_part_enable(every=1, bands=gc.bands(prm))
        slab.HipSlabEngine.group_run(engines, 5)
        before = _per_rank([e])
        assert before[0][0]["n_samples"] == 5
        # a bad config: the identifiers of section 2n, from the library and from the binding's own checks; the sums stay
        nan = float("nan")
        for bad in (dict(n_bins=-1), dict(n_bins=641), dict(every=0), dict(t_from=nan), dict(det_min=-0.01), dict(det_min=nan), dict(with_walls=2),
                    dict(n_bands=3)):
            c2 = config(**bad)
            assert err_id(capi, L.sphx_slab_gstats_enable, h, C.byref(c2)) == ("SPHX:GradStats:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_slab_gstats_enable, h, None) == ("SPHX:GradStats:config", capi.SPHX_ERR_ARG)
        for kw in (dict(det_min=-1.0), dict(every=0), dict(n_bins=641), dict(bands=[(0.1, 0.1)] * 3)):
            with pytest.raises(capi.SphxError) as ei:
                e.grads_part_enable(**kw)
            assert ei.value.identifier == "SPHX:GradStats:config"
        gc.assert_identical(_per_rank([e])[0], before[0], "a refused enable leaves the sums as they were")
        slab.HipSlabEngine.group_run(engines, 2)
        assert e.grads_part_sums(0)["n_samples"] == 7  # ... and the sampler running
        for band in (-1, 3):
            assert err_id(capi, L.sphx_slab_gstats_read, h, band, 0, *nothing) == ("SPHX:GradStats:band", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as ei:
            e.grads_part_sums(3)
        assert ei.value.identifier == "SPHX:GradStats:band"
        n_bins = len(before[0][0]["count"])
        sums = np.full((len(gc.FIELDS), n_bins), -7.0)
        assert err_id(capi, L.sphx_slab_gstats_read, h, 0, n_bins - 1, None, capi.ptr(sums), *nothing[2:]) == ("SPHX:GradStats:capacity", capi.SPHX_ERR_ARG)
        assert np.all(sums == -7.0)
        nb, ns = C.c_int(0), C.c_int64(0)
        assert L.sphx_slab_gstats_read(h, 2, 0, C.byref(nb), None, C.byref(ns), None, None) == capi.SPHX_OK  # no array: no capacity
        assert (nb.value, ns.value) == (n_bins, 7)
        # the context's calls keep refusing a slab
        for fn, args in ((L.sphx_ctx_grad_stats_enable, (C.byref(cfg),)), (L.sphx_ctx_grad_stats_disable, ()), (L.sphx_ctx_grad_stats_reset, ()),
                         (L.sphx_ctx_grad_stats_sample, ()), (L.sphx_ctx_grad_stats_read, (0, 0, *nothing))):
            assert err_id(capi, fn, h, *args) == ("SPHX:GradStats:slab", capi.SPHX_ERR_ARG)
        for x in engines:
            x.sync()
        assert e.grads_part_sums(0)["n_samples"] == 7
