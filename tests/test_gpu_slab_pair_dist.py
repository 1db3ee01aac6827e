"""-m gpu: the pair statistics of a slab ring (include/sphx.h section 3a; k_pair_dist_s, sphx_slab_pairs_*), on in-process rings
(sphx_slab_group_run) on device 0, over the ring cases of tests/test_gpu_slab_samplers.py.  A slab counts the pairs whose CENTRE
it owns against everything it holds, halo copies included; the ring's histogram is the slabs' added up, its r2_min their
minimum.  Checked against the lattice table (exactly), against numpy's pair search over the owned particles of the snapshots
and against a single context stepped one step at a time -- by a rule on the CUMULATIVE counts that cannot hide a failure (see
_Bounds) --, for the gating, for leaving the ring and the other samplers bit for bit as they are -- chain, two-stream and
replayed-graph form --, for determinism, the lifecycle and the error identifiers."""
import ctypes as C

import numpy as np
import pytest

import pair_dist_cases as pc
import test_gpu_slab_samplers as rings  # the ring cases, their engines and calls, the guard: used as they are
from helpers import HISTORY_FIELDS, STATS_FIELDS, err_id, make_case, stats_bands

pytestmark = pytest.mark.gpu

CASES = rings.CASES
# A case whose state puts more pairs within tau of a bin edge than the tests below allow gets another seed here (case -> seed of
# make_case); none of rings.CASES needs one.
SEEDS = {}
N_BINS = 64


@pytest.fixture(scope="module")
def slab(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".slab")


_made = {}


def _case(cfgmod, geom, name):
    if name not in SEEDS:
        return rings._case(cfgmod, geom, name)
    if name not in _made:
        c = CASES[name]
        assert not c.get("leftward")
        _made[name] = make_case(cfgmod, geom, dp=c["dp"], DL=c["DL"], jitter=0.2, seed=SEEDS[name], developed=True, end_time=1e9)
    return _made[name]


class _Bounds:
    """What the ring's sums may be, from reference positions that agree with the ring's own only to a rounding: a halo copy's
    position is its owner's up to summation order, so a pair's r2 on the ring is the reference's r2 within tau.  For every band,
    kind and edge k the ring's CUMULATIVE count C_k = sum(counts[:k]) must lie in
        #(r2 < e2[k] - tau) <= C_k <= #(r2 < e2[k] + tau)
    over the reference pairs whose centre is in the band.  Where no pair lies within tau of an edge the two bounds coincide and
    the rule is equality, bin for bin; `ambiguous`, the sum over the edges of (upper - lower), counts the pairs that do, and
    the tests cap it -- a condition on the state, not a tolerance.  add(): one more sampled state (the bounds of the sums of
    several samples are the sums of the bounds)."""

    def __init__(self, profmod, prm, n_bins, r_max, y_margin, xbands, tau):
        self.profmod, self.prm, self.n_bins, self.r_max, self.y_margin, self.xbands, self.tau = profmod, prm, n_bins, r_max, y_margin, xbands, tau
        self.e2 = profmod.pair_edges(r_max, n_bins)[1]
        nb = 1 + len(xbands)
        self.lo = {k: np.zeros((nb, n_bins + 1), dtype=np.int64) for k in pc.COUNTS}
        self.hi = {k: np.zeros((nb, n_bins + 1), dtype=np.int64) for k in pc.COUNTS}
        self.plain = {k: np.zeros((nb, n_bins), dtype=np.int64) for k in pc.COUNTS}
        self.centres = np.zeros(nb, dtype=np.int64)
        self.r2_min = np.full(nb, np.inf)

    def add(self, pos, wall_pos):
        prm, profmod = self.prm, self.profmod
        sep = profmod.pair_separations(pos, prm.DL, self.r_max * (1.0 + 1e-6), wall_pos)  # (a superset: the pairs just outside too)
        centre = (pos[:, 1] >= self.y_margin) & (pos[:, 1] <= prm.DH - self.y_margin)
        members = [centre] + [centre & profmod.in_band(pos[:, 0], prm.DL, x, hw) for x, hw in self.xbands]
        for b, mine in enumerate(members):
            self.centres[b] += int(np.count_nonzero(mine))
            for kind in pc.COUNTS:
                i, r2 = sep["i_" + kind], sep["r2_" + kind]
                r2s = np.sort(r2[mine[i]])
                self.lo[kind][b] += np.searchsorted(r2s, self.e2 - self.tau, side="left")
                self.hi[kind][b] += np.searchsorted(r2s, self.e2 + self.tau, side="left")
                k = np.searchsorted(self.e2, r2s[r2s < self.e2[-1]], side="right") - 1
                self.plain[kind][b] += np.bincount(k, minlength=self.n_bins).astype(np.int64)
                if kind == "ff" and np.any(r2s < self.e2[-1]):
                    self.r2_min[b] = min(self.r2_min[b], float(r2s[0]))

    def check(self, got, cap, what, with_walls=True):
        """got: the ring's pooled sums, one dict per band -> (ambiguous pairs, bins that differ from the plain histogram) per band"""
        assert len(got) == len(self.centres), what
        figures = []
        for b, d in enumerate(got):
            assert int(d["centres"]) == int(self.centres[b]), f"{what} band {b}: centres {d['centres']}, reference {self.centres[b]}"
            ambiguous = differ = 0
            for kind in pc.COUNTS:
                counts = np.asarray(d[kind])
                assert counts.dtype == np.int64 and counts.shape == (self.n_bins,)
                if kind == "fw" and not with_walls:
                    assert counts.sum() == 0, f"{what} band {b}: fw without a wall histogram"
                    continue
                cum = np.concatenate([[0], np.cumsum(counts)])
                lo, hi = self.lo[kind][b], self.hi[kind][b]
                ambiguous += int(np.sum(hi - lo))
                differ += int(np.count_nonzero(counts != self.plain[kind][b]))
                bad = np.flatnonzero((cum < lo) | (cum > hi))
                assert len(bad) == 0, (f"{what} band {b} {kind}: cumulative count outside its bounds at edges {bad[:5].tolist()}: "
                                       f"{cum[bad[:5]].tolist()} not in [{lo[bad[:5]].tolist()}, {hi[bad[:5]].tolist()}]")
            want = self.r2_min[b]
            assert (np.isinf(want) and np.isinf(d["r2_min"])) or abs(d["r2_min"] - want) <= self.tau, f"{what} band {b}: r2_min {d['r2_min']!r} {want!r}"
            print(f"{what} band {b}: {ambiguous} pairs within tau of an edge, {differ} bins differ from the plain histogram")
            assert ambiguous <= cap, f"{what} band {b}: {ambiguous} pairs within tau of a bin edge, at most {cap} allowed: another seed (SEEDS)"
            figures.append((ambiguous, differ))
        return figures


def _owned_positions(snaps):
    return np.vstack([np.column_stack([s["x"][s["owned"]], s["y"][s["owned"]]]) for s in snaps])


def _ints(per_rank):
    """the integers (and r2_min bits, and the head) of every rank's sums, for comparisons to the last bit"""
    return [[(d["ff"].tobytes(), d["fw"].tobytes(), int(d["centres"]), np.float64(d["r2_min"]).tobytes(), d["n_samples"],
              np.float64(d["t_first"]).tobytes(), np.float64(d["t_last"]).tobytes()) for d in bands] for bands in per_rank]


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 4])
def test_lattice_table_on_a_ring(cfgmod, geom, slab, world):
    """The lattice at rest: no lattice distance lies within 1e-3 dp of a bin edge (the nearest is sqrt(5) dp at 55.04 bin widths)
    and one step moves nobody by 1e-4 dp (asserted below; the CPU oracle's first step moves the particles next to the walls by
    9.4e-6 dp), so no distance changes by 3e-4 dp and there is no tolerance: the table of the single context, count for count."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.0, seed=11, developed=False)
    nf = parts["n_fluid"]
    assert (nf, parts["n_total"] - nf) == (1200, 480)
    xbands = pc.bands(prm)  # mid-channel and the seam
    out = {}
    for y_margin in (0.0, 2.0 * prm.h):
        engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, native=True) for r in range(world)]
        try:
            for e in engines:
                e.pairs_part_enable(n_bins=N_BINS, every=1, with_walls=True, y_margin=y_margin, bands=xbands)
            slab.HipSlabEngine.group_run(engines, 1)
            sts = [e.sync() for e in engines]
            out[y_margin] = dict(per_rank=[e.pairs_part_sums() for e in engines], snaps=[e.snapshot() for e in engines],
                                 pooled=slab.ring_pair_dist(engines))
        finally:
            for e in engines:
                e.close()
        assert all(st["step"] == 1 for st in sts)
    whole, bulk = out[0.0], out[2.0 * prm.h]
    snaps = whole["snaps"]
    ids = np.concatenate([s["id"][s["owned"]] for s in snaps])
    pos = _owned_positions(snaps)
    assert sorted(ids.tolist()) == list(range(nf))
    moved = pos - parts["pos"][ids]
    moved[:, 0] -= prm.DL * np.round(moved[:, 0] / prm.DL)
    assert np.max(np.abs(moved)) <= 1e-4 * prm.dp  # (one step from rest)
    want = np.zeros(N_BINS, dtype=np.int64)
    for k, v in pc.LATTICE_FF.items():
        want[k] = v
    pooled = whole["pooled"]
    assert pooled[0]["ff"].dtype == np.int64 and np.array_equal(pooled[0]["ff"], want) and pooled[0]["ff"].sum() == 22680
    assert pooled[0]["fw"].sum() == pc.LATTICE_FW_TOTAL and pooled[0]["centres"] == nf
    assert (bulk["pooled"][0]["centres"], bulk["pooled"][0]["n_neigh"]) == pc.LATTICE_BULK
    assert abs(pooled[0]["r_min"] / prm.dp - 1.0) <= 3e-4
    # x = 0 and x = DL / 2 are equivalent lattice sites: the seam band, whose centres' partners come from across the seam as
    # copies at x - DL and x + DL, counts what the mid-channel band counts
    for run in (whole, bulk):
        mid, seam = run["pooled"][1], run["pooled"][2]
        assert mid["centres"] == seam["centres"] > 0
        assert np.array_equal(mid["ff"], seam["ff"]) and np.array_equal(mid["fw"], seam["fw"]) and mid["ff"].sum() > 0
    for r, (sums, s) in enumerate(zip(whole["per_rank"], snaps)):  # a slab's centres are the particles it owns
        assert sums[0]["centres"] == int(np.count_nonzero(s["owned"])), r
        assert sums[0]["n_samples"] == 1 and sums[0]["t_first"] == sums[0]["t_last"] == sts[0]["t"]
    assert sum(p[0]["centres"] for p in whole["per_rank"]) == nf


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, with_walls, margin_h", [("a", True, 0.0), ("a", False, 2.0), ("b", True, 2.0), ("b", False, 0.0), ("e", True, 0.0)])
def test_one_sample_is_numpys_pair_search_over_the_owned_particles(cfgmod, geom, capi, profmod, slab, name, with_walls, margin_h):
    """tau = 1e-10 r_max^2: a copy's x is its owner's within a few ulps, which puts r2 off by about 1e-13 r_max^2 at dp = 0.01; at
    most 2 pairs per band may lie within tau of an edge."""
    prm, parts = _case(cfgmod, geom, name)
    nf, steps = parts["n_fluid"], rings._steps(name)
    r_max, y_margin, xbands = 2.0 * prm.h, margin_h * prm.h, pc.bands(prm)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.pairs_part_enable(n_bins=N_BINS, every=steps, with_walls=with_walls, y_margin=y_margin, bands=xbands)  # only the last step
        sts = rings._run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        per_rank = [e.pairs_part_sums() for e in engines]
        got = slab.ring_pair_dist_sums(engines)
        rebinned = rings._last_step_rebinned(capi, engines[0])
    pos = _owned_positions(snaps)
    assert len(pos) == nf
    for sums in per_rank:
        for d in sums:
            assert d["n_samples"] == 1 and d["t_first"] == d["t_last"] == sts[0]["t"]
    pc.assert_counts_equal(got, slab.pool_ring_pair_dist(per_rank), f"{name}: ring_pair_dist_sums", head=True)
    ref = _Bounds(profmod, prm, N_BINS, r_max, y_margin, xbands, 1e-10 * r_max * r_max)
    ref.add(pos, parts["pos"][nf:] if with_walls else None)
    ref.check(got, 2, f"{name} walls={with_walls} y_margin={margin_h}h", with_walls)
    assert got[0]["ff"].sum() > 10 * nf * (1 if margin_h == 0.0 else 0.5) and (got[0]["fw"].sum() > 0) == (with_walls and margin_h == 0.0)
    if not rebinned and margin_h == 0.0:  # (a re-binning in the last step hands particles over behind the sample)
        for sums, s in zip(per_rank, snaps):
            y = s["y"][s["owned"]]
            assert sums[0]["centres"] == int(np.count_nonzero((y >= 0.0) & (y <= prm.DH)))


# 3 ---------------------------------------------------------------------------------------------------------------
_refs = {}


def _reference(cfgmod, geom, capi, profmod, name):
    """The single context of case `name`'s state, stepped one step at a time: the bounds of the sums of every step (tau = 1e-8
    r_max^2: rings._guard's docstring has ring and context agree to 1e-9 per particle), the context's own sampler, the guard."""
    c = CASES[name]
    steps = rings._steps(name)
    key = (c["dp"], c["DL"], SEEDS.get(name, c.get("seed", 11)), bool(c.get("leftward")), steps)  # (cases a and c: one state)
    if key not in _refs:
        prm, parts = _case(cfgmod, geom, name)
        nf, xbands, r_max = parts["n_fluid"], pc.bands(prm), 2.0 * prm.h
        ref = _Bounds(profmod, prm, N_BINS, r_max, 0.0, xbands, 1e-8 * r_max * r_max)
        guard = None
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.pair_dist_enable(n_bins=N_BINS, every=1, with_walls=True, bands=xbands)
            for k in range(steps):
                ctx.advance(1e9, max_steps=1)
                pos = ctx.download(fields=("pos",))["pos"]
                ref.add(pos[:nf], parts["pos"][nf:])  # (walls do not move)
                if guard is None:
                    try:
                        rings._guard(prm, pos[:nf], xbands, profmod.n_profile_bins(prm.DH, prm.dp), f"{name} step {k + 1}")
                    except AssertionError as e:
                        guard = str(e)
            sums = ctx.pair_dist_sums()
        _refs[key] = dict(bounds=ref, sums=sums, guard=guard)
    return _refs[key]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_sums_of_every_step_match_a_single_context(cfgmod, geom, capi, profmod, slab, name):
    """The runs cross the scheduled re-binning (a, c) and include leftward flow with x < 0 (b); at most 8 pairs per band may lie
    within tau of an edge over the whole run."""
    prm, parts = _case(cfgmod, geom, name)
    steps = rings._steps(name)
    ref = _reference(cfgmod, geom, capi, profmod, name)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.pairs_part_enable(n_bins=N_BINS, every=1, with_walls=True, bands=pc.bands(prm))
        rings._run(slab, engines, name)
        per_rank = [e.pairs_part_sums() for e in engines]
        got = slab.ring_pair_dist_sums(engines)
        if name == "b":
            assert min(float(np.min(e.snapshot()["x"])) for e in engines) < 0.0
    want = ref["sums"]
    for b in range(3):
        assert got[b]["n_samples"] == want[b]["n_samples"] == steps
        assert all(p[b]["n_samples"] == steps for p in per_rank)
        assert abs(got[b]["t_first"] - want[b]["t_first"]) <= 1e-12 * want[b]["t_first"]
        assert abs(got[b]["t_last"] - want[b]["t_last"]) <= 1e-12 * want[b]["t_last"]
    assert ref["guard"] is None, ref["guard"]  # (no particle near a band edge or y = 0, DH: the centres are the same particles)
    ref["bounds"].check(want, 8, f"{name}: the context's own sampler")  # (the reference positions are its own: the plain histogram)
    ref["bounds"].check(got, 8, f"{name}: ring against context")


# 4 ---------------------------------------------------------------------------------------------------------------
def test_gating_samples_the_steps_a_context_samples(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    steps = rings._steps("a")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.pair_dist_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        (want,) = ctx.pair_dist_sums()
    assert want["n_samples"] == 3  # steps 15, 20, 25
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.pairs_part_enable(every=5, t_from=t_from)
        rings._run(slab, engines, "a")
        got = [e.pairs_part_sums()[0] for e in engines]
    for g in got:
        assert g["n_samples"] == want["n_samples"]
        assert abs(g["t_first"] - want["t_first"]) <= 1e-12 * want["t_first"] and abs(g["t_last"] - want["t_last"]) <= 1e-12 * want["t_last"]
        assert pc.same_bits(g["t_first"], got[0]["t_first"]) and pc.same_bits(g["t_last"], got[0]["t_last"])
    assert sum(g["centres"] for g in got) == want["centres"] > 0


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_the_ring_and_the_other_samplers_do_not_feel_it(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form; flow
    statistics and history are on in both runs."""
    prm, parts = _case(cfgmod, geom, name)
    bands, steps = stats_bands(prm), rings._steps(name)
    runs = []
    for on in (False, True):
        with rings._ring(slab, prm, parts, name) as engines:
            for e in engines:
                e.flow_stats_enable(every=1, bands=bands)
                e.history_enable(every=1)
                if on:
                    e.pairs_part_enable(every=1, with_walls=True, bands=pc.bands(prm))
            rings._run(slab, engines, name)
            runs.append(dict(bits=rings._state_bits([e.snapshot() for e in engines]),
                             sums=[[e.flow_stats_sums(b) for b in range(3)] for e in engines],
                             hist=[e.history_records() for e in engines]))
            if on:
                assert all(e.pairs_part_sums()[0]["n_samples"] == steps for e in engines)
    off, on = runs
    assert off["bits"] == on["bits"]
    for r in range(len(off["sums"])):
        for b in range(3):
            for k in STATS_FIELDS + ("n_samples", "t_first", "t_last"):
                assert np.array_equal(off["sums"][r][b][k], on["sums"][r][b][k]), (r, b, k)
        assert off["hist"][r][1] == on["hist"][r][1] == 0 and off["hist"][r][0].shape == (steps, len(HISTORY_FIELDS))
        assert np.array_equal(off["hist"][r][0], on["hist"][r][0]), r


# 6 ---------------------------------------------------------------------------------------------------------------
def test_replayed_graph_eager_form_and_a_second_run_give_the_same_integers(cfgmod, geom, slab):
    """Case d: replays of the step graph, the same calls without graph_prepare, and those once more: every rank's integers."""
    prm, parts = _case(cfgmod, geom, "d")
    steps = rings._steps("d")
    runs = []
    for calls in (None, CASES["d"]["calls"], CASES["d"]["calls"]):  # (explicit calls: no graph)
        with rings._ring(slab, prm, parts, "d") as engines:
            for e in engines:
                e.pairs_part_enable(every=1, with_walls=True, bands=pc.bands(prm))
            rings._run(slab, engines, "d", calls=calls)
            runs.append([e.pairs_part_sums() for e in engines])
    assert all(p[0]["n_samples"] == steps and p[0]["centres"] > 0 for p in runs[0])
    assert _ints(runs[0]) == _ints(runs[1]), "replayed graph against eager form"
    assert _ints(runs[1]) == _ints(runs[2]), "two identical runs"


def test_enabling_after_graph_prepare_drops_the_graph_and_samples(cfgmod, geom, slab):
    """A graph prepared without the sampler carries no launch for it: enabling drops it, the loop runs eagerly and samples every
    step -- the integers of a ring that never had a graph."""
    prm, parts = _case(cfgmod, geom, "d")
    runs = []
    for graph in (True, False):
        with rings._ring(slab, prm, parts, "d") as engines:
            slab.HipSlabEngine.group_run(engines, 3)
            if graph:
                slab.HipSlabEngine.graph_prepare(engines)
            for e in engines:
                e.pairs_part_enable(every=1, bands=pc.bands(prm))
            slab.HipSlabEngine.group_run(engines, 25)
            for e in engines:
                e.sync()
            runs.append([e.pairs_part_sums() for e in engines])
    assert all(p[0]["n_samples"] == 25 for p in runs[0])
    assert _ints(runs[0]) == _ints(runs[1])


# 7 ---------------------------------------------------------------------------------------------------------------
def _empty(d):
    return (d["n_samples"] == 0 and d["ff"].sum() == 0 and d["fw"].sum() == 0 and d["centres"] == 0 and np.isinf(d["r2_min"])
            and np.isnan(d["t_first"]) and np.isnan(d["t_last"]))


def test_reset_and_disable_run_enable_start_from_zero(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.pairs_part_enable(every=1, with_walls=True, bands=pc.bands(prm))
        slab.HipSlabEngine.group_run(engines, 5)
        first = slab.ring_pair_dist_sums(engines)  # (no sync: the read waits for the slab's streams itself)
        slab.HipSlabEngine.group_run(engines, 2)
        for e in engines:  # (no sync: the samples of everything enqueued land before the sums are cleared)
            e.pairs_part_reset()
        cleared = [e.pairs_part_sums() for e in engines]
        slab.HipSlabEngine.group_run(engines, 2)
        resumed = slab.ring_pair_dist_sums(engines)
        for e in engines:  # (no sync in between: disable waits too)
            e.pairs_part_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.pairs_part_enable(every=1)
        before = [e.pairs_part_sums() for e in engines]
        slab.HipSlabEngine.group_run(engines, 3)
        after = slab.ring_pair_dist_sums(engines)
        sts = [e.sync() for e in engines]
    nf = parts["n_fluid"]
    assert sts[0]["step"] == 16
    assert first[0]["n_samples"] == 5 and 4 * nf < first[0]["centres"] <= 5 * nf and first[0]["fw"].sum() > 0
    assert all(_empty(d) for p in cleared for d in p) and all(len(p) == 3 for p in cleared)
    assert resumed[0]["n_samples"] == 2 and nf < resumed[0]["centres"] <= 2 * nf and resumed[0]["t_first"] > first[0]["t_last"]
    assert all(len(p) == 1 and _empty(p[0]) for p in before)
    assert len(after) == 1 and after[0]["n_samples"] == 3 and 2 * nf < after[0]["centres"] <= 3 * nf and after[0]["fw"].sum() == 0
    assert after[0]["t_last"] == sts[0]["t"]


def test_stale_contents_never_show(cfgmod, geom, capi, slab):
    """The sums of 3 x 2 x 1024 counters go back to the pool at disable and are filled with 0xFF words there: a counter of the
    smaller block that enable did not set would show."""
    prm, parts = _case(cfgmod, geom, "a")
    xbands = pc.bands(prm)
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.pairs_part_enable(every=1, n_bins=1024, with_walls=True, bands=xbands)
        slab.HipSlabEngine.group_run(engines, 4)
        assert all(e.pairs_part_sums()[0]["n_samples"] == 4 for e in engines)
        for e in engines:
            e.pairs_part_disable()
        assert capi.pool_scrub(0xFFFFFFFF) >= 1
        for e in engines:
            e.pairs_part_enable(every=1, n_bins=100, with_walls=True, bands=xbands)
        slab.HipSlabEngine.group_run(engines, 2)
        got = [e.pairs_part_sums() for e in engines]
    with rings._ring(slab, prm, parts, "a") as engines:  # a ring that enabled late
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.pairs_part_enable(every=1, n_bins=100, with_walls=True, bands=xbands)
        slab.HipSlabEngine.group_run(engines, 2)
        want = [e.pairs_part_sums() for e in engines]
    for r, (g, w) in enumerate(zip(got, want)):
        assert g[0]["n_samples"] == 2 and g[0]["ff"].shape == (100,) and np.any(g[0]["ff"] == 0) and g[0]["ff"].sum() > 0
        pc.assert_counts_equal(g, w, f"rank {r}: after re-enabling with fewer bins", head=True)


# 8 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    L = capi.lib()
    nothing = (None,) * 8

    def config(**kw):
        return capi.SphxPairDistConfig(**dict(dict(n_bins=64, every=1, t_from=0.0, r_max=0.0, y_margin=0.0, with_walls=0, n_bands=0), **kw))

    cfg = config()

    def calls(h):
        return [(L.sphx_slab_pairs_enable, h, C.byref(cfg)), (L.sphx_slab_pairs_disable, h), (L.sphx_slab_pairs_reset, h),
                (L.sphx_slab_pairs_read, h, 0, 0, *nothing)]

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
        for fn, args in ((L.sphx_slab_pairs_read, (0, 0, *nothing)), (L.sphx_slab_pairs_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:PairDist:disabled", capi.SPHX_ERR_STATE)
        for call in (e.pairs_part_sums, e.pairs_part_reset):
            with pytest.raises(capi.SphxError) as ei:
                call()
            assert ei.value.identifier == "SPHX:PairDist:disabled"
        assert L.sphx_slab_pairs_disable(h) == capi.SPHX_OK  # (off already)
        e.pairs_part_disable()
        for x in engines:
            x.pairs_part_enable(every=1, bands=pc.bands(prm))
        slab.HipSlabEngine.group_run(engines, 5)
        before = e.pairs_part_sums()
        assert before[0]["n_samples"] == 5
        # a bad config: the identifiers of section 2l, from the library and from the binding's own checks; the sums stay
        nan, two_h = float("nan"), 2.0 * prm.h
        for bad in (dict(n_bins=0), dict(n_bins=1025), dict(every=0), dict(t_from=nan), dict(r_max=-0.01), dict(r_max=np.nextafter(two_h, 1.0)),
                    dict(y_margin=-0.1), dict(with_walls=2), dict(n_bands=3)):
            c2 = config(**bad)
            assert err_id(capi, L.sphx_slab_pairs_enable, h, C.byref(c2)) == ("SPHX:PairDist:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_slab_pairs_enable, h, None) == ("SPHX:PairDist:config", capi.SPHX_ERR_ARG)
        for kw in (dict(r_max=2.5 * prm.h), dict(every=0), dict(n_bins=0), dict(bands=[(0.1, 0.1)] * 3)):
            with pytest.raises(capi.SphxError) as ei:
                e.pairs_part_enable(**kw)
            assert ei.value.identifier == "SPHX:PairDist:config"
        pc.assert_counts_equal(e.pairs_part_sums(), before, "a refused enable leaves the sums as they were", head=True)
        slab.HipSlabEngine.group_run(engines, 2)
        assert e.pairs_part_sums()[0]["n_samples"] == 7  # ... and the sampler running
        for band in (-1, 3):
            assert err_id(capi, L.sphx_slab_pairs_read, h, band, 0, *nothing) == ("SPHX:PairDist:band", capi.SPHX_ERR_ARG)
        ff, fw = np.full(64, -7, dtype=np.int64), np.full(64, -7, dtype=np.int64)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        assert err_id(capi, L.sphx_slab_pairs_read, h, 0, 63, None, i64(ff), *nothing[2:]) == ("SPHX:PairDist:capacity", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_slab_pairs_read, h, 0, 63, None, None, i64(fw), *nothing[3:]) == ("SPHX:PairDist:capacity", capi.SPHX_ERR_ARG)
        assert np.all(ff == -7) and np.all(fw == -7)
        nb, cen = C.c_int(0), C.c_int64(0)
        assert L.sphx_slab_pairs_read(h, 2, 0, C.byref(nb), None, None, C.byref(cen), *nothing[4:]) == capi.SPHX_OK  # no array: no capacity
        now = e.pairs_part_sums()
        assert (nb.value, cen.value) == (64, now[2]["centres"])
        assert L.sphx_slab_pairs_read(h, 0, 64, None, i64(ff), i64(fw), *nothing[3:]) == capi.SPHX_OK
        assert np.array_equal(ff, now[0]["ff"]) and np.all(fw == 0)  # (no wall histogram: zeros)
        # the context's calls keep refusing a slab
        for fn, args in ((L.sphx_ctx_pair_dist_enable, (C.byref(cfg),)), (L.sphx_ctx_pair_dist_disable, ()), (L.sphx_ctx_pair_dist_reset, ()),
                         (L.sphx_ctx_pair_dist_sample, ()), (L.sphx_ctx_pair_dist_read, (0, 0, *nothing))):
            assert err_id(capi, fn, h, *args) == ("SPHX:PairDist:slab", capi.SPHX_ERR_ARG)
        for x in engines:
            x.sync()
        assert e.pairs_part_sums()[0]["n_samples"] == 7
