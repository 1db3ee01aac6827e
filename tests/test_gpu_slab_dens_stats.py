"""-m gpu: the density statistics of a slab ring (include/sphx.h section 3a; k_dens_stats_s, sphx_slab_dstats_*), on in-process
rings (sphx_slab_group_run) on device 0, over the ring cases of tests/test_gpu_slab_samplers.py used as they are.  A slab bins
the re-summed densities of the particles it OWNS; a density takes the POSITION of every partner the slab holds, halo copies --
those from across the seam at x - DL / x + DL -- and the slab's wall particles in the first halo column included: a missing or
stale copy changes every partner's density, so this is the sampler that checks where the copies ARE.  The ring's sums are the
slabs' added up, its extremes their minimum / maximum.  The integers are compared exactly but for the particles the reference
state holds at an edge (`loose`), the summed fields and extremes within the bounds of tests/slab_dens_stats_cases.py (derived
from the measured SENSITIVITY; no figure of the code under test went into them).  Checked against numpy over the owned rows of
the snapshots (pooled and per slab), against the flow statistics' count, against a single context stepped one step at a time,
on the lattice at rest, for outliers, at the LDS limit, for the gating, for leaving the ring and the other eight samplers bit
for bit as they are -- chain, two-stream and replayed-graph form --, for determinism, the lifecycle and the error identifiers."""
import ctypes as C

import numpy as np
import pytest

import dens_stats_cases as dc
import pair_dist_cases as pc
import slab_dens_stats_cases as sc
import test_gpu_slab_samplers as rings  # the ring cases, their engines and calls, the guard: used as they are
from helpers import err_id, make_case, stats_bands

pytestmark = pytest.mark.gpu

CASES = rings.CASES
DEFAULT_HIST = dict(n_hist=64, hist_range=0.05)


@pytest.fixture(scope="module")
def slab(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".slab")


def _per_rank(engines, n_bands=3):
    return [[e.dens_part_sums(b) for b in range(n_bands)] for e in engines]


def _bits(per_rank):
    """every field, the histogram and the head of every rank's sums, for comparisons to the last bit"""
    return [[tuple(np.asarray(d[f]).tobytes() for f in dc.FIELDS + ("hist",)) + (d["below"], d["above"], d["n_samples"],
                                                                                np.float64(d["t_first"]).tobytes(), np.float64(d["t_last"]).tobytes())
             for d in bands] for bands in per_rank]


def _blob(x):
    """anything a sampler's read returns, as something == compares to the last bit"""
    if isinstance(x, dict):
        return tuple((k, _blob(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_blob(v) for v in x)
    if x is None or isinstance(x, (str, bool, int)):
        return x
    return np.asarray(x).tobytes()


def _owned_rows(parts, snaps):
    """the owned rows of the snapshots, pooled in rank order: pos, mass (by id), the rank of every row"""
    pos = np.vstack([np.column_stack([s["x"][s["owned"]], s["y"][s["owned"]]]) for s in snaps])
    ids = np.concatenate([s["id"][s["owned"]] for s in snaps])
    rank = np.concatenate([np.full(int(s["owned"].sum()), r) for r, s in enumerate(snaps)])
    assert sorted(ids.tolist()) == list(range(parts["n_fluid"]))
    return pos, parts["mass"][ids], rank


def _density(profmod, prm, parts, pos, mass):
    """the single-context definition over the pooled owned rows: the whole, periodic channel and all of its wall particles"""
    return profmod.summation_density(pos, mass, prm.DL, prm.h, prm.rho0, prm.inv_sigma0, **sc.walls_of(prm, parts))


def _sums(profmod, prm, pos, mass, dens, rows, n_bins, xbands, **setting):
    """the reference's per-particle densities binned over `rows` alone"""
    return profmod.dens_stats_sums(pos[rows], mass[rows], prm.DL, prm.DH, prm.h, prm.rho0, prm.inv_sigma0, n_bins, bands=xbands,
                                   density=(dens[0][rows], dens[1][rows]), **setting)


def _counts(sums):
    return [b["count"].sum() for b in sums]


# 1 ---------------------------------------------------------------------------------------------------------------
def _one_sample(cfgmod, geom, capi, profmod, slab, name, n_bins=0, **setting):
    prm, parts = rings._case(cfgmod, geom, name)
    nf, steps, xbands = parts["n_fluid"], rings._steps(name), dc.bands(prm)
    hist = {k: setting.get(k, DEFAULT_HIST[k]) for k in DEFAULT_HIST}
    delta_bound = setting.get("delta_bound", 0.5)
    what = f"{name} {setting}"
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.dens_part_enable(n_bins=n_bins, every=steps, bands=xbands, **setting)  # only the last step
        sts = rings._run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        per_rank = _per_rank(engines)
        got = slab.ring_dens_stats_sums(engines)
        figures = slab.ring_dens_stats(engines)
        rebinned = rings._last_step_rebinned(capi, engines[0])
    n_bins = n_bins or profmod.n_profile_bins(prm.DH, prm.dp)
    assert all(st["t"] == sts[0]["t"] for st in sts)
    for sums in per_rank:  # every slab stamps the sample, whatever it owns
        for d in sums:
            assert d["n_samples"] == 1 and d["t_first"] == d["t_last"] == sts[0]["t"]
    dc.assert_identical(got, [slab.pool_ring_dens_stats([p[b] for p in per_rank]) for b in range(3)], f"{what}: ring_dens_stats_sums")
    assert np.array_equal(figures[0]["count"], got[0]["count"]) and figures[0]["d_mean"].shape == (n_bins,)

    pos, mass, rank = _owned_rows(parts, snaps)
    rings._guard(prm, pos, xbands, n_bins, what)
    dens = _density(profmod, prm, parts, pos, mass)
    delta = dens[0] / prm.rho0 - 1.0
    everyone = np.ones(nf, dtype=bool)
    want = _sums(profmod, prm, pos, mass, dens, everyone, n_bins, xbands, **hist, delta_bound=delta_bound)
    loose = sc.loose_per_band(profmod, prm, pos, delta, xbands, sc.EDGE_ONE_SAMPLE, **hist, delta_bound=delta_bound)
    sc.assert_loose_under_cap(loose, [b["count"].sum() + b["outliers"].sum() for b in want], what)
    # per slab: the reference's densities over the rows that slab owns, the quantisation term of that slab's own scales
    quant = None
    for r, (sums, s) in enumerate(zip(per_rank, snaps)):
        mine = rank == r
        want_r = _sums(profmod, prm, pos, mass, dens, mine, n_bins, xbands, **hist, delta_bound=delta_bound)
        q_r = dc.quantisation(want_r, profmod.dens_scales(delta_bound, len(s["id"])))  # (the count the slab holds)
        quant = q_r if quant is None else dc.add_quantisation(quant, q_r)
        if not rebinned:  # (a re-binning in the last step hands particles over behind the sample: the snapshot shows the new owners)
            loose_r = sc.loose_per_band(profmod, prm, pos[mine], delta[mine], xbands, sc.EDGE_ONE_SAMPLE, **hist, delta_bound=delta_bound)
            sc.assert_bands_match(sums, want_r, q_r, loose_r, f"{what} rank {r}", sc.BOUND_ONE_SAMPLE)
            y = s["y"][s["owned"]]
            assert sums[0]["count"].sum() + sums[0]["outliers"].sum() == int(np.count_nonzero((y >= 0.0) & (y <= prm.DH))), r
    sc.assert_bands_match(got, want, quant, loose, f"{what} pooled", sc.BOUND_ONE_SAMPLE)  # (band 2: the seam, by the folded definition)
    dev = dc.deviation(got, want)
    print(f"{what}: pooled sums off by {dev[0]:.3e} ({dev[1]}, band {dev[2]}), bound {sc.BOUND_ONE_SAMPLE:.2e} plus quantum; particles on an "
          f"edge per band {loose}; rebinned in the last step: {rebinned}")
    assert got[0]["count"].sum() + got[0]["outliers"].sum() == nf and got[1]["count"].sum() > 0 and got[2]["count"].sum() > 0
    return got, per_rank


@pytest.mark.parametrize("name, setting", [("a", {}), ("a", sc.HIST_WIDE), ("b", sc.HIST_WIDE), ("e", sc.HIST_WIDE)])
def test_one_sample_is_numpys_over_what_the_ring_holds(cfgmod, geom, capi, profmod, slab, name, setting):
    """(b: leftward flow, x < 0, three slabs; e: several workgroups per slab)"""
    got, _ = _one_sample(cfgmod, geom, capi, profmod, slab, name, **setting)
    assert got[0]["outliers"].sum() == 0
    if setting:
        assert got[0]["below"] == got[0]["above"] == 0 and np.count_nonzero(got[0]["hist"]) > 3


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_count_plus_outliers_is_the_flow_statistics_count(cfgmod, geom, slab, name):
    """per slab, bin and band, every step; delta_bound = 0.04 makes some particles outliers"""
    prm, parts = rings._case(cfgmod, geom, name)
    steps = rings._steps(name)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.flow_stats_enable(every=1, bands=dc.bands(prm))
            e.dens_part_enable(every=1, hist_range=0.02, delta_bound=0.04, bands=dc.bands(prm))
        rings._run(slab, engines, name)
        dens = _per_rank(engines)
        stats = [[e.flow_stats_sums(b) for b in range(3)] for e in engines]
    for r, (g, f) in enumerate(zip(dens, stats)):
        for b in range(3):
            assert g[b]["n_samples"] == f[b]["n_samples"] == steps
            assert np.array_equal(g[b]["count"] + g[b]["outliers"], f[b]["count"]), (name, r, b)
            assert g[b]["hist"].sum() + g[b]["below"] + g[b]["above"] == g[b]["count"].sum(), (name, r, b)
    assert sum(g[0]["count"].sum() for g in dens) > 0 and sum(g[0]["outliers"].sum() for g in dens) > 0


# 3 ---------------------------------------------------------------------------------------------------------------
_refs = {}


def _reference(cfgmod, geom, capi, profmod, name, setting):
    """The single context of case `name`'s state stepped one step at a time with the sampler on: its sums, the quantisation
    terms of its samples, per band the particles of every step's state within EDGE_EVERY_STEP of an edge, and the guard."""
    c = CASES[name]
    steps = rings._steps(name)
    key = (c["dp"], c["DL"], c.get("seed", 11), bool(c.get("leftward")), steps, tuple(sorted(setting.items())))  # (cases a and c: one state)
    if key not in _refs:
        prm, parts = rings._case(cfgmod, geom, name)
        nf, xbands = parts["n_fluid"], dc.bands(prm)
        n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
        scales = profmod.dens_scales(setting.get("delta_bound", 0.5), nf)
        quant, trouble, loose = None, None, [0, 0, 0]
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.dens_stats_enable(every=1, bands=xbands, **setting)
            for k in range(steps):
                ctx.advance(1e9, max_steps=1)
                pos = ctx.download(fields=("pos",))["pos"]
                dens = dc.density(profmod, prm, parts, pos)
                one = dc.numpy_sums(profmod, prm, parts, pos, n_bins, xbands, dens, **setting)
                q = dc.quantisation(one, scales)
                quant = q if quant is None else dc.add_quantisation(quant, q)
                near = sc.loose_per_band(profmod, prm, pos[:nf], dens[0] / prm.rho0 - 1.0, xbands, sc.EDGE_EVERY_STEP, **setting)
                loose = [a + b for a, b in zip(loose, near)]
                if trouble is None:
                    try:
                        rings._guard(prm, pos[:nf], xbands, n_bins, f"{name} step {k + 1}")
                    except AssertionError as e:
                        trouble = str(e)
            sums = [ctx.dens_stats_sums(b) for b in range(3)]
        _refs[key] = dict(sums=sums, quant=quant, trouble=trouble, loose=loose)
    return _refs[key]


def _every_step(cfgmod, geom, capi, profmod, slab, name, setting):
    prm, parts = rings._case(cfgmod, geom, name)
    steps = rings._steps(name)
    ref = _reference(cfgmod, geom, capi, profmod, name, setting)
    with rings._ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.dens_part_enable(every=1, bands=dc.bands(prm), **setting)
        rings._run(slab, engines, name)
        per_rank = _per_rank(engines)
        got = slab.ring_dens_stats_sums(engines)
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
    what = f"{name} {setting}: ring against context"
    sc.assert_loose_under_cap(ref["loose"], [b["count"].sum() + b["outliers"].sum() for b in want], what)
    quant = dc.add_quantisation(ref["quant"], ref["quant"])
    sc.assert_bands_match(got, want, quant, ref["loose"], what, sc.BOUND_EVERY_STEP)
    dev = dc.deviation(got, want)
    print(f"{what} over {steps} steps off by {dev[0]:.3e} ({dev[1]}, band {dev[2]}), bound {sc.BOUND_EVERY_STEP:.2e} plus quantum; particles on "
          f"an edge per band {ref['loose']} of {[int(c) for c in _counts(want)]}")
    return got, want


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_sums_of_every_step_match_a_single_context(cfgmod, geom, capi, profmod, slab, name):
    """The runs cross the scheduled re-binning (a, c), include leftward flow with x < 0 (b) and the two-stream form (c); the
    histogram is compared too, within `loose`.  The quantisation term is the context's samples' plus as much again for the
    slabs': a slab holds fewer particles than the channel, so its quantum is no coarser than the context's."""
    got, _ = _every_step(cfgmod, geom, capi, profmod, slab, name, sc.HIST_WIDE)
    assert got[0]["outliers"].sum() == 0 and np.count_nonzero(got[0]["hist"]) > 3


def test_a_narrow_delta_bound_counts_outliers_as_a_context_does(cfgmod, geom, capi, profmod, slab):
    """delta_bound = 0.04 lies inside the state's range of delta: e = -4 is every rank's, and a particle is an outlier on the
    ring where it is one on the context (but for those within the edge clearance of +-0.04: `loose`)."""
    got, want = _every_step(cfgmod, geom, capi, profmod, slab, "a", dict(n_hist=8, hist_range=0.04, delta_bound=0.04))
    assert got[0]["outliers"].sum() > 100 and got[0]["count"].sum() > 100 and (got[0]["below"], got[0]["above"]) == (0, 0)
    assert abs(got[0]["outliers"].sum() - want[0]["outliers"].sum()) <= _reference(cfgmod, geom, capi, profmod, "a", dict(
        n_hist=8, hist_range=0.04, delta_bound=0.04))["loose"][0]
    assert np.all(got[0]["d_max"][got[0]["count"] > 0] <= 0.04) and np.all(got[0]["d_min"][got[0]["count"] > 0] >= -0.04)


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 4])
def test_lattice_at_rest(cfgmod, geom, profmod, slab, world):
    """The lattice of dp = 0.05, DL = 3 (23 cell columns: slabs of 5 or 6 at world = 4).  A slab has no "sample now", so the
    sample is taken behind ONE step that leaves the lattice where it is: a step of 1e-9 (a dt^2 is 1e-18, far below an ulp of
    any coordinate) with transport_coeff = 0 -- the transport shift is the one displacement of a step that does not scale with
    dt (next to a wall it moves the lattice's rows by some 1e-9 in y, 1e-7 in delta).  LATTICE_DELTA depends on dp and h alone.
    Every owned particle's delta is LATTICE_DELTA -- next to the cuts, across the seam and in the wall rows alike: the walls
    continue the lattice, in the halo columns too."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.0, developed=False, end_time=1e9, transport_coeff=0.0)
    nf = parts["n_fluid"]
    assert nf == 1200
    engines = []
    try:
        engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, native=True) for r in range(world)]
        for e in engines:
            e.dens_part_enable(n_bins=20, every=1, bands=dc.bands(prm))
        slab.HipSlabEngine.group_run(engines, 1, t_target=1e-9)
        sts = [e.sync() for e in engines]
        snaps = [e.snapshot() for e in engines]
        per_rank = _per_rank(engines)
        got = slab.ring_dens_stats_sums(engines)
    finally:
        for e in engines:
            e.close()
    assert sts[0]["step"] == 1 and sts[0]["t"] <= 1e-9
    pos, _, _ = _owned_rows(parts, snaps)
    for k in (0, 1):  # the lattice, unmoved
        assert np.max(np.abs(np.sort(pos[:, k]) - np.sort(parts["pos"][:nf, k]))) <= 1e-15, k
    for r, sums in enumerate(per_rank):
        s = sums[0]
        some = s["count"] > 0
        assert some.all() and s["n_samples"] == 1 and np.all(s["outliers"] == 0), r
        assert np.all(np.abs(s["d_min"] - dc.LATTICE_DELTA) <= 1e-13) and np.all(np.abs(s["d_max"] - dc.LATTICE_DELTA) <= 1e-13), r
        assert s["hist"][31] == s["count"].sum() == s["hist"].sum() and (s["below"], s["above"]) == (0, 0), r
    s = got[0]
    assert np.all(s["count"] == nf / 20) and np.all(s["outliers"] == 0)
    assert np.all(np.abs(s["d_min"] - dc.LATTICE_DELTA) <= 1e-13) and np.all(np.abs(s["d_max"] - dc.LATTICE_DELTA) <= 1e-13)
    assert s["hist"][31] == nf and s["hist"].sum() == nf
    quantum = world * 2.0 ** -(profmod.dens_scales(0.5, nf)["s_wall"] + 1)  # (the coarsest scale; a slab holds fewer than nf)
    assert np.all(np.abs(s["sum_d"] / s["count"] - dc.LATTICE_DELTA) <= 1e-13 + quantum)
    # the seam band is the mid-channel band, field for field: two columns of 20 particles each, every delta the lattice's
    mid, seam = got[1], got[2]
    assert np.all(mid["count"] == 2) and np.array_equal(mid["count"], seam["count"]) and np.array_equal(mid["outliers"], seam["outliers"])
    assert np.array_equal(mid["hist"], seam["hist"]) and (mid["below"], mid["above"]) == (seam["below"], seam["above"]) == (0, 0)
    for f in dc.SUMMED + dc.EXTREMES:
        assert np.all(np.abs(mid[f] - seam[f]) <= mid["count"] * (1e-13 + quantum)), f
    assert np.count_nonzero(seam["sum_wall"]) == np.count_nonzero(s["sum_wall"]) > 0


# 5 ---------------------------------------------------------------------------------------------------------------
def test_the_lds_limit_on_a_ring(cfgmod, geom, capi, profmod, slab):
    """311 bins in three bands beside 64 histogram bins: 7662 of the 7680 words, 61 296 B of dynamic LDS for k_dens_stats_s.
    Integers against numpy over the owned rows of the snapshots; every 4th step of four is sampled."""
    prm, parts = rings._case(cfgmod, geom, "a")
    xbands, n_bins = dc.bands(prm), dc.BINS[-1]
    assert 3 * (8 * n_bins + 64 + 2) <= profmod.DENS_MAX_WORDS < 3 * (8 * (n_bins + 1) + 64 + 2)
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.dens_part_enable(n_bins=n_bins, every=4, bands=xbands, **sc.HIST_WIDE)
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.sync()
        snaps = [e.snapshot() for e in engines]
        got = slab.ring_dens_stats_sums(engines)
        with pytest.raises(capi.SphxError) as ei:  # one bin more does not fit
            engines[0].dens_part_enable(n_bins=n_bins + 1, every=4, bands=xbands, **sc.HIST_WIDE)
        assert ei.value.identifier == "SPHX:DensStats:config"
        assert engines[0].dens_part_sums(0)["n_samples"] == 1
    pos, mass, _ = _owned_rows(parts, snaps)
    rings._guard(prm, pos, xbands, n_bins, "the LDS limit")
    dens = _density(profmod, prm, parts, pos, mass)
    want = _sums(profmod, prm, pos, mass, dens, np.ones(len(pos), dtype=bool), n_bins, xbands, **sc.HIST_WIDE)
    loose = sc.loose_per_band(profmod, prm, pos, dens[0] / prm.rho0 - 1.0, xbands, sc.EDGE_ONE_SAMPLE, **sc.HIST_WIDE)
    sc.assert_loose_under_cap(loose, _counts(want), "the LDS limit")
    quant = dc.quantisation(want, profmod.dens_scales(0.5, max(len(s["id"]) for s in snaps)))  # (the coarsest slab's quantum for all)
    sc.assert_bands_match(got, want, quant, loose, "the LDS limit", sc.BOUND_ONE_SAMPLE)
    for b in range(3):
        assert got[b]["count"].shape == (n_bins,) and got[b]["n_samples"] == 1
    assert got[0]["count"].sum() == parts["n_fluid"] and np.count_nonzero(got[0]["count"]) > 50


# 6 ---------------------------------------------------------------------------------------------------------------
def test_gating_samples_the_steps_a_context_samples(cfgmod, geom, capi, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    steps = rings._steps("a")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.dens_stats_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        want = ctx.dens_stats_sums(0)
    assert want["n_samples"] == 3  # steps 15, 20, 25
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.dens_part_enable(every=5, t_from=t_from)
        rings._run(slab, engines, "a")
        got = [e.dens_part_sums(0) for e in engines]
    for g in got:
        assert g["n_samples"] == want["n_samples"]
        assert abs(g["t_first"] - want["t_first"]) <= 1e-12 * want["t_first"] and abs(g["t_last"] - want["t_last"]) <= 1e-12 * want["t_last"]
        assert pc.same_bits(g["t_first"], got[0]["t_first"]) and pc.same_bits(g["t_last"], got[0]["t_last"])
    assert sum(g["count"].sum() + g["outliers"].sum() for g in got) == want["count"].sum() + want["outliers"].sum() > 0


# 7 ---------------------------------------------------------------------------------------------------------------
def _others_on(prm, parts, e):
    """the other eight samplers, every step"""
    e.flow_stats_enable(every=1, bands=stats_bands(prm))
    e.history_enable(every=1)
    e.field_part_enable(nx=24, ny=9, every=1, with_walls=True)
    pts = np.array([[0.25 * prm.DL, 0.5 * prm.DH], [0.5 * prm.DL, 0.1 * prm.DH], [0.0, 0.5 * prm.DH], [0.9 * prm.DL, 0.8 * prm.DH]])
    e.probes_part_enable(pts, every=1, with_walls=True)
    e.profile_series_enable(every=1, bands=stats_bands(prm))
    e.pairs_part_enable(every=1, with_walls=True, bands=pc.bands(prm))
    e.grads_part_enable(every=1, with_walls=True, bands=stats_bands(prm))
    e.tracers_part_enable(np.arange(0, parts["n_fluid"], 7, dtype=np.int32), every=1, capacity=64)


def _others_read(e):
    return _blob([[e.flow_stats_sums(b) for b in range(3)], e.history_records()[0], e.field_part_sums(), e.probes_part_records(),
                  e.profile_series_sums(), e.pairs_part_sums(), [e.grads_part_sums(b) for b in range(3)], e.tracers_part_records()])


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_the_ring_and_the_other_samplers_do_not_feel_it(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form; the other
    eight samplers are on in both runs."""
    prm, parts = rings._case(cfgmod, geom, name)
    steps = rings._steps(name)
    runs = []
    for on in (False, True):
        with rings._ring(slab, prm, parts, name) as engines:
            for e in engines:
                _others_on(prm, parts, e)
                if on:
                    e.dens_part_enable(every=1, bands=dc.bands(prm), **sc.HIST_WIDE)
            rings._run(slab, engines, name)
            runs.append(dict(bits=rings._state_bits([e.snapshot() for e in engines]), others=[_others_read(e) for e in engines]))
            if on:
                assert all(e.dens_part_sums(0)["n_samples"] == steps and e.dens_part_sums(0)["count"].sum() > 0 for e in engines)
    off, on = runs
    assert off["bits"] == on["bits"]
    for r in range(len(off["others"])):
        assert off["others"][r] == on["others"][r], r


def test_replayed_graph_eager_form_and_a_second_run_give_the_same_bytes(cfgmod, geom, slab):
    """Case d: replays of the step graph, the same calls without graph_prepare, and those once more: every rank's bytes."""
    prm, parts = rings._case(cfgmod, geom, "d")
    steps = rings._steps("d")
    runs = []
    for calls in (None, CASES["d"]["calls"], CASES["d"]["calls"]):  # (explicit calls: no graph)
        with rings._ring(slab, prm, parts, "d") as engines:
            for e in engines:
                e.dens_part_enable(every=1, bands=dc.bands(prm), **sc.HIST_WIDE)
            rings._run(slab, engines, "d", calls=calls)
            runs.append(_per_rank(engines))
    assert all(p[0]["n_samples"] == steps and p[0]["count"].sum() > 0 and np.any(p[0]["sum_d"] != 0.0) for p in runs[0])
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
                e.dens_part_enable(every=1, bands=dc.bands(prm))
            slab.HipSlabEngine.group_run(engines, 25)
            for e in engines:
                e.sync()
            runs.append(_per_rank(engines))
    assert all(p[0]["n_samples"] == 25 for p in runs[0])
    assert _bits(runs[0]) == _bits(runs[1])


# 8 ---------------------------------------------------------------------------------------------------------------
def _empty(d):
    return (d["n_samples"] == 0 and all(not np.any(d[f]) for f in dc.COUNTS + dc.SUMMED) and np.all(d["d_min"] == np.inf)
            and np.all(d["d_max"] == -np.inf) and not np.any(d["hist"]) and (d["below"], d["above"]) == (0, 0)
            and np.isnan(d["t_first"]) and np.isnan(d["t_last"]))


def test_reset_and_disable_run_enable_start_from_zero(cfgmod, geom, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    with rings._ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.dens_part_enable(every=1, bands=dc.bands(prm))
        slab.HipSlabEngine.group_run(engines, 5)
        first = slab.ring_dens_stats_sums(engines)  # (no sync: the read waits for the slab's streams itself)
        slab.HipSlabEngine.group_run(engines, 2)
        for e in engines:  # (no sync: the samples of everything enqueued land before the sums are cleared)
            e.dens_part_reset()
        cleared = _per_rank(engines)
        slab.HipSlabEngine.group_run(engines, 2)
        resumed = slab.ring_dens_stats_sums(engines)
        for e in engines:  # (no sync in between: disable waits too)
            e.dens_part_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.dens_part_enable(every=1, n_bins=7, n_hist=16)
        before = _per_rank(engines, 1)
        slab.HipSlabEngine.group_run(engines, 3)
        after = slab.ring_dens_stats_sums(engines)
        sts = [e.sync() for e in engines]
    nf = parts["n_fluid"]
    assert sts[0]["step"] == 16
    assert first[0]["n_samples"] == 5 and first[0]["count"].sum() + first[0]["outliers"].sum() == 5 * nf
    assert all(_empty(d) for p in cleared for d in p) and all(len(p) == 3 for p in cleared)
    assert resumed[0]["n_samples"] == 2 and resumed[0]["count"].sum() + resumed[0]["outliers"].sum() == 2 * nf
    assert resumed[0]["t_first"] > first[0]["t_last"]
    assert all(_empty(p[0]) and p[0]["count"].shape == (7,) and p[0]["hist"].shape == (16,) for p in before)
    assert len(after) == 1 and after[0]["n_samples"] == 3 and after[0]["count"].sum() + after[0]["outliers"].sum() == 3 * nf
    assert after[0]["t_last"] == sts[0]["t"]


# 9 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    L = capi.lib()
    nothing = (None,) * 9

    def config(**kw):
        return capi.SphxDensStatsConfig(**dict(dict(n_bins=0, every=1, t_from=0.0, n_hist=64, n_bands=0, hist_range=0.05, delta_bound=0.5), **kw))

    cfg = config()

    def calls(h):
        return [(L.sphx_slab_dstats_enable, h, C.byref(cfg)), (L.sphx_slab_dstats_disable, h), (L.sphx_slab_dstats_reset, h),
                (L.sphx_slab_dstats_read, h, 0, 0, 0, *nothing)]

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
        for fn, args in ((L.sphx_slab_dstats_read, (0, 0, 0, *nothing)), (L.sphx_slab_dstats_reset, ())):
            assert err_id(capi, fn, h, *args) == ("SPHX:DensStats:disabled", capi.SPHX_ERR_STATE)
        for call in (e.dens_part_sums, e.dens_part_reset):
            with pytest.raises(capi.SphxError) as ei:
                call()
            assert ei.value.identifier == "SPHX:DensStats:disabled"
        assert L.sphx_slab_dstats_disable(h) == capi.SPHX_OK  # (off already)
        e.dens_part_disable()
        for x in engines:
            x.dens_part_enable(every=1, bands=dc.bands(prm))
        slab.HipSlabEngine.group_run(engines, 5)
        before = _per_rank([e])
        assert before[0][0]["n_samples"] == 5
        # a bad config: the identifiers of section 2r, from the library and from the binding's own checks; the sums stay
        nan = float("nan")
        for bad in (dict(n_bins=-1), dict(n_bins=952), dict(every=0), dict(t_from=nan), dict(n_hist=0), dict(n_hist=1025), dict(hist_range=0.0),
                    dict(hist_range=0.6), dict(delta_bound=0.0), dict(delta_bound=0.6), dict(delta_bound=nan), dict(n_bands=3)):
            c2 = config(**bad)
            assert err_id(capi, L.sphx_slab_dstats_enable, h, C.byref(c2)) == ("SPHX:DensStats:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_slab_dstats_enable, h, None) == ("SPHX:DensStats:config", capi.SPHX_ERR_ARG)
        for kw in (dict(delta_bound=0.6), dict(every=0), dict(n_bins=952), dict(bands=[(0.1, 0.1)] * 3)):
            with pytest.raises(capi.SphxError) as ei:
                e.dens_part_enable(**kw)
            assert ei.value.identifier == "SPHX:DensStats:config"
        dc.assert_identical(_per_rank([e])[0], before[0], "a refused enable leaves the sums as they were")
        slab.HipSlabEngine.group_run(engines, 2)
        assert e.dens_part_sums(0)["n_samples"] == 7  # ... and the sampler running
        for band in (-1, 3):
            assert err_id(capi, L.sphx_slab_dstats_read, h, band, 0, 0, *nothing) == ("SPHX:DensStats:band", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError) as ei:
            e.dens_part_sums(3)
        assert ei.value.identifier == "SPHX:DensStats:band"
        n_bins = len(before[0][0]["count"])
        sums = np.full((len(dc.FIELDS), n_bins), -7.0)
        hist = np.full(64, -7, dtype=np.int64)
        hist_p = hist.ctypes.data_as(C.POINTER(C.c_int64))
        assert err_id(capi, L.sphx_slab_dstats_read, h, 0, n_bins - 1, 0, None, None, capi.ptr(sums), *nothing[3:]) == ("SPHX:DensStats:capacity", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_slab_dstats_read, h, 0, 0, 63, None, None, None, hist_p, *nothing[4:]) == ("SPHX:DensStats:capacity", capi.SPHX_ERR_ARG)
        assert np.all(sums == -7.0) and np.all(hist == -7)
        nb, nh, ns = C.c_int(0), C.c_int(0), C.c_int64(0)
        assert L.sphx_slab_dstats_read(h, 2, 0, 0, C.byref(nb), C.byref(nh), None, None, None, None, C.byref(ns), None, None) == capi.SPHX_OK  # no array: no capacity
        assert (nb.value, nh.value, ns.value) == (n_bins, 64, 7)
        # the context's calls keep refusing a slab, and say where to go
        for fn, args in ((L.sphx_ctx_dens_stats_enable, (C.byref(cfg),)), (L.sphx_ctx_dens_stats_disable, ()), (L.sphx_ctx_dens_stats_reset, ()),
                         (L.sphx_ctx_dens_stats_sample, ()), (L.sphx_ctx_dens_stats_read, (0, 0, 0, *nothing))):
            assert err_id(capi, fn, h, *args) == ("SPHX:DensStats:slab", capi.SPHX_ERR_ARG)
            assert "sphx_slab_dstats_" in L.sphx_last_error().decode()
        for x in engines:
            x.sync()
        assert e.dens_part_sums(0)["n_samples"] == 7
