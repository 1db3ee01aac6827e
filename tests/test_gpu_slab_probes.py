"""-m gpu: point probes of a slab ring (include/sphx.h section 3a; k_point_probes_s), on in-process rings
(sphx_slab_group_run) on device 0.  The ring's points are divided among the slabs; a slab records the complete sample of every
probe it owns -- weight, u_x, u_y and the summation density rho -- from its owned particles and its halo copies, and the
ring's series is the slabs' columns put back in the list's order.  Checked against profile.shepard_points (numpy) of the owned
particles of the snapshots with the masses of their ids (one sample), against a single context of the same state recording
every step, for the owners partitioning the points, for leaving the ring's state and the other three samplers bit for bit as
they are -- in the chain, the two-stream and the replayed-graph form of the step -- for captured against eager runs, for
gating, drain and capacity, and for the error identifiers.

Bounds.  One sample against numpy: probe_cases.BOUND = 1e-12 of the largest |value| of a column, the bound and argument of
tests/test_gpu_probes.py (a probe sums up to about 150 non-negative weights, each product rounded to 1.1e-16, then divides
once; the worst value measured there was 1.4e-14).  rho = sum m_j W_j is the first sampled value that depends on the MASS of a
halo copy: a stale or wrongly shifted copy, or a copy without its mass, is off by 1e-3 or more at a probe within 2h of a cut;
those probes are asserted (and printed) separately.  Every step against a context: the ring's state agrees with the context's to
1e-9 per particle, and the fields are allowed 1e-8 of a record's largest |value|, RING_BOUND of
tests/test_gpu_slab_field_map.py.

The cases a, b, c, d and f are those of tests/test_gpu_slab_field_map.py (copied, not imported).  HipSlabEngine passes skin_h and
rebuild_every through, so test 8 runs one sample on a ring with a skin of 2 h, where a column run of three cells holds more
than a wave's 64 candidates and a lane takes a second one -- from halo columns too."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from helpers import HISTORY_FIELDS, STATS_FIELDS, err_id, make_case, make_variant, stats_bands
from probe_cases import BOUND, FIELDS, assert_series_identical, assert_values_match, random_points

pytestmark = pytest.mark.gpu

CASES = {
    "a": dict(world=2, dp=0.05, DL=3.0, calls=[27]),                            # crosses the scheduled re-binning at K = 24
    "b": dict(world=3, dp=0.05, DL=4.5, calls=[23], leftward=True, kw=dict(rebuild_every=4)),  # ownership migrates left, x < 0
    "c": dict(world=2, dp=0.05, DL=3.0, calls=[5, 18, 1, 1, 2], overlap="always"),  # the two-stream form of the step
    "d": dict(world=2, dp=0.05, DL=3.0, calls=[3, 25, 19], graph_after=0),      # replays of the step graph carry the sampler
    "f": dict(world=4, dp=0.05, DL=4.5, calls=[26]),                            # four slabs: two of them have no periodic seam
    # test 8: cells 4 h = 5.2 dp wide hold ~27 particles, a column run of three ~80; uneven mass, moving walls
    "wide": dict(world=2, dp=0.05, DL=6.0, calls=[7], variant=True, kw=dict(rebuild_every=16, skin_h=2.0)),
}
PLANES = ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")
RING_BOUND = 1e-8    # every step against a single context


@pytest.fixture(scope="module")
def slab(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".slab")


_made = {}


def _case(cfgmod, geom, name):
    if name not in _made:
        c = CASES[name]
        common = dict(dp=c["dp"], DL=c["DL"], jitter=0.2, seed=c.get("seed", 11), developed=True, end_time=1e9)
        if c.get("leftward"):
            prm, parts = make_variant(cfgmod, geom, U_bulk=-0.666667, top_ux=-0.8, bottom_ux=0.3, rho0=2.5, transport_coeff=0.1,
                                      **common)
            assert prm.gravity_g < 0
        elif c.get("variant"):
            prm, parts = make_variant(cfgmod, geom, **common)
        else:
            prm, parts = make_case(cfgmod, geom, **common)
        _made[name] = (prm, parts)
    return _made[name]


@contextlib.contextmanager
def _ring(slab, prm, parts, name, world=None):
    """The engines of case `name`'s ring; SPHX_SLAB_OVERLAP is read when a slab's buffers are made (the first group_run)."""
    c = CASES[name]
    world = world or c["world"]
    env_before = os.environ.pop("SPHX_SLAB_OVERLAP", None)
    if c.get("overlap"):
        os.environ["SPHX_SLAB_OVERLAP"] = c["overlap"]
    engines = []
    try:
        engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, native=True, **c.get("kw", {})) for r in range(world)]
        yield engines
    finally:
        for e in engines:
            e.close()
        os.environ.pop("SPHX_SLAB_OVERLAP", None)
        if env_before is not None:
            os.environ["SPHX_SLAB_OVERLAP"] = env_before


def _run(slab, engines, name, calls=None):
    c = CASES[name]
    for k, n in enumerate(c["calls"] if calls is None else calls):
        slab.HipSlabEngine.group_run(engines, n)
        if calls is None and c.get("graph_after") == k:
            slab.HipSlabEngine.graph_prepare(engines)
    return [e.sync() for e in engines]


def _steps(name):
    return sum(CASES[name]["calls"])


def _owned_state(snaps, prm, parts):
    """The owned particles of the ring's snapshots as one channel: pos (x mod DL), vel, and the mass of each one's id."""
    own = [s["owned"] for s in snaps]
    cat = lambda k: np.concatenate([s[k][o] for s, o in zip(snaps, own)])
    pos = np.column_stack([np.mod(cat("x"), prm.DL), cat("y")])
    vel = np.column_stack([cat("vx"), cat("vy")])
    ids = cat("id")
    assert len(ids) == parts["n_fluid"] and len(np.unique(ids)) == len(ids)
    return pos, vel, parts["mass"][ids]


# ---- the ring's cell grid and the point sets ----
def _grid(prm, parts, engines):
    """(layouts, cuts, csx, cell size in y, y of row 0): cut r = col0 of rank r times the column width, the library's arithmetic"""
    layouts = [e.layout() for e in engines]
    ncx = layouts[-1]["col1"]                  # the ring's cell columns
    csx = prm.DL / ncx
    skin = C.c_double(0.0)
    engines[0].capi.check(engines[0].capi.lib().sphx_ctx_grid_policy(engines[0]._h, None, C.byref(skin), None, None))
    return layouts, [lay["col0"] * csx for lay in layouts], csx, 2.0 * prm.h + skin.value, float(np.min(parts["pos"][:, 1]))


def _cut_points(prm, parts, grid):
    """The set `cuts` and what the tests need to know of it: points [P, 2]; near [P] (within 2h of a cut, the seam included);
    on_cut [(index, rank)]: points exactly on cut `rank`; dup (i, j): a duplicate pair; mid [indices]: mid-channel points on a cut."""
    _, cuts, csx, cs, y_min = grid
    DL, DH, h = prm.DL, prm.DH, prm.h
    nf = parts["n_fluid"]
    pts, on_cut, mid = [], [], []
    rows = [j for j in range(1, 64) if 0.1 * DH < y_min + j * cs < 0.9 * DH]
    for r, c in enumerate(cuts):
        y = (0.35 + 0.1 * (r % 4)) * DH
        on_cut.append((len(pts), r))
        mid.append(len(pts))
        pts += [(c + off, y) for off in (0.0, 1e-12, -1e-12, h, -h, 1.9 * h, -1.9 * h)]
        on_cut += [(len(pts), r), (len(pts) + 1, r), (len(pts) + 2, r)]
        pts += [(c, 0.0), (c, DH), (c, y_min + rows[r % len(rows)] * cs)]   # both wall lines and a cell corner, on the cut
    pts += [(0.0, 0.5 * DH), (DL - 5e-13, 0.31 * DH), (DL, 0.62 * DH), (-DL, 0.27 * DH)]   # (DL and -DL fold to 0)
    inside = np.flatnonzero((parts["pos"][:nf, 1] > 0.1 * DH) & (parts["pos"][:nf, 1] < 0.9 * DH))
    pts.append(tuple(parts["pos"][inside[17]]))                         # a particle's own (initial) position
    dup = (len(pts), len(pts) + 1)
    pts += [(cuts[-1] + 0.5 * h, 0.44 * DH)] * 2                        # one duplicate pair
    pts = np.concatenate([np.array(pts, dtype=np.float64), random_points(prm, 40, 21)])
    x = np.mod(pts[:, 0], DL)
    d = np.min([np.minimum(np.abs(x - c), DL - np.abs(x - c)) for c in cuts], axis=0)
    return dict(points=pts, near=d <= 2.0 * h, on_cut=on_cut, dup=dup, mid=mid)


def _point_sets(prm, parts, grid):
    """name -> points: P = 1, 16 (a workgroup's waves), 17 and 300 (19 workgroups and more over the ring), the last with `cuts`
    in front"""
    cuts = _cut_points(prm, parts, grid)["points"]
    return {"1": random_points(prm, 1, 1), "16": random_points(prm, 16, 3), "17": np.concatenate([cuts[:4], random_points(prm, 13, 4)]),
            "300": np.concatenate([cuts, random_points(prm, 300 - len(cuts), 5)]), "cuts": cuts}


def _numpy(profmod, prm, parts, snaps, pts, walls):
    pos, vel, mass = _owned_state(snaps, prm, parts)
    nf = parts["n_fluid"]
    kw = dict(wall_pos=parts["pos"][nf:], wall_vel=parts["wall_vel"][nf:]) if walls else {}
    return profmod.shepard_points(pos, vel, mass, prm.DL, prm.h, prm.dp, pts, **kw)


def _check_partition(per_rank, P):
    seen = np.zeros(P, dtype=int)
    for p in per_rank:
        idx = p["index"]
        assert np.all(np.diff(idx) > 0) and (len(idx) == 0 or (idx[0] >= 0 and idx[-1] < P))
        assert all(p[k].shape == (len(p["step"]), len(idx)) for k in FIELDS)
        seen[idx] += 1
    assert np.all(seen == 1), seen   # disjoint, and their union is range(P)


# 1 ---------------------------------------------------------------------------------------------------------------
ONE_SAMPLE = {                      # case, with_walls, point set
    "a": ("a", False, "300"),
    "b": ("b", False, "300"),
    "f": ("f", False, "300"),
    "b_walls": ("b", True, "300"),   # (case b's walls move)
    "b_2x2": ("b", False, "2x2"),    # the middle slab owns nothing
}


@pytest.mark.parametrize("variant", list(ONE_SAMPLE))
def test_one_sample_is_numpys_shepard_points_of_the_owned_particles(cfgmod, geom, capi, profmod, slab, variant):
    name, walls, which = ONE_SAMPLE[variant]
    prm, parts = _case(cfgmod, geom, name)
    steps = _steps(name)
    with _ring(slab, prm, parts, name) as engines:
        grid = _grid(prm, parts, engines)
        cuts = _cut_points(prm, parts, grid)
        if which == "2x2":
            pts = np.array([(0.0, 0.0), (0.0, prm.DH), (prm.DL - 5e-13, 0.0), (prm.DL - 5e-13, prm.DH)])
        else:
            pts = _point_sets(prm, parts, grid)[which]
        for e in engines:
            e.probes_part_enable(pts, every=steps, with_walls=walls)  # only the last step is recorded
        sts = _run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        per_rank = [e.probes_part_records() for e in engines]
        got = slab.ring_probes(engines)
        extra = []
        if variant == "a":   # the small sets, one more step each: one probe, a full workgroup, one wave more
            for label in ("1", "16", "17"):
                small = _point_sets(prm, parts, grid)[label]
                for e in engines:
                    e.probes_part_enable(small, every=1, with_walls=True)
                slab.HipSlabEngine.group_run(engines, 1)
                extra.append((label, small, slab.ring_probes(engines), [e.snapshot() for e in engines]))
    for p in per_rank:   # every slab, one without a probe too, has the one record with the step's {step, t}
        assert p["step"].tolist() == [steps] and p["t"].tolist() == [sts[0]["t"]] and p["n_dropped"] == 0
    _check_partition(per_rank, len(pts))
    assert got["step"].tolist() == [steps] and got["u_x"].shape == (1, len(pts))
    want = _numpy(profmod, prm, parts, snaps, pts, walls)
    assert np.array_equal(got["points"], want["points"])
    assert_values_match(got, want, variant, row=0)
    if which == "2x2":
        assert [p["index"].tolist() for p in per_rank] == [[0, 1], [], [2, 3]]
        assert per_rank[1]["u_x"].shape == (1, 0)
        return
    near = np.flatnonzero(cuts["near"])   # `cuts` is in front of the set
    assert len(near) >= 9 * CASES[name]["world"]
    scale = {k: max(float(np.nanmax(np.abs(want[k]))), 1e-300) for k in FIELDS}
    off = {k: float(np.max(np.abs(got[k][0][near] - want[k][near]))) / scale[k] for k in FIELDS}
    print(f"{variant}: at the {len(near)} probes within 2h of a cut, off by (of the column's largest |value|) "
          + ", ".join(f"{k} {v:.3e}" for k, v in off.items()))
    for k in FIELDS:
        assert off[k] <= BOUND, f"{variant}: {k} off by {off[k]:.3e} within 2h of a cut"
    # a sanity line, not a tolerance: a slab that dropped its halo would read about half of rho0 on a cut
    assert np.all(got["rho"][0][cuts["mid"]] > 0.9 * prm.rho0), got["rho"][0][cuts["mid"]] / prm.rho0
    for label, small, g, sn in extra:
        assert g["step"].tolist() == [steps + 1 + ("1", "16", "17").index(label)] and g["u_x"].shape == (1, len(small))
        assert_values_match(g, _numpy(profmod, prm, parts, sn, small, True), f"a, P={label}", row=0)


# 2 ---------------------------------------------------------------------------------------------------------------
_every_step = {}


def _both(cfgmod, geom, capi, slab, name):
    """Case `name` with the probes recording every step: the ring's parts and pooled series, and a single context's."""
    if name not in _every_step:
        prm, parts = _case(cfgmod, geom, name)
        with _ring(slab, prm, parts, name) as engines:
            pts = _point_sets(prm, parts, _grid(prm, parts, engines))["300"]
            for e in engines:  # (before the first call: the replays of case d carry the sampler)
                e.probes_part_enable(pts, every=1, with_walls=True)
            _run(slab, engines, name)
            ring = dict(parts=[e.probes_part_records() for e in engines], pooled=slab.ring_probes(engines))
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.probes_enable(pts, every=1, with_walls=True)
            ctx.advance(1e9, max_steps=_steps(name))
            ref = ctx.probes()
        _every_step[name] = (ring, ref)
    return _every_step[name]


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f"])
def test_series_of_every_step_match_a_single_context(cfgmod, geom, capi, driver, slab, name):
    ring, want = _both(cfgmod, geom, capi, slab, name)
    prm, _ = _case(cfgmod, geom, name)
    got = ring["pooled"]
    steps = _steps(name)
    assert np.array_equal(got["points"], want["points"]) and got["n_dropped"] == want["n_dropped"] == 0
    assert got["step"].tolist() == want["step"].tolist() == list(range(1, steps + 1))
    assert np.all(np.abs(got["t"] - want["t"]) <= 1e-12 * want["t"])
    worst = dict.fromkeys(FIELDS, 0.0)
    for r in range(steps):
        for k in FIELDS:
            assert not np.any(np.isnan(got[k][r])) and not np.any(np.isnan(want[k][r])), (r, k)   # no void probe here
            worst[k] = max(worst[k], float(np.max(np.abs(got[k][r] - want[k][r]))) / max(float(np.max(np.abs(want[k][r]))), 1e-300))
    print(f"{name}: ring against context over {steps} records, off by (of a record's largest |value|) "
          + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in FIELDS:
        assert worst[k] <= RING_BOUND, f"{name}: {k} off by {worst[k]:.3e}"
    fr, fc = driver.probe_figures(prm, got), driver.probe_figures(prm, want)   # the pooled dict goes straight in
    assert fr["n_records"] == fc["n_records"] == steps and np.all(np.isfinite(fr["u_x_mean"]))


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 4])
def test_owners_partition_the_points(cfgmod, geom, slab, world):
    prm, parts = _case(cfgmod, geom, "f")
    with _ring(slab, prm, parts, "f", world=world) as engines:
        grid = _grid(prm, parts, engines)
        cuts = _cut_points(prm, parts, grid)
        for label, pts in _point_sets(prm, parts, grid).items():
            for e in engines:
                e.probes_part_enable(pts, every=1)
            slab.HipSlabEngine.group_run(engines, 2)
            per_rank = [e.probes_part_records() for e in engines]  # (no sync: the read waits)
            _check_partition(per_rank, len(pts))
            for p in per_rank:
                assert p["step"].tolist() == per_rank[0]["step"].tolist() and len(p["step"]) == 2
                assert len(p["points"]) == len(pts)
            pooled = slab.pool_ring_probes(per_rank)
            assert pooled["u_x"].shape == (2, len(pts)) and not np.any(np.isnan(pooled["u_x"]))
            if label in ("300", "cuts"):   # (`cuts` is in front of "300")
                owner = np.empty(len(pts), dtype=int)
                for r, p in enumerate(per_rank):
                    owner[p["index"]] = r
                for i, r in cuts["on_cut"]:  # a point on cut r is rank r's, never rank r - 1's
                    assert owner[i] == r, (label, i, r, owner[i], pts[i])
                i, j = cuts["dup"]
                assert np.array_equal(pts[i], pts[j]) and owner[i] == owner[j]
                for k in FIELDS:
                    assert pooled[k][:, i].tobytes() == pooled[k][:, j].tobytes(), k
        for e in engines:
            e.sync()


# 4 ---------------------------------------------------------------------------------------------------------------
def _state_bits(snaps):
    return [tuple(s[k].tobytes() for k in ("x", "y", "vx", "vy", "drho", "id", "owned")) for s in snaps]


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_probes_leave_the_ring_and_the_other_samplers_bit_for_bit(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form."""
    prm, parts = _case(cfgmod, geom, name)
    bits, sums, records, planes = [], [], [], []
    for others, probes in ((False, False), (False, True), (True, False), (True, True)):
        with _ring(slab, prm, parts, name) as engines:
            pts = _point_sets(prm, parts, _grid(prm, parts, engines))["300"]
            for e in engines:
                if others:
                    e.flow_stats_enable(every=1, bands=stats_bands(prm))
                    e.history_enable(every=1)
                    e.field_part_enable(every=1)
                if probes:
                    e.probes_part_enable(pts, every=1, with_walls=True)
            _run(slab, engines, name)
            bits.append(_state_bits([e.snapshot() for e in engines]))
            if others:
                sums.append([[e.flow_stats_sums(b) for b in range(3)] for e in engines])
                records.append([e.history_records() for e in engines])
                planes.append([e.field_part_sums() for e in engines])
            if probes:
                assert all(len(e.probes_part_records()["step"]) == _steps(name) for e in engines)
    assert bits[0] == bits[1] == bits[2] == bits[3]
    for without, with_probes in zip(sums[0], sums[1]):  # per rank
        for b in range(3):
            for k in STATS_FIELDS + ("n_samples", "t_first", "t_last"):
                assert np.array_equal(without[b][k], with_probes[b][k]), (b, k)
    for (rec, dropped), (rec_p, dropped_p) in zip(records[0], records[1]):
        assert rec.shape[1] == len(HISTORY_FIELDS) and np.array_equal(rec, rec_p) and dropped == dropped_p
    for without, with_probes in zip(planes[0], planes[1]):
        for k in PLANES + ("i_lo", "i_hi", "n_samples", "t_first", "t_last"):
            assert np.array_equal(without[k], with_probes[k]), k


# 5 ---------------------------------------------------------------------------------------------------------------
def test_captured_and_eager_forms_give_the_same_bits(cfgmod, geom, capi, slab):
    """Case d (replays of the step graph) against the same calls without graph_prepare: every slab's series bit for bit."""
    ring, _ = _both(cfgmod, geom, capi, slab, "d")
    prm, parts = _case(cfgmod, geom, "d")
    with _ring(slab, prm, parts, "d") as engines:
        pts = _point_sets(prm, parts, _grid(prm, parts, engines))["300"]
        for e in engines:
            e.probes_part_enable(pts, every=1, with_walls=True)
        _run(slab, engines, "d", calls=CASES["d"]["calls"])  # (explicit calls: no graph)
        eager = [e.probes_part_records() for e in engines]
    for r, (got, want) in enumerate(zip(eager, ring["parts"])):
        assert np.array_equal(got["index"], want["index"]) and len(got["step"]) == _steps("d")
        assert_series_identical(got, want, f"slab {r}: eager against replayed")


# 6 ---------------------------------------------------------------------------------------------------------------
def test_gating_records_the_steps_a_context_records(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    steps = _steps("a")
    pts = random_points(prm, 17, 6)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.probes_enable(pts, every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        want = ctx.probes()
    assert want["step"].tolist() == [15, 20, 25]
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.probes_part_enable(pts, every=5, t_from=t_from)
        _run(slab, engines, "a")
        per_rank = [e.probes_part_records() for e in engines]
        got = slab.pool_ring_probes(per_rank)
    for p in per_rank:
        assert p["step"].tolist() == [15, 20, 25]
    assert got["step"].tolist() == want["step"].tolist() and np.all(np.abs(got["t"] - want["t"]) <= 1e-12 * want["t"])
    for r in range(3):
        assert_values_match(got, {k: want[k][r] for k in FIELDS}, f"gated: record {r}", row=r, bound=RING_BOUND)


def test_full_buffer_drops_and_drain_resumes_from_row_zero(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    pts = random_points(prm, 40, 7)
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.probes_part_enable(pts, every=1, capacity=4)
        _run(slab, engines, "a")                        # 27 steps
        full = [e.probes_part_records() for e in engines]
        again = [e.probes_part_records() for e in engines]          # reading without drain changes nothing
        drained = [e.probes_part_records(drain=True) for e in engines]
        empty = [e.probes_part_records() for e in engines]
        slab.HipSlabEngine.group_run(engines, 2)
        resumed = [e.probes_part_records() for e in engines]
        for e in engines:
            e.sync()
    for r in range(len(full)):
        assert full[r]["step"].tolist() == [1, 2, 3, 4] and full[r]["n_dropped"] == 23, r
        assert_series_identical(full[r], again[r], "read twice")
        assert_series_identical(full[r], drained[r], "read with drain")
        assert len(empty[r]["step"]) == 0 and empty[r]["n_dropped"] == 0 and empty[r]["u_x"].shape == (0, len(full[r]["index"]))
        assert resumed[r]["step"].tolist() == [28, 29] and resumed[r]["n_dropped"] == 0
    assert slab.pool_ring_probes(resumed)["u_x"].shape == (2, 40)


def test_disable_run_enable_starts_from_zero(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    pts = random_points(prm, 17, 8)
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.probes_part_enable(pts, every=1)
        slab.HipSlabEngine.group_run(engines, 5)
        for e in engines:  # (no sync in between: disable waits for the slab's streams itself)
            e.probes_part_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.probes_part_enable(pts[:3], every=1)
        slab.HipSlabEngine.group_run(engines, 3)
        got = slab.ring_probes(engines)  # (no sync either: the read waits)
        sts = [e.sync() for e in engines]
    assert sts[0]["step"] == 12
    assert got["step"].tolist() == [10, 11, 12] and got["u_x"].shape == (3, 3) and got["n_dropped"] == 0


# 7 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    L = capi.lib()
    good = np.array([[0.5, 0.5], [2.9, 0.25]])
    nothing = (None,) * 8  # times, values, index, the four counts ...

    def config(points=good, **kw):
        pts = None if points is None else np.ascontiguousarray(points, dtype=np.float64)
        c = capi.SphxProbesConfig(n_points=0 if pts is None else len(pts), every=1, capacity=16, with_walls=0, t_from=0.0,
                                  points=capi.ptr(pts))
        for k, v in kw.items():
            setattr(c, k, v)
        return c, pts

    def read(h, cap=0, arrays=nothing):
        return (L.sphx_slab_probes_read, h, cap, *arrays, 0)  # ... and drain

    cfg, keep = config()

    def calls(h):
        return [(L.sphx_slab_probes_enable, h, C.byref(cfg)), (L.sphx_slab_probes_disable, h), read(h)]

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
    with _ring(slab, prm, parts, "a") as engines:
        e = engines[0]
        h = e._h
        assert err_id(capi, *read(h)) == ("SPHX:Probe:disabled", capi.SPHX_ERR_STATE)
        with pytest.raises(capi.SphxError) as ei:
            e.probes_part_records()
        assert ei.value.identifier == "SPHX:Probe:disabled"
        assert L.sphx_slab_probes_disable(h) == capi.SPHX_OK  # (off already)
        # a bad config: the identifiers of section 2h, from the library and from the binding's own checks
        nan, inf = float("nan"), float("inf")
        refused = [dict(points=None, n_points=2), dict(n_points=0), dict(n_points=4097), dict(every=0), dict(t_from=nan),
                   dict(points=[[nan, 0.5]]), dict(points=[[inf, 0.5]]), dict(points=[[0.5, -1e-9]]),
                   dict(points=[[0.5, prm.DH * (1 + 1e-12)]]), dict(capacity=0), dict(capacity=(1 << 24) + 1), dict(with_walls=2)]
        for bad in refused:
            c2, keep2 = config(**bad)
            assert err_id(capi, L.sphx_slab_probes_enable, h, C.byref(c2)) == ("SPHX:Probe:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_slab_probes_enable, h, None) == ("SPHX:Probe:config", capi.SPHX_ERR_ARG)
        for kw in (dict(points=np.zeros((0, 2))), dict(points=np.zeros((4097, 2))), dict(every=0), dict(t_from=nan),
                   dict(points=[[inf, 0.5]]), dict(points=[[0.5, 1.5 * prm.DH]]), dict(capacity=0)):
            with pytest.raises(capi.SphxError) as ei:
                e.probes_part_enable(**dict(dict(points=good), **kw))
            assert ei.value.identifier == "SPHX:Probe:config", kw
        for x in engines:
            x.probes_part_enable(good, every=1, capacity=16)
        slab.HipSlabEngine.group_run(engines, 3)
        before = e.probes_part_records()
        assert before["step"].tolist() == [1, 2, 3] and before["index"].tolist() == [0]   # (2.9 is the other slab's)
        times, values = np.zeros((3, 2)), np.zeros((3, 1, 4))
        assert err_id(capi, *read(h, 2, (capi.ptr(times),) + (None,) * 7)) == ("SPHX:Probe:capacity", capi.SPHX_ERR_ARG)
        assert err_id(capi, *read(h, -1, (None, capi.ptr(values)) + (None,) * 6)) == ("SPHX:Probe:capacity", capi.SPHX_ERR_ARG)
        assert np.all(times == 0) and np.all(values == 0)
        ring_n, own, n = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.sphx_slab_probes_read(h, 0, capi.ptr(times), capi.ptr(values), None, C.byref(ring_n), C.byref(own), C.byref(n),
                                       None, 1) == capi.SPHX_OK   # capacity = 0: the sizes only, nothing copied or drained
        assert (ring_n.value, own.value, n.value) == (2, 1, 3) and np.all(times == 0) and np.all(values == 0)
        # a refused enable leaves the running probes, and their records, as they are
        c2, keep2 = config(every=0)
        assert err_id(capi, L.sphx_slab_probes_enable, h, C.byref(c2)) == ("SPHX:Probe:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError):
            e.probes_part_enable(good, every=0)
        assert_series_identical(e.probes_part_records(), before, "a refused enable leaves the records as they were")
        # the context's calls keep refusing a slab
        for fn, args in ((L.sphx_ctx_probes_enable, (C.byref(cfg),)), (L.sphx_ctx_probes_disable, ()), (L.sphx_ctx_probes_sample, ()),
                         (L.sphx_ctx_probes_read, (0, None, None, None, None, None, 0))):
            assert err_id(capi, fn, h, *args) == ("SPHX:Probe:slab", capi.SPHX_ERR_ARG)
        slab.HipSlabEngine.group_run(engines, 2)
        for x in engines:
            x.sync()
        assert e.probes_part_records()["step"].tolist() == [1, 2, 3, 4, 5]   # ... and the sampler running


# 8 ---------------------------------------------------------------------------------------------------------------
def test_a_column_run_longer_than_a_wave_on_a_ring(cfgmod, geom, capi, profmod, slab):
    """A skin of 2 h: a column's run of three cells holds about 80 particles, so a lane takes a second candidate (the k += 64
    loop) -- at the probes on and beside a cut from a halo column."""
    name = "wide"
    prm, parts = _case(cfgmod, geom, name)
    nf, steps = parts["n_fluid"], _steps(name)
    with _ring(slab, prm, parts, name) as engines:
        grid = _grid(prm, parts, engines)
        layouts, cut_x, csx, cs, y_min = grid
        cuts = _cut_points(prm, parts, grid)
        pts = cuts["points"]
        # the longest run of three cells in the columns around a probe on a cut, by the initial positions: one of the three
        # columns is a halo column of the owner
        ncx = layouts[-1]["col1"]
        cx = np.minimum((parts["pos"][:nf, 0] / csx).astype(int), ncx - 1)
        cy = ((parts["pos"][:nf, 1] - y_min) / cs).astype(int)
        longest = 0
        for i in cuts["mid"]:
            px, py = int(round(pts[i, 0] / csx)), int((pts[i, 1] - y_min) / cs)
            longest = max([longest] + [int(np.count_nonzero((cx == c % ncx) & (np.abs(cy - py) <= 1))) for c in (px - 1, px)])
        assert longest > 64, longest
        for e in engines:
            e.probes_part_enable(pts, every=steps, with_walls=True)
        _run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        got = slab.ring_probes(engines)
    want = _numpy(profmod, prm, parts, snaps, pts, True)
    assert_values_match(got, want, "wide skin", row=0)
    near = np.flatnonzero(cuts["near"])
    for k in FIELDS:
        scale = max(float(np.nanmax(np.abs(want[k]))), 1e-300)
        assert float(np.max(np.abs(got[k][0][near] - want[k][near]))) <= BOUND * scale, k
