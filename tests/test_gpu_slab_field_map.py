"""-m gpu: velocity-field maps of a slab ring (include/sphx.h section 3a; k_field_map_s), on in-process rings
(sphx_slab_group_run) on device 0.  A slab samples the node columns it owns, every node completely, from its owned particles
and its halo copies; the ring's map is the slabs' blocks side by side.  Checked against profile.shepard_field (numpy) of the
owned particles of the snapshots (one sample), against a single context of the same state sampling every step, for the
blocks partitioning the node columns, for leaving the ring's state and the other two samplers bit for bit as they are -- in
the chain, the two-stream and the replayed-graph form of the step -- for the gating and for the error identifiers.

Bounds.  One sample against numpy: a node sums up to about 150 non-negative weights, each product rounded to 1.1e-16, then
divides once -- about 1e-13 of the largest |value| of a plane; 1e-12 is allowed, as in tests/test_gpu_field_map.py.  A halo
copy one step stale would be off by dt |v| / h ~ 1e-3 of a kernel radius and miss that by many orders of magnitude at the
node columns next to a cut, which are asserted (and printed) separately.  Every step against a context: the ring's state
agrees with the context's to 1e-9 per particle, the kernel weight is continuous at 2h, and the sums over 27 steps are allowed
1e-8 of the plane's largest |sum|, the bound of tests/test_gpu_slab_samplers.py.

The cases a - d are those of tests/test_gpu_slab_samplers.py (copied, not imported); f is a ring of four slabs small enough for
numpy's all-pairs Shepard sums."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from helpers import HISTORY_FIELDS, STATS_FIELDS, err_id, make_case, make_variant, stats_bands

pytestmark = pytest.mark.gpu

CASES = {
    "a": dict(world=2, dp=0.05, DL=3.0, calls=[27]),                            # crosses the scheduled re-binning at K = 24
    "b": dict(world=3, dp=0.05, DL=4.5, calls=[23], leftward=True, kw=dict(rebuild_every=4)),  # ownership migrates left, x < 0
    "c": dict(world=2, dp=0.05, DL=3.0, calls=[5, 18, 1, 1, 2], overlap="always"),  # the two-stream form of the step
    "d": dict(world=2, dp=0.05, DL=3.0, calls=[3, 25, 19], graph_after=0),      # replays of the step graph carry the sampler
    "f": dict(world=4, dp=0.05, DL=4.5, calls=[26]),                            # four slabs: two of them have no periodic seam
}
PLANES = ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")
BOUND = 1e-12        # one sample against numpy
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


def _owned_state(snaps, prm):
    """The owned particles of the ring's snapshots as one channel: pos (x mod DL), vel."""
    own = [s["owned"] for s in snaps]
    x = np.concatenate([s["x"][o] for s, o in zip(snaps, own)])
    pos = np.column_stack([np.mod(x, prm.DL), np.concatenate([s["y"][o] for s, o in zip(snaps, own)])])
    vel = np.column_stack([np.concatenate([s[k][o] for s, o in zip(snaps, own)]) for k in ("vx", "vy")])
    return pos, vel


def _numpy_planes(prm, f):  # (tests/test_gpu_field_map.py)
    hit = f["S0"] > 0.0
    z = lambda v: np.where(hit, v, 0.0)
    return dict(count=hit.astype(np.float64), sum_w=z(f["S0"] * prm.dp ** 2), sum_ux=z(f["u_x"]), sum_uy=z(f["u_y"]),
                sum_ux2=z(f["u_x"] ** 2), sum_uy2=z(f["u_y"] ** 2))


def _columns_at_cuts(prm, layouts, nx):
    """The node columns within one cell column of a cut between two slabs (the periodic seam is one), and columns 0 and nx - 1."""
    ncx = layouts[-1]["col1"]                 # the ring's cell columns
    csx = prm.DL / ncx
    x = np.linspace(0.0, prm.DL, nx)
    near = np.zeros(nx, dtype=bool)
    for cut in [lay["col0"] * csx for lay in layouts] + [prm.DL]:
        near |= np.abs(x - cut) <= csx
    near[0] = near[nx - 1] = True
    return near


def _deviation(got, want, cols=None):
    """per plane: max |got - want| by the largest |want| of the WHOLE plane, over all node columns or the chosen ones"""
    out = {}
    for k in PLANES[1:]:
        scale = max(float(np.max(np.abs(want[k]))), 1e-300)
        d = np.abs(got[k] - want[k])
        out[k] = float(np.max(d if cols is None else d[:, cols], initial=0.0)) / scale
    return out


def _assert_within(got, want, bound, what, near):
    assert np.array_equal(got["count"], want["count"]), what + ": count"
    everywhere, at_cuts = _deviation(got, want), _deviation(got, want, near)
    print(f"{what}: off by (of the plane's largest |value|) " + ", ".join(f"{k} {v:.3e}" for k, v in everywhere.items())
          + f"; at the {int(near.sum())} node columns next to a cut or an end: " + ", ".join(f"{k} {v:.3e}" for k, v in at_cuts.items()))
    for k in PLANES[1:]:
        assert at_cuts[k] <= bound, f"{what}: {k} off by {at_cuts[k]:.3e} next to a cut"
        assert everywhere[k] <= bound, f"{what}: {k} off by {everywhere[k]:.3e}"


# 1 ---------------------------------------------------------------------------------------------------------------
ONE_SAMPLE = {                       # case, nx, ny, with_walls
    "a": ("a", 0, 0, False),
    "b": ("b", 0, 0, False),
    "f": ("f", 0, 0, False),
    "b_walls": ("b", 0, 0, True),    # (case b's walls move)
    "a_on_cuts": ("a", "ncx+1", 0, False),   # every node column on a cell-column boundary
    "b_2x2": ("b", 2, 2, False),     # the middle slab owns no node
}


@pytest.mark.parametrize("variant", list(ONE_SAMPLE))
def test_one_sample_is_numpys_shepard_field_of_the_owned_particles(cfgmod, geom, capi, profmod, slab, variant):
    name, nx, ny, walls = ONE_SAMPLE[variant]
    prm, parts = _case(cfgmod, geom, name)
    nf, steps = parts["n_fluid"], _steps(name)
    if nx == "ncx+1":
        nx = slab.n_cell_columns(prm) + 1
    with _ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.field_part_enable(nx=nx, ny=ny, every=steps, with_walls=walls)  # only the last step is sampled
        sts = _run(slab, engines, name)
        snaps = [e.snapshot() for e in engines]
        per_rank = [e.field_part_sums() for e in engines]
        layouts = [e.layout() for e in engines]
    pos, vel = _owned_state(snaps, prm)
    assert len(pos) == nf
    got = slab.pool_ring_field_map(per_rank)
    nx, ny = capi.field_map_shape(prm, nx, ny)
    assert got["count"].shape == (ny, nx)
    for p in per_rank:
        assert (p["nx"], p["ny"]) == (nx, ny) and p["n_samples"] == 1 and p["t_first"] == p["t_last"] == sts[0]["t"]
    kw = dict(wall_pos=parts["pos"][nf:], wall_vel=parts["wall_vel"][nf:]) if walls else {}
    f = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny, **kw)
    _assert_within(got, _numpy_planes(prm, f), BOUND, variant, _columns_at_cuts(prm, layouts, nx))
    assert np.all(got["count"] == 1)  # every node has a contributor
    if walls:
        fluid_only = profmod.shepard_field(pos, vel, prm.DL, prm.DH, prm.h, nx, ny)
        assert np.all(got["sum_w"][0] > 1.5 * fluid_only["S0"][0] * prm.dp ** 2)   # the wall rows did enter
    if variant == "b_2x2":
        assert [(p["i_lo"], p["i_hi"]) for p in per_rank] == [(0, 1), (1, 1), (1, 2)]
        assert per_rank[1]["count"].shape == (2, 0) and per_rank[1]["n_samples"] == 1  # no node, but the head counts


# 2 ---------------------------------------------------------------------------------------------------------------
_every_step = {}


def _both(cfgmod, geom, capi, slab, name):
    """Case `name` with the map sampled every step: the ring's pooled planes and map, and a single context's."""
    if name not in _every_step:
        prm, parts = _case(cfgmod, geom, name)
        with _ring(slab, prm, parts, name) as engines:
            for e in engines:  # (before the first call: the replays of case d carry the sampler)
                e.field_part_enable(every=1)
            _run(slab, engines, name)
            ring = dict(parts=[e.field_part_sums() for e in engines], map=slab.ring_field_map(engines),
                        layouts=[e.layout() for e in engines])
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.field_map_enable(every=1)
            ctx.advance(1e9, max_steps=_steps(name))
            ref = dict(sums=ctx.field_map_sums(), map=ctx.field_map())
        _every_step[name] = (ring, ref)
    return _every_step[name]


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f"])
def test_planes_of_every_step_match_a_single_context(cfgmod, geom, capi, driver, slab, name):
    ring, ref = _both(cfgmod, geom, capi, slab, name)
    prm, _ = _case(cfgmod, geom, name)
    got, want = slab.pool_ring_field_map(ring["parts"]), ref["sums"]
    steps = _steps(name)
    assert got["n_samples"] == want["n_samples"] == steps
    assert abs(got["t_first"] - want["t_first"]) <= 1e-12 * want["t_first"]
    assert abs(got["t_last"] - want["t_last"]) <= 1e-12 * want["t_last"]
    nx = want["count"].shape[1]
    _assert_within(got, want, RING_BOUND, f"{name}: ring against context", _columns_at_cuts(prm, ring["layouts"], nx))
    fr, fc = driver.field_figures(prm, ring["map"]), driver.field_figures(prm, ref["map"])
    print(f"{name}: x_spread ring {fr['x_spread']:.6f} % at ix {fr['ix']}, context {fc['x_spread']:.6f} % at ix {fc['ix']}")
    assert (fr["ix"], fr["iy"]) == (fc["ix"], fc["iy"])
    # (x_spread is a deviation of a mean u_x in % of |U_max|: the plane's bound, on sum_ux / n_samples)
    scale = 100.0 * float(np.max(np.abs(want["sum_ux"]))) / steps / abs(fc["U_max"])
    assert abs(fr["x_spread"] - fc["x_spread"]) <= 2.0 * RING_BOUND * scale


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 4])
def test_blocks_partition_the_node_columns(cfgmod, geom, capi, slab, world):
    prm, parts = _case(cfgmod, geom, "f")
    shapes = [(0, 0), (2, 2), (3, 5), (37, 9), (slab.n_cell_columns(prm) + 1, 4)]
    with _ring(slab, prm, parts, "f", world=world) as engines:
        for nx, ny in shapes:
            for e in engines:
                e.field_part_enable(nx=nx, ny=ny, every=1)
            slab.HipSlabEngine.group_run(engines, 2)
            per_rank = [e.field_part_sums() for e in engines]  # (no sync: the read waits)
            gx, gy = capi.field_map_shape(prm, nx, ny)
            at = 0
            for p in per_rank:
                assert (p["nx"], p["ny"]) == (gx, gy) and p["i_lo"] == at and p["i_hi"] >= at, (nx, ny, p["i_lo"], p["i_hi"])
                assert all(p[k].shape == (gy, p["i_hi"] - p["i_lo"]) for k in PLANES)
                assert p["n_samples"] == 2
                at = p["i_hi"]
            assert at == gx
            assert per_rank[-1]["i_hi"] - per_rank[-1]["i_lo"] >= 1  # node nx - 1 (x = DL) is the last slab's
            pooled = slab.pool_ring_field_map(per_rank)
            assert np.all(pooled["count"] == 2), (nx, ny)  # every node sampled by exactly one slab, every time
        for e in engines:
            e.sync()


# 4 ---------------------------------------------------------------------------------------------------------------
def _state_bits(snaps):
    return [tuple(s[k].tobytes() for k in ("x", "y", "vx", "vy", "drho", "id", "owned")) for s in snaps]


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_map_leaves_the_ring_and_the_other_samplers_bit_for_bit(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form."""
    prm, parts = _case(cfgmod, geom, name)
    bits, sums, records = [], [], []
    for others, fmap in ((False, False), (False, True), (True, False), (True, True)):
        with _ring(slab, prm, parts, name) as engines:
            for e in engines:
                if others:
                    e.flow_stats_enable(every=1, bands=stats_bands(prm))
                    e.history_enable(every=1)
                if fmap:
                    e.field_part_enable(every=1)
            _run(slab, engines, name)
            bits.append(_state_bits([e.snapshot() for e in engines]))
            if others:
                sums.append([[e.flow_stats_sums(b) for b in range(3)] for e in engines])
                records.append([e.history_records() for e in engines])
            if fmap:
                assert all(e.field_part_sums()["n_samples"] == _steps(name) for e in engines)
    assert bits[0] == bits[1] == bits[2] == bits[3]
    for without, with_map in zip(sums[0], sums[1]):  # per rank
        for b in range(3):
            for k in STATS_FIELDS + ("n_samples", "t_first", "t_last"):
                assert np.array_equal(without[b][k], with_map[b][k]), (b, k)
    for (rec, dropped), (rec_m, dropped_m) in zip(records[0], records[1]):
        assert rec.shape[1] == len(HISTORY_FIELDS) and np.array_equal(rec, rec_m) and dropped == dropped_m


# 5 ---------------------------------------------------------------------------------------------------------------
def test_captured_and_eager_forms_give_the_same_bits(cfgmod, geom, capi, slab):
    """Case d (replays of the step graph) against the same calls without graph_prepare: every plane bit for bit."""
    ring, _ = _both(cfgmod, geom, capi, slab, "d")
    prm, parts = _case(cfgmod, geom, "d")
    with _ring(slab, prm, parts, "d") as engines:
        for e in engines:
            e.field_part_enable(every=1)
        _run(slab, engines, "d", calls=CASES["d"]["calls"])  # (explicit calls: no graph)
        eager = [e.field_part_sums() for e in engines]
    for got, want in zip(eager, ring["parts"]):
        for k in PLANES + ("i_lo", "i_hi", "n_samples", "t_first", "t_last"):
            assert np.array_equal(got[k], want[k]), k


# 6 ---------------------------------------------------------------------------------------------------------------
def test_gating_samples_the_steps_a_context_samples(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    steps = _steps("a")
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.field_map_enable(every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        want = ctx.field_map_sums()
    assert want["n_samples"] == 3  # steps 15, 20, 25
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.field_part_enable(every=5, t_from=t_from)
        _run(slab, engines, "a")
        got = slab.pool_ring_field_map([e.field_part_sums() for e in engines])
        layouts = [e.layout() for e in engines]
    assert got["n_samples"] == want["n_samples"]
    assert abs(got["t_first"] - want["t_first"]) <= 1e-12 * want["t_first"] and abs(got["t_last"] - want["t_last"]) <= 1e-12 * want["t_last"]
    _assert_within(got, want, RING_BOUND, "gated", _columns_at_cuts(prm, layouts, want["count"].shape[1]))


def test_disable_run_enable_starts_from_zero_and_reset_empties(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.field_part_enable(every=1)
        slab.HipSlabEngine.group_run(engines, 5)
        for e in engines:  # (no sync in between: disable waits for the slab's streams itself)
            e.field_part_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.field_part_enable(every=1)
        slab.HipSlabEngine.group_run(engines, 3)
        first = slab.pool_ring_field_map([e.field_part_sums() for e in engines])  # (no sync either: the read waits)
        for e in engines:
            e.field_part_reset()
        empty = slab.pool_ring_field_map([e.field_part_sums() for e in engines])
        sts = [e.sync() for e in engines]
        slab.HipSlabEngine.group_run(engines, 2)
        again = slab.pool_ring_field_map([e.field_part_sums() for e in engines])
        for e in engines:
            e.sync()
    assert sts[0]["step"] == 12
    assert first["n_samples"] == 3 and np.all(first["count"] == 3)
    assert empty["n_samples"] == 0 and np.isnan(empty["t_first"]) and all(not empty[k].any() for k in PLANES)
    assert again["n_samples"] == 2 and np.all(again["count"] == 2) and again["t_first"] > sts[0]["t"]


# 7 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    L = capi.lib()
    cfg = capi.field_map_config()
    gx, gy, lo, hi = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    nothing = (None,) * 9  # six planes and the head

    def read(h, cap=0, planes=nothing):
        return (L.sphx_slab_field_map_read, h, cap, C.byref(gx), C.byref(gy), C.byref(lo), C.byref(hi), *planes)

    def calls(h):
        return [(L.sphx_slab_field_map_enable, h, C.byref(cfg)), (L.sphx_slab_field_map_disable, h), (L.sphx_slab_field_map_reset, h),
                read(h)]

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
        assert err_id(capi, *read(h)) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_slab_field_map_reset, h) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        for fn in (e.field_part_sums, e.field_part_reset):
            with pytest.raises(capi.SphxError) as ei:
                fn()
            assert ei.value.identifier == "SPHX:Field:disabled"
        assert L.sphx_slab_field_map_disable(h) == capi.SPHX_OK  # (off already)
        # a bad config: the identifiers of section 2e, from the library and from the binding's own checks
        for bad in (capi.SphxFieldMapConfig(nx=1, ny=0, every=1, with_walls=0, t_from=0.0),
                    capi.SphxFieldMapConfig(nx=0, ny=0, every=0, with_walls=0, t_from=0.0),
                    capi.SphxFieldMapConfig(nx=0, ny=0, every=1, with_walls=2, t_from=0.0),
                    capi.SphxFieldMapConfig(nx=1 << 13, ny=1 << 13, every=1, with_walls=0, t_from=0.0)):  # nx * ny > 1 << 25
            assert err_id(capi, L.sphx_slab_field_map_enable, h, C.byref(bad)) == ("SPHX:Field:config", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_slab_field_map_enable, h, None) == ("SPHX:Field:config", capi.SPHX_ERR_ARG)
        for kw in (dict(nx=1), dict(every=0), dict(t_from=float("nan")), dict(with_walls=2), dict(nx=1 << 13, ny=1 << 13)):
            with pytest.raises(capi.SphxError) as ei:
                e.field_part_enable(**kw)
            assert ei.value.identifier == "SPHX:Field:config"
        for x in engines:
            x.field_part_enable()
        slab.HipSlabEngine.group_run(engines, 3)
        small = np.zeros(4)
        planes = (capi.ptr(small),) + (None,) * 8
        assert err_id(capi, *read(h, 4, planes)) == ("SPHX:Field:capacity", capi.SPHX_ERR_ARG)
        assert err_id(capi, *read(h, -1, planes)) == ("SPHX:Field:capacity", capi.SPHX_ERR_ARG)
        # a refused enable leaves the running sampler as it is
        bad = capi.SphxFieldMapConfig(nx=1, ny=0, every=1, with_walls=0, t_from=0.0)
        assert err_id(capi, L.sphx_slab_field_map_enable, h, C.byref(bad)) == ("SPHX:Field:config", capi.SPHX_ERR_ARG)
        # the context's calls keep refusing a slab
        assert err_id(capi, L.sphx_ctx_field_map_enable, h, C.byref(cfg)) == ("SPHX:Field:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_field_map_disable, h) == ("SPHX:Field:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_field_map_reset, h) == ("SPHX:Field:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_field_map_sample, h) == ("SPHX:Field:slab", capi.SPHX_ERR_ARG)
        assert err_id(capi, L.sphx_ctx_field_map_read, h, 0, C.byref(gx), C.byref(gy), *nothing) == ("SPHX:Field:slab", capi.SPHX_ERR_ARG)
        for x in engines:
            x.sync()
        got = e.field_part_sums()
        assert got["n_samples"] == 3 and got["i_lo"] == 0 and np.all(got["count"] == 3)
