"""-m gpu: particle tracers of a slab ring (include/sphx.h section 3a; k_tracers_s), on in-process rings (sphx_slab_group_run)
on device 0.  Ownership moves with the particle: a slab copies the tracked particles it owns at the sampled step into dense
records, NaN where it was not the owner, and counts them (n_owned); the ring's series is every column from the one rank that
wrote it.  Checked against the ring's own snapshots step by step (records, owners, n_owned), for the run really migrating
across every cut, for subsets of the ids, against a single context of the same state, for leaving the ring's state and the other
seven samplers bit for bit as they are -- chain, two-stream and replayed form -- for captured against eager runs, for gating,
the buffer (drops, drain and the NaN refill, disable / enable), for stale slots behind a shrunken population, and for the error
identifiers.

Bounds.  Values compared with the ring's own snapshots use np.array_equal: k_tracers_s copies, there is no tolerance.  The one
exception is x of a particle that changed hands across the periodic seam in the very step of the record: the record holds x in
the old owner's frame, the snapshot behind the re-binning holds xn + shift (shift = +-DL, one rounding) in the new owner's, and
the comparison repeats that sum in float64.  Against a single context: the ring's state is a context's to 1e-9 per particle, and
every field is allowed RING_BOUND = 1e-8 of the record's largest |value| (the bound and argument of
tests/test_gpu_slab_field_map.py), x modulo DL by the nearest image.

The cases a, b, c, d, f and wide are those of tests/test_gpu_slab_probes.py (copied, not imported)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from helpers import err_id, make_case, make_variant, stats_bands
from tracer_cases import FIELDS, id_sets

pytestmark = pytest.mark.gpu

CASES = {
    "a": dict(world=2, dp=0.05, DL=3.0, calls=[27]),                            # crosses the scheduled re-binning at K = 24
    "b": dict(world=3, dp=0.05, DL=4.5, calls=[23], leftward=True, kw=dict(rebuild_every=4)),  # ownership migrates left, x < 0
    "c": dict(world=2, dp=0.05, DL=3.0, calls=[5, 18, 1, 1, 2], overlap="always"),  # the two-stream form of the step
    "d": dict(world=2, dp=0.05, DL=3.0, calls=[3, 25, 19], graph_after=0),      # replays of the step graph carry the sampler
    "f": dict(world=4, dp=0.05, DL=4.5, calls=[26]),                            # four slabs: two of them have no periodic seam
    "wide": dict(world=2, dp=0.05, DL=6.0, calls=[7], variant=True, kw=dict(rebuild_every=16, skin_h=2.0)),
}
# Steps taken one per call.  Ownership goes by the binned column, so it changes hands at re-binnings only, and only once a
# particle has drifted out of its owner's columns: on a and f (K = 24) the first re-binning that moves any comes at the end of
# step 28 and the next at 36 (measured: 10 and 12 ids on a, 22 and 22 on f), on b (K = 4) one id by step 13 and three more by
# step 21 -- dt is 1e-3 here, not the 2e-3 of a first estimate, so the runs are longer than 20 to 24 steps: two steps past the
# second of those re-binnings on a and f, K * 15 + 3 on b.
STEPWISE = {"a": 38, "b": 63, "f": 38}
RING_BOUND = 1e-8                        # every step against a single context
CAPACITY = 64


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


def _all_ids(parts):
    return id_sets(parts["n_fluid"])["all"]   # every row, shuffled


def _by_id(snaps, nf):
    """The owned particles of the ring's snapshots by id: owner [nf] and x, y, u_x, u_y [nf]; every row has exactly one owner."""
    out = dict(owner=np.full(nf, -1, dtype=np.int64), held=[len(s["id"]) for s in snaps], **{k: np.full(nf, np.nan) for k in FIELDS})
    for r, s in enumerate(snaps):
        o = s["owned"]
        i = s["id"][o]
        assert np.all(out["owner"][i] == -1) and len(np.unique(i)) == len(i), f"rows held twice: rank {r}"
        out["owner"][i] = r
        for k, src in zip(FIELDS, ("x", "y", "vx", "vy")):
            out[k][i] = s[src][o]
    assert np.all(out["owner"] >= 0), f"{int(np.count_nonzero(out['owner'] < 0))} rows lost"
    return out


def _assert_record_is_snapshot(prm, world, ids, pooled, per_rank, row, before, after, what):
    """Record `row` of the pooled series against the snapshots in front of and behind its step, by id."""
    T = len(ids)
    assert sum(int(p["n_owned"][row]) for p in per_rank) == T, f"{what}: n_owned {[int(p['n_owned'][row]) for p in per_rank]}"
    assert np.array_equal(pooled["owner"][row], before["owner"][ids]), f"{what}: the owner during a step is the binned column's"
    for k in ("y", "u_x", "u_y"):
        assert np.array_equal(pooled[k][row], after[k][ids]), f"{what}: {k}"
    x_rec, x_snap = pooled["x"][row], after["x"][ids]
    a, b = before["owner"][ids], after["owner"][ids]
    seam = (a != b) & (np.minimum(a, b) == 0) & (np.maximum(a, b) == world - 1)   # changed hands between rank 0 and the last
    shifted = (x_snap == x_rec + prm.DL) | (x_snap == x_rec - prm.DL)
    ok = (x_snap == x_rec) | (seam & shifted)
    assert np.all(ok), f"{what}: x differs for ids {ids[~ok][:8].tolist()} (owners {a[~ok][:8].tolist()} -> {b[~ok][:8].tolist()})"
    return int(np.count_nonzero(seam & shifted & (x_snap != x_rec)))


# 1, 2 ------------------------------------------------------------------------------------------------------------
_stepwise = {}


def _one_step_per_call(cfgmod, geom, slab, name, n_steps, capacity=CAPACITY):
    """Case `name` with every row tracked, one step per group_run call: the snapshots by id in front of the first call and behind
    each one, the ranks' parts and the pooled series."""
    key = (name, n_steps)
    if key not in _stepwise:
        prm, parts = _case(cfgmod, geom, name)
        nf = parts["n_fluid"]
        ids = _all_ids(parts)
        with _ring(slab, prm, parts, name) as engines:
            grid = [e.layout() for e in engines]
            for e in engines:
                e.tracers_part_enable(ids, every=1, capacity=capacity)
            snaps = [_by_id([e.snapshot() for e in engines], nf)]
            for _ in range(n_steps):
                slab.HipSlabEngine.group_run(engines, 1)
                snaps.append(_by_id([e.snapshot() for e in engines], nf))
            per_rank = [e.tracers_part_records() for e in engines]
            pooled = slab.ring_tracers(engines)
            for e in engines:
                e.sync()
        _stepwise[key] = dict(ids=ids, snaps=snaps, per_rank=per_rank, pooled=pooled, layouts=grid)
    return _stepwise[key]


@pytest.mark.parametrize("name", list(STEPWISE))
def test_records_are_the_snapshots(cfgmod, geom, slab, name):
    prm, parts = _case(cfgmod, geom, name)
    N, world = STEPWISE[name], CASES[name]["world"]
    run = _one_step_per_call(cfgmod, geom, slab, name, N)
    ids, pooled, per_rank, snaps = run["ids"], run["pooled"], run["per_rank"], run["snaps"]
    assert 1200 <= len(ids) <= 1800 and pooled["x"].shape == (N, len(ids)) and pooled["step"].tolist() == list(range(1, N + 1))
    assert pooled["n_dropped"] == 0 and pooled["n_missing"] == 0 and not any(np.isnan(pooled[k]).any() for k in FIELDS)
    for p in per_rank:
        assert p["step"].tolist() == pooled["step"].tolist() and p["n_owned"].dtype == np.int64
        for k in FIELDS:   # the four fields of a column are written together or not at all
            assert np.array_equal(np.isnan(p[k]), np.isnan(p["x"])), k
    across = sum(_assert_record_is_snapshot(prm, world, ids, pooled, per_rank, r, snaps[r], snaps[r + 1], f"{name}: record {r}")
                 for r in range(N))
    print(f"{name}: {N} records of {len(ids)} tracers equal the snapshots; {across} values met behind a shift across the seam")


@pytest.mark.parametrize("name", list(STEPWISE))
def test_the_run_really_migrates_across_every_cut(cfgmod, geom, slab, name):
    prm, parts = _case(cfgmod, geom, name)
    N, world = STEPWISE[name], CASES[name]["world"]
    run = _one_step_per_call(cfgmod, geom, slab, name, N)
    snaps, layouts = run["snaps"], run["layouts"]
    csx = prm.DL / layouts[-1]["col1"]
    cuts = np.array([lay["col0"] * csx for lay in layouts])   # cut r: the left edge of rank r (cut 0 is the seam, at 0 = DL)
    crossers = [set() for _ in cuts]
    for r in range(N):
        a, b = snaps[r]["owner"], snaps[r + 1]["owner"]
        for i in np.flatnonzero(a != b):
            x = np.mod(snaps[r]["x"][i], prm.DL)
            d = np.abs(x - cuts)
            crossers[int(np.argmin(np.minimum(d, prm.DL - d)))].add(int(i))
    counts = [len(c) for c in crossers]
    print(f"{name}: ids that change owner in {N} steps, per cut (cut 0 is the seam): {counts}")
    assert len(counts) == world and all(c >= 1 for c in counts), counts
    moved = np.flatnonzero(np.any(np.diff(run["pooled"]["owner"], axis=0) != 0, axis=0))
    assert len(moved) >= 1   # ... and the series shows it (the last step's change is behind the last record)


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["1", "63", "64", "65", "300", "all"])
def test_subsets_are_the_matching_columns_of_the_all_rows_run(cfgmod, geom, slab, which):
    name = "a"
    prm, parts = _case(cfgmod, geom, name)
    N = STEPWISE[name]
    ref = _one_step_per_call(cfgmod, geom, slab, name, N)
    ids = id_sets(parts["n_fluid"])[which]
    col = np.full(parts["n_fluid"], -1)
    col[ref["ids"]] = np.arange(len(ref["ids"]))
    with _ring(slab, prm, parts, name) as engines:
        for e in engines:
            e.tracers_part_enable(ids, every=1, capacity=CAPACITY)
        _run(slab, engines, name, calls=[N])
        per_rank = [e.tracers_part_records() for e in engines]
        got = slab.pool_ring_tracers(per_rank)
    assert np.array_equal(got["ids"], ids) and got["x"].shape == (N, len(ids)) and got["n_dropped"] == 0
    assert np.array_equal(got["step"], ref["pooled"]["step"]) and got["t"].tobytes() == ref["pooled"]["t"].tobytes()
    for k in FIELDS + ("owner",):
        assert got[k].tobytes() == np.ascontiguousarray(ref["pooled"][k][:, col[ids]]).tobytes(), (which, k)
    assert np.array_equal(sum(p["n_owned"] for p in per_rank), np.full(N, len(ids)))


# 4 ---------------------------------------------------------------------------------------------------------------
_every_step = {}


def _both(cfgmod, geom, capi, slab, name):
    """Case `name` with every row recorded at every step: the ring's parts and pooled series, and a single context's."""
    if name not in _every_step:
        prm, parts = _case(cfgmod, geom, name)
        ids = _all_ids(parts)
        with _ring(slab, prm, parts, name) as engines:
            for e in engines:  # (before the first call: the replays of case d carry the sampler)
                e.tracers_part_enable(ids, every=1, capacity=CAPACITY)
            _run(slab, engines, name)
            ring = dict(parts=[e.tracers_part_records() for e in engines], pooled=slab.ring_tracers(engines))
        with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
            ctx.tracers_enable(ids, every=1, capacity=CAPACITY)
            ctx.advance(1e9, max_steps=_steps(name))
            ref = ctx.tracers()
        _every_step[name] = (ring, ref)
    return _every_step[name]


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f"])
def test_series_of_every_step_match_a_single_context(cfgmod, geom, capi, driver, slab, name):
    ring, want = _both(cfgmod, geom, capi, slab, name)
    prm, _ = _case(cfgmod, geom, name)
    got, steps = ring["pooled"], _steps(name)
    assert np.array_equal(got["ids"], want["ids"]) and got["n_dropped"] == want["n_dropped"] == 0 and want["n_missing"] == 0
    assert got["step"].tolist() == want["step"].tolist() == list(range(1, steps + 1))
    assert np.all(np.abs(got["t"] - want["t"]) <= 1e-12 * want["t"])
    worst = dict.fromkeys(FIELDS, 0.0)
    for r in range(steps):
        for k in FIELDS:
            d = got[k][r] - want[k][r]
            if k == "x":
                d = d - np.round(d / prm.DL) * prm.DL   # the nearest image
            worst[k] = max(worst[k], float(np.max(np.abs(d))) / max(float(np.max(np.abs(want[k][r]))), 1e-300))
    print(f"{name}: ring against context over {steps} records of {len(got['ids'])} tracers, off by (of a record's largest |value|) "
          + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in FIELDS:
        assert worst[k] <= RING_BOUND, f"{name}: {k} off by {worst[k]:.3e}"
    fr, fc = driver.tracer_figures(prm, got), driver.tracer_figures(prm, want)   # the pooled dict goes straight in
    assert fr["n_records"] == fc["n_records"] == steps and fr["n_tracers"] == fc["n_tracers"]


# 5 ---------------------------------------------------------------------------------------------------------------
def _bits(v):
    """anything a sampler's read returns, as something == compares bit for bit"""
    if isinstance(v, dict):
        return {k: _bits(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_bits(x) for x in v]
    a = np.asarray(v)
    return (a.dtype.str, a.shape, a.tobytes())


def _state_bits(snaps):
    return [tuple(s[k].tobytes() for k in ("x", "y", "vx", "vy", "drho", "id", "owned")) for s in snaps]


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_tracers_leave_the_ring_and_the_other_samplers_bit_for_bit(cfgmod, geom, slab, name):
    """Chain, two-stream (where a misplaced launch would race with phase 3 or the next pass A) and replayed-graph form."""
    prm, parts = _case(cfgmod, geom, name)
    ids = id_sets(parts["n_fluid"])["300"]
    pts = np.column_stack([np.linspace(0.0, prm.DL, 23, endpoint=False), np.linspace(0.1, 0.9, 23) * prm.DH])
    bits, others_out = [], []
    for others, tracers in ((False, False), (False, True), (True, False), (True, True)):
        with _ring(slab, prm, parts, name) as engines:
            for e in engines:
                if others:
                    e.flow_stats_enable(every=1, bands=stats_bands(prm))
                    e.history_enable(every=1)
                    e.field_part_enable(every=1)
                    e.probes_part_enable(pts, every=1, with_walls=True)
                    e.profile_series_enable(every=1, capacity=CAPACITY)
                    e.pairs_part_enable(every=1)
                    e.grads_part_enable(every=1)
                if tracers:
                    e.tracers_part_enable(ids, every=1, capacity=CAPACITY)
            _run(slab, engines, name)
            bits.append(_state_bits([e.snapshot() for e in engines]))
            if others:
                others_out.append(_bits([[[e.flow_stats_sums(b) for b in range(3)], e.history_records(), e.field_part_sums(),
                                          e.probes_part_records(), e.profile_series_sums(), e.pairs_part_sums(), e.grads_part_sums()]
                                         for e in engines]))
            if tracers:
                got = slab.ring_tracers(engines)
                assert got["step"].tolist() == list(range(1, _steps(name) + 1)) and got["n_dropped"] == 0
    assert bits[0] == bits[1] == bits[2] == bits[3]
    assert others_out[0] == others_out[1]


def test_captured_and_eager_forms_give_the_same_bytes(cfgmod, geom, capi, slab):
    """Case d (replays of the step graph) against the same calls without graph_prepare: every slab's series byte for byte."""
    ring, _ = _both(cfgmod, geom, capi, slab, "d")
    prm, parts = _case(cfgmod, geom, "d")
    with _ring(slab, prm, parts, "d") as engines:
        for e in engines:
            e.tracers_part_enable(_all_ids(parts), every=1, capacity=CAPACITY)
        _run(slab, engines, "d", calls=CASES["d"]["calls"])  # (explicit calls: no graph)
        eager = [e.tracers_part_records() for e in engines]
    for r, (got, want) in enumerate(zip(eager, ring["parts"])):
        assert len(got["step"]) == _steps("d")
        assert _bits(got) == _bits(want), f"slab {r}: eager against replayed"


# 6 ---------------------------------------------------------------------------------------------------------------
def test_gating_records_the_steps_a_context_records(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    steps = _steps("a")
    ids = id_sets(parts["n_fluid"])["65"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        t_from = ctx.advance(1e9, max_steps=12)["t"]
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.tracers_enable(ids, every=5, t_from=t_from)
        ctx.advance(1e9, max_steps=steps)
        want = ctx.tracers()
    assert want["step"].tolist() == [15, 20, 25]
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.tracers_part_enable(ids, every=5, t_from=t_from)
        _run(slab, engines, "a")
        per_rank = [e.tracers_part_records() for e in engines]
        got = slab.pool_ring_tracers(per_rank, fold_DL=prm.DL)
    for p in per_rank:
        assert p["step"].tolist() == [15, 20, 25]
    assert got["step"].tolist() == want["step"].tolist() and np.all(np.abs(got["t"] - want["t"]) <= 1e-12 * want["t"])
    for r in range(3):
        for k in FIELDS:
            d = got[k][r] - want[k][r]
            if k == "x":
                d = d - np.round(d / prm.DL) * prm.DL
            assert np.max(np.abs(d)) <= RING_BOUND * np.max(np.abs(want[k][r])), (r, k)


def test_a_slab_without_a_tracer_still_stamps_the_record(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "f")
    with _ring(slab, prm, parts, "f") as engines:
        for e in engines:
            e.tracers_part_enable([parts["n_fluid"] // 2], every=2, capacity=CAPACITY)
        _run(slab, engines, "f")
        per_rank = [e.tracers_part_records() for e in engines]
        got = slab.pool_ring_tracers(per_rank)
    steps = list(range(2, _steps("f") + 1, 2))
    for p in per_rank:
        assert p["step"].tolist() == steps and p["t"].tobytes() == per_rank[0]["t"].tobytes() and p["x"].shape == (len(steps), 1)
        assert np.array_equal(p["n_owned"], (~np.isnan(p["x"][:, 0])).astype(np.int64))
    assert np.array_equal(sum(p["n_owned"] for p in per_rank), np.ones(len(steps), dtype=np.int64))
    assert sum(1 for p in per_rank if not p["n_owned"].any()) >= 2   # at least two of the four slabs never own it
    assert got["x"].shape == (len(steps), 1) and not np.isnan(got["x"]).any()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_full_buffer_drops_and_drain_refills_with_nan(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    nf = parts["n_fluid"]
    ids = _all_ids(parts)
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.tracers_part_enable(ids, every=1, capacity=4)
        _run(slab, engines, "a")                        # 27 steps, across the re-binning at K = 24
        full = [e.tracers_part_records() for e in engines]
        again = [e.tracers_part_records() for e in engines]          # reading without drain changes nothing
        drained = [e.tracers_part_records(drain=True) for e in engines]
        empty = [e.tracers_part_records() for e in engines]
        slab.HipSlabEngine.group_run(engines, 1)      # step 28 ends with the first re-binning that moves ownership
        before = _by_id([e.snapshot() for e in engines], nf)
        slab.HipSlabEngine.group_run(engines, 1)
        after = _by_id([e.snapshot() for e in engines], nf)
        resumed = [e.tracers_part_records() for e in engines]
        for e in engines:
            e.sync()
    for r in range(len(full)):
        assert full[r]["step"].tolist() == [1, 2, 3, 4] and full[r]["n_dropped"] == 23, r
        assert _bits(full[r]) == _bits(again[r]) == _bits(drained[r])
        assert len(empty[r]["step"]) == 0 and empty[r]["n_dropped"] == 0 and empty[r]["x"].shape == (0, nf) and len(empty[r]["n_owned"]) == 0
        assert resumed[r]["step"].tolist() == [28, 29] and resumed[r]["n_dropped"] == 0
    first = slab.pool_ring_tracers(full)                # (n_owned and the one-owner check hold on the kept records)
    second = slab.pool_ring_tracers(resumed)
    # ownership of some columns of row 1 differs between its two fillings (steps 2 and 29): the former owner must read NaN now
    moved = np.flatnonzero(first["owner"][1] != second["owner"][1])
    print(f"{len(moved)} of {nf} columns of row 1 changed owner between the first and the second filling")
    assert len(moved) >= 1
    for k in moved:
        was = int(first["owner"][1, k])
        assert not np.isnan(full[was]["x"][1, k])
        assert all(np.isnan(resumed[was][f][1, k]) for f in FIELDS), f"column {k}: rank {was} still holds its value of step 2"
    _assert_record_is_snapshot(prm, 2, ids, second, resumed, 1, before, after, "resumed: record 1")


def test_disable_run_enable_starts_from_zero(cfgmod, geom, slab):
    prm, parts = _case(cfgmod, geom, "a")
    ids = id_sets(parts["n_fluid"])["65"]
    with _ring(slab, prm, parts, "a") as engines:
        for e in engines:
            e.tracers_part_enable(ids, every=1, capacity=CAPACITY)
        slab.HipSlabEngine.group_run(engines, 5)
        for e in engines:  # (no sync in between: disable waits for the slab's streams itself)
            e.tracers_part_disable()
        slab.HipSlabEngine.group_run(engines, 4)
        for e in engines:
            e.tracers_part_enable(ids[:3], every=1, capacity=CAPACITY)
        slab.HipSlabEngine.group_run(engines, 3)
        got = slab.ring_tracers(engines)  # (no sync either: the read waits)
        sts = [e.sync() for e in engines]
    assert sts[0]["step"] == 12
    assert got["step"].tolist() == [10, 11, 12] and got["x"].shape == (3, 3) and got["n_dropped"] == 0
    assert np.array_equal(got["ids"], ids[:3])


# 8 ---------------------------------------------------------------------------------------------------------------
def test_no_column_is_written_from_a_stale_slot_behind_a_shrunken_population(cfgmod, geom, slab):
    """A skin of 2 h, re-binning every 16th step: a re-binning that leaves a slab with fewer slots than before leaves stale ids
    behind clk->n; a scan that read them would write a column twice (n_owned too large, or a halo's old value)."""
    name, N = "wide", 35
    prm, parts = _case(cfgmod, geom, name)
    run = _one_step_per_call(cfgmod, geom, slab, name, N)
    ids, pooled, per_rank, snaps = run["ids"], run["pooled"], run["per_rank"], run["snaps"]
    held = np.array([s["held"] for s in snaps])          # [N + 1, world] slots held
    shrank = np.argwhere(np.diff(held, axis=0) < 0)
    print(f"wide: slots held per slab from {held[0].tolist()} to {held[-1].tolist()}; shrank at (step, rank) "
          f"{[(int(s) + 1, int(r)) for s, r in shrank]}")
    assert len(shrank) >= 1
    assert min(int(s) for s, _ in shrank) + 1 < N        # ... with records behind it
    for r in range(N):
        _assert_record_is_snapshot(prm, 2, ids, pooled, per_rank, r, snaps[r], snaps[r + 1], f"wide: record {r}")


# 9 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi, slab):
    prm, parts = _case(cfgmod, geom, "a")
    nf, nt = parts["n_fluid"], parts["n_total"]
    L = capi.lib()
    good = np.array([5, nf - 1, 0], dtype=np.int32)
    nothing = (None,) * 8  # times, values, n_owned, ids, the four counts ...

    def config(ids=good, **kw):
        arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        c = capi.SphxTracersConfig(n_tracers=0 if arr is None else len(arr), every=1, capacity=16, t_from=0.0,
                                   ids=None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int32)))
        for k, v in kw.items():
            setattr(c, k, v)
        return c, arr

    def read(h, cap=0, arrays=nothing):
        return (L.sphx_slab_tracers_read, h, cap, *arrays, 0)  # ... and drain

    cfg, keep = config()

    def calls(h):
        return [(L.sphx_slab_tracers_enable, h, C.byref(cfg)), (L.sphx_slab_tracers_disable, h), read(h)]

    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        for call in calls(ctx._h):
            assert err_id(capi, *call) == ("SPHX:Slab:ctx", capi.SPHX_ERR_ARG), call[0].__name__
    # a slab of the caller-driven protocol (rebuild_every = 1), on a stream of the library's own
    h, f = C.c_void_p(), capi.f64
    params = capi.make_params(prm, 1e9, None, 0, 0, 1, 0.0)
    capi.check(L.sphx_slab_create(C.byref(h), C.byref(params), C.c_int(nf), C.c_int(nt),
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
        assert err_id(capi, *read(h)) == ("SPHX:Tracers:disabled", capi.SPHX_ERR_STATE)
        with pytest.raises(capi.SphxError) as ei:
            e.tracers_part_records()
        assert ei.value.identifier == "SPHX:Tracers:disabled"
        assert L.sphx_slab_tracers_disable(h) == capi.SPHX_OK  # (off already)
        # a bad config: the identifiers of section 2p, from the library and from the binding's own checks
        nan = float("nan")
        over = (1 << 27) // (3 * 4) + 1   # capacity * n_tracers * 4 just over the bound
        refused = [dict(ids=None, n_tracers=3), dict(n_tracers=0), dict(ids=[nf]), dict(ids=[nt - 1]), dict(ids=[nt]), dict(ids=[-1]),
                   dict(ids=[4, 9, 4]), dict(every=0), dict(capacity=0), dict(capacity=over), dict(t_from=nan)]
        for bad in refused:
            c2, keep2 = config(**bad)
            assert err_id(capi, L.sphx_slab_tracers_enable, h, C.byref(c2)) == ("SPHX:Tracers:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_slab_tracers_enable, h, None) == ("SPHX:Tracers:config", capi.SPHX_ERR_ARG)
        for kw in (dict(ids=[]), dict(ids=[nf]), dict(ids=[nt]), dict(ids=[-1]), dict(ids=[4, 9, 4]), dict(every=0), dict(capacity=0),
                   dict(capacity=over), dict(t_from=nan)):
            with pytest.raises(capi.SphxError) as ei:
                e.tracers_part_enable(**dict(dict(ids=good), **kw))
            assert ei.value.identifier == "SPHX:Tracers:config", kw
        slab.HipSlabEngine.group_run(engines, 2)   # (a step graph is captured behind the second step at the earliest)
        for x in engines:
            x.tracers_part_enable(good, every=1, capacity=16)
        slab.HipSlabEngine.graph_prepare(engines)
        slab.HipSlabEngine.group_run(engines, 3)
        before = e.tracers_part_records()
        assert before["step"].tolist() == [3, 4, 5]
        times, values, owned = np.zeros((3, 2)), np.zeros((3, 3, 4)), np.zeros(3, dtype=np.int64)
        i64 = owned.ctypes.data_as(C.POINTER(C.c_int64))
        assert err_id(capi, *read(h, 2, (capi.ptr(times),) + (None,) * 7)) == ("SPHX:Tracers:capacity", capi.SPHX_ERR_ARG)
        assert err_id(capi, *read(h, -1, (None, capi.ptr(values)) + (None,) * 6)) == ("SPHX:Tracers:capacity", capi.SPHX_ERR_ARG)
        assert err_id(capi, *read(h, 2, (None, None, i64) + (None,) * 5)) == ("SPHX:Tracers:capacity", capi.SPHX_ERR_ARG)
        assert np.all(times == 0) and np.all(values == 0) and np.all(owned == 0)
        n_tr, n = C.c_int(0), C.c_int(0)
        assert L.sphx_slab_tracers_read(h, 0, capi.ptr(times), capi.ptr(values), i64, None, C.byref(n_tr), C.byref(n), None,
                                        1) == capi.SPHX_OK   # capacity = 0: the sizes only, nothing copied or drained
        assert (n_tr.value, n.value) == (3, 3) and np.all(times == 0) and np.all(values == 0) and np.all(owned == 0)
        # a refused enable leaves the running series and its records as they are (and the prepared graph: every check is made
        # before the graph is dropped -- the next ten steps are one replay of it, which no call of the library counts)
        c2, keep2 = config(every=0)
        assert err_id(capi, L.sphx_slab_tracers_enable, h, C.byref(c2)) == ("SPHX:Tracers:config", capi.SPHX_ERR_ARG)
        with pytest.raises(capi.SphxError):
            e.tracers_part_enable(good, every=0)
        assert _bits(e.tracers_part_records()) == _bits(before)
        # the context's calls keep refusing a slab
        for fn, args in ((L.sphx_ctx_tracers_enable, (C.byref(cfg),)), (L.sphx_ctx_tracers_disable, ()), (L.sphx_ctx_tracers_sample, ()),
                         (L.sphx_ctx_tracers_read, (0, None, None, None, None, None, None, None, 0))):
            assert err_id(capi, fn, h, *args) == ("SPHX:Tracers:slab", capi.SPHX_ERR_ARG)
        slab.HipSlabEngine.group_run(engines, 10)
        for x in engines:
            x.sync()
        assert e.tracers_part_records()["step"].tolist() == list(range(3, 16))   # ... and the sampler running
        assert slab.ring_tracers(engines)["x"].shape == (13, 3)

