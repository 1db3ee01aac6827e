"""-m gpu: the step kernels on dense neighbourhoods, up to the capacity of their list rows.

Every other state of the suite is a jittered lattice: at most 24 neighbours and a superset of at most 54, so a lane reads only
the rows of its list column that the kernels request ahead (two of the step's list at 16 and 32 lanes per particle, 64 / lanes
of the superset list) and never the general row fetch behind them; no list comes near its capacity, and every cell column
holds the same load.  The states of tests/dense_cases.py do all of that (tests/test_dense_cases.py holds the census):

  A  list max 59, superset 100: fits every lane count                      (rows per lane at 16 lanes: 4 and 7)
  B  list max 89, superset 152: fits 96 entries, not the 144 of the superset list at 1, 2 and 4 lanes
  C  list max 106, superset 182: needs 8 lanes (128 / 192) or more
  cluster(n): every member holds exactly n - 1 -- the capacity itself (n - 1 = 96 / 128 / 256 / 512) and one more

(a) 24 steps across re-binnings against the oracle at every lane count that holds the case, (b) the same without a skin, (c)
and (d) overflow is reported with SPHX_ERR_GRID, never truncated, and exactly the capacity is accepted and right, (f) a batch
whose members' lists differ in length by 4 x.  The tolerances are the suite's (rtol 1e-9, atol_scale 1e-10 after <= 25 steps):
the serial and the threaded oracle differ by less than 1e-4 of it on these states (tests/test_dense_cases.py)."""
import numpy as np
import pytest

import dense_cases as dc
from helpers import assert_close, canon_pairs, full_state

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
N_STEPS = 24
SKINNED = dict(rebuild_every=8, skin_h=1.05)
_inputs, _refs = {}, {}


def _case(name, cfgmod, geom):
    """(prm, parts) of "plain", "A", "B", "C" at the small size or of ("cluster", n); built once, never changed."""
    if name not in _inputs:
        if isinstance(name, tuple):
            _inputs[name] = dc.cluster(cfgmod, geom, name[1])
        else:
            _inputs[name] = (dc.plain if name == "plain" else dc.CASES[name])(cfgmod, geom, "small")
    return _inputs[name]


def _ref(name, n_steps, cfgmod, geom, oracle):
    """The oracle's state after n_steps: computed once, shared by the tests that need it."""
    if (name, n_steps) not in _refs:
        prm, parts = _case(name, cfgmod, geom)
        _refs[name, n_steps] = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n_steps, enable_sort=False)
    return _refs[name, n_steps]


def _worst(got, ref):
    return {k: float(np.max(np.abs(got[k] - ref[k])) / max(np.max(np.abs(ref[k])), 1e-300)) for k in FIELDS}


def _compare_state(what, got, st, mon, ref, n_steps):
    """All nine outputs, t, dt_last, vmax, the pair count and the wall shear (tests/test_gpu_large_configs.py::_compare)."""
    rs = ref["stats"]
    worst = _worst(got, ref)
    print(f"[dense] {what}: {n_steps} steps, worst {max(worst.values()):.1e} ({max(worst, key=worst.get)}) "
          f"dt {abs(st['dt_last'] - rs['dt_last']) / rs['dt_last']:.1e} vmax {abs(st['vmax'] - rs['vmax']) / rs['vmax']:.1e}")
    assert st["step"] == n_steps == rs["steps"]
    assert abs(st["t"] - rs["t"]) <= 1e-13 * rs["t"]
    assert abs(st["dt_last"] - rs["dt_last"]) <= 1e-12 * rs["dt_last"]
    assert abs(st["vmax"] - rs["vmax"]) <= 1e-9 * rs["vmax"]
    for k in FIELDS:
        assert_close(got[k], ref[k], rtol=1e-9, atol_scale=1e-10, name=f"{what}:{k}@{n_steps}")
    if mon is not None:
        tb, tt, npairs = mon
        assert npairs == rs["n_pairs_last"], (npairs, rs["n_pairs_last"])
        assert_close(np.array([tb, tt]), np.array([rs["tau_bottom"], rs["tau_top"]]), rtol=1e-8, atol_scale=1e-9,
                     name=f"{what}:tau")


def _assert_list_is_the_oracles(what, ctx, prm, parts, oracle):
    nb = ctx.neighbor_list()
    pos = ctx.download(fields=("pos",))["pos"]
    ref = oracle.neighbor_search(pos, parts["n_fluid"], parts["n_total"], prm.h, prm.DL)
    a, b = canon_pairs(nb), canon_pairs(ref)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    assert_close(a[4], b[4], rtol=1e-13, atol=1e-15 * prm.DL, name=f"{what}: r")


def _assert_forms(ctx, lpp):
    """walk kernels up to 8 lanes per particle, the compact ones from 16"""
    forms = ctx.kernel_forms()
    assert ctx.tuning()["lanes_per_particle"] == lpp and forms["walk_kernels"] == (lpp <= 8), (lpp, forms)


def _run_against_oracle(name, lpp, n_steps, kw, cfgmod, geom, capi, oracle):
    prm, parts = _case(name, cfgmod, geom)
    ref = _ref(name, n_steps, cfgmod, geom, oracle)
    what = f"{name if isinstance(name, str) else 'cluster %d' % name[1]} lpp {lpp} K {kw['rebuild_every']}"
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=lpp, **kw) as ctx:
        _assert_forms(ctx, lpp)
        pol, rebins0 = ctx.grid_policy(), ctx.schedule()["rebins"]
        assert pol["rebuild_every"] == kw["rebuild_every"], pol
        assert pol["skin"] == (kw["skin_h"] * prm.h if "skin_h" in kw else 0.0), pol
        st = ctx.advance(1e9, max_steps=n_steps)
        got = ctx.download()
        mon = ctx.monitor(tau=True, pairs=True)
        rebins = ctx.schedule()["rebins"] - rebins0 + ctx.grid_policy()["forced_rebuilds"]
    _compare_state(what, got, st, mon, ref, n_steps)
    nf = parts["n_fluid"]
    assert np.all(got["pos"][:nf, 0] >= 0) and np.all(got["pos"][:nf, 0] <= prm.DL)
    return rebins


# (a) ------------------------------------------------------------------------------------------------------------------
# by what the lane count holds: 96 / 144 entries up to 4 lanes, 128 / 192 at 8, 256 / 384 and 512 / 768 at 16 and 32
STEPPED = [(1, "A"), (2, "A"), (4, "A"), (8, "A"), (8, "C"), (16, "A"), (16, "B"), (16, "C"), (32, "A"), (32, "B"), (32, "C")]


@pytest.mark.parametrize("lpp,name", STEPPED, ids=[f"lpp{l}-{n}" for l, n in STEPPED])
def test_stepped_parity_across_rebinnings(lpp, name, cfgmod, geom, capi, oracle):
    """24 steps on the superset list (K = 8, skin 1.05 h): pass A walks up to 182 superset entries, passes B, CD and E up to 106
    list entries per particle -- 7 rows of a lane's column at 16 lanes, 12 of the superset -- and the patches burst on the
    way (voids of 5 to 10 neighbours, |v| of 12 to 37 against U = 1), so the drift bound forces re-binnings as well."""
    rebins = _run_against_oracle(name, lpp, N_STEPS, SKINNED, cfgmod, geom, capi, oracle)
    assert rebins >= 2, rebins


@pytest.mark.parametrize("lpp,name", STEPPED, ids=[f"lpp{l}-{n}" for l, n in STEPPED])
def test_device_pair_list_is_the_oracles(lpp, name, cfgmod, geom, capi, oracle):
    """ctx.neighbor_list() at the start (the longest lists) and after 3 steps, from a grid binned 3 steps ago"""
    prm, parts = _case(name, cfgmod, geom)
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=lpp, **SKINNED) as ctx:
        _assert_forms(ctx, lpp)
        _assert_list_is_the_oracles(f"{name} lpp {lpp} at the start", ctx, prm, parts, oracle)
        assert ctx.advance(1e9, max_steps=3)["step"] == 3
        _assert_list_is_the_oracles(f"{name} lpp {lpp} after 3 steps", ctx, prm, parts, oracle)


# (b) ------------------------------------------------------------------------------------------------------------------
SWEPT = [(1, "B"), (2, "B"), (4, "B"), (8, "B"), (16, "B"), (32, "A")]


@pytest.mark.parametrize("lpp,name", SWEPT, ids=[f"lpp{l}-{n}" for l, n in SWEPT])
def test_stepped_parity_without_a_skin(lpp, name, cfgmod, geom, capi, oracle):
    """rebuild_every = 1: every step re-bins and pass A sweeps the cells -- no superset list, so B (89 of 96) fits few lanes"""
    _run_against_oracle(name, lpp, 6, dict(rebuild_every=1), cfgmod, geom, capi, oracle)


# (c) ------------------------------------------------------------------------------------------------------------------
def _assert_overflow_is_reported(prm, parts, capi, **kw):
    with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
        with pytest.raises(capi.SphxError) as e:
            ctx.advance(1e9, max_steps=2)
        assert e.value.code == capi.SPHX_ERR_GRID, e.value


@pytest.mark.parametrize("lpp", [2, 4])
def test_superset_overflow_is_reported_while_the_list_fits(lpp, cfgmod, geom, capi):
    """B: the step's list fits (89 of 96), the superset list does not (152 of 144)"""
    _assert_overflow_is_reported(*_case("B", cfgmod, geom), capi, lanes_per_particle=lpp, **SKINNED)


@pytest.mark.parametrize("lpp", [1, 2, 4])
def test_list_overflow_is_reported_without_a_skin(lpp, cfgmod, geom, capi):
    """C: 106 neighbours against 96"""
    _assert_overflow_is_reported(*_case("C", cfgmod, geom), capi, lanes_per_particle=lpp, rebuild_every=1)


# (d) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(rebuild_every=1), SKINNED], ids=["swept", "skinned"])
@pytest.mark.parametrize("lpp", sorted(dc.LIST_CAPACITY))
def test_exactly_the_capacity_is_accepted_and_one_more_is_reported(lpp, kw, cfgmod, geom, capi, oracle):
    """cluster(capacity + 1): every member's list is full to the last entry of its last row -- 3 steps must be the oracle's, and
    the device's pair list the oracle's.  cluster(capacity + 2): the first advance raises SPHX_ERR_GRID.  (The superset of a
    member is the cluster and a few: it must stay below 1.5 x the capacity, or the skinned run would test another bound.)"""
    cap = dc.LIST_CAPACITY[lpp]
    prm, parts = _case(("cluster", cap + 1), cfgmod, geom)
    c = dc.census(oracle, prm, parts, 3, skin_h=1.05)
    assert c["list_max"][0] == cap and np.all(c["list_max"] <= cap) and np.all(c["superset_max"] < 1.5 * cap), dc.census_line("", c)
    _run_against_oracle(("cluster", cap + 1), lpp, 3, kw, cfgmod, geom, capi, oracle)
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=lpp, **kw) as ctx:
        _assert_list_is_the_oracles(f"cluster {cap + 1} lpp {lpp}", ctx, prm, parts, oracle)
    prm, parts = _case(("cluster", cap + 2), cfgmod, geom)
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=lpp, **kw) as ctx:
        with pytest.raises(capi.SphxError) as e:
            ctx.advance(1e9, max_steps=1)
        assert e.value.code == capi.SPHX_ERR_GRID, e.value


# (f) ------------------------------------------------------------------------------------------------------------------
def test_batch_of_plain_A_and_B(cfgmod, geom, capi, oracle):
    """Three members on one geometry whose longest lists are 24, 59 and 89 entries: a row bound taken from the wrong member
    shows.  A drift-forced re-binning re-bins all members of a batch, which a standalone context would not do at that step, so
    interval and skin are given: K = 4 with a skin of 2 h -- the oracle's particles move at most 0.85 h in four steps of B
    (0.68 h in A, 0.25 h in the plain variant) against the half skin of 1 h; that nothing was forced is asserted.  The superset
    radius is 4 h then: 90, 131 and 195 entries of 384."""
    names = ("plain", "A", "B")
    members = [_case(n, cfgmod, geom) for n in names]
    kw = dict(t_end=1e9, lanes_per_particle=16, rebuild_every=4, skin_h=2.0)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        assert b.info()["lanes_per_particle"] == 16 and b.info()["rebuild_every"] == 4
        b.enqueue_steps(N_STEPS)
        sts = b.sync()
        got = [full_state(b.download(m), sts[m], b.monitor(m, tau=True, pairs=True)) for m in range(len(members))]
        info = b.info()
    assert info["realignments"] == 0 and info["forced_rebuilds"] == 0, info
    for m, (prm, parts) in enumerate(members):
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.enqueue_steps(N_STEPS)
            st = ctx.sync()
            alone = full_state(ctx.download(), st, ctx.monitor(tau=True, pairs=True))
            assert ctx.grid_policy()["forced_rebuilds"] == 0
        for k in alone:
            assert np.array_equal(np.asarray(got[m][k]), np.asarray(alone[k])), f"member {m} ({names[m]}): {k} differs"
        ref = _ref(names[m], N_STEPS, cfgmod, geom, oracle)
        _compare_state(f"batch member {names[m]}", got[m], sts[m], (got[m]["tau"][0], got[m]["tau"][1], got[m]["pairs"]), ref,
                       N_STEPS)
