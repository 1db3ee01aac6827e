"""The dense cases do what they are for (not gpu): conditions on the INPUTS of tests/test_gpu_dense_lists.py, the dense sets of
test_gpu_switches.py and the dense rings of test_slab.py, established with the oracle and numpy alone (dense_cases.census),
never with the library under test.  Run with -s for the census table of every case.

Why the file exists: the states the rest of the suite steps are lattices with a jitter of at most 0.3 dp.  Their lists hold at
most 24 neighbours and their superset lists (2h + 1.05h) at most 54, against rows of 96 to 512 and 144 to 768 entries
(dense_cases.LIST_CAPACITY), so a lane of a 16-lane group reads at most 2 rows of its list and 4 of the superset, of a 32-lane
group 1 and 2: exactly the rows the compact kernels request ahead.  test_the_suites_own_states_stay_short records that.

Measured, small (dp 0.04, DL 1.5, seed 11: 950 fluid particles of 1 254), 24 counted steps, skin 1.05 h:

  case  s     R     list max at the start  lists > 64  superset max        over 24 steps
  A     0.55  0.30  59                     0           100                 list max 27 at the end, min 10, vmax 12.4
  B     0.45  0.40  89                     103         152 (12 > 144)      list max 31 at the end, min 8, vmax 16.8
  C     0.40  0.45  106                    205         182 (115 > 144)     list max 49 at the end, min 5, vmax 36.6

and A at the worker's size (dp 0.025, seed 31: 2 400 of 2 880), 35 steps: list max 69, superset max 141, the fullest cell
column 219 particles and the fullest three adjacent ones 560 (the plain variant: 160 and 480 in every column).  Both maxima
fall from the first step on: the patches burst.  Clusters of n = 97 .. 514 particles (dense_cases.cluster): every member holds
exactly n - 1 at the start and never more, the superset of a member n + 5 at the most, everybody else at most 24."""
import numpy as np
import pytest

import dense_cases as dc
from helpers import assert_close, make_case, make_variant

N_STEPS = 24
FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
_cache = {}


def _census(name, size, cfgmod, geom, oracle, n_steps=N_STEPS):
    if (name, size) not in _cache:
        prm, parts = (dc.plain if name == "plain" else dc.CASES[name])(cfgmod, geom, size)
        c = dc.census(oracle, prm, parts, n_steps)
        print(dc.census_line(f"{name} {size}", c))
        _cache[name, size] = prm, parts, c
    return _cache[name, size]


def test_the_suites_own_states_stay_short(cfgmod, geom, oracle):
    """The reason this file exists: no state of the default suite has a list longer than 32 or a superset longer than 64."""
    states = {
        "headline parity variant": make_variant(cfgmod, geom, dp=0.04, DL=3.0, jitter=0.2, seed=21, developed=True, rho0=2.5,
                                                transport_coeff=0.1),
        "grid-skin variant": make_variant(cfgmod, geom, dp=0.04, DL=1.5, jitter=0.3, seed=11, developed=True, rho0=2.5,
                                          transport_coeff=0.1),
        "switch worker variant": dc.plain(cfgmod, geom, "worker"),
        "dp 0.02, DL 3 make_case": make_case(cfgmod, geom, dp=0.02, DL=3.0, seed=7, developed=True),
    }
    for name, (prm, parts) in states.items():
        n2 = dc.list_lengths(oracle, prm, parts)
        ns = dc.list_lengths(oracle, prm, parts, radius_h=3.05)
        print(f"{name:>26}: list max {n2.max()} mean {n2.mean():.1f}, superset max {ns.max()}")
        assert n2.max() <= 32 and ns.max() <= 64, name
        # rows a lane owns: the prefetched ones only (two of the list at 16 and 32 lanes; 64 / lanes of the superset)
        for lpp in (16, 32):
            assert -(-int(n2.max()) // lpp) <= 2 and -(-int(ns.max()) // lpp) <= 64 // lpp, (name, lpp)


def test_sizes(cfgmod, geom):
    for size, (nf, nt) in dict(small=(950, 1254), worker=(2400, 2880)).items():
        prm0, plain = dc.plain(cfgmod, geom, size)
        for name, build in dc.CASES.items():
            prm, parts = build(cfgmod, geom, size)
            assert (parts["n_fluid"], parts["n_total"]) == (nf, nt) and prm == prm0, name
            x, y = parts["pos"][:nf, 0], parts["pos"][:nf, 1]
            assert np.all((x >= 0) & (x < prm.DL) & (y >= 0) & (y <= prm.DH)), name
            # a pull moves positions only: the members of one batch share everything else
            for k in ("vel", "mass", "wall_vel", "drho_dt"):
                assert np.array_equal(parts[k], plain[k]), (name, k)
            assert np.array_equal(parts["pos"][nf:], plain["pos"][nf:]), name


def test_A_runs_past_32_and_fits_every_lane_count(cfgmod, geom, oracle):
    prm, parts, c = _census("A", "small", cfgmod, geom, oracle)
    assert (c["list_max"][0], c["over64"][0], c["superset_max"][0]) == (59, 0, 100), dc.census_line("A", c)
    assert 32 < c["list_max"][0] and np.all(c["list_max"] <= 64) and np.all(c["superset_max"] <= 144)
    assert c["list_max"][-1] <= 32 and c["list_min"].min() <= 13 and c["finite"] and c["vmax"] > 5.0   # it bursts, voids open


def test_B_fits_96_but_not_the_superset_of_144(cfgmod, geom, oracle):
    prm, parts, c = _census("B", "small", cfgmod, geom, oracle)
    assert (c["list_max"][0], c["over64"][0], c["superset_max"][0], c["over144"][0]) == (89, 103, 152, 12), dc.census_line("B", c)
    assert 64 < c["list_max"][0] and np.all(c["list_max"] <= 96) and c["superset_max"][0] > 144
    assert np.all(c["superset_max"] <= 384)   # 16 and 32 lanes hold it
    assert c["list_max"][-1] <= 40 and c["finite"] and c["vmax"] > 5.0


def test_C_exceeds_96_and_fits_8_lanes(cfgmod, geom, oracle):
    prm, parts, c = _census("C", "small", cfgmod, geom, oracle)
    assert (c["list_max"][0], c["over64"][0], c["superset_max"][0], c["over144"][0]) == (106, 205, 182, 115), dc.census_line("C", c)
    assert 96 < c["list_max"][0] and np.all(c["list_max"] <= 128) and np.all(c["superset_max"] <= 192)
    assert c["finite"] and c["vmax"] > 5.0


def test_A_at_the_workers_size_loads_the_columns_unevenly(cfgmod, geom, oracle):
    prm, parts, c0 = _census("plain", "worker", cfgmod, geom, oracle, 2)
    assert (c0["column_max"][0], c0["three_columns_max"][0]) == (160, 480)
    assert c0["list_max"].max() <= 32 and c0["superset_max"].max() <= 64
    prm, parts, c = _census("A", "worker", cfgmod, geom, oracle, 35)
    assert (c["list_max"][0], c["superset_max"][0], c["column_max"][0], c["three_columns_max"][0]) == (69, 141, 219, 560)
    assert c["three_columns_max"][0] >= 1.1 * 480
    assert np.all(c["list_max"] <= 96) and np.all(c["superset_max"] <= 144)   # fits 2 lanes per particle on every step
    assert c["finite"]


def test_the_dense_ring_of_test_slab_straddles_its_cut(cfgmod, geom, oracle, pkg):
    """tests/test_slab.py's dense rings: A's pulls on the dp 0.04, DL 3 variant, one centred on the cut between two slabs."""
    import importlib
    slab = importlib.import_module(pkg.__name__ + ".slab")
    prm, parts = make_variant(cfgmod, geom, dp=0.04, DL=3.0, jitter=0.2, seed=11, developed=True, end_time=1e9, rho0=2.5,
                              transport_coeff=0.1)
    ncx = slab.n_cell_columns(prm)
    cut = slab.partition(ncx, 2)[0][1] * prm.DL / ncx
    s, R = dc.PULLS["A"]
    parts = dc.pulled(prm, parts, s, R, at=[(cut, 0.5 * prm.DH), (0.0, dc.SEAM_Y)])
    c = dc.census(oracle, prm, parts, 27)
    print(dc.census_line("A on the ring", c))
    nf = parts["n_fluid"]
    n2, x = c["lengths0"], parts["pos"][:nf, 0]
    for lo, hi in ((cut - R, cut), (cut, cut + R), (0.0, R), (prm.DL - R, prm.DL)):   # long lists on both sides of both cuts
        assert n2[(x >= lo) & (x < hi)].max() > 40, (lo, hi)
    assert 32 < c["list_max"][0] <= 64 and np.all(c["list_max"] <= 64) and np.all(c["superset_max"] <= 144) and c["finite"]


@pytest.mark.parametrize("n", [97, 98, 129, 130, 257, 258, 513, 514])
def test_cluster_members_hold_exactly_n_minus_one(n, cfgmod, geom, oracle):
    prm, parts = dc.cluster(cfgmod, geom, n)
    nf, nt = parts["n_fluid"], parts["n_total"]
    for k, width in dict(pos=2, vel=2, wall_vel=2, drho_dt=0, mass=0).items():
        assert parts[k].shape == ((nt, 2) if width else (nt,)), k
    rows = dc.cluster_rows(parts)
    assert not np.any(parts["vel"][rows]) and not np.any(parts["drho_dt"][rows])
    assert np.all(parts["mass"][rows] == prm.rho0 * prm.dp ** 2) and np.all(parts["pos"][nf:, 1] * (parts["pos"][nf:, 1] - prm.DH) > 0)
    c = dc.census(oracle, prm, parts, 4)
    print(dc.census_line(f"cluster {n}", c))
    others = np.delete(c["lengths0"], rows)
    assert np.all(c["lengths0"][rows] == n - 1) and others.max() <= 32
    assert np.all(c["list_max"] <= n - 1) and c["list_max"][0] == n - 1      # the maximum is at the start
    cap = max(v for v in dc.LIST_CAPACITY.values() if v <= n - 1)             # the capacity this cluster is the boundary of
    assert np.all(c["superset_max"] < 1.5 * cap), (c["superset_max"], cap)
    assert c["finite"]


def test_serial_and_threaded_oracle_agree_on_the_dense_states(cfgmod, geom, oracle):
    """The reference's own error on these states: the serial oracle against the OpenMP one (same formulas, another order of
    summation) after 4, 12 and 24 steps, at 1e-2 of the suite's tolerance -- the suite's tolerance holds here unchanged."""
    oracle.set_num_threads(8)
    for name in dc.CASES:
        prm, parts = dc.CASES[name](cfgmod, geom, "small")
        for n in (4, 12, 24):
            a = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n, enable_sort=False)
            b = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n, enable_sort=False, omp=True)
            worst = {}
            for k in FIELDS:
                scale = np.max(np.abs(a[k]))
                worst[k] = float(np.max(np.abs(a[k] - b[k]) / (1e-9 * np.abs(a[k]) + 1e-10 * scale + 1e-300)))
                assert_close(b[k], a[k], rtol=1e-11, atol_scale=1e-12, name=f"{name}:{k}@{n}")
            print(f"{name} @ {n:2d} steps: serial against threaded oracle, worst {max(worst.values()):.1e} of the tolerance "
                  f"({max(worst, key=worst.get)})")
