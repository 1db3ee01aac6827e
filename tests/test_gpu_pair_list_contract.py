"""-m gpu: the pair-list contract of the stateless MEX surface -- any order, either side first, bad rows skipped.

csrc/sphx_pairlist.hip does not walk the caller's list as the reference does: every call builds an incidence structure from it
(inc_degree, a three-kernel tiled scan, inc_fill with integer atomics, inc_rank) and runs each mode as a gather over a
particle's own row, 8 lanes per row.  Its header promises that the list may come "in any order", that "the summation order is a
function of the list alone, so results are bitwise repeatable" and that "pairs the reference skips (index out of range,
r <= 1e-12) are skipped here as well".  tests/test_gpu_mex_surface.py hands the modes only the list oracle.neighbor_search
writes (pair_i ascending, i < j, fluid first, no repeated or r = 0 rows, incidence rows of 17-24 entries, 600-1 875 fluid particles);
this file hands them the lists of tests/pair_list_cases.py, on which the reference's own binaries equal the oracle bit for bit
(tests/test_reference_anchor.py), so the oracle on the SAME list is the judge.

All eight modes run through helpers.run_modes, chained as test_reference_anchor.check_modes chains them; every mode takes its
inputs from the oracle's run, so the two sides are compared mode by mode on identical inputs.  Tolerances are those of
test_gpu_mex_surface.py, unchanged: rtol 1e-10 plus helpers.field_atol for viscous_force and the integrators, its per-mode
values for density, transport and tau.  Every comparison prints its worst error relative to the field's largest magnitude."""
import numpy as np
import pytest

import pair_list_cases
from helpers import assert_close, canon_pairs, field_atol, make_case, modes_dt, oracle_surface, run_modes

pytestmark = pytest.mark.gpu

BASES = pair_list_cases.STATES  # the states test_reference_anchor.py shows reference == oracle on, list by list
# n_fluid around the scan's tile (kScanTile = 1024 rows per workgroup): one short of a tile, a full tile, one row into the
# second, two full tiles; and 16 particles in one cell column (DL < 4 h), whose rows are wider than the whole channel is long
SIZES = {1023: dict(dp=1 / 31, DL=33 / 31), 1024: dict(dp=1 / 32, DL=1.0), 1025: dict(dp=0.04, DL=1.64),
         2048: dict(dp=1 / 32, DL=2.0), 16: dict(dp=0.25, DL=1.0)}


def tolerances(prm, parts, nb):
    """name of a run_modes output -> assert_close keywords, as tests/test_gpu_mex_surface.py has them.  nb: the list whose dW
    sizes helpers.field_atol's floors -- one without NaN geometry, or the floors are NaN and nothing can fail (asserted)."""
    at0, at = field_atol(prm, parts, nb, 0.0), field_atol(prm, parts, nb, modes_dt(prm))
    assert all(np.isfinite(v) for v in list(at0.values()) + list(at.values())), (at0, at)
    tol = {"density.rho": {}, "density.Vol": {}, "density.B": dict(rtol=1e-10, atol_scale=1e-12),
           "viscous": dict(rtol=1e-10, atol=at0["force"]), "tau": dict(rtol=1e-10, atol_scale=1e-12)}
    for mode, names in (("int1", ("rho", "p", "pos", "force", "drho")), ("int2", ("pos", "drho", "zeros")),
                        ("verlet", ("rho", "p", "pos", "vel", "drho", "force")),
                        ("advance", ("rho", "p", "pos", "vel", "drho", "force", "force_prior", "Vol", "B"))):
        for n in names:
            tol[f"{mode}.{n}"] = dict(rtol=1e-10, atol=at[n])
    return tol


def compare(what, got, want, prm, parts, nb):
    tol = tolerances(prm, parts, nb)
    err = {k: float(np.max(np.abs(np.asarray(got[k]) - np.asarray(want[k]))) / max(float(np.max(np.abs(want[k]))), 1e-300))
           for k in want}
    worst = max(err, key=lambda k: (np.isnan(err[k]), err[k]))
    print(f"[pair lists] {what}: worst error / field scale {err[worst]:.1e} ({worst})")
    assert set(got) == set(want)
    for k in want:
        kw = tol.get(k, dict(rtol=1e-13, atol_scale=1e-14))  # the three transport outputs
        assert k in tol or k.startswith("transport("), k
        assert_close(got[k], want[k], name=f"{what}: {k}", **kw)
    assert not np.any(got["int2.zeros"])


def same_bits(a, b, what):
    for k in a:
        x, y = (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in (a[k], b[k]))
        assert np.array_equal(x, y), f"{what}: {k} differs in {int(np.count_nonzero(x != y))} of {x.size} elements"


def device_vs_oracle(what, mex, oracle, prm, parts, c):
    """Both sides on the list c["nb"] (c: an entry of pair_list_cases.contract_lists).  The floors of the tolerances come from
    the list's rows that the modes read: all of them, or those outside c["mask"] where the mask marks rows with NaN geometry.
    -> device outputs, oracle outputs"""
    want = run_modes(oracle_surface(oracle), prm, parts, c["nb"], h=c["h"], monitor_nb=c["monitor_nb"])
    got = run_modes(mex.sph_physics_shell_mex, prm, parts, c["nb"], h=c["h"], given=want, monitor_nb=c["monitor_nb"])
    read = tuple(col[~c["mask"]] for col in c["nb"]) if c.get("nan_rows") else c["nb"]
    compare(what, got, want, prm, parts, read)
    return got, want


@pytest.fixture(scope="module", params=list(BASES))
def base(request, cfgmod, geom, oracle):
    prm, parts = BASES[request.param](cfgmod, geom)
    nf, nt = parts["n_fluid"], parts["n_total"]
    assert nf == 600
    nb = oracle.neighbor_search(parts["pos"], nf, nt, prm.h, prm.DL)
    lists = pair_list_cases.contract_lists(oracle, prm, parts, nb)
    clean = run_modes(oracle_surface(oracle), prm, parts, lists["any_order"]["nb"])
    return request.param, prm, parts, nb, lists, clean


@pytest.mark.parametrize("name", ["any_order", "one_sided"])
def test_any_order_either_side(name, base, mex, oracle):
    """(a) The shuffled list with half of its fluid-fluid rows said the other way round, and the oracle's list with five
    particles that are the second of every pair they have (rows purely of side 1) and five that are always the first."""
    tag, prm, parts, nb, lists, _ = base
    device_vs_oracle(f"{tag} {name}", mex, oracle, prm, parts, lists[name])


def test_modes_are_bitwise_repeatable(base, mex):
    """(b) Three calls of every mode on the shuffled and swapped list: identical bits.  inc_fill places a row's entries in the
    order its atomics arrive in; inc_rank is what makes that order a function of the list."""
    tag, prm, parts, nb, lists, clean = base
    c = lists["any_order"]
    runs = [run_modes(mex.sph_physics_shell_mex, prm, parts, c["nb"], given=clean) for _ in range(3)]
    same_bits(runs[0], runs[1], f"{tag}: second call")
    same_bits(runs[0], runs[2], f"{tag}: third call")


def test_neighbor_search_is_bitwise_repeatable(base, mex):
    """(b) Two searches of one state: the same seven columns bit for bit once sorted by (i, j) -- and as returned too: the
    search counts, scans and fills per particle (emit_pairs), so the order of its list is a function of the state as well."""
    tag, prm, parts, nb, _, _ = base
    raw = [mex.sph_neighbor_search_mex(parts["pos"], parts["n_fluid"], parts["n_total"], prm.h, prm.DL) for _ in range(2)]
    assert len(raw[0][0]) == len(nb[0])
    names = ("pair_i", "pair_j", "dx", "dy", "r", "W", "dW")
    same_bits(dict(zip(names, canon_pairs(raw[0]))), dict(zip(names, canon_pairs(raw[1]))), f"{tag}: second search, sorted")
    same_bits(dict(zip(names, raw[0])), dict(zip(names, raw[1])), f"{tag}: second search, as returned")


def test_skipped_rows_are_skipped_exactly(base, mex, oracle):
    """(c) 64 rows with an index out of range and NaN for geometry, inserted at random places: the device returns, bit for bit,
    what it returns on the list without them (inserting rows keeps the order of the others, so every incidence row holds the
    same pairs in the same order; only the pair indices shift), matches the oracle on the same list, and is finite everywhere
    (assert_close checks that): one skipped row's geometry read, and a NaN shows."""
    tag, prm, parts, nb, lists, clean = base
    got, _ = device_vs_oracle(f"{tag} skipped", mex, oracle, prm, parts, lists["skipped"])
    without = run_modes(mex.sph_physics_shell_mex, prm, parts, lists["any_order"]["nb"], given=clean)
    with_rows = run_modes(mex.sph_physics_shell_mex, prm, parts, lists["skipped"]["nb"], given=clean,
                          monitor_nb=lists["skipped"]["monitor_nb"])
    same_bits(with_rows, without, f"{tag}: with 64 skipped rows against without")
    assert all(np.all(np.isfinite(v)) for v in got.values())


@pytest.mark.parametrize("name", ["repeats", "coincident"])
def test_repeated_and_coincident_rows_count_as_in_the_reference(name, base, mex, oracle):
    """(d) A row said twice is summed twice; a row with r = 0 adds its W to the density and is skipped by every other sum.  The
    oracle's density on these lists differs from the clean list's by more than 1e-3 of its scale (asserted), so a surface
    that dropped such rows could not pass."""
    tag, prm, parts, nb, lists, clean = base
    _, want = device_vs_oracle(f"{tag} {name}", mex, oracle, prm, parts, lists[name])
    assert np.max(np.abs(want["density.rho"] - clean["density.rho"])) > 1e-3 * np.max(np.abs(clean["density.rho"]))


def test_empty_rows(base, mex, oracle):
    """(e) Fluid particles 0, n_fluid - 1 (the end of the incidence: row[n_fluid]) and two between them without a single pair:
    the oracle's result, and the identity for their B."""
    tag, prm, parts, nb, lists, _ = base
    got, _ = device_vs_oracle(f"{tag} empty rows", mex, oracle, prm, parts, lists["empty_rows"])
    for k in ("density.B", "advance.B"):
        assert np.array_equal(got[k][lists["empty_rows"]["emptied"]], np.tile([1.0, 0.0, 0.0, 1.0], (4, 1))), k


def test_long_rows(base, mex, oracle):
    """(f) The oracle's list for a kernel 2.5 times as wide (incidence rows of 115-137 entries: 15-18 rounds of the 8-lane row loop
    instead of 3), shuffled and half swapped, with h' = 2.5 h passed as the modes' h.  field_atol's floors, which count 30 terms per row, are
    left as they are: they hold (worst error 5.1e-14 of the field's scale, advance.p)."""
    tag, prm, parts, nb, lists, _ = base
    rows = pair_list_cases.row_lengths(lists["wide"]["nb"], parts["n_fluid"])
    assert rows.min() >= 100
    device_vs_oracle(f"{tag} wide (rows {rows.min()}-{rows.max()})", mex, oracle, prm, parts, lists["wide"])


@pytest.mark.parametrize("nf", list(SIZES))
def test_scan_edges(nf, cfgmod, geom, mex, oracle):
    """(g) n_fluid one short of the scan's tile, a full tile, one row beyond it, two tiles -- and 16 particles in a channel of
    one cell column, on the oracle's list (the geometry is the caller's).  The shuffled and half-swapped list over all modes."""
    prm, parts = make_case(cfgmod, geom, jitter=0.2, developed=True, seed=200 + nf, **SIZES[nf])
    assert parts["n_fluid"] == nf
    nb = oracle.neighbor_search(parts["pos"], nf, parts["n_total"], prm.h, prm.DL)
    sh, _ = pair_list_cases.shuffled(nb, nf)
    ss, rows = pair_list_cases.swapped(sh, nf, nf + 1)
    assert len(rows) > 0
    lengths = pair_list_cases.row_lengths(ss, nf)
    device_vs_oracle(f"nf {nf} (rows {lengths.min()}-{lengths.max()})", mex, oracle, prm, parts,
                     dict(nb=ss, h=prm.h, monitor_nb=None))
