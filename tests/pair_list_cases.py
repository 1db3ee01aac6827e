"""Pair lists a caller of the stateless surface may legally hand in, and what a test needs to know about each.

oracle.neighbor_search writes one kind of list: pair_i ascending, fluid-fluid pairs with i < j, no repeated and no r = 0 rows,
17-24 pairs per fluid particle.  The contract of sph_physics_shell_mex is wider (csrc/sphx_pairlist.hip, header): every pair once, in ANY
order, with either partner first, and the rows the reference skips (an index out of range, r <= 1e-12) skipped.  The functions
here turn a 7-column list (pair_i, pair_j, dx, dy, r, W, dW; indices 1-based, stored as doubles) into such lists: seeded, pure
numpy, the input left untouched.  Each returns the new list first and then what a test asserts about it.

Shared by tests/test_reference_anchor.py (the reference's own binaries against the oracle on these lists, and a census that the
lists are what they claim) and tests/test_gpu_pair_list_contract.py.  A plain module: no fixtures."""
import numpy as np

import regime_cases
from helpers import make_variant

# the two states the lists are built over, 600 fluid particles each: moving walls with uneven mass and rho0 != 1, and c_f = 0.3
# with hundreds of pairs on the cap of the Riemann term -- both see the reversed side of a swapped pair
STATES = {
    "moving_walls": lambda c, g: make_variant(c, g, dp=0.05, DL=1.5, jitter=0.2, seed=11, developed=True, rho0=2.5,
                                              transport_coeff=0.1),
    "capped": lambda c, g: regime_cases.capped(c, g, "small"),
}


def _take(nb, idx):
    return tuple(np.ascontiguousarray(np.asarray(c)[idx]) for c in nb)


def _insert(nb, at, rows):
    """rows (7 columns) put in front of the original positions `at`: the original rows keep their relative order.
    -> the list, the mask of the inserted rows in it"""
    out = tuple(np.insert(np.asarray(c, dtype=np.float64), at, np.asarray(v, dtype=np.float64)) for c, v in zip(nb, rows))
    new = np.insert(np.zeros(len(nb[0]), dtype=bool), at, True)
    return out, new


def _swap_rows(nb, rows):
    out = [np.array(c, dtype=np.float64, copy=True) for c in nb]
    out[0][rows], out[1][rows] = nb[1][rows], nb[0][rows]
    out[2][rows], out[3][rows] = -nb[2][rows], -nb[3][rows]
    return tuple(out)


def fluid_fluid(nb, nf):
    return (nb[0] >= 1) & (nb[0] <= nf) & (nb[1] >= 1) & (nb[1] <= nf)


def row_lengths(nb, nf, nt=None):
    """Entries per fluid particle's incidence row: the pairs it takes part in, on either side.  nt: also leave out the rows
    with j beyond n_total (a list with skipped rows); without it every j >= n_fluid counts as a wall particle."""
    i, j = nb[0].astype(np.int64) - 1, nb[1].astype(np.int64) - 1
    ok = (i >= 0) & (i < nf) & (j >= 0) & (True if nt is None else j < nt)
    return np.bincount(np.concatenate([i[ok], j[ok & (j < nf)]]), minlength=nf)[:nf]


def shuffled(nb, seed):
    """A random permutation of the rows.  -> list, the permutation"""
    perm = np.random.default_rng(seed).permutation(len(nb[0]))
    return _take(nb, perm), perm


def swapped(nb, nf, seed, fraction=0.5):
    """pair_i and pair_j exchanged, dx and dy negated, on `fraction` of the fluid-fluid rows; never a fluid-wall row (the wall
    particle of a pair is always its second).  -> list, the swapped rows"""
    ff = np.flatnonzero(fluid_fluid(nb, nf))
    rows = ff[np.random.default_rng(seed).random(len(ff)) < fraction]
    return _swap_rows(nb, rows), rows


def pick_one_sided(nb, nf, seed, n=5):
    """2 n fluid particles away from the walls (no wall partner in nb), no two of them partners of each other.
    -> always_second, always_first (0-based)"""
    i, j = nb[0].astype(np.int64) - 1, nb[1].astype(np.int64) - 1
    near_wall = np.zeros(nf, dtype=bool)
    near_wall[i[j >= nf]] = True
    ff = j < nf
    chosen = []
    for c in np.random.default_rng(seed).permutation(np.flatnonzero(~near_wall)):
        partners = np.concatenate([j[ff & (i == c)], i[ff & (j == c)]])
        if len(partners) and not np.intersect1d(partners, chosen).size:
            chosen.append(int(c))
        if len(chosen) == 2 * n:
            break
    assert len(chosen) == 2 * n, "too few interior particles"
    return np.array(chosen[:n]), np.array(chosen[n:])


def one_sided(nb, nf, always_second, always_first):
    """Exactly the fluid-fluid rows swapped that make every particle of always_second the second particle of all its pairs and
    every particle of always_first the first of all of its (0-based indices).  The always_second particles must have no wall
    partner: their incidence rows are then purely second-side.  Asserted here.  -> list, the swapped rows"""
    i, j = nb[0].astype(np.int64) - 1, nb[1].astype(np.int64) - 1
    ff = fluid_fluid(nb, nf)
    sec, fst = np.isin(i, always_second), np.isin(j, always_first)
    assert not np.any(ff & np.isin(i, always_second) & np.isin(j, always_second)), "two always_second particles are partners"
    assert not np.any(ff & np.isin(i, always_first) & np.isin(j, always_first)), "two always_first particles are partners"
    rows = np.flatnonzero(ff & (sec | fst))
    out = _swap_rows(nb, rows)
    assert is_one_sided(out, nf, always_second, always_first)
    return out, rows


def is_one_sided(nb, nf, always_second, always_first):
    i, j = nb[0].astype(np.int64) - 1, nb[1].astype(np.int64) - 1
    return bool(not np.any(np.isin(i, always_second)) and not np.any(np.isin(j, always_first))
                and all(np.count_nonzero(j == p) > 0 for p in always_second)
                and all(np.count_nonzero((i == p) & (j < nf)) > 0 for p in always_first))


def with_skipped_rows(nb, nf, nt, seed, k=64, beyond_n_total=True):
    """k rows the reference skips on their indices, at random places, NaN in all five geometry columns: a row whose geometry is
    read shows.  The rows cycle through i = 0, i = nf + 1 (a wall row), i = nt, i = -3, a valid i with j = 0 and with j = -1 --
    and, with beyond_n_total, a valid i with j = nt + 1 and j = nt + 5 (not for wall_shear_monitor: the reference's monitor has
    no upper bound on j, see test_reference_anchor.test_modes_skip_out_of_range_pair_indices_alike).
    -> list, the mask of the inserted rows"""
    rng = np.random.default_rng(seed)
    kinds = [(0, None), (nf + 1, None), (nt, None), (-3, None), (None, 0), (None, -1)]
    if beyond_n_total:
        kinds += [(None, nt + 1), (None, nt + 5)]
    bad_i, bad_j = np.zeros(k), np.zeros(k)
    for n in range(k):
        i, j = kinds[n % len(kinds)]
        bad_i[n] = rng.integers(1, nf + 1) if i is None else i
        bad_j[n] = rng.integers(1, nt + 1) if j is None else j
    at = np.sort(rng.integers(0, len(nb[0]) + 1, size=k))
    order = rng.permutation(k)  # which kind lands where
    rows = (bad_i[order], bad_j[order]) + (np.full(k, np.nan),) * 5
    return _insert(nb, at, rows)


def with_repeats(nb, seed, k=40):
    """k random rows of the list said a second time, at random places.  -> list, the mask of the added rows"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(nb[0]), size=k, replace=False)
    at = rng.integers(0, len(nb[0]) + 1, size=k)
    order = np.argsort(at, kind="stable")
    return _insert(nb, at[order], _take(nb, rows[order]))


def with_coincident(nb, nf, h, seed=0):
    """Three rows of coincident partners (dx = dy = r = dW = 0, W = W(0) = 10 / (7 pi h^2)) shuffled in: a fluid-fluid pair with
    i < j, one with i > j, and a fluid-wall pair (the first wall particle).  The density sum counts their W; every other sum
    skips them on r <= 1e-12.  -> list, the mask of the added rows"""
    rng = np.random.default_rng(seed)
    a, b, c, d, e = (int(x) + 1 for x in rng.choice(nf, size=5, replace=False))
    pi = np.array([min(a, b), max(c, d), e], dtype=np.float64)
    pj = np.array([max(a, b), min(c, d), nf + 1], dtype=np.float64)
    z = np.zeros(3)
    rows = (pi, pj, z, z, z, np.full(3, 10.0 / (7.0 * np.pi * h * h)), z)
    return _insert(nb, np.sort(rng.integers(0, len(nb[0]) + 1, size=3)), rows)


def emptied(nf):
    """The fluid particles without_particles is used on: the first, the last (its row ends the incidence) and two in between."""
    return np.array([0, nf // 3, nf // 2 + 1, nf - 1])


def without_particles(nb, particles):
    """Every pair of the listed fluid particles (0-based) dropped: their incidence rows are empty.  -> list, the rows kept"""
    i, j = nb[0].astype(np.int64) - 1, nb[1].astype(np.int64) - 1
    keep = np.flatnonzero(~(np.isin(i, particles) | np.isin(j, particles)))
    return _take(nb, keep), keep


def wide(oracle, parts, prm, factor=2.5):
    """The oracle's list for a kernel factor times as wide: rows factor^2 times as long.  -> list, h' = factor * prm.h, which
    the caller passes wherever a mode takes h.  The periodic box must still hold two supports: 4 h' <= DL."""
    hw = factor * prm.h
    assert 4 * hw <= prm.DL, (hw, prm.DL)
    return oracle.neighbor_search(parts["pos"], parts["n_fluid"], parts["n_total"], hw, prm.DL), hw


def contract_lists(oracle, prm, parts, nb, seed=0):
    """Every list above over one state and its oracle list nb.  -> {name: dict(nb, h, monitor_nb, ...)}: h is what the modes
    take as h, monitor_nb the list for wall_shear_monitor where it differs from nb (None: nb itself).  All but `one_sided` and
    `wide` derive from `any_order`, the shuffled and half-swapped list, named `clean` in their entries.  nan_rows: the rows of
    `mask` hold NaN geometry.  `shuffled` (order alone, no side swapped) is for the CPU anchor."""
    nf, nt = parts["n_fluid"], parts["n_total"]
    sh, perm = shuffled(nb, seed + 1)
    ss, swapped_rows = swapped(sh, nf, seed + 2)
    second, first = pick_one_sided(nb, nf, seed + 3)
    one, _ = one_sided(nb, nf, second, first)
    skipped, skipped_mask = with_skipped_rows(ss, nf, nt, seed + 4)
    skipped_mon, skipped_mon_mask = with_skipped_rows(ss, nf, nt, seed + 4, beyond_n_total=False)
    repeats, repeats_mask = with_repeats(ss, seed + 5)
    coincident, coincident_mask = with_coincident(ss, nf, prm.h, seed + 6)
    gone = emptied(nf)
    empty, _ = without_particles(ss, gone)
    wd, hw = wide(oracle, parts, prm)
    wd, _ = swapped(shuffled(wd, seed + 7)[0], nf, seed + 8)
    base = dict(h=prm.h, monitor_nb=None, clean=ss)
    return {
        "shuffled": dict(base, nb=sh, perm=perm),
        "any_order": dict(base, nb=ss, swapped_rows=swapped_rows),
        "one_sided": dict(base, nb=one, always_second=second, always_first=first, clean=nb),
        "skipped": dict(base, nb=skipped, monitor_nb=skipped_mon, mask=skipped_mask, monitor_mask=skipped_mon_mask, nan_rows=True),
        "repeats": dict(base, nb=repeats, mask=repeats_mask),
        "coincident": dict(base, nb=coincident, mask=coincident_mask),
        "empty_rows": dict(base, nb=empty, emptied=gone),
        "wide": dict(base, nb=wd, h=hw, clean=wd),
    }
