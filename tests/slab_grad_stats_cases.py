"""Cases, bounds and the synthetic ring shared by tests/test_slab_grad_stats_host.py, tests/slab_grad_stats_worker.py and
tests/test_gpu_slab_grad_stats.py (gradient statistics of a slab ring, include/sphx.h section 3a).  The fields, bands, BOUND,
deviation() and the comparisons are tests/grad_stats_cases.py's, used as they are.

The bounds of the GPU comparisons.  count and skipped are integers and compared exactly.  A summed field is compared bin by bin,
relative to that field's largest |sum| over the band (grad_stats_cases.assert_sums_match), within
    one sample against numpy on the ring's own state:   BOUND + MARGIN * SENSITIVITY * D_COPY   = 1e-12 + 16 * 700 * 4e-14 = 4.5e-10
    every step against a single context:                MARGIN * SENSITIVITY * RING_AGREEMENT   =         16 * 700 * 1e-9  = 1.1e-5
plus the quantisation term count * 2^-(s+1) of each slab's own scales (profile.grad_scales with the count the slab HOLDS).

SENSITIVITY is the one measured figure: how much the sums move, in grad_stats_cases.deviation's measure, per unit of a
perturbation of every fluid position and velocity by uniform +-eps.  The estimate differentiates the state, so this is of the
order (bin population)^-1/2 / h times the conditioning of M, a few hundred.  MEASURED on the states of ring cases a, b and e of
tests/test_gpu_slab_samplers.py as they are uploaded, with and without wall partners, eps = 1e-14 and 1e-9
(tests/test_slab_grad_stats_host.py::test_sensitivity prints deviation / eps and asserts it stays below the constant; the
figures are in profiles/r34_slab_grad_stats.txt); the constant is the largest, rounded up.  It is linear in eps and the counts do
not change.  Consequence: the 1e-12 floor of the single-GPU tests cannot hold on a ring, where a halo copy's state is its
owner's only to a few ulps.

MARGIN = 16 is grad_stats_cases' factor for a different association (there: the device's lane-strided pass and shuffle tree
against numpy's pairwise sums; here also: a perturbation that is not uniform noise but whatever the copies' roundings are).

D_COPY is the largest deviation of a halo copy's position or velocity from its owner's row at the sampling point.  The
snapshots do not show it: sphx_slab_snapshot reads the state behind phase 3, whose halo refresh has then overwritten the copies
next to the cuts with their owners' rows (the GPU test measures the snapshot's figure, prints it and asserts it is below D_COPY
all the same).  The value ASSUMED is taken from profiles/r25_slab_point_probes.txt: the point probes of a ring, which
interpolate the same copies in front of phase 3, deviate from numpy over the owners' rows by at most 3.7e-14 of a record's
largest value in one sample (1.3e-14 without the tiny u_y column of the wall-line probes); rounded up, 4e-14.

RING_AGREEMENT = 1e-9 is the per-particle agreement of a ring's state with a single context's that
test_gpu_slab_samplers._guard documents.

Conditions, not tolerances (a test that meets one fails with "another seed"): test_gpu_slab_samplers._guard holds, no reference
particle has |det M - det_min| < 1e-6 and none a component within 1e-6 of the bound."""
import numpy as np

import grad_stats_cases as gc

SENSITIVITY = 700.0
MARGIN = 16.0
D_COPY = 4e-14
RING_AGREEMENT = 1e-9
BOUND_ONE_SAMPLE = gc.BOUND + MARGIN * SENSITIVITY * D_COPY
BOUND_EVERY_STEP = MARGIN * SENSITIVITY * RING_AGREEMENT
EDGE = 1e-6            # the clearance of det M from det_min and of |g| from the bound
SENSITIVITY_CASES = ("a", "b", "e")
EPS = (1e-14, 1e-9)
HEAD = dict(n_samples=1, t_first=0.5, t_last=0.5)


def fluid_state(prm, parts):
    """(pos, vel, vol) of the fluid rows of an uploaded state"""
    nf = parts["n_fluid"]
    return np.array(parts["pos"][:nf]), np.array(parts["vel"][:nf]), np.array(parts["mass"][:nf]) / prm.rho0


def u_max(prm):
    return abs(prm.gravity_g) * prm.DH * prm.DH / (8.0 * prm.nu)


def cuts(prm, world):
    """the left edges of `world` windows of [0, DL) and DL: whole columns of width 2h, as even as they come"""
    ncx = int(np.floor(prm.DL / (2.0 * prm.h)))
    csx = prm.DL / ncx
    return [((r * ncx) // world) * csx for r in range(world)] + [prm.DL]


def window_rows(x, lo, hi, DL, halo):
    """The rows a window [lo, hi) of a periodic channel holds: (index, shift, owned) -- what it owns (lo <= x < hi, shift 0) and
    copies of what lies within `halo` of it, those from across the seam with shift -DL or +DL (x + shift is the slab-frame x)."""
    idx, shift, owned = [], [], []
    mine = np.flatnonzero((x >= lo) & (x < hi))
    idx.append(mine), shift.append(np.zeros(len(mine))), owned.append(np.ones(len(mine), dtype=bool))
    for s in (-DL, 0.0, DL):
        xs = x + s
        sel = np.flatnonzero(((xs >= lo - halo) & (xs < lo)) | ((xs >= hi) & (xs < hi + halo)))
        idx.append(sel), shift.append(np.full(len(sel), s)), owned.append(np.zeros(len(sel), dtype=bool))
    return np.concatenate(idx), np.concatenate(shift), np.concatenate(owned)


def synthetic_ring(profmod, prm, parts, world, with_walls, n_bins, tweak=None, vmax=None, det_min=0.05):
    """The state of parts cut into `world` windows, each holding what it owns plus copies of everything within 4 columns (8h) of
    it, those from across the seam at x - DL or x + DL; -> (the ranks' partial sums by profile.grad_stats_sums_part, one list of
    band dicts per rank; the held rows per rank as (index, shift, owned)).  tweak(rank, index, shift, owned, pos, vel): changes
    the held rows of a rank in place before they are sampled (the teeth of the comparison)."""
    pos, vel, vol = fluid_state(prm, parts)
    nf = parts["n_fluid"]
    wpos, wvel, wvol = parts["pos"][nf:], parts["wall_vel"][nf:], parts["mass"][nf:] / prm.rho0
    edges, halo = cuts(prm, world), 8.0 * prm.h
    if vmax is None:
        vmax = float(np.sqrt(np.max(np.sum(vel * vel, axis=1))))
    ranks, held = [], []
    for r in range(world):
        idx, shift, owned = window_rows(pos[:, 0], edges[r], edges[r + 1], prm.DL, halo)
        p, v = pos[idx].copy(), vel[idx].copy()
        p[:, 0] += shift
        if tweak is not None:
            tweak(r, idx, shift, owned, p, v)
        walls = {}
        if with_walls:
            widx, wshift, _ = window_rows(wpos[:, 0], edges[r], edges[r + 1], prm.DL, halo)
            wp = wpos[widx].copy()
            wp[:, 0] += wshift
            walls = dict(wall_pos=wp, wall_vel=wvel[widx], wall_vol=wvol[widx])
        ranks.append(profmod.grad_stats_sums_part(p, v, vol[idx], owned, prm.DL, prm.DH, prm.h, n_bins, bands=gc.bands(prm), det_min=det_min,
                                                  vmax=vmax, **walls))
        held.append((idx, shift, owned))
    return ranks, held


def pooled(slab, ranks):
    """slab.pool_ring_grad_stats band by band: one dict per band"""
    return [slab.pool_ring_grad_stats([r[b] for r in ranks]) for b in range(len(ranks[0]))]


def with_head(ranks, **head):
    return [[dict(d, **dict(HEAD, **head)) for d in r] for r in ranks]


def unsplit(profmod, prm, parts, with_walls, n_bins, det_min=0.05, state=None):
    """profile.grad_stats_sums of the whole channel: one dict per band; state: (pos, vel) of the fluid rows, else parts' own"""
    pos, vel, vol = fluid_state(prm, parts)
    if state is not None:
        pos, vel = state
    walls = gc.walls_of(prm, parts) if with_walls else {}
    return profmod.grad_stats_sums(pos, vel, vol, prm.DL, prm.DH, prm.h, n_bins, bands=gc.bands(prm), det_min=det_min, **walls)


def perturbed(prm, parts, eps, seed=7):
    """(pos, vel) of the fluid rows, every component moved by uniform +-eps"""
    pos, vel, _ = fluid_state(prm, parts)
    rng = np.random.default_rng(seed)
    return pos + eps * (2.0 * rng.random(pos.shape) - 1.0), vel + eps * (2.0 * rng.random(vel.shape) - 1.0)


def census(profmod, prm, parts, with_walls):
    """det M and max |G| over the fluid particles of an uploaded state"""
    pos, vel, vol = fluid_state(prm, parts)
    walls = gc.walls_of(prm, parts) if with_walls else {}
    g = profmod.velocity_gradients(pos, vel, vol, prm.DL, prm.h, **walls)
    return g["det"], np.max(np.abs(g["G"]), axis=1)


def det_min_that_skips(det, gap=1e-4, at_least=20):
    """a det_min in the middle of the first gap of at least `gap` in the sorted det M that has `at_least` particles or more
    below it: those with the smallest det M -- the wall-adjacent ones, whose support is one-sided -- are then skipped.
    -> (det_min, the number of particles below it)"""
    d = np.sort(det)
    k = at_least + np.flatnonzero(np.diff(d)[at_least - 1:] >= gap)
    assert len(k), "no gap in det M: another seed"
    return float(0.5 * (d[k[0] - 1] + d[k[0]])), int(k[0])
