"""Cases, bounds and the synthetic ring shared by tests/test_slab_dens_stats_host.py, tests/slab_dens_stats_worker.py and
tests/test_gpu_slab_dens_stats.py (density statistics of a slab ring, include/sphx.h section 3a).  The fields, bands, BOUND,
deviation(), near_edges() and the comparisons are tests/dens_stats_cases.py's, the cuts and the windows of the synthetic ring
tests/slab_grad_stats_cases.py's, all used as they are.

The bounds of the GPU comparisons.  count, outliers, the histogram, below and above are integers and compared exactly, but for
the particles near_edges finds on the REFERENCE state, which may move between two adjacent counters (assert_sums_match's
`loose`, band by band).  A summed field is compared bin by bin, relative to that field's largest |sum| over the band, within
    one sample against numpy on the ring's own state:   BOUND + MARGIN * SENSITIVITY * D_COPY   = 1e-12 + 16 * 600 * 4e-14 = 3.9e-10
    every step against a single context:                MARGIN * SENSITIVITY * RING_AGREEMENT   =         16 * 600 * 1e-9  = 9.6e-6
plus the quantisation term count * 2^-(s+1) of each slab's own scales (profile.dens_scales(delta_bound, the count the slab
HOLDS)), added over slabs and samples.  d_min / d_max are compared within the same bounds of the largest |delta|.

SENSITIVITY is the one measured figure: how much the sums move, in dens_stats_cases.deviation's measure, per unit of a
perturbation of every fluid position by uniform +-eps.  A density is a sum of W(r_ij), so a particle's delta moves by the slope
of W / sigma0 summed over its partners, about 1 / h per unit, and a bin's sum by that times (bin population)^1/2 against a sum of
(bin population) x a delta of a per cent or so.  MEASURED on the states of ring cases a, b and e of
tests/test_gpu_slab_samplers.py as they are uploaded, eps = 1e-14 and 1e-9
(tests/test_slab_dens_stats_host.py::test_sensitivity prints deviation / eps and asserts it stays below the constant; the
figures are in profiles/r38_slab_dens_stats.txt): a 153, b 162, e 571 at both eps (linear); the constant is the largest,
rounded up.  The same run measures PARTICLE_SENSITIVITY, the largest |d delta_i| / eps over the particles -- a 19, b 19, e 108,
rounded up to 120 --: what moves one particle's delta past a histogram edge or past +-delta_bound.  The edge clearance is
therefore
    one sample:   max(dens_stats_cases.EDGE, MARGIN * PARTICLE_SENSITIVITY * D_COPY)   = max(1e-10, 7.7e-11) = 1e-10
    every step:   MARGIN * PARTICLE_SENSITIVITY * RING_AGREEMENT                         = 1.9e-6
and the particles of the reference state within it are the `loose` ones.

MARGIN = 16, D_COPY = 4e-14 (the largest deviation of a halo copy's position from its owner's row at the sampling point, as the
ring's point probes show it) and RING_AGREEMENT = 1e-9 (the per-particle agreement of a ring's state with a single context's,
test_gpu_slab_samplers._guard) are tests/slab_grad_stats_cases.py's, for the reasons given there.

Conditions, not tolerances (a test that meets one fails with "another seed", it never skips): test_gpu_slab_samplers._guard
holds, and per band the loose particles are at most LOOSE_CAP = 0.5 % of the band's summed count.  The histogram of the
every-step comparisons is HIST_WIDE (64 bins on +-0.25): an edge every 7.8e-3 keeps the loose particles far below the cap."""
import numpy as np

import dens_stats_cases as dc
import slab_grad_stats_cases as gsc

SENSITIVITY = 600.0
PARTICLE_SENSITIVITY = 120.0
MARGIN = gsc.MARGIN
D_COPY = gsc.D_COPY
RING_AGREEMENT = gsc.RING_AGREEMENT
BOUND_ONE_SAMPLE = dc.BOUND + MARGIN * SENSITIVITY * D_COPY
BOUND_EVERY_STEP = MARGIN * SENSITIVITY * RING_AGREEMENT
EDGE_ONE_SAMPLE = max(dc.EDGE, MARGIN * PARTICLE_SENSITIVITY * D_COPY)
EDGE_EVERY_STEP = MARGIN * PARTICLE_SENSITIVITY * RING_AGREEMENT
LOOSE_CAP = 0.005
SENSITIVITY_CASES = ("a", "b", "e")
EPS = (1e-14, 1e-9)
HIST_WIDE = dict(n_hist=64, hist_range=0.25)
HEAD = dict(n_samples=1, t_first=0.5, t_last=0.5)

cuts = gsc.cuts
window_rows = gsc.window_rows


def fluid_state(parts):
    """(pos, mass) of the fluid rows of an uploaded state"""
    nf = parts["n_fluid"]
    return np.array(parts["pos"][:nf]), np.array(parts["mass"][:nf])


def walls_of(prm, parts):
    nf = parts["n_fluid"]
    return dict(wall_pos=np.array(parts["pos"][nf:]), wall_vol=np.array(parts["mass"][nf:]) / prm.rho0)


def synthetic_ring(profmod, prm, parts, world, n_bins, tweak=None, wall_tweak=None, **setting):
    """The state of parts cut into `world` windows, each holding what it owns plus copies of everything within 4 columns (8h) of
    it -- fluid and wall particles alike --, those from across the seam at x - DL or x + DL; -> (the ranks' partial sums by
    profile.dens_stats_sums_part, one list of band dicts per rank; the held fluid rows per rank as (index, shift, owned)).
    tweak(rank, index, shift, owned, pos) -> None or a bool mask of the held fluid rows to KEEP, after changing pos in place;
    wall_tweak(rank, index, shift, wall_pos) likewise for the held wall rows (the teeth of the comparison)."""
    pos, mass = fluid_state(parts)
    w = walls_of(prm, parts)
    edges, halo = cuts(prm, world), 8.0 * prm.h
    ranks, held = [], []
    for r in range(world):
        idx, shift, owned = window_rows(pos[:, 0], edges[r], edges[r + 1], prm.DL, halo)
        p = pos[idx].copy()
        p[:, 0] += shift
        if tweak is not None:
            keep = tweak(r, idx, shift, owned, p)
            if keep is not None:
                idx, shift, owned, p = idx[keep], shift[keep], owned[keep], p[keep]
        widx, wshift, _ = window_rows(w["wall_pos"][:, 0], edges[r], edges[r + 1], prm.DL, halo)
        wp = w["wall_pos"][widx].copy()
        wp[:, 0] += wshift
        if wall_tweak is not None:
            keep = wall_tweak(r, widx, wshift, wp)
            if keep is not None:
                widx, wp = widx[keep], wp[keep]
        ranks.append(profmod.dens_stats_sums_part(p, mass[idx], owned, prm.DL, prm.DH, prm.h, prm.rho0, prm.inv_sigma0, n_bins,
                                                  bands=dc.bands(prm), wall_pos=wp, wall_vol=w["wall_vol"][widx], **setting))
        held.append((idx, shift, owned))
    return ranks, held


def pooled(slab, ranks):
    """slab.pool_ring_dens_stats band by band: one dict per band"""
    return [slab.pool_ring_dens_stats([r[b] for r in ranks]) for b in range(len(ranks[0]))]


def with_head(ranks, **head):
    return [[dict(d, **dict(HEAD, **head)) for d in r] for r in ranks]


def density(profmod, prm, parts, pos=None):
    """(rho, wall) of the fluid rows pos (None: parts' own) in the whole, periodic channel, with parts' masses and walls"""
    p, mass = fluid_state(parts)
    return profmod.summation_density(p if pos is None else pos, mass, prm.DL, prm.h, prm.rho0, prm.inv_sigma0, **walls_of(prm, parts))


def unsplit(profmod, prm, parts, n_bins, pos=None, dens=None, **setting):
    """profile.dens_stats_sums of the whole channel: one dict per band; pos: the fluid rows, else parts' own"""
    p, mass = fluid_state(parts)
    p = p if pos is None else pos
    dens = dens if dens is not None else density(profmod, prm, parts, p)
    return profmod.dens_stats_sums(p, mass, prm.DL, prm.DH, prm.h, prm.rho0, prm.inv_sigma0, n_bins, bands=dc.bands(prm), density=dens,
                                   **setting)


def perturbed(parts, eps, seed=7):
    """the fluid positions, every component moved by uniform +-eps"""
    pos, _ = fluid_state(parts)
    rng = np.random.default_rng(seed)
    return pos + eps * (2.0 * rng.random(pos.shape) - 1.0)


def loose_per_band(profmod, prm, pos, delta, xbands, edge, n_hist=64, hist_range=0.05, delta_bound=0.5):
    """per band (band 0 first) the number of particles of pos with 0 <= y <= DH whose delta lies within `edge` of a histogram
    edge or of +-delta_bound: the particles that may move between two adjacent counters"""
    near = dc.near_edges(delta, n_hist, hist_range, delta_bound, tol=edge) & (pos[:, 1] >= 0.0) & (pos[:, 1] <= prm.DH)
    return [int(near.sum())] + [int((near & profmod.in_band(pos[:, 0], prm.DL, x, hw)).sum()) for x, hw in xbands]


def assert_loose_under_cap(loose, counts, what):
    """the condition on `loose`: per band at most LOOSE_CAP of the band's summed count"""
    for b, (n, c) in enumerate(zip(loose, counts)):
        assert n <= LOOSE_CAP * c, f"{what}: band {b}: {n} of {int(c)} particles on an edge, more than {LOOSE_CAP:.1%}: another seed"


def assert_bands_match(got, want, quant, loose, what, bound):
    """dens_stats_cases.assert_sums_match band by band, each with its own `loose`"""
    assert len(got) == len(want) == len(quant) == len(loose), what
    for b in range(len(got)):
        dc.assert_sums_match([got[b]], [want[b]], [quant[b]], f"{what} [band {b}]", bound=bound, loose=loose[b])
