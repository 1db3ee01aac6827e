"""Cases, bounds and comparisons shared by tests/test_dens_stats_host.py, tests/test_gpu_dens_stats.py and
tests/test_gpu_batch_dens_stats.py (density statistics, include/sphx.h sections 2r / 2s).

The bound of the GPU comparisons.  count, outliers, the histogram, below and above are integers and compared exactly (on states
the GPU produced a particle within EDGE of a histogram edge or of +-delta_bound may move between the two adjacent counters).  A
summed field is compared with numpy's (profile.dens_stats_sums) bin by bin, relative to that field's largest |sum| over the
band, within
    BOUND = max(16 * FP_DEVIATION, 1e-12)   plus the quantisation term count * 2^-(s+1) of that field's scale.
FP_DEVIATION is the rounding error of the reference itself: the largest deviation, over every state of CASES and ANCHOR as
uploaded and every field, of the float64 sums from the sums whose per-particle sums are accumulated in np.longdouble in
reversed partner order.  MEASURED (tests/test_dens_stats_host.py::test_floating_point_bound prints it and asserts it stays
below the constant): 4.84e-15, on two_cols, field sum_d2, band 1; one_col 3.5e-15 (sum_d2, band 2), the other cases 1.8e-15 to
2.5e-15 (sum_dvol); the constant is rounded up to 8e-15.  delta is what is left of rho / rho0 after 1 is taken off, so it
carries rho's rounding error (1.1e-16 of rho0) whatever its own size: relative to sums of deltas of a few per cent that is the
few 1e-15 above.  The lattice at rest is the exception and is kept out of the constant: every delta there is -5.3e-05, the sums
are 1e-4 of the other states' and the same absolute error is 6.3e-12 of them; it is compared with its known value particle by
particle, within 1e-13 absolute, on the CPU and on the GPU.  16 x is for the device's different association (a lane-strided
pass and a shuffle tree against numpy's pairwise sums, and a fused multiply-add spline), and 16 * 8e-15 = 1.3e-13 < 1e-12:
the floor, the field map's bound (tests/test_gpu_field_map.py:BOUND), is what holds.  The quantisation term is derived, not measured: a particle's term is rounded to the nearest multiple of 2^-s, so a bin
of `count` particles is off by at most count * 2^-(s+1).  d_min and d_max are compared within BOUND of the largest |delta|."""
import numpy as np

import pair_dist_cases
import probe_cases

CASES = probe_cases.CASES        # compact, walk, dynamic and dual-rate forms, two columns, one column, 30 k particles, a wide skin
ANCHOR = pair_dist_cases.ANCHOR  # the four states of the oracle anchor: (dp, DL, jitter) of make_case(seed=11, developed=True)
FIELDS = ("count", "sum_d", "sum_d2", "sum_dvol", "sum_wall", "outliers", "d_min", "d_max")
COUNTS = ("count", "outliers")
SUMMED = ("sum_d", "sum_d2", "sum_dvol", "sum_wall")
EXTREMES = ("d_min", "d_max")
SCALE_OF = dict(sum_d="s_d", sum_d2="s_d2", sum_dvol="s_dvol", sum_wall="s_wall")
FP_DEVIATION = 8e-15
BOUND = max(16 * FP_DEVIATION, 1e-12)
EDGE = 1e-10                     # a delta this close to a histogram edge or to +-delta_bound may fall either side
HIST = ((64, 0.05), (64, 0.25))  # (n_hist, hist_range): the default, and a range that holds the jittered states' -0.144 .. 0.189
# n_bins of the sample-now sweep: in three bands (8 * n_bins + n_hist + 2) * 3 <= 7680 words of LDS, so 311 bins beside 64
# histogram bins (3 * (2488 + 66) = 7662) are the largest that fit: 312 ask for 7686
BINS = (1, 20, 311)
LATTICE_DELTA = -5.32310441e-05  # every particle of the lattice at rest, dp = 0.05, h = 1.3 dp: the walls continue the lattice
LATTICE_FP_DEVIATION = 8e-12     # the lattice's own figure (measured 6.3e-12, sum_d2, band 2: see above), for its GPU comparison


def bands(prm):
    hw = max(prm.dp, prm.h)
    return [(0.5 * prm.DL, hw), (0.0, hw)]  # mid-channel and the periodic seam


def density(profmod, prm, parts, pos, **how):
    """profile.summation_density -> (rho, wall) of the fluid rows of pos [n_total, 2] with the masses and walls of parts"""
    nf = parts["n_fluid"]
    return profmod.summation_density(pos[:nf], parts["mass"][:nf], prm.DL, prm.h, prm.rho0, prm.inv_sigma0, wall_pos=parts["pos"][nf:],
                                     wall_vol=parts["mass"][nf:] / prm.rho0, **how)


def numpy_sums(profmod, prm, parts, pos, n_bins, xbands, dens, n_hist=64, hist_range=0.05, delta_bound=0.5, quantise=False):
    """profile.dens_stats_sums of the fluid rows of pos from their density dens = (rho, wall): one dict per band"""
    nf = parts["n_fluid"]
    return profmod.dens_stats_sums(pos[:nf], parts["mass"][:nf], prm.DL, prm.DH, prm.h, prm.rho0, prm.inv_sigma0, n_bins, bands=xbands,
                                   n_hist=n_hist, hist_range=hist_range, delta_bound=delta_bound, density=dens, quantise=quantise)


def near_edges(delta, n_hist, hist_range, delta_bound, tol=EDGE):
    """the particles whose delta lies within tol of a histogram edge or of +-delta_bound: a bool per particle"""
    delta = np.asarray(delta, dtype=np.float64)
    edges = -hist_range + (2.0 * hist_range / n_hist) * np.arange(n_hist + 1)
    k = np.clip(np.searchsorted(edges, delta), 1, n_hist)
    near = np.minimum(np.abs(delta - edges[k - 1]), np.abs(delta - edges[k])) <= tol
    return near | (np.abs(np.abs(delta) - delta_bound) <= tol)


def deviation(a, b):
    """(largest deviation of a summed field's bin sum between two lists of sums, relative to that field's largest |sum| over the
    band; the field and band it was met in)"""
    worst = (0.0, None, None)
    for band, (x, y) in enumerate(zip(a, b)):
        for f in SUMMED:
            scale = float(np.max(np.abs(y[f])))
            if scale > 0.0:
                worst = max(worst, (float(np.max(np.abs(x[f] - y[f]))) / scale, f, band), key=lambda w: w[0])
    return worst


def quantisation(want, scales):
    """what the fixed-point grid of one sample may cost a bin: one {field: [n_bins]} per band, count * 2^-(s+1) with the scales
    profile.dens_scales gives for the sample"""
    return [{f: y["count"] * 2.0 ** -(scales[SCALE_OF[f]] + 1) for f in SUMMED} for y in want]


def add_quantisation(a, b):
    return [{f: x[f] + y[f] for f in SUMMED} for x, y in zip(a, b)]


def assert_sums_match(got, want, quant, what, bound=BOUND, loose=0):
    """two lists of sums, one dict per band: count, outliers, the histogram, below and above equal, every summed field within
    bound of the field's largest |sum| over the band plus the quantisation term (quantisation(), added up over the samples),
    d_min / d_max within bound of the largest |delta|.  loose: that many particles per band may each have moved between two
    adjacent integer counters (near_edges found them): every integer field may then differ by that much in all, and a summed
    bin by that many particles' terms (at most delta_bound-sized: the caller passes none unless it found such particles)."""
    assert len(got) == len(want) == len(quant), what
    for band, (x, y, q) in enumerate(zip(got, want, quant)):
        hx = np.concatenate([np.asarray(x["hist"], dtype=np.int64), [x["below"], x["above"]]])
        hy = np.concatenate([np.asarray(y["hist"], dtype=np.int64), [y["below"], y["above"]]])
        if loose == 0:
            for f in COUNTS:
                assert np.array_equal(x[f], y[f]), f"{what}: band {band} {f}: {x[f].sum()} {y[f].sum()}"
            assert np.array_equal(hx, hy), f"{what}: band {band} histogram: {np.flatnonzero(hx != hy)}"
        else:
            # a particle that crossed an edge leaves one counter and enters its neighbour: at most 2 * loose in all, sum kept
            assert np.abs(hx - hy).sum() <= 2 * loose and hx.sum() + x["outliers"].sum() == hy.sum() + y["outliers"].sum(), f"{what}: band {band} histogram"
            assert np.array_equal(x["count"] + x["outliers"], y["count"] + y["outliers"]), f"{what}: band {band} count + outliers"
            assert np.abs(x["count"] - y["count"]).sum() <= loose, f"{what}: band {band} count"
            if not np.array_equal(x["count"], y["count"]):
                continue  # (a particle at +-delta_bound went the other way: its terms are in one set of sums only)
        assert hx.sum() == x["count"].sum(), f"{what}: band {band}: the histogram holds {hx.sum()} of {x['count'].sum()}"
        for f in SUMMED:
            scale = float(np.max(np.abs(y[f])))
            allowed = bound * scale + q[f]
            err = np.abs(x[f] - y[f])
            k = int(np.argmax(err - allowed))
            print(f"{what}: band {band} {f} off by {err.max() / max(scale, 1e-300):.3e} of the largest |sum| {scale:.3e}, quantisation {q[f].max():.3e}")
            assert np.all(np.isfinite(x[f])) and np.all(err <= allowed), \
                f"{what}: band {band} {f} bin {k}: {x[f][k]!r} against {y[f][k]!r}, allowed {allowed[k]:.3e}"
        some = y["count"] > 0
        assert np.array_equal(np.isinf(x["d_min"]), ~some) and np.array_equal(np.isinf(x["d_max"]), ~some), f"{what}: band {band} empty bins"
        if some.any():
            top = max(float(np.max(np.abs(y["d_min"][some]))), float(np.max(np.abs(y["d_max"][some]))))
            for f in EXTREMES:
                err = float(np.max(np.abs(x[f][some] - y[f][some])))
                print(f"{what}: band {band} {f} off by {err / max(top, 1e-300):.3e} of the largest |delta| {top:.3e}")
                assert err <= bound * top, f"{what}: band {band} {f}"


def assert_identical(a, b, what, head=True):
    """two lists of sums, one dict per band: every field byte for byte, and the sample window"""
    assert len(a) == len(b), what
    for band, (x, y) in enumerate(zip(a, b)):
        for f in FIELDS + ("hist",):
            assert np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), f"{what}: band {band} {f}"
        assert (x["below"], x["above"]) == (y["below"], y["above"]), f"{what}: band {band} below / above"
        if head:
            assert (x["n_samples"], x["t_first"], x["t_last"]) == (y["n_samples"], y["t_first"], y["t_last"]), f"{what}: band {band} window"


def add_sums(profmod, a, b):
    """two lists of sums (one dict per band) as one: profile.add_dens_stats band by band"""
    return [profmod.add_dens_stats(x, y) for x, y in zip(a, b)]


def read_all(ctx, n_bands):
    """every band's sums of a context (or of one member: a list picked by the caller)"""
    return [ctx.dens_stats_sums(b) for b in range(n_bands)]
