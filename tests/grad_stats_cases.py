"""Cases, bounds and comparisons shared by tests/test_grad_stats_host.py, tests/test_gpu_grad_stats.py and
tests/test_gpu_batch_grad_stats.py (gradient statistics, include/sphx.h sections 2n / 2o).

The bound of the GPU comparisons.  count and skipped are integers and compared exactly.  A summed field is compared with numpy's
(profile.grad_stats_sums) bin by bin, relative to that field's largest |sum| over the band, within
    BOUND = max(16 * FP_DEVIATION, 1e-12)   plus the quantisation term count * 2^-(s+1) of the sample's own scale.
FP_DEVIATION is the rounding error of the reference itself: the largest deviation, over every state below and every field, of
the float64 sums from the sums whose per-particle sums are accumulated in np.longdouble in reversed partner order.  The states
are those of CASES as they are uploaded; the GPU tests compare seven steps later, on nearly the same arrangements and velocities,
which no CPU test can hold.  one_col starts at rest, where every sum is zero, so it is measured with the analytic parabola on
its arrangement.  MEASURED (tests/test_grad_stats_host.py::test_floating_point_bound prints it and asserts it stays below the
constant): 2.7e-15, on one_col, field sum_gxx2, band 1; two_cols 1.8e-15 (sum_gxx, band 0), the other cases 0.8e-15 to 1.0e-15;
the constant is rounded up to 4e-15.  16 x is for the
device's different association (a lane-strided pass and a shuffle tree against numpy's pairwise sums), and 16 * 4e-15 =
6.4e-14 < 1e-12: the floor, the field
map's bound (tests/test_gpu_field_map.py:BOUND), is what holds.  The quantisation term is derived, not measured: a particle's
term is rounded to the nearest multiple of 2^-s, so a bin of `count` particles is off by at most count * 2^-(s+1)."""
import numpy as np

import pair_dist_cases
import probe_cases

CASES = probe_cases.CASES        # compact, walk, dynamic and dual-rate forms, two columns, one column, 30 k particles, a wide skin
ANCHOR = pair_dist_cases.ANCHOR  # the four states of the oracle anchor: (dp, DL, jitter) of make_case(seed=11, developed=True)
FIELDS = ("count", "sum_gxx", "sum_gxy", "sum_gyx", "sum_gyy", "sum_gxx2", "sum_gxy2", "sum_gyx2", "sum_gyy2", "sum_div2", "sum_vort2",
          "skipped")
COUNTS = ("count", "skipped")
SUMMED = FIELDS[1:-1]
SCALE_OF = dict({f: "s1" for f in FIELDS[1:5]}, **{f: "s2" for f in FIELDS[5:9]}, sum_div2="s3", sum_vort2="s3")
FP_DEVIATION = 4e-15
BOUND = max(16 * FP_DEVIATION, 1e-12)
BINS = (1, 20, 213)              # 213 bins in three bands are 639 of the 640 a workgroup's LDS holds


def bands(prm):
    hw = max(prm.dp, prm.h)
    return [(0.5 * prm.DL, hw), (0.0, hw)]  # mid-channel and the periodic seam


def walls_of(prm, parts):
    """the wall particles as the keywords of profile.velocity_gradients / grad_stats_sums"""
    nf = parts["n_fluid"]
    return dict(wall_pos=parts["pos"][nf:], wall_vel=parts["wall_vel"][nf:], wall_vol=parts["mass"][nf:] / prm.rho0)


def gradients(profmod, prm, parts, state, with_walls, **how):
    """profile.velocity_gradients of the fluid rows of state (pos, vel) with the masses and walls of parts"""
    nf = parts["n_fluid"]
    walls = walls_of(prm, parts) if with_walls else {}
    return profmod.velocity_gradients(state["pos"][:nf], state["vel"][:nf], parts["mass"][:nf] / prm.rho0, prm.DL, prm.h, **walls, **how)


def numpy_sums(profmod, prm, parts, state, n_bins, xbands, grads, vmax=None, det_min=0.05):
    """profile.grad_stats_sums of a state from its gradients: one dict per band"""
    nf = parts["n_fluid"]
    return profmod.grad_stats_sums(state["pos"][:nf], state["vel"][:nf], parts["mass"][:nf] / prm.rho0, prm.DL, prm.DH, prm.h, n_bins,
                                   bands=xbands, det_min=det_min, vmax=vmax, gradients=grads)


def vmax_of(parts, state):
    nf = parts["n_fluid"]
    return float(np.sqrt(np.max(np.sum(state["vel"][:nf] ** 2, axis=1))))


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
    profile.grad_scales gives for the sample"""
    return [{f: y["count"] * 2.0 ** -(scales[SCALE_OF[f]] + 1) for f in SUMMED} for y in want]


def add_quantisation(a, b):
    return [{f: x[f] + y[f] for f in SUMMED} for x, y in zip(a, b)]


def assert_sums_match(got, want, quant, what, bound=BOUND):
    """two lists of sums, one dict per band: count and skipped equal, every summed field within bound of the field's largest
    |sum| over the band plus the quantisation term (quantisation(), added up over the samples)"""
    assert len(got) == len(want) == len(quant), what
    for band, (x, y, q) in enumerate(zip(got, want, quant)):
        for f in COUNTS:
            assert np.array_equal(x[f], y[f]), f"{what}: band {band} {f}: {x[f].sum()} {y[f].sum()}"
        for f in SUMMED:
            scale = float(np.max(np.abs(y[f])))
            allowed = bound * scale + q[f]
            err = np.abs(x[f] - y[f])
            k = int(np.argmax(err - allowed))
            print(f"{what}: band {band} {f} off by {err.max() / max(scale, 1e-300):.3e} of the largest |sum| {scale:.3e}, quantisation {q[f].max():.3e}")
            assert np.all(np.isfinite(x[f])) and np.all(err <= allowed), \
                f"{what}: band {band} {f} bin {k}: {x[f][k]!r} against {y[f][k]!r}, allowed {allowed[k]:.3e}"


def assert_identical(a, b, what, head=True):
    """two lists of sums, one dict per band: every field byte for byte, and the sample window"""
    assert len(a) == len(b), what
    for band, (x, y) in enumerate(zip(a, b)):
        for f in FIELDS:
            assert np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), f"{what}: band {band} {f}"
        if head:
            assert (x["n_samples"], x["t_first"], x["t_last"]) == (y["n_samples"], y["t_first"], y["t_last"]), f"{what}: band {band} window"


def add_sums(a, b):
    """the fields of two lists of sums (one dict per band) added"""
    return [{f: x[f] + y[f] for f in FIELDS} for x, y in zip(a, b)]


def linear_field(prm, parts, a=0.3, b=1.7, c=-0.4):
    """parts with u = (a + b y, c y) on the fluid and the same field on the wall particles: G = (0, b, 0, c) everywhere"""
    nf = parts["n_fluid"]
    y = parts["pos"][:, 1]
    field = np.asfortranarray(np.column_stack([a + b * y, c * y]))
    vel = field.copy(order="F")
    vel[nf:] = 0.0
    wall_vel = field.copy(order="F")
    wall_vel[:nf] = 0.0
    return dict(parts, vel=vel, wall_vel=wall_vel), (0.0, b, 0.0, c)
