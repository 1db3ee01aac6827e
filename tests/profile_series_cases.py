"""Cases, numpy binning and comparisons shared by tests/test_profile_series_host.py, tests/test_gpu_profile_series.py and
tests/test_gpu_batch_profile_series.py (profile series, include/sphx.h sections 2j / 2k)."""
import numpy as np

FIELDS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2")
SERIES = ("step", "t") + FIELDS

# name: (dp, DL, context options, make_case options) -- the flow statistics' cases, each for a path of the kernel or the step
CASES = {
    "dp05_auto": (0.05, 3.0, dict(), dict()),                          # 1 200 fluid particles: one workgroup, no ticket
    "dp01_multi": (0.01, 3.0, dict(), dict()),                         # 30 k particles: global int64 sums + ticket
    "dp025_walk": (0.025, 1.5, dict(lanes_per_particle=4), dict()),    # the large-channel ("_w") kernels
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1), dict()),        # the device-decided schedule
    "dp025_dual": (0.025, 1.5, dict(lanes_per_particle=16, dual_rate=2), dict()),
    "leftward": (0.05, 3.0, dict(), dict(U_bulk=-0.666667)),           # g < 0: negative sums, the wrap at x < 0
}


def case(maker, cfgmod, geom, name, seed=11):
    """(prm, parts, context options) of CASES[name] from helpers.make_case"""
    dp, DL, kw, mk = CASES[name]
    prm, parts = maker(cfgmod, geom, **dict(dict(dp=dp, DL=DL, jitter=0.2, seed=seed, developed=True), **mk))
    return prm, parts, kw


def bands(prm):
    hw = max(prm.dp, prm.h)
    return [(0.5 * prm.DL, hw), (0.0, hw)]  # mid-channel and the periodic seam


def numpy_sums(pos, vel, prm, n_bins, band=None):
    """the five sums of one band of the fluid rows pos / vel in numpy: the reference's bins (linspace edges, discretize),
    compute_mid_channel_profile's band membership"""
    x, y, ux, uy = pos[:, 0], pos[:, 1], vel[:, 0], vel[:, 1]
    if band is not None:
        xw = np.mod(x, prm.DL)
        d = np.abs(xw - band[0])
        d = np.minimum(d, prm.DL - d)
        sel = d <= band[1]
        y, ux, uy = y[sel], ux[sel], uy[sel]
    edges = np.linspace(0.0, prm.DH, n_bins + 1)
    inside = (y >= edges[0]) & (y <= edges[-1])
    k = np.minimum(np.searchsorted(edges, y[inside], side="right") - 1, n_bins - 1)
    ux, uy = ux[inside], uy[inside]
    return dict(zip(FIELDS, [np.bincount(k, weights=w, minlength=n_bins).astype(np.float64)
                             for w in (np.ones_like(ux), ux, ux * ux, uy, uy * uy)]))


def assert_record_matches(series, r, b, want, what):
    """record r, band b of a raw series against numpy_sums: counts exactly, sums within 1e-12 of the band's largest |sum| (the
    flow statistics' bound: the device sums exactly in fixed point with a quantum of 2^-(62 - L - e) of max|v|, numpy in
    floating point with up to n roundings of 1.1e-16 -- tests/test_gpu_flow_stats.py)"""
    assert np.array_equal(series["count"][r, b], want["count"]), f"{what}: counts"
    scale = max(max(float(np.max(np.abs(want[f]))) for f in FIELDS[1:]), 1e-300)
    for f in FIELDS[1:]:
        err = float(np.max(np.abs(series[f][r, b] - want[f])))
        assert err <= 1e-12 * scale, f"{what}: {f} off by {err / scale:.3e} of the largest |sum|"


def assert_series_identical(a, b, what, counters=True):
    """two raw series bit for bit: step, t and the five fields, and (counters) n_dropped"""
    for k in SERIES:
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape, f"{what}: {k} {np.asarray(a[k]).shape} {np.asarray(b[k]).shape}"
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"
    if counters:
        assert a["n_dropped"] == b["n_dropped"], what


def running_sums(series, band):
    """the records of one band added in order, one by one, in float64 (not np.sum, which adds pairwise): what the flow
    statistics' running sums hold after the same samples"""
    out = {}
    for f in FIELDS:
        total = np.zeros(series[f].shape[2])
        for r in range(series[f].shape[0]):
            total = total + series[f][r, band]
        out[f] = total
    return out


def synthetic_series(profmod, prm, times, n_bins=20, n_bands=2, count=10.0, empty=()):
    """A series as capi.Context.profile_series returns it whose u_mean IS poiseuille_startup at the bin centres, in every band,
    with `count` particles per bin; the bins of `empty` hold nothing (count 0, NaN means)."""
    t = np.asarray(times, dtype=np.float64)
    edges = np.linspace(0.0, prm.DH, n_bins + 1)
    y = 0.5 * (edges[:-1] + edges[1:])
    u = profmod.poiseuille_startup(y, t, prm.gravity_g, prm.nu, prm.DH).T           # [n, n_bins]
    u_mean = np.repeat(u[:, None, :], n_bands, axis=1)
    cnt = np.full(u_mean.shape, float(count))
    for k in empty:
        u_mean[:, :, k] = np.nan
        cnt[:, :, k] = 0.0
    zeros = np.where(np.isnan(u_mean), np.nan, 0.0)
    return dict(step=np.arange(1, len(t) + 1, dtype=np.int64), t=t, y_mid=y, count=cnt, u_mean=u_mean, u_std=zeros.copy(),
                uy_mean=zeros.copy(), uy_std=zeros.copy(), n_dropped=0)
