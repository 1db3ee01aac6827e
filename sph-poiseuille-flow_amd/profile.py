"""Velocity-profile monitors and the L2 metric.

compute_binned_profile_mean / compute_mid_channel_profile: SPH_Poiseuille.m:579-605.
final_profile: SPH_Poiseuille.m:617-623.  l2_error: SPH_Poiseuille_postprocess.m:37-42.
flow_stats_profile: the sums of the device's flow statistics (include/sphx.h section 2a) as a profile.
pool_flow_stats: the sums of several channels (the members of a batch, section 2c) as one ensemble-averaged profile.
shepard_field: one sample of the device's field map (include/sphx.h section 2e) in numpy; field_map_means: its sums as a map.
pool_field_maps: the planes of several channels (the members of a batch, section 2g) as one ensemble-averaged map.
poiseuille_startup: the series solution of the start-up of plane Poiseuille flow from rest; profile_series_profiles: the
records of the device's profile series (include/sphx.h section 2j) as one profile per record.
pair_histogram: one sample of the device's pair statistics (include/sphx.h section 2l) in numpy, count for count;
pair_dist_profiles: its sums as g(r), the neighbour count and r_min; pool_pair_dist: the sums of several channels as one;
pair_histogram_part: the sample of one slab of a ring (the centres it owns against everything it holds).
velocity_gradients: the renormalised velocity-gradient estimate of the device's gradient statistics (include/sphx.h section 2n)
in numpy; grad_stats_sums: one binned sample; grad_stats_profiles: the sums as profiles; pool_grad_stats: several channels' as one;
grad_stats_sums_part: the sample of one slab of a ring (the particles it owns, estimated from everything it holds).
summation_density: the density of the device's density statistics (include/sphx.h section 2r) in numpy (fold=False: the open
window of a slab); dens_stats_sums: one binned sample; dens_stats_sums_part: the sample of one slab of a ring.
mode_sums: one sample of the device's mode amplitudes (include/sphx.h section 2t) in numpy, the definition; mode_scales: the
fixed-point scales of a sample; mode_b_exact: the sine coefficients of the start-up of plane Poiseuille flow, mode by mode.
"""
from __future__ import annotations

import numpy as np


def compute_binned_profile_mean(y_values, u_values, y_min, y_max, n_bins):
    y_values = np.asarray(y_values, dtype=np.float64).ravel()
    u_values = np.asarray(u_values, dtype=np.float64).ravel()
    edges = np.linspace(y_min, y_max, n_bins + 1)
    y_mid = 0.5 * (edges[:-1] + edges[1:])
    # discretize(): bin k holds edges[k] <= y < edges[k+1]; the last bin also holds y == edges[end]
    inside = (y_values >= edges[0]) & (y_values <= edges[-1])
    bin_id = np.searchsorted(edges, y_values[inside], side="right") - 1
    bin_id = np.minimum(bin_id, n_bins - 1)
    sum_u = np.bincount(bin_id, weights=u_values[inside], minlength=n_bins).astype(np.float64)
    cnt_u = np.bincount(bin_id, minlength=n_bins).astype(np.float64)
    u_mean = sum_u / np.maximum(cnt_u, 1.0)
    u_mean[cnt_u == 0] = np.nan
    return y_mid, u_mean


def compute_mid_channel_profile(pos, u_x, DL, DH, mid_x, half_width, n_bins):
    x_wrap = np.mod(pos[:, 0], DL)
    dx_mid = np.abs(x_wrap - mid_x)
    dx_mid = np.minimum(dx_mid, DL - dx_mid)
    is_mid = dx_mid <= half_width
    if not np.any(is_mid):
        return compute_binned_profile_mean([], [], 0.0, DH, n_bins)
    return compute_binned_profile_mean(pos[is_mid, 1], u_x[is_mid], 0.0, DH, n_bins)


def n_profile_bins(DH, dp):
    """SPH_Poiseuille.m:234."""
    return max(20, int(np.floor(DH / dp + 0.5)))


def final_profile(pos_fluid, vel_x_fluid, prm):
    n_bins = n_profile_bins(prm.DH, prm.dp)
    y_mid, u_mean = compute_binned_profile_mean(pos_fluid[:, 1], vel_x_fluid, 0.0, prm.DH, n_bins)
    u_exact = prm.gravity_g / (2.0 * prm.nu) * y_mid * (prm.DH - y_mid)
    return y_mid, u_mean, u_exact


def l2_error(u_mean, u_exact):
    valid = ~np.isnan(u_mean)
    if not np.any(valid):
        raise ValueError("velocity profile bins are all empty")
    return float(np.sqrt(np.sum((u_mean[valid] - u_exact[valid]) ** 2)
                         / max(np.sum(u_exact[valid] ** 2), np.finfo(np.float64).eps)))


def flow_stats_profile(DH, count, sum_ux, sum_ux2, sum_uy, sum_uy2, n_samples=0, t_first=np.nan, t_last=np.nan):
    """Per-bin sums over particle samples -> time-averaged profile.  Bins are those of compute_binned_profile_mean over
    [0, DH] (len(count) of them).  u_mean = sum u / N; u_std is the pooled spread of the particle samples in a bin,
    sqrt(max(sum u^2 / N - u_mean^2, 0)); bins without samples give NaN, as compute_binned_profile_mean does."""
    sums = [np.asarray(a, dtype=np.float64).ravel() for a in (count, sum_ux, sum_ux2, sum_uy, sum_uy2)]
    N, sx, sxx, sy, syy = sums
    n_bins = len(N)
    edges = np.linspace(0.0, DH, n_bins + 1)
    y_mid = 0.5 * (edges[:-1] + edges[1:])
    empty = N == 0
    Nd = np.where(empty, 1.0, N)

    def mean_std(s, ss):
        m = s / Nd
        sd = np.sqrt(np.maximum(ss / Nd - m * m, 0.0))
        m[empty] = np.nan
        sd[empty] = np.nan
        return m, sd

    u_mean, u_std = mean_std(sx, sxx)
    uy_mean, uy_std = mean_std(sy, syy)
    return dict(y_mid=y_mid, count=N, u_mean=u_mean, u_std=u_std, uy_mean=uy_mean, uy_std=uy_std,
                n_samples=int(n_samples), t_first=float(t_first), t_last=float(t_last),
                sum_ux=sx, sum_ux2=sxx, sum_uy=sy, sum_uy2=syy)


_SUMS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2")
STATS_FIELDS = _SUMS  # the five values per bin and band, in the order the library writes them


def profile_series_profiles(DH, sums):
    """The raw records of a profile series (capi.Context.profile_series_sums: the five STATS_FIELDS as [n_records, n_bands,
    n_bins] arrays of per-step sums, plus step, t, n_dropped, y_mid) -> one profile per record and band: u_mean, u_std,
    uy_mean, uy_std and count as [n_records, n_bands, n_bins] arrays by flow_stats_profile's rule applied per record (NaN
    where a bin is empty), plus step, t, n_dropped, y_mid."""
    N = np.asarray(sums["count"], dtype=np.float64)
    out = dict(step=sums["step"], t=sums["t"], n_dropped=int(sums["n_dropped"]), y_mid=sums["y_mid"], count=N)
    keys = ("u_mean", "u_std", "uy_mean", "uy_std")
    for k in keys:
        out[k] = np.full(N.shape, np.nan)
    for r in range(N.shape[0]):
        for b in range(N.shape[1]):
            prof = flow_stats_profile(DH, *[np.asarray(sums[f], dtype=np.float64)[r, b] for f in STATS_FIELDS])
            for k in keys:
                out[k][r, b] = prof[k]
    return out


def poiseuille_startup(y, t, g, nu, DH, n_terms=200):
    """The start-up of plane Poiseuille flow from rest under the body force g (Morris, Fox & Zhu 1997, eq. 21):
      u(y, t) = g / (2 nu) y (DH - y) - sum over odd n of 4 g DH^2 / (nu pi^3 n^3) sin(n pi y / DH) exp(-n^2 pi^2 nu t / DH^2)
    with the first n_terms odd n.  Broadcasts over y[:, None] and t[None, :]: -> [len(y), len(t)] (scalars: their shape)."""
    y, t = np.asarray(y, dtype=np.float64), np.asarray(t, dtype=np.float64)
    Y = y[:, None] if y.ndim == 1 and t.ndim == 1 else y
    T = t[None, :] if y.ndim == 1 and t.ndim == 1 else t
    u = g / (2.0 * nu) * Y * (DH - Y) + 0.0 * T
    for k in range(n_terms - 1, -1, -1):  # (small terms first)
        n = 2 * k + 1
        u = u - 4.0 * g * DH * DH / (nu * np.pi ** 3 * n ** 3) * np.sin(n * np.pi * Y / DH) * np.exp(-(n * np.pi / DH) ** 2 * nu * T)
    return u


def pool_flow_stats(DH, sums_list):
    """Ensemble- and time-averaged profile of several channels' flow-statistics sums (dicts as capi.Batch.flow_stats_sums
    returns, one per member): the per-bin sums are added in member order and turned into flow_stats_profile of the total;
    n_samples is the total over the members, t_first / t_last the earliest / latest sample.  Adds
      u_mean_se   per bin, the standard error across members of the members' own time-averaged u_mean,
                  std(ddof=1) / sqrt(M); NaN for M < 2 and in bins that are empty for some member
      n_members   M"""
    sums_list = list(sums_list)
    if not sums_list:
        raise ValueError("pool_flow_stats needs the sums of at least one member")
    per = [[np.asarray(s[k], dtype=np.float64).ravel() for k in _SUMS] for s in sums_list]
    total = [a.copy() for a in per[0]]
    for member in per[1:]:
        for k in range(len(_SUMS)):
            total[k] = total[k] + member[k]
    n_samples, t_first, t_last = _window(sums_list)
    out = flow_stats_profile(DH, *total, n_samples=n_samples, t_first=t_first, t_last=t_last)
    M = len(per)
    se = np.full(len(total[0]), np.nan)
    if M >= 2:
        means = np.stack([flow_stats_profile(DH, *member)["u_mean"] for member in per])
        ok = ~np.any(np.isnan(means), axis=0)
        se[ok] = np.std(means[:, ok], axis=0, ddof=1) / np.sqrt(M)
    out.update(u_mean_se=se, n_members=M)
    return out


def _window(sums_list):
    """n_samples in all, and the earliest t_first / latest t_last, of several channels' sums"""
    n_samples = sum(int(s.get("n_samples", 0)) for s in sums_list)
    t_first = [float(s.get("t_first", np.nan)) for s in sums_list]
    t_last = [float(s.get("t_last", np.nan)) for s in sums_list]
    return (n_samples, min((t for t in t_first if not np.isnan(t)), default=np.nan),
            max((t for t in t_last if not np.isnan(t)), default=np.nan))


def field_map_nodes(DL, DH, nx, ny):
    """The node coordinates of a field map (include/sphx.h section 2e): linspace over [0, DL] and [0, DH], ends included."""
    return np.linspace(0.0, DL, nx), np.linspace(0.0, DH, ny)


def _shepard_sums(X, Y, pos, vel, DL, h, chunk, mass=None):
    """S0 = sum W, S1 = sum W u_x, S2 = sum W u_y (and, with mass, Sm = sum m W) at the points (X, Y) over the rows of pos / vel:
    cubic spline of the physics, every particle within 2h, nearest image in x, no lower cut.  [3 or 4, len(X)]."""
    sigma, rcut2 = 10.0 / (7.0 * np.pi * h * h), (2.0 * h) * (2.0 * h)
    px, py, ux, uy = pos[:, 0], pos[:, 1], vel[:, 0], vel[:, 1]
    S = np.zeros((3 if mass is None else 4, len(X)))
    for a in range(0, len(X), chunk):
        dx = X[a:a + chunk, None] - px[None, :]
        dx -= DL * np.round(dx / DL)  # the nearest image (x in [0, DL): at most one period, the device's single fold)
        dy = Y[a:a + chunk, None] - py[None, :]
        r2 = dx * dx + dy * dy
        q = np.sqrt(r2) / h
        tq = 2.0 - q
        W = np.where(q < 1.0, sigma * (1.0 - 1.5 * q * q + 0.75 * q * q * q), sigma * 0.25 * tq * tq * tq)
        W = np.where(r2 < rcut2, W, 0.0)
        S[0, a:a + chunk] = W.sum(axis=1)
        S[1, a:a + chunk] = W @ ux
        S[2, a:a + chunk] = W @ uy
        if mass is not None:
            S[3, a:a + chunk] = W @ mass
    return S


def shepard_points(pos, vel, mass, DL, h, dp, points, wall_pos=None, wall_vel=None, chunk=2048):
    """One sample of the point probes of include/sphx.h section 2h, in numpy, at the points [P, 2] (x any finite value, folded
    into [0, DL)): the Shepard sums of shepard_field at arbitrary points plus Sm = sum m_j W_j.  pos / vel / mass: the fluid
    rows; wall_pos / wall_vel: wall rows that enter S0, S1 and S2 (with_walls) -- never Sm, the summation density from the
    fluid, which within 2h of a wall lacks the wall's share.
    Returns points [P, 2] as folded, S0, weight = S0 dp^2, u_x = S1 / S0, u_y = S2 / S0, rho = Sm as [P] arrays; where
    S0 == 0 the velocities are NaN and weight = rho = 0.  The oracle of the device kernel and the host route for a state
    that never was on the device."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    pts = np.array(points, dtype=np.float64).reshape(-1, 2)
    f = pts[:, 0] - np.floor(pts[:, 0] / DL) * DL
    pts[:, 0] = np.where((f >= 0.0) & (f < DL), f, 0.0)
    if wall_pos is not None:
        pos = np.concatenate([pos, np.asarray(wall_pos, dtype=np.float64)])
        vel = np.concatenate([vel, np.asarray(wall_vel, dtype=np.float64)])
        mass = np.concatenate([mass, np.zeros(len(pos) - len(mass))])
    S = _shepard_sums(pts[:, 0], pts[:, 1], pos, vel, DL, h, chunk, mass)
    hit = S[0] > 0.0
    safe = np.where(hit, S[0], 1.0)
    return dict(points=pts, S0=S[0], weight=np.where(hit, S[0] * (dp * dp), 0.0), u_x=np.where(hit, S[1] / safe, np.nan),
                u_y=np.where(hit, S[2] / safe, np.nan), rho=np.where(hit, S[3], 0.0))


def shepard_field(pos, vel, DL, DH, h, nx, ny, wall_pos=None, wall_vel=None, chunk=2048, nodes=None):
    """One sample of the field map of include/sphx.h section 2e, in numpy: Shepard interpolation of vel onto the nx x ny
    nodes with the cubic spline of the physics over every particle within 2h (minimum image in x -- the nearest image
    only -- and no lower cut).  pos / vel: the fluid rows [n x 2]; wall_pos / wall_vel: wall rows that enter the same sums
    (with_walls).  Chunked over nodes (chunk x n distances at a time).
    Returns x [nx], y [ny] and S0 = sum W, S1 = sum W u_x, S2 = sum W u_y, u_x = S1 / S0, u_y = S2 / S0 (NaN where S0 == 0)
    as [ny, nx] arrays -- or, with nodes = flat node indices i * ny + k, as 1-D arrays over just those nodes.  The oracle of
    the device kernel and the host route to a map of a final state that never was on the device."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    if wall_pos is not None:
        pos = np.concatenate([pos, np.asarray(wall_pos, dtype=np.float64)])
        vel = np.concatenate([vel, np.asarray(wall_vel, dtype=np.float64)])
    xs, ys = field_map_nodes(DL, DH, nx, ny)
    flat = np.arange(nx * ny) if nodes is None else np.asarray(nodes, dtype=np.int64)
    S = _shepard_sums(xs[flat // ny], ys[flat % ny], pos, vel, DL, h, chunk)
    hit = S[0] > 0.0
    safe = np.where(hit, S[0], 1.0)
    fields = dict(S0=S[0], S1=S[1], S2=S[2], u_x=np.where(hit, S[1] / safe, np.nan), u_y=np.where(hit, S[2] / safe, np.nan))
    if nodes is None:
        fields = {k: np.ascontiguousarray(v.reshape(nx, ny).T) for k, v in fields.items()}
    return dict(x=xs, y=ys, **fields)


FIELD_MAP_PLANES = ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")


def field_map_means(DL, DH, count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2, n_samples=0, t_first=np.nan, t_last=np.nan):
    """The six planes of a field map ([ny, nx] each) -> the time-averaged map: x, y, count, weight = sum_w / count (about 1
    inside the fluid), u_x, u_y = the mean of the per-sample Shepard values, u_x_std, u_y_std = their spread over the
    samples, sqrt(max(sum u^2 / N - mean^2, 0)); NaN where count == 0."""
    N, sw, sx, sy, sxx, syy = [np.asarray(a, dtype=np.float64) for a in (count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2)]
    ny, nx = N.shape
    xs, ys = field_map_nodes(DL, DH, nx, ny)
    empty = N == 0
    Nd = np.where(empty, 1.0, N)

    def mean_std(s, ss):
        m = s / Nd
        sd = np.sqrt(np.maximum(ss / Nd - m * m, 0.0))
        m[empty] = np.nan
        sd[empty] = np.nan
        return m, sd

    u_x, u_x_std = mean_std(sx, sxx)
    u_y, u_y_std = mean_std(sy, syy)
    weight = sw / Nd
    weight[empty] = np.nan
    return dict(x=xs, y=ys, count=N, weight=weight, u_x=u_x, u_y=u_y, u_x_std=u_x_std, u_y_std=u_y_std,
                n_samples=int(n_samples), t_first=float(t_first), t_last=float(t_last))


def pool_field_maps(DL, DH, sums_list):
    """Ensemble- and time-averaged map of several channels' field-map planes (dicts as capi.Batch.field_map_sums returns, one
    per member, all of one shape): the six planes are added in member order and turned into field_map_means of the total;
    n_samples is the total over the members, t_first / t_last the earliest / latest sample.  Adds
      u_x_se      per node, the standard error across members of the members' own time-averaged u_x,
                  std(ddof=1) / sqrt(M); NaN for M < 2 and at nodes some member never sampled
      n_members   M"""
    sums_list = list(sums_list)
    if not sums_list:
        raise ValueError("pool_field_maps needs the planes of at least one member")
    per = [[np.asarray(s[k], dtype=np.float64) for k in FIELD_MAP_PLANES] for s in sums_list]
    total = [a.copy() for a in per[0]]
    for member in per[1:]:
        for k in range(len(FIELD_MAP_PLANES)):
            total[k] = total[k] + member[k]
    n_samples, t_first, t_last = _window(sums_list)
    out = field_map_means(DL, DH, *total, n_samples=n_samples, t_first=t_first, t_last=t_last)
    M = len(per)
    se = np.full(total[0].shape, np.nan)
    if M >= 2:
        means = np.stack([field_map_means(DL, DH, *member)["u_x"] for member in per])
        ok = ~np.any(np.isnan(means), axis=0)
        se[ok] = np.std(means[:, ok], axis=0, ddof=1) / np.sqrt(M)
    out.update(u_x_se=se, n_members=M)
    return out


# ---- pair statistics (include/sphx.h sections 2l, 2m) ----

def pair_edges(r_max, n_bins):
    """(r_edges, e2): the n_bins + 1 bin edges in r and the squared edges the comparisons use: e2[k] = (k * (r_max / n_bins))^2
    for k < n_bins, e2[n_bins] = r_max * r_max."""
    e = np.arange(n_bins, dtype=np.float64) * (r_max / n_bins)
    return np.append(e, r_max), np.append(e * e, r_max * r_max)


def in_band(x, DL, x_centre, half_width):
    """compute_mid_channel_profile's membership (stats_in_band on the device)."""
    d = np.abs(np.mod(x, DL) - x_centre)
    return np.minimum(d, DL - d) <= half_width


def pair_separations(pos, DL, r_max, wall_pos=None, chunk=512):
    """Every ordered pair (i, j != i) of the fluid particles pos [n, 2] with r2 < r_max^2, and every (fluid i, wall j) pair of
    wall_pos: dict(i_ff, r2_ff, i_fw, r2_fw), i the centre's index.  dx = x_i - x_j folded by the minimum image (dx > DL/2 ->
    dx - DL, dx < -DL/2 -> dx + DL), dy = y_i - y_j, r2 = dx*dx + dy*dy: the doubles the device computes.  Chunked over centres
    sorted by x; a chunk meets only the partners whose x lies within r_max of its own range (a superset: the exact test is r2)."""
    pos = np.asarray(pos, dtype=np.float64)
    rmax2 = r_max * r_max
    half = DL / 2
    margin = r_max * (1.0 + 1e-9) + 1e-12 * DL

    def sweep(partners, same):
        px = np.mod(partners[:, 0], DL)
        order_p = np.argsort(px, kind="stable")
        pxs = px[order_p]
        cx = np.mod(pos[:, 0], DL)
        order_c = np.argsort(cx, kind="stable")
        out_i, out_r2 = [], []
        for a in range(0, len(order_c), chunk):
            ci = order_c[a:a + chunk]
            lo, hi = cx[ci[0]] - margin, cx[ci[-1]] + margin
            if hi - lo >= DL:
                cand = order_p
            else:
                parts = [order_p[np.searchsorted(pxs, lo, "left"):np.searchsorted(pxs, hi, "right")]]
                if lo < 0.0:
                    parts.append(order_p[np.searchsorted(pxs, lo + DL, "left"):])
                if hi > DL:
                    parts.append(order_p[:np.searchsorted(pxs, hi - DL, "right")])
                cand = np.unique(np.concatenate(parts))
            dx = pos[ci, 0][:, None] - partners[cand, 0][None, :]
            dx = np.where(dx > half, dx - DL, np.where(dx < -half, dx + DL, dx))
            dy = pos[ci, 1][:, None] - partners[cand, 1][None, :]
            r2 = dx * dx + dy * dy
            keep = r2 < rmax2
            if same:
                keep &= ci[:, None] != cand[None, :]
            rows, cols = np.nonzero(keep)
            out_i.append(ci[rows])
            out_r2.append(r2[rows, cols])
        if not out_i:
            return np.zeros(0, dtype=np.int64), np.zeros(0)
        return np.concatenate(out_i).astype(np.int64), np.concatenate(out_r2)

    i_ff, r2_ff = sweep(pos, True)
    if wall_pos is not None and len(wall_pos):
        i_fw, r2_fw = sweep(np.asarray(wall_pos, dtype=np.float64), False)
    else:
        i_fw, r2_fw = np.zeros(0, dtype=np.int64), np.zeros(0)
    return dict(i_ff=i_ff, r2_ff=r2_ff, i_fw=i_fw, r2_fw=r2_fw, r_max=float(r_max))


def pair_histogram(pos, DL, DH, r_max, n_bins, bands=(), y_margin=0.0, wall_pos=None, separations=None):
    """One sample of the pair statistics of include/sphx.h section 2l in numpy -- the oracle of k_pair_dist.  pos [n, 2]: the
    fluid particles; bands: [(x_centre, half_width), ...]; wall_pos: the wall particles, or None for no wall histogram.  -> one
    dict per band (band 0: the whole channel): r_edges [n_bins + 1], ff, fw [n_bins] (int64; ordered pairs, a pair of two
    centres counts twice), centres, r2_min (the smallest counted fluid-fluid r2, +inf without a pair) and r_min = sqrt(r2_min).
    Bin k holds e2[k] <= r2 < e2[k+1] (pair_edges): searchsorted(e2, r2, side="right") - 1; r2 >= r_max^2 is not counted.
    separations: pair_separations(pos, DL, R, wall_pos) of an R >= r_max, to share the pair search between calls."""
    pos = np.asarray(pos, dtype=np.float64)
    r_edges, e2 = pair_edges(r_max, n_bins)
    sep = separations if separations is not None else pair_separations(pos, DL, r_max, wall_pos)
    assert sep["r_max"] >= r_max
    centre = (pos[:, 1] >= y_margin) & (pos[:, 1] <= DH - y_margin)
    members = [centre] + [centre & in_band(pos[:, 0], DL, x, hw) for x, hw in bands]
    out = []
    for mine in members:
        d = dict(r_edges=r_edges, centres=int(np.count_nonzero(mine)))
        for kind in ("ff", "fw"):
            i, r2 = sep["i_" + kind], sep["r2_" + kind]
            if wall_pos is None and kind == "fw":
                i, r2 = i[:0], r2[:0]
            take = mine[i] & (r2 < e2[-1])
            k = np.searchsorted(e2, r2[take], side="right") - 1
            d[kind] = np.bincount(k, minlength=n_bins).astype(np.int64)
            if kind == "ff":
                d["r2_min"] = float(np.min(r2[take])) if np.any(take) else np.inf
        d["r_min"] = float(np.sqrt(d["r2_min"]))
        out.append(d)
    return out


def pair_histogram_part(pos, owned, DL, DH, r_max, n_bins, bands=(), y_margin=0.0, wall_pos=None):
    """One sample of a SLAB's pair statistics (include/sphx.h section 3a) in numpy -- the oracle of k_pair_dist_s.  pos [n, 2]:
    every fluid particle the slab holds, in the slab's own frame (its halo copies at x - DL or x + DL where they come from
    across the seam); owned [n] bool: the rows it owns.  The CENTRES are the owned rows with y_margin <= y <= DH - y_margin,
    the PARTNERS all the other rows and, with wall_pos, the wall particles the slab holds; dx = x_i - x_j as it stands, with no
    fold: the window is open.  Bands go by in_band, whose mod brings x < 0 and x >= DL back.  -> pair_histogram's list of dicts,
    the slab's partial sums: slab.pool_ring_pair_dist of the ranks' gives the channel's."""
    pos = np.asarray(pos, dtype=np.float64)
    own = np.flatnonzero(np.asarray(owned, dtype=bool))
    r_edges, e2 = pair_edges(r_max, n_bins)
    walls = None if wall_pos is None else np.asarray(wall_pos, dtype=np.float64).reshape(-1, 2)
    centre = (pos[own, 1] >= y_margin) & (pos[own, 1] <= DH - y_margin)
    members = [centre] + [centre & in_band(pos[own, 0], DL, x, hw) for x, hw in bands]

    def separations(partners, same, chunk=256):
        """(row of `own`, r2) of every counted pair"""
        rows, r2s = [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
        for a in range(0, len(own), chunk):
            ci = own[a:a + chunk]
            dx = pos[ci, 0][:, None] - partners[None, :, 0]
            dy = pos[ci, 1][:, None] - partners[None, :, 1]
            r2 = dx * dx + dy * dy
            keep = r2 < e2[-1]
            if same:
                keep &= ci[:, None] != np.arange(len(partners))[None, :]
            i, j = np.nonzero(keep)
            rows.append(a + i)
            r2s.append(r2[i, j])
        return np.concatenate(rows), np.concatenate(r2s)

    sep = dict(ff=separations(pos, True), fw=separations(walls, False) if walls is not None and len(walls) else separations(pos[:0], False))
    out = []
    for mine in members:
        d = dict(r_edges=r_edges, centres=int(np.count_nonzero(mine)))
        for kind in ("ff", "fw"):
            i, r2 = sep[kind]
            take = mine[i]
            k = np.searchsorted(e2, r2[take], side="right") - 1
            d[kind] = np.bincount(k, minlength=n_bins).astype(np.int64)
            if kind == "ff":
                d["r2_min"] = float(np.min(r2[take])) if np.any(take) else np.inf
        d["r_min"] = float(np.sqrt(d["r2_min"]))
        out.append(d)
    return out


def pair_dist_profiles(sums, dp):
    """The sums of one band (capi.Context.pair_dist_sums()[band], pair_histogram(...)[band]) as figures: r_mid, the radial
    distribution function g = ff / (centres * pi (e_{k+1}^2 - e_k^2) / dp^2) -- ordered pairs per centre over the particles an
    ideal lattice of spacing dp puts into the ring --, g_wall the same of fw, n_neigh = sum(ff) / centres and r_min; NaN without
    a centre."""
    e = np.asarray(sums["r_edges"], dtype=np.float64)
    ff, fw = np.asarray(sums["ff"], dtype=np.float64), np.asarray(sums["fw"], dtype=np.float64)
    c = float(sums["centres"])
    ring = np.pi * (e[1:] ** 2 - e[:-1] ** 2) / (dp * dp)
    norm = c * ring if c > 0 else np.full(len(ff), np.nan)
    return dict(r_mid=0.5 * (e[:-1] + e[1:]), g=ff / norm, g_wall=fw / norm, n_neigh=float(ff.sum() / c) if c > 0 else float("nan"),
                r_min=float(sums["r_min"]))


def pool_pair_dist(sums_list):
    """The sums of the same band of several channels (the members of a batch or of an ensemble) as one: the integers added,
    the smallest r_min, all samples (n_samples added, the window from the first t_first to the last t_last).  A list of lists
    (one list of bands per channel, what capi.Batch.pair_dist_sums returns) is pooled band by band."""
    sums_list = list(sums_list)
    assert sums_list, "nothing to pool"
    if isinstance(sums_list[0], (list, tuple)):
        return [pool_pair_dist([s[b] for s in sums_list]) for b in range(len(sums_list[0]))]
    first = sums_list[0]
    assert all(np.array_equal(s["r_edges"], first["r_edges"]) for s in sums_list), "the channels have different bins"
    r2 = min(float(s["r2_min"]) for s in sums_list)
    out = dict(r_edges=np.asarray(first["r_edges"]), ff=sum(np.asarray(s["ff"], dtype=np.int64) for s in sums_list),
               fw=sum(np.asarray(s["fw"], dtype=np.int64) for s in sums_list), centres=int(sum(int(s["centres"]) for s in sums_list)),
               r2_min=r2, r_min=float(np.sqrt(r2)))
    if all("n_samples" in s for s in sums_list):
        sampled = [s for s in sums_list if s["n_samples"] > 0]
        out.update(n_samples=int(sum(s["n_samples"] for s in sums_list)),
                   t_first=min((s["t_first"] for s in sampled), default=float("nan")),
                   t_last=max((s["t_last"] for s in sampled), default=float("nan")))
    return out


# ---- gradient statistics (include/sphx.h sections 2n, 2o) ----

# the twelve values per bin and band, in the order the library writes them
GRAD_FIELDS = ("count", "sum_gxx", "sum_gxy", "sum_gyx", "sum_gyy", "sum_gxx2", "sum_gxy2", "sum_gyx2", "sum_gyy2", "sum_div2",
               "sum_vort2", "skipped")
GRAD_COMPONENTS = ("gxx", "gxy", "gyx", "gyy")  # G_ab = d u_a / d x_b
GRAD_MAX_BINS = 640


def velocity_gradients(pos, vel, vol, DL, h, wall_pos=None, wall_vel=None, wall_vol=None, chunk=512, acc=np.float64, reverse=False,
                       fold=True):
    """The velocity gradient at every fluid particle by the renormalised estimator of include/sphx.h section 2n, in numpy -- the
    definition k_grad_stats is tested against.  pos, vel [n, 2]: the fluid particles; vol: their volumes V_j = mass_j / rho0 (an
    array [n] or one number); wall_pos, wall_vel [m, 2] and wall_vol [m]: wall particles that are partners too, with these
    velocities, or None.  Over every partner j != i with 1e-24 < r2 < (2h)^2, nearest image in x:
        d = r_i - r_j,  w_j = V_j W'(|d|) / |d|,  M_i = - sum w_j d (x) d,  A_i = sum w_j (v_j - v_i) (x) d,  G_i = A_i M_i^-1
    -> dict(G [n, 4]: g_xx, g_xy, g_yx, g_yy with G_ab = d u_a / d x_b, NaN where det M_i == 0; det [n]: det M_i).
    Chunked over particles sorted by x, a chunk against the partners within 2h of its x-range.  acc / reverse exist for the tests alone: the type the
    per-particle sums are accumulated in and whether the partners are added in reversed order, which together measure the
    rounding error of these sums (tests/grad_stats_cases.py); no caller in the package sets them.  fold=False: the OPEN window of
    a slab of a ring (grad_stats_sums_part) -- x is taken as it stands, dx = x_i - x_j with no nearest image, and DL is not used."""
    pos, vel = np.asarray(pos, dtype=np.float64).reshape(-1, 2), np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    n = len(pos)
    vol = np.broadcast_to(np.asarray(vol, dtype=np.float64), (n,))
    sigma_h, rcut2, half = 10.0 / (7.0 * np.pi * h * h) / h, (2.0 * h) * (2.0 * h), DL / 2
    margin = 2.0 * h * (1.0 + 1e-9) + 1e-12 * DL
    S = np.zeros((7, n), dtype=acc)  # m11, m12, m22, a11, a12, a21, a22
    cx = np.mod(pos[:, 0], DL) if fold else pos[:, 0]
    order_c = np.argsort(cx, kind="stable")

    def sweep(p_pos, p_vel, p_vol, same):
        px = np.mod(p_pos[:, 0], DL) if fold else p_pos[:, 0]
        order_p = np.argsort(px, kind="stable")
        pxs = px[order_p]
        for a in range(0, n, chunk):
            ci = order_c[a:a + chunk]
            lo, hi = cx[ci[0]] - margin, cx[ci[-1]] + margin
            if not fold:
                cand = np.sort(order_p[np.searchsorted(pxs, lo, "left"):np.searchsorted(pxs, hi, "right")])
            elif hi - lo >= DL:
                cand = np.sort(order_p)
            else:
                parts = [order_p[np.searchsorted(pxs, lo, "left"):np.searchsorted(pxs, hi, "right")]]
                if lo < 0.0:
                    parts.append(order_p[np.searchsorted(pxs, lo + DL, "left"):])
                if hi > DL:
                    parts.append(order_p[:np.searchsorted(pxs, hi - DL, "right")])
                cand = np.unique(np.concatenate(parts))
            if reverse:
                cand = cand[::-1]
            dx = pos[ci, 0][:, None] - p_pos[cand, 0][None, :]
            if fold:
                dx = np.where(dx > half, dx - DL, np.where(dx < -half, dx + DL, dx))
            dy = pos[ci, 1][:, None] - p_pos[cand, 1][None, :]
            r2 = dx * dx + dy * dy
            keep = (r2 > 1e-24) & (r2 < rcut2)
            if same:
                keep &= ci[:, None] != cand[None, :]
            r = np.sqrt(np.where(keep, r2, 1.0))
            q = r / h
            dW = np.where(q < 1.0, sigma_h * (-3.0 * q + 2.25 * q * q), -sigma_h * 0.75 * (2.0 - q) * (2.0 - q))
            w = np.where(keep, p_vol[cand][None, :] * dW / r, 0.0)
            dvx = p_vel[cand, 0][None, :] - vel[ci, 0][:, None]
            dvy = p_vel[cand, 1][None, :] - vel[ci, 1][:, None]
            wx, wy = w * dx, w * dy
            for k, term in enumerate((-wx * dx, -wx * dy, -wy * dy, dvx * wx, dvx * wy, dvy * wx, dvy * wy)):
                S[k, ci] += term.astype(acc, copy=False).sum(axis=1)

    sweep(pos, vel, vol, True)
    if wall_pos is not None and len(wall_pos):
        wall_pos = np.asarray(wall_pos, dtype=np.float64).reshape(-1, 2)
        sweep(wall_pos, np.asarray(wall_vel, dtype=np.float64).reshape(-1, 2),
              np.broadcast_to(np.asarray(wall_vol, dtype=np.float64), (len(wall_pos),)), False)
    m11, m12, m22, a11, a12, a21, a22 = S
    det = m11 * m22 - m12 * m12
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        G = np.stack([(a11 * m22 - a12 * m12) * inv, (a12 * m11 - a11 * m12) * inv, (a21 * m22 - a22 * m12) * inv,
                      (a22 * m11 - a21 * m12) * inv], axis=1)
    return dict(G=G.astype(np.float64), det=det.astype(np.float64))


def grad_scales(vmax, h, n):
    """The fixed-point scales of one sample of the gradient statistics, as the device picks them: with n <= 2^L particles and
    the bound 2^e > max(16 vmax / h, 2^-60), a component is summed in units of 2^-s1, its square of 2^-s2, div^2 and vort^2 of
    2^-s3: s1 = 62 - L - e, s2 = 62 - L - 2e, s3 = 60 - L - 2e.  -> dict(s1, s2, s3, bound)."""
    L = 0
    while L < 31 and (1 << L) < n:
        L += 1
    x = 16.0 * float(vmax) / h
    e = int(np.frexp(x if x > 2.0 ** -60 else 2.0 ** -60)[1])  # (a NaN vmax leaves the floor)
    return dict(s1=62 - L - e, s2=62 - L - 2 * e, s3=60 - L - 2 * e, bound=float(np.ldexp(1.0, e)))


def grad_stats_sums(pos, vel, vol, DL, DH, h, n_bins, bands=(), det_min=0.05, wall_pos=None, wall_vel=None, wall_vol=None, vmax=None,
                    gradients=None, quantise=False):
    """One sample of the gradient statistics of include/sphx.h section 2n in numpy -- the oracle of k_grad_stats: the estimate
    of velocity_gradients binned with the flow statistics' rules (compute_binned_profile_mean's bins over [0, DH], y outside
    dropped; band 0 the whole channel, bands [(x_centre, half_width), ...] by in_band).  A particle with det M <= det_min, a
    component that is not finite or one above the bound of grad_scales(vmax, h, n) is counted in `skipped`, not summed; vmax:
    the clock's max |v| (None: that of vel).  -> one dict of the GRAD_FIELDS as [n_bins] arrays per band.  gradients: the
    result of velocity_gradients of the same state, to share it between calls.  quantise (set by the tests alone; no caller in
    the package sets it): every particle's terms are rounded to the device's fixed-point grid before they are added (a component to 2^-s1, a square to 2^-s2, div^2 and vort^2 to 2^-s3 of
    grad_scales), as k_grad_stats rounds them: the sums are then the device's up to the rounding of the estimate itself, and
    a value far below the quantum -- the 1e-16 a symmetric lattice leaves in g_xx -- is the exact zero the device records."""
    pos, vel = np.asarray(pos, dtype=np.float64).reshape(-1, 2), np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    g = gradients if gradients is not None else velocity_gradients(pos, vel, vol, DL, h, wall_pos, wall_vel, wall_vol)
    return _grad_stats_binned(pos, vel, g, None, DL, DH, h, n_bins, bands, det_min, vmax, quantise)


def _grad_stats_binned(pos, vel, g, rows, DL, DH, h, n_bins, bands, det_min, vmax, quantise):
    """the estimates g of the particles pos (rows: those that are binned, None: all of them) as one sample's sums per band; the
    scales are those of len(pos) particles"""
    G, det = g["G"], g["det"]
    if vmax is None:
        vmax = float(np.sqrt(np.max(np.sum(vel * vel, axis=1)))) if len(vel) else 0.0
    sc = grad_scales(vmax, h, len(pos))
    bound = sc["bound"]
    with np.errstate(invalid="ignore"):
        ok = (det > det_min) & np.all(np.abs(G) <= bound, axis=1)  # (a NaN or an infinity fails the comparison)
    edges = np.linspace(0.0, DH, n_bins + 1)
    inside = (pos[:, 1] >= edges[0]) & (pos[:, 1] <= edges[-1])
    if rows is not None:
        inside &= np.asarray(rows, dtype=bool)
    bin_id = np.minimum(np.searchsorted(edges, pos[:, 1], side="right") - 1, n_bins - 1)
    Gz = np.where(ok[:, None], G, 0.0)
    div, vort = Gz[:, 0] + Gz[:, 3], Gz[:, 2] - Gz[:, 1]
    values = [np.ones(len(pos))] + [Gz[:, k] for k in range(4)] + [Gz[:, k] * Gz[:, k] for k in range(4)] + [div * div, vort * vort]
    if quantise:
        shifts = [0] + [sc["s1"]] * 4 + [sc["s2"]] * 4 + [sc["s3"]] * 2
        values = [np.ldexp(np.rint(np.ldexp(v, k)), -k) for v, k in zip(values, shifts)]
    out = []
    for mine in [inside] + [inside & in_band(pos[:, 0], DL, x, hw) for x, hw in bands]:
        take, skip = mine & ok, mine & ~ok
        d = {f: np.bincount(bin_id[take], weights=v[take], minlength=n_bins).astype(np.float64) for f, v in zip(GRAD_FIELDS, values)}
        d["skipped"] = np.bincount(bin_id[skip], minlength=n_bins).astype(np.float64)
        out.append(d)
    return out


def grad_stats_sums_part(pos, vel, vol, owned, DL, DH, h, n_bins, bands=(), det_min=0.05, wall_pos=None, wall_vel=None, wall_vol=None,
                         vmax=None, quantise=False):
    """One sample of a SLAB's gradient statistics (include/sphx.h section 3a) in numpy -- the oracle of k_grad_stats_s.  pos, vel
    [n, 2] and vol: every fluid particle the slab holds, in the slab's own frame (its halo copies at x - DL or x + DL where they
    come from across the seam); owned [n] bool: the rows it bins.  The estimate of an owned row takes every other row and, where
    given, the wall particles the slab holds as partners, with dx = x_i - x_j as it stands and no fold: the window is open
    (velocity_gradients(fold=False)).  Bands go by in_band, whose mod brings x < 0 and x >= DL back.  The scales are those of the
    n rows HELD (grad_scales(vmax, h, n)) and vmax is the ring's (None: that of vel, which is the slab's own).  -> grad_stats_sums'
    list of dicts, the slab's partial sums: slab.pool_ring_grad_stats of the ranks' gives the channel's."""
    pos, vel = np.asarray(pos, dtype=np.float64).reshape(-1, 2), np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    g = velocity_gradients(pos, vel, vol, DL, h, wall_pos, wall_vel, wall_vol, fold=False)
    return _grad_stats_binned(pos, vel, g, owned, DL, DH, h, n_bins, bands, det_min, vmax, quantise)


def grad_stats_profiles(DH, sums):
    """The sums of one band (capi.Context.grad_stats_sums(band), grad_stats_sums(...)[band]) as profiles: y_mid, count, skipped
    and per bin the mean and the standard deviation of each component over the particle samples (gxx_mean, gxx_std, ...,
    sqrt(max(sum g^2 / N - mean^2, 0))), div_rms = sqrt(sum div^2 / N), vort_mean = (sum g_yx - sum g_xy) / N and vort_rms;
    NaN where a bin has no sample.  n_samples, t_first and t_last are handed on where the sums have them."""
    s = {f: np.asarray(sums[f], dtype=np.float64).ravel() for f in GRAD_FIELDS}
    N = s["count"]
    n_bins = len(N)
    edges = np.linspace(0.0, DH, n_bins + 1)
    empty = N == 0
    Nd = np.where(empty, 1.0, N)
    out = dict(y_mid=0.5 * (edges[:-1] + edges[1:]), count=N, skipped=s["skipped"])
    for c in GRAD_COMPONENTS:
        m = s["sum_" + c] / Nd
        sd = np.sqrt(np.maximum(s["sum_" + c + "2"] / Nd - m * m, 0.0))
        out[c + "_mean"], out[c + "_std"] = np.where(empty, np.nan, m), np.where(empty, np.nan, sd)
    out["div_rms"] = np.where(empty, np.nan, np.sqrt(s["sum_div2"] / Nd))
    out["vort_mean"] = np.where(empty, np.nan, (s["sum_gyx"] - s["sum_gxy"]) / Nd)
    out["vort_rms"] = np.where(empty, np.nan, np.sqrt(s["sum_vort2"] / Nd))
    for k in ("n_samples", "t_first", "t_last"):
        if k in sums:
            out[k] = sums[k]
    return out


def pool_grad_stats(DH, sums_list):
    """The sums of the same band of several channels (the members of a batch or of an ensemble) as one profile: the GRAD_FIELDS
    added in member order and turned into grad_stats_profiles of the total (with the total's sums beside it); n_samples is the
    total over the members, t_first / t_last the earliest / latest sample; n_members = M."""
    sums_list = list(sums_list)
    if not sums_list:
        raise ValueError("pool_grad_stats needs the sums of at least one member")
    total = {f: np.asarray(sums_list[0][f], dtype=np.float64).ravel().copy() for f in GRAD_FIELDS}
    for member in sums_list[1:]:
        for f in GRAD_FIELDS:
            total[f] = total[f] + np.asarray(member[f], dtype=np.float64).ravel()
    n_samples, t_first, t_last = _window(sums_list)
    total.update(n_samples=n_samples, t_first=t_first, t_last=t_last)
    out = grad_stats_profiles(DH, total)
    out.update({f: total[f] for f in GRAD_FIELDS}, n_members=len(sums_list))
    return out


# ---- particle tracers (include/sphx.h sections 2p / 2q): the Lagrangian view ----
TRACER_FIELDS = ("x", "y", "u_x", "u_y")  # the four values per tracer and record, in the order the library writes them


def tracer_rows(pos, vel, ids):
    """The definition of a tracer record: x, y, u_x, u_y [T] of the rows `ids` of a downloaded state (pos, vel [n, 2]), copied."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64).ravel()
    return dict(x=pos[ids, 0].copy(), y=pos[ids, 1].copy(), u_x=vel[ids, 0].copy(), u_y=vel[ids, 1].copy())


def unwrap_tracers(tr, DL):
    """A copy of the tracers dict tr (capi.tracers_dict: t [n], x, u_x [n, T]) with x_unwrapped [n, T]: record 0 as it is, then
    the image x + k DL of each x nearest to x_prev + 0.5 (u_prev + u) (t - t_prev), the trapezoidal prediction from the record
    before.  k DL is added once to the recorded x, so the result is the exact unwrapped position wherever that is
    representable.  Raises ValueError when |u_x| (t - t_prev) >= DL / 2 for any tracer and record: the series is then too
    coarse for the nearest image to be the right one."""
    t = np.asarray(tr["t"], dtype=np.float64)
    x, u = np.asarray(tr["x"], dtype=np.float64), np.asarray(tr["u_x"], dtype=np.float64)
    if x.ndim != 2 or x.shape != u.shape or len(t) != len(x):
        raise ValueError("unwrap_tracers: t [n] and x, u_x [n, T] expected")
    xu = x.copy()
    if len(t) > 1:
        dt = np.diff(t)[:, None]
        if np.any(dt < 0.0):
            raise ValueError("unwrap_tracers: t must not decrease")
        far = np.maximum(np.abs(u[1:]), np.abs(u[:-1])) * dt
        if np.any(~(far < 0.5 * DL)):
            r, k = np.argwhere(~(far < 0.5 * DL))[0]
            raise ValueError(f"unwrap_tracers: the series is too coarse to unwrap: tracer {int(k)} moves {float(far[r, k]):.4g} between "
                             f"records {int(r)} and {int(r) + 1}, DL / 2 is {0.5 * DL:.4g}")
        for r in range(1, len(t)):
            pred = xu[r - 1] + 0.5 * (u[r - 1] + u[r]) * dt[r - 1]
            xu[r] = x[r] + np.round((pred - x[r]) / DL) * DL
    return dict(tr, x_unwrapped=xu)


def poiseuille_u(y, g, nu, DH):
    """The analytic steady profile u(y) = g / (2 nu) y (DH - y)."""
    y = np.asarray(y, dtype=np.float64)
    return g / (2.0 * nu) * y * (DH - y)


def tracer_profiles(tr, DL, DH, g, nu, lags=None, y_margin=0.0):
    """The Lagrangian figures of a tracers dict, over the tracers whose first recorded y lies at least y_margin from both walls:
    lags [L] (in records; default 1, 2, 4, ... up to a quarter of the series), tau [L] (the mean time span of a lag), msd_y [L]
    (mean square of y(r + lag) - y(r) over the tracers and the origins r = 0, lag, 2 lag, ...: windows that do not overlap),
    msd_x_rel [L] (the same of the unwrapped x displacement minus u_exact(y(r)) * (t(r + lag) - t(r))), D_y (half the
    least-squares slope of msd_y against tau; one lag: msd_y / (2 tau)), y_drift (the mean of (y_last - y_first) / (t_last -
    t_first)), u_dev_rms (the r.m.s. of u_x - u_exact(y) along the paths, in units of |U_max| = |g| DH^2 / (8 nu)), n_tracers,
    n_records.  In laminar Poiseuille flow every one of them is zero for the exact solution."""
    t = np.asarray(tr["t"], dtype=np.float64)
    keep = (np.asarray(tr["y"], dtype=np.float64)[0] >= y_margin) & (np.asarray(tr["y"], dtype=np.float64)[0] <= DH - y_margin) \
        if len(t) else np.zeros(np.asarray(tr["y"]).shape[1:], dtype=bool)
    R = len(t)
    if R < 2 or not np.any(keep):
        raise ValueError("tracer_profiles needs at least two records and one tracer inside the margins")
    xu = np.asarray(tr["x_unwrapped"] if "x_unwrapped" in tr else unwrap_tracers(tr, DL)["x_unwrapped"], dtype=np.float64)[:, keep]
    y, u = np.asarray(tr["y"], dtype=np.float64)[:, keep], np.asarray(tr["u_x"], dtype=np.float64)[:, keep]
    if lags is None:
        lags = [1]
        while 2 * lags[-1] <= max((R - 1) // 4, 1):
            lags.append(2 * lags[-1])
    lags = np.asarray(lags, dtype=np.int64).ravel()
    if len(lags) < 1 or np.any(lags < 1) or np.any(lags > R - 1):
        raise ValueError("tracer_profiles: lags must be record counts in 1 .. n_records - 1")
    tau, msd_y, msd_x = np.zeros(len(lags)), np.zeros(len(lags)), np.zeros(len(lags))
    for j, lag in enumerate(lags):
        r0 = np.arange(0, R - lag, lag)
        span = (t[r0 + lag] - t[r0])[:, None]
        dy = y[r0 + lag] - y[r0]
        dx = xu[r0 + lag] - xu[r0] - poiseuille_u(y[r0], g, nu, DH) * span
        tau[j], msd_y[j], msd_x[j] = float(np.mean(span)), float(np.mean(dy * dy)), float(np.mean(dx * dx))
    D_y = 0.5 * float(np.polyfit(tau, msd_y, 1)[0]) if len(lags) > 1 else 0.5 * msd_y[0] / tau[0]
    U_max = abs(g) * DH * DH / (8.0 * nu)
    dev = u - poiseuille_u(y, g, nu, DH)
    return dict(lags=lags, tau=tau, msd_y=msd_y, msd_x_rel=msd_x, D_y=D_y, y_drift=float(np.mean((y[-1] - y[0]) / (t[-1] - t[0]))),
                u_dev_rms=float(np.sqrt(np.mean(dev * dev))) / U_max, n_tracers=int(np.count_nonzero(keep)), n_records=R)


def pool_tracers(tr_list):
    """The tracer series of several channels (the members of an ensemble) as one: the columns of every member side by side, in
    member order -- x, y, u_x, u_y (and x_unwrapped where every member has it) [n, M T], ids [M T] and member [M T], the member a
    column came from.  The members must have recorded the same ids at the same steps and times: ValueError otherwise."""
    tr_list = list(tr_list)
    if not tr_list:
        raise ValueError("pool_tracers needs the series of at least one member")
    first = tr_list[0]
    for m, tr in enumerate(tr_list[1:], 1):
        for k in ("ids", "step", "t"):
            if not np.array_equal(np.asarray(tr[k]), np.asarray(first[k])):
                raise ValueError(f"pool_tracers: member {m} differs from member 0 in {k}")
    T = len(np.asarray(first["ids"]).ravel())
    fields = TRACER_FIELDS + (("x_unwrapped",) if all("x_unwrapped" in tr for tr in tr_list) else ())
    out = dict(ids=np.tile(np.asarray(first["ids"]).ravel(), len(tr_list)), member=np.repeat(np.arange(len(tr_list)), T),
               step=np.asarray(first["step"]).copy(), t=np.asarray(first["t"], dtype=np.float64).copy())
    out.update({k: np.concatenate([np.asarray(tr[k], dtype=np.float64).reshape(len(out["t"]), T) for tr in tr_list], axis=1) for k in fields})
    out.update(n_dropped=int(sum(tr.get("n_dropped", 0) for tr in tr_list)), n_missing=int(sum(tr.get("n_missing", 0) for tr in tr_list)),
               n_members=len(tr_list))
    return out


# ---- density statistics (include/sphx.h sections 2r, 2s, 3a): the state of compression ----

# the eight values per bin and band, in the order the library writes them; the first six add up over samples and channels
DENS_FIELDS = ("count", "sum_d", "sum_d2", "sum_dvol", "sum_wall", "outliers", "d_min", "d_max")
DENS_SUMS = DENS_FIELDS[:6]
DENS_MAX_HIST = 1024
DENS_MAX_WORDS = 7680  # (n_bands + 1) * (8 * n_bins + n_hist + 2): the 60 KB of LDS of a workgroup


def summation_density(pos, mass, DL, h, rho0, inv_sigma0, wall_pos=None, wall_vol=None, chunk=512, acc=np.float64, reverse=False,
                      fold=True):
    """The summation density of every fluid particle as the step's first pass computes it, in numpy -- the definition
    k_dens_stats is tested against (include/sphx.h section 2r).  pos [n, 2] and mass [n] (or one number): the fluid particles;
    wall_pos [m, 2] and wall_vol [m]: the wall particles and their volumes, or None.  Over every fluid partner j != i and every
    wall particle with 1e-24 < r2 < (2h)^2, nearest image in x:
        s_in = W(0) + sum W(r_ij),  s_ct = sum W(r_ij) V_j,  rho_i = s_in rho0 inv_sigma0 + s_ct rho0^2 inv_sigma0 / mass_i
    and rho_i = rho0 where that is <= 1e-12 (the step's floor).  -> rho [n], wall [n] = s_ct rho0 inv_sigma0 / mass_i, the walls'
    share of rho_i / rho0.  Chunked over particles sorted by x, a chunk against the partners within 2h of its x-range.  acc /
    reverse exist for the tests alone: the type the per-particle sums are accumulated in and whether the partners are added in
    reversed order, which together measure the rounding error of these sums (tests/dens_stats_cases.py); no caller in the
    package sets them.  fold=False: the OPEN window of a slab of a ring (dens_stats_sums_part) -- x is taken as it stands, dx =
    x_i - x_j with no nearest image, and DL is not used."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    n = len(pos)
    mass = np.broadcast_to(np.asarray(mass, dtype=np.float64), (n,))
    sigma, rcut2, half = 10.0 / (7.0 * np.pi * h * h), (2.0 * h) * (2.0 * h), DL / 2
    margin = 2.0 * h * (1.0 + 1e-9) + 1e-12 * DL
    S = np.zeros((2, n), dtype=acc)  # s_in without W(0), s_ct
    cx = np.mod(pos[:, 0], DL) if fold else pos[:, 0]
    order_c = np.argsort(cx, kind="stable")

    def sweep(p_pos, p_vol, same, row):
        px = np.mod(p_pos[:, 0], DL) if fold else p_pos[:, 0]
        order_p = np.argsort(px, kind="stable")
        pxs = px[order_p]
        for a in range(0, n, chunk):
            ci = order_c[a:a + chunk]
            lo, hi = cx[ci[0]] - margin, cx[ci[-1]] + margin
            if not fold:
                cand = np.sort(order_p[np.searchsorted(pxs, lo, "left"):np.searchsorted(pxs, hi, "right")])
            elif hi - lo >= DL:
                cand = np.sort(order_p)
            else:
                parts = [order_p[np.searchsorted(pxs, lo, "left"):np.searchsorted(pxs, hi, "right")]]
                if lo < 0.0:
                    parts.append(order_p[np.searchsorted(pxs, lo + DL, "left"):])
                if hi > DL:
                    parts.append(order_p[:np.searchsorted(pxs, hi - DL, "right")])
                cand = np.unique(np.concatenate(parts))
            if reverse:
                cand = cand[::-1]
            dx = pos[ci, 0][:, None] - p_pos[cand, 0][None, :]
            if fold:
                dx = np.where(dx > half, dx - DL, np.where(dx < -half, dx + DL, dx))
            dy = pos[ci, 1][:, None] - p_pos[cand, 1][None, :]
            r2 = dx * dx + dy * dy
            keep = (r2 > 1e-24) & (r2 < rcut2)
            if same:
                keep &= ci[:, None] != cand[None, :]
            q = np.sqrt(np.where(keep, r2, 1.0)) / h
            tq = 2.0 - q
            W = np.where(q < 1.0, sigma * (1.0 - 1.5 * q * q + 0.75 * q * q * q), sigma * 0.25 * tq * tq * tq)
            term = np.where(keep, W if p_vol is None else W * p_vol[cand][None, :], 0.0)
            S[row, ci] += term.astype(acc, copy=False).sum(axis=1)

    sweep(pos, None, True, 0)
    if wall_pos is not None and len(wall_pos):
        wall_pos = np.asarray(wall_pos, dtype=np.float64).reshape(-1, 2)
        sweep(wall_pos, np.broadcast_to(np.asarray(wall_vol, dtype=np.float64), (len(wall_pos),)), False, 1)
    s_in, s_ct = S[0] + acc(sigma), S[1]
    wall = s_ct * acc(rho0) * acc(inv_sigma0) / mass.astype(acc)
    rho = s_in * acc(rho0) * acc(inv_sigma0) + wall * acc(rho0)
    rho = np.where(rho <= 1e-12, acc(rho0), rho)
    return rho.astype(np.float64), wall.astype(np.float64)


def dens_scales(delta_bound, n):
    """The fixed-point scales of one sample of the density statistics, as the device picks them: with n <= 2^L particles and
    2^e >= delta_bound (e <= -1 for delta_bound <= 0.5), delta is summed in units of 2^-s_d, delta^2 of 2^-s_d2, dvol of 2^-s_dvol,
    wall of 2^-s_wall: s_d = 62 - L - e, s_d2 = 62 - L - 2e, s_dvol = 61 - L - e, s_wall = 61 - L.  -> dict(s_d, s_d2, s_dvol,
    s_wall, e)."""
    L = 0
    while L < 31 and (1 << L) < n:
        L += 1
    m, e = np.frexp(float(delta_bound))
    e = int(e) - 1 if m == 0.5 else int(e)
    return dict(s_d=62 - L - e, s_d2=62 - L - 2 * e, s_dvol=61 - L - e, s_wall=61 - L, e=e)


def dens_hist_bin(delta, n_hist, hist_range):
    """The histogram word of every delta: 0 .. n_hist - 1 the bin floor((delta + hist_range) * (n_hist / (2 hist_range))) of
    [-hist_range, hist_range), n_hist: below, n_hist + 1: above -- in the device's operation order."""
    delta = np.asarray(delta, dtype=np.float64)
    scale = float(n_hist) / (2.0 * hist_range)
    k = np.clip(np.floor((delta + hist_range) * scale), 0, n_hist - 1).astype(np.int64)
    return np.where(delta < -hist_range, n_hist, np.where(delta >= hist_range, n_hist + 1, k))


def dens_stats_sums(pos, mass, DL, DH, h, rho0, inv_sigma0, n_bins, bands=(), n_hist=64, hist_range=0.05, delta_bound=0.5,
                    wall_pos=None, wall_vol=None, density=None, quantise=False):
    """One sample of the density statistics of include/sphx.h section 2r in numpy -- the oracle of k_dens_stats: delta = rho /
    rho0 - 1, dvol = rho0 / rho - 1 and wall of summation_density binned with the flow statistics' rules
    (compute_binned_profile_mean's bins over [0, DH], y outside dropped; band 0 the whole channel, bands [(x_centre,
    half_width), ...] by in_band).  A particle with |delta| > delta_bound or a delta that is not finite is counted in
    `outliers`, summed nowhere and in no histogram.  -> per band one dict of the DENS_FIELDS as [n_bins] arrays (d_min / d_max:
    +inf / -inf in an empty bin), hist [n_hist] int64, below, above.  density: (rho, wall) of the same state -- from
    summation_density, or from a download's mass / Vol -- to share it between calls.  quantise (set by the tests alone; no
    caller in the package sets it): every particle's terms are rounded to the device's fixed-point grid of dens_scales before
    they are added, as k_dens_stats rounds them."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    rho, wall = density if density is not None else summation_density(pos, mass, DL, h, rho0, inv_sigma0, wall_pos, wall_vol)
    return _dens_stats_binned(pos, rho, wall, None, DL, DH, rho0, n_bins, bands, n_hist, hist_range, delta_bound, quantise)


def _dens_stats_binned(pos, rho, wall, rows, DL, DH, rho0, n_bins, bands, n_hist, hist_range, delta_bound, quantise):
    """the densities (rho, wall) of the particles pos (rows: those that are binned, None: all of them) as one sample's sums per
    band; the scales are those of len(pos) particles"""
    n = len(pos)
    rho, wall = np.asarray(rho, dtype=np.float64), np.asarray(wall, dtype=np.float64)
    delta = rho / rho0 - 1.0
    with np.errstate(invalid="ignore"):
        ok = np.abs(delta) <= delta_bound  # (a NaN or an infinity fails the comparison)
    dz = np.where(ok, delta, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dvol = np.where(ok, rho0 / rho - 1.0, 0.0)
    values = [np.ones(n), dz, dz * dz, dvol, np.where(ok, wall, 0.0)]
    if quantise:
        sc = dens_scales(delta_bound, n)
        shifts = [0, sc["s_d"], sc["s_d2"], sc["s_dvol"], sc["s_wall"]]
        values = [np.ldexp(np.rint(np.ldexp(v, k)), -k) for v, k in zip(values, shifts)]
    edges = np.linspace(0.0, DH, n_bins + 1)
    inside = (pos[:, 1] >= edges[0]) & (pos[:, 1] <= edges[-1])
    if rows is not None:
        inside &= np.asarray(rows, dtype=bool)
    bin_id = np.minimum(np.searchsorted(edges, pos[:, 1], side="right") - 1, n_bins - 1)
    word = dens_hist_bin(dz, n_hist, hist_range)
    out = []
    for mine in [inside] + [inside & in_band(pos[:, 0], DL, x, hw) for x, hw in bands]:
        take, skip = mine & ok, mine & ~ok
        d = {f: np.bincount(bin_id[take], weights=v[take], minlength=n_bins).astype(np.float64) for f, v in zip(DENS_SUMS, values)}
        d["outliers"] = np.bincount(bin_id[skip], minlength=n_bins).astype(np.float64)
        d_min, d_max = np.full(n_bins, np.inf), np.full(n_bins, -np.inf)
        np.minimum.at(d_min, bin_id[take], delta[take])
        np.maximum.at(d_max, bin_id[take], delta[take])
        h_all = np.bincount(word[take], minlength=n_hist + 2).astype(np.int64)
        d.update(d_min=d_min, d_max=d_max, hist=h_all[:n_hist], below=int(h_all[n_hist]), above=int(h_all[n_hist + 1]))
        out.append(d)
    return out


def dens_stats_sums_part(pos, mass, owned, DL, DH, h, rho0, inv_sigma0, n_bins, bands=(), n_hist=64, hist_range=0.05, delta_bound=0.5,
                         wall_pos=None, wall_vol=None, quantise=False):
    """One sample of a SLAB's density statistics (include/sphx.h section 3a) in numpy -- the oracle of k_dens_stats_s.  pos [n, 2]
    and mass: every fluid particle the slab holds, in the slab's own frame (its halo copies at x - DL or x + DL where they come
    from across the seam); owned [n] bool: the rows it bins.  The density of an owned row takes every other row and the wall
    particles the slab holds (wall_pos, wall_vol, in the same frame) as partners, with dx = x_i - x_j as it stands and no fold:
    the window is open (summation_density(fold=False)).  Bands go by in_band, whose mod brings x < 0 and x >= DL back.  The
    scales are those of the n rows HELD (dens_scales(delta_bound, n)).  -> dens_stats_sums' list of dicts, the slab's partial
    sums: slab.pool_ring_dens_stats of the ranks' gives the channel's."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    rho, wall = summation_density(pos, mass, DL, h, rho0, inv_sigma0, wall_pos, wall_vol, fold=False)
    return _dens_stats_binned(pos, rho, wall, owned, DL, DH, rho0, n_bins, bands, n_hist, hist_range, delta_bound, quantise)


def add_dens_stats(a, b):
    """The sums of two samples, or of the same band of two channels, as one: the DENS_SUMS, the histogram, below and above added
    (a first), the smaller d_min and the larger d_max."""
    out = {f: np.asarray(a[f], dtype=np.float64) + np.asarray(b[f], dtype=np.float64) for f in DENS_SUMS}
    out.update(d_min=np.minimum(a["d_min"], b["d_min"]), d_max=np.maximum(a["d_max"], b["d_max"]),
               hist=np.asarray(a["hist"], dtype=np.int64) + np.asarray(b["hist"], dtype=np.int64),
               below=int(a["below"]) + int(b["below"]), above=int(a["above"]) + int(b["above"]))
    return out


def dens_stats_profiles(DH, p0, sums, hist_range=None):
    """The sums of one band (capi.Context.dens_stats_sums(band), dens_stats_sums(...)[band]) as profiles: y_mid, count, outliers
    and per bin d_mean and d_std (sqrt(max(sum delta^2 / N - mean^2, 0))) of delta = rho / rho0 - 1 over the particle samples,
    d_min, d_max, the pressure p_mean = p0 d_mean and p_std = p0 d_std, wall_mean (the walls' share of rho / rho0) and packing =
    1 + sum dvol / N (the mean of rho0 / rho: the area the particles claim over the area they were given); NaN where a bin has
    no sample.  hist_density: the band's histogram as a probability density over delta, hist / (N_band * bin width) with N_band
    = sum(hist) + below + above, at hist_centres (hist_range: the sums' own where they carry it); NaN without a particle.
    n_samples, t_first and t_last are handed on where the sums have them."""
    s = {f: np.asarray(sums[f], dtype=np.float64).ravel() for f in DENS_FIELDS}
    N = s["count"]
    n_bins = len(N)
    edges = np.linspace(0.0, DH, n_bins + 1)
    empty = N == 0
    Nd = np.where(empty, 1.0, N)
    mean = s["sum_d"] / Nd
    sd = np.sqrt(np.maximum(s["sum_d2"] / Nd - mean * mean, 0.0))
    nan = np.nan
    out = dict(y_mid=0.5 * (edges[:-1] + edges[1:]), count=N, outliers=s["outliers"],
               d_mean=np.where(empty, nan, mean), d_std=np.where(empty, nan, sd),
               d_min=np.where(empty, nan, s["d_min"]), d_max=np.where(empty, nan, s["d_max"]),
               p_mean=np.where(empty, nan, p0 * mean), p_std=np.where(empty, nan, p0 * sd),
               wall_mean=np.where(empty, nan, s["sum_wall"] / Nd), packing=np.where(empty, nan, 1.0 + s["sum_dvol"] / Nd))
    hist = np.asarray(sums["hist"], dtype=np.float64).ravel()
    hist_range = sums.get("hist_range") if hist_range is None else hist_range
    if hist_range is not None:
        width = 2.0 * float(hist_range) / len(hist)
        total = float(hist.sum()) + float(sums["below"]) + float(sums["above"])
        out["hist_centres"] = -float(hist_range) + width * (np.arange(len(hist)) + 0.5)
        out["hist_density"] = hist / (total * width) if total > 0 else np.full(len(hist), nan)
    for k in ("n_samples", "t_first", "t_last"):
        if k in sums:
            out[k] = sums[k]
    return out


def pool_dens_stats(DH, p0, sums_list, hist_range=None):
    """The sums of the same band of several channels (the members of a batch or of an ensemble) as one profile: the DENS_SUMS, the
    histogram, below and above added in member order, the smallest d_min and the largest d_max, turned into dens_stats_profiles
    of the total (with the total's sums beside it); n_samples is the total over the members, t_first / t_last the earliest /
    latest sample; n_members = M."""
    sums_list = list(sums_list)
    if not sums_list:
        raise ValueError("pool_dens_stats needs the sums of at least one member")
    first = sums_list[0]
    total = {f: np.array(first[f], dtype=np.float64).ravel() for f in DENS_FIELDS}
    total.update(hist=np.array(first["hist"], dtype=np.int64).ravel(), below=int(first["below"]), above=int(first["above"]))
    for member in sums_list[1:]:
        total = add_dens_stats(total, member)
    n_samples, t_first, t_last = _window(sums_list)
    total.update(n_samples=n_samples, t_first=t_first, t_last=t_last)
    if hist_range is None:
        hist_range = sums_list[0].get("hist_range")
    if hist_range is not None:
        total["hist_range"] = hist_range
    out = dens_stats_profiles(DH, p0, total)
    out.update({f: total[f] for f in DENS_FIELDS}, hist=total["hist"], below=total["below"], above=total["above"], n_members=len(sums_list))
    return out


# the fields and bases of a mode (include/sphx.h section 2t), in the order of the last axes of a record
MODE_FIELDS = ("n", "ux", "uy")
MODE_BASES = ("cc", "sc", "cs", "ss")


def mode_sums(pos, vel, DL, DH, mx, ny, acc=np.float64):
    """One sample of the device's mode amplitudes (include/sphx.h section 2t) in numpy -- the definition: for the fluid rows
    pos / vel [N, 2], thx = 2 pi x / DL and thy = pi y / DH, and for 0 <= m <= mx, 0 <= n <= ny
      S[m, n, f, k] = sum_i q_i basis_k(i),  q = 1, u_x, u_y,  basis = cos(m thx) cos(n thy), sin cos, cos sin, sin sin.
    -> dict of n, ux, uy as [mx + 1, ny + 1, 4] float64 arrays and abs_n, abs_ux, abs_uy, the sums of |q_i| a comparison is
    relative to (the sums themselves cancel to ~0 for most modes).  acc: the float type the terms are formed and added in."""
    pos, vel = np.asarray(pos, dtype=acc), np.asarray(vel, dtype=acc)
    two, pi = acc(2.0), np.arccos(acc(-1.0))
    thx = two * pi * pos[:, 0] / acc(DL)
    thy = pi * pos[:, 1] / acc(DH)
    m = np.arange(mx + 1, dtype=acc)[:, None]
    n = np.arange(ny + 1, dtype=acc)[:, None]
    bx = (np.cos(m * thx[None, :]), np.sin(m * thx[None, :]))  # [mx + 1, N] each
    by = (np.cos(n * thy[None, :]), np.sin(n * thy[None, :]))  # [ny + 1, N]
    q = dict(n=np.ones(len(pos), dtype=acc), ux=vel[:, 0], uy=vel[:, 1])
    out = {}
    for f in MODE_FIELDS:
        S = np.zeros((mx + 1, ny + 1, len(MODE_BASES)), dtype=acc)
        for k, (ix, iy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            S[:, :, k] = (bx[ix] * q[f][None, :]) @ by[iy].T
        out[f] = S.astype(np.float64)
        out["abs_" + f] = float(np.abs(q[f]).sum())
    return out


def mode_scales(vmax, n):
    """The fixed-point scales of one sample of the mode amplitudes, as the device picks them: with n <= 2^L particles and the
    bound 2^e > max(2 vmax, 2^-60), the field n is summed in units of 2^-s0, ux and uy of 2^-s1: s0 = 62 - L, s1 = 62 - L - e.
    -> dict(s0, s1, bound)."""
    L = 0
    while L < 31 and (1 << L) < n:
        L += 1
    x = 2.0 * float(vmax)
    e = int(np.frexp(x if x > 2.0 ** -60 else 2.0 ** -60)[1])  # (a NaN vmax leaves the floor)
    return dict(s0=62 - L, s1=62 - L - e, bound=float(np.ldexp(1.0, e)))


def mode_b_exact(n, t, g, nu, DH):
    """The sine coefficient b_n(t) of u_x of the start-up of plane Poiseuille flow from rest (poiseuille_startup, term by
    term): b_n(inf) (1 - exp(-nu n^2 pi^2 t / DH^2)) with b_n(inf) = 32 U_max / (n pi)^3 = 4 g DH^2 / (nu pi^3 n^3) for odd n,
    0 for even n.  Broadcasts over n and t."""
    n, t = np.asarray(n, dtype=np.float64), np.asarray(t, dtype=np.float64)
    b_inf = np.where(n % 2 == 1, 4.0 * g * DH * DH / (nu * np.pi ** 3 * np.maximum(n, 1.0) ** 3), 0.0)
    return b_inf * (1.0 - np.exp(-nu * (n * np.pi / DH) ** 2 * t))
