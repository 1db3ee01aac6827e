"""Host driver -- the time loop of SPH_Poiseuille.m S5-S7 on top of libsphx.

Two engines with the same observable behaviour:
  * engine="resident" (default): state lives in HBM in a sphx context; every inner-while of
    SPH_Poiseuille.m:250-292 is one sphx_ctx_advance call, the host only acts at output points
    (:294-301) and for the every-20-steps log line (:285-291, opt-in).
  * engine="mex": the reference's own call sequence, six MEX-surface calls per step through
    mex_surface.py (:254-281) -- kept to show that the per-call surface is a drop-in.
Restart / post-process files (:127-163,:295,:305-306) go through restart.py; the plots (S7) are out of scope.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from . import capi
from .geometry import init_particles
from .mex_surface import sph_neighbor_search_mex, sph_physics_shell_mex
from . import restart
from .profile import (compute_mid_channel_profile, dens_stats_profiles, mode_b_exact, field_map_means, final_profile, flow_stats_profile,
                      grad_stats_profiles, l2_error, n_profile_bins, pool_dens_stats, pool_field_maps, pair_dist_profiles,
                      pool_flow_stats, pool_grad_stats, pool_pair_dist,
                      poiseuille_startup, pool_tracers, profile_series_profiles, tracer_profiles, unwrap_tracers)


@dataclass
class RunResult:
    prm: object
    n_fluid: int
    n_total: int
    t: float
    steps: int
    wall_seconds: float
    pos: np.ndarray
    vel: np.ndarray
    y_mid: np.ndarray
    u_mean: np.ndarray
    u_exact: np.ndarray
    L2_error: float
    profile_times: list = field(default_factory=list)
    mid_profile_u: list = field(default_factory=list)
    tau_bottom: float = 0.0
    tau_top: float = 0.0
    tau_target: float = 0.0
    grid_policy: dict = field(default_factory=dict)  # resident engine: rebuild interval, skin, forced rebuilds
    full_profile_u: list = field(default_factory=list)  # whole-channel binned u_x(y) at every output point
    n_inner: int = 1  # inner sub-steps per counted step (> 1 only with the opt-in dual-rate loop)
    time_avg: dict = None  # run(..., average_from=...): device-side time-averaged profiles and figures (see time_average)
    history: dict = None  # run(..., history_every=...): the device-side step history of the whole run (capi.Context.history)
    field_avg: dict = None  # run(..., field_from=...): the device-side time-averaged velocity map (capi.Context.field_map); a
                            # member of run_ensemble / run_sweep(..., field_from=...): its own (capi.Batch.field_map)
    probes: dict = None  # run / run_sweep(..., probe_points=...): the device-side point-probe series of the whole run
                         # (capi.Context.probes; probe_figures() turns it into means, RMS and spectral peaks)

    profile_series: dict = None  # run / run_sweep(..., profiles_every=...): the device-side profile series of the whole run
                                 # (capi.Context.profile_series; profile_series_figures() compares it with the start-up solution)

    pair_dist: list = None  # run / run_sweep / run_ensemble(..., pairs_from=...): the device-side pair statistics of the run, one
                            # dict per band (capi.Context.pair_dist: the integer sums with g, n_neigh, r_min; pair_dist_figures())

    grad_stats: list = None  # run / run_sweep / run_ensemble(..., gradients_from=...): the device-side gradient statistics of the
                             # run, one dict per band (capi.Context.grad_stats: the sums with the profiles; grad_figures())

    tracers: dict = None  # run / run_sweep / run_ensemble(..., tracers=...): the device-side tracer series of the whole run
                          # (capi.Context.tracers: x, y, u_x, u_y of the tracked fluid rows per record; tracer_figures())

    dens_stats: list = None  # run / run_sweep / run_ensemble(..., density_from=...): the device-side density statistics of the
                             # run, one dict per band (capi.Context.dens_stats: the sums with the profiles; density_figures())

    modes: dict = None  # run / run_sweep(..., modes_every=...): the device-side mode amplitudes of the whole run
                        # (capi.Context.modes: n, ux, uy per record and mode; mode_figures())

    def L2_time_mean(self, last=5):
        """L2 of the whole-channel profile averaged over the last `last` output points: the instantaneous profile of
        one chaotic realisation wanders by ~0.1 pp around its mean, the average does not."""
        u = np.nanmean(np.stack(self.full_profile_u[-last:]), axis=0)
        return l2_error(u, self.u_exact)

    @property
    def particle_steps_per_s(self):
        return self.n_total * self.steps / max(self.wall_seconds, 1e-30)


def verlet_time_step(vel_fluid, c_max, h, nu, gravity_g, remain):
    """SPH_Poiseuille.m:519-527 (used by the 'mex' engine; the resident engine does this on device)."""
    v_max = float(np.max(np.sqrt(vel_fluid[:, 0] ** 2 + vel_fluid[:, 1] ** 2))) if len(vel_fluid) else 0.0
    dt_acoustic = 0.25 * h / max(c_max + v_max, 1e-12)
    dt_viscous = 0.125 * h * h / max(nu, 1e-12)
    dt_body = 0.25 * np.sqrt(h / max(abs(gravity_g), 1e-12))
    return max(min(dt_acoustic, dt_viscous, dt_body, remain), 1e-12)


def periodic_bounding(pos, n_fluid, DL):
    """SPH_Poiseuille.m:570-577."""
    x = pos[:n_fluid, 0]
    pos[:n_fluid, 0] = x - np.floor(x / DL) * DL
    return pos


def time_average(prm, whole, mid):
    """Figures of a time window from the device's flow statistics (capi.Context.flow_stats of band 0 / the mid band).
    U_max = g DH^2 / (8 nu), the centre-line speed of the analytic profile: signed, negative for a leftward flow; the rms
    and spread figures are magnitudes and are divided by |U_max|.
      profile, mid_profile   the whole-channel and mid-band flow_stats dicts (u_mean, u_std, ... per bin)
      u_exact, L2            analytic profile at the bin centres and l2_error of the time-averaged whole-channel u_mean
      uy_rms_over_umax       sqrt(sum over bins of sum u_y^2 / sum over bins of N) / |U_max| (all particle samples)
      ux_std_centre_over_umax  count-weighted RMS of the per-bin u_x spread u_std over the bins whose centres lie in
                             [0.4, 0.6] DH, sqrt(sum N u_std^2 / sum N), / |U_max|
      n_samples, t_first, t_last  the window actually sampled"""
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    y = whole["y_mid"]
    u_exact = prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y)
    N = whole["count"]
    n_all = float(np.sum(N))
    uy_rms = np.sqrt(np.sum(whole["sum_uy2"]) / n_all) if n_all > 0 else np.nan
    centre = (y >= 0.4 * prm.DH) & (y <= 0.6 * prm.DH) & (N > 0)
    n_c = float(np.sum(N[centre]))
    ux_sd = np.sqrt(np.sum(N[centre] * whole["u_std"][centre] ** 2) / n_c) if n_c > 0 else np.nan
    return dict(profile=whole, mid_profile=mid, y_mid=y, u_mean=whole["u_mean"], mid_u_mean=mid["u_mean"], u_exact=u_exact,
                L2=l2_error(whole["u_mean"], u_exact), uy_rms_over_umax=float(uy_rms / abs(u_max)),
                ux_std_centre_over_umax=float(ux_sd / abs(u_max)), U_max=u_max, n_samples=whole["n_samples"],
                t_first=whole["t_first"], t_last=whole["t_last"])


def history_figures(prm, hist, t_from=0.0, tol=0.05):
    """Figures of a step history (capi.Context.history / RunResult.history) against the analytic flow, on the host.
      tau_bottom_mean, tau_top_mean, u_bulk_mean   dt-weighted time means over the records with t >= t_from (a record
                             stands for the step that ended at its t, so its weight is its dt; NaN without such records)
      tau_target, u_bulk_exact   g rho0 DH / 2 and the analytic bulk velocity g DH^2 / (12 nu)
      tau_bottom_dev, tau_top_dev, u_bulk_dev   relative deviation of the means, (mean - exact) / exact
      t_settled              the first t from which |tau - tau_target| / tau_target of BOTH walls stays below tol up to
                             the last record (over all records, whatever t_from; NaN if the last record is outside)
      n_records              records that entered the means"""
    t, dt = np.asarray(hist["t"], dtype=np.float64), np.asarray(hist["dt"], dtype=np.float64)
    tau_target = prm.gravity_g * prm.rho0 * prm.DH / 2.0
    u_exact = prm.gravity_g * prm.DH ** 2 / (12.0 * prm.nu)
    sel = t >= t_from
    w = dt[sel]
    wsum = float(np.sum(w))

    def mean(key):  # (about the first value: a constant series gives that value exactly)
        v = np.asarray(hist[key], dtype=np.float64)[sel]
        return float(v[0] + np.sum(w * (v - v[0])) / wsum) if wsum > 0.0 else float("nan")

    out = dict(tau_target=tau_target, u_bulk_exact=u_exact, n_records=int(np.count_nonzero(sel)), tol=tol)
    for key, exact in (("tau_bottom", tau_target), ("tau_top", tau_target), ("u_bulk", u_exact)):
        out[key + "_mean"] = mean(key)
        out[key + "_dev"] = (out[key + "_mean"] - exact) / exact
    dev = np.maximum(np.abs(np.asarray(hist["tau_bottom"], dtype=np.float64) - tau_target),
                     np.abs(np.asarray(hist["tau_top"], dtype=np.float64) - tau_target)) / abs(tau_target)
    outside = np.flatnonzero(~(dev < tol))
    first_inside = 0 if len(outside) == 0 else int(outside[-1]) + 1
    out["t_settled"] = float(t[first_inside]) if first_inside < len(t) else float("nan")
    return out


def field_figures(prm, field):
    """Figures of a velocity map (capi.Context.field_map / RunResult.field_avg, or profile.shepard_field of one state: x, y,
    u_x, u_y as [ny, nx] arrays) against the analytic flow, on the host.  Nodes never sampled (NaN) are left out.
      u_row_mean, u_exact    the x-mean of u_x per row and the analytic profile at the rows' y
      rows, L2               the rows at least 2h from both walls, and l2_error of u_row_mean against u_exact over them
      x_spread, ix, iy       the largest deviation of a node's u_x from its row's x-mean over those rows, in % of |U_max|, and
                             the node where it occurs (a seam defect shows up at ix near 0 or nx - 1)
      uy_rms                 RMS of u_y over all sampled nodes
      U_max                  g DH^2 / (8 nu), signed"""
    y = np.asarray(field["y"], dtype=np.float64)
    ux, uy = np.asarray(field["u_x"], dtype=np.float64), np.asarray(field["u_y"], dtype=np.float64)
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    u_exact = prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y)
    ok = ~np.isnan(ux)
    n_row = np.maximum(ok.sum(axis=1), 1)
    first = np.where(ok.any(axis=1), ux[np.arange(len(y)), np.argmax(ok, axis=1)], np.nan)
    # (about the row's first sampled node: a row of equal values gives that value exactly)
    row_mean = first + np.where(ok, ux - first[:, None], 0.0).sum(axis=1) / n_row
    rows = (y >= 2.0 * prm.h) & (y <= prm.DH - 2.0 * prm.h)
    sel = rows & ~np.isnan(row_mean)
    dev = np.where(ok & rows[:, None], np.abs(ux - row_mean[:, None]), -1.0)
    iy, ix = np.unravel_index(int(np.argmax(dev)), dev.shape)
    x_spread = 100.0 * float(dev[iy, ix]) / abs(u_max) if dev[iy, ix] >= 0.0 else float("nan")
    uy_ok = uy[~np.isnan(uy)]
    return dict(u_row_mean=row_mean, u_exact=u_exact, rows=rows,
                L2=l2_error(np.where(sel, row_mean, np.nan), u_exact) if sel.any() else float("nan"),
                x_spread=x_spread, ix=int(ix), iy=int(iy),
                uy_rms=float(np.sqrt(np.mean(uy_ok * uy_ok))) if uy_ok.size else float("nan"), U_max=u_max)


def probe_figures(prm, probes, t_from=None):
    """Figures of a point-probe series (capi.Context.probes / RunResult.probes) per probe, on the host, over the records with
    t >= t_from (None: all).  A record stands for the interval that ended at its t, so its weight is the time since the record
    before it (the first record's: the second's).
      u_x_mean, u_y_mean, p_mean   dt-weighted time means of u_x, u_y and p = p0 (rho / rho0 - 1), [P]
      u_x_rms, u_y_rms, p_rms      dt-weighted RMS about those means, [P]
      u_exact                      the analytic profile g / (2 nu) y_p (DH - y_p) at the probes' y, [P]
      f_peak_uy, f_peak_p          the frequency of the largest line of the spectrum of the fluctuation of u_y and of p, [P]:
                                   the series resampled (linearly) onto a uniform time grid of its median dt, mean removed,
                                   numpy.fft.rfft; NaN with fewer than 4 records or a series with a NaN
      f_bin, n_records             the spectral resolution 1 / (n * median dt) and the records that entered
    The line to look for is the cross-channel acoustic mode: a pressure wave sloshing between the walls at
    f = c / (2 DH) with the artificial speed of sound c = c_f |U_bulk| (U_bulk = g DH^2 / (12 nu))."""
    t = np.asarray(probes["t"], dtype=np.float64)
    sel = np.ones(len(t), dtype=bool) if t_from is None else t >= t_from
    t = t[sel]
    n = len(t)
    y = np.asarray(probes["points"], dtype=np.float64)[:, 1]
    P = len(y)
    series = dict(u_x=np.asarray(probes["u_x"], dtype=np.float64)[sel], u_y=np.asarray(probes["u_y"], dtype=np.float64)[sel],
                  p=prm.p0 * (np.asarray(probes["rho"], dtype=np.float64)[sel] / prm.rho0 - 1.0))
    out = dict(u_exact=prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y), n_records=n,
               f_acoustic=prm.c_f * abs(prm.gravity_g * prm.DH ** 2 / (12.0 * prm.nu)) / (2.0 * prm.DH))
    nan = np.full(P, np.nan)
    if n >= 2:
        w = np.diff(t, prepend=t[0] - (t[1] - t[0]))
    else:
        w = np.ones(n)
    wsum = float(np.sum(w))
    for key, v in series.items():
        if n == 0 or not wsum > 0.0:
            out[key + "_mean"], out[key + "_rms"] = nan.copy(), nan.copy()
            continue
        # (about the first value: a constant series gives that value exactly)
        mean = v[0] + (w[:, None] * (v - v[0])).sum(axis=0) / wsum
        out[key + "_mean"] = mean
        out[key + "_rms"] = np.sqrt((w[:, None] * (v - mean) ** 2).sum(axis=0) / wsum)
    dt = float(np.median(np.diff(t))) if n >= 2 else float("nan")
    out["f_bin"] = float("nan")
    for key, name in (("u_y", "f_peak_uy"), ("p", "f_peak_p")):
        out[name] = nan.copy()
        if n < 4 or not dt > 0.0:
            continue
        tu = t[0] + dt * np.arange(int(np.floor((t[-1] - t[0]) / dt)) + 1)
        freq = np.fft.rfftfreq(len(tu), dt)
        out["f_bin"] = float(freq[1]) if len(freq) > 1 else float("nan")
        for k in range(P):
            v = series[key][:, k]
            if np.any(np.isnan(v)) or len(freq) < 2:
                continue
            u = np.interp(tu, t, v)
            amp = np.abs(np.fft.rfft(u - u.mean()))
            out[name][k] = freq[1 + int(np.argmax(amp[1:]))]
    return out


def _concat_probes(points, DL, chunks):
    """the series of a whole run from the drained chunks (none: an empty series at the points as folded)"""
    if not chunks:
        pts = np.array(points, dtype=np.float64).reshape(-1, 2)
        pts[:, 0] = capi.probes_fold(pts[:, 0], DL)
        return capi.probes_dict(pts, np.zeros((0, 2)), np.zeros((0, len(pts), len(capi.PROBE_FIELDS))))
    out = dict(points=chunks[0]["points"])
    out.update({k: np.concatenate([c[k] for c in chunks]) for k in ("step", "t") + capi.PROBE_FIELDS})
    out["n_dropped"] = int(sum(c["n_dropped"] for c in chunks))
    return out


def _records_lost(who, what, option, p, t, capacity):
    """the error of a run whose record buffer (`what`, sized by `option`) overflowed between two output points"""
    return RuntimeError(f"{who}{what} lost {p['n_dropped']} records before t={t:.6f}; the output interval needs "
                        f"{option} >= {len(p['step']) + p['n_dropped']} (it is {capacity})")


def _probes_lost(who, p, t, capacity):
    return _records_lost(who, "the point probes", "probe_capacity", p, t, capacity)


def _profiles_lost(who, p, t, capacity):
    return _records_lost(who, "the profile series", "profiles_capacity", p, t, capacity)


def _modes_lost(who, p, t, capacity):
    return _records_lost(who, "the mode amplitudes", "modes_capacity", p, t, capacity)


_MODE_KEYS = ("step", "t") + capi.MODE_FIELDS


def _concat_modes(chunks):
    """the mode amplitudes of a whole run (capi.modes_dict) from the drained chunks, in their order (at least one: its shape
    is the series')"""
    out = {k: np.concatenate([np.asarray(c[k]) for c in chunks]) for k in _MODE_KEYS}
    out["n_dropped"] = int(sum(c["n_dropped"] for c in chunks))
    return out


def mode_figures(prm, modes):
    """Figures of the mode amplitudes of a run (capi.Context.modes / RunResult.modes: n, ux, uy as [n_records, mx + 1, ny + 1, 4],
    bases cc, sc, cs, ss) on the host, with N = n[:, 0, 0, cc] the particle count of a record.
      b [n_records, ny + 1]       the sine coefficients of u_x across the channel, (2 / N) ux[:, 0, n, cs]
      b_exact [n_records, ny + 1] those of the start-up of plane Poiseuille flow from rest (profile.mode_b_exact): for odd n
                                  32 U_max / (n pi)^3 (1 - exp(-t / tau_exact[n])), one exponential per mode; 0 for even n
      tau_fit [ny + 1]            the decay time of mode n: minus the inverse slope of a least-squares line through
                                  log |b_exact(inf) - b| over the records with 0 < t <= 2 tau_exact[n]; NaN for even n and
                                  with fewer than two such records
      tau_exact [ny + 1]          DH^2 / (nu n^2 pi^2) (inf for n = 0)
      S [mx + 1, ny + 1]          the structure factor, the time mean of (cc^2 + sc^2 + cs^2 + ss^2) / N of the field n
      E_uy [mx + 1, ny + 1]       the same of the field uy, in U_max^2
      f_peak [mx + 1, ny + 1]     the frequency of the largest line of the summed spectra of the four fluctuating amplitudes
                                  of the field n (records resampled to the median dt, numpy.fft.rfft); NaN with fewer than 4
                                  records
      f_box [mx + 1, ny + 1]      the box's acoustic mode beside it, c sqrt((m / DL)^2 + (n / (2 DH))^2) with the artificial
                                  speed of sound c = c_f |U_bulk| of probe_figures; f_bin: the resolution of f_peak
    U_max = g DH^2 / (8 nu)."""
    t = np.asarray(modes["t"], dtype=np.float64)
    cnt, ux, uy = (np.asarray(modes[k], dtype=np.float64) for k in capi.MODE_FIELDS)
    R, MX, NY = cnt.shape[0], cnt.shape[1], cnt.shape[2]
    g, nu, DH, DL = prm.gravity_g, prm.nu, prm.DH, prm.DL
    u_max = g * DH * DH / (8.0 * nu)
    N = cnt[:, 0, 0, 0]
    n = np.arange(NY)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = 2.0 * ux[:, 0, :, 2] / N[:, None]
        tau_exact = np.where(n > 0, DH * DH / (nu * np.maximum(n, 1) ** 2 * np.pi ** 2), np.inf)
        S = np.mean((cnt ** 2).sum(axis=3) / N[:, None, None], axis=0) if R else np.full((MX, NY), np.nan)
        E_uy = np.mean((uy ** 2).sum(axis=3) / N[:, None, None], axis=0) / u_max ** 2 if R else np.full((MX, NY), np.nan)
    b_exact = mode_b_exact(n[None, :], t[:, None], g, nu, DH)
    b_inf = np.where(n % 2 == 1, 32.0 * u_max / (np.maximum(n, 1) * np.pi) ** 3, 0.0)
    tau_fit = np.full(NY, np.nan)
    for k in range(1, NY, 2):
        gap = np.abs(b_inf[k] - b[:, k])
        sel = (t > 0.0) & (t <= 2.0 * tau_exact[k]) & np.isfinite(gap) & (gap > 0.0)
        if np.count_nonzero(sel) >= 2 and np.ptp(t[sel]) > 0.0:
            slope = np.polyfit(t[sel], np.log(gap[sel]), 1)[0]
            tau_fit[k] = -1.0 / slope if slope != 0.0 else np.nan
    c = prm.c_f * abs(g * DH ** 2 / (12.0 * nu))
    f_box = c * np.sqrt((np.arange(MX)[:, None] / DL) ** 2 + (n[None, :] / (2.0 * DH)) ** 2)
    f_peak, f_bin = np.full((MX, NY), np.nan), float("nan")
    dt = float(np.median(np.diff(t))) if R >= 2 else float("nan")
    if R >= 4 and dt > 0.0:
        tu = t[0] + dt * np.arange(int(np.floor((t[-1] - t[0]) / dt)) + 1)
        freq = np.fft.rfftfreq(len(tu), dt)
        if len(freq) >= 2:
            f_bin = float(freq[1])
            for m in range(MX):
                for k in range(NY):
                    power = np.zeros(len(freq))
                    for q in range(4):
                        v = np.interp(tu, t, cnt[:, m, k, q])
                        power += np.abs(np.fft.rfft(v - v.mean())) ** 2
                    if np.all(np.isfinite(power)) and power[1:].max() > 0.0:
                        f_peak[m, k] = freq[1 + int(np.argmax(power[1:]))]
    return dict(b=b, b_exact=b_exact, tau_fit=tau_fit, tau_exact=tau_exact, S=S, E_uy=E_uy, f_peak=f_peak, f_box=f_box, f_bin=f_bin,
                U_max=float(u_max))


_SERIES_KEYS = ("step", "t") + capi.STATS_FIELDS


def _concat_profile_series(DH, chunks, who=""):
    """The raw series of a whole run (capi.profile_series_dict) from the drained chunks, in their order.  A chunk that lost
    records raises RuntimeError and names the capacity that output interval needed (ceil: a whole number of records); chunks
    of different bins or bands are refused."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError("_concat_profile_series needs at least one chunk (its shape is the series')")
    shape = np.asarray(chunks[0]["count"]).shape[1:]
    for c in chunks:
        if np.asarray(c["count"]).shape[1:] != shape:
            raise ValueError(f"{who}profile-series chunks of different shapes (n_bands, n_bins): "
                             f"{np.asarray(c['count']).shape[1:]} and {shape}")
        if c["n_dropped"]:
            need = int(np.ceil(len(c["step"]) + c["n_dropped"]))
            t = float(c["t"][-1]) if len(c["t"]) else float("nan")
            raise RuntimeError(f"{who}the profile series lost {c['n_dropped']} records after t={t:.6f}; the output interval "
                               f"needs profiles_capacity >= {need} (it held {len(c['step'])})")
    out = {k: np.concatenate([np.asarray(c[k]) for c in chunks]) for k in _SERIES_KEYS}
    out.update(n_dropped=0, y_mid=np.asarray(chunks[0]["y_mid"], dtype=np.float64))
    return profile_series_profiles(DH, out) | {k: out[k] for k in capi.STATS_FIELDS}


def profile_series_figures(prm, series, band=1, tol=0.02):
    """Figures of a profile series (capi.Context.profile_series / RunResult.profile_series) of band `band` against the start-up
    of plane Poiseuille flow from rest, on the host; [n_records] arrays unless said otherwise.
      L2_startup   relative L2 of u_mean against profile.poiseuille_startup(y_mid, t) per record, over the non-empty bins, by
                   profile.l2_error's rule (NaN for a record whose bins are all empty)
      L2_steady    the same against the steady parabola u_exact
      u_centre     the mean of the two middle bins (the middle bin's value for an odd n_bins)
      t_developed  the first record time from which L2_steady stays <= tol up to the last record; NaN if never
      tau_fit      the decay time of U_max - u_centre: minus the inverse slope of a least-squares line through
                   log |U_max - u_centre| over the records with 0.5 <= t pi^2 nu / DH^2 <= 3 (there the n = 3 mode is below
                   e^-4 of the first), with U_max taken where u_centre is -- the mean of u_exact over the same middle bins,
                   U_max (1 - 1 / n_bins^2) for an even n_bins: the difference would otherwise stay in the gap as a constant
                   and bend the line (1.6 % of tau at 20 bins); NaN with fewer than two such records
      tau_exact    DH^2 / (pi^2 nu), beside it; U_max = g DH^2 / (8 nu); u_exact [n_bins]"""
    t = np.asarray(series["t"], dtype=np.float64)
    y = np.asarray(series["y_mid"], dtype=np.float64)
    u = np.asarray(series["u_mean"], dtype=np.float64)[:, band, :]
    g, nu, DH = prm.gravity_g, prm.nu, prm.DH
    u_exact = g / (2.0 * nu) * y * (DH - y)
    u_max = g * DH * DH / (8.0 * nu)
    tau_exact = DH * DH / (np.pi ** 2 * nu)
    start = poiseuille_startup(y, t, g, nu, DH) if len(t) else np.zeros((len(y), 0))

    def l2(a, b):
        return l2_error(a, b) if not np.all(np.isnan(a)) else float("nan")

    L2_startup = np.array([l2(u[r], start[:, r]) for r in range(len(t))])
    L2_steady = np.array([l2(u[r], u_exact) for r in range(len(t))])
    mid = len(y) // 2
    centre = (lambda v: v[..., mid]) if len(y) % 2 else (lambda v: 0.5 * (v[..., mid - 1] + v[..., mid]))
    u_centre = centre(u)
    t_developed = float("nan")
    ok = L2_steady <= tol
    if len(t) and ok[-1]:
        bad = np.nonzero(~ok)[0]
        t_developed = float(t[bad[-1] + 1] if len(bad) else t[0])
    tau_fit = float("nan")
    gap = np.abs(centre(u_exact) - u_centre)
    sel = (t / tau_exact >= 0.5) & (t / tau_exact <= 3.0) & np.isfinite(gap) & (gap > 0.0)
    if np.count_nonzero(sel) >= 2 and np.ptp(t[sel]) > 0.0:
        slope = np.polyfit(t[sel], np.log(gap[sel]), 1)[0]
        tau_fit = float(-1.0 / slope) if slope != 0.0 else float("nan")
    return dict(L2_startup=L2_startup, L2_steady=L2_steady, u_centre=u_centre, t_developed=t_developed, tau_fit=tau_fit,
                tau_exact=float(tau_exact), U_max=float(u_max), u_exact=u_exact)


def _pair_bands(prm, bands):
    """the x-bands of a run's pair statistics: mid-channel and the periodic seam unless given"""
    hw = max(prm.dp, prm.h)
    return [(0.5 * prm.DL, hw), (0.0, hw)] if bands is None else bands


def _pair_dist_bands(sums, dp):
    """a channel's sums, one dict per band, each with the figures of profile.pair_dist_profiles"""
    return [dict(s, **pair_dist_profiles(s, dp)) for s in sums]


def pair_dist_figures(prm, pd):
    """Figures of a run's pair statistics (RunResult.pair_dist, capi.Context.pair_dist_sums(): one dict per band), on the host:
      r_min_dp   the smallest fluid-fluid separation met, in units of dp (inf before any pair): pairing shows as r_min << dp
      n_neigh    partners within r_max per centre, band 0
      sigma1_dp  the width of the first shell: the standard deviation of r over the pairs with r < 1.207 dp (half way between
                 the lattice's first and second shell, dp and sqrt(2) dp), taken from the mid-points of the bins whose mid-point
                 lies below that, in units of dp; 0 within a bin width on a lattice, NaN without such a pair
      seam_dev   with at least two x-bands (band 1 mid-channel, band 2 the periodic seam, the default of run()): the largest
                 |g_seam - g_mid| over the bins, relative to the largest g of either; NaN otherwise.  A neighbour missed at the
                 seam shows here."""
    whole = pd[0]
    dp = prm.dp
    prof = [pair_dist_profiles(b, dp) for b in pd]
    r_mid, ff = prof[0]["r_mid"], np.asarray(whole["ff"], dtype=np.float64)
    first = r_mid < 1.207 * dp
    n1 = ff[first].sum()
    sigma1 = float("nan")
    if n1 > 0:
        mean = (ff[first] * r_mid[first]).sum() / n1
        sigma1 = float(np.sqrt(max((ff[first] * (r_mid[first] - mean) ** 2).sum() / n1, 0.0)) / dp)
    seam_dev = float("nan")
    if len(pd) >= 3 and pd[1]["centres"] > 0 and pd[2]["centres"] > 0:
        top = max(float(np.max(prof[1]["g"])), float(np.max(prof[2]["g"])))
        seam_dev = float(np.max(np.abs(prof[2]["g"] - prof[1]["g"])) / top) if top > 0 else 0.0
    return dict(r_min_dp=float(whole["r_min"]) / dp, n_neigh=prof[0]["n_neigh"], sigma1_dp=sigma1, seam_dev=seam_dev)


def _grad_bands(prm, bands):
    """the x-bands of a run's gradient statistics: the mid-channel band of the output-point profiles (band 1) unless given"""
    return [(0.5 * prm.DL, max(prm.dp, prm.h))] if bands is None else bands


def _grad_stats_bands(DH, sums):
    """a channel's sums, one dict per band, each with the profiles of profile.grad_stats_profiles"""
    return [dict(s, **grad_stats_profiles(DH, s)) for s in sums]


def grad_figures(prm, gs, band=0):
    """Figures of a run's gradient statistics (RunResult.grad_stats, or [capi.Context.grad_stats_sums(b) for b in bands]: one
    dict per band), on the host, from band `band`:
      y_mid, shear    the bin centres and the bin-mean shear rate g_xy = du_x/dy (NaN where a bin is empty)
      shear_exact     the analytic g / (2 nu) (DH - 2 y) at y_mid; its sign follows the body force, as U_max's does
      L2_shear        l2_error(shear, shear_exact) over the bins at least 2h from a wall; L2_shear_all over all bins (next to a
                      wall the support is one-sided and the estimate first order: the wall bins read low)
      tau, tau_line   mu * shear and (slope, intercept) of its least-squares line over the bins at least 2h from a wall;
                      tau_fit_residual: the largest |tau - line| over those bins
      tau_wall_bottom, tau_wall_top   the line extrapolated to the walls, as the stress on each wall: line(0) and -line(DH),
                      to be read beside tau_target = g rho0 DH / 2 (the momentum balance makes tau linear in y)
      div_rms         sqrt(sum div^2 / count) over the whole band, in units of |U_max| / DH, U_max = g DH^2 / (8 nu)
      vort_mean       (sum g_yx - sum g_xy) / count over the whole band (zero by symmetry in plane Poiseuille flow)"""
    b = gs[band]
    prof = grad_stats_profiles(prm.DH, b)
    y, shear = prof["y_mid"], prof["gxy_mean"]
    exact = prm.gravity_g / (2.0 * prm.nu) * (prm.DH - 2.0 * y)
    inner = (y >= 2.0 * prm.h) & (y <= prm.DH - 2.0 * prm.h)
    ok = ~np.isnan(shear)
    nan = float("nan")
    tau = prm.mu * shear
    fit = inner & ok
    slope = icpt = resid = nan
    if np.count_nonzero(fit) >= 2:
        slope, icpt = (float(v) for v in np.polyfit(y[fit], tau[fit], 1))
        resid = float(np.max(np.abs(tau[fit] - (slope * y[fit] + icpt))))
    count = float(np.sum(b["count"]))
    u_max = prm.gravity_g * prm.DH * prm.DH / (8.0 * prm.nu)
    unit = abs(u_max) / prm.DH
    return dict(y_mid=y, shear=shear, shear_exact=exact,
                L2_shear=l2_error(np.where(inner, shear, np.nan), exact) if np.any(fit) else nan,
                L2_shear_all=l2_error(shear, exact) if np.any(ok) else nan,
                tau=tau, tau_line=(slope, icpt), tau_fit_residual=resid, tau_wall_bottom=icpt, tau_wall_top=-(slope * prm.DH + icpt),
                tau_target=prm.gravity_g * prm.rho0 * prm.DH / 2,
                div_rms=float(np.sqrt(np.sum(b["sum_div2"]) / count) / unit) if count > 0 else nan,
                vort_mean=float((np.sum(b["sum_gyx"]) - np.sum(b["sum_gxy"])) / count) if count > 0 else nan)


def _grad_columns(prms, grads):
    """The gradient columns of a sweep's table, one [M] array each: L2_shear, tau_wall_dev (the larger deviation of
    tau_wall_bottom / tau_wall_top from tau_target, relative to |tau_target|) and div_rms of grad_figures(prm_m, grad_stats_m)."""
    figs = [grad_figures(p, g) for p, g in zip(prms, grads)]
    dev = [max(abs(f["tau_wall_bottom"] - f["tau_target"]), abs(f["tau_wall_top"] - f["tau_target"])) / abs(f["tau_target"]) for f in figs]
    return dict(L2_shear=np.array([f["L2_shear"] for f in figs]), tau_wall_dev=np.array(dev), div_rms=np.array([f["div_rms"] for f in figs]))


def tracer_ids(tracers, n_fluid, seed=0):
    """The fluid rows a `tracers=` argument of run / run_sweep / run_ensemble names, as a sorted int64 array: "all" -- every
    fluid row; an int n, 1 <= n <= n_fluid -- that many rows, a seeded choice (the same rows for the same n, n_fluid and seed);
    anything else -- the rows themselves, as given (capi.tracers_config checks them).  ValueError for another string, a bool or
    an n out of range: before any device is touched."""
    if isinstance(tracers, str):
        if tracers != "all":
            raise ValueError(f'tracers must be a list of fluid rows, "all" or a number of rows, not {tracers!r}')
        return np.arange(n_fluid, dtype=np.int64)
    if isinstance(tracers, (bool, np.bool_)):
        raise ValueError('tracers must be a list of fluid rows, "all" or a number of rows, not a bool')
    if isinstance(tracers, (int, np.integer)):
        if not 1 <= tracers <= n_fluid:
            raise ValueError(f"tracers = {int(tracers)}: the number of rows must be 1 .. n_fluid = {n_fluid}")
        return np.sort(np.random.default_rng(seed).choice(n_fluid, size=int(tracers), replace=False)).astype(np.int64)
    return tracers


def _tracers_request(tracers, tracers_every, tracers_from, tracers_capacity, n_fluid, n_total, n_members=1):
    """the `tracers` of run / _run_batch -- (ids, every, capacity, t_from), every check made -- or None without tracers=;
    tracers_capacity None: 65536 records, or as many as the bound on capacity * n_tracers * 4 (over the members) allows"""
    if tracers is None:
        return None
    ids = tracer_ids(tracers, n_fluid)
    T = max(int(np.size(ids)), 1)
    if tracers_capacity is None:
        tracers_capacity = max(min(65536, (1 << 27) // (n_members * T * len(capi.TRACER_FIELDS))), 1)
    t_from = 0.0 if tracers_from is None else tracers_from
    _, ids = capi.tracers_config(n_fluid, n_total, ids, tracers_every, tracers_capacity, t_from, n_members=n_members)
    return ids, tracers_every, tracers_capacity, t_from


def _concat_tracers(ids, chunks):
    """the series of a whole run from the drained chunks (none: an empty series of these ids)"""
    if not chunks:
        return capi.tracers_dict(ids, np.zeros((0, 2)), np.zeros((0, len(ids), len(capi.TRACER_FIELDS))))
    out = dict(ids=chunks[0]["ids"])
    out.update({k: np.concatenate([c[k] for c in chunks]) for k in ("step", "t") + capi.TRACER_FIELDS})
    out.update(n_dropped=int(sum(c["n_dropped"] for c in chunks)), n_missing=int(sum(c["n_missing"] for c in chunks)))
    return out


def _tracers_lost(who, p, t, capacity):
    return _records_lost(who, "the tracers", "tracers_capacity", p, t, capacity)


def tracer_figures(prm, tracers, lags=None, y_margin=None):
    """Figures of a tracer series (capi.Context.tracers / RunResult.tracers), on the host: profile.tracer_profiles of the
    unwrapped series over the tracers that start at least y_margin (None: 2h) from both walls -- lags, tau, msd_y, msd_x_rel,
    D_y, y_drift, u_dev_rms, n_tracers, n_records -- plus D_y_nu = D_y / nu, the numerical cross-stream diffusivity in units of
    the physical one.  In laminar Poiseuille flow a fluid element never leaves its streamline: all of them measure the scheme."""
    margin = 2.0 * prm.h if y_margin is None else y_margin
    out = tracer_profiles(unwrap_tracers(tracers, prm.DL), prm.DL, prm.DH, prm.gravity_g, prm.nu, lags=lags, y_margin=margin)
    out["D_y_nu"] = out["D_y"] / prm.nu
    return out


_TRACER_COLUMNS = ("D_y_nu", "y_drift", "u_dev_rms")


def _tracer_columns(prms, series):
    """The tracer columns of a sweep's table, one [M] array each: D_y_nu, y_drift, u_dev_rms of tracer_figures(prm_m, tracers_m)."""
    figs = [tracer_figures(p, tr) for p, tr in zip(prms, series)]
    return {k: np.array([f[k] for f in figs]) for k in _TRACER_COLUMNS}


def _dens_bands(prm, bands):
    """the x-bands of a run's density statistics: the mid-channel band of the output-point profiles (band 1) unless given"""
    return [(0.5 * prm.DL, max(prm.dp, prm.h))] if bands is None else bands


def _dens_stats_bands(prm, sums):
    """a channel's sums, one dict per band, each with the profiles of profile.dens_stats_profiles"""
    return [dict(s, **dens_stats_profiles(prm.DH, prm.p0, s)) for s in sums]


def density_figures(prm, dens, band=0):
    """Figures of a run's density statistics (RunResult.dens_stats, or [capi.Context.dens_stats_sums(b) for b in bands]: one dict
    per band), on the host, from band `band`; delta = rho / rho0 - 1 of the density every step starts from:
      delta_rms, delta_mean   sqrt(sum delta^2 / N) and sum delta / N over the whole band
      delta_max    the largest |delta| met: the larger of |d_min| and |d_max| over the bins
      outliers     the particles left out (|delta| > delta_bound), over the whole band
      ma2          U_max^2 rho0 / p0 = (U_max / c)^2 with p0 = rho0 c^2, U_max = g DH^2 / (8 nu): the density variation a weakly
                   compressible flow at this Mach number is expected to show, to read delta_rms and delta_max beside
      p_spread     the spread (max - min) of the bin means of p = p0 delta over the bins at least 2h from a wall, in units of
                   rho0 U_max^2: plane Poiseuille flow keeps p flat in y
      wall_bias    the mean delta of the bins within 2h of a wall minus that of the bins at least 2h from one (by bin centre,
                   each side weighted by its counts)
      packing      1 + sum dvol / N over the whole band: the mean of rho0 / rho, the area sum m / rho the particles claim over
                   the area sum m / rho0 they were given
    NaN where the band holds no particle (p_spread, wall_bias: where a side has none)."""
    b = dens[band]
    prof = dens_stats_profiles(prm.DH, prm.p0, b)
    y = prof["y_mid"]
    N = np.asarray(b["count"], dtype=np.float64)
    total = float(N.sum())
    nan = float("nan")
    u_max = prm.gravity_g * prm.DH * prm.DH / (8.0 * prm.nu)
    inner = (y >= 2.0 * prm.h) & (y <= prm.DH - 2.0 * prm.h)
    some = N > 0

    def mean(rows):
        n = float(N[rows & some].sum())
        return float(np.asarray(b["sum_d"])[rows & some].sum()) / n if n > 0 else nan

    p_in = prof["p_mean"][inner & some]
    ends = [v for v in (np.abs(np.asarray(b["d_min"])[some]), np.abs(np.asarray(b["d_max"])[some])) if len(v)]
    return dict(delta_rms=float(np.sqrt(np.sum(b["sum_d2"]) / total)) if total > 0 else nan,
                delta_mean=float(np.sum(b["sum_d"]) / total) if total > 0 else nan,
                delta_max=float(max(np.max(v) for v in ends)) if ends else nan,
                outliers=int(np.sum(b["outliers"])), ma2=float(u_max * u_max * prm.rho0 / prm.p0),
                p_spread=float((np.max(p_in) - np.min(p_in)) / (prm.rho0 * u_max * u_max)) if len(p_in) else nan,
                wall_bias=mean(~inner) - mean(inner),
                packing=float(1.0 + np.sum(b["sum_dvol"]) / total) if total > 0 else nan)


def _dens_columns(prms, dens):
    """The density columns of a sweep's table, one [M] array each: delta_rms, delta_max, p_spread of
    density_figures(prm_m, dens_stats_m)."""
    figs = [density_figures(p, d) for p, d in zip(prms, dens)]
    return {k: np.array([f[k] for f in figs]) for k in ("delta_rms", "delta_max", "p_spread")}


def _density_request(density_from, density_every, density_hist, density_bands):
    """the `density` of _run_batch: None without density_from"""
    return None if density_from is None else (density_from, density_every, density_hist, density_bands)


def _concat_history(chunks):
    if not chunks:
        return capi.history_dict(np.zeros((0, len(capi.HISTORY_FIELDS))))
    out = {k: np.concatenate([c[k] for c in chunks]) for k in capi.HISTORY_FIELDS}
    out["n_dropped"] = int(sum(c["n_dropped"] for c in chunks))
    return out


def run(prm, engine="resident", log=None, log_every=0, parts=None, lanes_per_particle=0, steps_per_graph=0,
        rebuild_every=0, restart_path=None, postprocess_path=None, dual_rate=0, mat_format="auto", average_from=None,
        average_every=1, history_every=None, history_capacity=65536, field_from=None, field_every=1, field_shape=None,
        field_walls=False, probe_points=None, probe_every=1, probe_capacity=65536, probe_from=None, probe_walls=False,
        profiles_every=None, profiles_from=None, profiles_capacity=4096, profiles_bands=None, pairs_from=None, pairs_every=1,
        pairs_bins=64, pairs_walls=False, pairs_bands=None, gradients_from=None, gradients_every=1, gradients_walls=False,
        gradients_bands=None, tracers=None, tracers_every=1, tracers_from=None, tracers_capacity=None, density_from=None,
        density_every=1, density_hist=(64, 0.05), density_bands=None, modes_every=None, modes=(4, 8), modes_from=0.0,
        modes_capacity=4096):
    """Run to prm.t_end and return the final profile and L2 (SPH_Poiseuille.m:246-307 + postprocess :42).

    restart_path (resident engine): the reference's restart.mat protocol -- resume from it when
    prm.restart_from_file is set and its signature / sizes match (:132-163), rewrite it at every output point
    (:295).  postprocess_path: write SPH_Poiseuille_postprocess.mat at the end (:305-306).  mat_format: "7.3" (HDF5, what
    the reference writes), "5", or "auto" = 7.3 where a libhdf5 can be loaded (restart.py); either is read back.
    dual_rate (resident engine, opt-in, NOT the reference's loop): up to that many acoustic sub-steps per outer step,
    see sphx_params.dual_rate in include/sphx.h; the result then carries n_inner and steps counts outer steps.
    average_from (resident engine): accumulate, on the device and inside the step loop, every average_every-th step ending
    at t >= average_from into the reference's profile bins, for the whole channel and the mid-channel band (DL/2,
    max(dp, h)); RunResult.time_avg then holds the time-averaged profiles, their L2 against u_exact and the stability
    figures defined in time_average().  The output-point snapshots are taken as without it.
    history_every (resident engine): record every history_every-th step on the device (include/sphx.h section 2d: step, t,
    dt, vmax, tau_bottom, tau_top, kinetic_energy, u_bulk); the buffer (history_capacity records) is drained at every
    output point, so a capacity that holds one output interval suffices, and RunResult.history is the series of the
    whole run (history_figures() turns it into means and a settling time).
    field_from (resident engine): accumulate, on the device and inside the step loop, every field_every-th step ending at
    t >= field_from into a velocity map on a regular grid (include/sphx.h section 2e; field_shape = (nx, ny), None = the
    reference's 2 round(DL/dp) x 2 round(DH/dp); field_walls: the wall particles contribute with their wall velocity);
    RunResult.field_avg is capi.Context.field_map() at the end (field_figures() turns it into an x-mean profile, its L2
    and the spread along x).  A map of the final state of any engine: profile.shepard_field(res.pos[:nf], res.vel[:nf], ...).
    probe_points (resident engine): record, on the device and inside the step loop, the Shepard sample of the flow at these
    points [P, 2] (include/sphx.h section 2h: weight, u_x, u_y, rho per point) every probe_every-th step ending at
    t >= probe_from (None: from the start; probe_walls: the wall particles contribute with their wall velocity); the buffer
    (probe_capacity records) is drained at every output point, so a capacity that holds one output interval suffices --
    a run that lost records raises RuntimeError and names the capacity needed -- and RunResult.probes is the series of the
    whole run (probe_figures() turns it into means, RMS and spectral peaks per probe).
    profiles_every (resident engine): record, on the device and inside the step loop, the binned velocity profile (include/sphx.h
    section 2j: the flow statistics' sample of one step) every profiles_every-th step ending at t >= profiles_from (None: from
    the start) in the reference's bins, for the whole channel and the bands profiles_bands (None: the mid-channel band (DL/2,
    max(dp, h)) the output-point profiles use); the buffer (profiles_capacity records) is drained at every output point -- a
    run that lost records raises RuntimeError and names the capacity needed -- and RunResult.profile_series is the series of
    the whole run (profile_series_figures() compares it with the start-up solution).  The output-point snapshots are taken
    as without it.
    pairs_from (resident engine; default off): count, on the device and inside the step loop, the pair-distance histogram of
    the fluid particles (include/sphx.h section 2l) every pairs_every-th step ending at t >= pairs_from: pairs_bins bins on
    [0, 2h), centres at least 2h from both walls (so g(r) is a bulk figure), the whole channel and the bands pairs_bands (None:
    mid-channel and the periodic seam, (DL/2, max(dp, h)) and (0, max(dp, h))), pairs_walls: the fluid-wall histogram too.
    RunResult.pair_dist is one dict per band; pair_dist_figures() gives r_min, the neighbour count, the width of the first
    shell and the seam's deviation.  A sample costs 1.6-1.9 cell sweeps of the density pass: pairs_every is the control.
    gradients_from (resident engine; default off): estimate, on the device and inside the step loop, the velocity gradient at
    every fluid particle (include/sphx.h section 2n) every gradients_every-th step ending at t >= gradients_from and bin it into
    the reference's profile bins, for the whole channel and the bands gradients_bands (None: the mid-channel band (DL/2,
    max(dp, h)) as band 1); gradients_walls: the wall particles are partners too (off: they carry the wall's velocity and pull
    the wall-adjacent bins down).  RunResult.grad_stats is one dict per band; grad_figures() gives the shear-rate profile and its
    L2 against the analytic one, tau(y) with its line extrapolated to the walls, div_rms and the mean vorticity.
    tracers (resident engine; default off): follow, on the device and inside the step loop, chosen fluid rows (include/sphx.h
    section 2p: x, y, u_x, u_y per tracer, the bits download() returns in that row): a list of rows, "all", or an int -- that many
    rows, a seeded choice (tracer_ids) -- every tracers_every-th step ending at t >= tracers_from (None: from the start); the
    buffer (tracers_capacity records; None: 65536, or what the bound on capacity * n_tracers * 4 allows) is drained at every
    output point -- a run that lost records raises RuntimeError and names the capacity needed -- and RunResult.tracers is the
    series of the whole run (tracer_figures() gives the cross-stream diffusivity, the drift and the Lagrangian velocity error).
    density_from (resident engine; default off): re-sum, on the device and inside the step loop, the density every step starts
    from at every fluid particle (include/sphx.h section 2r) every density_every-th step ending at t >= density_from and bin
    delta = rho / rho0 - 1 into the reference's profile bins, for the whole channel and the bands density_bands (None: the
    mid-channel band (DL/2, max(dp, h)) as band 1), with a histogram of delta of density_hist = (n_hist, hist_range).
    RunResult.dens_stats is one dict per band; density_figures() gives delta_rms, delta_max, the spread of the pressure across
    the channel, the bias next to the walls and the packing.
    modes_every (resident engine; default off): project, on the device and inside the step loop, the count, u_x and u_y of the
    fluid particles on the channel's modes (include/sphx.h section 2t: modes = (mx, ny)) every modes_every-th step ending at
    t >= modes_from; the buffer (modes_capacity records) is drained at every output point -- a run that lost records raises
    RuntimeError and names the capacity needed -- and RunResult.modes is the series of the whole run (mode_figures() gives the
    start-up coefficients b_n(t) beside the closed form, their decay times, the structure factor and the spectral peaks)."""
    if modes_every is not None and engine != "resident":
        raise ValueError("modes_every needs the resident engine (the amplitudes are summed on the device)")
    if density_from is not None and engine != "resident":
        raise ValueError("density_from needs the resident engine (the density is re-summed on the device)")
    if tracers is not None and engine != "resident":
        raise ValueError("tracers needs the resident engine (the tracers are recorded on the device)")
    if gradients_from is not None and engine != "resident":
        raise ValueError("gradients_from needs the resident engine (the gradients are estimated on the device)")
    if pairs_from is not None and engine != "resident":
        raise ValueError("pairs_from needs the resident engine (the pairs are counted on the device)")
    if profiles_every is not None and engine != "resident":
        raise ValueError("profiles_every needs the resident engine (the series is recorded on the device)")
    if probe_points is not None and engine != "resident":
        raise ValueError("probe_points needs the resident engine (the probes are recorded on the device)")
    if field_from is not None and engine != "resident":
        raise ValueError("field_from needs the resident engine (the map is accumulated on the device)")
    if average_from is not None and engine != "resident":
        raise ValueError("average_from needs the resident engine (the statistics are accumulated on the device)")
    if history_every is not None and engine != "resident":
        raise ValueError("history_every needs the resident engine (the history is recorded on the device)")
    parts = init_particles(prm) if parts is None else parts
    nf, nt = parts["n_fluid"], parts["n_total"]
    tracing = _tracers_request(tracers, tracers_every, tracers_from, tracers_capacity, nf, nt)
    t_start, step_start, n_inner = 0.0, 0, 1
    if restart_path and engine != "resident":
        raise ValueError("restart files are handled by the resident engine")
    if restart_path and prm.restart_from_file:
        st, why = restart.load_restart(restart_path, nt, prm.config_signature)
        if st is not None:
            parts = dict(parts, pos=st["pos"], vel=st["vel"], drho_dt=st["drho_dt"])
            t_start, step_start = st["t"], st["step"]
            if log:
                log(f"Restart: resuming from t={t_start:.6f}, step={step_start}")
        elif log:
            log(f"Restart file not used ({why}); starting from scratch")
    n_bins = n_profile_bins(prm.DH, prm.dp)
    mid_x, mid_hw = 0.5 * prm.DL, max(prm.dp, prm.h)
    profile_times, mid_profiles, full_profiles = [0.0], [], []
    _, u0 = compute_mid_channel_profile(parts["pos"][:nf], parts["vel"][:nf, 0], prm.DL, prm.DH, mid_x, mid_hw, n_bins)
    mid_profiles.append(u0)
    tau_b = tau_t = 0.0
    policy = {}
    time_avg = None
    history, history_chunks = None, []
    field_avg = None
    probes, probe_chunks = None, []
    series, series_chunks = None, []
    pair_dist = None
    grad_stats = None
    tracer_series, tracer_chunks = None, []
    dens_stats = None
    mode_series, mode_chunks = None, []
    t0 = time.perf_counter()
    if engine == "resident":
        ctx = capi.Context.from_parts(prm, parts, t0=t_start, step0=step_start, lanes_per_particle=lanes_per_particle,
                                      steps_per_graph=steps_per_graph, rebuild_every=rebuild_every, dual_rate=dual_rate)
        t, step = t_start, step_start
        try:
            n_inner = ctx.substeps()
            if average_from is not None:
                ctx.flow_stats_enable(n_bins=n_bins, every=average_every, t_from=average_from, bands=[(mid_x, mid_hw)])
            if history_every is not None:
                ctx.history_enable(every=history_every, capacity=history_capacity)
            if field_from is not None:
                fnx, fny = field_shape if field_shape is not None else (0, 0)
                ctx.field_map_enable(nx=fnx, ny=fny, every=field_every, t_from=field_from, with_walls=field_walls)
            if probe_points is not None:
                ctx.probes_enable(probe_points, every=probe_every, capacity=probe_capacity,
                                  t_from=t_start if probe_from is None else probe_from, with_walls=probe_walls)
            if profiles_every is not None:
                ctx.profile_series_enable(n_bins=n_bins, every=profiles_every, capacity=profiles_capacity,
                                          t_from=t_start if profiles_from is None else profiles_from,
                                          bands=[(mid_x, mid_hw)] if profiles_bands is None else profiles_bands)
            if pairs_from is not None:
                ctx.pair_dist_enable(n_bins=pairs_bins, every=pairs_every, t_from=pairs_from, y_margin=2.0 * prm.h,
                                     with_walls=pairs_walls, bands=_pair_bands(prm, pairs_bands))
            if gradients_from is not None:
                ctx.grad_stats_enable(n_bins=n_bins, every=gradients_every, t_from=gradients_from, with_walls=gradients_walls,
                                      bands=_grad_bands(prm, gradients_bands))
            if tracing:
                ctx.tracers_enable(tracing[0], every=tracing[1], capacity=tracing[2],
                                   t_from=t_start if tracers_from is None else tracing[3])
            if density_from is not None:
                ctx.dens_stats_enable(n_bins=n_bins, every=density_every, t_from=density_from, n_hist=density_hist[0],
                                      hist_range=density_hist[1], bands=_dens_bands(prm, density_bands))
            if modes_every is not None:
                ctx.modes_enable(mx=modes[0], ny=modes[1], every=modes_every, capacity=modes_capacity, t_from=modes_from)
            while t < prm.t_end - 1e-12:
                target = min(t + prm.output_interval, prm.t_end)
                while t < target - 1e-12:
                    st = ctx.advance(target, max_steps=log_every if log_every else 0)
                    t, step = st["t"], st["step"]
                    if log and log_every:
                        tb, tt, npairs = ctx.monitor(tau=True, pairs=True)
                        log(f"step={step}, t={t:.6f}/{prm.t_end:.6f}, dt={st['dt_last']:.4e}, pairs={int(npairs)}, "
                            f"vmax={st['vmax']:.4f}\n  [thick-wall-noslip] tau_bot={tb:.4f}, tau_top={tt:.4f}, "
                            f"tau_target={prm.gravity_g * prm.rho0 * prm.DH / 2:.4f}")
                d = ctx.download() if restart_path else ctx.download(fields=("pos", "vel"))
                _, u = compute_mid_channel_profile(d["pos"][:nf], d["vel"][:nf, 0], prm.DL, prm.DH, mid_x, mid_hw, n_bins)
                profile_times.append(t)
                mid_profiles.append(u)
                full_profiles.append(final_profile(np.column_stack([np.mod(d["pos"][:nf, 0], prm.DL), d["pos"][:nf, 1]]),
                                                   d["vel"][:nf, 0], prm)[1])
                if history_every is not None:
                    history_chunks.append(ctx.history(drain=True))
                if probe_points is not None:
                    probe_chunks.append(ctx.probes(drain=True))
                    if probe_chunks[-1]["n_dropped"]:
                        raise _probes_lost("", probe_chunks[-1], t, probe_capacity)
                if profiles_every is not None:
                    series_chunks.append(ctx.profile_series_sums(drain=True))
                    if series_chunks[-1]["n_dropped"]:
                        raise _profiles_lost("", series_chunks[-1], t, profiles_capacity)
                if tracing:
                    tracer_chunks.append(ctx.tracers(drain=True))
                    if tracer_chunks[-1]["n_dropped"]:
                        raise _tracers_lost("", tracer_chunks[-1], t, tracing[2])
                if modes_every is not None:
                    mode_chunks.append(ctx.modes(drain=True))
                    if mode_chunks[-1]["n_dropped"]:
                        raise _modes_lost("", mode_chunks[-1], t, modes_capacity)
                if restart_path:
                    restart.save_restart(restart_path, prm.config_signature, dict(d, t=t, step=step), fmt=mat_format)
                if log:
                    log(f"output point: t={t:.6f}, step={step}")
            wall = time.perf_counter() - t0
            tau_b, tau_t, _ = ctx.monitor(tau=True)
            d = ctx.download(fields=("pos", "vel"))
            pos, vel = d["pos"], d["vel"]
            policy = ctx.grid_policy()
            if average_from is not None:
                time_avg = time_average(prm, ctx.flow_stats(0), ctx.flow_stats(1))
            if history_every is not None:
                history = _concat_history(history_chunks)
            if field_from is not None:
                field_avg = ctx.field_map()
            if probe_points is not None:
                probes = _concat_probes(probe_points, prm.DL, probe_chunks)
            if profiles_every is not None:
                series = _concat_profile_series(prm.DH, series_chunks or [ctx.profile_series_sums()])
            if pairs_from is not None:
                pair_dist = _pair_dist_bands(ctx.pair_dist_sums(), prm.dp)
            if gradients_from is not None:
                grad_stats = _grad_stats_bands(prm.DH, [ctx.grad_stats_sums(b) for b in range(1 + len(_grad_bands(prm, gradients_bands)))])
            if tracing:
                tracer_series = _concat_tracers(tracing[0], tracer_chunks)
            if density_from is not None:
                dens_stats = _dens_stats_bands(prm, [ctx.dens_stats_sums(b) for b in range(1 + len(_dens_bands(prm, density_bands)))])
            if modes_every is not None:
                mode_series = _concat_modes(mode_chunks or [ctx.modes()])
        finally:
            ctx.close()
    elif engine == "mex":
        S = {k: np.array(parts[k], order="F", copy=True) for k in ("pos", "vel", "drho_dt", "mass", "wall_vel")}
        nb = sph_neighbor_search_mex(S["pos"], nf, nt, prm.h, prm.DL)
        t, step = 0.0, 0
        while t < prm.t_end - 1e-12:
            target = min(t + prm.output_interval, prm.t_end)
            while t < target - 1e-12:
                step += 1
                remain = min(target - t, prm.t_end - t)
                pi, pj, dx, dy, r, W, dW = nb
                rho, Vol, B = sph_physics_shell_mex("density_correction", pi, pj, dx, dy, r, W, dW, S["mass"], nf, nt,
                                                    prm.rho0, prm.h, prm.inv_sigma0)
                fp = sph_physics_shell_mex("viscous_force", pi, pj, dx, dy, r, dW, S["vel"], Vol, B, prm.mu, prm.h,
                                           nf, nt, S["mass"], S["wall_vel"])
                fp[:nf, 0] += S["mass"][:nf] * prm.gravity_g
                fp[nf:, :] = 0.0
                S["pos"] = sph_physics_shell_mex("transport_correction", pi, pj, dx, dy, r, dW, Vol, B, S["pos"],
                                                 prm.h, nf, nt, prm.transport_coeff)
                dt = verlet_time_step(S["vel"][:nf], prm.c_f, prm.h, prm.nu, prm.gravity_g, remain)
                if dt < 1e-14:
                    raise RuntimeError(f"unified Verlet dt collapsed (dt={dt:.2e}) at t={t:.6f} step={step}")
                rho, p, S["pos"], S["vel"], S["drho_dt"], force = sph_physics_shell_mex(
                    "integration_verlet", pi, pj, dx, dy, r, dW, Vol, B, rho, S["mass"], S["pos"], S["vel"],
                    S["drho_dt"], fp, dt, nf, nt, prm.rho0, prm.p0, prm.c_f, S["wall_vel"])
                t += dt
                periodic_bounding(S["pos"], nf, prm.DL)
                S["vel"][nf:, :] = 0.0
                nb = sph_neighbor_search_mex(S["pos"], nf, nt, prm.h, prm.DL)
                pi, pj, dx, dy, r, W, dW = nb
                tau_b, tau_t = sph_physics_shell_mex("wall_shear_monitor", pi, pj, dx, dy, r, dW, S["pos"], S["vel"],
                                                     S["wall_vel"], Vol, B, nf, prm.DL, prm.DH, prm.mu, prm.h)
                if log and log_every and step % log_every == 0:
                    log(f"step={step}, t={t:.6f}/{prm.t_end:.6f}, dt={dt:.4e}, pairs={len(pi)}")
            _, u = compute_mid_channel_profile(S["pos"][:nf], S["vel"][:nf, 0], prm.DL, prm.DH, mid_x, mid_hw, n_bins)
            profile_times.append(t)
            mid_profiles.append(u)
            full_profiles.append(final_profile(S["pos"][:nf], S["vel"][:nf, 0], prm)[1])
        wall = time.perf_counter() - t0
        pos, vel = S["pos"], S["vel"]
    else:
        raise ValueError("engine must be 'resident' or 'mex'")
    if postprocess_path:
        restart.save_postprocess_data(postprocess_path, restart.make_postprocess_data(
            prm, nf, pos, vel, n_bins, profile_times, np.column_stack([np.nan_to_num(u, nan=np.nan) for u in mid_profiles])),
                                      fmt=mat_format)
    return _run_result(prm, nf, nt, pos, vel, t=t, steps=int(step), wall_seconds=wall, profile_times=profile_times,
                       mid_profile_u=mid_profiles, tau_bottom=tau_b, tau_top=tau_t, grid_policy=policy,
                       full_profile_u=full_profiles, n_inner=n_inner, time_avg=time_avg, history=history, field_avg=field_avg,
                       probes=probes, profile_series=series, pair_dist=pair_dist, grad_stats=grad_stats, tracers=tracer_series,
                       dens_stats=dens_stats, modes=mode_series)


def _run_result(prm, nf, nt, pos, vel, **fields):
    """The RunResult of a final state: x wrapped into the channel, the final profile and its L2 against the analytic one,
    tau_target; `fields` are the RunResult fields the caller knows."""
    fluid_pos = pos[:nf].copy()
    fluid_pos[:, 0] = np.mod(fluid_pos[:, 0], prm.DL)
    y_mid, u_mean, u_exact = final_profile(fluid_pos, vel[:nf, 0], prm)
    return RunResult(prm=prm, n_fluid=nf, n_total=nt, pos=pos, vel=vel, y_mid=y_mid, u_mean=u_mean, u_exact=u_exact,
                     L2_error=l2_error(u_mean, u_exact), tau_target=prm.gravity_g * prm.rho0 * prm.DH / 2, **fields)


def _batch_inputs(prms, parts_list):
    """What the batch drivers ask of their (non-empty) inputs: one set of output points, one particle set per member."""
    p0 = prms[0]
    for k, p in enumerate(prms):
        if p.output_interval != p0.output_interval or p.t_end != p0.t_end:
            raise ValueError(f"member {k}: output_interval / t_end differ from member 0 (members share the output points)")
    parts_list = [init_particles(p) for p in prms] if parts_list is None else list(parts_list)
    if len(parts_list) != len(prms):
        raise ValueError("parts_list needs one particle set per parameter set")
    return parts_list


def _batch_policy(b):
    info = b.info()
    return dict(rebuild_every=info["rebuild_every"], skin=info["skin"], forced_rebuilds=info["forced_rebuilds"],
                realignments=info["realignments"])


def _batch_member_result(b, m, prm, nf, nt, st, times, wall, policy, **extra):
    """Member m's RunResult at the end of a batch run: final state, profile and L2, tau of the last step."""
    tau_b, tau_t, _ = b.monitor(m, tau=True)
    d = b.download(m, fields=("pos", "vel"))
    s = st[m] if st else dict(t=0.0, step=0)
    return _run_result(prm, nf, nt, d["pos"], d["vel"], t=s["t"], steps=int(s["step"]), wall_seconds=wall,
                       profile_times=list(times), tau_bottom=tau_b, tau_top=tau_t, grid_policy=dict(policy), **extra)


def _run_batch(name, prms, parts_list, launch, log, snapshots=False, average=None, history=None, field=None, probe=None,
               profiles=None, pairs=None, gradients=None, tracers=None, density=None, modes=None):
    """The batch run behind run_batch, run_ensemble and run_sweep (`name`, for the refusals): check and default the inputs,
    open the batch with the launch keywords `launch`, enable what was asked for, advance output point by output point, build
    every member's RunResult.
      snapshots  download every member at every output point: its mid_profile_u and full_profile_u
      average    (average_from, average_every): the flow statistics of the whole channel and the mid-channel band (DL/2,
                 max(dp, h)); every member gets a time_avg
      history    (history_every, history_capacity): the step history, drained at every output point; every member gets a
                 history, and one that lost records raises RuntimeError
      field      (field_from, field_every, field_shape, field_walls): the velocity map of include/sphx.h section 2g, enabled
                 before the first advance and read once at the end; every member gets a field_avg
      probe      (probe_points, probe_every, probe_capacity, probe_from, probe_walls): the point probes of include/sphx.h
                 section 2i, drained at every output point; every member gets its probes, and one that lost records raises
                 RuntimeError
      profiles   (profiles_every, profiles_from, profiles_capacity, profiles_bands): the profile series of include/sphx.h
                 section 2k, drained at every output point; every member gets its profile_series, and one that lost records
                 raises RuntimeError
      pairs      (pairs_from, pairs_every, pairs_bins, pairs_walls, pairs_bands): the pair statistics of include/sphx.h section
                 2m with the margin and the default bands of run(); every member gets its pair_dist
      gradients  (gradients_from, gradients_every, gradients_walls, gradients_bands): the gradient statistics of include/sphx.h
                 section 2o in the bins and with the default band of run(); every member gets its grad_stats
      tracers    (tracers, tracers_every, tracers_from, tracers_capacity) as run() takes them: the tracers of include/sphx.h
                 section 2q, one id list for all members, drained at every output point; every member gets its tracers, and one
                 that lost records raises RuntimeError
      density    (density_from, density_every, density_hist, density_bands): the density statistics of include/sphx.h section 2s
                 in the bins and with the default band of run(); every member gets its dens_stats
      modes      (modes_every, (mx, ny), modes_from, modes_capacity): the mode amplitudes of include/sphx.h section 2u, drained
                 at every output point; every member gets its modes, and one that lost records raises RuntimeError
    -> the members, the wall seconds, the grid policy, with average the raw sums (whole, mid) of all members, and with field the
    raw planes of all members."""
    prms = list(prms)
    if not prms:
        raise ValueError(f"{name} needs at least one parameter set")
    p0 = prms[0]
    parts_list = _batch_inputs(prms, parts_list)
    nf, nt = parts_list[0]["n_fluid"], parts_list[0]["n_total"]
    M = len(prms)
    tracing = _tracers_request(*tracers, nf, nt, n_members=M) if tracers else None
    n_bins = n_profile_bins(p0.DH, p0.dp)
    mid_x, mid_hw = 0.5 * p0.DL, max(p0.dp, p0.h)

    def mid_profile(d):
        return compute_mid_channel_profile(d["pos"][:nf], d["vel"][:nf, 0], p0.DL, p0.DH, mid_x, mid_hw, n_bins)[1]

    times = [0.0]
    mids = [[mid_profile(pa)] for pa in parts_list] if snapshots else None
    fulls = [[] for _ in range(M)]
    chunks = [[] for _ in range(M)]
    pchunks = [[] for _ in range(M)]
    schunks = [[] for _ in range(M)]
    tchunks = [[] for _ in range(M)]
    mchunks = [[] for _ in range(M)]
    t0 = time.perf_counter()
    with capi.Batch.from_parts(prms, parts_list, **launch) as b:
        if history:
            b.history_enable(every=history[0], capacity=history[1])
        if average:
            b.flow_stats_enable(n_bins=n_bins, every=average[1], t_from=float(average[0]), bands=[(mid_x, mid_hw)])
        if field:
            fnx, fny = field[2] if field[2] is not None else (0, 0)
            b.field_map_enable(nx=fnx, ny=fny, every=field[1], t_from=field[0], with_walls=field[3])
        if probe:
            b.probes_enable(probe[0], every=probe[1], capacity=probe[2], t_from=0.0 if probe[3] is None else probe[3],
                            with_walls=probe[4])
        if profiles:
            b.profile_series_enable(n_bins=n_bins, every=profiles[0], capacity=profiles[2],
                                    t_from=0.0 if profiles[1] is None else profiles[1],
                                    bands=[(mid_x, mid_hw)] if profiles[3] is None else profiles[3])
        if pairs:
            b.pair_dist_enable(n_bins=pairs[2], every=pairs[1], t_from=float(pairs[0]), y_margin=2.0 * p0.h, with_walls=pairs[3],
                               bands=_pair_bands(p0, pairs[4]))
        if gradients:
            b.grad_stats_enable(n_bins=n_bins, every=gradients[1], t_from=float(gradients[0]), with_walls=gradients[2],
                                bands=_grad_bands(p0, gradients[3]))
        if tracing:
            b.tracers_enable(tracing[0], every=tracing[1], capacity=tracing[2], t_from=tracing[3])
        if density:
            b.dens_stats_enable(n_bins=n_bins, every=density[1], t_from=float(density[0]), n_hist=density[2][0], hist_range=density[2][1],
                                bands=_dens_bands(p0, density[3]))
        if modes:
            b.modes_enable(mx=modes[1][0], ny=modes[1][1], every=modes[0], capacity=modes[3], t_from=modes[2])
        t = 0.0
        st = None
        while t < p0.t_end - 1e-12:
            target = min(t + p0.output_interval, p0.t_end)
            st = b.advance(target)
            t = min(s["t"] for s in st)
            times.append(t)
            if snapshots:
                for m in range(M):
                    d = b.download(m, fields=("pos", "vel"))
                    mids[m].append(mid_profile(d))
                    fulls[m].append(final_profile(np.column_stack([np.mod(d["pos"][:nf, 0], p0.DL), d["pos"][:nf, 1]]),
                                                  d["vel"][:nf, 0], prms[m])[1])
            if history:
                for m, h in enumerate(b.history(drain=True)):
                    if h["n_dropped"]:
                        raise RuntimeError(f"member {m}: the step history lost {h['n_dropped']} records before t={t:.6f}; "
                                           f"the output interval needs history_capacity >= "
                                           f"{len(h['step']) + h['n_dropped']} (it is {history[1]})")
                    chunks[m].append(h)
            if probe:
                for m, p in enumerate(b.probes(drain=True)):
                    if p["n_dropped"]:
                        raise _probes_lost(f"member {m}: ", p, t, probe[2])
                    pchunks[m].append(p)
            if profiles:
                for m, p in enumerate(b.profile_series_sums(drain=True)):
                    if p["n_dropped"]:
                        raise _profiles_lost(f"member {m}: ", p, t, profiles[2])
                    schunks[m].append(p)
            if tracing:
                for m, p in enumerate(b.tracers(drain=True)):
                    if p["n_dropped"]:
                        raise _tracers_lost(f"member {m}: ", p, t, tracing[2])
                    tchunks[m].append(p)
            if modes:
                for m, p in enumerate(b.modes(drain=True)):
                    if p["n_dropped"]:
                        raise _modes_lost(f"member {m}: ", p, t, modes[3])
                    mchunks[m].append(p)
            if log:
                log(f"output point: t={t:.6f}, steps={[s['step'] for s in st]}")
        wall = time.perf_counter() - t0
        policy = _batch_policy(b)
        sums = (b.flow_stats_sums(0), b.flow_stats_sums(1)) if average else None
        planes = b.field_map_sums() if field else None
        empty_series = b.profile_series_sums() if profiles and not schunks[0] else None
        empty_modes = b.modes() if modes and not mchunks[0] else None
        pair_sums = b.pair_dist_sums() if pairs else None
        grad_sums = [b.grad_stats_sums(k) for k in range(1 + len(_grad_bands(p0, gradients[3])))] if gradients else None  # [band][member]
        dens_sums = [b.dens_stats_sums(k) for k in range(1 + len(_dens_bands(p0, density[3])))] if density else None  # [band][member]
        members = []
        for m, prm in enumerate(prms):
            extra = {}
            if snapshots:
                extra.update(mid_profile_u=mids[m], full_profile_u=fulls[m])
            if average:
                extra.update(time_avg=time_average(prm, *[flow_stats_profile(prm.DH, **band[m]) for band in sums]))
            if history:
                extra.update(history=_concat_history(chunks[m]))
            if field:
                extra.update(field_avg=field_map_means(prm.DL, prm.DH, **planes[m]))
            if probe:
                extra.update(probes=_concat_probes(probe[0], prm.DL, pchunks[m]))
            if profiles:
                extra.update(profile_series=_concat_profile_series(prm.DH, schunks[m] or [empty_series[m]], f"member {m}: "))
            if pairs:
                extra.update(pair_dist=_pair_dist_bands(pair_sums[m], prm.dp))
            if gradients:
                extra.update(grad_stats=_grad_stats_bands(prm.DH, [band[m] for band in grad_sums]))
            if tracing:
                extra.update(tracers=_concat_tracers(tracing[0], tchunks[m]))
            if density:
                extra.update(dens_stats=_dens_stats_bands(prm, [band[m] for band in dens_sums]))
            if modes:
                extra.update(modes=_concat_modes(mchunks[m] or [empty_modes[m]]))
            members.append(_batch_member_result(b, m, prm, nf, nt, st, times, wall, policy, **extra))
    return members, wall, policy, sums, planes


def _pairs_request(pairs_from, pairs_every, pairs_bins, pairs_walls, pairs_bands):
    """the `pairs` of _run_batch: None without pairs_from"""
    return None if pairs_from is None else (pairs_from, pairs_every, pairs_bins, pairs_walls, pairs_bands)


def _gradients_request(gradients_from, gradients_every, gradients_walls, gradients_bands):
    """the `gradients` of _run_batch: None without gradients_from"""
    return None if gradients_from is None else (gradients_from, gradients_every, gradients_walls, gradients_bands)


def _field_request(field_from, field_every, field_shape, field_walls):
    """the `field` of _run_batch: None without field_from"""
    return None if field_from is None else (field_from, field_every, field_shape, field_walls)


def run_batch(prms, parts_list=None, engine="resident", lanes_per_particle=0, steps_per_graph=0, rebuild_every=0,
              restart_path=None, postprocess_path=None, average_from=None, log=None, history_every=None, field_from=None):
    """run() for M channels of one geometry stepped together as one batch (capi.Batch, include/sphx.h section 2b): a
    parameter sweep (mu, c_f, p0, gravity_g, transport_coeff) or an ensemble of realisations (parts_list).  Every member
    reaches the same output points (output_interval and t_end are shared and must agree) and gets a RunResult of its own:
    final profile and L2, the output-point profiles, tau.  The resident engine only; restart / post-process files are
    single-channel features, and time averaging of a batch is run_ensemble's."""
    if engine != "resident":
        raise ValueError("run_batch runs the resident engine only (a batch is device-resident)")
    if restart_path or postprocess_path:
        raise ValueError("run_batch writes no restart / post-process files (run() does, per channel)")
    if average_from is not None:
        raise ValueError("run_batch does no time averaging (run_ensemble and run_sweep do, for every member)")
    if history_every is not None:
        raise ValueError("run_batch records no step history (run_sweep does, for every member)")
    if field_from is not None:
        raise ValueError("run_batch accumulates no field map (run_ensemble and run_sweep do, for every member)")
    return _run_batch("run_batch", prms, parts_list, dict(lanes_per_particle=lanes_per_particle, steps_per_graph=steps_per_graph,
                                                          rebuild_every=rebuild_every), log, snapshots=True)[0]


@dataclass
class EnsembleResult:
    members: list        # one RunResult per member: final profile and L2, tau, time_avg (time_average of its own sums),
                         # field_avg (with field_from)
    pooled: dict         # members sharing mu, c_f, p0, gravity_g, transport_coeff: time_average of the pooled sums plus
                         # u_mean_se, L2_members, L2_mean, L2_std; None for a parameter sweep
    wall_seconds: float
    grid_policy: dict = field(default_factory=dict)
    pooled_field: dict = None  # with field_from, under the condition of `pooled`: profile.pool_field_maps of the members' planes
    pooled_pairs: list = None  # with pairs_from, under the condition of `pooled`: profile.pool_pair_dist of the members' sums, one
                               # dict per band, with the figures of profile.pair_dist_profiles
    pooled_grad: list = None   # with gradients_from, under the condition of `pooled`: profile.pool_grad_stats of the members' sums,
                               # one dict per band
    pooled_density: list = None  # with density_from, under the condition of `pooled`: profile.pool_dens_stats of the members' sums,
                                 # one dict per band
    pooled_tracers: dict = None  # with tracers, under the condition of `pooled` and where the members recorded at the same steps
                                 # and times (profile.pool_tracers refuses others): the members' columns side by side


_PHYSICS = ("mu", "c_f", "p0", "gravity_g", "transport_coeff")


def run_ensemble(prms, *, average_from, parts_list=None, average_every=1, lanes_per_particle=0, steps_per_graph=0,
                 rebuild_every=0, log=None, history_every=None, field_from=None, field_every=1, field_shape=None,
                 field_walls=False, pairs_from=None, pairs_every=1, pairs_bins=64, pairs_walls=False, pairs_bands=None,
                 gradients_from=None, gradients_every=1, gradients_walls=False, gradients_bands=None, tracers=None, tracers_every=1,
                 tracers_from=None, tracers_capacity=None, density_from=None, density_every=1, density_hist=(64, 0.05),
                 density_bands=None):
    """Time-averaged profiles of M channels of one geometry stepped as one batch (capi.Batch), averaged on the device
    inside the step loop (include/sphx.h section 2c) as run(average_from=...) does for one channel: every
    average_every-th step ending at t >= average_from, whole channel and the mid-channel band (DL/2, max(dp, h)).  The
    members advance output point by output point as in run_batch, so their trajectories are run_batch's; nothing is
    downloaded before the end.  parts_list: the members' initial states (e.g. geometry.perturbed_particles), default the
    lattice.  field_from: every member's velocity map as well (include/sphx.h section 2g), with the keywords of run(): every
    member gets a field_avg, and members that share their physics a pooled_field.  pairs_from: every member's pair statistics
    as well (include/sphx.h section 2m), with the keywords of run(): every member gets a pair_dist, and members that share their
    physics pooled_pairs (the integers added, the smallest r_min).  gradients_from: every member's gradient statistics as well
    (include/sphx.h section 2o), with the keywords of run(): every member gets a grad_stats, and members that share their physics
    pooled_grad (profile.pool_grad_stats, one dict per band).  tracers: every member's tracers as well (include/sphx.h section
    2q), with the keywords of run(): one id list for all members, every member gets its tracers, and members that share their
    physics and whose clocks agreed record by record pooled_tracers (profile.pool_tracers).  density_from: every member's density statistics as well
    (include/sphx.h section 2s), with the keywords of run(): every member gets a dens_stats, and members that share their physics
    pooled_density (profile.pool_dens_stats, one dict per band).  Returns an EnsembleResult."""
    prms = list(prms)
    if history_every is not None:
        raise ValueError("run_ensemble records no step history (run_sweep does, for every member)")
    if prms and (average_from is None or np.isnan(float(average_from))):  # (no parameter set: refused first, below)
        raise ValueError("run_ensemble needs average_from (the start of the averaging window)")
    members, wall, policy, (whole, mid), planes = _run_batch(
        "run_ensemble", prms, parts_list, dict(lanes_per_particle=lanes_per_particle, steps_per_graph=steps_per_graph,
                                               rebuild_every=rebuild_every), log, average=(average_from, average_every),
        field=_field_request(field_from, field_every, field_shape, field_walls),
        pairs=_pairs_request(pairs_from, pairs_every, pairs_bins, pairs_walls, pairs_bands),
        gradients=_gradients_request(gradients_from, gradients_every, gradients_walls, gradients_bands),
        tracers=None if tracers is None else (tracers, tracers_every, tracers_from, tracers_capacity),
        density=_density_request(density_from, density_every, density_hist, density_bands))
    p0, M = prms[0], len(prms)
    pooled = pooled_field = pooled_pairs = pooled_grad = pooled_tracers = pooled_density = None
    if all(getattr(p, k) == getattr(p0, k) for p in prms for k in _PHYSICS):
        pw, pm = pool_flow_stats(p0.DH, whole), pool_flow_stats(p0.DH, mid)
        pooled = time_average(p0, pw, pm)
        L2s = [r.time_avg["L2"] for r in members]
        pooled.update(u_mean_se=pw["u_mean_se"], L2_members=L2s, L2_mean=float(np.mean(L2s)),
                      L2_std=float(np.std(L2s, ddof=1)) if M > 1 else float("nan"))
        if planes is not None:
            pooled_field = pool_field_maps(p0.DL, p0.DH, planes)
        if pairs_from is not None:
            pooled_pairs = _pair_dist_bands(pool_pair_dist([r.pair_dist for r in members]), p0.dp)
        if gradients_from is not None:
            pooled_grad = [pool_grad_stats(p0.DH, [r.grad_stats[b] for r in members]) for b in range(len(members[0].grad_stats))]
        if tracers is not None and all(np.array_equal(r.tracers[k], members[0].tracers[k]) for r in members for k in ("step", "t")):
            pooled_tracers = pool_tracers([r.tracers for r in members])
        if density_from is not None:
            pooled_density = [pool_dens_stats(p0.DH, p0.p0, [r.dens_stats[b] for r in members]) for b in range(len(members[0].dens_stats))]
    return EnsembleResult(members=members, pooled=pooled, wall_seconds=wall, grid_policy=policy, pooled_field=pooled_field,
                          pooled_pairs=pooled_pairs, pooled_grad=pooled_grad, pooled_tracers=pooled_tracers,
                          pooled_density=pooled_density)


@dataclass
class SweepResult:
    members: list        # one RunResult per member: final profile and L2, tau, history (the whole run's series), time_avg
                         # (with average_from), field_avg (with field_from)
    table: dict          # [M] arrays: the _PHYSICS values, steps, every figure of history_figures(), n_dropped; with
                         # field_from also field_L2, field_x_spread, field_ix, field_uy_rms (field_figures of field_avg)
    wall_seconds: float
    grid_policy: dict = field(default_factory=dict)


def sweep_table(prms, histories, steps, history_from=0.0, settle_tol=0.05):
    """The table of a sweep: one [M] array per column -- the members' _PHYSICS values, their step counts, every figure of
    history_figures(prm_m, history_m, t_from=history_from, tol=settle_tol), and the records member m lost (n_dropped).  A
    member without a record at t >= history_from has NaN means and deviations."""
    figs = [history_figures(p, h, t_from=history_from, tol=settle_tol) for p, h in zip(prms, histories)]
    table = {k: np.array([float(getattr(p, k)) for p in prms]) for k in _PHYSICS}
    table["steps"] = np.array([int(n) for n in steps], dtype=np.int64)
    for k in (figs[0] if figs else ()):
        table[k] = np.array([f[k] for f in figs])
    table["n_dropped"] = np.array([int(h["n_dropped"]) for h in histories], dtype=np.int64)
    return table


_FIELD_COLUMNS = (("field_L2", "L2"), ("field_x_spread", "x_spread"), ("field_ix", "ix"), ("field_uy_rms", "uy_rms"))


def field_table(prms, field_avgs):
    """The field-map columns of a sweep's table, one [M] array each: field_L2, field_x_spread, field_ix, field_uy_rms =
    L2, x_spread, ix, uy_rms of field_figures(prm_m, field_avg_m)."""
    figs = [field_figures(p, f) for p, f in zip(prms, field_avgs)]
    return {col: np.array([f[k] for f in figs]) for col, k in _FIELD_COLUMNS}


def run_sweep(prms, *, history_every=1, history_capacity=65536, history_from=0.0, settle_tol=0.05, average_from=None,
              average_every=1, parts_list=None, lanes_per_particle=0, steps_per_graph=0, rebuild_every=0, log=None,
              field_from=None, field_every=1, field_shape=None, field_walls=False, probe_points=None, probe_every=1,
              probe_capacity=65536, probe_from=None, probe_walls=False, profiles_every=None, profiles_from=None,
              profiles_capacity=4096, profiles_bands=None, pairs_from=None, pairs_every=1, pairs_bins=64, pairs_walls=False,
              pairs_bands=None, gradients_from=None, gradients_every=1, gradients_walls=False, gradients_bands=None, tracers=None,
              tracers_every=1, tracers_from=None, tracers_capacity=None, density_from=None, density_every=1, density_hist=(64, 0.05),
              density_bands=None, modes_every=None, modes=(4, 8), modes_from=0.0, modes_capacity=4096):
    """A parameter sweep: M channels of one geometry that differ in mu, c_f, p0, gravity_g, transport_coeff, stepped as one
    batch (capi.Batch) with every member's step history recorded on the device, inside the step loop (include/sphx.h
    section 2f) as run(history_every=...) does for one channel.  The members advance output point by output point as in
    run_batch, so their trajectories are run_batch's; the record buffers (history_capacity records per member) are drained
    at every output point, so a capacity that holds one output interval suffices, and nothing else is downloaded before
    the end.  history_from: the start of the window the table's means are taken over (every history_every-th step of the
    whole run is recorded); settle_tol: the band of t_settled (history_figures).  average_from: the batch's flow
    statistics as well, as in run_ensemble -- every average_every-th step ending at t >= average_from -- and each member
    gets a time_avg.  field_from: every member's velocity map as well (include/sphx.h section 2g), with the keywords of
    run(): each member gets a field_avg and the table the columns field_L2, field_x_spread, field_ix, field_uy_rms of
    field_figures(prm_m, field_avg_m).  probe_points: every member's point probes as well (include/sphx.h section 2i), with
    the keywords of run(): one set of points for all members, and each member gets its probes.  profiles_every: every member's
    profile series as well (include/sphx.h section 2k), with the keywords of run(): each member gets its profile_series and the
    table the columns t_developed and tau_fit of profile_series_figures(prm_m, series_m).  pairs_from: every member's pair
    statistics as well (include/sphx.h section 2m), with the keywords of run(): each member gets its pair_dist and the table the
    columns r_min_dp, n_neigh, sigma1_dp of pair_dist_figures(prm_m, pair_dist_m) -- the figures that respond to
    transport_coeff.  gradients_from: every member's gradient statistics as well (include/sphx.h section 2o), with the keywords of
    run(): each member gets its grad_stats and the table the columns L2_shear, tau_wall_dev, div_rms of
    grad_figures(prm_m, grad_stats_m).  tracers: every member's tracers as well (include/sphx.h section 2q), with the keywords of
    run(): one id list for all members, each member gets its tracers and the table the columns D_y_nu, y_drift, u_dev_rms of
    tracer_figures(prm_m, tracers_m) -- the Lagrangian figures that respond to transport_coeff.  density_from: every member's density
    statistics as well (include/sphx.h section 2s), with the keywords of run(): each member gets its dens_stats and the table the
    columns delta_rms, delta_max, p_spread of density_figures(prm_m, dens_stats_m).  modes_every: every member's mode amplitudes
    as well (include/sphx.h section 2u), with the keywords of run(): each member gets its modes and the table the columns
    tau1_fit, tau3_fit, the decay times of the first two start-up modes of mode_figures(prm_m, modes_m) (NaN where modes[1]
    does not reach the mode).  A member that lost records to a full buffer raises RuntimeError, which names the member and the
    capacity the output interval needed.  Returns a SweepResult."""
    prms = list(prms)
    members, wall, policy, _, planes = _run_batch(
        "run_sweep", prms, parts_list, dict(lanes_per_particle=lanes_per_particle, steps_per_graph=steps_per_graph,
                                            rebuild_every=rebuild_every), log, history=(history_every, history_capacity),
        average=None if average_from is None else (average_from, average_every),
        field=_field_request(field_from, field_every, field_shape, field_walls),
        probe=None if probe_points is None else (probe_points, probe_every, probe_capacity, probe_from, probe_walls),
        profiles=None if profiles_every is None else (profiles_every, profiles_from, profiles_capacity, profiles_bands),
        pairs=_pairs_request(pairs_from, pairs_every, pairs_bins, pairs_walls, pairs_bands),
        gradients=_gradients_request(gradients_from, gradients_every, gradients_walls, gradients_bands),
        tracers=None if tracers is None else (tracers, tracers_every, tracers_from, tracers_capacity),
        density=_density_request(density_from, density_every, density_hist, density_bands),
        modes=None if modes_every is None else (modes_every, modes, modes_from, modes_capacity))
    table = sweep_table(prms, [r.history for r in members], [r.steps for r in members], history_from, settle_tol)
    if planes is not None:
        table.update(field_table(prms, [r.field_avg for r in members]))
    if profiles_every is not None:
        figs = [profile_series_figures(p, r.profile_series) for p, r in zip(prms, members)]
        table.update(t_developed=np.array([f["t_developed"] for f in figs]), tau_fit=np.array([f["tau_fit"] for f in figs]))
    if pairs_from is not None:
        figs = [pair_dist_figures(p, r.pair_dist) for p, r in zip(prms, members)]
        table.update({k: np.array([f[k] for f in figs]) for k in ("r_min_dp", "n_neigh", "sigma1_dp")})
    if gradients_from is not None:
        table.update(_grad_columns(prms, [r.grad_stats for r in members]))
    if tracers is not None:
        table.update(_tracer_columns(prms, [r.tracers for r in members]))
    if density_from is not None:
        table.update(_dens_columns(prms, [r.dens_stats for r in members]))
    if modes_every is not None:
        taus = [mode_figures(p, r.modes)["tau_fit"] for p, r in zip(prms, members)]
        table.update({f"tau{k}_fit": np.array([tf[k] if len(tf) > k else np.nan for tf in taus]) for k in (1, 3)})
    return SweepResult(members=members, table=table, wall_seconds=wall, grid_policy=policy)
