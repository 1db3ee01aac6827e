"""Manual probe (not a test): what the device-side flow statistics (include/sphx.h section 2a) cost, and what they measure.
    python tools/probes/probe_flow_stats.py --workload C2 --workload C5 [--steps K] [--reps R]
    python tools/probes/probe_flow_stats.py --workload C5 --t-end 20 --average-from 16     # the long-run record
Per workload (bench.py's channels, developed parabolic start): us/step of replayed batches with the statistics off and on
(every = 1, whole channel + mid band), alternating R times, each batch prepared first so that it is pure replay; the
per-launch time of k_flow_stats from sphx_ctx_profile_read (eager, HIP events); and the L2 of the time-averaged profile.
With --t-end: driver.run to that time with average_from instead (the figures of RunResult.time_avg).  One JSON line each."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (workload table)

pkg = importlib.import_module(bench.PKG)
capi, config, geometry, driver, profile = pkg.capi, pkg.config, pkg.geometry, pkg.driver, pkg.profile


def developed_state(prm):
    parts = geometry.init_particles(prm)
    nf = parts["n_fluid"]
    vel = parts["vel"].copy(order="F")
    y = parts["pos"][:nf, 1]
    vel[:nf, 0] = prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y)
    return dict(parts, vel=vel)


def timed(ctx, steps):
    ctx.prepare_steps(steps)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.enqueue_steps(steps)
    ctx.sync()
    return 1e6 * (time.perf_counter() - t0) / steps


def probe(name, steps, reps, warm):
    _, kw = bench.parse_workload(name)
    prm = config.params_from_values(end_time=1e9, output_interval=1e9, **kw)
    parts = developed_state(prm)
    nf, nt = parts["n_fluid"], parts["n_total"]
    n_bins = profile.n_profile_bins(prm.DH, prm.dp)
    band = (0.5 * prm.DL, max(prm.dp, prm.h))
    out = dict(workload=name, n_fluid=nf, n_total=nt, n_bins=n_bins, steps=steps, reps=reps, us_off=[], us_on=[])
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.advance(1e9, max_steps=warm)
        for _ in range(reps):
            ctx.flow_stats_disable()
            out["us_off"].append(timed(ctx, steps))
            ctx.flow_stats_enable(n_bins=n_bins, every=1, bands=[band])
            out["us_on"].append(timed(ctx, steps))
        ta = driver.time_average(prm, ctx.flow_stats(0), ctx.flow_stats(1))
        ctx.profile_enable(True)
        ctx.advance(1e9, max_steps=min(steps, 50))
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        out["tuning"] = ctx.tuning()
        out["schedule"] = ctx.schedule()
    out["us_off_median"] = float(np.median(out["us_off"]))
    out["us_on_median"] = float(np.median(out["us_on"]))
    out["k_flow_stats_us"] = 1e3 * prof.get("k_flow_stats", {}).get("avg_ms", float("nan"))
    out["kernels_us"] = {k: round(1e3 * v["avg_ms"], 2) for k, v in prof.items()}
    out["time_avg"] = dict(L2=ta["L2"], n_samples=ta["n_samples"], t_first=ta["t_first"], t_last=ta["t_last"],
                           uy_rms_over_umax=ta["uy_rms_over_umax"], ux_std_centre_over_umax=ta["ux_std_centre_over_umax"])
    return out


def long_run(name, t_end, average_from, every):
    _, kw = bench.parse_workload(name)
    prm = config.params_from_values(end_time=t_end, output_interval=max(t_end / 20, 1e-3), **kw)
    t0 = time.perf_counter()
    res = driver.run(prm, average_from=average_from, average_every=every)
    ta = res.time_avg
    return dict(workload=name, t_end=t_end, average_from=average_from, every=every, steps=res.steps, t=res.t,
                wall_seconds=time.perf_counter() - t0, L2_final=res.L2_error, L2_five_snapshots=res.L2_time_mean(),
                time_avg={k: ta[k] for k in ("L2", "uy_rms_over_umax", "ux_std_centre_over_umax", "n_samples", "t_first",
                                             "t_last")}, tau_bottom=res.tau_bottom, tau_top=res.tau_top, tau_target=res.tau_target)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=[])
    ap.add_argument("--steps", type=int, default=0, help="steps per timed batch (0: 2000 below 10^5 particles, else 100)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--t-end", type=float, default=0.0)
    ap.add_argument("--average-from", type=float, default=None)
    ap.add_argument("--every", type=int, default=1)
    a = ap.parse_args()
    for name in a.workload or ["C2"]:
        if a.t_end > 0:
            r = long_run(name, a.t_end, a.t_end * 0.8 if a.average_from is None else a.average_from, a.every)
        else:
            nf_guess = bench.parse_workload(name)[1]
            n_est = nf_guess["DL"] / nf_guess["dp"] / nf_guess["dp"]
            r = probe(name, a.steps or (2000 if n_est < 1e5 else 100), a.reps, a.warm)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
