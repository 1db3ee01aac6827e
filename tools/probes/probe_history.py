"""Manual probe (not a test): what the device-side step history (include/sphx.h section 2d) costs.
    python tools/probes/probe_history.py --workload C2 --workload dp=0.01,DL=3 [--steps K] [--reps R]
    SPHX_LIB=tools/_exp/libsphx_<tag>.so python tools/probes/probe_history.py --off-only ...   # an earlier library (tools/build_baseline_lib.sh)
Per workload (bench.py's channels, developed parabolic start): us/step of replayed batches with the history off, with
every = 1 and with every = 16, alternating R times, each batch prepared first so that it is pure replay (min / median / max
over the R batches: the spread the comparison has to be read against); us/step of the host-driven series the history
replaces, advance(max_steps=1) + monitor() per step; the per-launch time of k_step_history from sphx_ctx_profile_read (eager,
HIP events); and the last record against monitor().  --off-only times the "off" batches alone, which is all a library from
before the history can do.  One JSON line each."""
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
capi, config, geometry = pkg.capi, pkg.config, pkg.geometry


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


def host_driven(ctx, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.advance(1e9, max_steps=1)
        ctx.monitor(tau=True)
    return 1e6 * (time.perf_counter() - t0) / steps


def spread(v):
    return dict(min=round(float(np.min(v)), 3), median=round(float(np.median(v)), 3), max=round(float(np.max(v)), 3))


def probe(name, steps, reps, warm, off_only):
    _, kw = bench.parse_workload(name)
    prm = config.params_from_values(end_time=1e9, output_interval=1e9, **kw)
    parts = developed_state(prm)
    nf, nt = parts["n_fluid"], parts["n_total"]
    capacity = min(1 << 22, reps * steps + 64)
    us = dict(off=[], every1=[], every16=[], host_driven=[])
    out = dict(workload=name, library=capi.LIB_PATH, n_fluid=nf, n_total=nt, steps=steps, reps=reps)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.advance(1e9, max_steps=warm)
        for _ in range(reps):
            if not off_only:
                ctx.history_disable()
            us["off"].append(timed(ctx, steps))
            if off_only:
                continue
            ctx.history_enable(every=1, capacity=capacity)
            us["every1"].append(timed(ctx, steps))
            ctx.history_enable(every=16, capacity=capacity)
            us["every16"].append(timed(ctx, steps))
        if not off_only:
            ctx.history_disable()
            for _ in range(reps):
                us["host_driven"].append(host_driven(ctx, min(steps, 1000)))
            ctx.history_enable(every=1, capacity=256)
            ctx.profile_enable(True)
            ctx.advance(1e9, max_steps=min(steps, 50))
            prof = ctx.profile_read()
            ctx.profile_enable(False)
            hist = ctx.history()
            tb, tt, _ = ctx.monitor(tau=True)
            out["k_step_history_us"] = round(1e3 * prof.get("k_step_history", {}).get("avg_ms", float("nan")), 3)
            out["kernels_us"] = {k: round(1e3 * v["avg_ms"], 2) for k, v in prof.items() if v["launches"] > 0}
            out["last_record"] = {k: float(hist[k][-1]) for k in capi.HISTORY_FIELDS}
            out["last_tau_vs_monitor"] = [abs(hist["tau_bottom"][-1] - tb) / abs(tb), abs(hist["tau_top"][-1] - tt) / abs(tt)]
        out["tuning"] = ctx.tuning()
        out["schedule"] = ctx.schedule()
    out["us_per_step"] = {k: spread(v) for k, v in us.items() if v}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=[])
    ap.add_argument("--steps", type=int, default=2000, help="steps per timed batch")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--off-only", action="store_true", help="time the batches without the history only (earlier libraries)")
    a = ap.parse_args()
    for name in a.workload or ["C2"]:
        print(json.dumps(probe(name, a.steps, a.reps, a.warm, a.off_only)), flush=True)


if __name__ == "__main__":
    main()
