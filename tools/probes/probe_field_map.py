"""Manual probe (not a test): what the device-side field map (include/sphx.h section 2e) costs.
    python tools/probes/probe_field_map.py --workload C2 --workload C4 [--steps 400] [--rounds 7]
    python tools/probes/probe_field_map.py --workload C2 --modes off            # one library's "off" figure (SPHX_LIB=...)
    python tools/probes/probe_field_map.py --workload C2 --trace-steps 200      # nothing timed: steps for a kernel trace
Per workload (bench.py's channels, developed parabolic start): us per step slot of replayed batches with the map off, with
every = 1 and with every = 10 (the reference's grid shape), the modes alternating over the rounds, every batch prepared
first so that it is pure replay (enqueue_steps + sync); the per-launch time of k_field_map from sphx_ctx_profile_read
(eager, HIP events); and what the host route costs for the same shape: a download of pos and vel plus
profile.shepard_field.  One JSON line each."""
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
capi, config, geometry, profile = pkg.capi, pkg.config, pkg.geometry, pkg.profile

MODES = {"off": None, "every1": 1, "every10": 10}


def developed_state(prm):
    parts = geometry.init_particles(prm)
    nf = parts["n_fluid"]
    vel = parts["vel"].copy(order="F")
    y = parts["pos"][:nf, 1]
    vel[:nf, 0] = prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y)
    return dict(parts, vel=vel)


def set_mode(ctx, mode):
    has_map = hasattr(ctx, "field_map_enable")  # (a library from before the feature: "off" only)
    if MODES[mode] is None:
        if has_map and ctx._field_map is not None:
            ctx.field_map_disable()
    else:
        ctx.field_map_enable(every=MODES[mode])


def timed(ctx, steps):
    ctx.prepare_steps(steps)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.enqueue_steps(steps)
    ctx.sync()
    return 1e6 * (time.perf_counter() - t0) / steps


def probe(name, steps, rounds, warm, modes, trace_steps, host_nodes):
    _, kw = bench.parse_workload(name)
    prm = config.params_from_values(end_time=1e9, output_interval=1e9, **kw)
    parts = developed_state(prm)
    nf, nt = parts["n_fluid"], parts["n_total"]
    nx, ny = capi.field_map_shape(prm)
    out = dict(workload=name, n_fluid=nf, n_total=nt, nx=nx, ny=ny, steps=steps, rounds=rounds, lib=capi.LIB_PATH,
               us={m: [] for m in modes})
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.advance(1e9, max_steps=warm)
        if trace_steps:
            ctx.field_map_enable(every=1)
            ctx.enqueue_steps(trace_steps)
            ctx.sync()
            out["traced_steps"] = trace_steps
            return out
        for m in modes:  # every mode's graphs captured and replayed once before anything is timed
            set_mode(ctx, m)
            timed(ctx, steps)
        for _ in range(rounds):
            for m in modes:
                set_mode(ctx, m)
                out["us"][m].append(timed(ctx, steps))
        if "every1" in modes:
            set_mode(ctx, "every1")
            ctx.profile_enable(True)
            ctx.advance(1e9, max_steps=50)
            prof = ctx.profile_read()
            ctx.profile_enable(False)
            out["k_field_map_us"] = 1e3 * prof.get("k_field_map", {}).get("avg_ms", float("nan"))
            out["kernels_us"] = {k: round(1e3 * v["avg_ms"], 2) for k, v in prof.items()}
            # the host route: download, then the same interpolation in numpy (on host_nodes nodes, scaled to all)
            t0 = time.perf_counter()
            d = ctx.download(fields=("pos", "vel"))
            out["host_download_ms"] = 1e3 * (time.perf_counter() - t0)
            nodes = None if nx * ny <= host_nodes else np.random.default_rng(0).choice(nx * ny, host_nodes, replace=False)
            t0 = time.perf_counter()
            profile.shepard_field(d["pos"][:nf], d["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny, nodes=nodes)
            scale = 1.0 if nodes is None else nx * ny / host_nodes
            out["host_shepard_ms"] = 1e3 * (time.perf_counter() - t0) * scale
            out["host_shepard_extrapolated"] = nodes is not None
        out["tuning"] = ctx.tuning()
        out["schedule"] = ctx.schedule()
    out["us_median"] = {m: float(np.median(v)) for m, v in out["us"].items()}
    out["us_spread"] = {m: [float(np.min(v)), float(np.max(v))] for m, v in out["us"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=[])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--modes", default="off,every1,every10")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--host-nodes", type=int, default=4800)
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    assert all(m in MODES for m in modes), modes
    for name in a.workload or ["C2"]:
        print(json.dumps(probe(name, a.steps, a.rounds, a.warm, modes, a.trace_steps, a.host_nodes)), flush=True)


if __name__ == "__main__":
    main()
