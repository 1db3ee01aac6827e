"""Manual probe (not a test): what the device-side point probes (include/sphx.h sections 2h / 2i) cost.
    python tools/probes/probe_point_probes.py --workload C2 [--steps 400] [--rounds 3] [--members 16]
    python tools/probes/probe_point_probes.py --workload C2 --points 0            # one library's "off" figure (SPHX_LIB=...)
Per workload (bench.py's channels, developed parabolic start), on a standalone context and on a batch of --members members:
us per step slot of replayed batches with the probes off and with every = 1 at P = 1, 16, 256 and 4096 random points, off and
on alternating over the rounds, every batch prepared first so that it is pure replay (enqueue_steps + sync); on the context
also the per-launch times of k_point_probes and, for comparison, of k_field_map on the reference's grid, from
sphx_ctx_profile_read (eager, HIP events).  One JSON line per (channel kind, P)."""
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


def timed(ch, steps):
    if hasattr(ch, "prepare_steps"):
        ch.prepare_steps(steps)
    ch.sync()
    t0 = time.perf_counter()
    ch.enqueue_steps(steps)
    ch.sync()
    return 1e6 * (time.perf_counter() - t0) / steps


def set_mode(ch, pts):
    has = hasattr(ch, "probes_enable")  # (a library from before the feature: "off" only)
    if pts is None:
        if has and ch._probes is not None:
            ch.probes_disable()
    else:
        ch.probes_enable(pts, every=1, capacity=512)  # (16 members x 512 x 4096 points x 4 is the library's 1 << 27 doubles)


def measure(ch, pts, steps, rounds):
    us = {"off": [], "on": []}
    modes = [("off", None)] + ([("on", pts)] if pts is not None else [])
    for _, p in modes:  # every mode's graphs captured and replayed once before anything is timed
        set_mode(ch, p)
        timed(ch, steps)
    for _ in range(rounds):
        for m, p in modes:
            set_mode(ch, p)   # (enable empties the buffer: steps <= capacity, nothing is dropped)
            us[m].append(timed(ch, steps))
    return {m: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for m, v in us.items() if v}


def probe(name, steps, rounds, warm, members, counts):
    _, kw = bench.parse_workload(name)
    prm = config.params_from_values(end_time=1e9, output_interval=1e9, **kw)
    parts = developed_state(prm)
    rng = np.random.default_rng(0)
    for kind in ("context", "batch"):
        if kind == "context":
            ch = capi.Context.from_parts(prm, parts, t_end=1e9)
        else:
            ch = capi.Batch.from_parts([prm] * members, [parts] * members, t_end=1e9)
        with ch:
            ch.advance(1e9, max_steps=warm)
            for P in counts:
                pts = np.column_stack([rng.random(P) * prm.DL, rng.random(P) * prm.DH]) if P else None
                out = dict(workload=name, kind=kind, members=members if kind == "batch" else 1, n_fluid=parts["n_fluid"], P=P,
                           steps=steps, rounds=rounds, lib=capi.LIB_PATH, us=measure(ch, pts, steps, rounds))
                if kind == "context" and P:
                    set_mode(ch, pts)
                    ch.field_map_enable(every=1)
                    ch.profile_enable(True)
                    ch.advance(1e9, max_steps=50)
                    prof = ch.profile_read()
                    ch.profile_enable(False)
                    ch.field_map_disable()
                    out["k_point_probes_us"] = round(1e3 * prof.get("k_point_probes", {}).get("avg_ms", float("nan")), 2)
                    out["k_field_map_us"] = round(1e3 * prof.get("k_field_map", {}).get("avg_ms", float("nan")), 2)
                print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=[])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--points", default="1,16,256,4096")
    a = ap.parse_args()
    counts = [int(p) for p in a.points.split(",") if p]
    for name in a.workload or ["C2"]:
        probe(name, a.steps, a.rounds, a.warm, a.members, counts)


if __name__ == "__main__":
    main()
