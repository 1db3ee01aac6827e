"""Manual probe (not a test): what the device-side particle tracers (include/sphx.h sections 2p / 2q) cost.
    python tools/probes/probe_tracers.py --workload C2 --workload dp=0.005,DL=6 [--steps 256] [--rounds 3]
    python tools/probes/probe_tracers.py --workload C2 --tracers ""              # the "never enabled" figure alone
Per workload (bench.py's channels, developed parabolic start), on a standalone context: us per step slot of replayed batches
with the sampler never enabled and with T = 1, 4 096 and n_fluid tracers at every = 1 and every = 16, in alternating lines:
each "on" line is followed by an "off" line of the same context (tracers_disable: the launches of a context that never enabled
them, which tests/test_gpu_tracers.py::test_off_means_no_extra_launch asserts), every batch prepared first so that it is pure
replay (enqueue_steps + sync); also the per-launch time of k_tracers from sphx_ctx_profile_read (eager, HIP events).  The first
line of a workload is a context on which the sampler was never enabled.  One JSON line per (T, every)."""
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
    ch.prepare_steps(steps)
    ch.sync()
    t0 = time.perf_counter()
    ch.enqueue_steps(steps)
    ch.sync()
    return 1e6 * (time.perf_counter() - t0) / steps


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def probe(name, steps, rounds, warm, counts, everies):
    _, kw = bench.parse_workload(name)
    prm = config.params_from_values(end_time=1e9, output_interval=1e9, **kw)
    parts = developed_state(prm)
    nf = parts["n_fluid"]
    rng = np.random.default_rng(0)
    base = dict(workload=name, n_fluid=nf, steps=steps, rounds=rounds, lib=capi.LIB_PATH)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ch:      # the sampler never enabled
        ch.advance(1e9, max_steps=warm)
        timed(ch, steps)
        print(json.dumps(dict(base, T=0, every=0, us=dict(never=stats([timed(ch, steps) for _ in range(rounds)])))), flush=True)
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ch:
        ch.advance(1e9, max_steps=warm)
        for T in counts:
            T = nf if T <= 0 else min(T, nf)
            ids = np.sort(rng.choice(nf, size=T, replace=False))
            for every in everies:
                cap = max(min(steps // every + 1, (1 << 27) // (4 * T)), 1)   # (records beyond the capacity are dropped: the scan still runs)
                us = {"on": [], "off": []}
                for _ in range(rounds + 1):                           # the first round captures and replays once, untimed
                    ch.tracers_enable(ids, every=every, capacity=cap)
                    on = timed(ch, steps)
                    ch.tracers_disable()
                    off = timed(ch, steps)
                    if _:
                        us["on"].append(on)
                        us["off"].append(off)
                out = dict(base, T=T, every=every, capacity=cap, us={k: stats(v) for k, v in us.items()})
                ch.tracers_enable(ids, every=every, capacity=cap)
                ch.profile_enable(True)
                ch.advance(1e9, max_steps=48)
                prof = ch.profile_read()
                ch.profile_enable(False)
                ch.tracers_disable()
                out["k_tracers_us"] = round(1e3 * prof.get("k_tracers", {}).get("avg_ms", float("nan")), 2)
                print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", default=[])
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--tracers", default="1,4096,0", help="tracer counts, 0 = every fluid row")
    ap.add_argument("--every", default="1,16")
    a = ap.parse_args()
    counts = [int(p) for p in a.tracers.split(",") if p]
    everies = [int(p) for p in a.every.split(",") if p]
    for name in a.workload or ["C2"]:
        probe(name, a.steps, a.rounds, a.warm, counts, everies)


if __name__ == "__main__":
    main()
