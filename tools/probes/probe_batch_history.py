"""Manual probe (not a test): what the step history of a batch (include/sphx.h section 2f, k_step_history_b) costs per step
slot, beside what it costs a single context and beside the host-driven route it replaces.
    python tools/probes/probe_batch_history.py [--dp 0.025,0.04] [--members 1,16,64] [--modes off,1,16] [--steps N] [--reps R]
    SPHX_LIB=tools/_exp/libsphx_<tag>.so python tools/probes/probe_batch_history.py --off-only ...   # an earlier library
Channels of DL 3 at each dp (0.025 is C2; developed parabolic start, members jittered by their own seed, as
probe_batch_flow_stats.py).  Per dp and member count M: warmed graphs, then R rounds; each round runs every mode once --
history off, every = 1, every = 16 -- as a warm-up enqueue_steps(N) + sync (enable / disable re-capture the graphs) and a
timed one around a host clock.  One JSON line per (dp, M): us per step slot of every round and mode, the medians, the
round-to-round spread (max - min) of every mode, the ratio to the slot without history, the cost of a record per member,
(us_every1 - us_off) / M, and the host-driven route: advance(max_steps=1) + monitor() of every member, per step.  A line for
a standalone context (M = 0 in the output) gives the single-context figures.  --off-only times the "off" rounds alone,
which is all a library from before the batch history can do."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("sph-poiseuille-flow_amd")
capi, config, geometry = pkg.capi, pkg.config, pkg.geometry


def member_state(prm, seed):
    parts = geometry.init_particles(prm)
    nf = parts["n_fluid"]
    rng = np.random.default_rng(seed)
    pos = parts["pos"].copy(order="F")
    pos[:nf] += (rng.random((nf, 2)) * 2 - 1) * 0.05 * prm.dp
    pos[:nf, 0] = np.mod(pos[:nf, 0], prm.DL)
    vel = parts["vel"].copy(order="F")
    y = pos[:nf, 1]
    vel[:nf, 0] = prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y)
    return dict(parts, pos=pos, vel=vel)


def run_modes(obj, modes, steps, reps, capacity):
    us = {m: [] for m in modes}
    for _ in range(reps):
        for mode in modes:
            if mode != "off":
                obj.history_enable(every=int(mode), capacity=capacity)
            elif len(modes) > 1:
                obj.history_disable()
            obj.enqueue_steps(steps)  # warm: the graphs of this mode captured and replayed once
            obj.sync()
            t0 = time.perf_counter()
            obj.enqueue_steps(steps)
            obj.sync()
            us[mode].append(1e6 * (time.perf_counter() - t0) / steps)
    return us


def host_driven(obj, members, steps):
    """the route the history replaces: one step, then the wall shear of every member through the host"""
    t0 = time.perf_counter()
    for _ in range(steps):
        obj.advance(1e9, max_steps=1)
        if members:
            for m in range(members):
                obj.monitor(m, tau=True)
        else:
            obj.monitor(tau=True)
    return 1e6 * (time.perf_counter() - t0) / steps


def summary(dp, M, nt, steps, us, extra):
    med = {m: statistics.median(v) for m, v in us.items()}
    out = dict(dp=dp, members=M, n_total=nt, steps=steps, library=capi.LIB_PATH, **extra,
               us_per_slot={m: [round(x, 2) for x in v] for m, v in us.items()},
               median_us={m: round(v, 2) for m, v in med.items()},
               spread_us={m: round(max(v) - min(v), 2) for m, v in us.items()})
    if "off" in med and len(med) > 1:
        out["ratio_to_off"] = {m: round(v / med["off"], 4) for m, v in med.items() if m != "off"}
        out["record_us_per_member"] = {m: round((v - med["off"]) / max(M, 1), 3) for m, v in med.items() if m != "off"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dp", default="0.025,0.04")
    ap.add_argument("--members", default="1,16,64")
    ap.add_argument("--modes", default="off,1,16")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=100, help="steps of the host-driven route (0: skip it)")
    ap.add_argument("--no-single", action="store_true", help="skip the standalone context")
    ap.add_argument("--off-only", action="store_true", help="time the slots without the history only (earlier libraries)")
    a = ap.parse_args()
    modes = ["off"] if a.off_only else a.modes.split(",")
    capacity = 2 * a.steps + 64  # (a mode's warm-up and its timed round; enable empties the buffer)
    for dp in [float(x) for x in a.dp.split(",")]:
        prm = config.params_from_values(dp=dp, DL=3.0)
        if not a.no_single:
            s = member_state(prm, 1000)
            nt = s["n_total"]
            with capi.Context.from_parts(prm, s, t_end=1e9) as ctx:
                us = run_modes(ctx, modes, a.steps, a.reps, capacity)
                extra = dict(standalone=True)
                if not a.off_only:
                    ctx.history_disable()
                    if a.host_steps:
                        extra["host_driven_us"] = round(host_driven(ctx, 0, a.host_steps), 2)
                    ctx.history_enable(every=1, capacity=64)  # the kernel's own time: eager launches between HIP events
                    ctx.profile_enable(True)
                    ctx.advance(1e9, max_steps=50)
                    prof = ctx.profile_read()
                    ctx.profile_enable(False)
                    extra["k_step_history_us"] = round(1e3 * prof.get("k_step_history", {}).get("avg_ms", float("nan")), 3)
            print(json.dumps(summary(dp, 0, nt, a.steps, us, extra)), flush=True)
        for M in [int(x) for x in a.members.split(",")]:
            states = [member_state(prm, 1000 + m) for m in range(M)]
            nt = states[0]["n_total"]
            with capi.Batch.from_parts([prm] * M, states, t_end=1e9) as b:
                us = run_modes(b, modes, a.steps, a.reps, capacity)
                extra = {}
                if not a.off_only:
                    n_rec = [len(h["step"]) for h in b.history()]
                    extra["records_last_mode"] = [min(n_rec), max(n_rec)]
                    b.history_disable()
                    if a.host_steps:
                        extra["host_driven_us"] = round(host_driven(b, M, a.host_steps), 2)
                info, gs = b.info(), b.graph_stats()
            print(json.dumps(summary(dp, M, nt, a.steps, us, dict(extra, lanes=info["lanes_per_particle"],
                                                                   realignments=info["realignments"],
                                                                   slots_eager=gs["slots_eager"],
                                                                   graphs_captured=gs["graphs_captured"]))), flush=True)


if __name__ == "__main__":
    main()
