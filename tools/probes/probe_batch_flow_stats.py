"""Manual probe (not a test): what the flow statistics of a batch (include/sphx.h section 2c, k_flow_stats_b) cost per step
slot, beside what they cost a single context.
    python tools/probes/probe_batch_flow_stats.py [--members 1,16,64] [--modes off,1,10] [--steps N] [--reps R]
C2 (dp 0.025, DL 3; developed parabolic start, members jittered by their own seed, as probe_batch.py).  Per member count M:
warmed graphs, then R rounds; each round runs every mode once -- statistics off, every = 1, every = 10 (whole channel +
mid band, the reference's bins) -- as a warm-up enqueue_steps(N) + sync (enable / disable re-capture the graphs) and a
timed one around a host clock.  One JSON line per M: us per step slot of every round and mode, the medians, the ratio to
the slot without statistics and the cost of a sample per member, (us_every1 - us_off) / M.  A line for a standalone C2
context (M = 0 in the output) gives the single-context cost of a sample."""
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
capi, config, geometry, profile = pkg.capi, pkg.config, pkg.geometry, pkg.profile


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


def run_modes(obj, modes, steps, reps, n_bins, band):
    us = {m: [] for m in modes}
    for _ in range(reps):
        for mode in modes:
            if mode == "off":
                obj.flow_stats_disable()
            else:
                obj.flow_stats_enable(n_bins=n_bins, every=int(mode), bands=[band])
            obj.enqueue_steps(steps)  # warm: the graphs of this mode captured and replayed once
            obj.sync()
            t0 = time.perf_counter()
            obj.enqueue_steps(steps)
            obj.sync()
            us[mode].append(1e6 * (time.perf_counter() - t0) / steps)
    return us


def summary(M, nt, steps, us, extra):
    med = {m: statistics.median(v) for m, v in us.items()}
    out = dict(case="C2", members=M, n_total=nt, steps=steps, **extra,
               us_per_slot={m: [round(x, 2) for x in v] for m, v in us.items()},
               median_us={m: round(v, 2) for m, v in med.items()})
    if "off" in med:
        out["ratio_to_off"] = {m: round(v / med["off"], 4) for m, v in med.items() if m != "off"}
        out["sample_us_per_member"] = {m: round((v - med["off"]) / max(M, 1), 3) for m, v in med.items() if m != "off"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="1,16,64")
    ap.add_argument("--modes", default="off,1,10")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-single", action="store_true", help="skip the standalone context")
    a = ap.parse_args()
    modes = a.modes.split(",")
    prm = config.params_from_values(dp=0.025, DL=3.0)
    n_bins = profile.n_profile_bins(prm.DH, prm.dp)
    band = (0.5 * prm.DL, max(prm.dp, prm.h))
    if not a.no_single:
        s = member_state(prm, 1000)
        nt = s["n_total"]
        with capi.Context.from_parts(prm, s, t_end=1e9) as ctx:
            us = run_modes(ctx, modes, a.steps, a.reps, n_bins, band)
        print(json.dumps(summary(0, nt, a.steps, us, dict(standalone=True))), flush=True)
    for M in [int(x) for x in a.members.split(",")]:
        states = [member_state(prm, 1000 + m) for m in range(M)]
        nt = states[0]["n_total"]
        with capi.Batch.from_parts([prm] * M, states, t_end=1e9) as b:
            us = run_modes(b, modes, a.steps, a.reps, n_bins, band)
            info, gs = b.info(), b.graph_stats()
        print(json.dumps(summary(M, nt, a.steps, us, dict(lanes=info["lanes_per_particle"], realignments=info["realignments"],
                                                          slots_eager=gs["slots_eager"],
                                                          graphs_captured=gs["graphs_captured"]))), flush=True)


if __name__ == "__main__":
    main()
