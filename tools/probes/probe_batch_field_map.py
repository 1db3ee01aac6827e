"""Manual probe (not a test): what the field maps of a batch (include/sphx.h section 2g, k_field_map_b) cost per step slot,
beside what a map costs a single context.
    python tools/probes/probe_batch_field_map.py [--members 1,16,64] [--modes off,1,10] [--steps N] [--reps R]
    SPHX_LIB=tools/_exp/libsphx_<tag>.so python tools/probes/probe_batch_field_map.py --modes off   # an earlier library's slot
C2 (dp 0.025, DL 3, the default map of 240 x 80 nodes; developed parabolic start, members jittered by their own seed, as
probe_batch_flow_stats.py).  Per member count M: warmed graphs, then R rounds; each round runs every mode once -- map off,
every = 1, every = 10 -- as a warm-up enqueue_steps(N) + sync (enable / disable re-capture the graphs) and a timed one
around a host clock.  One JSON line per M: us per step slot of every round and mode, the medians and the spread of the
rounds, the ratio to the slot without a map and the cost of a sample per member, (us_every1 - us_off) / M.  A line for a
standalone C2 context (members = 0 in the output) gives the single-context cost of a sample.  With --modes off nothing of
the map's interface is touched, so a library from before the feature can be timed through SPHX_LIB."""
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


def run_modes(obj, modes, steps, reps):
    us = {m: [] for m in modes}
    samples = {}
    for _ in range(reps):
        for mode in modes:
            if mode != "off":
                obj.field_map_enable(every=int(mode))
            elif obj._field_map is not None:
                obj.field_map_disable()
            obj.enqueue_steps(steps)  # warm: the graphs of this mode captured and replayed once
            obj.sync()
            t0 = time.perf_counter()
            obj.enqueue_steps(steps)
            obj.sync()
            us[mode].append(1e6 * (time.perf_counter() - t0) / steps)
            if mode != "off":  # what was sampled in the two windows: 2 * steps / every samples a channel
                sums = obj.field_map_sums()
                samples[mode] = [s["n_samples"] for s in (sums if isinstance(sums, list) else [sums])][:4]
    return us, samples


def summary(M, nt, steps, us, extra):
    med = {m: statistics.median(v) for m, v in us.items()}
    out = dict(case="C2", members=M, n_total=nt, steps=steps, lib=os.path.basename(capi.LIB_PATH), **extra,
               us_per_slot={m: [round(x, 2) for x in v] for m, v in us.items()},
               median_us={m: round(v, 2) for m, v in med.items()},
               spread_us={m: round(max(v) - min(v), 2) for m, v in us.items()})
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
    if not a.no_single:
        s = member_state(prm, 1000)
        nt = s["n_total"]
        with capi.Context.from_parts(prm, s, t_end=1e9) as ctx:
            us, samples = run_modes(ctx, modes, a.steps, a.reps)
        print(json.dumps(summary(0, nt, a.steps, us, dict(standalone=True, n_samples=samples))), flush=True)
    for M in [int(x) for x in a.members.split(",") if x]:
        states = [member_state(prm, 1000 + m) for m in range(M)]
        nt = states[0]["n_total"]
        with capi.Batch.from_parts([prm] * M, states, t_end=1e9) as b:
            us, samples = run_modes(b, modes, a.steps, a.reps)
            info, gs = b.info(), b.graph_stats()
        print(json.dumps(summary(M, nt, a.steps, us, dict(lanes=info["lanes_per_particle"], realignments=info["realignments"],
                                                          slots_eager=gs["slots_eager"], graphs_captured=gs["graphs_captured"],
                                                          n_samples=samples))), flush=True)


if __name__ == "__main__":
    main()
