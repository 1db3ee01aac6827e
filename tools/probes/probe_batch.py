"""Manual probe (not a test): the aggregate rate of a batched context (include/sphx.h section 2b) against one standalone context.
    python tools/probes/probe_batch.py [--case C2 --case dp04] [--members 1,2,4,...] [--steps N] [--reps R] [--call S]
Per case (C2 = dp 0.025, DL 3; dp04 = dp 0.04, DL 3; developed parabolic start, members jittered by their own seed) and
member count M: warmed graphs, then R timed rounds of enqueue_steps(N) + sync around a host clock, standalone and batch
alternating.  Rate = M * n_total * N / seconds (particle-steps/s).  One JSON line per (case, M): the rounds, their median,
and the ratio of the batch's median aggregate rate to the standalone's.  --call S enqueues the N steps of a round in calls of S
steps: below the shortest graph (4 steps) every slot is launched eagerly, which is where host time per launch shows."""
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

CASES = {"C2": dict(dp=0.025, DL=3.0), "dp04": dict(dp=0.04, DL=3.0)}


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


def rounds(obj, steps, reps, sink, call):
    def enqueue():
        for _ in range(steps // call):
            obj.enqueue_steps(call)
        obj.sync()

    enqueue()  # warm: graphs captured and replayed once
    for _ in range(reps):
        t0 = time.perf_counter()
        enqueue()
        sink.append(time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--members", default="1,2,4,8,16,32,64,256")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--call", type=int, default=0, help="steps per enqueue_steps call (0: one call per round); must divide --steps")
    a = ap.parse_args()
    call = a.call or a.steps
    assert a.steps % call == 0, "--call must divide --steps"
    for name in a.case or ["C2", "dp04"]:
        prm = config.params_from_values(**CASES[name])
        for M in [int(x) for x in a.members.split(",")]:
            states = [member_state(prm, 1000 + m) for m in range(M)]
            nt = states[0]["n_total"]
            single, batch = [], []
            with capi.Context.from_parts(prm, states[0], t_end=1e9) as ctx, \
                    capi.Batch.from_parts([prm] * M, states, t_end=1e9) as b:
                for _ in range(2):  # alternate, so that drifts of the clock or of the box hit both
                    rounds(ctx, a.steps, (a.reps + 1) // 2, single, call)
                    rounds(b, a.steps, (a.reps + 1) // 2, batch, call)
                info, gs = b.info(), b.graph_stats()
            work = nt * a.steps
            r1 = [work / s for s in single]
            rM = [M * work / s for s in batch]
            print(json.dumps(dict(case=name, n_total=nt, members=M, steps=a.steps, call=call, lanes=info["lanes_per_particle"],
                                  rebuild_every=info["rebuild_every"], realignments=info["realignments"],
                                  forced_rebuilds=info["forced_rebuilds"], slots_eager=gs["slots_eager"],
                                  single_us_per_step=[round(1e6 * s / a.steps, 3) for s in single],
                                  batch_us_per_step=[round(1e6 * s / a.steps, 3) for s in batch],
                                  single_rate=statistics.median(r1), batch_rate=statistics.median(rM),
                                  batch_rate_min=min(rM), batch_rate_max=max(rM),
                                  ratio=statistics.median(rM) / statistics.median(r1))), flush=True)


if __name__ == "__main__":
    main()
