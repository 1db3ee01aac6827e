"""Child process of tests/test_gpu_rebin_fold.py: SPHX_DEBUG_SWITCHES is read once per process, so the folded re-binning step
and today's chain (no_fold_rebin) each run in a fresh one.  Steps one case, writes what download() returns to --out (npz) and
prints ONE JSON line: the clock after the last step, the schedule, the re-binnings carried out and the launches a profiled
stretch listed (the compared run itself when --mode profile, else 20 eager steps taken AFTER the download).  Exit code 0: ran
to the end.

    SPHX_DEBUG_SWITCHES=no_fold_rebin python tests/rebin_fold_worker.py --case c2 --mode graph --out /tmp/a.npz
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    sys.path.insert(0, p)

STEPS = {"c2": 56, "c1": 56, "variant": 50, "three": 50, "two": 6}


def make_state(pkg, case):
    """(prm, parts, pos, vel) of one case"""
    from helpers import make_case, make_variant
    cfg, geo = pkg.config, pkg.geometry
    if case in ("c2", "c1"):  # the benchmark's workloads and its start state
        prm = cfg.params_from_values(end_time=1e9, dp=0.025 if case == "c2" else 0.04, DL=3.0)
        parts = geo.init_particles(prm)
        pos, vel = geo.developed_state(prm, parts, jitter=0.05, seed=12345)
        return prm, parts, pos, vel
    if case == "variant":  # moving walls, uneven mass, rho0 = 2.5
        prm, parts = make_variant(cfg, geo, dp=0.025, DL=1.5, jitter=0.25, seed=31, developed=True, rho0=2.5,
                                  transport_coeff=0.1)
    elif case == "three":  # three cell columns: every +-1 column is a wrap
        prm, parts = make_case(cfg, geo, dp=0.05, DL=0.7, jitter=0.25, seed=9, developed=True)
    elif case == "two":  # two cell columns: the +-1 columns coincide
        prm, parts = make_case(cfg, geo, dp=0.1, DL=0.7, jitter=0.25, seed=9, developed=True)
    else:
        raise SystemExit(f"unknown case {case}")
    return prm, parts, parts["pos"], parts["vel"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(STEPS))
    ap.add_argument("--mode", default="advance", choices=("advance", "graph", "profile"))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    capi = pkg.capi
    prm, parts, pos, vel = make_state(pkg, args.case)
    steps = STEPS[args.case]
    with capi.Context.from_parts(prm, parts, pos=pos, vel=vel, t_end=1e9) as ctx:
        info, sched0, policy, tuning = ctx.info(), ctx.schedule(), ctx.grid_policy(), ctx.tuning()
        if args.mode == "advance":
            st = ctx.advance(1e9, max_steps=steps)
        elif args.mode == "graph":  # the benchmark's cadence: warm-up, then batches replayed as graphs
            ctx.enqueue_steps(5)
            ctx.sync()
            for _ in range(5):
                ctx.prepare_steps(20)
                ctx.enqueue_steps(20)
                st = ctx.sync()
        else:
            ctx.profile_enable(True)
            ctx.enqueue_steps(steps)
            st = ctx.sync()
            launches = ctx.profile_read()
            ctx.profile_enable(False)
        got = ctx.download()
        sched1, graphs, policy = ctx.schedule(), ctx.graph_stats(), ctx.grid_policy()
        if args.mode != "profile":  # which chain this context runs: a profiled stretch that holds a scheduled re-binning
            ctx.profile_enable(True)
            ctx.enqueue_steps(20)
            ctx.sync()
            launches = ctx.profile_read()
            ctx.profile_enable(False)
    np.savez(args.out, **got)
    print(json.dumps(dict(switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), case=args.case, mode=args.mode,
                          step=int(st["step"]), t=st["t"], dt_last=st["dt_last"], vmax=st["vmax"], device_status=int(st["device_status"]),
                          rebins=int(sched1["rebins"] - sched0["rebins"]), schedule=sched0, graphs=graphs,
                          n_cell_x=info["n_cell_x"], rebuild_every=policy["rebuild_every"], lanes=tuning["lanes_per_particle"],
                          forced_rebuilds=int(policy["forced_rebuilds"]),
                          launches={k: int(v["launches"]) for k, v in launches.items()},
                          avg_us={k: 1e3 * v["avg_ms"] for k, v in launches.items()})), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
