"""Child process of tests/test_gpu_batch_switches.py: SPHX_DEBUG_SWITCHES is read once per process, so every switch set runs in
a fresh one.  Builds the moving-wall batch of test_gpu_batch.py (helpers.make_variant: moving walls, uneven mass, rho0 = 2.5;
dp 0.05, DL 1.5, four members) or, with --case regimes, the four members of test_gpu_regimes.py (default physics, flow to the
left, c_f = 0.3, mu = 2 on fixed walls) and the same four channels as standalone contexts, enables flow statistics on all of them
(every step, one band at DL/2), advances 2K+3 steps and compares member by member, bit for bit: the nine fields, t, dt_last,
vmax, step, both tau, the pair count, and the raw flow-statistics sums of both bands.  Prints ONE JSON line: the schedule a
standalone context chose, what the batch says about itself, and what differed.  Exit code 0: ran to the end (whatever the
comparison said).

    SPHX_DEBUG_SWITCHES=no_fuse_ea python tests/batch_switch_worker.py --lpp 16 --mode eager

--dump DIR also writes what was downloaded from the batch as DIR/m<member>_<name>.npy, so that two builds of the library
(SPHX_LIB) can be compared byte for byte on the same case.
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

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
SUMS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2", "n_samples", "t_first", "t_last")
# (as test_gpu_batch.VARIANTS)
VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=17.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=13.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]


def collect(dl, st, mon, sums):
    out = dict(dl, t=st["t"], dt_last=st["dt_last"], vmax=st["vmax"], step=st["step"], tau_bottom=mon[0], tau_top=mon[1],
               pairs=mon[2])
    for band, s in enumerate(sums):
        for k in SUMS:
            out[f"stats{band}_{k}"] = s[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lpp", type=int, default=16)
    ap.add_argument("--rebuild-every", type=int, default=0, help="0: the library's choice")
    ap.add_argument("--mode", choices=("graph", "eager"), default="graph", help="eager: one-step calls")
    ap.add_argument("--dump", metavar="DIR", help="also write what the batch returned as DIR/*.npy")
    ap.add_argument("--skin-h", type=float, default=0.0, help="cell skin in units of h (0: the library's choice)")
    ap.add_argument("--case", choices=("", "regimes"), default="", help="regimes: the four members of test_gpu_regimes.py")
    args = ap.parse_args()
    from helpers import make_variant
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    capi = pkg.capi
    members = []
    if args.case == "regimes":  # default physics, flow to the left, c_f = 0.3, mu = 2: fixed walls and even mass, shared as they are
        import regime_cases
        members = [getattr(regime_cases, name)(pkg.config, pkg.geometry, "small")
                   for name in ("default", "leftward_plain", "capped", "viscous_plain")]
    for v in VARIANTS if not members else ():
        prm, parts = make_variant(pkg.config, pkg.geometry, dp=0.05, DL=1.5, jitter=0.2, seed=v["seed"], developed=True, rho0=2.5,
                                  mu=v["mu"], c_f=v["c_f"], transport_coeff=v["transport_coeff"])
        if members:  # walls and masses are the batch's, not the member's
            parts.update(mass=members[0][1]["mass"], wall_vel=members[0][1]["wall_vel"])
        members.append((prm, parts))
    kw = dict(t_end=1e9, lanes_per_particle=args.lpp)
    if args.rebuild_every:
        kw["rebuild_every"] = args.rebuild_every
    if args.skin_h:
        kw["skin_h"] = args.skin_h
    stats = dict(every=1, bands=[(0.75, 0.2)])  # one band at DL/2

    def advance(obj, n):
        if args.mode == "graph":
            return obj.advance(1e9, max_steps=n)
        for _ in range(n):
            st = obj.advance(1e9, max_steps=1)
        return st

    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        info = b.info()
        n = 2 * info["rebuild_every"] + 3
        b.flow_stats_enable(**stats)
        sts = advance(b, n)
        sums = [b.flow_stats_sums(band) for band in (0, 1)]
        got = [collect(b.download(m), sts[m], b.monitor(m, tau=True, pairs=True), [s[m] for s in sums])
               for m in range(len(members))]
        info, graph_stats = b.info(), b.graph_stats()
    differs, sched, rebins = [], None, []
    for m, (prm, parts) in enumerate(members):
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            before = ctx.schedule()
            ctx.flow_stats_enable(**stats)
            st = advance(ctx, n)
            ref = collect(ctx.download(), st, ctx.monitor(tau=True, pairs=True), [ctx.flow_stats_sums(band) for band in (0, 1)])
            rebins.append(int(ctx.schedule()["rebins"] - before["rebins"]))
            sched = sched or before
        for k in ref:
            if not np.array_equal(np.asarray(got[m][k]), np.asarray(ref[k]), equal_nan=k.endswith(("t_first", "t_last"))):
                differs.append(f"member {m}: {k}")
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for m, g in enumerate(got):
            for k, v in g.items():
                np.save(os.path.join(args.dump, f"m{m}_{k}.npy"), np.asarray(v))
    print(json.dumps(dict(switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), lpp=args.lpp, mode=args.mode, case=args.case, steps=n,
                          steps_taken=[int(g["step"]) for g in got], schedule=sched, rebins=rebins, info=info,
                          graph_stats=graph_stats, n_samples=[int(g["stats0_n_samples"]) for g in got], differs=differs)),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
