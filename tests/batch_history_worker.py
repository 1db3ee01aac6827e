"""Child process of tests/test_gpu_batch_history.py: SPHX_DEBUG_SWITCHES is read once per process, so every switch set runs in
a fresh one.  The switches no_fuse_ea, no_fold_rebin and no_tail_clock move what k_step_history_b reads -- the Vol / B buffers
of the finished step (tmp_par of the slot's parity or of parity 0), the chain that re-bins (src_of) and the launch that
updates the clock the gate reads.  Builds a 3-member batch (dp 0.05, DL 3, different mu / c_f / transport_coeff) and the same
three channels as standalone contexts in this process, records every step of 2K+3 on all of them and compares member by
member, bit for bit: the eight fields of every record, the counts, and the status.  Prints ONE JSON line: the schedule a
standalone context chose, what the batch says about itself, and what differed.  Exit code 0: ran to the end (whatever the
comparison said).

    SPHX_DEBUG_SWITCHES=no_fuse_ea python tests/batch_history_worker.py
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

VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=17.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=13.0, transport_coeff=0.30, seed=9)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lpp", type=int, default=16)
    args = ap.parse_args()
    from helpers import make_case
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    capi = pkg.capi
    members = [make_case(pkg.config, pkg.geometry, dp=0.05, DL=3.0, jitter=0.2, seed=v["seed"], developed=True, mu=v["mu"],
                         c_f=v["c_f"], transport_coeff=v["transport_coeff"]) for v in VARIANTS]
    kw = dict(t_end=1e9, lanes_per_particle=args.lpp)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        n = 2 * b.info()["rebuild_every"] + 3
        b.history_enable(every=1)
        sts = b.advance(1e9, max_steps=n)
        got = b.history_records()
        info = b.info()
    differs, sched, rebins = [], None, []
    for m, (prm, parts) in enumerate(members):
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            before = ctx.schedule()
            ctx.history_enable(every=1)
            st = ctx.advance(1e9, max_steps=n)
            rec, dropped = ctx.history_records()
            rebins.append(int(ctx.schedule()["rebins"] - before["rebins"]))
            sched = sched or before
        if st != sts[m]:
            differs.append(f"member {m}: status")
        if rec.shape != got[m][0].shape or dropped != got[m][1]:
            differs.append(f"member {m}: counts {got[m][0].shape[0]}/{got[m][1]} vs {rec.shape[0]}/{dropped}")
            continue
        for j, k in enumerate(capi.HISTORY_FIELDS):
            if not np.array_equal(got[m][0][:, j], rec[:, j]):
                differs.append(f"member {m}: {k}")
    print(json.dumps(dict(switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), lpp=args.lpp, steps=n,
                          steps_taken=[int(s["step"]) for s in sts], schedule=sched, rebins=rebins, info=info,
                          n_records=[int(g[0].shape[0]) for g in got], n_dropped=[int(g[1]) for g in got], differs=differs)),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
