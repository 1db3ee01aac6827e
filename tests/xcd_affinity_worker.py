"""Child process of tests/test_gpu_xcd_affinity.py: SPHX_DEBUG_SWITCHES is read once per process, so the default numbering of
the workgroups and no_xcd_align each run in a fresh one.  Steps one case 20 steps (re-binning every 8th, so re-binnings are
crossed), writes what was downloaded -- the nine fields, t, dt_last, vmax and step; of every member for a batch -- as .npy files
into --dump DIR, then takes 9 more steps with the per-kernel timer on, which launches eagerly and counts the launches by name.
Prints ONE JSON line: the workgroups of a pass, the kernel forms and the schedule the context chose, the re-binnings, the graph
counters and the launches per kernel name.  Exit code 0: ran to the end.

    SPHX_DEBUG_SWITCHES=no_xcd_align python tests/xcd_affinity_worker.py --case nb300 --dump /tmp/a
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
STEPS, TRACED_STEPS, REBUILD_EVERY, BLOCK = 20, 9, 8, 256
# name -> (dp, DL, lanes per particle, members)
CASES = {
    "nb300": (0.025, 3.0, 16, 1),   # 4 800 fluid particles: 300 workgroups per pass, the A half starts at residue 4
    "nb235": (0.04, 3.0, 32, 1),    # 1 875: 235 workgroups, residue 3
    "nb320": (0.025, 3.2, 16, 1),   # 5 120: 320 workgroups, residue 0 -- both numberings are the same mapping
    "nb625w": (0.01, 2.0, 8, 1),    # 20 000 at 8 lanes: 625 workgroups, the large-channel form of the fused launch
    "batch3": (0.04, 3.0, 32, 3),   # three members, rows of 471 workgroups in the fused launch
}


def save(dump, prefix, dl, st):
    for k in FIELDS:
        np.save(os.path.join(dump, f"{prefix}{k}.npy"), np.asarray(dl[k]))
    for k in ("t", "dt_last", "vmax", "step"):
        np.save(os.path.join(dump, f"{prefix}{k}.npy"), np.asarray(st[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--dump", metavar="DIR", required=True)
    args = ap.parse_args()
    from helpers import make_variant
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    capi = pkg.capi
    dp, DL, lpp, n_members = CASES[args.case]
    members = [make_variant(pkg.config, pkg.geometry, dp=dp, DL=DL, jitter=0.2, seed=41 + m, developed=True, rho0=2.5,
                            transport_coeff=0.1 + 0.1 * m) for m in range(n_members)]
    for prm, parts in members[1:]:  # walls and masses are the batch's
        parts.update(mass=members[0][1]["mass"], wall_vel=members[0][1]["wall_vel"])
    kw = dict(t_end=1e9, lanes_per_particle=lpp, rebuild_every=REBUILD_EVERY)
    os.makedirs(args.dump, exist_ok=True)
    out = dict(switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), case=args.case,
               blocks=-(-members[0][1]["n_fluid"] * lpp // BLOCK))
    with capi.Context.from_parts(*members[0], **kw) as ctx:  # (a batch steps through its member 0's launch layer)
        out.update(forms=ctx.kernel_forms(), schedule=ctx.schedule())
        st = ctx.advance(1e9, max_steps=STEPS)
        save(args.dump, "", ctx.download(), st)
        out.update(steps=int(st["step"]), rebins=int(ctx.schedule()["rebins"] - out["schedule"]["rebins"]),
                   graph_stats=ctx.graph_stats())
        ctx.profile_enable(True)
        ctx.advance(1e9, max_steps=TRACED_STEPS)
        out["launches"] = {k: int(v["launches"]) for k, v in ctx.profile_read().items()}
    if n_members > 1:
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            sts = b.advance(1e9, max_steps=STEPS)
            for m in range(n_members):
                save(args.dump, f"m{m}_", b.download(m), sts[m])
            out.update(batch_info=b.info(), batch_graph_stats=b.graph_stats(), batch_steps=[int(s["step"]) for s in sts])
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
