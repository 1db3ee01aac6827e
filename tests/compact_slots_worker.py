"""Child process of tests/test_gpu_compact_slots.py and tests/golden/make_compact_slots.py: SPHX_DEBUG_SWITCHES is read once per
process, so each block size of the compact step kernels (block_256, block_320) runs in a fresh one.  Runs every case of CASES at
16 and at 32 lanes per particle for 35 steps and writes what a caller can see of each -- the nine downloaded fields, t, dt_last,
vmax, the pair count, both wall shears -- to OUT/<case>_lpp<lanes>.npz, and prints ONE JSON line: per run the block size, the
lane count and the schedule the context reports, the population and the cell columns.

    SPHX_DEBUG_SWITCHES=block_320 python tests/compact_slots_worker.py OUT

The channel is dp = 1/21, DL = 23/21: 483 fluid + 184 wall particles in five cell columns.  483 is no multiple of the 8, 10, 16 or
20 particles a workgroup of 256 or 320 threads holds at 32 or 16 lanes each, so the last workgroup of every pass is partly filled;
five columns take the folded re-binning step, and at a period this short the periodic seam lies inside every pass."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    sys.path.insert(0, p)

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
SCALARS = ("t", "dt_last", "vmax", "pairs", "tau_bottom", "tau_top")
STEPS = 35
DP, DL = 1.0 / 21.0, 23.0 / 21.0
LANES = (16, 32)


def channel(cfg, geo):
    prm = cfg.params_from_values(dp=DP, DL=DL, end_time=1e9)
    return prm, geo.init_particles(prm)


def developed(cfg, geo):
    """The benchmark's start: the analytic parabola and a position jitter of 0.05 dp."""
    prm, parts = channel(cfg, geo)
    pos, vel = geo.developed_state(prm, parts, jitter=0.05, seed=12345)
    return prm, parts, dict(pos=pos, vel=vel)


def rest(cfg, geo):
    """The lattice at rest."""
    prm, parts = channel(cfg, geo)
    return prm, parts, {}


CASES = {"developed": developed, "rest": rest}


def main():
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    capi = pkg.capi
    facts = {}
    for name, state in CASES.items():
        for lpp in LANES:
            prm, parts, start = state(pkg.config, pkg.geometry)
            with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=lpp, **start) as ctx:
                info, tuning, sched = ctx.info(), ctx.tuning(), ctx.schedule()
                st = ctx.advance(1e9, max_steps=STEPS)
                got = ctx.download()
                tb, tt, npairs = ctx.monitor(tau=True, pairs=True)
                after = ctx.schedule()
            scalars = dict(t=st["t"], dt_last=st["dt_last"], vmax=st["vmax"], pairs=npairs, tau_bottom=tb, tau_top=tt)
            run = f"{name}_lpp{lpp}"
            np.savez(os.path.join(out_dir, run + ".npz"), **{k: got[k] for k in FIELDS}, **{k: np.asarray(v) for k, v in scalars.items()})
            facts[run] = dict(block_size=tuning["block_size"], lanes=tuning["lanes_per_particle"], fuse_ea=sched["fuse_ea"],
                              tail_clock=sched["tail_clock"], dynamic=sched["dynamic"], steps=int(st["step"]),
                              rebins=int(after["rebins"] - sched["rebins"]), n_fluid=int(info["n_fluid"]), n_wall=int(info["n_wall"]),
                              n_cell_x=int(info["n_cell_x"]), finite=bool(all(np.all(np.isfinite(got[k])) for k in FIELDS)))
    print(json.dumps(dict(switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), runs=facts)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
