"""Manual probe (not a test): what one sample of the device-side pair statistics (include/sphx.h section 2l) costs, beside the
cell sweep of the step's density pass of the same context in the same run.
    python tools/probes/probe_pair_dist.py [--case C2 --case dp=0.005,DL=6.25 ...] [--bins 64] [--walls]
Per case (bench.py's channels or dp=..,DL=..) and state -- `lattice` (the initialiser's particles at rest) and `developed`
(make_case's: +-0.2 dp of jitter, a parabolic profile; then --settle steps so that the arrangement is the solver's own) --
per-launch times from sphx_ctx_profile_read (eager launches, HIP events) over --steps steps with the sampler at every = 1, mid
band and seam band, in a context that re-bins every step, so that every step's density pass is the cell sweep
(k_density_build): k_pair_dist, k_density_build, and their ratio.  Then the same with the context's own re-binning policy, where
the sweep runs once per cycle and the other steps walk the list: every kernel's time, for the cost per step.  One JSON line
per case and state."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CASES = ("C2", "dp=0.005,DL=6.25")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[])
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--walls", action="store_true")
    a = ap.parse_args()
    import bench
    from helpers import make_case
    pkg = importlib.import_module(bench.PKG)
    capi, config, geometry = pkg.capi, pkg.config, pkg.geometry
    for case in a.case or CASES:
        kw = bench.parse_workload(case)[1]
        for state in ("lattice", "developed"):
            prm, parts = make_case(config, geometry, jitter=0.0 if state == "lattice" else 0.2, developed=state == "developed", seed=3, **kw)
            hw = max(prm.dp, prm.h)
            out = dict(case=case, state=state, n_fluid=parts["n_fluid"], n_bins=a.bins, walls=a.walls, steps=a.steps)
            for policy, more in (("rebin_every_step", dict(rebuild_every=1)), ("own_policy", dict())):
                with capi.Context.from_parts(prm, parts, t_end=1e9, **more) as ctx:
                    if state == "developed":
                        ctx.advance(1e9, max_steps=a.settle)
                    ctx.pair_dist_enable(n_bins=a.bins, every=1, y_margin=2.0 * prm.h, with_walls=a.walls,
                                         bands=[(0.5 * prm.DL, hw), (0.0, hw)])
                    ctx.advance(1e9, max_steps=8)
                    ctx.pair_dist_reset()
                    ctx.profile_enable(True)
                    ctx.advance(1e9, max_steps=a.steps)
                    prof = ctx.profile_read()
                    ctx.profile_enable(False)
                    pd = ctx.pair_dist(0)
                us = {k: round(1e3 * v["avg_ms"], 2) for k, v in prof.items() if v["launches"] > 0}
                row = dict(kernels_us=us, launches={k: v["launches"] for k, v in prof.items() if v["launches"] > 0},
                           n_neigh=round(pd["n_neigh"], 3), r_min_dp=round(pd["r_min"] / prm.dp, 4), bins_hit=int((pd["ff"] > 0).sum()))
                if "k_density_build" in us:
                    row["pair_dist_over_cell_sweep"] = round(us["k_pair_dist"] / us["k_density_build"], 2)
                out[policy] = row
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
