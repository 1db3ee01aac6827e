"""Manual probe (not a test): what one sample of the device-side gradient statistics (include/sphx.h section 2n) costs, beside
the pair statistics' sample and the cell sweep of the step's density pass of the same context in the same run.
    python tools/probes/probe_grad_stats.py [--case C2 --case dp=0.005,DL=6.25 ...] [--bins 0] [--walls]
Per case (bench.py's channels or dp=..,DL=..) and state -- `lattice` (the initialiser's particles at rest) and `developed`
(make_case's: +-0.2 dp of jitter, a parabolic profile; then --settle steps so that the arrangement is the solver's own) --
per-launch times from sphx_ctx_profile_read (eager launches, HIP events) over --steps steps with both samplers at every = 1,
mid band and seam band, in a context that re-bins every step, so that every step's density pass is the cell sweep
(k_density_build): k_grad_stats, k_pair_dist, k_density_build, and the ratios.  Then the same with the context's own re-binning
policy.  One JSON line per case and state.  A lane-count variant (tools/probes/build_variant_lib.sh glanes4
-DSPHX_EXP_GRAD_LANES=4) is measured by running the probe with SPHX_LIB=tools/_exp/libsphx_glanes4.so."""
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
    ap.add_argument("--bins", type=int, default=0)
    ap.add_argument("--walls", action="store_true")
    ap.add_argument("--policy", action="append", default=[], choices=["rebin_every_step", "own_policy"])
    a = ap.parse_args()
    import bench
    from helpers import make_case
    pkg = importlib.import_module(bench.PKG)
    capi, config, geometry = pkg.capi, pkg.config, pkg.geometry
    policies = dict(rebin_every_step=dict(rebuild_every=1), own_policy=dict())
    for case in a.case or CASES:
        kw = bench.parse_workload(case)[1]
        for state in ("lattice", "developed"):
            prm, parts = make_case(config, geometry, jitter=0.0 if state == "lattice" else 0.2, developed=state == "developed", seed=3, **kw)
            hw = max(prm.dp, prm.h)
            bands = [(0.5 * prm.DL, hw), (0.0, hw)]
            out = dict(case=case, state=state, n_fluid=parts["n_fluid"], n_bins=a.bins, walls=a.walls, steps=a.steps,
                       lib=os.path.basename(capi.LIB_PATH))
            for policy in a.policy or list(policies):
                with capi.Context.from_parts(prm, parts, t_end=1e9, **policies[policy]) as ctx:
                    if state == "developed":
                        ctx.advance(1e9, max_steps=a.settle)
                    ctx.grad_stats_enable(n_bins=a.bins, every=1, with_walls=a.walls, bands=bands)
                    ctx.pair_dist_enable(n_bins=64, every=1, y_margin=2.0 * prm.h, with_walls=a.walls, bands=bands)
                    ctx.advance(1e9, max_steps=8)
                    ctx.grad_stats_reset()
                    ctx.profile_enable(True)
                    ctx.advance(1e9, max_steps=a.steps)
                    prof = ctx.profile_read()
                    ctx.profile_enable(False)
                    gs = ctx.grad_stats_sums(0)
                us = {k: round(1e3 * v["avg_ms"], 2) for k, v in prof.items() if v["launches"] > 0}
                row = dict(kernels_us=us, launches={k: v["launches"] for k, v in prof.items() if v["launches"] > 0},
                           count=int(gs["count"].sum()), skipped=int(gs["skipped"].sum()))
                if "k_density_build" in us:
                    row["grad_stats_over_cell_sweep"] = round(us["k_grad_stats"] / us["k_density_build"], 2)
                row["grad_stats_over_pair_dist"] = round(us["k_grad_stats"] / us["k_pair_dist"], 2)
                out[policy] = row
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
