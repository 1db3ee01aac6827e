"""Manual probe (not a test): what one sample of the device-side density statistics (include/sphx.h section 2r) costs, beside
the pair statistics' and the gradient statistics' samples of the same context in the same run, and what the sampler reports
of a run.
    python tools/probes/probe_dens_stats.py [--case C2 --case dp=0.005,DL=6.25 ...] [--bins 0] [--eager-only]
    python tools/probes/probe_dens_stats.py --physics [--coeff 0.05 --coeff 0.1 --coeff 0.2] [--dp 0.05] [--from 16] [--end 20]
Cost.  Per case (bench.py's channels or dp=..,DL=..) and state -- `lattice` (the initialiser's particles at rest) and `developed`
(make_case's: +-0.2 dp of jitter, a parabolic profile; then --settle steps so that the arrangement is the solver's own) -- per-launch
times from sphx_ctx_profile_read (eager launches, HIP events) over --steps steps with the three samplers at every = 1, mid band and
seam band, walls off for the other two, in a context that re-bins every step and in one on its own re-binning policy:
k_dens_stats, k_pair_dist, k_grad_stats, the cell sweep of the density pass, and the ratios.  Then "in the loop": the wall time of
--loop steps replayed from graphs with no sampler, and with each of the three alone at every = 1; the difference per step is what
a sample costs inside the loop.  One JSON line per case and state.  A lane-count variant (tools/probes/build_variant_lib.sh
dlanes4 -DSPHX_EXP_DENS_LANES=4) is measured by running the probe with SPHX_LIB=tools/_exp/libsphx_dlanes4.so.
Physics.  driver.run of the reference configuration at --dp to --end with density_from = --from and density_every = 1, once per
--coeff (transport_coeff): density_figures and the profiles of band 0, one JSON line each."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CASES = ("C2", "dp=0.005,DL=6.25")
SAMPLERS = ("k_dens_stats", "k_pair_dist", "k_grad_stats")


def _enable(ctx, prm, which, bins):
    hw = max(prm.dp, prm.h)
    bands = [(0.5 * prm.DL, hw), (0.0, hw)]
    if which == "k_dens_stats":
        ctx.dens_stats_enable(n_bins=bins, every=1, bands=bands)
    elif which == "k_pair_dist":
        ctx.pair_dist_enable(n_bins=64, every=1, y_margin=2.0 * prm.h, bands=bands)
    elif which == "k_grad_stats":
        ctx.grad_stats_enable(n_bins=bins, every=1, bands=bands)


def cost(a):
    import bench
    from helpers import make_case
    pkg = importlib.import_module(bench.PKG)
    capi, config, geometry = pkg.capi, pkg.config, pkg.geometry
    policies = dict(rebin_every_step=dict(rebuild_every=1), own_policy=dict())
    for case in a.case or CASES:
        kw = bench.parse_workload(case)[1]
        for state in ("lattice", "developed"):
            prm, parts = make_case(config, geometry, jitter=0.0 if state == "lattice" else 0.2, developed=state == "developed", seed=3, **kw)
            out = dict(case=case, state=state, n_fluid=parts["n_fluid"], n_bins=a.bins, steps=a.steps, lib=os.path.basename(capi.LIB_PATH))
            for policy, launch in policies.items():
                with capi.Context.from_parts(prm, parts, t_end=1e9, **launch) as ctx:
                    if state == "developed":
                        ctx.advance(1e9, max_steps=a.settle)
                    for which in SAMPLERS:
                        _enable(ctx, prm, which, a.bins)
                    ctx.advance(1e9, max_steps=8)
                    ctx.dens_stats_reset()
                    ctx.profile_enable(True)
                    ctx.advance(1e9, max_steps=a.steps)
                    prof = ctx.profile_read()
                    ctx.profile_enable(False)
                    ds = ctx.dens_stats_sums(0)
                us = {k: round(1e3 * v["avg_ms"], 2) for k, v in prof.items() if v["launches"] > 0}
                row = dict(kernels_us=us, launches={k: v["launches"] for k, v in prof.items() if v["launches"] > 0},
                           count=int(ds["count"].sum()), outliers=int(ds["outliers"].sum()))
                sweep = us.get("k_density_build", us.get("k_density"))
                if sweep:
                    row["dens_stats_over_cell_sweep"] = round(us["k_dens_stats"] / sweep, 2)
                row["dens_stats_over_pair_dist"] = round(us["k_dens_stats"] / us["k_pair_dist"], 2)
                row["dens_stats_over_grad_stats"] = round(us["k_dens_stats"] / us["k_grad_stats"], 2)
                out[policy] = row
            if not a.eager_only:
                loop = {}
                for which in (None,) + SAMPLERS:
                    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
                        if state == "developed":
                            ctx.advance(1e9, max_steps=a.settle)
                        if which:
                            _enable(ctx, prm, which, a.bins)
                        ctx.advance(1e9, max_steps=a.loop)      # the graphs are captured here
                        ctx.sync()
                        best = None
                        for _ in range(3):
                            t0 = time.perf_counter()
                            ctx.advance(1e9, max_steps=a.loop)
                            ctx.sync()
                            dt = time.perf_counter() - t0
                            best = dt if best is None else min(best, dt)
                        loop[which or "none"] = round(1e6 * best / a.loop, 2)
                out["in_loop_us_per_step"] = loop
                out["in_loop_sample_us"] = {k: round(loop[k] - loop["none"], 2) for k in SAMPLERS}
            print(json.dumps(out), flush=True)


def physics(a):
    import bench
    pkg = importlib.import_module(bench.PKG)
    config, driver = pkg.config, pkg.driver
    for coeff in a.coeff or [0.05, 0.1, 0.2]:
        prm = config.params_from_values(dp=a.dp, DL=3.0, transport_coeff=coeff, end_time=a.end, output_interval=1.0)
        res = driver.run(prm, density_from=a.t_from, density_every=1, density_hist=(64, 0.05))
        ds = res.dens_stats
        fig = driver.density_figures(prm, ds)
        mid = driver.density_figures(prm, ds, band=1)
        out = dict(dp=prm.dp, DL=prm.DL, transport_coeff=coeff, n_fluid=res.n_fluid, steps=res.steps, t=res.t, wall_seconds=round(res.wall_seconds, 2),
                   n_samples=ds[0]["n_samples"], t_first=ds[0]["t_first"], t_last=ds[0]["t_last"], L2_profile=res.L2_error, **fig,
                   mid_band={k: mid[k] for k in ("delta_rms", "delta_max", "p_spread", "wall_bias", "packing")},
                   below=ds[0]["below"], above=ds[0]["above"], hist=[int(v) for v in ds[0]["hist"]],
                   d_mean=[round(float(v), 6) for v in ds[0]["d_mean"]], d_std=[round(float(v), 6) for v in ds[0]["d_std"]],
                   wall_mean=[round(float(v), 5) for v in ds[0]["wall_mean"]])
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[])
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--loop", type=int, default=512)
    ap.add_argument("--bins", type=int, default=0)
    ap.add_argument("--eager-only", action="store_true")
    ap.add_argument("--physics", action="store_true")
    ap.add_argument("--coeff", action="append", type=float, default=[])
    ap.add_argument("--dp", type=float, default=0.05)
    ap.add_argument("--from", dest="t_from", type=float, default=16.0)
    ap.add_argument("--end", type=float, default=20.0)
    a = ap.parse_args()
    (physics if a.physics else cost)(a)


if __name__ == "__main__":
    main()
