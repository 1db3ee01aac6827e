"""Manual probe (not a test): what the device-side mode amplitudes (include/sphx.h sections 2t / 2u) cost, beside the profile
series (sections 2j / 2k) in the same run and build.
    python tools/probes/probe_modes.py [--case C2 --case dp=0.005,DL=6.25 ...] [--modes 4,8 --modes 16,16] [--every 1]
Per case (bench.py's channels or dp=..,DL=.., developed parabolic start): us/step of replayed batches, prepared first so that
they are pure replay, with no sampler on, with the profile series on (whole channel + mid band, the reference's bins) and with
the mode amplitudes on (one line per --modes), a fresh context each, the three alternating --reps times; the cost of a sampler
is its median minus the median with none on.  With a sampler on, the per-launch time of its kernel from sphx_ctx_profile_read
(eager, HIP events) as well.  One JSON line per case and set of modes."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = ("C2", "dp=0.005,DL=6.25")
MODES = ("4,8", "16,16")


def timed(capi, prm, parts, steps, warm, enable, kernel):
    """(us per replayed step, us per eager launch of `kernel`, records) of a fresh context with enable(ctx) applied"""
    with capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:
        ctx.advance(1e9, max_steps=warm)
        n_records = enable(ctx, steps)
        ctx.prepare_steps(steps)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.enqueue_steps(steps)
        ctx.sync()
        us = 1e6 * (time.perf_counter() - t0) / steps
        got = n_records(ctx) if n_records else None
        eager = None
        if kernel:
            ctx.profile_enable(True)
            ctx.advance(1e9, max_steps=min(steps, 48))
            prof = ctx.profile_read()
            ctx.profile_enable(False)
            eager = 1e3 * prof.get(kernel, {}).get("avg_ms", float("nan"))
    return us, eager, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[])
    ap.add_argument("--modes", action="append", default=[])
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0, help="steps per timed batch (0: 2000 below 10^5 particles, else 200)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=64)
    a = ap.parse_args()
    import numpy as np

    import bench
    pkg = importlib.import_module(bench.PKG)
    capi, config, geometry, profile = pkg.capi, pkg.config, pkg.geometry, pkg.profile
    for case in a.case or CASES:
        kw = bench.parse_workload(case)[1]
        prm = config.params_from_values(end_time=1e9, output_interval=1e9, **kw)
        parts = geometry.init_particles(prm)
        nf = parts["n_fluid"]
        vel = parts["vel"].copy(order="F")
        y = parts["pos"][:nf, 1]
        vel[:nf, 0] = prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y)
        parts = dict(parts, vel=vel)
        steps = a.steps or (2000 if nf < 1e5 else 200)
        band = (0.5 * prm.DL, max(prm.dp, prm.h))

        def series_on(ctx, n):
            ctx.profile_series_enable(every=a.every, bands=[band], capacity=n // a.every + 2)
            return lambda c: len(c.profile_series_sums()["step"])

        for modes in a.modes or MODES:
            mx, ny = (int(v) for v in modes.split(","))

            def modes_on(ctx, n):
                ctx.modes_enable(mx=mx, ny=ny, every=a.every, capacity=n // a.every + 2)
                return lambda c: len(c.modes()["step"])

            sides = dict(off=(lambda ctx, n: None, None), series=(series_on, "k_profile_series"), modes=(modes_on, "k_modes"))
            rows = {s: [] for s in sides}
            for _ in range(a.reps):
                for s, (enable, kernel) in sides.items():
                    rows[s].append(timed(capi, prm, parts, steps, a.warm, enable, kernel))
            med = {s: float(np.median([r[0] for r in rows[s]])) for s in rows}
            print(json.dumps(dict(case=case, n_fluid=nf, steps=steps, every=a.every, modes=[mx, ny], counters=(mx + 1) * (ny + 1) * 12,
                                  n_bins=profile.n_profile_bins(prm.DH, prm.dp),
                                  **{f"us_{s}": [round(r[0], 3) for r in rows[s]] for s in rows},
                                  **{f"us_{s}_median": round(med[s], 3) for s in rows},
                                  series_cost_us_per_step=round(med["series"] - med["off"], 3),
                                  modes_cost_us_per_step=round(med["modes"] - med["off"], 3),
                                  k_profile_series_us=rows["series"][-1][1], k_modes_us=rows["modes"][-1][1],
                                  records=dict(series=rows["series"][-1][2], modes=rows["modes"][-1][2]))), flush=True)


if __name__ == "__main__":
    main()
