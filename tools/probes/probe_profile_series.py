"""Manual probe (not a test): what the device-side profile series (include/sphx.h sections 2j / 2k) costs.
    tools/build_baseline_lib.sh <parent commit> parent
    python tools/probes/probe_profile_series.py --baseline tools/_exp/libsphx_parent.so [--case C2:1 --case C5:16 ...]
Per case (bench.py's channels, developed parabolic start; NAME:every, or NAME:every:M for a batch of M members): us/step of
replayed batches, prepared first so that they are pure replay, with the series OFF -- the parent commit's library, which has
no such sampler (SPHX_LIB) -- and ON (this build, whole channel + mid band, the reference's bins), alternating --reps times.
A library is chosen when the package is imported, so every timed batch runs in a child process of its own (--child); the
series' buffer holds every record of a batch.  With the series on, the per-launch time of k_profile_series from
sphx_ctx_profile_read (eager, HIP events) as well.  One JSON line per case."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = ("C2:1", "C2:16", "C5:1", "C5:16", "C2:1:16")


def parse_case(s):
    name, every, *m = s.split(":")
    return name, int(every), int(m[0]) if m else 1


def child(case, on, steps, warm):
    """one timed batch in this process, with whatever library SPHX_LIB names; prints one JSON line"""
    import importlib

    import numpy as np

    import bench
    pkg = importlib.import_module(bench.PKG)
    capi, config, geometry, profile = pkg.capi, pkg.config, pkg.geometry, pkg.profile
    name, every, M = parse_case(case)
    prm = config.params_from_values(end_time=1e9, output_interval=1e9, **bench.parse_workload(name)[1])
    parts = geometry.init_particles(prm)
    nf = parts["n_fluid"]
    vel = parts["vel"].copy(order="F")
    y = parts["pos"][:nf, 1]
    vel[:nf, 0] = prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y)
    parts = dict(parts, vel=vel)
    band = (0.5 * prm.DL, max(prm.dp, prm.h))
    out = dict(case=case, on=on, lib=os.path.relpath(capi.LIB_PATH, ROOT), n_fluid=nf, n_bins=profile.n_profile_bins(prm.DH, prm.dp), steps=steps)
    ctx = capi.Context.from_parts(prm, parts, t_end=1e9) if M == 1 else capi.Batch.from_parts([prm] * M, [parts] * M, t_end=1e9)
    with ctx:
        ctx.advance(1e9, max_steps=warm)
        if on:
            ctx.profile_series_enable(every=every, bands=[band], capacity=steps // every + 2)
        if M == 1:
            ctx.prepare_steps(steps)
        else:
            ctx.advance(1e9, max_steps=steps)  # (a batch has no prepare: one batch of the same length captures its graphs)
            if on:
                ctx.profile_series_sums(drain=True)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.enqueue_steps(steps)
        ctx.sync()
        out["us_per_step"] = 1e6 * (time.perf_counter() - t0) / steps
        if on:
            s = ctx.profile_series_sums()
            s = s[0] if M > 1 else s
            out["n_records"], out["n_dropped"] = len(s["step"]), s["n_dropped"]
            out["count_per_record"] = float(np.sum(s["count"][-1, 0])) if len(s["step"]) else None
            if M == 1:
                ctx.profile_enable(True)
                ctx.advance(1e9, max_steps=min(steps, 48))
                prof = ctx.profile_read()
                ctx.profile_enable(False)
                out["k_profile_series_us"] = 1e3 * prof.get("k_profile_series", {}).get("avg_ms", float("nan"))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[])
    ap.add_argument("--baseline", default=None, help="the parent commit's libsphx.so (tools/build_baseline_lib.sh)")
    ap.add_argument("--steps", type=int, default=0, help="steps per timed batch (0: 2000 below 10^5 particles, else 96)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--child", choices=("off", "on"), default=None)
    a = ap.parse_args()
    if a.child:
        child(a.case[0], a.child == "on", a.steps, a.warm)
        return
    if not a.baseline or not os.path.exists(a.baseline):
        sys.exit("--baseline: the parent commit's library is needed for the OFF side (tools/build_baseline_lib.sh <commit> parent)")
    import numpy as np

    import bench
    for case in a.case or CASES:
        kw = bench.parse_workload(parse_case(case)[0])[1]
        steps = a.steps or (2000 if kw["DL"] / kw["dp"] / kw["dp"] < 1e5 else 96)
        rows = dict(off=[], on=[])
        for _ in range(a.reps):
            for side in ("off", "on"):
                env = dict(os.environ)
                env.pop("SPHX_LIB", None)
                if side == "off":
                    env["SPHX_LIB"] = os.path.abspath(a.baseline)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--case", case, "--steps", str(steps),
                                      "--warm", str(a.warm)], env=env, capture_output=True, text=True, timeout=600)
                if res.returncode != 0:  # nothing more is started after a child that failed
                    sys.exit(f"{case} {side}: the child ended with status {res.returncode}\n{res.stdout}\n{res.stderr}")
                rows[side].append(json.loads(res.stdout.strip().splitlines()[-1]))
        med = {s: float(np.median([r["us_per_step"] for r in rows[s]])) for s in rows}
        last = rows["on"][-1]
        print(json.dumps(dict(case=case, steps=steps, n_fluid=last["n_fluid"], n_bins=last["n_bins"],
                              us_off=[round(r["us_per_step"], 3) for r in rows["off"]], us_on=[round(r["us_per_step"], 3) for r in rows["on"]],
                              us_off_median=round(med["off"], 3), us_on_median=round(med["on"], 3), cost_us_per_step=round(med["on"] - med["off"], 3),
                              cost_us_per_sampled_step=round((med["on"] - med["off"]) * parse_case(case)[1], 3),
                              n_records=last.get("n_records"), n_dropped=last.get("n_dropped"),
                              k_profile_series_us=last.get("k_profile_series_us"), lib_off=rows["off"][-1]["lib"], lib_on=last["lib"])),
              flush=True)


if __name__ == "__main__":
    main()
