"""What the density statistics of a slab ring cost (manual probe): an in-process ring on one device, us per ring step with the
sampler off and on in this build, sampling every step (every = 1) and every 10th (every = 10): the reference's profile bins,
64 histogram bins, the whole channel plus the mid-channel and the seam band (driver.run's setting); the walls are always in.  Off is the SAME ring of
the same build with no call of the sampler's made -- or, where a fifth argument names it, another library (the parent
commit's, which has no launch for it).  A library is loaded once per process, so every figure comes from a process of its
own and the runs alternate: off, every = 1, off, every = 10, `rounds` times; medians of the rounds.
    tools/build_baseline_lib.sh HEAD~1 parent                                     (the parent's library, into tools/_exp/)
    python tools/probes/probe_slab_dens_stats.py C4 2 400 3                                  (two slabs of 0.25 M particles)
    python tools/probes/probe_slab_dens_stats.py C2x2 2 2000 3                               (two C2 slabs)
    python tools/probes/probe_slab_dens_stats.py C4 2 400 3 tools/_exp/libsphx_parent.so     (off = the parent's library)
    python tools/probes/probe_slab_dens_stats.py C2x2 2 2000 --one 10              (one figure, in this process: SPHX_LIB decides
                                                                                   the library; --one 0 = off)
The method is probe_slab_pair_dist.py's: a host clock around group_run + sync of every slab, after a warm-up in the same
setting."""
import importlib, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W = {"C2x2": dict(dp=0.025, DL=6.0), "C3": dict(dp=0.01, DL=6.0), "C4": dict(dp=0.005, DL=12.0)}
name, world, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])


def one(every):
    """us per ring step of `steps` steps with the densities sampled every `every`-th step (0: off, no call of the sampler's made)"""
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    slab = importlib.import_module("sph-poiseuille-flow_amd.slab")
    cfg, geo = pkg.config, pkg.geometry
    prm = cfg.params_from_values(end_time=1e9, **W[name])
    parts = geo.init_particles(prm)
    pos, vel = geo.developed_state(prm, parts, jitter=0.05, seed=12345)
    engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, pos=pos, vel=vel, native=True) for r in range(world)]
    slab.HipSlabEngine.group_run(engines, 48); [e.sync() for e in engines]
    if every:
        hw = max(prm.dp, prm.h)
        for e in engines:
            e.dens_part_enable(every=every, bands=[(0.5 * prm.DL, hw), (0.0, hw)])
    slab.HipSlabEngine.group_run(engines, 16); [e.sync() for e in engines]
    if every:
        for e in engines:
            e.dens_part_reset()
    t0 = time.perf_counter(); slab.HipSlabEngine.group_run(engines, steps); [e.sync() for e in engines]
    us = 1e6 * (time.perf_counter() - t0) / steps
    n_local = engines[0].layout()["n_local"]
    figures = []
    if every:
        ds = slab.ring_dens_stats(engines)
        fig = pkg.driver.density_figures(prm, ds)
        figures = [ds[0]["n_samples"], int(ds[0]["outliers"].sum()), round(float(fig["delta_rms"]), 6), round(float(fig["delta_max"]), 6)]
    for e in engines: e.close()
    return us, n_local, figures


if sys.argv[4] == "--one":
    us, n_local, figures = one(int(sys.argv[5]))
    print(f"FIGURE {us:.3f} {n_local} {figures}")
    sys.exit(0)

rounds, baseline = int(sys.argv[4]), (os.path.abspath(sys.argv[5]) if len(sys.argv) > 5 else None)
assert baseline is None or os.path.exists(baseline), f"{baseline}: build the parent's library with tools/build_baseline_lib.sh first"
MODES = {"off": 0, "every=1": 1, "every=10": 10}
got, n_local = {m: [] for m in MODES}, None
for _ in range(rounds):
    for m in ("off", "every=1", "off", "every=10"):
        env = dict(os.environ)
        env.pop("SPHX_LIB", None)
        if m == "off" and baseline:
            env["SPHX_LIB"] = baseline
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(world), str(steps), "--one", str(MODES[m])],
                           env=env, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:  # (a figure that could not be made ends the probe: nothing more is started on the device)
            sys.exit(f"{m}: exit status {r.returncode}\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("FIGURE ")][-1].split(None, 3)
        got[m].append(float(line[1]))
        n_local = int(line[2])
        print(f"  {m:9s} {float(line[1]):9.1f} us/step  [samples, outliers, delta_rms, delta_max] {line[3]}", flush=True)
off = statistics.median(got["off"])
print(f"{name}: ring of {world} slabs on one device, {steps} steps per figure, slab 0 holds {n_local} particles; off = {baseline or 'this build, sampler never enabled'}")
for m, v in got.items():
    print(f"  {m:9s} median {statistics.median(v):8.1f} us/step  {statistics.median(v) - off:+7.1f} us  ratio to off {statistics.median(v) / off:5.3f}  "
          f"min {min(v):.1f} max {max(v):.1f}  rounds: " + " ".join(f"{x:.1f}" for x in v))
