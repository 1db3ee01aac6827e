"""What the point probes of a slab ring cost (manual probe): an in-process ring on one device, us per ring step with P probes
recorded every step (every = 1; P = 1, 16, 256, 4096 random points, the same list on every slab) -- each alternating with
the probes off, `rounds` times; medians of the rounds.
python tools/probes/probe_slab_probes.py C2x2 2 2000 3           (two C2 slabs; C2x2 8: eight slabs)
python tools/probes/probe_slab_probes.py C2x2 2 2000 3 off-only   (off only, one figure per round: runs on a library without
                                                                  the slab probes too -- SPHX_LIB -- for the A/B against it)
The method is probe_slab_field_map.py's: a host clock around group_run + sync of every slab, after a warm-up in the same setting."""
import importlib, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("sph-poiseuille-flow_amd")
slab = importlib.import_module("sph-poiseuille-flow_amd.slab")
cfg, geo = pkg.config, pkg.geometry
W = {"C2x2": dict(dp=0.025, DL=6.0), "C3": dict(dp=0.01, DL=6.0), "C4": dict(dp=0.005, DL=12.0)}
name, world, steps, rounds = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
off_only = "off-only" in sys.argv[5:]
prm = cfg.params_from_values(end_time=1e9, **W[name])
parts = geo.init_particles(prm)
pos, vel = geo.developed_state(prm, parts, jitter=0.05, seed=12345)
engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, pos=pos, vel=vel, native=True) for r in range(world)]
rng = np.random.default_rng(7)
POINTS = {P: np.column_stack([rng.random(P) * prm.DL, rng.random(P) * prm.DH]) for P in (1, 16, 256, 4096)}
MODES = {"off": 0, **{f"P={P}": P for P in POINTS}}


def timed(mode):
    if not off_only:
        for e in engines:
            e.probes_part_disable()
            if MODES[mode]: e.probes_part_enable(POINTS[MODES[mode]], every=1, capacity=steps + 16)  # (no record is dropped)
    slab.HipSlabEngine.group_run(engines, 16); [e.sync() for e in engines]
    t0 = time.perf_counter(); slab.HipSlabEngine.group_run(engines, steps); [e.sync() for e in engines]
    return 1e6 * (time.perf_counter() - t0) / steps


slab.HipSlabEngine.group_run(engines, 48); [e.sync() for e in engines]
got = {m: [] for m in MODES}
for _ in range(rounds):
    for m in (["off"] if off_only else [x for P in POINTS for x in ("off", f"P={P}")]):
        got[m].append(timed(m))
lay = engines[0].layout()
owned = []
if not off_only:
    for e in engines:
        e.probes_part_enable(POINTS[4096], capacity=1)
        owned.append(len(e.probes_part_records()["index"]))
for e in engines: e.close()
lib = os.environ.get("SPHX_LIB", "this build")
off = statistics.median(got["off"])
print(f"{name}: ring of {world} slabs on one device, {steps} steps per figure, slab 0 holds {lay['n_local']} particles [{lib}]"
      + (f", of 4096 points the slabs own {owned}" if owned else ""))
for m, v in got.items():
    if v:
        print(f"  {m:8s} median {statistics.median(v):8.1f} us/step  ratio to off {statistics.median(v) / off:5.3f}  "
              f"min {min(v):.1f} max {max(v):.1f}  rounds: " + " ".join(f"{x:.1f}" for x in v))
