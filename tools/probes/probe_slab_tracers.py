"""What the particle tracers of a slab ring cost (manual probe): an in-process ring on one device, us per ring step with T
tracers recorded every step and every 16th (T = 1, 4096 and every fluid row, the same shuffled list on every slab) -- each
alternating with the tracers off, `rounds` times; medians of the rounds.  Off is the same build with the sampler never enabled.
python tools/probes/probe_slab_tracers.py C2x2 2 2000 3           (two C2 slabs)
python tools/probes/probe_slab_tracers.py C4 2 400 3              (two slabs of 0.24 M particles each)
The method is probe_slab_probes.py's: a host clock around group_run + sync of every slab, after a warm-up in the same setting.
A record of every row is large (capacity * T * 4 <= 1 << 27 doubles per slab), so a figure is taken in chunks of at most the
capacity, with a draining read -- not timed -- between them: no record is dropped."""
import importlib, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("sph-poiseuille-flow_amd")
slab = importlib.import_module("sph-poiseuille-flow_amd.slab")
cfg, geo = pkg.config, pkg.geometry
W = {"C2x2": dict(dp=0.025, DL=6.0), "C3": dict(dp=0.01, DL=6.0), "C4": dict(dp=0.005, DL=12.0)}
name, world, steps, rounds = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
prm = cfg.params_from_values(end_time=1e9, **W[name])
parts = geo.init_particles(prm)
pos, vel = geo.developed_state(prm, parts, jitter=0.05, seed=12345)
engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, pos=pos, vel=vel, native=True) for r in range(world)]
nf = parts["n_fluid"]
ids = np.random.default_rng(7).permutation(nf)
SETS = {"1": ids[:1], "4096": ids[:min(4096, nf)], "all": ids}
MODES = {"off": None, **{f"T={k} every={ev}": (k, ev) for k in SETS for ev in (1, 16)}}


def timed(mode):
    chunk = steps
    for e in engines:
        e.tracers_part_disable()
    if MODES[mode]:
        k, ev = MODES[mode]
        cap = max(1, min(steps // ev + 2, (1 << 27) // (4 * len(SETS[k]))))
        chunk = min(steps, cap * ev)
        for e in engines:
            e.tracers_part_enable(SETS[k], every=ev, capacity=cap)
    slab.HipSlabEngine.group_run(engines, 16); [e.sync() for e in engines]
    spent, left, dropped = 0.0, steps, 0
    while left > 0:
        if MODES[mode]:
            dropped += sum(e.tracers_part_records(drain=True)["n_dropped"] for e in engines)   # (not timed)
        n = min(chunk, left)
        t0 = time.perf_counter(); slab.HipSlabEngine.group_run(engines, n); [e.sync() for e in engines]
        spent += time.perf_counter() - t0
        left -= n
    if MODES[mode]:
        dropped += sum(e.tracers_part_records()["n_dropped"] for e in engines)
        assert dropped == 0, dropped
    return 1e6 * spent / steps


slab.HipSlabEngine.group_run(engines, 48); [e.sync() for e in engines]
got = {m: [] for m in MODES}
for _ in range(rounds):
    for m in [x for on in MODES if on != "off" for x in ("off", on)]:
        got[m].append(timed(m))
lay = engines[0].layout()
for e in engines:
    e.tracers_part_enable(SETS["4096"], capacity=1)
slab.HipSlabEngine.group_run(engines, 1)
owned = [int(e.tracers_part_records()["n_owned"][0]) for e in engines]
for e in engines: e.close()
off = statistics.median(got["off"])
print(f"{name}: ring of {world} slabs on one device, {steps} steps per figure, {nf} fluid rows, slab 0 holds {lay['n_local']} particles "
      f"(capacity {lay['capacity']}), of {len(SETS['4096'])} tracers the slabs own {owned}")
for m, v in got.items():
    print(f"  {m:18s} median {statistics.median(v):8.1f} us/step  ratio to off {statistics.median(v) / off:5.3f}  "
          f"min {min(v):.1f} max {max(v):.1f}  rounds: " + " ".join(f"{x:.1f}" for x in v))
