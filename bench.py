#!/usr/bin/env python3
"""bench.py -- particle-steps/s of the device-resident SPH step on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload C2|C3|C4|C5|dp=..,DL=..] [--dump-outputs DIR] [--full]

A "step" is one full time step of SPH_Poiseuille.m:250-292 (density/KGC, viscous+gravity, transport
shift, dt rule, Verlet integration, periodic wrap, neighbour rebuild) on synthetic particles that are
resident in HBM when the timed region starts.  N=1 runs BASELINE.json's headline configuration
(configs[1]: dp = 0.025, DL = 3, DH = 1 -> 5 760 particles); N>1 shards the channel into x-slabs, one
rank per GPU.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line.  --full adds the side measurements on top:
per-kernel device times and the roofline of the dominant kernel, the C3/C4/C5 windows and the accuracy run of the
default workload (aux), and the CPU baseline.  --dump-outputs DIR writes the state of the last timed step as .npy files.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
PKG = "sph-poiseuille-flow_amd"

WORKLOADS = {  # BASELINE.json configs; actual particle counts are those of the reference initialiser
    "C1": dict(dp=0.04, DL=3.0),
    "C2": dict(dp=0.025, DL=3.0),
    "C3": dict(dp=0.01, DL=6.0),
    "C4": dict(dp=0.005, DL=12.0),
    "C5": dict(dp=0.002, DL=24.0),
}
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
# algorithmic bytes per fluid particle per pass mapped onto our kernels
BYTES_PER_FLUID = {"k_density": 40, "k_kgc": 56, "k_forces": 112 + 192, "k_continuity": 104,
                   "k_clock_scan": 0, "k_scatter": 8, "k_reorder": 16}
BYTES_PER_WALL = {"k_density": 24, "k_kgc": 24, "k_forces": 48, "k_continuity": 24}
# Large-channel kernels (<= 8 lanes per particle) write the output-only fields of a step -- force, force_prior (pass CD: 32 B)
# and rho, p (pass E: 16 B) -- in the LAST step of a batch only (FluidTmp::lazy_out): the bytes a replayed
# launch of those passes is credited with are SURVEY 8d's minus the fields it does not write.
LAZY_UNWRITTEN = {"k_forces": 32, "k_continuity": 16}
STEP_BYTES_FLUID, STEP_BYTES_WALL = 528, 120
DUMP_BYTES_MAX = 64 << 20  # --dump-outputs: the most all files together may hold
_ALIAS = {"k_density_build": "k_density", "k_density_walk": "k_density", "k_density_dyn": "k_density",
          "k_continuity_clock": "k_continuity"}


def algorithmic_bytes(kernel, nf, nw, lazy):
    """SURVEY 8d bytes of one launch of `kernel` on nf fluid / nw wall particles (lazy: see LAZY_UNWRITTEN)."""
    if kernel == "k_continuity_density":  # pass E of a step and pass A of the next one in one launch
        return algorithmic_bytes("k_continuity", nf, nw, lazy) + algorithmic_bytes("k_density", nf, nw, lazy)
    k = _ALIAS.get(kernel, kernel)
    per_fluid = BYTES_PER_FLUID.get(k, 0) - (LAZY_UNWRITTEN.get(k, 0) if lazy else 0)
    return per_fluid * nf + BYTES_PER_WALL.get(k, 0) * nw


def step_bytes(nf, nw, lazy):
    return (STEP_BYTES_FLUID - (sum(LAZY_UNWRITTEN.values()) if lazy else 0)) * nf + STEP_BYTES_WALL * nw

def parse_workload(s):
    if s in WORKLOADS:
        return s, dict(WORKLOADS[s])
    kw = {}
    for part in s.split(","):
        k, v = part.split("=")
        kw[k.strip()] = float(v)
    return s, kw


def cpu_baseline(cfg, geo, prm, parts, budget_s=20.0):
    """Oracle (kind 'port': our C restatement of the reference MEX path, same serial neighbour search +
    OpenMP parallel-for/atomic pair loops) on this box's host cores, bounded sample of the same workload."""
    import oracle
    oracle.build()
    nt = parts["n_total"]
    # the reference's pair loops are omp-parallel with atomic scatter and its neighbour search is serial, so
    # more threads is not faster: calibrate 1, 4, 8, 16 threads on a few steps and keep the fastest
    ncpu = os.cpu_count() or 1
    best = None
    for th in sorted({1, min(4, ncpu), min(8, ncpu), min(16, ncpu)}):
        oracle.set_num_threads(th)
        t0 = time.perf_counter()
        oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=8, enable_sort=False, omp=True)
        per = max((time.perf_counter() - t0) / 8, 1e-6)
        if best is None or per < best[1]:
            best = (th, per)
    threads, per_step = best
    oracle.set_num_threads(threads)
    n = int(max(10, min(20000, budget_s / per_step)))
    t0 = time.perf_counter()
    st = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=n, enable_sort=True, omp=True)
    dt = time.perf_counter() - t0
    return dict(value=nt * st["stats"]["steps"] / dt, unit="particle-steps/s", cores=int(threads), kind="port",
                sample=f"{st['stats']['steps']} steps of the same {nt}-particle workload "
                       f"({st['stats']['seconds_neighbor']:.1f}s serial neighbour search + "
                       f"{st['stats']['seconds_physics']:.1f}s OpenMP pair loops, {threads} threads)")


def dump_outputs(out_dir, fields, st):
    """--dump-outputs: what a caller of the timed path receives after its last step -- Context.download(), state and
    step outputs in the caller's row order, f64 -- as DIR/<field>.npy, and sim.npy = [step, t, dt, vmax].  When the
    arrays exceed DUMP_BYTES_MAX, every one of them keeps the same rows, a seeded sample (rows.npy: their numbers)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    n = len(next(iter(fields.values())))
    row_bytes = sum(a[:1].nbytes for a in fields.values())
    rows = None
    if n * row_bytes > DUMP_BYTES_MAX - (1 << 16):  # (the margin holds the .npy headers and sim.npy)
        k = (DUMP_BYTES_MAX - (1 << 16)) // (row_bytes + 8)
        rows = np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
        np.save(os.path.join(out_dir, "rows.npy"), rows.astype(np.float64))
    for name, a in fields.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a if rows is None else a[rows], dtype=np.float64))
    np.save(os.path.join(out_dir, "sim.npy"), np.array([st["step"], st["t"], st["dt_last"], st["vmax"]], dtype=np.float64))


def pmc_traffic(name, kernel, key="traffic_bytes"):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 --pmc passes (profiles/pmc_traffic.json:
    2*FETCH_SIZE + WRITE_SIZE, the gfx950 read-side correction of MI355X_MICROARCH.md applied); None if not profiled.
    key="valu_active_frac": the share of the launch's cycles in which its SIMDs issued vector-ALU instructions."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            return json.load(f)[name][{"k_continuity_clock": "k_continuity"}.get(kernel, kernel)][key]
    except (OSError, KeyError, ValueError):
        return None


def run_case(capi, cfg, geo, name, kw, steps, warmup, profile_steps, lpp=0, spg=0, lattice=False,
             rebuild_every=0, skin_h=0.0, dynamic=0, sustained=None, dump=None):
    """Time `steps` resident steps of one workload; returns (result dict, prm, parts, pos, vel).
    dump: directory for dump_outputs() of the last timed step, written before anything else runs on the context.
    sustained = (skip, n): afterwards run `skip` more steps untimed -- past the point where the synthetic start's jittered
    lattice has broken up -- and time another n: the rate a long physical run sustains, reported next to the window's."""
    import torch
    prm = cfg.params_from_values(end_time=1e9, **kw)
    parts = geo.init_particles(prm)
    nf, nw, nt = parts["n_fluid"], parts["n_wall"], parts["n_total"]
    if lattice:
        pos, vel, start = parts["pos"], parts["vel"], "lattice at rest"
    else:
        pos, vel = geo.developed_state(prm, parts, jitter=0.05, seed=12345)
        start = "developed (analytic parabola + 0.05dp jitter, seed 12345)"
    ctx = capi.Context(prm, nf, nt, pos, vel, parts["drho_dt"], parts["mass"], parts["wall_vel"], t_end=1e9,
                       lanes_per_particle=lpp, steps_per_graph=spg, rebuild_every=rebuild_every,
                       skin_h=skin_h, dynamic_rebin=dynamic)
    info, tuning, forms = ctx.info(), ctx.tuning(), ctx.kernel_forms()
    if warmup > 0:
        ctx.enqueue_steps(warmup)  # untimed: includes graph capture/instantiation
    st0 = ctx.sync()
    # still warm-up: capture (not run) the graph of a `steps`-long batch entered at the phase the warm-up ended in --
    # the one-time cost a caller with a fixed cadence pays on its first call
    ctx.prepare_steps(steps)
    g0 = ctx.graph_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.enqueue_steps(steps)
    st1 = ctx.sync()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    g1 = ctx.graph_stats()
    assert st1["step"] - st0["step"] == steps, (st0, st1)
    replay = {k: g1[k] - g0[k] for k in ("slots_replayed", "slots_eager", "graphs_captured")}
    if dump:
        dump_outputs(dump, ctx.download(), st1)
    roof, kernels = None, {}
    if profile_steps > 0:  # per-kernel device time, live: HIP event pair around every launch on the ctx stream
        ctx.profile_enable(True)
        ctx.enqueue_steps(profile_steps)
        ctx.sync()
        kernels = ctx.profile_read()
        ctx.profile_enable(False)
        if kernels:
            dom = max(kernels, key=lambda k: kernels[k]["avg_ms"] * kernels[k]["launches"])  # most device time
            ms_eager = kernels[dom]["avg_ms"]
            try:  # the dominant kernel alone, back-to-back in a replayed graph: the regime of the timed region
                ms = ctx.time_kernel(dom, reps=max(20, min(400, int(0.05 / max(ms_eager * 1e-3, 1e-7)))))
            except capi.SphxError:
                ms = ms_eager
            lazy = bool(forms["walk_kernels"])  # (single contexts on the large-channel kernels: lazy_out = 1)
            alg = algorithmic_bytes(dom, nf, nw, lazy)
            achieved = alg / (ms * 1e-3) / 1e9
            traffic = pmc_traffic(name, dom)
            roof = dict(bound="hbm", kernel=dom, achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=achieved / HBM_PEAK_GBS, traffic=traffic,
                        # what the launch really moved through HBM, as a fraction of the peak (None without a PMC record)
                        hbm_frac=(traffic / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                        traffic_over_algorithmic=(traffic / alg) if traffic and alg else None,
                        # context for a low HBM fraction: the same committed passes' vector-ALU utilisation (the pair
                        # arithmetic is FP64 on the vector ALU; the large-channel passes are bound there)
                        valu_busy_pmc=pmc_traffic(name, dom, "valu_active_frac"),
                        traffic_source="profiles/pmc_traffic.json: 2*FETCH_SIZE + WRITE_SIZE per launch from separate "
                                       "rocprofv3 --pmc passes of this kernel on this workload, committed -- not "
                                       "collected in this run (counters need the profiler)",
                        launch_ms=ms, launch_ms_eager=ms_eager,
                        algorithmic_bytes=alg, lazy_outputs=lazy,
                        algorithmic_bytes_note="SURVEY 8d bytes per launch" + (
                            " minus the output-only fields a non-final step does not write (force, force_prior: 32 B; rho, p: 16 B "
                            "per fluid particle)" if lazy else ""),
                        step_achieved=step_bytes(nf, nw, lazy) * steps / seconds / 1e9,
                        step_achieved_survey8d=step_bytes(nf, nw, False) * steps / seconds / 1e9)
    sus = None
    if sustained:
        skip, n_sus = sustained
        ctx.enqueue_steps(skip)
        s0 = ctx.sync()
        ctx.prepare_steps(n_sus)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.enqueue_steps(n_sus)
        s1 = ctx.sync()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        assert s1["step"] - s0["step"] == n_sus, (s0, s1)
        sus = dict(value=nt * n_sus / sec, ms_per_step=1e3 * sec / n_sus,
                   window=f"steps {s0['step']}..{s1['step']} after the start (the jittered lattice has broken up by step ~500)",
                   forced_rebuilds=ctx.grid_policy()["forced_rebuilds"])
    tuning.update(ctx.grid_policy())
    ctx.close()
    res = dict(value=nt * steps / seconds, ms_per_step=1e3 * seconds / steps, seconds=seconds, roofline=roof,
               kernels_ms={k: round(v["avg_ms"], 6) for k, v in kernels.items()},
               workload=f"{name}: dp={prm.dp}, DL={prm.DL}, DH={prm.DH}, n_fluid={nf}, n_wall={nw}, n_total={nt}, "
                        f"c_f={prm.c_f}, transport_coeff={prm.transport_coeff}; start={start}",
               cells=[info["n_cell_x"], info["n_cell_y"]], tuning=tuning, replay=replay, sustained=sus,
               sim={"t": st1["t"], "dt": st1["dt_last"], "vmax": st1["vmax"]})
    return res, prm, parts, pos, vel


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int, argv) -> int:
    """`python bench.py --gpus N` run bare (no launcher): start N ranks as CHILD processes, one per GPU, through
    torch.distributed.run on 127.0.0.1, relay their output and exit with their code.  This parent makes no GPU call and
    never replaces itself (no exec): it has not even imported torch."""
    import subprocess
    port = int(os.environ.get("MASTER_PORT") or _free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]
    sys.stderr.write(f"bench.py: --gpus {n} without a launcher: starting {n} ranks: {' '.join(cmd)}\n")
    sys.stderr.flush()
    rc = subprocess.call(cmd, env=env, cwd=ROOT)
    if rc != 0:
        sys.stderr.write(f"bench.py: the {n}-rank run failed (exit {rc})\n")
    raise SystemExit(rc)


def check_launch(rank: int, world: int, args) -> None:
    """--check-launch: every rank joins the gloo control plane, the ranks count themselves (all-reduce SUM of ones must
    equal --gpus), rank 0 prints the launch fields of the JSON line.  Touches no GPU."""
    n_seen = 1
    if world > 1:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo")
        one = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(one)
        n_seen = int(one.item())
        dist.barrier()
        dist.destroy_process_group()
    if n_seen != args.gpus:
        raise SystemExit(f"check-launch: {n_seen} rank(s) answered, --gpus {args.gpus}")
    if rank == 0:
        print(json.dumps({"metric": "particle-steps/s", "value": None, "unit": "particle-steps/s", "n_gpus": n_seen,
                          "steps": args.steps, "warmup": args.warmup, "check_launch": True}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--workload", default=None, help="C1..C5 or 'dp=0.01,DL=6' (default: C2 at 1 GPU)")
    ap.add_argument("--lpp", type=int, default=0, help="lanes per particle (0 = auto)")
    ap.add_argument("--spg", type=int, default=0, help="steps per hipGraph replay (0 = auto)")
    ap.add_argument("--rebuild-every", type=int, default=0, help="re-bin particles every K-th step (0 = auto)")
    ap.add_argument("--skin", type=float, default=0.0, help="cell skin in units of h (0 = sized from K)")
    ap.add_argument("--dynamic", type=int, default=0, help="device-side re-bin decision: 0 = by size, 1 = on, 2 = off")
    ap.add_argument("--full", action="store_true",
                    help="after the headline: per-kernel times + roofline, the C3/C4/C5 windows and accuracy run of the "
                         "default workload (aux), the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step computed as DIR/<name>.npy (f64, at most 64 MB)")
    ap.add_argument("--profile-steps", type=int, default=None,
                    help="with --full: eager steps timed per kernel with HIP events (default 200)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-aux", action="store_true", help="with --full: skip the side measurements of the default run")
    ap.add_argument("--cpu-budget", type=float, default=20.0)
    ap.add_argument("--lattice", action="store_true", help="pristine lattice start instead of the developed state")
    ap.add_argument("--check-launch", action="store_true",
                    help="bring the ranks up, agree on the world size over the control plane, print the line's launch "
                         "fields (value null) and exit: no GPU call, no compute")
    args = ap.parse_args()
    if args.profile_steps and not args.full:
        ap.error("--profile-steps times kernels in a --full run only")
    if args.dump_outputs and args.gpus > 1:
        ap.error("--dump-outputs writes the state of a --gpus 1 run only")
    profile_steps = (200 if args.profile_steps is None else args.profile_steps) if args.full else 0

    # ---- launch decision: BEFORE anything touches the GPU (a process that has initialised HIP must never start
    # or become another GPU program; the parent below only spawns children and relays their exit code) ----
    world_env = os.environ.get("WORLD_SIZE")
    under_launcher = world_env is not None and ("RANK" in os.environ or "TORCHELASTIC_RUN_ID" in os.environ)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if not under_launcher:
        if args.gpus > 1:
            return launch_ranks(args.gpus, sys.argv[1:])
        rank, world, local_rank = 0, 1, 0
    else:
        rank, world = int(os.environ.get("RANK", "0")), int(world_env)
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if world != args.gpus:  # includes world == 1 under a launcher with --gpus N: never measure something else silently
            sys.stderr.write(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} rank(s); run\n"
                             f"  python bench.py --gpus {args.gpus} ...   (bench.py starts its own ranks), or\n"
                             f"  python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 "
                             f"--master-port P bench.py --gpus {args.gpus} ...\n")
            raise SystemExit(2)
    if args.check_launch:  # rendezvous only: no GPU call, no compute -- what the CPU test of the launch logic runs
        return check_launch(rank, world, args)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (libsphx has no CPU fallback)")
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)

    pkg = importlib.import_module(PKG)
    cfg, geo, capi = pkg.config, pkg.geometry, pkg.capi
    capi.set_device(local_rank)

    if world > 1:
        slab = importlib.import_module(PKG + ".slab")
        return slab.bench_main(args, rank, world, local_rank)

    name, kw = parse_workload(args.workload or "C2")
    r, prm, parts, pos, vel = run_case(capi, cfg, geo, name, kw, args.steps, args.warmup, profile_steps, args.lpp,
                                       args.spg, args.lattice, args.rebuild_every, args.skin, args.dynamic,
                                       dump=args.dump_outputs)
    value = r["value"]
    out = {
        "metric": "particle-steps/s", "value": value, "unit": "particle-steps/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": r["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": r["workload"], "cells": r["cells"],
                   "lanes_per_particle": r["tuning"]["lanes_per_particle"],
                   "steps_per_graph": r["tuning"]["steps_per_graph"],
                   "rebuild_every": r["tuning"]["rebuild_every"], "skin": r["tuning"]["skin"],
                   "forced_rebuilds": r["tuning"]["forced_rebuilds"],
                   "timed_slots": r["replay"],  # step slots of the timed region replayed from hipGraphs / launched eagerly
                   "parallelism": "1 GPU, device-resident loop, " +
                                  ("hipGraph replay" if r["replay"]["slots_eager"] == 0 else
                                   f"hipGraph replay of {r['replay']['slots_replayed']} slots + {r['replay']['slots_eager']} eager launches")},
        "roofline": r["roofline"], "kernels_ms": r["kernels_ms"], "sim": r["sim"],
    }
    if args.full and not args.no_aux and args.workload is None:
        # the headline case is launch-latency bound (5 760 particles); report the same loop at 0.5 M and 6.1 M
        # particles as well so the kernels' throughput regime is on record (not the headline value)
        out["aux"] = {}
        # windows end before the synthetic start's jittered lattice breaks up (~500 steps in, a transient during which
        # nearly every step re-bins); sustained figures come from full physical runs
        # ... and, in the same context, the rate sustained once it has (`sustained`: 2 000 / 1 000 steps in)
        for aux_name, aux_steps, aux_sus in (("C3", 2000, None), ("C4", 300, (2000, 1000)), ("C5", 100, (1000, 300))):
            try:
                a = run_case(capi, cfg, geo, aux_name, dict(WORKLOADS[aux_name]), aux_steps, 40, 16 if aux_sus else 64, sustained=aux_sus)[0]
                out["aux"][aux_name] = {k: a[k] for k in ("value", "ms_per_step", "roofline", "kernels_ms", "workload", "tuning", "sustained")}
                out["aux"][aux_name]["window"] = (f"{aux_steps} steps right after a developed start; `sustained` = the same context "
                                                  "further in (disordered particles idle more lanes and the drift bound triggers "
                                                  "re-binnings); full physical runs: DESIGN.md section 4 / profiles/r0*_longrun_*.json")
            except Exception as e:  # never let the side measurements break the headline line
                out["aux"][aux_name] = {"error": repr(e)}
        # second half of the north-star metric: u(y) L2 vs the analytic parabola after the reference's full run
        # (dp = 0.025, lattice at rest, t = 20 s, output every second) -- about a second of GPU time
        try:
            driver = importlib.import_module(PKG + ".driver")
            full = driver.run(cfg.params_from_values(dp=0.025, DL=3.0, end_time=20.0, output_interval=1.0))
            out["accuracy"] = {"config": "dp=0.025, DL=3, lattice at rest, t_end=20 s (BASELINE.md section 2: reference 39 496 steps, L2 0.84 %)",
                               "L2": full.L2_error, "L2_mean_profile_t16_20": full.L2_time_mean(last=5), "steps": full.steps, "wall_seconds": full.wall_seconds,
                               "particle_steps_per_s": full.particle_steps_per_s,
                               "wall_shear": [full.tau_bottom, full.tau_top], "wall_shear_target": full.tau_target}
        except Exception as e:
            out["accuracy"] = {"error": repr(e)}
    if args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, geo, prm, dict(parts, pos=pos, vel=vel), args.cpu_budget)
        out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
