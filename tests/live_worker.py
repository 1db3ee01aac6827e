"""Child process of tests/test_gpu_live_neighbours.py: is a block of the device-memory pool ever recycled while somebody still
uses it?

All device memory of libsphx comes from the caching pool of csrc/sphx_common.hip, and a block goes back with a bare pool_free:
no stream, no event.  What keeps that right is one invariant -- a block returns to the pool only after every stream that was
given it has been waited for -- and it is kept by a sync somewhere in each call that releases memory: the temporaries of
download / monitor / the stateless modes, every sampler's enable (a reallocation), disable, reset and draining read, every
dropped graph, every destructor.  One object on one in-order stream cannot notice a missing sync (the next owner of the block
is ordered behind the last); tests/pool_history_worker.py looks at recycled blocks at quiescent points only.  Here objects
live SIDE BY SIDE, the risky call is made while the subject has N steps in flight, and capi.pool_poison_on_free(True, 3) fills
every block with the word 3 the moment it is released -- on the pool's own stream, which alone is waited for.  A block released
too early is then written by the fill (and by its next owner) while its former owner still reads or writes it, and the
former owner's or the new owner's numbers come out wrong.  The word 3 is an in-bounds index, count or cell as an int and a
denormal as a double pair on these shapes (tests/test_gpu_pool_history.py): wrong numbers, never a stray access.

A MOMENT: prepare_steps(N) on the subject; enqueue_steps(N) -- a pure replay, it returns at once; straight away one risky call,
on the subject or on a neighbour.  The REFERENCE of an object is the same sequence of calls on that object ALONE, with sync() in
front of every risky call and the poison off.  The library promises that call patterns do not change the bits, so everything an
object returns -- downloads, status, monitors, pair lists, every sampler's sums and records -- must be the same bytes in the
scene as alone.  Not equally wrong: the quiescent observation of every kind of object a scene holds (pool_history_worker's
observe on the scene's state) is checked against the oracle by pool_history_worker.check_fresh at the suite's tolerances, and
a context's scene script starts with that observation's own 35 steps, compared byte for byte with it.

IN FLIGHT FOR SURE is a condition: the child times enqueue_steps(N) + sync() of the subject alone (T_N) and, at every moment,
the host time from the return of enqueue_steps to the entry of the risky call; that must stay below T_N / 2 or the scene
fails as "not exercised".  N is chosen so that the host time is at most a tenth of T_N; N and both times go into the JSON.

A neighbour's round comes straight after the risky call, in front of any wait of the subject's: it enables its field map and
its history (two allocations with nothing released in front of them -- with the poison on, the pool hands out the block
released LAST, the subject's if it has just let one go), takes eight steps and returns everything.

The scenes (SCENES below has every object and every moment by name; tests/test_live_scenes_host.py takes a census of it):
    solo                every subject of pool_history_worker.SUBJECTS with its own 35-step call sequence, poison off, then on
    samplers_in_flight  a 16-lane context with all nine samplers on; per sampler its disable, its enable with another
                        configuration (in front of both it is enabled afresh with the scene's configuration, so both release
                        buffers of the sizes the neighbour asks for and the steps in flight write where a new owner would),
                        its reset, sample-now call and draining read where it has them (SAMPLERS)
    reads_in_flight     download, monitor(tau, pairs), the pair list, prepare_steps with another count, advance by a chunk that
                        has no graph; a 16-lane and a 2-lane (walk kernels) subject
    close_in_flight     a context, a batch of four closed with N steps in flight; at once pool_history_worker's observation of
                        a context (35 steps), of the stateless surface, as the newcomer
    neighbour_churn     beside a subject in flight: three contexts created, stepped three times, destroyed; the stateless
                        surface in full (pool_history_worker.observe_surface); a batch created, advanced to one time, destroyed
    ring                an in-process ring of two slabs, then of three, all its samplers on, group_run(N) in flight: every slab
                        sampler's *_part_disable and *_part_enable on slab 0 only, graph_prepare, and the engines closed one at
                        a time with no sync in front, first to last and last to first -- what the slabs still alive return is
                        read after the first close
    threads             three Python threads: a 16-lane and a 2-lane context, each created, prepared (its first capture),
                        stepped in chunks of CHUNKS with sampler reads in between and closed on its own thread, the
                        stateless surface three times on the third; each ends with a refused call and reads its own error id
Objects of one scene have equal sizes on purpose: a freed block must fall into a size class the neighbour asks for, which
pool_stats() hits show.  Moments the C ABI cannot express are not made: a batch has no prepare_steps (its first
enqueue_steps of a count captures, the one in flight replays), a ring has no pure-replay enqueue before graph_prepare
(group_run(N) launches kernel by kernel, so N is 60 there), and the history has neither a reset nor a sample-now call.

Prints ONE JSON line; exit code 0: ran to the end, whatever the comparisons said (threads: non-zero when a thread was still
alive at its time limit).

    python tests/live_worker.py --scene reads_in_flight
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    sys.path.insert(0, p)

import pool_history_worker as phw  # noqa: E402
from pool_history_worker import (FIELDS, PAIR_COLUMNS, STEPS, Env, check_fresh, enable_samplers, put, put_samplers,  # noqa: E402
                                 read_ctx)

POISON_WORD = 3
N_FLIGHT = 300                      # steps in flight at a moment (ring: 60, its steps are enqueued kernel by kernel)
N_RING = 60
WALL = dict(dp=0.025, DL=1.5)       # tests/switch_worker.py's moving-wall variant: 2 880 particles
CHUNKS = (5, 18, 1, 1, 10)          # 35 steps, as the threads take them
THREAD_SECONDS = 120.0
NEIGHBOUR_STEPS = 8
SOLO_SUBJECTS = tuple(phw.SUBJECTS)

# sampler -> (has a reset, has a sample-now call, the draining read or None); every one has <name>_enable and <name>_disable
SAMPLERS = {
    "flow_stats": (True, True, None),
    "history": (False, False, "history"),
    "field_map": (True, True, None),
    "probes": (False, True, "probes"),
    "profile_series": (False, True, "profile_series"),
    "pair_dist": (True, True, None),
    "grad_stats": (True, True, None),
    "tracers": (False, True, "tracers"),
    "dens_stats": (True, True, None),
}
RING_PARTS = ("field_part", "probes_part", "pairs_part", "grads_part", "tracers_part", "dens_part")


def _sampler_moments():
    out = []
    for s, (reset, sample, drain) in SAMPLERS.items():
        out.append((f"{s}.enable_other", "Context", f"{s}_enable"))
        if reset:
            out.append((f"{s}.reset", "Context", f"{s}_reset"))
        if sample:
            out.append((f"{s}.sample", "Context", f"{s}_sample"))
        if drain:
            out.append((f"{s}.drain", "Context", drain))
        out.append((f"{s}.disable", "Context", f"{s}_disable"))
    return out


def _read_moments(tag):
    return [(f"{tag}.download", "Context", "download"), (f"{tag}.monitor", "Context", "monitor"),
            (f"{tag}.pair_list", "Context", "neighbor_list"), (f"{tag}.prepare_other", "Context", "prepare_steps"),
            (f"{tag}.advance_new_chunk", "Context", "advance")]


def _ring_moments(world):
    out = []
    for s in RING_PARTS:
        out += [(f"w{world}.{s}.disable", "HipSlabEngine", f"{s}_disable"), (f"w{world}.{s}.enable", "HipSlabEngine", f"{s}_enable")]
    out.append((f"w{world}.graph_prepare", "HipSlabEngine", "graph_prepare"))
    out += [(f"w{world}.close_forward", "HipSlabEngine", "close"), (f"w{world}.close_backward", "HipSlabEngine", "close")]
    return out


# scene -> state ("wall": the moving-wall variant; "ring": pool_history_worker's own state, which its ring is cut from; "own":
# every subject of pool_history_worker on its own state), objects (label, subject of pool_history_worker.SUBJECTS whose kind and
# options it has) and moments (label, the class the risky call is made on, the call)
SCENES = {
    "solo": dict(state="own", objects=[(s, s) for s in SOLO_SUBJECTS],
                 moments=[(f"{s}.poisoned", "pool", "pool_poison_on_free") for s in SOLO_SUBJECTS]),
    "samplers_in_flight": dict(state="wall", objects=[("subject", "samplers"), ("neighbour", "samplers")], moments=_sampler_moments()),
    "reads_in_flight": dict(state="wall", objects=[("subject16", "ctx16"), ("subject2", "ctx2"), ("neighbour", "samplers")],
                            moments=_read_moments("lanes16") + _read_moments("lanes2")),
    "close_in_flight": dict(state="wall", objects=[("subject", "ctx16"), ("subject_batch", "batch4"), ("newcomer", "ctx16"),
                                                   ("newcomer_surface", "surface")],
                            moments=[("ctx_then_ctx", "Context", "close"), ("batch_then_ctx", "Batch", "close"),
                                     ("ctx_then_surface", "Context", "close")]),
    "neighbour_churn": dict(state="wall", objects=[("subject", "ctx16"), ("short_lived", "ctx16"), ("surface", "surface"),
                                                   ("batch", "batch4")],
                            moments=[("contexts_come_and_go", "Context", "close"), ("surface_runs", "mex_surface", "sph_physics_shell_mex"),
                                     ("batch_comes_and_goes", "Batch", "close")]),
    "ring": dict(state="ring", objects=[("ring", "ring2"), ("neighbour", "samplers")], moments=_ring_moments(2) + _ring_moments(3)),
    "threads": dict(state="wall", objects=[("thread16", "samplers"), ("thread2", "ctx2"), ("thread_surface", "surface")],
                    moments=[("first_prepare_16", "Context", "prepare_steps"), ("first_prepare_2", "Context", "prepare_steps"),
                             ("surface_x3", "mex_surface", "sph_physics_shell_mex")]),
}


def scene_envs(scene):
    """{subject: Env} of a scene, on the scene's state (no device needed)."""
    sc = SCENES[scene]
    if sc["state"] == "wall":
        phw.BASE = dict(phw.BASE, **WALL)  # (Env and Env.members read it when called: this process holds one scene)
    envs = {}
    for _, subject in sc["objects"]:
        if subject not in envs:
            envs[subject] = Env(subject)
    return envs


class Run:
    """One pass over a scene: live (neighbours side by side, no sync in front of a risky call, poison on) or quiet (one object
    alone, sync in front of every risky call, poison off)."""

    def __init__(self, live, n=N_FLIGHT):
        self.live, self.n = live, n
        self.out = {}      # object label -> {name: array}
        self.gaps = {}     # moment -> host seconds from the return of enqueue to the entry of the risky call
        self.t_n = {}      # subject label -> seconds of enqueue_steps(N) + sync() alone
        self.done = []     # moments made

    def obj(self, label):
        return self.out.setdefault(label, {})

    def time_flight(self, label, enqueue, sync):
        """T_N: N steps enqueued and waited for, nothing else going on (both passes make these calls: the same sequence)."""
        t0 = time.perf_counter()
        enqueue()
        sync()
        self.t_n[label] = time.perf_counter() - t0

    def moment(self, name, enqueue, sync, risky):
        """enqueue(): N steps of the subject, returns at once; risky(): the call under test, made straight away (quiet: after
        a sync).  -> what risky returned."""
        enqueue()
        t_ret = time.perf_counter()
        if not self.live:
            sync()
        t_in = time.perf_counter()
        got = risky()
        self.gaps[name] = t_in - t_ret
        self.done.append(name)
        return got


def ctx_flight(ctx, n):
    def enqueue():
        ctx.prepare_steps(n)
        ctx.enqueue_steps(n)
    return enqueue


def all_samplers_config(env, prm, parts, other=False):
    """The keywords of every sampler's enable: the scene's configuration, or another one (other sizes: a reallocation)."""
    from helpers import stats_bands
    pts, nf = env.probe_points(prm), parts["n_fluid"]
    ids = np.arange(5, nf, max(nf // 6, 1))[:6]
    if other:
        return dict(flow_stats=dict(every=1, n_bins=24), history=dict(every=1, capacity=4096), field_map=dict(every=1, nx=20, ny=12),
                    probes=dict(points=pts[:3], every=1, capacity=4096), profile_series=dict(every=1, n_bins=24, capacity=1024),
                    pair_dist=dict(every=1, n_bins=32), grad_stats=dict(every=1, n_bins=24),
                    tracers=dict(ids=ids[::-1][:4], every=1, capacity=4096), dens_stats=dict(every=1, n_bins=24, n_hist=32))
    return dict(flow_stats=dict(every=1, bands=stats_bands(prm)), history=dict(every=1), field_map=dict(every=1),
                probes=dict(points=pts, every=1), profile_series=dict(every=1), pair_dist=dict(every=1), grad_stats=dict(every=1),
                tracers=dict(ids=ids, every=1), dens_stats=dict(every=1))


def read_sampler(out, prefix, ctx, s):
    """Everything one sampler of a context returns."""
    if s == "flow_stats":
        for band in range(ctx._flow_stats[1]):
            put(out, f"{prefix}.flow_stats{band}", ctx.flow_stats_sums(band))
    elif s == "history":
        rec, dropped = ctx.history_records()
        put(out, f"{prefix}.history", dict(records=rec, n_dropped=dropped))
    elif s == "field_map":
        put(out, f"{prefix}.field_map", ctx.field_map_sums())
    elif s == "probes":
        put(out, f"{prefix}.probes", ctx.probes())
    elif s == "profile_series":
        put(out, f"{prefix}.profile_series", ctx.profile_series_sums())
    elif s == "pair_dist":
        for b, d in enumerate(ctx.pair_dist_sums()):
            put(out, f"{prefix}.pair_dist{b}", d)
    elif s == "grad_stats":
        put(out, f"{prefix}.grad_stats", ctx.grad_stats_sums(0))
    elif s == "tracers":
        put(out, f"{prefix}.tracers", ctx.tracers())
    else:
        put(out, f"{prefix}.dens_stats", ctx.dens_stats_sums(0))


def first_35(env, ctx, out):
    """The 35 steps of pool_history_worker.observe_ctx, read as it reads them: s35.* must be its bytes."""
    ctx.advance(1e9, max_steps=1)
    put(out, f"s{STEPS}.status", ctx.advance(1e9, max_steps=STEPS - 1))
    read_ctx(out, f"s{STEPS}", ctx)


# ---- scripts: generators that yield after every moment, so that a neighbour's round can follow at once ----
def neighbour_script(run, env, label="neighbour"):
    """A live context of the scene's sizes with pool_history_worker's four samplers on.  A round: the field map and the history
    are enabled (two allocations and nothing released in front of them: with the poison on the pool hands out the block
    released last, a block the subject has just let go if there is one), eight steps, everything read, and both are disabled
    again for the next round."""
    capi, out = env.capi, run.obj(label)
    with capi.Context.from_parts(env.prm, env.parts, t_end=1e9, lanes_per_particle=16) as ctx:
        enable_samplers(env, ctx, env.prm)
        ctx.field_map_disable()
        ctx.history_disable()
        k = 0
        while True:
            go_on = yield
            if not go_on:
                break
            ctx.field_map_enable(every=1)
            ctx.history_enable(every=1)
            put(out, f"round{k}.status", ctx.advance(1e9, max_steps=NEIGHBOUR_STEPS))
            put(out, f"round{k}", ctx.download(fields=FIELDS))
            put_samplers(out, f"round{k}", ctx)
            ctx.field_map_disable()
            ctx.history_disable()
            k += 1
        put(out, "end.status", ctx.sync())
        read_ctx(out, "end", ctx)
    yield


def samplers_script(run, env, label="subject"):
    capi, out, prm, parts = env.capi, run.obj(label), env.prm, env.parts
    on, other = all_samplers_config(env, prm, parts), all_samplers_config(env, prm, parts, other=True)
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=16) as ctx:
        for s in SAMPLERS:
            getattr(ctx, s + "_enable")(**on[s])
        first_35(env, ctx, out)
        run.time_flight(label, ctx_flight(ctx, run.n), ctx.sync)
        for s, (reset, sample, drain) in SAMPLERS.items():
            enable = getattr(ctx, s + "_enable")
            # disable first and enable-with-another-configuration second: both release buffers of the scene's own
            # configuration, the sizes the neighbour asks for; in front of each the sampler is enabled afresh, so that the
            # steps in flight write where a new owner of its buffers would
            calls = [("disable", getattr(ctx, s + "_disable")), ("enable_other", lambda s=s: getattr(ctx, s + "_enable")(**other[s]))]
            if reset:
                calls.append(("reset", getattr(ctx, s + "_reset")))
            if sample:
                calls.append(("sample", getattr(ctx, s + "_sample")))
            if drain:
                calls.append(("drain", lambda drain=drain: getattr(ctx, drain)(drain=True)))
            for what, call in calls:
                name = f"{s}.{what}"
                if what in ("disable", "enable_other"):
                    enable(**on[s])  # (quiescent: every moment ends with a sync)
                got = run.moment(name, ctx_flight(ctx, run.n), ctx.sync, call)
                yield  # the neighbour's round comes straight after the risky call, in front of any wait of the subject's
                if what == "drain":
                    put(out, name + ".drained", got)
                put(out, name + ".status", ctx.sync())
                if what != "disable":
                    read_sampler(out, name, ctx, s)
            enable(**on[s])  # all nine on again for the next sampler's moments
        put(out, "end.status", ctx.sync())
        read_ctx(out, "end", ctx)
        for s in SAMPLERS:
            read_sampler(out, "end", ctx, s)


def reads_script(run, env, tag, label):
    capi, out, prm, parts = env.capi, run.obj(label), env.prm, env.parts
    with capi.Context.from_parts(prm, parts, t_end=1e9, **env.kw) as ctx:
        env.facts.update(forms=ctx.kernel_forms(), tuning=ctx.tuning())
        first_35(env, ctx, out)
        run.time_flight(label, ctx_flight(ctx, run.n), ctx.sync)
        calls = [("download", lambda: ctx.download(fields=FIELDS)),
                 ("monitor", lambda: dict(zip(("tau_bottom", "tau_top", "pairs"), ctx.monitor(tau=True, pairs=True)))),
                 ("pair_list", lambda: dict(zip(PAIR_COLUMNS, ctx.neighbor_list()))),
                 ("prepare_other", lambda: ctx.prepare_steps(run.n + 7)),
                 ("advance_new_chunk", lambda: ctx.advance(1e9, max_steps=37))]
        for what, call in calls:
            name = f"{tag}.{what}"
            got = run.moment(name, ctx_flight(ctx, run.n), ctx.sync, call)
            yield  # the neighbour's round comes straight after the risky call, in front of any wait of the subject's
            if got is not None:
                put(out, name, got)
            put(out, name + ".status", ctx.sync())
            put(out, name + ".after", ctx.download(fields=FIELDS))
        read_ctx(out, tag + ".end", ctx)


def run_side_by_side(run, subject, neighbours):
    """live: after every moment of the subject every neighbour takes a round.  -> the rounds."""
    for nb in neighbours:
        next(nb)
    rounds = 0
    for _ in subject:
        rounds += 1
        for nb in neighbours:
            nb.send(True)
    for nb in neighbours:
        nb.send(False)
    return rounds


def run_alone(script, rounds=None):
    """quiet: a subject's script to its end (-> its moments), or a neighbour's for as many rounds as it took in the scene."""
    if rounds is None:
        return sum(1 for _ in script)
    next(script)
    for _ in range(rounds):
        script.send(True)
    script.send(False)
    return rounds


class Scene:
    """What a scene's child reports."""

    def __init__(self, name, capi):
        self.name, self.capi = name, capi
        self.failures, self.compared, self.differing = [], 0, []
        self.live, self.quiet = Run(True), Run(False)
        self.neighbour_pool = dict(hits=0, misses=0)
        self.fresh_checked = []
        self.use_poison = True  # (--no-poison: the live pass as it is, the mode never switched on; for profiles/r39_live_neighbours.txt)

    def poison(self, on):
        self.capi.pool_poison_on_free(on and self.use_poison, POISON_WORD)

    def fresh(self, env, obs=None):
        """The quiescent observation of this kind of object on the scene's state against its oracle (once per kind)."""
        if obs is None:
            obs = {}
            phw.OBSERVE[env.kind](env, env.prm, env.parts, obs)
        before = len(self.failures)
        check_fresh(env, obs, lambda m: self.failures.append(f"fresh {env.subject}: {m}"))
        self.fresh_checked.append(dict(subject=env.subject, arrays=len(obs), failures=len(self.failures) - before))
        return obs

    def link(self, label, obs, prefix=f"s{STEPS}"):
        """The scene script's first 35 steps are the observation's: the same bytes."""
        mine = self.quiet.out[label]
        for k, v in obs.items():
            if k.startswith(prefix + ".") and k in mine and mine[k].tobytes() != v.tobytes():
                self.failures.append(f"{label}: {k} of the scene script is not the quiescent observation's")

    def compare(self):
        for label, ref in self.quiet.out.items():
            got = self.live.out.get(label, {})
            if set(got) != set(ref):
                self.failures.append(f"{label}: different outputs {sorted(set(got) ^ set(ref))[:6]}")
            for k in sorted(set(got) & set(ref)):
                self.compared += 1
                if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype or got[k].tobytes() != ref[k].tobytes():
                    self.differing.append(f"{label}:{k}")
        if set(self.live.out) != set(self.quiet.out):
            self.failures.append(f"objects {sorted(set(self.live.out) ^ set(self.quiet.out))}")
        # in flight for sure
        for name, gap in self.live.gaps.items():
            t_n = min(self.live.t_n.values()) if self.live.t_n else 0.0
            if not gap < 0.5 * t_n:
                self.failures.append(f"not exercised: {name}: {gap:.2e} s from enqueue to the risky call, T_N = {t_n:.2e} s")
        want = [m[0] for m in SCENES[self.name]["moments"]]
        if sorted(self.live.done) != sorted(want) or sorted(self.quiet.done) != sorted(want):
            self.failures.append(f"moments made {sorted(self.live.done)} / {sorted(self.quiet.done)}, the table has {sorted(want)}")

    def neighbours(self, fn):
        """fn() with its pool hits and misses added to the neighbours' account."""
        before = self.capi.pool_stats()
        got = fn()
        after = self.capi.pool_stats()
        for k in self.neighbour_pool:
            self.neighbour_pool[k] += after[k] - before[k]
        return got

    def report(self, **more):
        gaps, t_n = self.live.gaps, self.live.t_n
        return dict(scene=self.name, n_flight=self.live.n, t_n={k: round(v, 6) for k, v in t_n.items()},
                    t_n_quiet={k: round(v, 6) for k, v in self.quiet.t_n.items()},
                    gap_max=max(gaps.values()) if gaps else None, gap_worst=max(gaps, key=gaps.get) if gaps else None,
                    moments=len(self.live.done), poison=self.capi.pool_poison_stats(), pool=self.capi.pool_stats(),
                    neighbour_pool=self.neighbour_pool, compared=self.compared, differing=self.differing,
                    fresh=self.fresh_checked, failures=self.failures, **more)


# ---- the scenes ----
def scene_samplers(sc, envs):
    env = envs["samplers"]
    obs = sc.fresh(env)
    rounds = run_alone(samplers_script(sc.quiet, env))
    run_alone(neighbour_script(sc.quiet, env), rounds)
    sc.link("subject", obs)
    sc.poison(True)
    nb = neighbour_script(sc.live, env)
    rounds_live = run_side_by_side(sc.live, samplers_script(sc.live, env), [_counted(sc, nb)])
    sc.poison(False)
    assert rounds_live == rounds


class _counted:
    """A neighbour's generator whose rounds are booked on the scene's neighbour account of pool hits and misses."""

    def __init__(self, sc, gen):
        self.sc, self.gen = sc, gen

    def __next__(self):
        return next(self.gen)

    def send(self, v):
        return self.sc.neighbours(lambda: self.gen.send(v))


def scene_reads(sc, envs):
    nb_env = envs["samplers"]
    sc.fresh(nb_env)
    for tag, subject, label in (("lanes16", "ctx16", "subject16"), ("lanes2", "ctx2", "subject2")):
        env = envs[subject]
        obs = sc.fresh(env)
        rounds = run_alone(reads_script(sc.quiet, env, tag, label))
        run_alone(neighbour_script(sc.quiet, nb_env, "neighbour." + tag), rounds)
        sc.link(label, obs)
        sc.poison(True)
        run_side_by_side(sc.live, reads_script(sc.live, env, tag, label), [_counted(sc, neighbour_script(sc.live, nb_env, "neighbour." + tag))])
        sc.poison(False)
    want = dict(ctx16=False, ctx2=True)
    for subject, walk in want.items():
        if envs[subject].facts["forms"]["walk_kernels"] != walk:
            sc.failures.append(f"{subject}: kernel forms {envs[subject].facts['forms']}")


def scene_close(sc, envs):
    """The newcomers are pool_history_worker's own observations (35 steps of a context; the stateless surface), so the quiet
    pass of a newcomer IS the observation check_fresh checks."""
    capi = sc.capi
    env16, envb, envs_ = envs["ctx16"], envs["batch4"], envs["surface"]
    prm, parts = env16.prm, env16.parts
    newcomers = {"ctx_then_ctx": env16, "batch_then_ctx": env16, "ctx_then_surface": envs_}
    quiet = {}
    for env in (env16, envs_):
        quiet[env.subject] = sc.fresh(env)
    sc.fresh(envb)

    def subject_ctx():
        return capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=16)

    def subject_batch():
        prms, parts_list = envb.members(prm, parts)
        return capi.Batch.from_parts(prms, parts_list, t_end=1e9, **envb.kw)

    for run in (sc.quiet, sc.live):
        sc.poison(run.live)
        for name, env in newcomers.items():
            batch = name.startswith("batch")
            subj = subject_batch() if batch else subject_ctx()
            subj.advance(1e9, max_steps=2)
            if batch:  # (a batch has no prepare_steps: the first enqueue of a count captures, the ones after it replay)
                def enqueue(subj=subj):
                    subj.enqueue_steps(run.n)
                enqueue()
                subj.sync()
            else:
                enqueue = ctx_flight(subj, run.n)
            run.time_flight(name, enqueue, subj.sync)
            run.moment(name, enqueue, subj.sync, subj.close)
            out = run.obj("newcomer." + name)
            if run.live:
                sc.neighbours(lambda: phw.OBSERVE[env.kind](env, env.prm, env.parts, out))
            else:
                out.update(quiet[env.subject])  # alone, in front of nothing: the observation itself
    sc.poison(False)


def scene_churn(sc, envs):
    capi = sc.capi
    env16, envb, envs_ = envs["ctx16"], envs["batch4"], envs["surface"]
    prm, parts = env16.prm, env16.parts
    obs16 = sc.fresh(env16)
    sc.fresh(envb)
    sc.fresh(envs_)

    def short_lived(out):
        for k in range(3):
            with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=16) as c:
                put(out, f"ctx{k}.status", c.advance(1e9, max_steps=3))
                put(out, f"ctx{k}", c.download(fields=FIELDS))

    def surface(out):
        phw.observe_surface(envs_, envs_.prm, envs_.parts, out)

    def batch(out, t_goal):
        prms, parts_list = envb.members(prm, parts)
        with capi.Batch.from_parts(prms, parts_list, t_end=1e9, **envb.kw) as b:
            sts = b.advance(t_goal)  # every member to one time: each by its own number of steps
            for m in range(len(prms)):
                put(out, f"m{m}.status", sts[m])
                put(out, f"m{m}", b.download(m, fields=FIELDS))
            put(out, "info", b.info())

    for run in (sc.quiet, sc.live):
        sc.poison(run.live)
        out = run.obj("subject")
        with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=16) as ctx:
            first_35(env16, ctx, out)
            t_goal = float(out[f"s{STEPS}.status.t"]) * 12.0 / STEPS
            run.time_flight("subject", ctx_flight(ctx, run.n), ctx.sync)
            acts = (("contexts_come_and_go", "short_lived", short_lived), ("surface_runs", "surface", surface),
                    ("batch_comes_and_goes", "batch", lambda o: batch(o, t_goal)))
            for name, label, act in acts:
                nb_out = run.obj(label)
                if run.live:
                    run.moment(name, ctx_flight(ctx, run.n), ctx.sync, lambda: sc.neighbours(lambda: act(nb_out)))
                else:  # alone: the subject's steps without a neighbour, the neighbour's work without the subject's
                    run.moment(name, ctx_flight(ctx, run.n), ctx.sync, lambda: None)
                put(out, name + ".status", ctx.sync())
                put(out, name, ctx.download(fields=FIELDS))
            read_ctx(out, "end", ctx)
        if not run.live:
            for name, label, act in acts:
                act(run.obj(label))
    sc.poison(False)
    sc.link("subject", obs16)


def ring_script(run, env, world, order, close_only):
    """An in-process ring with its samplers on and group_run(N) in flight.  close_only: the ring is made for the close moment
    alone (`order`: the engines closed one at a time, first to last or last to first, no sync in front)."""
    slab, capi, prm, parts = env.slab, env.capi, env.prm, env.parts
    ids = np.arange(5, parts["n_fluid"], max(parts["n_fluid"] // 6, 1))[:6]
    label = "ring"
    out = run.obj(label)
    engines = []
    part_on = dict(field_part=dict(every=1), probes_part=dict(points=env.probe_points(prm), every=1), pairs_part=dict(every=1),
                   grads_part=dict(every=1), tracers_part=dict(ids=ids, every=1), dens_part=dict(every=1))
    part_read = dict(field_part=lambda e: e.field_part_sums(), probes_part=lambda e: e.probes_part_records(),
                     pairs_part=lambda e: e.pairs_part_sums()[0], grads_part=lambda e: e.grads_part_sums(0),
                     tracers_part=lambda e: e.tracers_part_records(), dens_part=lambda e: e.dens_part_sums(0))

    def sync_all():
        return [e.sync() for e in engines]

    def flight():
        slab.HipSlabEngine.group_run(engines, run.n)

    enabled = dict(field_part="_field_part", probes_part="_probes_part", pairs_part="_pair_dist", grads_part="_grad_stats",
                   tracers_part="_tracers_part", dens_part="_dens_stats")  # what the wrapper keeps while a sampler is on

    def read_all(tag, which=None):
        for r, e in enumerate(which if which is not None else engines):
            r = engines.index(e)
            put(out, f"{tag}.r{r}.status", e.sync())
            put(out, f"{tag}.r{r}", e.snapshot())
            for band in range(3):
                put(out, f"{tag}.r{r}.stats{band}", e.flow_stats_sums(band))
            rec, dropped = e.history_records()
            put(out, f"{tag}.r{r}.history", dict(records=rec, n_dropped=dropped))
            for s in RING_PARTS:
                if getattr(e, enabled[s], None) is not None:
                    put(out, f"{tag}.r{r}.{s}", part_read[s](e))

    try:
        engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, native=True) for r in range(world)]
        for e in engines:
            enable_samplers(env, e, prm, ring=True)
            for s in RING_PARTS[2:]:
                getattr(e, s + "_enable")(**part_on[s])
        slab.HipSlabEngine.group_run(engines, 2)
        sync_all()
        run.time_flight(f"ring{world}", flight, sync_all)
        tag = f"w{world}"
        if not close_only:
            for s in RING_PARTS:
                for what, call in (("disable", getattr(engines[0], s + "_disable")),
                                   ("enable", lambda s=s: getattr(engines[0], s + "_enable")(**part_on[s]))):
                    name = f"{tag}.{s}.{what}"
                    run.moment(name, flight, sync_all, call)
                    yield  # (the neighbour's round straight after the risky call)
                    sync_all()
                    read_all(name)
            name = f"{tag}.graph_prepare"
            run.moment(name, flight, sync_all, lambda: slab.HipSlabEngine.graph_prepare(engines))
            yield
            slab.HipSlabEngine.group_run(engines, 20)  # two replays of the graph just made
            sync_all()
            read_all(name)
        else:
            name = f"{tag}.close_{order}"
            seq = engines if order == "forward" else engines[::-1]
            read_all(name + ".before")
            run.moment(name, flight, sync_all, seq[0].close)
            yield  # (a neighbour's round between the first engine's close and the next)
            read_all(name + ".survivors", which=seq[1:])  # a slab still alive is its owner's to read: its neighbour is gone, it is not
            for e in seq[1:]:
                e.close()
                yield
    finally:
        for e in engines:
            e.close()


def scene_ring(sc, envs):
    """Each slab sampler's *_part_disable and *_part_enable on slab 0 only, graph_prepare, and the engines closed one at a time
    in both orders, for a ring of two slabs and of three, a neighbour context stepping beside it.  What a closed ring returns
    cannot be read: the close moments are checked through the neighbour, which takes the blocks the slabs release."""
    env, nb_env = envs["ring2"], envs["samplers"]
    sc.fresh(env)
    sc.fresh(nb_env)
    for run in (sc.quiet, sc.live):
        run.n = N_RING
    for world in (2, 3):
        for order in ("all", "forward", "backward"):
            nb_label = f"neighbour.w{world}.{order}"
            mk = lambda run: ring_script(_Relabel(run, f"ring.w{world}.{order}"), env, world, order, order != "all")
            rounds = run_alone(mk(sc.quiet))
            run_alone(neighbour_script(sc.quiet, nb_env, nb_label), rounds)
            sc.poison(True)
            run_side_by_side(sc.live, mk(sc.live), [_counted(sc, neighbour_script(sc.live, nb_env, nb_label))])
            sc.poison(False)


class _Relabel:
    """A Run whose "ring" object is booked under another label (one ring per world and order)."""

    def __init__(self, run, label):
        self._run, self._label = run, label

    def obj(self, _):
        return self._run.obj(self._label)

    def __getattr__(self, k):
        return getattr(self._run, k)


def scene_solo(sc, envs, subjects):
    """Every subject of pool_history_worker with its own call sequence, poison off and then on: one object in one stream order
    must not notice the mode."""
    for s in subjects:
        env = envs[s]
        off = sc.quiet.obj(s)
        phw.OBSERVE[env.kind](env, env.prm, env.parts, off)
        sc.fresh(env, off)
        sc.quiet.done.append(f"{s}.poisoned")
        filled = sc.capi.pool_poison_stats()["filled"]
        sc.poison(True)
        sc.neighbours(lambda: phw.OBSERVE[env.kind](env, env.prm, env.parts, sc.live.obj(s)))
        sc.poison(False)
        sc.live.done.append(f"{s}.poisoned")
        if not sc.capi.pool_poison_stats()["filled"] > filled:
            sc.failures.append(f"{s}: no block was filled")


def thread_work(env, capi, kind, out, errs, name):
    """What one thread of the `threads` scene does; its own error id last."""
    try:
        if kind == "surface":
            for k in range(3):
                o = {}
                phw.observe_surface(env, env.prm, env.parts, o)
                put(out, f"run{k}", o)
            rc = capi.lib().sphx_neighbor_fetch(None, None, None, None, None, None, None, 0)  # (no search is pending)
        else:
            with capi.Context.from_parts(env.prm, env.parts, t_end=1e9, **env.kw) as ctx:
                enable_samplers(env, ctx, env.prm)
                done = 0
                for c in CHUNKS:
                    ctx.prepare_steps(c)  # (the first capture of this context happens on this thread)
                    done += c
                    put(out, f"s{done}.status", ctx.advance(1e9, max_steps=c))
                    put_samplers(out, f"s{done}", ctx)
                read_ctx(out, f"s{done}", ctx)
                rc = capi.lib().sphx_ctx_prepare_steps(ctx._h, C.c_int64(-1)) if kind == "ctx16" else capi.lib().sphx_pool_stats(None)
        errs[name] = (int(rc), capi.lib().sphx_last_error_id().decode())
    except BaseException as e:  # noqa: BLE001 -- reported by the child, thread by thread
        errs[name] = ("raised", repr(e))


def scene_threads(sc, envs):
    """Three threads (ctypes releases the GIL in every call): a 16-lane and a 2-lane context, each created, prepared (its first
    capture), stepped in chunks of CHUNKS with sampler reads in between and closed on its own thread, and the stateless surface
    three times on the third.  Every thread ends with a refused call of its own and reads sphx_last_error_id()."""
    capi = sc.capi
    e16, e2, es = envs["samplers"], envs["ctx2"], envs["surface"]
    work = (("thread16", e16, "ctx16"), ("thread2", e2, "ctx2"), ("thread_surface", es, "surface"))
    sc.fresh(es)
    errs_q, errs_l = {}, {}
    for name, env, kind in work:  # single-threaded, one after the other
        thread_work(env, capi, kind, sc.quiet.obj(name), errs_q, name)
    sc.quiet.done += [m[0] for m in SCENES["threads"]["moments"]]
    sc.poison(True)
    before = capi.pool_stats()
    threads = [threading.Thread(target=thread_work, args=(env, capi, kind, sc.live.obj(name), errs_l, name), daemon=True)
               for name, env, kind in work]
    for t in threads:
        t.start()
    deadline = time.time() + THREAD_SECONDS
    for t in threads:
        t.join(max(deadline - time.time(), 0.0))
    alive = [w[0] for w, t in zip(work, threads) if t.is_alive()]
    if alive:
        return alive
    after = capi.pool_stats()
    sc.poison(False)
    for k in sc.neighbour_pool:
        sc.neighbour_pool[k] += after[k] - before[k]
    sc.live.done += [m[0] for m in SCENES["threads"]["moments"]]
    if errs_l != errs_q:
        sc.failures.append(f"error ids: threads {errs_l}, single-threaded {errs_q}")
    ids = [v[1] for v in errs_l.values()]
    if len(set(ids)) != len(work) or any(v[0] in (0, "raised") for v in errs_l.values()):
        sc.failures.append(f"every thread must read its own error id: {errs_l}")
    # the 35th step is the oracle's: the chunked, sampled run against pool_history_worker's observation of the same context
    for name, env, kind in work[:2]:
        obs = {}
        env_plain = Env("samplers" if kind == "ctx16" else "ctx2")
        phw.observe_ctx(env_plain, env_plain.prm, env_plain.parts, obs)
        sc.fresh(env_plain, obs)
        for f in FIELDS:
            if obs[f"s{STEPS}.{f}"].tobytes() != sc.quiet.out[name][f"s{STEPS}.{f}"].tobytes():
                sc.failures.append(f"{name}: {f} after {STEPS} steps in chunks is not the quiescent observation's")
    return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", required=True, choices=list(SCENES))
    ap.add_argument("--subjects", default="", help="solo: the subjects of this child, comma-separated (default: all but ctx2tiles, "
                                                   "which needs SPHX_DEBUG_SWITCHES=tiles_be_from_1)")
    ap.add_argument("--no-poison", action="store_true", help="never switch the poison on (what does a scene see without it?)")
    ap.add_argument("--n", type=int, default=0, help="steps in flight at a moment (default: N_FLIGHT, a ring N_RING)")
    args = ap.parse_args()
    t0 = time.time()
    envs = scene_envs(args.scene)
    capi = next(iter(envs.values())).capi
    sc = Scene(args.scene, capi)
    sc.use_poison = not args.no_poison
    if args.n:
        sc.live.n = sc.quiet.n = args.n
    alive, more = [], {}
    try:
        if args.scene == "solo":
            subjects = [s for s in args.subjects.split(",") if s] or [s for s in SOLO_SUBJECTS if s != "ctx2tiles"]
            scene_solo(sc, envs, subjects)
            more["subjects"] = subjects
            SCENES["solo"]["moments"] = [(f"{s}.poisoned", "pool", "pool_poison_on_free") for s in subjects]
        elif args.scene == "samplers_in_flight":
            scene_samplers(sc, envs)
        elif args.scene == "reads_in_flight":
            scene_reads(sc, envs)
        elif args.scene == "close_in_flight":
            scene_close(sc, envs)
        elif args.scene == "neighbour_churn":
            scene_churn(sc, envs)
        elif args.scene == "ring":
            scene_ring(sc, envs)
        else:
            alive = scene_threads(sc, envs)
        if not alive:
            sc.compare()
    except capi.SphxError as e:
        sc.failures.append(f"the scene stopped at a refused call: {e!r}")
    more.update(overlap=os.environ.get("SPHX_SLAB_OVERLAP", ""), switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""),
                seconds=round(time.time() - t0, 3), threads_alive=alive)
    print(json.dumps(sc.report(**more)), flush=True)
    sys.stdout.flush()
    if alive:
        os._exit(3)  # a thread is stuck inside the library: no clean exit to be had
    return 0


if __name__ == "__main__":
    sys.exit(main())
