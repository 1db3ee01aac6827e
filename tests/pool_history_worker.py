"""Child process of tests/test_gpu_pool_history.py: does what an object computes depend on what the device-memory pool held
before?

All device memory of libsphx comes from a caching pool (csrc/sphx_common.hip) that hands a freed block to the next request of
its size class as it was returned.  A kernel that reads a row before it is written, or a call that returns a row nobody
wrote, then reads what the previous owner of the block left there -- in a test suite, usually the right answer of the test
before.  The library promises bit-identical results between runs, so one --subject is observed four times in ONE process:

    fresh     the subject as the first device work of the process
    foreign   after a predecessor of the same object kind, sizes and options on another state (seed 32, flowing to the left,
              walls moving the other way, wider mass spread), advanced 19 steps, with 8 more enqueued, closed without a sync
    scrub3    after capi.pool_scrub(3): every cached free block filled with the word 3 -- an in-bounds index, count or cell as
              an int, a denormal as a double: invisible inside a sum, visible bit for bit in a row nobody wrote
    nan       after a predecessor on the subject's own state with vel[3, 0] = NaN, advanced until SPHX_ERR_DIVERGED (the
              stateless surface: NaN in every payload argument, never in the pair-index or geometry columns)

`observe` collects everything the subject can return; --dump DIR writes it as DIR/<history>.npz, one array per name, for the
test to compare byte for byte.  capi.pool_stats() is read before a subject is created and after it is closed: in the three
later runs `misses` must not have grown (every block the subject took was a recycled one), which the child reports and the
test asserts.  The fresh run is also checked against the oracle (or, for a ring, against a single context; for the dual-rate
loop, against tests/dual_rate_reference.py) at the tolerances of the suite, and one sample of the field map and of the probes
against profile.shepard_field / shepard_points.  Prints ONE JSON line; exit code 0: ran to the end, whatever the comparisons
said.

    python tests/pool_history_worker.py --subject ctx2 --dump /tmp/ctx2
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    sys.path.insert(0, p)

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")
STATE = ("pos", "vel", "drho_dt")
PAIR_COLUMNS = ("pair_i", "pair_j", "dx", "dy", "r", "W", "dW")
HISTORIES = ("fresh", "foreign", "scrub3", "nan")
STEPS = 35
BASE = dict(dp=0.05, DL=3.0, jitter=0.25, seed=31, developed=True, rho0=2.5, transport_coeff=0.1)
FOREIGN = dict(seed=32, U_bulk=-0.666667, top_ux=-0.8, bottom_ux=0.3, mass_spread=0.4)
DUAL = dict(dp=0.025, DL=2.0, jitter=0.05, seed=2, developed=True)  # tests/test_gpu_dual_rate.py, default lanes
BATCH_MU = (1.0, 0.8, 1.25, 1.6)                                    # times the base state's mu, member by member
SURFACE_LISTS = ("skipped", "repeats", "empty_rows")                # of pair_list_cases.contract_lists, on both of its STATES

# subject -> (kind, context options)
SUBJECTS = {
    "ctx16": ("ctx", dict(lanes_per_particle=16)),
    "ctx32": ("ctx", dict(lanes_per_particle=32)),
    "ctx2": ("ctx", dict(lanes_per_particle=2)),
    "ctx4dyn": ("ctx", dict(lanes_per_particle=4, dynamic_rebin=1, rebuild_every=8)),
    "ctxK1": ("ctx", dict(lanes_per_particle=16, rebuild_every=1)),
    "ctx2tiles": ("ctx", dict(lanes_per_particle=2)),                # under SPHX_DEBUG_SWITCHES=tiles_be_from_1
    "dual": ("ctx", dict(dual_rate=2)),
    "samplers": ("ctx", dict(lanes_per_particle=16)),
    "batch4": ("batch", dict(lanes_per_particle=16)),
    "ring2": ("ring", dict()),
    "surface": ("surface", dict()),
}
RING_RUNS = (("auto", dict()), ("k5", dict(rebuild_every=5)))


class Env:
    """The modules and the states of one subject."""

    def __init__(self, subject):
        self.subject = subject
        self.kind, self.kw = SUBJECTS[subject]
        self.pkg = importlib.import_module("sph-poiseuille-flow_amd")
        self.capi, self.mex, self.profile = self.pkg.capi, self.pkg.mex_surface, self.pkg.profile
        self.slab = importlib.import_module("sph-poiseuille-flow_amd.slab")
        self.sampled = subject in ("samplers", "batch4", "ring2")
        from helpers import make_case, make_variant
        cfg, geo = self.pkg.config, self.pkg.geometry
        if subject == "dual":
            self.prm, self.parts = make_case(cfg, geo, **DUAL)
            self.f_prm, self.f_parts = make_variant(cfg, geo, **dict(DUAL, **FOREIGN))
        else:
            self.prm, self.parts = make_variant(cfg, geo, **BASE)
            self.f_prm, self.f_parts = make_variant(cfg, geo, **dict(BASE, **FOREIGN))
        assert self.f_parts["n_total"] == self.parts["n_total"] and self.f_parts["n_fluid"] == self.parts["n_fluid"]
        self.n_parts = dict(self.parts, vel=np.array(self.parts["vel"], order="F", copy=True))
        self.n_parts["vel"][3, 0] = np.nan
        self.facts = {}
        self.cache = {}  # the stateless surface: the oracle's outputs the modes take as inputs, made once

    def probe_points(self, prm):
        """On x = 0, mid-channel, within 2h of the bottom wall, and on the top wall line one period and a half to the right
        (folded into [0, DL)).  A point outside [0, DH] is refused by probes_enable and this state has no void inside."""
        return np.array([(0.0, 0.37 * prm.DH), (0.5 * prm.DL, 0.5 * prm.DH), (0.7 * prm.DL, 0.5 * prm.h), (1.5 * prm.DL + 0.01, prm.DH)])

    def members(self, prm, parts):
        """The four members of a batch on one state: mu differs"""
        from helpers import make_variant
        cfg, geo = self.pkg.config, self.pkg.geometry
        kw = dict(BASE, **FOREIGN) if prm is self.f_prm else BASE
        prms = [make_variant(cfg, geo, **dict(kw, mu=prm.mu * f))[0] for f in BATCH_MU]
        return prms, [parts] * len(prms)


def put(out, prefix, d):
    for k, v in d.items():
        out[f"{prefix}.{k}"] = np.asarray(v)


def enable_samplers(env, obj, prm, ring=False):
    from helpers import stats_bands
    obj.flow_stats_enable(every=1, bands=stats_bands(prm))
    obj.history_enable(every=1)
    if ring:
        obj.field_part_enable(every=1)
        obj.probes_part_enable(env.probe_points(prm), every=1)
    else:
        obj.field_map_enable(every=1)
        obj.probes_enable(env.probe_points(prm), every=1)


def put_samplers(out, prefix, obj, member=None, ring=False):
    """Everything the four samplers return (of one member of a batch)."""
    pick = (lambda v: v) if member is None else (lambda v: v[member])
    for band in range(3):
        put(out, f"{prefix}.stats{band}", pick(obj.flow_stats_sums(band)))
    rec, dropped = pick(obj.history_records())
    put(out, f"{prefix}.history", dict(records=rec, n_dropped=dropped))
    put(out, f"{prefix}.field", obj.field_part_sums() if ring else pick(obj.field_map_sums()))
    put(out, f"{prefix}.probes", obj.probes_part_records() if ring else pick(obj.probes()))


def read_ctx(out, tag, ctx, first=False):
    put(out, tag, ctx.download(fields=STATE if first else FIELDS))
    tb, tt, npairs = ctx.monitor(tau=not first, pairs=True)  # (wall shear needs Vol / B of a completed step)
    put(out, tag, dict(pairs=npairs) if first else dict(pairs=npairs, tau_bottom=tb, tau_top=tt))
    put(out, tag + ".list", dict(zip(PAIR_COLUMNS, ctx.neighbor_list())))


def observe_ctx(env, prm, parts, out, steps=STEPS, until_diverged=False):
    capi = env.capi
    with capi.Context.from_parts(prm, parts, t_end=1e9, **env.kw) as ctx:
        env.facts.update(forms=ctx.kernel_forms(), substeps=ctx.substeps(), tuning=ctx.tuning())
        if env.sampled:
            enable_samplers(env, ctx, prm)
        if until_diverged:
            return run_until_diverged(capi, lambda: ctx.advance(1e9, max_steps=4))
        if out is None:  # the foreign predecessor: the other buffer parity live, work still enqueued at the close
            ctx.advance(1e9, max_steps=19)
            ctx.enqueue_steps(8)
            return
        read_ctx(out, "s0", ctx, first=True)
        put(out, "s1.status", ctx.advance(1e9, max_steps=1))
        read_ctx(out, "s1", ctx)
        put(out, f"s{steps}.status", ctx.advance(1e9, max_steps=steps - 1))
        read_ctx(out, f"s{steps}", ctx)
        put(out, "end.status", ctx.sync())
        put(out, "end.policy", ctx.grid_policy())
        put(out, "end.schedule", ctx.schedule())
        if env.sampled:
            put_samplers(out, "end", ctx)
            ctx.field_map_reset()
            ctx.field_map_sample()      # one sample of the state just downloaded: what the numpy definition is compared with
            put(out, "one.field", ctx.field_map_sums())


def run_until_diverged(capi, advance):
    try:
        advance()
    except capi.SphxError as e:
        assert e.code == capi.SPHX_ERR_DIVERGED, e
        return
    raise AssertionError("the NaN predecessor did not raise SPHX_ERR_DIVERGED")


def observe_batch(env, prm, parts, out, steps=STEPS, until_diverged=False):
    capi = env.capi
    prms, parts_list = env.members(prm, parts)
    with capi.Batch.from_parts(prms, parts_list, t_end=1e9, **env.kw) as b:
        enable_samplers(env, b, prm)
        if until_diverged:
            return run_until_diverged(capi, lambda: b.advance(1e9, max_steps=4))
        if out is None:
            b.advance(1e9, max_steps=19)
            b.enqueue_steps(8)
            return

        def read(tag, first=False, sts=None):
            for m in range(len(prms)):
                put(out, f"{tag}.m{m}", b.download(m, fields=STATE if first else FIELDS))
                tb, tt, npairs = b.monitor(m, tau=not first, pairs=True)
                put(out, f"{tag}.m{m}", dict(pairs=npairs) if first else dict(pairs=npairs, tau_bottom=tb, tau_top=tt))
                if sts:
                    put(out, f"{tag}.m{m}.status", sts[m])

        read("s0", first=True)
        read("s1", sts=b.advance(1e9, max_steps=1))
        read(f"s{steps}", sts=b.advance(1e9, max_steps=steps - 1))
        put(out, "end.info", b.info())
        for m in range(len(prms)):
            put_samplers(out, f"end.m{m}", b, member=m)
        b.field_map_reset()
        b.field_map_sample()
        for m, s in enumerate(b.field_map_sums()):
            put(out, f"one.m{m}.field", s)


def observe_ring(env, prm, parts, out, steps=STEPS, until_diverged=False):
    slab, capi = env.slab, env.capi
    for tag, kw in RING_RUNS:
        engines = []
        try:
            engines = [slab.HipSlabEngine(prm, parts, r, 2, 0, t_end=1e9, native=True, **kw) for r in range(2)]
            for e in engines:
                enable_samplers(env, e, prm, ring=True)
            run = lambda n: slab.HipSlabEngine.group_run(engines, n)
            if until_diverged:  # the slab that owns the NaN raises it at its sync; its neighbour hears of it through the maxima
                run(4)
                codes = []
                for e in engines:
                    try:
                        e.sync()
                    except capi.SphxError as err:
                        codes.append(err.code)
                assert capi.SPHX_ERR_DIVERGED in codes, codes
                continue
            if out is None:
                run(19)
                run(8)
                continue

            def read(name):
                for r, e in enumerate(engines):
                    put(out, f"{tag}.{name}.r{r}.status", e.sync())
                    put(out, f"{tag}.{name}.r{r}", e.snapshot())

            read("s0")
            run(1)
            read("s1")
            run(steps - 1)
            read(f"s{steps}")
            for r, e in enumerate(engines):
                put_samplers(out, f"{tag}.end.r{r}", e, ring=True)
        finally:
            for e in engines:
                e.close()


def surface_inputs(env):
    """(name, prm, parts, list entry) of every list of part (b), made on the CPU once: the oracle's list of
    pair_list_cases.STATES turned into the lists with skipped (out-of-range), repeated and empty rows."""
    if "lists" not in env.cache:
        import oracle
        import pair_list_cases
        cfg, geo = env.pkg.config, env.pkg.geometry
        env.cache["lists"] = []
        for sname, make in pair_list_cases.STATES.items():
            prm, parts = make(cfg, geo)
            nb = oracle.neighbor_search(parts["pos"], parts["n_fluid"], parts["n_total"], prm.h, prm.DL)
            lists = pair_list_cases.contract_lists(oracle, prm, parts, nb)
            for lname in SURFACE_LISTS:
                env.cache["lists"].append((f"{sname}.{lname}", prm, parts, lists[lname]))
    return env.cache["lists"]


def observe_surface(env, prm, parts, out, steps=None, until_diverged=False):
    """The search on the state, the eight modes (helpers.run_modes) on the search's own list (a) and on the lists of part
    (b).  Every mode takes the oracle's outputs of the modes before it as its inputs (made once, on the fresh run's list), so
    all histories and the oracle see identical inputs.  until_diverged: the NaN predecessor -- the same calls with NaN in
    every payload argument (mass, pos, vel, drho_dt, and Vol, B, rho, force through `given`), the lists as they are."""
    import oracle
    from helpers import oracle_surface, run_modes
    mex = env.mex
    nb = mex.sph_neighbor_search_mex(parts["pos"], parts["n_fluid"], parts["n_total"], prm.h, prm.DL)
    runs = [("own" if prm is env.prm else "own_foreign", prm, parts, dict(nb=nb, h=prm.h, monitor_nb=None))] + surface_inputs(env)
    if out is not None:
        put(out, "search", dict(zip(PAIR_COLUMNS, nb)))
    for name, rprm, rparts, c in runs:
        if name not in env.cache:
            env.cache[name] = run_modes(oracle_surface(oracle), rprm, rparts, c["nb"], h=c["h"], monitor_nb=c["monitor_nb"])
            env.cache.setdefault("meta", {})[name] = (rprm, rparts, c)
        given = env.cache[name]
        if until_diverged:
            nan = lambda a: np.full_like(np.asarray(a, dtype=np.float64), np.nan)
            rparts = dict(rparts, **{k: nan(rparts[k]) for k in ("mass", "pos", "vel", "drho_dt")})
            given = {k: nan(v) for k, v in given.items()}
        got = run_modes(mex.sph_physics_shell_mex, rprm, rparts, c["nb"], h=c["h"], given=given, monitor_nb=c["monitor_nb"])
        if out is not None:
            put(out, name, got)


OBSERVE = dict(ctx=observe_ctx, batch=observe_batch, ring=observe_ring, surface=observe_surface)


# ---- the fresh run is the right answer ----
def check_state(tag, got, status, mon, ref, prm, nf, fail, steps=STEPS):
    from helpers import assert_close
    rs = ref["stats"]

    def check(name, fn):
        try:
            fn()
        except AssertionError as e:
            fail(f"{tag} {name}: {e}")

    for k in FIELDS:
        check(k, lambda k=k: assert_close(got[k], ref[k], rtol=1e-9, atol_scale=1e-10, name=k))
    if mon is not None:
        check("tau", lambda: assert_close(np.array(mon[:2]), np.array([rs["tau_bottom"], rs["tau_top"]]), rtol=1e-8, atol_scale=1e-9,
                                          name="tau"))
        if mon[2] != rs["n_pairs_last"]:
            fail(f"{tag} pairs {mon[2]} vs {rs['n_pairs_last']}")
    if status["step"] != steps or rs["steps"] != steps:
        fail(f"{tag} steps {status['step']} / {rs['steps']}")
    if abs(status["t"] - rs["t"]) > 1e-13 * rs["t"]:
        fail(f"{tag} t {status['t']!r} vs {rs['t']!r}")
    if abs(status["dt_last"] - rs["dt_last"]) > 1e-12 * rs["dt_last"]:
        fail(f"{tag} dt {status['dt_last']!r} vs {rs['dt_last']!r}")
    if abs(status["vmax"] - rs["vmax"]) > 1e-9 * rs["vmax"]:
        fail(f"{tag} vmax {status['vmax']!r} vs {rs['vmax']!r}")


def sub(obs, prefix):
    return {k[len(prefix) + 1:]: v for k, v in obs.items() if k.startswith(prefix + ".")}


def check_start(tag, obs, prefix, parts, prm, fail):
    import oracle
    nf, nt = parts["n_fluid"], parts["n_total"]
    for k in STATE:
        if obs[f"{prefix}.{k}"].tobytes() != np.asarray(parts[k], dtype=np.float64).tobytes():
            fail(f"{tag} step 0: {k} is not the input")
    n_ref = len(oracle.neighbor_search(parts["pos"], nf, nt, prm.h, prm.DL)[0])
    if float(obs[f"{prefix}.pairs"]) != n_ref:
        fail(f"{tag} step 0: {float(obs[f'{prefix}.pairs'])} pairs, the oracle {n_ref}")


def check_samples(env, tag, obs, end, one, state, prm, parts, fail):
    """One sample of the field map (taken at the end, after a reset) and the last record of the probes against the numpy
    definitions on the downloaded state, at the sampler tests' bound (1e-12 of a plane's / a column's largest |value|)."""
    import probe_cases
    from test_gpu_field_map import _assert_planes_match, _numpy_planes
    nf = parts["n_fluid"]
    nx, ny = env.capi.field_map_shape(prm)
    f = env.profile.shepard_field(state["pos"][:nf], state["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny)
    probes = sub(obs, end + ".probes")
    want = probe_cases.numpy_probes(env.profile, prm, parts, state, env.probe_points(prm))
    try:
        _assert_planes_match(sub(obs, one), _numpy_planes(env.profile, prm, f), f"{tag} field map")
        assert int(obs[one + ".n_samples"]) == 1
        assert probes["step"].tolist() == list(range(1, STEPS + 1)) and int(probes["n_dropped"]) == 0, probes["step"]
        assert np.array_equal(probes["points"], want["points"])
        probe_cases.assert_values_match(probes, want, f"{tag} probes", row=STEPS - 1)
    except AssertionError as e:
        fail(f"{tag} samplers: {e}")


def check_fresh(env, obs, fail):
    import oracle
    prm, parts = env.prm, env.parts
    nf = parts["n_fluid"]
    end = f"s{STEPS}"
    if env.kind == "ctx":
        check_start(env.subject, obs, "s0", parts, prm, fail)
        if env.subject == "dual":
            import dual_rate_reference as drr
            ref = drr.run(prm, parts, env.facts["substeps"], max_outer=STEPS)
            ref["stats"] = dict(steps=ref["steps"], t=ref["t"], dt_last=ref["dt_last"], vmax=ref["vmax"])
            mon = None
        else:
            ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=STEPS, enable_sort=False)
            mon = (float(obs[end + ".tau_bottom"]), float(obs[end + ".tau_top"]), float(obs[end + ".pairs"]))
        st = {k: obs[f"{end}.status.{k}"].item() for k in ("step", "t", "dt_last", "vmax")}
        check_state(env.subject, sub(obs, end), st, mon, ref, prm, nf, fail)
        if env.sampled:
            check_samples(env, env.subject, obs, "end", "one.field", sub(obs, end), prm, parts, fail)
    elif env.kind == "batch":
        prms, _ = env.members(prm, parts)
        for m, pm in enumerate(prms):
            check_start(f"member {m}", obs, f"s0.m{m}", parts, pm, fail)
            ref = oracle.run(pm, parts, t_end=1e9, output_interval=1e9, max_steps=STEPS, enable_sort=False)
            got = sub(obs, f"{end}.m{m}")
            st = {k: obs[f"{end}.m{m}.status.{k}"].item() for k in ("step", "t", "dt_last", "vmax")}
            check_state(f"member {m}", got, st, (float(got["tau_bottom"]), float(got["tau_top"]), float(got["pairs"])), ref, pm, nf, fail)
            check_samples(env, f"member {m}", obs, f"end.m{m}", f"one.m{m}.field", got, pm, parts, fail)
    elif env.kind == "ring":
        from helpers import assert_close
        with env.capi.Context.from_parts(prm, parts, t_end=1e9) as ctx:  # tests/test_slab.py, test_slab_native_ring_in_one_process
            rs = ctx.advance(1e9, max_steps=STEPS)
            ref = ctx.download(fields=STATE)
        for tag, _ in RING_RUNS:
            pos, vel, drho = np.full((nf, 2), np.nan), np.full((nf, 2), np.nan), np.full(nf, np.nan)
            seen = np.zeros(nf, dtype=int)
            for r in range(2):
                sn = sub(obs, f"{tag}.{end}.r{r}")
                o = sn["owned"]
                i = sn["id"][o]
                pos[i, 0], pos[i, 1], vel[i, 0], vel[i, 1], drho[i] = sn["x"][o], sn["y"][o], sn["vx"][o], sn["vy"][o], sn["drho"][o]
                np.add.at(seen, i, 1)
                if int(sn["status.step"]) != STEPS or abs(float(sn["status.t"]) - rs["t"]) > 1e-12 * rs["t"]:
                    fail(f"ring {tag} rank {r}: step {int(sn['status.step'])} t {float(sn['status.t'])!r} vs {rs['t']!r}")
            if not np.all(seen == 1):
                fail(f"ring {tag}: {int((seen == 0).sum())} particles unowned, {int((seen > 1).sum())} owned twice")
                continue
            pos[:, 0] -= np.round((pos[:, 0] - ref["pos"][:nf, 0]) / prm.DL) * prm.DL  # a slab keeps x in its window's frame
            for name, a, b in (("pos", pos, ref["pos"][:nf]), ("vel", vel, ref["vel"][:nf]), ("drho_dt", drho, ref["drho_dt"][:nf])):
                try:
                    assert_close(a, b, rtol=1e-9, atol_scale=1e-10, name=name)
                except AssertionError as e:
                    fail(f"ring {tag}: {e}")
    else:
        from test_gpu_pair_list_contract import compare
        for name, (rprm, rparts, c) in env.cache["meta"].items():
            if name == "own_foreign":
                continue
            # (the floors of the tolerances come from the rows the modes read: not from the skipped rows' NaN geometry)
            read = tuple(col[~c["mask"]] for col in c["nb"]) if c.get("nan_rows") else c["nb"]
            try:
                compare(f"surface {name}", sub(obs, name), env.cache[name], rprm, rparts, read)
            except AssertionError as e:
                fail(f"surface {name}: {e}")
        import oracle as orc
        from helpers import canon_pairs
        a = canon_pairs(tuple(obs[f"search.{k}"] for k in PAIR_COLUMNS))
        b = canon_pairs(orc.neighbor_search(parts["pos"], nf, parts["n_total"], prm.h, prm.DL))
        if not (len(a[0]) == len(b[0]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
            fail("surface: the search's pairs are not the oracle's")


def check_finite(env, all_obs, fail):
    """No output the fresh run (checked against the oracle above) has finite is non-finite in any history."""
    fresh = all_obs["fresh"]
    for h in HISTORIES[1:]:
        for k, v in all_obs[h].items():
            if v.dtype.kind == "f" and k in fresh and fresh[k].shape == v.shape and np.any(np.isfinite(fresh[k]) & ~np.isfinite(v)):
                fail(f"{h}: {k} has non-finite values where the fresh run is finite")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subject", required=True, choices=list(SUBJECTS))
    ap.add_argument("--dump", metavar="DIR", help="write what every history observed as DIR/<history>.npz")
    args = ap.parse_args()
    env = Env(args.subject)
    capi = env.capi
    observe = OBSERVE[env.kind]
    failures, deltas, seconds, scrubbed, all_obs = [], {}, {}, 0, {}

    def subject_run(history):
        t0 = time.time()
        before = capi.pool_stats()
        out = {}
        observe(env, env.prm, env.parts, out)
        after = capi.pool_stats()
        deltas[history] = dict(hits=after["hits"] - before["hits"], misses=after["misses"] - before["misses"])
        seconds[history] = round(time.time() - t0, 3)
        all_obs[history] = out

    subject_run("fresh")
    observe(env, env.f_prm, env.f_parts, None)                    # the foreign predecessor
    subject_run("foreign")
    scrubbed = capi.pool_scrub(3)
    subject_run("scrub3")
    observe(env, env.prm, env.n_parts, None, until_diverged=True)  # the NaN predecessor
    subject_run("nan")

    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for h, out in all_obs.items():
            np.savez(os.path.join(args.dump, h + ".npz"), **out)
    t0 = time.time()
    check_fresh(env, all_obs["fresh"], failures.append)
    check_finite(env, all_obs, failures.append)
    seconds["checks"] = round(time.time() - t0, 3)
    differing = {h: sorted(k for k in all_obs["fresh"] if k not in all_obs[h] or all_obs[h][k].tobytes() != all_obs["fresh"][k].tobytes())
                 for h in HISTORIES[1:]}
    print(json.dumps(dict(subject=args.subject, switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), n_arrays=len(all_obs["fresh"]),
                          facts=env.facts, deltas=deltas, scrubbed=int(scrubbed), pool=capi.pool_stats(), seconds=seconds,
                          differing=differing, failures=failures)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
