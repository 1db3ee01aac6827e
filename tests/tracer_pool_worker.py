"""Child process of tests/test_gpu_tracers.py::test_records_do_not_depend_on_recycled_memory: do the tracer records depend on
what the device-memory pool held before?

The record buffer comes from the caching pool (csrc/sphx_common.hip) as the previous owner left it, and k_tracers writes a
column only when it meets that tracer's id: a column nobody wrote would return the previous owner's bytes.  As in
tests/pool_history_worker.py (whose states, predecessors and four histories these are), the subject is observed four times in
ONE process -- as the first device work, after a foreign predecessor that leaves valid but wrong data behind (itself
recording tracers, closed with work enqueued), after capi.pool_scrub(3), and after a predecessor that ran into NaN.

The subject: a context (16 lanes) and a batch of four members in mu, every fluid row tracked, 35 steps recorded at every step
plus one ungated sample.  Prints ONE JSON line: per history a digest of every array, the pool's hits / misses around the
subject, and whether the fresh run's last record is the downloaded state.

    python tests/tracer_pool_worker.py"""
import hashlib
import json
import sys

import numpy as np

import pool_history_worker as phw

STEPS = phw.STEPS
SERIES = ("ids", "step", "t", "x", "y", "u_x", "u_y", "n_dropped", "n_missing")


def observe(env, prm, parts, out, until_diverged=False):
    capi = env.capi
    ids = np.random.default_rng(4).permutation(parts["n_fluid"])
    with capi.Context.from_parts(prm, parts, t_end=1e9, **env.kw) as ctx:
        ctx.tracers_enable(ids, every=1, capacity=STEPS + 1)
        if until_diverged:
            phw.run_until_diverged(capi, lambda: ctx.advance(1e9, max_steps=4))
        elif out is None:
            ctx.advance(1e9, max_steps=19)
            ctx.enqueue_steps(8)
        else:
            ctx.advance(1e9, max_steps=STEPS)
            ctx.tracers_sample()
            phw.put(out, "ctx", {k: v for k, v in ctx.tracers().items() if k in SERIES})
            phw.put(out, "ctx.state", ctx.download(fields=("pos", "vel")))
    prms, parts_list = env.members(prm, parts)
    with capi.Batch.from_parts(prms, parts_list, t_end=1e9, **env.kw) as b:
        b.tracers_enable(ids, every=1, capacity=STEPS + 1)
        if until_diverged:
            phw.run_until_diverged(capi, lambda: b.advance(1e9, max_steps=4))
        elif out is None:
            b.advance(1e9, max_steps=19)
            b.enqueue_steps(8)
        else:
            b.advance(1e9, max_steps=STEPS)
            b.tracers_sample()
            for m, tr in enumerate(b.tracers()):
                phw.put(out, f"batch.m{m}", {k: v for k, v in tr.items() if k in SERIES})
    return ids


def main():
    env = phw.Env("ctx16")
    capi = env.capi
    digests, deltas, failures = {}, {}, []
    scrubbed = 0
    for history in phw.HISTORIES:
        if history == "foreign":
            observe(env, env.f_prm, env.f_parts, None)
        elif history == "scrub3":
            scrubbed = capi.pool_scrub(3)
        elif history == "nan":
            observe(env, env.prm, env.n_parts, None, until_diverged=True)
        before = capi.pool_stats()
        out = {}
        ids = observe(env, env.prm, env.parts, out)
        after = capi.pool_stats()
        deltas[history] = dict(hits=after["hits"] - before["hits"], misses=after["misses"] - before["misses"])
        digests[history] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in out.items()}
        if history == "fresh":   # not four equal wrong answers: the last record is the state, the counters are clean
            rows = env.profile.tracer_rows(out["ctx.state.pos"], out["ctx.state.vel"], ids)
            for k, f in (("x", "x"), ("y", "y"), ("u_x", "u_x"), ("u_y", "u_y")):
                if not np.array_equal(out[f"ctx.{k}"][-1], rows[f]):
                    failures.append(f"fresh: the last record's {k} is not the downloaded state")
            for tag in ["ctx"] + [f"batch.m{m}" for m in range(len(phw.BATCH_MU))]:
                if out[f"{tag}.step"].tolist() != list(range(1, STEPS + 1)) + [STEPS] or int(out[f"{tag}.n_missing"]) or int(out[f"{tag}.n_dropped"]):
                    failures.append(f"fresh: {tag} steps / counters")
    differing = {h: sorted(k for k in digests["fresh"] if digests[h].get(k) != digests["fresh"][k]) for h in phw.HISTORIES[1:]}
    print(json.dumps(dict(n_arrays=len(digests["fresh"]), deltas=deltas, scrubbed=int(scrubbed), differing=differing, failures=failures)),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
