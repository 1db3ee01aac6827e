"""Child process of tests/test_gpu_switches.py: SPHX_DEBUG_SWITCHES is read once per process, so every switch set runs in a
fresh one.  Steps the moving-wall variant (helpers.make_variant: moving walls, uneven mass, rho0 = 2.5; 2 880 particles) or,
with --case NAME, a regime case of tests/regime_cases.py (left_capped: the same variant mirrored, flowing to the left, with
c_f = 0.3) or a dense case of tests/dense_cases.py (A: the variant pulled towards two centres, lists of up to 69 entries and
cell columns of up to 219 particles) at the same size across its re-binnings, compares every field with the oracle at the tolerances of test_gpu_resident.py and prints ONE JSON
line: the kernel forms and the schedule the context chose, the worst error per field, and what failed.  Exit code 0: ran to the
end (whatever the comparison said).

    SPHX_DEBUG_SWITCHES=tiles_be_from_1 python tests/switch_worker.py --lpp 2 --steps 35

--dump DIR also writes what was downloaded -- the nine fields, t, dt_last, vmax, the pair count and both tau -- as .npy files, so
that two builds of the library (SPHX_LIB) can be compared byte for byte on the same case.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    sys.path.insert(0, p)

FIELDS = ("pos", "vel", "rho", "p", "drho_dt", "force", "force_prior", "Vol", "B")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lpp", type=int, default=2)
    ap.add_argument("--steps", type=int, default=35)
    ap.add_argument("--dynamic", action="store_true", help="dynamic re-binning, every 8th step")
    ap.add_argument("--dump", metavar="DIR", help="also write the downloaded fields and scalars as DIR/*.npy")
    ap.add_argument("--case", default="", help="a name of tests/regime_cases.py's or tests/dense_cases.py's CASES at its worker "
                                               "size in place of the moving-wall variant")
    args = ap.parse_args()
    import oracle
    from helpers import assert_close, make_variant
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    capi = pkg.capi
    if args.case:
        import dense_cases
        import regime_cases
        cases = dict(regime_cases.CASES, **dense_cases.CASES)
        prm, parts = cases[args.case](pkg.config, pkg.geometry, "worker")
    else:
        prm, parts = make_variant(pkg.config, pkg.geometry, dp=0.025, DL=1.5, jitter=0.25, seed=31, developed=True, rho0=2.5,
                                  transport_coeff=0.1)
    nf, nt = parts["n_fluid"], parts["n_total"]
    ref = oracle.run(prm, parts, t_end=1e9, output_interval=1e9, max_steps=args.steps, enable_sort=False)
    kw = dict(dynamic_rebin=1, rebuild_every=8) if args.dynamic else {}
    with capi.Context.from_parts(prm, parts, t_end=1e9, lanes_per_particle=args.lpp, **kw) as ctx:
        forms, sched = ctx.kernel_forms(), ctx.schedule()
        st = ctx.advance(1e9, max_steps=args.steps)
        got = ctx.download()
        tb, tt, npairs = ctx.monitor(tau=True, pairs=True)
        sched_after, pol = ctx.schedule(), ctx.grid_policy()
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        scalars = dict(t=st["t"], dt_last=st["dt_last"], vmax=st["vmax"], pairs=npairs, tau_bottom=tb, tau_top=tt)
        for k, v in list((k, got[k]) for k in FIELDS) + list(scalars.items()):
            np.save(os.path.join(args.dump, k + ".npy"), np.asarray(v))
    rs = ref["stats"]
    failures, errors = [], {}

    def check(name, fn):
        try:
            fn()
        except AssertionError as e:
            failures.append(f"{name}: {e}")

    for k in FIELDS:
        errors[k] = float(np.max(np.abs(got[k] - ref[k])) / max(np.max(np.abs(ref[k])), 1e-300))
        check(k, lambda k=k: assert_close(got[k], ref[k], rtol=1e-9, atol_scale=1e-10, name=k))
    check("tau_bottom", lambda: assert_close(tb, rs["tau_bottom"], rtol=1e-8, atol_scale=1e-9, name="tau_bottom"))
    check("tau_top", lambda: assert_close(tt, rs["tau_top"], rtol=1e-8, atol_scale=1e-9, name="tau_top"))
    if st["step"] != args.steps or rs["steps"] != args.steps:
        failures.append(f"steps {st['step']} / {rs['steps']}")
    if abs(st["t"] - rs["t"]) > 1e-13 * rs["t"]:
        failures.append(f"t {st['t']!r} vs {rs['t']!r}")
    if abs(st["dt_last"] - rs["dt_last"]) > 1e-12 * rs["dt_last"]:
        failures.append(f"dt {st['dt_last']!r} vs {rs['dt_last']!r}")
    if abs(st["vmax"] - rs["vmax"]) > 1e-9 * rs["vmax"]:
        failures.append(f"vmax {st['vmax']!r} vs {rs['vmax']!r}")
    if npairs != rs["n_pairs_last"]:
        failures.append(f"pairs {npairs} vs {rs['n_pairs_last']}")
    nf_x = got["pos"][:nf, 0]
    if not (np.all(nf_x >= 0.0) and np.all(nf_x <= prm.DL)):
        failures.append(f"x outside [0, DL]: {float(nf_x.min())!r} .. {float(nf_x.max())!r}")
    print(json.dumps(dict(switches=os.environ.get("SPHX_DEBUG_SWITCHES", ""), lpp=args.lpp, case=args.case, n_total=nt, steps=int(st["step"]),
                          forms=forms, schedule=sched, rebins=int(sched_after["rebins"] - sched["rebins"]),
                          forced_rebuilds=int(pol["forced_rebuilds"]), errors=errors, failures=failures)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
