"""An in-process ring after sphx_slab_group_run, two libraries compared byte for byte (manual probe):
    SPHX_LIB=tools/_exp/libsphx_<tag>.so python tools/probes/probe_slab_parity.py dump chain A.npz   # an earlier library
    python tools/probes/probe_slab_parity.py dump chain B.npz
    python tools/probes/probe_slab_parity.py compare A.npz B.npz
dump: one ring (chain | split | graph | protocol) in this process; the owned particles of all slabs by id (x, y, vx, vy, drho) and
every slab's t, dt (last and next), max |v| and step.  compare: exit status 0 and "identical" when every array has the same
bytes; else one line per array that differs, and exit status 2 when all of them agree within the ring test's tolerances
(tests/test_slab.py: rtol 1e-9, atol_scale 1e-10), 1 when one does not."""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RINGS = {  # world, DL, calls, graph_prepare after call, SPHX_SLAB_OVERLAP, engine keywords
    "chain": (2, 3.0, [27], None, None, dict()),
    "split": (3, 4.5, [23], None, "always", dict(rebuild_every=4)),
    "graph": (2, 3.0, [3, 25, 19], 0, None, dict()),
    "protocol": (2, 3.0, [7], None, None, dict(rebuild_every=1)),
}
FIELDS = ("x", "y", "vx", "vy", "drho")


def dump(ring, out):
    from helpers import make_case
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    slab = importlib.import_module("sph-poiseuille-flow_amd.slab")
    world, DL, calls, graph_after, overlap, kw = RINGS[ring]
    os.environ.pop("SPHX_SLAB_OVERLAP", None)
    if overlap:
        os.environ["SPHX_SLAB_OVERLAP"] = overlap
    prm, parts = make_case(pkg.config, pkg.geometry, dp=0.05, DL=DL, jitter=0.2, seed=11, developed=True, end_time=1e9)
    nf = parts["n_fluid"]
    engines = [slab.HipSlabEngine(prm, parts, r, world, 0, t_end=1e9, native=True, **kw) for r in range(world)]
    for k, n in enumerate(calls):
        slab.HipSlabEngine.group_run(engines, n)
        if graph_after == k:
            slab.HipSlabEngine.graph_prepare(engines)
    sts = [e.sync() for e in engines]
    snaps = [e.snapshot() for e in engines]
    for e in engines:
        e.close()
    res = {f: np.full(nf, np.nan) for f in FIELDS}
    seen = np.zeros(nf, dtype=int)
    for sn in snaps:
        o = sn["owned"]
        i = sn["id"][o]
        for f in FIELDS:
            res[f][i] = sn[f][o]
        np.add.at(seen, i, 1)
    assert np.all(seen == 1)
    for f in ("t", "dt_last", "dt_next", "vmax"):
        res[f] = np.array([st[f] for st in sts], dtype=np.float64)
    res["step"] = np.array([st["step"] for st in sts], dtype=np.int64)
    np.savez(out, **res)
    print(f"{ring}: {world} slabs, {nf} fluid particles, step {res['step'].tolist()}, t {res['t'][0]!r} -> {out}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files)
    differ = [f for f in a.files if a[f].tobytes() != b[f].tobytes()]
    nbytes = sum(a[f].nbytes for f in a.files)
    if not differ:
        print(f"identical: {len(a.files)} arrays, {nbytes} bytes")
        return 0
    within = True
    for f in differ:
        x, y = a[f].astype(np.float64), b[f].astype(np.float64)
        err = np.abs(x - y).max()
        ok = bool(np.all(np.abs(x - y) <= 1e-9 * np.abs(y) + 1e-10 * max(np.abs(y).max(), 1e-300)))
        within = within and ok
        print(f"differs: {f}: max |a - b| = {err:.3e}, {int((x != y).sum())} of {x.size} entries, within the ring test's tolerances: {ok}")
    return 2 if within else 1


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2], sys.argv[3]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
