"""Manual probe (not a test): every output of the three slot samplers, and the state, of a few short runs in one .npz -- to be
compared bit for bit between two libraries.
    SPHX_LIB=tools/_exp/libsphx_<tag>.so python tools/probes/probe_samplers_dump.py OUT_A.npz   # an earlier library (tools/build_baseline_lib.sh)
    python tools/probes/probe_samplers_dump.py OUT_B.npz
    python tools/probes/probe_samplers_dump.py --compare OUT_A.npz OUT_B.npz
Cases (tests/test_gpu_slot_samplers.py and tests/test_gpu_history.py): dp 0.025, DL 3 at 16 lanes per particle; dp 0.05, DL 3
re-binning dynamically; dp 0.025, DL 1.5 in the dual-rate loop.  Each: developed, jittered start, flow statistics (two bands),
history and field map on with every = 1, 40 steps in one advance.  --compare prints one line per array and exits 1 unless
np.array_equal holds on every one."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from helpers import make_case  # noqa: E402

PKG = "sph-poiseuille-flow_amd"
CASES = {
    "dp025_lpp16": (0.025, 3.0, dict(lanes_per_particle=16)),
    "dp05_dynamic": (0.05, 3.0, dict(dynamic_rebin=1)),
    "dp025_dual": (0.025, 1.5, dict(lanes_per_particle=16, dual_rate=2)),
}
STEPS = 40


def dump(path):
    pkg = importlib.import_module(PKG)
    capi = pkg.capi
    out = {}
    for name, (dp, DL, kw) in CASES.items():
        prm, parts = make_case(pkg.config, pkg.geometry, dp=dp, DL=DL, jitter=0.2, seed=11, developed=True)
        with capi.Context.from_parts(prm, parts, t_end=1e9, **kw) as ctx:
            ctx.flow_stats_enable(bands=((0.5 * DL, 0.1 * DL),))
            ctx.history_enable(capacity=64)
            ctx.field_map_enable()
            st = ctx.advance(1e9, max_steps=STEPS)
            assert st["step"] == STEPS, st
            for band in (0, 1):
                for k, v in ctx.flow_stats_sums(band).items():
                    out[f"{name}/stats{band}/{k}"] = np.asarray(v)
            rec, dropped = ctx.history_records()
            out[f"{name}/history/records"] = rec
            out[f"{name}/history/n_dropped"] = np.asarray(dropped)
            for k, v in ctx.field_map_sums().items():
                out[f"{name}/field/{k}"] = np.asarray(v)
            for k, v in ctx.download().items():
                out[f"{name}/state/{k}"] = v
            for k in ("t", "dt_last", "vmax"):
                out[f"{name}/status/{k}"] = np.asarray(st[k])
    np.savez(path, **out)
    print(f"{capi.LIB_PATH}: {len(out)} arrays -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files)
    for k in sorted(set(A.files) | set(B.files)):
        eq = k in A.files and k in B.files and np.array_equal(A[k], B[k])
        same = same and eq
        print(f"{'equal  ' if eq else 'DIFFERS'} {k}" + (f" {A[k].shape}" if k in A.files else ""))
    print(f"{len(A.files)} arrays in {a}, {len(B.files)} in {b}: {'all equal' if same else 'NOT equal'}")
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("paths", nargs="+")
    a = ap.parse_args()
    sys.exit(compare(*a.paths) if a.compare else dump(a.paths[0]))
