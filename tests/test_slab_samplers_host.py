"""Samplers of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the seven entry points, the
engine has a context's argument checks, slab.pool_ring_sums / pool_ring_history make the unsplit channel's sums out of the
ranks' partial sums and refuse ranks that disagree, and slab.all_reduce_ring_sums / _history do the same between two and three
gloo processes on the CPU -- three, so that the order of the float sums shows."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import slab_samplers_worker as worker
from helpers import HISTORY_FIELDS, STATS_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_samplers_worker.py")
SYMBOLS = ("sphx_slab_flow_stats_enable", "sphx_slab_flow_stats_disable", "sphx_slab_flow_stats_reset", "sphx_slab_flow_stats_read",
           "sphx_slab_history_enable", "sphx_slab_history_disable", "sphx_slab_history_read")


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


def test_slab_sampler_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert "3a. Samplers of a slab ring" in raw
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)


def test_engine_binds_a_contexts_methods_and_checks(capi, slab):
    eng = slab.HipSlabEngine
    for name in ("flow_stats_enable", "flow_stats_disable", "flow_stats_reset", "flow_stats_sums", "history_enable",
                 "history_disable", "history_records"):
        assert getattr(eng, name) is getattr(capi.Context, name), name  # one binding: the same argument checks
    for name in ("flow_stats_sample", "field_map_enable", "field_map_sums"):  # out of scope on slabs
        assert not hasattr(eng, name), name
    assert eng._stem == "sphx_slab_"


def _binned(x, y, ux, uy, DH, n_bins):
    edges = np.linspace(0.0, DH, n_bins + 1)
    inside = (y >= edges[0]) & (y <= edges[-1])
    k = np.minimum(np.searchsorted(edges, y[inside], side="right") - 1, n_bins - 1)
    ux, uy = ux[inside], uy[inside]
    return dict(zip(STATS_FIELDS, [np.bincount(k, weights=w, minlength=n_bins).astype(np.float64)
                                   for w in (np.ones_like(ux), ux, ux * ux, uy, uy * uy)]))


def _three_ranks(seed=3, n=5000, DL=3.0, DH=1.0, n_bins=20):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0.0, DL, n), rng.uniform(-0.02, DH + 0.02, n)  # (some outside [0, DH]: dropped by every rank alike)
    ux, uy = rng.normal(1.0, 0.3, n), rng.normal(0.0, 0.1, n)
    cuts = np.sort(rng.uniform(0.0, DL, 2))
    rank = np.searchsorted(cuts, x)
    head = dict(n_samples=1, t_first=0.25, t_last=0.25)
    parts = [dict(_binned(x[rank == r], y[rank == r], ux[rank == r], uy[rank == r], DH, n_bins), **head) for r in range(3)]
    whole = dict(_binned(x, y, ux, uy, DH, n_bins), **head)
    assert all(p["count"].sum() > 0 for p in parts)
    return parts, whole


def test_pool_ring_sums_gives_the_unsplit_binning(slab):
    parts, whole = _three_ranks()
    got = slab.pool_ring_sums(parts)
    assert np.array_equal(got["count"], whole["count"])
    scale = max(float(np.max(np.abs(whole[f]))) for f in STATS_FIELDS[1:])
    for f in STATS_FIELDS[1:]:
        assert np.max(np.abs(got[f] - whole[f])) <= 1e-13 * scale, f
    assert (got["n_samples"], got["t_first"], got["t_last"]) == (1, 0.25, 0.25)
    # no sample yet: NaN times on every rank agree
    nan = float("nan")
    empty = [dict(p, n_samples=0, t_first=nan, t_last=nan) for p in parts]
    assert slab.pool_ring_sums(empty)["n_samples"] == 0


@pytest.mark.parametrize("key,value", [("n_samples", 2), ("t_first", 0.125), ("t_last", 0.5)])
def test_pool_ring_sums_refuses_ranks_that_disagree(slab, key, value):
    parts, _ = _three_ranks()
    parts[1] = dict(parts[1], **{key: value})
    with pytest.raises(ValueError, match="rank 1"):
        slab.pool_ring_sums(parts)


def _ring_records(n=6, ranks=3, seed=5):
    rng = np.random.default_rng(seed)
    clock = np.column_stack([np.arange(10, 10 + n), np.linspace(0.1, 0.2, n), np.full(n, 0.02), rng.uniform(1, 2, n)])
    recs = [(np.hstack([clock, rng.normal(size=(n, 4))]), 0) for _ in range(ranks)]
    return clock, recs


def test_pool_ring_history_keeps_the_clock_and_sums_the_partials(capi, slab):
    clock, recs = _ring_records()
    got = slab.pool_ring_history(recs)
    assert tuple(k for k in got if k != "n_dropped") == HISTORY_FIELDS and got["n_dropped"] == 0
    assert got["step"].dtype == np.int64
    for j, k in enumerate(HISTORY_FIELDS):
        if j < 4:
            assert np.array_equal(got[k], clock[:, j]), k
        else:
            want = recs[0][0][:, j] + recs[1][0][:, j] + recs[2][0][:, j]
            assert np.max(np.abs(got[k] - want)) <= 1e-15 * np.max(np.abs(want)), k
    empty = slab.pool_ring_history([(np.zeros((0, 8)), 0)] * 2)
    assert len(empty["step"]) == 0


def test_pool_ring_history_refuses_ranks_that_disagree(slab):
    _, recs = _ring_records()
    other = recs[2][0].copy()
    other[3, 0] += 1
    with pytest.raises(ValueError, match="rank 2"):
        slab.pool_ring_history(recs[:2] + [(other, 0)])
    with pytest.raises(ValueError, match="rank 1"):
        slab.pool_ring_history([recs[0], (recs[1][0][:-1], 0)])


def test_pool_ring_sums_refuses_a_rank_with_other_bins(slab):
    parts, _ = _three_ranks()
    parts[1] = dict(parts[1], **{f: parts[1][f][:-1] for f in STATS_FIELDS})
    with pytest.raises(ValueError, match="rank 1"):
        slab.pool_ring_sums(parts)
    with pytest.raises(ValueError, match="at least one slab"):
        slab.pool_ring_sums([])


def _gloo_workers(world, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == world, r.stdout


def test_all_reduce_ring_sums_and_history_in_two_gloo_processes():
    _gloo_workers(2, 29597)


def test_all_reduce_ring_sums_and_history_add_in_rank_order_in_three_gloo_processes(slab):
    """Two terms cannot tell a summation order; these three can: (a + b) + c != a + (b + c) in the worker's parts, and what every
    rank gets must be pool_ring_sums / pool_ring_history of the parts, which add one rank after the other."""
    sums, recs = worker.ring_parts(3)
    assert len(sums[0]["count"]) <= 48 and len(recs[0][0]) < 10
    for f in STATS_FIELDS[1:]:
        a, b, c = (s[f] for s in sums)
        assert np.any((a + b) + c != a + (b + c)), f
        assert np.array_equal(slab.pool_ring_sums(sums)[f], (a + b) + c), f
    a, b, c = (r[0][:, worker.ADDITIVE:] for r in recs)
    assert np.any((a + b) + c != a + (b + c))
    pooled = slab.pool_ring_history(recs)
    for j, k in enumerate(HISTORY_FIELDS[worker.ADDITIVE:]):
        assert np.array_equal(pooled[k], ((a + b) + c)[:, j]), k
    _gloo_workers(3, 29595)
