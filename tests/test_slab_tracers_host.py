"""Particle tracers of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the three entry
points, the engine has the tracers_part_* methods (and none of a context's tracers* names), slab.pool_ring_tracers takes every
column of every record from the one rank that owned it -- byte for byte, -0.0 included, whatever the order of the parts, with
columns that change owner between records and a rank that owns nothing for a while -- folds x where asked, refuses a column
without an owner or with two, a part whose columns are not as many as its n_owned and ranks that disagree about ids, step, t or
n_dropped, and slab.all_reduce_ring_tracers does the same between two and three gloo processes on the CPU."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import slab_tracers_worker as worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_tracers_worker.py")
SYMBOLS = ("sphx_slab_tracers_enable", "sphx_slab_tracers_disable", "sphx_slab_tracers_read")
FIELDS = worker.FIELDS


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


def test_slab_tracers_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "sphx_slab_tracers_sample" not in declared   # no slab sampler has a "sample now"
    assert "sphx_slab_tracers_sample" not in capi.EXPORTS and not hasattr(capi.lib(), "sphx_slab_tracers_sample")


def test_engine_has_the_tracers_part_methods_under_names_of_their_own(slab):
    eng = slab.HipSlabEngine
    for name in ("tracers_part_enable", "tracers_part_disable", "tracers_part_records"):
        assert callable(getattr(eng, name)), name
    for name in ("tracers_enable", "tracers_disable", "tracers_sample", "tracers"):  # a slab holds a PART of the ring's series
        assert not hasattr(eng, name), name
    for name in ("pool_ring_tracers", "ring_tracers", "all_reduce_ring_tracers"):
        assert callable(getattr(slab, name)), name


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_pool_ring_tracers_takes_every_column_from_its_owner(slab, world):
    parts, whole = worker.series(world)
    n, T = whole["x"].shape
    if world > 1:
        assert len(set(whole["owner"][:, 2].tolist())) == world          # a column that changes hands
        assert np.any(np.any(np.diff(whole["owner"], axis=0) != 0, axis=0))
    if world >= 3:
        assert parts[1]["n_owned"][:3].tolist() == [0, 0, 0] and np.isnan(parts[1]["x"][:3]).all() and parts[1]["n_owned"][3:].sum() > 0
    assert sum(int(p["n_owned"].sum()) for p in parts) == n * T
    got = slab.pool_ring_tracers(parts)
    assert worker.same(got, whole)
    assert got["step"].dtype == np.int64 and got["ids"].dtype == np.int32 and got["n_dropped"] == 2 and got["n_missing"] == 0
    assert got["owner"].dtype == np.int64 and got["owner"].shape == (n, T)
    assert np.signbit(got["u_y"][2, 5]) and got["u_y"][2, 5] == 0.0      # -0.0 stays -0.0: nothing is added
    assert not np.signbit(got["y"][3, 1])
    assert np.any(got["x"] < 0.0) and np.any(got["x"] >= worker.DL)      # the owners' frames
    assert worker.same(slab.pool_ring_tracers(iter(parts[::-1])), dict(whole, owner=world - 1 - whole["owner"]))
    folded = slab.pool_ring_tracers(parts, fold_DL=worker.DL)
    assert worker.same(folded, whole, fold=worker.DL)
    assert np.all(folded["x"] >= 0.0) and np.all(folded["x"] < worker.DL) and folded["x"][4, 3] == 0.0
    assert folded["x"][1, 0] == worker.DL - 0.125
    for k in ("y", "u_x", "u_y"):
        assert folded[k].tobytes() == got[k].tobytes()


def test_pool_ring_tracers_refuses_a_column_without_an_owner_or_with_two(slab):
    parts, whole = worker.series(3)
    bads = worker.bad_parts(parts[2], parts[0])
    with pytest.raises(ValueError) as ei:
        slab.pool_ring_tracers([parts[0], parts[1], bads["lost"]])
    r, k = (int(v) for v in np.argwhere(whole["owner"] == 2)[0])
    msg = str(ei.value)
    assert f"record {r} " in msg and f"step {int(whole['step'][r])}" in msg and f"id {int(whole['ids'][k])} " in msg and "ranks []" in msg
    with pytest.raises(ValueError) as ei:
        slab.pool_ring_tracers([parts[0], parts[1], bads["twice"]])
    r, k = (int(v) for v in np.argwhere(~np.isnan(parts[0]["x"]) & np.isnan(parts[2]["x"]))[0])
    msg = str(ei.value)
    assert f"record {r} " in msg and f"step {int(whole['step'][r])}" in msg and f"id {int(whole['ids'][k])} " in msg and "ranks [0, 2]" in msg
    with pytest.raises(ValueError, match="no rank"):
        slab.pool_ring_tracers(parts[:2])                                # a rank missing
    with pytest.raises(ValueError):
        slab.pool_ring_tracers([])


def test_pool_ring_tracers_refuses_a_part_that_miscounts(slab):
    parts, _ = worker.series(3)
    bads = worker.bad_parts(parts[1], parts[0])
    with pytest.raises(ValueError, match="rank 1.*n_owned"):
        slab.pool_ring_tracers([parts[0], bads["n_owned"], parts[2]])
    narrow = dict(parts[1], u_x=parts[1]["u_x"][:, :-1])
    with pytest.raises(ValueError, match="rank 1"):
        slab.pool_ring_tracers([parts[0], narrow, parts[2]])


def test_pool_ring_tracers_refuses_ranks_that_disagree(slab):
    parts, _ = worker.series(3)
    bads = worker.bad_parts(parts[1], parts[0])
    for name in ("step", "t", "dropped", "ids", "shorter"):
        with pytest.raises(ValueError, match="rank 1"):
            slab.pool_ring_tracers([parts[0], bads[name], parts[2]])


def test_pool_ring_tracers_refuses_a_part_that_lacks_a_key(slab):
    """what only the collective form used to turn into a refusal: a malformed part is a ValueError naming the rank"""
    parts, _ = worker.series(3)
    for key in ("n_dropped", "n_owned", "u_y"):
        with pytest.raises(ValueError, match="rank 1.*" + key):
            slab.pool_ring_tracers([parts[0], {k: v for k, v in parts[1].items() if k != key}, parts[2]])


def test_pool_ring_tracers_takes_more_ranks_than_a_word_has_bits(slab):
    """no cap on the world: 70 ranks, one record, every rank the owner of one column"""
    world = 70
    ids = np.arange(world, dtype=np.int32)
    x = np.arange(world, dtype=np.float64)[None, :] + 0.5
    parts = [dict({k: np.where(ids == r, x, np.nan) for k in FIELDS}, ids=ids, step=np.array([4]), t=np.array([0.5]),
                  n_owned=np.array([1]), n_dropped=0) for r in range(world)]
    got = slab.pool_ring_tracers(parts)
    assert np.array_equal(got["owner"], ids[None, :].astype(np.int64)) and np.array_equal(got["x"], x)


def test_pooled_series_goes_into_unwrap_tracers_in_either_frame(slab, profmod):
    parts, _ = worker.series(4)
    a = profmod.unwrap_tracers(slab.pool_ring_tracers(parts), worker.DL)
    b = profmod.unwrap_tracers(slab.pool_ring_tracers(parts, fold_DL=worker.DL), worker.DL)
    assert a["x_unwrapped"].shape == b["x_unwrapped"].shape == a["x"].shape
    d = a["x_unwrapped"] - b["x_unwrapped"]
    assert np.all(np.abs(d - np.round(d / worker.DL) * worker.DL) <= 1e-12)   # the same images up to the period and a rounding


@pytest.mark.parametrize("world,port", [(2, 29601), (3, 29602)])
def test_all_reduce_ring_tracers_in_gloo_processes(world, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == world, r.stdout
