"""Point probes of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the three entry
points, the engine has the probes_part_* methods (and none of a context's probes_* names), slab.pool_ring_probes puts the
ranks' columns back at their indices -- NaN exactly where the owner has it, a rank without a probe included -- and refuses
indices that do not partition the points or ranks that disagree about step, t, n_dropped or points, and
slab.all_reduce_ring_probes does the same between two and three gloo processes on the CPU."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import slab_probes_worker as worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_probes_worker.py")
SYMBOLS = ("sphx_slab_probes_enable", "sphx_slab_probes_disable", "sphx_slab_probes_read")
FIELDS = worker.FIELDS


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


def test_slab_probes_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "sphx_slab_probes_sample" not in declared   # no slab sampler has a "sample now"


def test_engine_has_the_probes_part_methods_under_names_of_their_own(slab):
    eng = slab.HipSlabEngine
    for name in ("probes_part_enable", "probes_part_disable", "probes_part_records"):
        assert callable(getattr(eng, name)), name
    for name in ("probes_enable", "probes_sample", "probes"):  # a slab holds a PART of the ring's series
        assert not hasattr(eng, name), name
    for name in ("pool_ring_probes", "ring_probes", "all_reduce_ring_probes"):
        assert callable(getattr(slab, name)), name


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_pool_ring_probes_scatters_the_columns(slab, world):
    parts, whole = worker.series(world)
    if world == 3:
        assert len(parts[1]["index"]) == 0 and parts[1]["u_x"].shape == (5, 0)   # a part with n_owned = 0
    got = slab.pool_ring_probes(parts)
    assert worker.same(got, whole)
    assert got["step"].dtype == np.int64 and got["n_dropped"] == 3
    for k in FIELDS:   # bit for bit, and NaN exactly where the owner has it
        assert got[k].tobytes() == whole[k].tobytes(), k
    assert np.isnan(got["u_x"][:, 4]).all() and 0 < np.isnan(got["u_x"]).sum() < got["u_x"].size
    assert worker.same(slab.pool_ring_probes(iter(parts[::-1])), whole)   # (the order of the parts does not matter)


def _moved(parts, whole, r, idx):
    """parts with rank r owning `idx` instead"""
    idx = np.asarray(idx, dtype=np.int64)
    out = list(parts)
    cols = np.minimum(idx, whole["rho"].shape[1] - 1)   # (an index outside range(P) still gets a column of the right shape)
    out[r] = dict(parts[r], index=idx, **{k: whole[k][:, cols] for k in FIELDS})
    return out


def test_pool_ring_probes_refuses_gaps_and_overlaps(slab):
    parts, whole = worker.series(3)
    i0, i2 = parts[0]["index"], parts[2]["index"]
    with pytest.raises(ValueError, match="no owner"):
        slab.pool_ring_probes(_moved(parts, whole, 2, i2[1:]))                        # a gap
    with pytest.raises(ValueError, match="more than one"):
        slab.pool_ring_probes(_moved(parts, whole, 2, np.sort(np.append(i2, i0[0]))))  # an overlap
    with pytest.raises(ValueError):
        slab.pool_ring_probes(_moved(parts, whole, 0, i0[::-1]))                      # not ascending
    with pytest.raises(ValueError):
        slab.pool_ring_probes(_moved(parts, whole, 0, np.append(i0[:-1], 23)))        # outside range(P)
    with pytest.raises(ValueError):
        slab.pool_ring_probes(parts[:2])                                              # a rank missing
    with pytest.raises(ValueError):
        slab.pool_ring_probes([])
    bad = list(parts)
    bad[0] = dict(parts[0], rho=parts[0]["rho"][:, :-1])                               # a field narrower than its index
    with pytest.raises(ValueError):
        slab.pool_ring_probes(bad)


def test_pool_ring_probes_refuses_ranks_that_disagree(slab):
    parts, _ = worker.series(3)
    p = parts[1]
    for bad in (dict(step=p["step"] + 1), dict(t=p["t"] * 2.0), dict(n_dropped=4), dict(points=p["points"] + 1e-9),
                dict(points=p["points"][:-1]), dict(step=p["step"][:-1], t=p["t"][:-1], **{k: p[k][:-1] for k in FIELDS})):
        with pytest.raises(ValueError, match="rank 1"):
            slab.pool_ring_probes([parts[0], dict(p, **bad), parts[2]])


def test_pool_ring_probes_refuses_a_part_that_lacks_a_key(slab):
    """what only the collective form used to turn into a refusal: a malformed part is a ValueError naming the rank"""
    parts, _ = worker.series(3)
    for key in ("n_dropped", "rho", "index"):
        with pytest.raises(ValueError, match="rank 2.*" + key):
            slab.pool_ring_probes([parts[0], parts[1], {k: v for k, v in parts[2].items() if k != key}])


@pytest.mark.parametrize("world,port", [(2, 29593), (3, 29594)])
def test_all_reduce_ring_probes_in_gloo_processes(world, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == world, r.stdout
