"""Pair statistics of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the four
sphx_slab_pairs_* entry points (and no "sample now"), the engine has the four pairs_part_* methods and neither pair_dist_enable
nor pair_dist, slab.pool_ring_pair_dist makes the unsplit channel's integers out of the ranks' partial sums
(profile.pair_histogram_part) for worlds 1 to 4 EXACTLY -- a state whose every r2 is exact in binary, with pairs on bin edges
across every cut and the seam -- and refuses ranks that disagree, slab.all_reduce_ring_pair_dist does the same between two gloo
processes on the CPU, and driver.pair_dist_figures takes the pooled list."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pair_dist_cases as pc
import slab_pair_dist_worker as worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_pair_dist_worker.py")
SYMBOLS = ("sphx_slab_pairs_enable", "sphx_slab_pairs_disable", "sphx_slab_pairs_reset", "sphx_slab_pairs_read")


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


def test_slab_pairs_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "sphx_slab_pairs_sample" not in declared and "sphx_slab_pairs_sample" not in capi.EXPORTS  # no "sample now" on slabs
    assert not hasattr(capi.lib(), "sphx_slab_pairs_sample")
    # the read takes a context's arguments
    ctx_read = re.search(r"int sphx_ctx_pair_dist_read\(sphx_ctx \*ctx,(.*?)\);", hdr, re.S).group(1)
    slab_read = re.search(r"int sphx_slab_pairs_read\(sphx_ctx \*ctx,(.*?)\);", hdr, re.S).group(1)
    assert " ".join(ctx_read.split()) == " ".join(slab_read.split())


def test_engine_has_the_four_part_methods_only(capi, slab):
    eng = slab.HipSlabEngine
    for name in ("pairs_part_enable", "pairs_part_disable", "pairs_part_reset", "pairs_part_sums"):
        assert callable(getattr(eng, name)), name
    for name in ("pair_dist_enable", "pair_dist", "pair_dist_sample", "pair_dist_sums", "pairs_part_sample"):
        assert not hasattr(eng, name), name  # g(r) of partial sums would mislead; no "sample now"
        assert name == "pairs_part_sample" or (hasattr(capi.Context, name) and hasattr(capi.Batch, name)), name
    assert (eng._stem, eng._pairs) == ("sphx_slab_", "pairs_")
    assert capi.Context._pairs == capi.Batch._pairs == "pair_dist_"
    import inspect
    assert inspect.signature(eng.pairs_part_enable) == inspect.signature(capi.Context.pair_dist_enable)  # the same keywords and defaults


@pytest.mark.parametrize("y_margin, with_walls", [(0.0, True), (0.125, False)])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_pool_ring_pair_dist_gives_the_unsplit_histogram_exactly(profmod, slab, world, y_margin, with_walls):
    parts, whole = worker.partial_sums(profmod, world, y_margin, with_walls)
    assert len(parts) == world and all(len(p) == 3 for p in parts)
    if world > 1:  # a slab that owns no centre of a band: zeros and +inf
        empty = [p for p in parts if p[1]["centres"] == 0]
        assert empty and all(p[1]["ff"].sum() == 0 and np.isinf(p[1]["r2_min"]) and p[0]["centres"] > 0 for p in empty)
    got = slab.pool_ring_pair_dist(parts)
    pc.assert_counts_equal(got, whole, f"world {world}")  # integers, r2_min bit for bit, r_edges
    assert sorted(got[0]) == sorted(parts[0][0])
    for d in got:  # the heads are the ranks', NOT added
        assert (d["n_samples"], d["t_first"], d["t_last"]) == (1, 0.5, 0.5)
        assert d["r_min"] == np.sqrt(d["r2_min"])
    # the state does hold what the test is about: pairs exactly on the bin edges (across the cuts and the seam), a coincident
    # pair, all bands filled, wall partners where asked for
    r2 = profmod.pair_separations(worker.channel()[0], worker.DL, worker.R_MAX)["r2_ff"]
    e2 = profmod.pair_edges(worker.R_MAX, worker.N_BINS)[1]
    if y_margin == 0.0:
        for k in (1, 2, 7, 31, 63):
            assert np.count_nonzero(r2 == e2[k]) >= 12, k  # six places, both orders
        assert got[0]["r2_min"] == 0.0
    assert all(d["centres"] > 0 and d["ff"].sum() > 0 for d in got) and got[0]["centres"] > got[1]["centres"]
    assert (got[0]["fw"].sum() > 0) == with_walls
    if world == 2:  # the order of the list does not matter for the integers
        pc.assert_counts_equal(slab.pool_ring_pair_dist(parts[::-1]), got, "two ranks, swapped", head=True)
    for p in parts:  # the parts are left as they were
        assert len(p) == 3 and p[0]["ff"].dtype == np.int64


def test_pool_ring_pair_dist_refuses_ranks_that_disagree(profmod, slab):
    parts, _ = worker.partial_sums(profmod, 3)
    p = parts[1]

    def changed(band, **kw):
        return [dict(d, **kw) if b == band else d for b, d in enumerate(p)]

    fewer_bins = [dict(d, r_edges=d["r_edges"][:-1], ff=d["ff"][:-1], fw=d["fw"][:-1]) for d in p]
    headless = [{k: v for k, v in d.items() if k not in ("n_samples", "t_first", "t_last")} for d in p]
    for bad in (changed(0, r_edges=p[0]["r_edges"] * 2.0), changed(2, r_edges=p[2]["r_edges"] + 1e-9), fewer_bins, p[:2], p + p[:1],
                changed(0, n_samples=2), changed(1, t_first=0.25), changed(2, t_last=0.75), headless):
        with pytest.raises(ValueError, match="rank 1"):
            slab.pool_ring_pair_dist([parts[0], bad, parts[2]])
    with pytest.raises(ValueError, match="at least one slab"):
        slab.pool_ring_pair_dist([])
    with pytest.raises(ValueError, match="fw"):  # a band whose own arrays do not fit together
        slab.pool_ring_pair_dist([changed(1, fw=p[1]["fw"][:-1])])
    with pytest.raises(ValueError, match="one dict per band"):
        slab.pool_ring_pair_dist([p[0]])
    nan = float("nan")  # before any sample every rank's times are NaN: they agree
    unsampled = [[dict(d, n_samples=0, t_first=nan, t_last=nan) for d in q] for q in parts]
    assert slab.pool_ring_pair_dist(unsampled)[0]["n_samples"] == 0


def test_pool_ring_pair_dist_refuses_a_slab_whose_bands_do_not_share_their_bins(profmod, slab):
    """what only the collective form used to refuse: every rank alike holds a band with fewer bins than its band 0, so the
    ranks agree with each other and each band's arrays fit its own r_edges"""
    parts, _ = worker.partial_sums(profmod, 3)

    def narrowed(p):
        return [dict(d, r_edges=d["r_edges"][:-1], ff=d["ff"][:-1], fw=d["fw"][:-1]) if b == 1 else d for b, d in enumerate(p)]

    with pytest.raises(ValueError, match="rank 0.*share the bins"):
        slab.pool_ring_pair_dist([narrowed(p) for p in parts])
    with pytest.raises(ValueError, match="rank 2.*share the bins"):
        slab.pool_ring_pair_dist([parts[0], parts[1], narrowed(parts[2])])
    with pytest.raises(ValueError, match="rank 1.*centres"):  # a band that lacks a key is a refusal too, not a KeyError
        slab.pool_ring_pair_dist([parts[0], [{k: v for k, v in d.items() if k != "centres"} for d in parts[1]], parts[2]])


def test_all_reduce_ring_pair_dist_in_two_gloo_processes():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29596", WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == 2, r.stdout


def test_figures_take_the_pooled_list(cfgmod, profmod, driver, slab):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    parts, whole = worker.partial_sums(profmod, 4)
    pooled = slab.pool_ring_pair_dist(parts)
    got, want = driver.pair_dist_figures(prm, pooled), driver.pair_dist_figures(prm, whole)
    assert set(got) == {"r_min_dp", "n_neigh", "sigma1_dp", "seam_dev"}
    for k, v in want.items():
        assert np.array_equal(got[k], v, equal_nan=True), k
    assert got["n_neigh"] == pooled[0]["ff"].sum() / pooled[0]["centres"] and np.isfinite(got["seam_dev"])
