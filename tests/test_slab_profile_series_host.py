"""Profile series of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the three
sphx_slab_pseries_* entry points (and no "sample now"), the engine binds a context's three methods and neither
profile_series_sample nor profile_series, slab.pool_ring_profile_series makes the unsplit channel's series out of the ranks'
partial series for worlds 1 to 4 and refuses ranks that disagree, slab.all_reduce_ring_profile_series does the same between
two gloo processes on the CPU, and driver.profile_series_figures takes the profiles of a pooled series."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import profile_series_cases as sc
import slab_profile_series_worker as worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_profile_series_worker.py")
SYMBOLS = ("sphx_slab_pseries_enable", "sphx_slab_pseries_disable", "sphx_slab_pseries_read")


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


def test_slab_pseries_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "sphx_slab_pseries_sample" not in declared and "sphx_slab_pseries_sample" not in capi.EXPORTS  # no "sample now" on slabs
    assert not hasattr(capi.lib(), "sphx_slab_pseries_sample")


def test_engine_binds_a_contexts_three_methods(capi, slab):
    eng = slab.HipSlabEngine
    for name in ("profile_series_enable", "profile_series_disable", "profile_series_sums"):
        assert getattr(eng, name) is getattr(capi.Context, name), name  # one binding: the same argument checks
        assert getattr(eng, name) is getattr(capi.Batch, name), name
    for name in ("profile_series_sample", "profile_series"):  # means of partial sums would mislead
        assert not hasattr(eng, name), name
        assert hasattr(capi.Context, name) and hasattr(capi.Batch, name), name
    assert (eng._stem, eng._series) == ("sphx_slab_", "pseries_")
    assert capi.Context._series == capi.Batch._series == "profile_series_"


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_pool_ring_profile_series_gives_the_unsplit_binning(slab, world):
    parts, whole, cuts = worker.partial_series(world)
    assert len(parts) == world and all(p["count"].shape == (4, 3, worker.N_BINS) for p in parts)
    assert whole["count"][:, 1].sum() > 0 and whole["count"][:, 0].sum() < 4 * 4000  # (band 1 is filled; some y outside [0, DH])
    if world > 1:  # a slab that owns nothing in a band holds that band's zeros
        assert any(p["count"][:, 1].sum() == 0 and p["count"][:, 0].sum() > 0 for p in parts)
    got = slab.pool_ring_profile_series(parts)
    assert got["step"].dtype == np.int64 and np.array_equal(got["step"], whole["step"]) and np.array_equal(got["t"], whole["t"])
    assert np.array_equal(got["y_mid"], whole["y_mid"]) and got["n_dropped"] == 0
    assert set(got) == set(whole)
    for r in range(4):
        for b in range(3):  # counts exactly, sums within 1e-12 of the band's largest |sum|
            sc.assert_record_matches(got, r, b, {f: whole[f][r, b] for f in sc.FIELDS}, f"world {world} record {r} band {b}")
    if world == 2:  # the order of the list does not matter for two ranks
        sc.assert_series_identical(slab.pool_ring_profile_series(parts[::-1]), got, "two ranks, swapped")
    for p in parts:  # the parts are left as they were
        assert p["count"].shape == (4, 3, worker.N_BINS)
    empty = slab.pool_ring_profile_series([{k: (v[:0] if k in sc.SERIES else v) for k, v in p.items()} for p in parts])
    assert empty["count"].shape == (0, 3, worker.N_BINS) and len(empty["step"]) == 0


def test_pool_ring_profile_series_refuses_ranks_that_disagree(slab):
    parts, _, _ = worker.partial_series(3)
    p = parts[1]
    fewer = {k: p[k][:-1] for k in sc.SERIES}
    other_bins = dict({k: p[k][:, :, :-1] for k in sc.FIELDS}, y_mid=p["y_mid"][:-1])
    other_bands = {k: p[k][:, :2] for k in sc.FIELDS}
    for bad in (dict(step=p["step"] + np.array([0, 1, 0, 0])), dict(t=p["t"] * 2.0), dict(n_dropped=4), dict(y_mid=p["y_mid"] + 1e-9),
                fewer, other_bins, other_bands):
        with pytest.raises(ValueError, match="rank 1"):
            slab.pool_ring_profile_series([parts[0], dict(p, **bad), parts[2]])
    with pytest.raises(ValueError, match="at least one slab"):
        slab.pool_ring_profile_series([])
    with pytest.raises(ValueError, match="sum_uy"):  # a series whose own fields do not fit together
        slab.pool_ring_profile_series([dict(p, sum_uy=p["sum_uy"][:-1])])


def test_pool_ring_profile_series_refuses_a_series_that_lacks_a_key(slab):
    """what only the collective form used to turn into a refusal: a malformed series is a ValueError naming the rank"""
    parts, _, _ = worker.partial_series(3)
    for key in ("n_dropped", "sum_ux2", "y_mid"):
        with pytest.raises(ValueError, match="rank 1.*" + key):
            slab.pool_ring_profile_series([parts[0], {k: v for k, v in parts[1].items() if k != key}, parts[2]])


def test_all_reduce_ring_profile_series_in_two_gloo_processes():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29599", WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == 2, r.stdout


def test_figures_take_the_profiles_of_a_pooled_series(cfgmod, profmod, driver, slab):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    tau = prm.DH ** 2 / (np.pi ** 2 * prm.nu)
    times = np.linspace(0.0, 4.0 * tau, 41)[1:]
    syn = sc.synthetic_series(profmod, prm, times)  # u_mean IS the start-up solution, 10 particles per bin, two bands
    raw = dict(step=syn["step"], t=syn["t"], y_mid=syn["y_mid"], n_dropped=0, count=syn["count"],
               sum_ux=syn["u_mean"] * syn["count"], sum_ux2=syn["u_mean"] ** 2 * syn["count"],
               sum_uy=np.zeros_like(syn["count"]), sum_uy2=np.zeros_like(syn["count"]))
    halves = [dict(raw, **{f: 0.5 * raw[f] for f in sc.FIELDS}) for _ in range(2)]  # (halving and adding back is exact)
    pooled = slab.pool_ring_profile_series(halves)
    sc.assert_series_identical(pooled, raw, "two halves")
    prof = profmod.profile_series_profiles(prm.DH, pooled)
    for band in (0, 1):
        got = driver.profile_series_figures(prm, prof, band=band)
        want = driver.profile_series_figures(prm, profmod.profile_series_profiles(prm.DH, raw), band=band)
        for k, v in want.items():
            assert np.array_equal(got[k], v, equal_nan=True), k
        assert np.max(got["L2_startup"]) <= 1e-14  # (sum / count gives u_mean back to a rounding)
        assert abs(got["tau_fit"] / tau - 1.0) <= 0.01
        direct = driver.profile_series_figures(prm, syn, band=band)
        assert np.max(np.abs(got["L2_steady"] - direct["L2_steady"])) <= 1e-14
