"""Gradient statistics of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the four
sphx_slab_gstats_* entry points (and no "sample now"), the engine has the four grads_part_* methods and neither grad_stats nor
grad_stats_enable, slab.pool_ring_grad_stats makes the unsplit channel's sums out of the ranks' partial sums
(profile.grad_stats_sums_part) for rings of 2, 3 and 4 windows -- counts exactly, sums within grad_stats_cases.BOUND, and a
comparison that one wrong halo copy fails by orders of magnitude -- and refuses ranks that disagree,
slab.all_reduce_ring_grad_stats does the same between two gloo processes on the CPU, driver.grad_figures takes the pooled list,
and the sensitivity of the sums to the state, on which the GPU tests' bounds rest, is measured."""
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import grad_stats_cases as gc
import slab_grad_stats_cases as sc
import test_gpu_slab_samplers as rings  # the ring cases and their states: used as they are

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_grad_stats_worker.py")
SYMBOLS = ("sphx_slab_gstats_enable", "sphx_slab_gstats_disable", "sphx_slab_gstats_reset", "sphx_slab_gstats_read")


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


# 1 ---------------------------------------------------------------------------------------------------------------
def test_slab_gstats_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "sphx_slab_gstats_sample" not in declared and "sphx_slab_gstats_sample" not in capi.EXPORTS  # no "sample now" on slabs
    assert not hasattr(capi.lib(), "sphx_slab_gstats_sample")
    # the read takes a context's arguments
    ctx_read = re.search(r"int sphx_ctx_grad_stats_read\(sphx_ctx \*ctx,(.*?)\);", hdr, re.S).group(1)
    slab_read = re.search(r"int sphx_slab_gstats_read\(sphx_ctx \*ctx,(.*?)\);", hdr, re.S).group(1)
    assert " ".join(ctx_read.split()) == " ".join(slab_read.split())


def test_engine_has_the_four_part_methods_only(capi, slab):
    eng = slab.HipSlabEngine
    for name in ("grads_part_enable", "grads_part_disable", "grads_part_reset", "grads_part_sums"):
        assert callable(getattr(eng, name)), name
    for name in ("grad_stats_enable", "grad_stats", "grad_stats_sample", "grad_stats_sums", "grad_stats_reset", "grad_stats_disable",
                 "grads_part_sample"):
        assert not hasattr(eng, name), name  # means of partial sums would mislead; no "sample now"
        assert name == "grads_part_sample" or (hasattr(capi.Context, name) and hasattr(capi.Batch, name)), name
    assert (eng._stem, eng._grads) == ("sphx_slab_", "gstats_")
    assert capi.Context._grads == capi.Batch._grads == "grad_stats_"
    assert inspect.signature(eng.grads_part_enable) == inspect.signature(capi.Context.grad_stats_enable)  # the same keywords and defaults
    assert inspect.signature(eng.grads_part_sums).parameters == inspect.signature(capi.Context.grad_stats_sums).parameters


# 2 ---------------------------------------------------------------------------------------------------------------
_whole = {}


def _unsplit(cfgmod, geom, profmod, with_walls):
    if with_walls not in _whole:
        prm, parts = rings._case(cfgmod, geom, "a")
        _whole[with_walls] = sc.unsplit(profmod, prm, parts, with_walls, profmod.n_profile_bins(prm.DH, prm.dp))
    return _whole[with_walls]


@pytest.mark.parametrize("with_walls", [True, False])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_pooled_parts_are_the_unsplit_channel(cfgmod, geom, profmod, slab, world, with_walls):
    """Both sides are numpy and see the same rows with the same dx (a shift by DL is exact to an ulp of x): only the association
    of the sums differs, so BOUND holds.  One first-halo-column copy with u_x off by 1e-3 U_max fails it by 100 x and more."""
    prm, parts = rings._case(cfgmod, geom, "a")
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    whole = _unsplit(cfgmod, geom, profmod, with_walls)
    ranks, held = sc.synthetic_ring(profmod, prm, parts, world, with_walls, n_bins)
    assert len(ranks) == world and all(len(r) == 3 for r in ranks)
    got = sc.pooled(slab, ranks)
    for x, y in zip(got, whole):
        for f in gc.COUNTS:
            assert np.array_equal(x[f], y[f]), f
    assert got[0]["count"].sum() == parts["n_fluid"] and got[1]["count"].sum() > 0 and got[2]["count"].sum() > 0
    assert sum(int(o.sum()) for _, _, o in held) == parts["n_fluid"] and all((~o).sum() > 0 for _, _, o in held)
    assert any(np.any(s != 0.0) for _, s, _ in held)  # copies from across the seam
    dev = gc.deviation(got, whole)
    print(f"world {world} walls {with_walls}: pooled parts off by {dev[0]:.3e} ({dev[1]}, band {dev[2]})")
    assert dev[0] <= gc.BOUND
    # a slab that owns nothing of a band bins nothing there
    if world > 2:
        assert any(r[1]["count"].sum() == 0 and r[1]["skipped"].sum() == 0 and not np.any(r[1]["sum_gxy"]) for r in ranks)

    # the teeth: rank 0's copy nearest to its right-hand cut, in its first halo column, mid-channel
    hi = sc.cuts(prm, world)[1]
    changed = []

    def tweak(r, idx, shift, owned, p, v):
        if r != 0:
            return
        cand = np.flatnonzero(~owned & (p[:, 0] >= hi) & (p[:, 0] < hi + 2.0 * prm.h) & (np.abs(p[:, 1] - 0.5 * prm.DH) < 0.2 * prm.DH))
        k = cand[np.argmin(p[cand, 0])]
        v[k, 0] += 1e-3 * sc.u_max(prm)
        changed.append(k)

    bad, _ = sc.synthetic_ring(profmod, prm, parts, world, with_walls, n_bins, tweak=tweak)
    assert len(changed) == 1
    dev_bad = gc.deviation(sc.pooled(slab, bad), whole)
    print(f"world {world} walls {with_walls}: with one wrong copy off by {dev_bad[0]:.3e} ({dev_bad[1]}, band {dev_bad[2]})")
    assert dev_bad[0] >= 100.0 * gc.BOUND


# 3 ---------------------------------------------------------------------------------------------------------------
def test_pool_ring_grad_stats_refuses_and_commutes(cfgmod, geom, profmod, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    ranks, _ = sc.synthetic_ring(profmod, prm, parts, 3, True, n_bins)
    ranks = sc.with_head(ranks)
    p = [r[0] for r in ranks]  # band 0 of the three ranks
    got = slab.pool_ring_grad_stats(p)
    assert (got["n_samples"], got["t_first"], got["t_last"]) == (1, 0.5, 0.5)  # rank 0's, NOT added
    assert sorted(got) == sorted(p[0]) and got["count"].sum() == parts["n_fluid"]
    fewer = {k: (v[:-1] if isinstance(v, np.ndarray) else v) for k, v in p[1].items()}
    headless = {k: v for k, v in p[1].items() if k not in ("n_samples", "t_first", "t_last")}
    for bad in (fewer, dict(p[1], n_samples=2), dict(p[1], t_first=0.25), dict(p[1], t_last=0.75), headless):
        with pytest.raises(ValueError, match="rank 1"):
            slab.pool_ring_grad_stats([p[0], bad, p[2]])
    with pytest.raises(ValueError, match="rank 1"):  # a dict whose own arrays do not fit together
        slab.pool_ring_grad_stats([p[0], dict(p[1], sum_gxy=p[1]["sum_gxy"][:-1])])
    with pytest.raises(ValueError, match="rank 0"):
        slab.pool_ring_grad_stats([{k: v for k, v in p[0].items() if k != "skipped"}])
    with pytest.raises(ValueError, match="at least one slab"):
        slab.pool_ring_grad_stats([])
    # two ranks swapped: the same bytes
    two, _ = sc.synthetic_ring(profmod, prm, parts, 2, True, n_bins)
    two = sc.with_head(two)
    gc.assert_identical(sc.pooled(slab, two), sc.pooled(slab, two[::-1]), "two ranks, swapped")
    nan = float("nan")  # before any sample every rank's times are NaN: they agree
    unsampled = [dict(d, n_samples=0, t_first=nan, t_last=nan) for d in p]
    assert slab.pool_ring_grad_stats(unsampled)["n_samples"] == 0
    for d in p:  # the parts are left as they were
        assert d["n_samples"] == 1 and d["count"].shape == (n_bins,)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_all_reduce_ring_grad_stats_in_two_gloo_processes():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29597", WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == 2, r.stdout


def test_figures_take_the_pooled_list(cfgmod, geom, profmod, driver, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    ranks, _ = sc.synthetic_ring(profmod, prm, parts, 4, False, profmod.n_profile_bins(prm.DH, prm.dp))
    got = driver.grad_figures(prm, sc.pooled(slab, ranks))
    want = driver.grad_figures(prm, _unsplit(cfgmod, geom, profmod, False))
    assert np.isfinite(got["L2_shear"]) and abs(got["L2_shear"] - want["L2_shear"]) <= 1e-9 and abs(got["div_rms"] - want["div_rms"]) <= 1e-9


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SENSITIVITY_CASES)
def test_sensitivity(cfgmod, geom, profmod, name):
    """The one measured figure: deviation / eps of the sums when every fluid position and velocity moves by uniform +-eps.
    Measured: a 319, b 168, e 555 at both eps (linear), counts unchanged; SENSITIVITY = 700."""
    prm, parts = rings._case(cfgmod, geom, name)
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    base = sc.unsplit(profmod, prm, parts, False, n_bins)
    det, gmax = sc.census(profmod, prm, parts, False)
    bound = profmod.grad_scales(gc.vmax_of(parts, parts), prm.h, parts["n_fluid"])["bound"]
    print(f"{name}: min det M {det.min():.4f}, max |G| {gmax.max():.2f} against the bound {bound:.0f}")
    assert det.min() > 0.05 + sc.EDGE and gmax.max() < bound - sc.EDGE and sum(b["skipped"].sum() for b in base) == 0
    ratios = []
    for eps in sc.EPS:
        moved = sc.unsplit(profmod, prm, parts, False, n_bins, state=sc.perturbed(prm, parts, eps))
        for x, y in zip(moved, base):
            for f in gc.COUNTS:
                assert np.array_equal(x[f], y[f]), (name, eps, f)
        dev = gc.deviation(moved, base)
        ratios.append(dev[0] / eps)
        print(f"{name}: eps {eps:g}: deviation / eps = {ratios[-1]:.1f} ({dev[1]}, band {dev[2]})")
        assert 0.0 < ratios[-1] < sc.SENSITIVITY
    assert abs(ratios[0] / ratios[1] - 1.0) < 0.1  # linear in eps
