"""Density statistics of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the four
sphx_slab_dstats_* entry points (and no "sample now"), the engine has the four dens_part_* methods and neither dens_stats nor
dens_stats_sample, slab.pool_ring_dens_stats makes the unsplit channel's sums out of the ranks' partial sums
(profile.dens_stats_sums_part) for rings of 2, 3 and 4 windows -- integers exactly, sums within dens_stats_cases.BOUND, and a
comparison that one missing halo copy, one missing wall particle of a halo column or one seam copy a period off fails by orders
of magnitude --, summation_density(fold=False) on a window's rows is fold=True on the whole channel for the owned rows,
the pooling refuses ranks that disagree and takes MIN / MAX through +-inf, slab.all_reduce_ring_dens_stats does the same between
two gloo processes on the CPU, driver.density_figures takes the pooled list, and the sensitivity of the sums and of a
particle's delta to the state, on which the GPU tests' bounds and edge clearances rest, is measured."""
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dens_stats_cases as dc
import slab_dens_stats_cases as sc
import test_gpu_slab_samplers as rings  # the ring cases and their states: used as they are

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_dens_stats_worker.py")
SYMBOLS = ("sphx_slab_dstats_enable", "sphx_slab_dstats_disable", "sphx_slab_dstats_reset", "sphx_slab_dstats_read")


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


# 1 ---------------------------------------------------------------------------------------------------------------
def test_slab_dstats_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "sphx_slab_dstats_sample" not in declared and "sphx_slab_dstats_sample" not in capi.EXPORTS  # no "sample now" on slabs
    assert not hasattr(capi.lib(), "sphx_slab_dstats_sample")
    # the read takes a context's arguments
    ctx_read = re.search(r"int sphx_ctx_dens_stats_read\(sphx_ctx \*ctx,(.*?)\);", hdr, re.S).group(1)
    slab_read = re.search(r"int sphx_slab_dstats_read\(sphx_ctx \*ctx,(.*?)\);", hdr, re.S).group(1)
    assert " ".join(ctx_read.split()) == " ".join(slab_read.split())


def test_engine_has_the_four_part_methods_only(capi, slab):
    eng = slab.HipSlabEngine
    for name in ("dens_part_enable", "dens_part_disable", "dens_part_reset", "dens_part_sums"):
        assert callable(getattr(eng, name)), name
    for name in ("dens_stats_enable", "dens_stats", "dens_stats_sample", "dens_stats_sums", "dens_stats_reset", "dens_stats_disable",
                 "dens_part_sample"):
        assert not hasattr(eng, name), name  # means of partial sums would mislead; no "sample now"
        assert name == "dens_part_sample" or (hasattr(capi.Context, name) and hasattr(capi.Batch, name)), name
    assert (eng._stem, eng._dens) == ("sphx_slab_", "dstats_")
    assert capi.Context._dens == capi.Batch._dens == "dens_stats_"
    assert inspect.signature(eng.dens_part_enable) == inspect.signature(capi.Context.dens_stats_enable)  # the same keywords and defaults
    assert inspect.signature(eng.dens_part_sums).parameters == inspect.signature(capi.Context.dens_stats_sums).parameters


# 2 ---------------------------------------------------------------------------------------------------------------
_whole = {}


def _unsplit(cfgmod, geom, profmod):
    if "a" not in _whole:
        prm, parts = rings._case(cfgmod, geom, "a")
        _whole["a"] = sc.unsplit(profmod, prm, parts, profmod.n_profile_bins(prm.DH, prm.dp), **sc.HIST_WIDE)
    return _whole["a"]


def _integers_equal(got, whole):
    for x, y in zip(got, whole):
        for f in dc.COUNTS + ("hist",):
            assert np.array_equal(x[f], y[f]), f
        assert (x["below"], x["above"]) == (y["below"], y["above"])


@pytest.mark.parametrize("world", [2, 3, 4])
def test_pooled_parts_are_the_unsplit_channel(cfgmod, geom, profmod, slab, world):
    """Both sides are numpy and see the same rows with the same dx (a shift by DL is exact to an ulp of x): only the association
    of the sums differs, so BOUND holds.  The teeth: one first-halo-column copy dropped, one wall particle of a halo column
    dropped, one seam copy shifted by DL the wrong way -- each moves the pooled sums beyond the one-sample bound of the GPU
    comparison, by orders of magnitude."""
    prm, parts = rings._case(cfgmod, geom, "a")
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    whole = _unsplit(cfgmod, geom, profmod)
    ranks, held = sc.synthetic_ring(profmod, prm, parts, world, n_bins, **sc.HIST_WIDE)
    assert len(ranks) == world and all(len(r) == 3 for r in ranks)
    got = sc.pooled(slab, ranks)
    _integers_equal(got, whole)
    assert got[0]["count"].sum() == parts["n_fluid"] and got[1]["count"].sum() > 0 and got[2]["count"].sum() > 0
    assert sum(int(o.sum()) for _, _, o in held) == parts["n_fluid"] and all((~o).sum() > 0 for _, _, o in held)
    assert any(np.any(s != 0.0) for _, s, _ in held)  # copies from across the seam
    dev = dc.deviation(got, whole)
    print(f"world {world}: pooled parts off by {dev[0]:.3e} ({dev[1]}, band {dev[2]})")
    assert dev[0] <= dc.BOUND
    quant = [{f: np.zeros(n_bins) for f in dc.SUMMED} for _ in got]
    dc.assert_sums_match(got, whole, quant, f"world {world}: pooled parts")  # (d_min / d_max through the ranks' +-inf too)
    # a slab that owns nothing of a band bins nothing there, and says so with +-inf
    if world > 2:
        assert any(r[1]["count"].sum() == 0 and r[1]["outliers"].sum() == 0 and not np.any(r[1]["sum_d"]) and r[1]["hist"].sum() == 0
                   and np.all(r[1]["d_min"] == np.inf) and np.all(r[1]["d_max"] == -np.inf) for r in ranks)

    hi = sc.cuts(prm, world)[1]
    changed = []

    def near_the_cut(owned, p):
        """rank 0's copies in its first halo column to the right, mid-channel"""
        return np.flatnonzero(~owned & (p[:, 0] >= hi) & (p[:, 0] < hi + 2.0 * prm.h) & (np.abs(p[:, 1] - 0.5 * prm.DH) < 0.2 * prm.DH))

    def drop_a_copy(r, idx, shift, owned, p):
        if r != 0:
            return None
        cand = near_the_cut(owned, p)
        keep = np.ones(len(p), dtype=bool)
        keep[cand[np.argmin(p[cand, 0])]] = False
        changed.append("copy")
        return keep

    def drop_a_wall_particle(r, widx, wshift, wp):
        if r != 0:
            return None
        cand = np.flatnonzero((wp[:, 0] >= hi) & (wp[:, 0] < hi + 2.0 * prm.h))
        k = cand[np.argmin(np.abs(wp[cand, 1]) + (wp[cand, 0] - hi))]  # the one next to the fluid, nearest to the cut
        keep = np.ones(len(wp), dtype=bool)
        keep[k] = False
        changed.append("wall")
        return keep

    def shift_a_seam_copy(r, idx, shift, owned, p):
        if r != 0:
            return None
        cand = np.flatnonzero(~owned & (shift == -prm.DL) & (p[:, 0] >= -2.0 * prm.h) & (np.abs(p[:, 1] - 0.5 * prm.DH) < 0.2 * prm.DH))
        k = cand[np.argmax(p[cand, 0])]
        p[k, 0] += 2.0 * prm.DL  # held at x + DL where the first slab must hold it at x - DL
        changed.append("seam")
        return None

    for what, kw in (("one halo copy dropped", dict(tweak=drop_a_copy)), ("one wall particle of a halo column dropped", dict(wall_tweak=drop_a_wall_particle)),
                     ("one seam copy shifted the wrong way", dict(tweak=shift_a_seam_copy))):
        bad, _ = sc.synthetic_ring(profmod, prm, parts, world, n_bins, **kw, **sc.HIST_WIDE)
        dev_bad = dc.deviation(sc.pooled(slab, bad), whole)
        print(f"world {world}: with {what} off by {dev_bad[0]:.3e} ({dev_bad[1]}, band {dev_bad[2]}); one-sample bound {sc.BOUND_ONE_SAMPLE:.2e}")
        assert dev_bad[0] >= 100.0 * sc.BOUND_ONE_SAMPLE, what
    assert changed == ["copy", "wall", "seam"]


def test_open_window_density_is_the_folded_channels_for_the_owned_rows(cfgmod, geom, profmod):
    """summation_density(fold=False) on what a window holds against fold=True on the whole channel, row for row: the same
    partners at the same distances (a shift by DL costs an ulp of x), so the densities agree to rho's rounding error."""
    prm, parts = rings._case(cfgmod, geom, "b")  # leftward case, three windows
    pos, mass = sc.fluid_state(parts)
    w = sc.walls_of(prm, parts)
    rho, wall = sc.density(profmod, prm, parts)
    edges = sc.cuts(prm, 3)
    seen = 0
    for r in range(3):
        idx, shift, owned = sc.window_rows(pos[:, 0], edges[r], edges[r + 1], prm.DL, 8.0 * prm.h)
        p = pos[idx].copy()
        p[:, 0] += shift
        widx, wshift, _ = sc.window_rows(w["wall_pos"][:, 0], edges[r], edges[r + 1], prm.DL, 8.0 * prm.h)
        wp = w["wall_pos"][widx].copy()
        wp[:, 0] += wshift
        got_rho, got_wall = profmod.summation_density(p, mass[idx], prm.DL, prm.h, prm.rho0, prm.inv_sigma0, wall_pos=wp,
                                                      wall_vol=w["wall_vol"][widx], fold=False)
        err = float(np.max(np.abs(got_rho[owned] - rho[idx[owned]]))) / prm.rho0
        print(f"window {r}: {int(owned.sum())} owned of {len(idx)} held; open-window density off by {err:.3e} rho0")
        assert err <= 1e-13 and float(np.max(np.abs(got_wall[owned] - wall[idx[owned]]))) <= 1e-13
        # without the fold a row at the far end of the window lacks its partners beyond it: the halo rows are NOT to be binned
        assert float(np.max(np.abs(got_rho[~owned] - rho[idx[~owned]]))) / prm.rho0 > 1e-3
        seen += int(owned.sum())
    assert seen == parts["n_fluid"]
    # DL is not used: any value gives the same bytes
    a = profmod.summation_density(p, mass[idx], prm.DL, prm.h, prm.rho0, prm.inv_sigma0, fold=False)
    b = profmod.summation_density(p, mass[idx], 1e9, prm.h, prm.rho0, prm.inv_sigma0, fold=False)
    assert a[0].tobytes() == b[0].tobytes()


# 3 ---------------------------------------------------------------------------------------------------------------
def test_pool_ring_dens_stats_refuses_and_commutes(cfgmod, geom, profmod, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    ranks, _ = sc.synthetic_ring(profmod, prm, parts, 3, n_bins)
    ranks = sc.with_head(ranks)
    p = [r[0] for r in ranks]  # band 0 of the three ranks
    got = slab.pool_ring_dens_stats(p)
    assert (got["n_samples"], got["t_first"], got["t_last"]) == (1, 0.5, 0.5)  # rank 0's, NOT added
    assert sorted(got) == sorted(p[0]) and got["count"].sum() == parts["n_fluid"]
    assert got["hist"].dtype == np.int64 and got["hist"].sum() + got["below"] + got["above"] == parts["n_fluid"]
    assert np.array_equal(got["d_min"], np.min([d["d_min"] for d in p], axis=0)) and np.array_equal(got["d_max"], np.max([d["d_max"] for d in p], axis=0))
    # MIN / MAX through +-inf: the seam band, of which the middle rank owns nothing
    seam = [r[2] for r in ranks]
    assert np.all(seam[1]["d_min"] == np.inf) and np.all(seam[1]["d_max"] == -np.inf) and seam[1]["count"].sum() == 0
    both = slab.pool_ring_dens_stats(seam)
    some = both["count"] > 0
    assert some.any() and np.all(np.isfinite(both["d_min"][some])) and np.all(both["d_min"][some] <= both["d_max"][some])
    assert np.all(both["d_min"][~some] == np.inf) and np.all(both["d_max"][~some] == -np.inf)
    nothing = slab.pool_ring_dens_stats([seam[1], seam[1]])
    assert np.all(nothing["d_min"] == np.inf) and np.all(nothing["d_max"] == -np.inf) and nothing["n_samples"] == 1
    fewer = {k: (v[:-1] if isinstance(v, np.ndarray) and k != "hist" else v) for k, v in p[1].items()}
    shorter_hist = dict(p[1], hist=p[1]["hist"][:-1])
    headless = {k: v for k, v in p[1].items() if k not in ("n_samples", "t_first", "t_last")}
    for bad in (fewer, shorter_hist, dict(p[1], n_samples=2), dict(p[1], t_first=0.25), dict(p[1], t_last=0.75), headless):
        with pytest.raises(ValueError, match="rank 1"):
            slab.pool_ring_dens_stats([p[0], bad, p[2]])
    with pytest.raises(ValueError, match="rank 1"):  # a dict whose own arrays do not fit together
        slab.pool_ring_dens_stats([p[0], dict(p[1], sum_d2=p[1]["sum_d2"][:-1])])
    for missing in ("outliers", "hist", "below"):
        with pytest.raises(ValueError, match="rank 0"):
            slab.pool_ring_dens_stats([{k: v for k, v in p[0].items() if k != missing}])
    with pytest.raises(ValueError, match="at least one slab"):
        slab.pool_ring_dens_stats([])
    # two ranks swapped: the same bytes
    two, _ = sc.synthetic_ring(profmod, prm, parts, 2, n_bins)
    two = sc.with_head(two)
    dc.assert_identical(sc.pooled(slab, two), sc.pooled(slab, two[::-1]), "two ranks, swapped")
    nan = float("nan")  # before any sample every rank's times are NaN: they agree
    unsampled = [dict(d, n_samples=0, t_first=nan, t_last=nan) for d in p]
    assert slab.pool_ring_dens_stats(unsampled)["n_samples"] == 0
    for d in p:  # the parts are left as they were
        assert d["n_samples"] == 1 and d["count"].shape == (n_bins,)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_all_reduce_ring_dens_stats_in_two_gloo_processes():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29611", WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == 2, r.stdout


def test_figures_take_the_pooled_list(cfgmod, geom, profmod, driver, slab):
    prm, parts = rings._case(cfgmod, geom, "a")
    ranks, _ = sc.synthetic_ring(profmod, prm, parts, 4, profmod.n_profile_bins(prm.DH, prm.dp), **sc.HIST_WIDE)
    got = driver.density_figures(prm, sc.pooled(slab, ranks))
    want = driver.density_figures(prm, _unsplit(cfgmod, geom, profmod))
    assert np.isfinite(got["delta_rms"]) and got["delta_rms"] > 0
    for k in ("delta_rms", "delta_mean", "p_spread", "wall_bias", "packing"):
        assert abs(got[k] - want[k]) <= 1e-9 * max(abs(want[k]), 1.0), k
    assert got["delta_max"] == want["delta_max"] and got["outliers"] == want["outliers"] == 0


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SENSITIVITY_CASES)
def test_sensitivity(cfgmod, geom, profmod, name):
    """The measured figures: deviation / eps of the sums, and the largest |d delta_i| / eps over the particles, when every fluid
    position moves by uniform +-eps.  Measured: a 153 / 19, b 162 / 19, e 571 / 108 at both eps (linear), count and outliers
    unchanged; SENSITIVITY = 600, PARTICLE_SENSITIVITY = 120.  Then the condition of the one-sample comparison on the uploaded
    state: the particles within EDGE_ONE_SAMPLE of a histogram edge or of the bound stay inside LOOSE_CAP, for both histograms
    the GPU tests use."""
    prm, parts = rings._case(cfgmod, geom, name)
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    pos, _ = sc.fluid_state(parts)
    d0 = sc.density(profmod, prm, parts)
    delta0 = d0[0] / prm.rho0 - 1.0
    base = sc.unsplit(profmod, prm, parts, n_bins, dens=d0)
    print(f"{name}: delta {delta0.min():.4f} .. {delta0.max():.4f}, h {prm.h:.4f}")
    assert np.max(np.abs(delta0)) < 0.5 - 0.1 and sum(b["outliers"].sum() for b in base) == 0
    ratios, part = [], []
    for eps in sc.EPS:
        moved_pos = sc.perturbed(parts, eps)
        d1 = sc.density(profmod, prm, parts, moved_pos)
        moved = sc.unsplit(profmod, prm, parts, n_bins, pos=moved_pos, dens=d1)
        for x, y in zip(moved, base):
            for f in dc.COUNTS:
                assert np.array_equal(x[f], y[f]), (name, eps, f)
        dev = dc.deviation(moved, base)
        ratios.append(dev[0] / eps)
        part.append(float(np.max(np.abs(d1[0] - d0[0]))) / prm.rho0 / eps)
        print(f"{name}: eps {eps:g}: deviation / eps = {ratios[-1]:.1f} ({dev[1]}, band {dev[2]}); largest |d delta_i| / eps = {part[-1]:.1f}")
        assert 0.0 < ratios[-1] < sc.SENSITIVITY
        assert 0.0 < part[-1] < sc.PARTICLE_SENSITIVITY
    assert abs(ratios[0] / ratios[1] - 1.0) < 0.1 and abs(part[0] / part[1] - 1.0) < 0.1  # linear in eps
    for hist in (dict(n_hist=64, hist_range=0.05), sc.HIST_WIDE):
        whole = sc.unsplit(profmod, prm, parts, n_bins, dens=d0, **hist)
        loose = sc.loose_per_band(profmod, prm, pos, delta0, dc.bands(prm), sc.EDGE_ONE_SAMPLE, **hist)
        print(f"{name}: {hist}: particles within {sc.EDGE_ONE_SAMPLE:.1e} of an edge per band {loose} of {[int(b['count'].sum()) for b in whole]}")
        sc.assert_loose_under_cap(loose, [b["count"].sum() for b in whole], f"{name} {hist}")
