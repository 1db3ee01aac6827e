"""Flow statistics of batches (include/sphx.h section 2c) without a GPU: the C ABI declares and exports the entry points and
refuses a NULL batch, capi.Batch checks its arguments before anything reaches the library, the pooling helper agrees
with numpy, the ensemble starts are reproducible, and driver.run_ensemble refuses bad inputs before the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sphx_batch_flow_stats_enable", "sphx_batch_flow_stats_disable", "sphx_batch_flow_stats_reset",
           "sphx_batch_flow_stats_sample", "sphx_batch_flow_stats_read")
FIELDS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2")


def test_symbols_declared_and_exported(capi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)


def test_null_batch_is_refused(capi):
    L = capi.lib()
    cfg = capi.SphxFlowStatsConfig(n_bins=0, every=1, t_from=0.0, n_bands=0)
    calls = {"sphx_batch_flow_stats_enable": (C.byref(cfg),), "sphx_batch_flow_stats_disable": (),
             "sphx_batch_flow_stats_reset": (), "sphx_batch_flow_stats_sample": (),
             "sphx_batch_flow_stats_read": (0, 0, None, *[None] * 5, None, None, None)}
    assert set(calls) == set(SYMBOLS)
    for name, args in calls.items():
        rc = getattr(L, name)(None, *args)
        assert rc == capi.SPHX_ERR_ARG, name
        assert L.sphx_last_error_id().decode() == "SPHX:Batch:null", name


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} made before the arguments were checked")


def _bare_batch(capi, monkeypatch, enabled=None, members=3):
    monkeypatch.setattr(capi, "lib", lambda: _NoLib())
    b = object.__new__(capi.Batch)
    b._h = C.c_void_p(0)
    b._flow_stats = enabled
    b.n_members = members
    b.params = [capi.SphxParams(DL=3.0, DH=1.0, dp=0.05) for _ in range(members)]
    return b


@pytest.mark.parametrize("kw", [dict(every=0), dict(every=-2), dict(every=1.5), dict(n_bins=-1), dict(n_bins=2.0),
                                dict(t_from=float("nan")), dict(t_from="soon"), dict(bands=[(1.5, 0.1)] * 3),
                                dict(bands=[(1.5,)]), dict(bands=[(1.5, -0.1)]), dict(bands=[(float("inf"), 0.1)]),
                                dict(n_bins=600, bands=[(1.5, 0.1), (0.0, 0.1)])])
def test_enable_checks_arguments_before_the_device(capi, monkeypatch, kw):
    b = _bare_batch(capi, monkeypatch)
    with pytest.raises(capi.SphxError) as e:
        b.flow_stats_enable(**kw)
    assert e.value.identifier == "SPHX:Stats:config"
    b._h = C.c_void_p()  # (nothing to destroy)


def test_read_checks_band_and_state_before_the_device(capi, monkeypatch):
    b = _bare_batch(capi, monkeypatch)
    for call in (lambda: b.flow_stats(0), lambda: b.flow_stats_sums(0), b.flow_stats_sample, b.flow_stats_reset):
        with pytest.raises(capi.SphxError) as e:
            call()
        assert e.value.identifier == "SPHX:Stats:disabled"
    b._flow_stats = (20, 2)
    for band in (-1, 2, 0.5, True):
        with pytest.raises(capi.SphxError) as e:
            b.flow_stats(band)
        assert e.value.identifier == "SPHX:Stats:band"
    b._h = C.c_void_p()


def _synthetic(rng, DH, n_bins, n, empty_top=0):
    y = rng.random(n) * DH * (1.0 - empty_top / n_bins)
    ux, uy = np.sin(3 * y) + 0.1 * rng.standard_normal(n), 0.01 * rng.standard_normal(n)
    edges = np.linspace(0.0, DH, n_bins + 1)
    k = np.minimum(np.searchsorted(edges, y, side="right") - 1, n_bins - 1)
    sums = [np.bincount(k, weights=w, minlength=n_bins).astype(np.float64) for w in (np.ones_like(ux), ux, ux * ux, uy, uy * uy)]
    return dict(zip(FIELDS, sums)), (y, ux, uy)


def test_pool_matches_numpy(profmod):
    rng = np.random.default_rng(3)
    DH, n_bins = 1.0, 24
    members = [_synthetic(rng, DH, n_bins, 4000 + 100 * m, empty_top=3 if m == 1 else 0) for m in range(4)]
    sums = [dict(s, n_samples=10 + m, t_first=1.0 + 0.1 * m, t_last=2.0 - 0.1 * m) for m, (s, _) in enumerate(members)]
    out = profmod.pool_flow_stats(DH, sums)
    y = np.concatenate([raw[0] for _, raw in members])
    ux = np.concatenate([raw[1] for _, raw in members])
    _, u_ref = profmod.compute_binned_profile_mean(y, ux, 0.0, DH, n_bins)
    np.testing.assert_allclose(out["u_mean"], u_ref, rtol=1e-12)
    total = sum(s["count"] for s in sums)
    assert np.array_equal(out["count"], total)
    assert out["n_samples"] == 10 + 11 + 12 + 13 and out["t_first"] == 1.0 and out["t_last"] == 2.0
    assert out["n_members"] == 4
    # per-member means -> standard error across members; the bins empty for member 1 give NaN
    means = np.stack([profmod.flow_stats_profile(DH, *[s[f] for f in FIELDS])["u_mean"] for s in sums])
    empty = np.any(np.isnan(means), axis=0)
    assert empty.sum() == 3 and not np.isnan(out["u_mean"][empty]).any()
    assert np.all(np.isnan(out["u_mean_se"][empty]))
    np.testing.assert_allclose(out["u_mean_se"][~empty], np.std(means[:, ~empty], axis=0, ddof=1) / 2.0, rtol=1e-12)


def test_pool_of_one_member_is_its_profile(profmod):
    rng = np.random.default_rng(5)
    s, _ = _synthetic(rng, 1.0, 20, 3000, empty_top=2)
    one = profmod.pool_flow_stats(1.0, [dict(s, n_samples=7, t_first=0.5, t_last=0.9)])
    ref = profmod.flow_stats_profile(1.0, *[s[f] for f in FIELDS], n_samples=7, t_first=0.5, t_last=0.9)
    for k in ("u_mean", "u_std", "uy_mean", "uy_std", "count"):
        assert np.array_equal(one[k], ref[k], equal_nan=True), k
    assert np.all(np.isnan(one["u_mean_se"])) and one["n_samples"] == 7
    with pytest.raises(ValueError):
        profmod.pool_flow_stats(1.0, [])


def test_perturbed_particles(cfgmod, geom):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    a, b = geom.perturbed_particles(prm, 0.01, 1), geom.perturbed_particles(prm, 0.01, 1)
    c = geom.perturbed_particles(prm, 0.01, 2)
    lat = geom.init_particles(prm)
    nf = a["n_fluid"]
    assert np.array_equal(a["pos"], b["pos"]) and not np.array_equal(a["pos"], c["pos"])
    assert np.all(a["pos"][:nf, 0] >= 0.0) and np.all(a["pos"][:nf, 0] < prm.DL)
    assert np.max(np.abs(a["pos"][:nf, 1] - lat["pos"][:nf, 1])) <= 0.01 * prm.dp
    assert np.array_equal(a["pos"][nf:], lat["pos"][nf:])  # walls untouched
    assert not np.any(a["vel"]) and not np.any(a["drho_dt"])
    wide = geom.perturbed_particles(prm, 0.6, 3)  # positions that cross the periodic seam are wrapped
    assert np.all(wide["pos"][:nf, 0] >= 0.0) and np.all(wide["pos"][:nf, 0] < prm.DL)


class _NoBatch:
    def __init__(self, *a, **k):
        raise AssertionError("a batch was created before the arguments were checked")

    @classmethod
    def from_parts(cls, *a, **k):
        cls()


def test_run_ensemble_refusals(cfgmod, geom, driver, monkeypatch):
    monkeypatch.setattr(driver.capi, "Batch", _NoBatch)
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu) for mu in (0.1, 0.2)]
    with pytest.raises(ValueError, match="at least one"):
        driver.run_ensemble([], average_from=0.0)
    with pytest.raises(ValueError, match="average_from"):
        driver.run_ensemble(prms, average_from=None)
    with pytest.raises(ValueError, match="average_from"):
        driver.run_ensemble(prms, average_from=float("nan"))
    other = cfgmod.params_from_values(dp=0.05, DL=3.0, output_interval=0.5)
    with pytest.raises(ValueError, match="output_interval"):
        driver.run_ensemble([prms[0], other], average_from=0.0)
    longer = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=prms[0].t_end + 1.0)
    with pytest.raises(ValueError, match="t_end"):
        driver.run_ensemble([prms[0], longer], average_from=0.0)
    with pytest.raises(ValueError, match="parts_list"):
        driver.run_ensemble(prms, average_from=0.0, parts_list=[geom.init_particles(prms[0])])
