"""Flow statistics (include/sphx.h section 2a) without a GPU: the C ABI declares and exports the new entry points, the
sums -> profile helper agrees with numpy (empty bins, pooled spread), the Python binding checks its arguments before
anything reaches the library, and the averaging switch of the driver refuses the MEX engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_SYMBOLS = ("sphx_ctx_flow_stats_enable", "sphx_ctx_flow_stats_disable", "sphx_ctx_flow_stats_reset",
                 "sphx_ctx_flow_stats_sample", "sphx_ctx_flow_stats_read")


def test_flow_stats_symbols_declared_and_exported(capi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert "sphx_flow_stats_config" in hdr
    for name in STATS_SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)


def test_config_struct_matches_the_header(capi):
    # int32 n_bins, int32 every, double t_from, int32 n_bands, double band_x[2], band_hw[2]
    assert C.sizeof(capi.SphxFlowStatsConfig) == 56
    assert capi.SphxFlowStatsConfig.t_from.offset == 8 and capi.SphxFlowStatsConfig.band_x.offset == 24


def _numpy_sums(y, ux, uy, DH, n_bins):
    edges = np.linspace(0.0, DH, n_bins + 1)
    inside = (y >= 0.0) & (y <= DH)
    k = np.minimum(np.searchsorted(edges, y[inside], side="right") - 1, n_bins - 1)
    ux, uy = ux[inside], uy[inside]
    return [np.bincount(k, weights=w, minlength=n_bins).astype(np.float64)
            for w in (np.ones_like(ux), ux, ux * ux, uy, uy * uy)]


def test_profile_helper_matches_numpy(profmod):
    rng = np.random.default_rng(7)
    DH, n_bins = 1.0, 24
    y = rng.random(5000) * 0.8 * DH       # the top bins stay empty
    y[:3] = [-1e-9, DH + 1e-9, 0.0]
    ux, uy = np.sin(3 * y) + 0.1 * rng.standard_normal(5000), 0.01 * rng.standard_normal(5000)
    sums = _numpy_sums(y, ux, uy, DH, n_bins)
    out = profmod.flow_stats_profile(DH, *sums, n_samples=3, t_first=0.5, t_last=1.5)
    y_mid, u_ref = profmod.compute_binned_profile_mean(y, ux, 0.0, DH, n_bins)
    assert np.array_equal(out["y_mid"], y_mid)
    empty = sums[0] == 0
    assert empty.any() and not empty.all()
    assert np.all(np.isnan(out["u_mean"][empty])) and np.all(np.isnan(out["u_std"][empty]))
    assert np.all(np.isnan(out["uy_mean"][empty])) and np.all(np.isnan(out["uy_std"][empty]))
    np.testing.assert_allclose(out["u_mean"][~empty], u_ref[~empty], rtol=1e-12)
    edges = np.linspace(0.0, DH, n_bins + 1)
    for k in np.flatnonzero(~empty):
        sel = (y >= edges[k]) & ((y < edges[k + 1]) | ((k == n_bins - 1) & (y <= DH)))
        np.testing.assert_allclose(out["u_std"][k], np.std(ux[sel]), rtol=1e-8, atol=1e-12)   # pooled: ddof 0
        np.testing.assert_allclose(out["uy_std"][k], np.std(uy[sel]), rtol=1e-6, atol=1e-12)
    assert out["n_samples"] == 3 and out["t_first"] == 0.5 and out["t_last"] == 1.5
    assert np.array_equal(out["count"], sums[0])


def test_profile_helper_clamps_negative_variance(profmod):
    # a bin whose sum of squares rounds below N mean^2 gives a spread of 0, not NaN
    out = profmod.flow_stats_profile(1.0, [3.0] + [0.0] * 19, [0.3] + [0.0] * 19, [0.0299] + [0.0] * 19,
                                     [0.0] * 20, [0.0] * 20)
    assert out["u_std"][0] == 0.0 and out["u_mean"][0] == pytest.approx(0.1)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} made before the arguments were checked")


def _bare_context(capi, monkeypatch, enabled=None):
    monkeypatch.setattr(capi, "lib", lambda: _NoLib())
    ctx = object.__new__(capi.Context)
    ctx._h = C.c_void_p(0)
    ctx._flow_stats = enabled
    ctx.params = capi.SphxParams(DL=3.0, DH=1.0, dp=0.05)
    return ctx


@pytest.mark.parametrize("kw", [dict(every=0), dict(every=-2), dict(every=1.5), dict(n_bins=-1), dict(n_bins=2.0),
                                dict(t_from=float("nan")), dict(t_from="soon"), dict(bands=[(1.5, 0.1)] * 3),
                                dict(bands=[(1.5,)]), dict(bands=[(1.5, -0.1)]), dict(bands=[(float("inf"), 0.1)]),
                                dict(n_bins=600, bands=[(1.5, 0.1), (0.0, 0.1)])])
def test_enable_checks_arguments_before_the_device(capi, monkeypatch, kw):
    ctx = _bare_context(capi, monkeypatch)
    with pytest.raises(capi.SphxError) as e:
        ctx.flow_stats_enable(**kw)
    assert e.value.identifier == "SPHX:Stats:config"
    ctx._h = C.c_void_p()  # (nothing to destroy)


def test_read_checks_band_and_state_before_the_device(capi, monkeypatch):
    ctx = _bare_context(capi, monkeypatch)
    for call in (lambda: ctx.flow_stats(0), ctx.flow_stats_sample, ctx.flow_stats_reset):
        with pytest.raises(capi.SphxError) as e:
            call()
        assert e.value.identifier == "SPHX:Stats:disabled"
    ctx._flow_stats = (20, 2)
    for band in (-1, 2, 0.5, True):
        with pytest.raises(capi.SphxError) as e:
            ctx.flow_stats(band)
        assert e.value.identifier == "SPHX:Stats:band"


def test_driver_average_needs_the_resident_engine(driver, cfgmod):
    prm = cfgmod.params_from_values(dp=0.1, DL=1.0, end_time=0.01, output_interval=0.01)
    with pytest.raises(ValueError, match="resident"):
        driver.run(prm, engine="mex", average_from=0.0)


def test_time_average_figures(driver, profmod, cfgmod):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    n_bins = 20
    y = np.linspace(0.0, prm.DH, n_bins + 1)
    y_mid = 0.5 * (y[:-1] + y[1:])
    u = prm.gravity_g / (2 * prm.nu) * y_mid * (prm.DH - y_mid)
    N = np.full(n_bins, 10.0)
    whole = profmod.flow_stats_profile(prm.DH, N, N * u, N * (u * u + 0.04), np.zeros(n_bins), N * 0.09, 5, 1.0, 2.0)
    ta = driver.time_average(prm, whole, whole)
    u_max = prm.gravity_g * prm.DH ** 2 / (8 * prm.nu)
    assert ta["L2"] < 1e-12
    assert ta["uy_rms_over_umax"] == pytest.approx(0.3 / u_max, rel=1e-12)
    assert ta["ux_std_centre_over_umax"] == pytest.approx(0.2 / u_max, rel=1e-6)
    assert ta["n_samples"] == 5 and (ta["t_first"], ta["t_last"]) == (1.0, 2.0)


def test_time_average_figures_of_a_mirrored_flow(driver, profmod, cfgmod):
    """A leftward flow (U_bulk < 0: g, u_x and U_max negative) is the mirror image of a rightward one: L2 and the rms and
    spread figures, which are magnitudes over |U_max|, are the same and not negative; U_max flips its sign."""
    n_bins = 20
    rng = np.random.default_rng(11)
    N = rng.integers(5, 30, n_bins).astype(np.float64)
    noise, uy2 = 0.02 * rng.standard_normal(n_bins), 0.09 * (1 + rng.random(n_bins))
    out = {}
    for sign in (1, -1):
        prm = cfgmod.params_from_values(dp=0.05, DL=3.0, U_bulk=sign * 0.666667)
        y = np.linspace(0.0, prm.DH, n_bins + 1)
        y_mid = 0.5 * (y[:-1] + y[1:])
        u = prm.gravity_g / (2 * prm.nu) * y_mid * (prm.DH - y_mid) + sign * noise
        whole = profmod.flow_stats_profile(prm.DH, N, N * u, N * (u * u + 0.04), np.zeros(n_bins), N * uy2, 5, 1.0, 2.0)
        out[sign] = driver.time_average(prm, whole, whole)
    a, b = out[1], out[-1]
    assert a["U_max"] > 0 and b["U_max"] == -a["U_max"]
    assert np.array_equal(b["u_exact"], -a["u_exact"])
    for k in ("L2", "uy_rms_over_umax", "ux_std_centre_over_umax"):
        assert a[k] > 0 and b[k] >= 0, (k, a[k], b[k])
        assert abs(a[k] - b[k]) <= 1e-12 * a[k], (k, a[k], b[k])
