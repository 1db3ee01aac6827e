"""Profile series (include/sphx.h sections 2j / 2k) without a GPU: the library exports the eight entry points and the ctypes
struct has the header's layout, the binding checks its arguments first, profile.poiseuille_startup is the start-up solution
(zero at t = 0, the parabola at late times, a solution of u_t = g + nu u_yy, symmetric, odd in g),
driver.profile_series_figures gives the known answers on a series built from that solution, and the drained chunks of a run
are put together in order, with a lost record or a change of shape refused."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import profile_series_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = tuple(f"sphx_{who}_profile_series_{what}" for who in ("ctx", "batch") for what in ("enable", "disable", "sample", "read"))


# 1 ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert len(SYMBOLS) == 8
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert not any("slab" in n and "profile_series" in n for n in declared)  # slab rings are out of scope
    assert re.search(r"^#define SPHX_PROFILE_SERIES_FIELDS 5\s*$", hdr, re.M)
    assert capi.STATS_FIELDS == sc.FIELDS


def test_config_struct_matches_the_header(capi):
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_profile_series_config \{(.*?)\} sphx_profile_series_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for t, names in re.findall(r"(int32_t|double)\s*([\w\s,\[\]]+);", body):
        members += [(t, n.strip()) for n in names.split(",")]
    assert members == [("int32_t", "n_bins"), ("int32_t", "every"), ("int32_t", "capacity"), ("double", "t_from"),
                       ("int32_t", "n_bands"), ("double", "band_x[2]"), ("double", "band_hw[2]")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    want = [(n.split("[")[0], ctype[t] * 2 if "[" in n else ctype[t]) for t, n in members]
    assert want == list(capi.SphxProfileSeriesConfig._fields_)
    S = capi.SphxProfileSeriesConfig
    assert (C.sizeof(S), S.capacity.offset, S.t_from.offset, S.n_bands.offset, S.band_x.offset, S.band_hw.offset) == (64, 8, 16, 24, 32, 48)


@pytest.mark.parametrize("kw", [dict(n_bins=-1), dict(n_bins=2.5), dict(every=0), dict(every=1.5), dict(capacity=0), dict(capacity=-3),
                                dict(capacity=2.0), dict(t_from=float("nan")), dict(t_from="soon"), dict(bands=[(1.5, 0.1)] * 3),
                                dict(bands=[(1.5,)]), dict(bands=[(float("inf"), 0.1)]), dict(bands=[(1.5, -0.1)]),
                                dict(n_bins=769, bands=[(1.5, 0.1)]), dict(n_bins=1537),
                                dict(capacity=(1 << 27) // 100 + 1),              # 20 bins x 1 band x 5 = 100 doubles a record
                                dict(capacity=(1 << 27) // 300 + 1, n_members=3)])
def test_binding_checks_the_config_first(capi, cfgmod, kw):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    assert prm.DH == 1.0
    with pytest.raises(capi.SphxError) as e:
        capi.profile_series_config(prm, **kw)
    assert e.value.identifier == "SPHX:ProfileSeries:config" and e.value.code == capi.SPHX_ERR_ARG


def test_binding_accepts_the_limits(capi, cfgmod):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    cfg = capi.profile_series_config(prm)
    assert (cfg.n_bins, cfg.every, cfg.capacity, cfg.t_from, cfg.n_bands) == (0, 1, 4096, 0.0, 0)
    cfg = capi.profile_series_config(prm, n_bins=512, every=7, capacity=(1 << 27) // (3 * 512 * 5), t_from=-1.0,
                                     bands=[(1.5, 0.1), (0.0, 0.2)])
    assert (cfg.n_bins, cfg.n_bands, list(cfg.band_x), list(cfg.band_hw)) == (512, 2, [1.5, 0.0], [0.1, 0.2])


# 2 ---------------------------------------------------------------------------------------------------------------
G, NU, DH = 0.8, 0.1, 1.0
U_MAX = G * DH * DH / (8.0 * NU)
TAU = DH * DH / (math.pi ** 2 * NU)
Y20 = (np.arange(20) + 0.5) / 20.0 * DH


def test_startup_is_zero_at_t0(profmod):
    # (with 200 terms the truncated tail is a sum of n^-3 beyond n = 400, about 3e-6 of the sum: 1e-6 of U_max holds with room)
    u = profmod.poiseuille_startup(Y20, np.array([0.0]), G, NU, DH)
    assert u.shape == (20, 1)
    assert np.max(np.abs(u)) <= 1e-6 * U_MAX


def test_startup_reaches_the_parabola(profmod):
    u = profmod.poiseuille_startup(Y20, np.array([50.0 * TAU]), G, NU, DH)[:, 0]
    assert np.max(np.abs(u - G / (2.0 * NU) * Y20 * (DH - Y20))) <= 1e-14


def test_startup_solves_the_equation(profmod):
    y, t, d = 0.3, 0.4, 1e-4
    f = lambda yy, tt: float(profmod.poiseuille_startup(yy, tt, G, NU, DH))
    u_t = (f(y, t + d) - f(y, t - d)) / (2.0 * d)
    u_yy = (f(y + d, t) - 2.0 * f(y, t) + f(y - d, t)) / (d * d)
    assert abs(u_t - (G + NU * u_yy)) <= 1e-6


def test_startup_symmetric_and_odd_in_g(profmod):
    t = np.array([0.0, 0.1, 0.5, 2.0])
    u = profmod.poiseuille_startup(Y20, t, G, NU, DH)
    assert u.shape == (20, 4)
    assert np.max(np.abs(u - u[::-1])) <= 1e-14 * U_MAX
    assert np.array_equal(profmod.poiseuille_startup(Y20, t, -G, NU, DH), -u)
    assert np.all(np.diff(u, axis=1) > 0)  # (it only ever speeds up)


# 3 ---------------------------------------------------------------------------------------------------------------
def _prm(cfgmod):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0)
    assert prm.DH == 1.0 and prm.nu > 0 and prm.gravity_g != 0
    return prm


def test_figures_on_the_startup_solution_itself(cfgmod, profmod, driver):
    prm = _prm(cfgmod)
    tau = prm.DH ** 2 / (math.pi ** 2 * prm.nu)
    times = np.linspace(0.0, 8.0 * tau, 161)[1:]
    series = sc.synthetic_series(profmod, prm, times)
    tol = 0.02
    fig = driver.profile_series_figures(prm, series, band=1, tol=tol)
    assert fig["tau_exact"] == tau and fig["L2_startup"].shape == fig["L2_steady"].shape == fig["u_centre"].shape == times.shape
    assert np.max(fig["L2_startup"]) <= 1e-14
    # (the fit window starts where the n = 3 mode is e^(-4) of the first: a one-mode fit is good to a per cent)
    assert abs(fig["tau_fit"] / tau - 1.0) <= 0.01
    u_exact = prm.gravity_g / (2.0 * prm.nu) * series["y_mid"] * (prm.DH - series["y_mid"])
    steady = np.array([profmod.l2_error(series["u_mean"][r, 1], u_exact) for r in range(len(times))])
    assert np.array_equal(fig["L2_steady"], steady) and np.all(np.diff(steady) < 0)
    assert steady[0] > tol > steady[-1]
    assert fig["t_developed"] == times[np.argmax(steady <= tol)]
    assert np.array_equal(fig["u_centre"], 0.5 * (series["u_mean"][:, 1, 9] + series["u_mean"][:, 1, 10]))
    # never developed: NaN
    assert math.isnan(driver.profile_series_figures(prm, series, band=1, tol=1e-9 * steady[-1])["t_developed"])
    short = {k: (v[:3] if isinstance(v, np.ndarray) and k != "y_mid" else v) for k, v in series.items()}
    assert math.isnan(driver.profile_series_figures(prm, short)["tau_fit"])  # no record inside the fit window


def test_figures_skip_empty_bins_as_l2_error_does(cfgmod, profmod, driver):
    prm = _prm(cfgmod)
    times = np.array([0.2, 0.6, 1.5])
    series = sc.synthetic_series(profmod, prm, times, empty=(0, 7))
    fig = driver.profile_series_figures(prm, series, band=0)
    y = series["y_mid"]
    for r, t in enumerate(times):
        want = profmod.poiseuille_startup(y, np.array([t]), prm.gravity_g, prm.nu, prm.DH)[:, 0]
        assert fig["L2_startup"][r] == profmod.l2_error(series["u_mean"][r, 0], want) <= 1e-14
    u_exact = prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y)
    assert fig["L2_steady"][0] == profmod.l2_error(series["u_mean"][0, 0], u_exact)
    void = sc.synthetic_series(profmod, prm, times, empty=range(20))
    fig = driver.profile_series_figures(prm, void, band=0)
    assert np.all(np.isnan(fig["L2_startup"])) and np.all(np.isnan(fig["L2_steady"])) and math.isnan(fig["t_developed"])


# 4 ---------------------------------------------------------------------------------------------------------------
def _chunk(capi, rng, steps, n_bands=2, n_bins=6, n_dropped=0):
    n = len(steps)
    rec = rng.standard_normal((n, n_bands, n_bins, 5))
    rec[..., 0] = rng.integers(0, 4, (n, n_bands, n_bins))  # counts, some of them zero
    times = np.column_stack([np.asarray(steps, dtype=np.float64), 0.01 * np.asarray(steps, dtype=np.float64)])
    return capi.profile_series_dict(1.0, times, rec, n_dropped)


def test_chunks_are_concatenated_in_order(capi, driver, profmod):
    rng = np.random.default_rng(3)
    chunks = [_chunk(capi, rng, [1, 2, 3]), _chunk(capi, rng, []), _chunk(capi, rng, [4, 5])]
    got = driver._concat_profile_series(1.0, chunks)
    assert got["step"].tolist() == [1, 2, 3, 4, 5] and got["step"].dtype == np.int64 and got["n_dropped"] == 0
    assert np.array_equal(got["t"], 0.01 * np.arange(1, 6)) and np.array_equal(got["y_mid"], chunks[0]["y_mid"])
    for f in sc.FIELDS:
        assert np.array_equal(got[f], np.concatenate([c[f] for c in chunks])) and got[f].shape == (5, 2, 6)
    for r, (c, k) in enumerate([(0, 0), (0, 1), (0, 2), (2, 0), (2, 1)]):
        for b in range(2):
            want = profmod.flow_stats_profile(1.0, *[chunks[c][f][k, b] for f in sc.FIELDS])
            for key in ("u_mean", "u_std", "uy_mean", "uy_std"):
                assert np.array_equal(got[key][r, b], want[key], equal_nan=True)
            assert np.array_equal(np.isnan(got["u_mean"][r, b]), chunks[c]["count"][k, b] == 0)


def test_a_chunk_that_lost_records_names_the_capacity(capi, driver):
    rng = np.random.default_rng(4)
    chunks = [_chunk(capi, rng, [1, 2, 3]), _chunk(capi, rng, [4, 5, 6], n_dropped=4)]
    with pytest.raises(RuntimeError, match=r"member 2: the profile series lost 4 records .* profiles_capacity >= 7 \(it held 3\)"):
        driver._concat_profile_series(1.0, chunks, "member 2: ")


def test_chunks_of_another_shape_are_refused(capi, driver):
    rng = np.random.default_rng(5)
    for other in (dict(n_bands=3), dict(n_bins=7)):
        with pytest.raises(ValueError, match="different shapes"):
            driver._concat_profile_series(1.0, [_chunk(capi, rng, [1, 2]), _chunk(capi, rng, [3], **other)])
    with pytest.raises(ValueError, match="at least one chunk"):
        driver._concat_profile_series(1.0, [])
