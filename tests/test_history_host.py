"""Step history (include/sphx.h section 2d) without a GPU: the C ABI declares and exports the three entry points, the
config struct has the header's layout, the Python binding checks its arguments before anything reaches the library, the
drivers refuse what they cannot do, and driver.history_figures is checked on synthetic records with known answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HISTORY_SYMBOLS = ("sphx_ctx_history_enable", "sphx_ctx_history_disable", "sphx_ctx_history_read")
FIELDS = ("step", "t", "dt", "vmax", "tau_bottom", "tau_top", "kinetic_energy", "u_bulk")


def test_history_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert "sphx_history_config" in hdr
    assert re.search(r"#define\s+SPHX_HISTORY_FIELDS\s+8\b", hdr)
    for name in HISTORY_SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert capi.HISTORY_FIELDS == FIELDS


def test_config_struct_matches_the_header(capi):
    # int32 every, int32 capacity, double t_from
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_history_config \{(.*?)\} sphx_history_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(t, n) for t, n in re.findall(r"(int32_t|double)\s+(\w+)\s*;", body)]
    assert members == [("int32_t", "every"), ("int32_t", "capacity"), ("double", "t_from")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in members] == list(capi.SphxHistoryConfig._fields_)
    assert C.sizeof(capi.SphxHistoryConfig) == 16
    assert (capi.SphxHistoryConfig.every.offset, capi.SphxHistoryConfig.capacity.offset,
            capi.SphxHistoryConfig.t_from.offset) == (0, 4, 8)


@pytest.mark.parametrize("kw", [dict(every=0), dict(every=-2), dict(every=1.5), dict(every=True), dict(capacity=0),
                                dict(capacity=(1 << 22) + 1), dict(capacity=2.0), dict(t_from=float("nan")),
                                dict(t_from=float("inf")), dict(t_from="soon")])
def test_binding_checks_the_config_first(capi, kw):
    with pytest.raises(capi.SphxError) as e:
        capi.history_config(**kw)
    assert e.value.identifier == "SPHX:History:config" and e.value.code == capi.SPHX_ERR_ARG


def test_binding_config_and_record_dict(capi):
    cfg = capi.history_config(every=3, capacity=1 << 22, t_from=0.25)
    assert (cfg.every, cfg.capacity, cfg.t_from) == (3, 1 << 22, 0.25)
    rec = np.arange(24, dtype=np.float64).reshape(3, 8)
    d = capi.history_dict(rec, 5)
    assert d["step"].dtype == np.int64 and list(d["step"]) == [0, 8, 16]
    for j, k in enumerate(FIELDS[1:], start=1):
        assert d[k].dtype == np.float64 and d[k].ndim == 1 and np.array_equal(d[k], rec[:, j])
    assert d["n_dropped"] == 5
    empty = capi.history_dict(np.zeros((0, 8)))
    assert all(empty[k].shape == (0,) for k in FIELDS) and empty["n_dropped"] == 0


def test_drivers_refuse_what_they_cannot_record(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.01, output_interval=0.01)
    with pytest.raises(ValueError, match="resident"):
        driver.run(prm, engine="mex", history_every=1)
    with pytest.raises(ValueError, match="history"):
        driver.run_batch([prm, prm], history_every=1)
    with pytest.raises(ValueError, match="history"):
        driver.run_ensemble([prm, prm], average_from=0.0, history_every=1)


# ---- history_figures on synthetic records ----
def _hist(t, dt, tau_b, tau_t, u_bulk):
    t = np.asarray(t, dtype=np.float64)
    n = len(t)
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).copy()
    return dict(step=np.arange(1, n + 1, dtype=np.int64), t=t, dt=full(dt), vmax=full(1.0), tau_bottom=full(tau_b),
                tau_top=full(tau_t), kinetic_energy=full(0.5), u_bulk=full(u_bulk), n_dropped=0)


def _exact(prm):
    return prm.gravity_g * prm.rho0 * prm.DH / 2.0, prm.gravity_g * prm.DH ** 2 / (12.0 * prm.nu)


def test_figures_constant_series_gives_exact_means(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    tau, ub = _exact(prm)
    rng = np.random.default_rng(3)
    dt = rng.uniform(1e-4, 3e-4, 200)
    hist = _hist(np.cumsum(dt), dt, 1.01 * tau, 0.98 * tau, 0.7 * ub)
    f = driver.history_figures(prm, hist, t_from=0.0, tol=0.05)
    assert (f["tau_target"], f["u_bulk_exact"]) == (tau, ub)
    assert f["tau_bottom_mean"] == 1.01 * tau and f["tau_top_mean"] == 0.98 * tau and f["u_bulk_mean"] == 0.7 * ub
    assert f["tau_bottom_dev"] == (1.01 * tau - tau) / tau and f["tau_top_dev"] == (0.98 * tau - tau) / tau
    assert f["u_bulk_dev"] == (0.7 * ub - ub) / ub
    assert f["n_records"] == 200
    assert f["t_settled"] == hist["t"][0]          # inside the 5 % band from the first record on
    assert np.isnan(driver.history_figures(prm, hist, tol=0.005)["t_settled"])  # 1 % / 2 % off: never inside 0.5 %


def test_figures_exponential_approach_gives_the_known_settling_time(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    tau, ub = _exact(prm)
    T, dt, tol = 0.4, 1e-3, 0.02
    t = dt * np.arange(1, 4001)
    # the bottom wall approaches from below with time constant T, the top wall twice as fast from above: the slower one
    # decides, |dev| = exp(-t / T) < tol  <=>  t > T ln(1 / tol)
    hist = _hist(t, dt, tau * (1.0 - np.exp(-t / T)), tau * (1.0 + np.exp(-2.0 * t / T)), ub)
    f = driver.history_figures(prm, hist, tol=tol)
    dev_b = np.abs(hist["tau_bottom"] - tau) / tau
    want = t[np.flatnonzero(~(dev_b < tol))[-1] + 1]
    assert f["t_settled"] == want
    assert 0.0 <= f["t_settled"] - T * np.log(1.0 / tol) <= dt * (1 + 1e-9)
    # a late excursion of ONE wall resets it; an excursion in the last record leaves no settled stretch at all
    late = dict(hist, tau_top=hist["tau_top"].copy())
    late["tau_top"][3000] = 1.5 * tau
    assert driver.history_figures(prm, late, tol=tol)["t_settled"] == t[3001]
    late["tau_top"][-1] = 1.5 * tau
    assert np.isnan(driver.history_figures(prm, late, tol=tol)["t_settled"])


def test_figures_ignore_records_before_t_from(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    tau, ub = _exact(prm)
    t = 0.01 * np.arange(1, 101)
    tb = np.where(t >= 0.5, 1.25 * tau, -7.0 * tau)    # garbage before the window
    tt = np.where(t >= 0.5, 0.75 * tau, 1e6)
    u = np.where(t >= 0.5, 0.5 * ub, np.nan)
    f = driver.history_figures(prm, _hist(t, 0.01, tb, tt, u), t_from=0.5)
    assert f["n_records"] == int(np.count_nonzero(t >= 0.5)) == 51   # t == t_from belongs to the window
    assert f["tau_bottom_mean"] == 1.25 * tau and f["tau_top_mean"] == 0.75 * tau and f["u_bulk_mean"] == 0.5 * ub
    none = driver.history_figures(prm, _hist(t, 0.01, tb, tt, u), t_from=2.0)
    assert none["n_records"] == 0 and np.isnan(none["tau_bottom_mean"]) and np.isnan(none["u_bulk_dev"])


def test_figures_honour_unequal_dt_weights(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    tau, ub = _exact(prm)
    dt = np.array([1.0, 3.0, 4.0]) * 2.0 ** -10
    f = driver.history_figures(prm, _hist(np.cumsum(dt), dt, [1.0, 2.0, 4.0], [8.0, 0.0, -2.0], [0.0, 0.0, 1.0]))
    assert f["tau_bottom_mean"] == (1 * 1 + 3 * 2 + 4 * 4) / 8       # not the plain mean 7 / 3
    assert f["tau_top_mean"] == (1 * 8 + 0 - 4 * 2) / 8
    assert f["u_bulk_mean"] == 0.5
    np.testing.assert_allclose(f["u_bulk_dev"], (0.5 - ub) / ub, rtol=1e-15)


def test_figures_of_a_mirrored_flow(cfgmod, driver):
    """g -> -g, tau and u_bulk -> their negatives: the means and the targets flip their sign, the relative deviations and
    t_settled (|tau - tau_target| over |tau_target|) stay."""
    T, dt, tol = 0.4, 1e-3, 0.02
    t = dt * np.arange(1, 2001)
    out = {}
    for sign in (1, -1):
        prm = cfgmod.params_from_values(dp=0.05, DL=3.0, U_bulk=sign * 0.666667)
        tau, ub = _exact(prm)
        assert np.sign(tau) == sign and np.sign(ub) == sign
        hist = _hist(t, dt, tau * (1.0 - np.exp(-t / T)), tau * (1.0 + np.exp(-2.0 * t / T)), ub * (1.0 - np.exp(-t / T)))
        out[sign] = driver.history_figures(prm, hist, t_from=0.5, tol=tol)
    a, b = out[1], out[-1]
    assert np.isfinite(a["t_settled"]) and a["t_settled"] > 1.0 and b["t_settled"] == a["t_settled"]
    for k in ("tau_target", "u_bulk_exact", "tau_bottom_mean", "tau_top_mean", "u_bulk_mean"):
        assert a[k] > 0 and abs(b[k] + a[k]) <= 1e-12 * a[k], (k, a[k], b[k])
    for k in ("tau_bottom_dev", "tau_top_dev", "u_bulk_dev"):
        assert abs(b[k] - a[k]) <= 1e-12 * abs(a[k]), (k, a[k], b[k])
    assert a["n_records"] == b["n_records"]
