"""Step history of batches (include/sphx.h section 2f) without a GPU: the C ABI declares and exports the three entry points
and refuses a NULL batch, capi.Batch checks its arguments before anything reaches the library, driver.run_sweep refuses bad
inputs before the device, and the sweep's table is checked on synthetic histories with known answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sphx_batch_history_enable", "sphx_batch_history_disable", "sphx_batch_history_read")
PHYSICS = ("mu", "c_f", "p0", "gravity_g", "transport_coeff")


def test_symbols_declared_and_exported(capi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)


def test_null_batch_is_refused(capi):
    L = capi.lib()
    cfg = capi.SphxHistoryConfig(every=1, capacity=16, t_from=0.0)
    calls = {"sphx_batch_history_enable": (C.byref(cfg),), "sphx_batch_history_disable": (),
             "sphx_batch_history_read": (0, None, None, None, 0)}
    assert set(calls) == set(SYMBOLS)
    for name, args in calls.items():
        rc = getattr(L, name)(None, *args)
        assert rc == capi.SPHX_ERR_ARG, name
        assert L.sphx_last_error_id().decode() == "SPHX:Batch:null", name


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} made before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(every=0), dict(every=1.5), dict(capacity=0), dict(capacity=(1 << 22) + 1),
                                dict(capacity=(1 << 24) // 5 + 1),  # 5 members: n_members * capacity > 1 << 24
                                dict(t_from=float("nan")), dict(t_from=float("inf")), dict(t_from="soon")])
def test_enable_checks_arguments_before_the_device(capi, monkeypatch, kw):
    monkeypatch.setattr(capi, "lib", lambda: _NoLib())
    b = object.__new__(capi.Batch)
    b._h = C.c_void_p()  # (nothing to destroy)
    b.n_members = 5
    with pytest.raises(capi.SphxError) as e:
        b.history_enable(**kw)
    assert e.value.identifier == "SPHX:History:config" and e.value.code == capi.SPHX_ERR_ARG


def test_the_total_cap_is_on_members_times_capacity(capi):
    assert capi.history_config(capacity=(1 << 24) // 5, n_members=5).capacity == (1 << 24) // 5
    assert capi.history_config(capacity=1 << 22, n_members=4).capacity == 1 << 22
    with pytest.raises(capi.SphxError):
        capi.history_config(capacity=1 << 22, n_members=5)


class _NoBatch:
    def __init__(self, *a, **k):
        raise AssertionError("a batch was created before the arguments were checked")

    @classmethod
    def from_parts(cls, *a, **k):
        cls()


def test_run_sweep_refusals(cfgmod, geom, driver, monkeypatch):
    monkeypatch.setattr(driver.capi, "Batch", _NoBatch)
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu) for mu in (0.1, 0.2)]
    with pytest.raises(ValueError, match="at least one"):
        driver.run_sweep([])
    other = cfgmod.params_from_values(dp=0.05, DL=3.0, output_interval=0.5)
    with pytest.raises(ValueError, match="output_interval"):
        driver.run_sweep([prms[0], other])
    longer = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=prms[0].t_end + 1.0)
    with pytest.raises(ValueError, match="t_end"):
        driver.run_sweep([prms[0], longer])
    with pytest.raises(ValueError, match="parts_list"):
        driver.run_sweep(prms, parts_list=[geom.init_particles(prms[0])])


# ---- the table, on synthetic histories ----
def _hist(t, dt, tau_b, tau_t, u_bulk, n_dropped=0):
    t = np.asarray(t, dtype=np.float64)
    n = len(t)
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).copy()
    return dict(step=np.arange(1, n + 1, dtype=np.int64), t=t, dt=full(dt), vmax=full(1.0), tau_bottom=full(tau_b),
                tau_top=full(tau_t), kinetic_energy=full(0.5), u_bulk=full(u_bulk), n_dropped=n_dropped)


def test_sweep_table_on_synthetic_histories(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, c_f=c_f, transport_coeff=tc)
            for mu, c_f, tc in ((0.1, 15.0, 0.3), (0.2, 17.0, 0.2), (0.05, 13.0, 0.1), (0.15, 15.0, 0.3))]
    exact = [(p.gravity_g * p.rho0 * p.DH / 2.0, p.gravity_g * p.DH ** 2 / (12.0 * p.nu)) for p in prms]
    T, dt, tol = 0.4, 1e-3, 0.02
    t = dt * np.arange(1, 4001)
    (tau0, ub0), (tau1, ub1), (tau2, ub2), (tau3, ub3) = exact
    hists = [
        _hist(t, dt, 1.01 * tau0, 0.98 * tau0, 0.7 * ub0),                                           # constant: exact means
        _hist(t, dt, tau1 * (1.0 - np.exp(-t / T)), tau1 * (1.0 + np.exp(-2.0 * t / T)), ub1),          # settles at T ln(1 / tol)
        _hist(t[:1500], dt, 1.25 * tau2, 0.75 * tau2, 0.5 * ub2, n_dropped=3),                          # ends before history_from
        _hist(t[:0], dt, tau3, tau3, ub3),                                                              # no record at all
    ]
    steps = [4000, 4000, 1500, 0]
    table = driver.sweep_table(prms, hists, steps, history_from=2.0, settle_tol=tol)
    figs = [driver.history_figures(p, h, t_from=2.0, tol=tol) for p, h in zip(prms, hists)]
    assert set(table) == set(PHYSICS) | {"steps", "n_dropped"} | set(figs[0])
    for k, v in table.items():
        assert isinstance(v, np.ndarray) and v.shape == (4,), k
    for k in PHYSICS:
        assert list(table[k]) == [getattr(p, k) for p in prms], k
    assert table["steps"].dtype == np.int64 and list(table["steps"]) == steps
    assert table["n_dropped"].dtype == np.int64 and list(table["n_dropped"]) == [0, 0, 3, 0]
    for k in figs[0]:
        assert np.array_equal(table[k], np.array([f[k] for f in figs]), equal_nan=True), k
    # known answers
    assert table["tau_bottom_mean"][0] == 1.01 * tau0 and table["tau_top_mean"][0] == 0.98 * tau0
    assert table["u_bulk_dev"][0] == (0.7 * ub0 - ub0) / ub0 and table["u_bulk_mean"][1] == ub1
    assert list(table["n_records"]) == [int(np.count_nonzero(t >= 2.0))] * 2 + [0, 0]
    assert np.isnan(table["t_settled"][0])                              # 1 % / 2 % off: never inside the 2 % band for good
    assert 0.0 <= table["t_settled"][1] - T * np.log(1.0 / tol) <= dt * (1 + 1e-9)
    # members without a record at t >= history_from: NaN means and deviations, the targets stay
    for m in (2, 3):
        for k in ("tau_bottom_mean", "tau_top_mean", "u_bulk_mean", "tau_bottom_dev", "tau_top_dev", "u_bulk_dev"):
            assert np.isnan(table[k][m]), (m, k)
        assert table["tau_target"][m] == exact[m][0] and table["u_bulk_exact"][m] == exact[m][1]
    assert np.isnan(table["t_settled"][2]) and np.isnan(table["t_settled"][3])  # 25 % off; nothing recorded


def test_sweep_result_fields(driver):
    res = driver.SweepResult(members=[], table={}, wall_seconds=1.0)
    assert res.grid_policy == {} and res.members == [] and res.table == {}
