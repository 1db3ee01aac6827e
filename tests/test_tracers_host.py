"""No device: the host side of the particle tracers (include/sphx.h sections 2p / 2q) -- profile.tracer_rows, unwrap_tracers,
tracer_profiles and pool_tracers on synthetic series whose answers are known in closed form, capi.tracers_config's refusals,
the driver's refusals of bad tracers= arguments before a device is touched, and the eight exported symbols."""
import numpy as np
import pytest

import tracer_cases as tc

DL, DH = 1.5, 1.0   # (dyadic: the wrapped and unwrapped positions below are exact in float64)


def _uniform(x0, step, n, u):
    """n records of tracers starting at x0 [T] that move by `step` per record at velocity u: the truth is representable"""
    k = np.arange(n)[:, None]
    x_true = np.asarray(x0, dtype=np.float64)[None, :] + k * step
    t = np.arange(n) * (step / u)
    return x_true, tc.synthetic_series(x_true, 0.5, u, t, DL)


# ---- unwrap_tracers ----
@pytest.mark.parametrize("step,u,what", [(0.25, 2.0, "to the right"), (-0.25, -2.0, "to the left"), (0.625, 1.0, "several crossings in a row"),
                                         (-0.625, -4.0, "several to the left")])
def test_unwrap_recovers_the_truth_exactly(profmod, step, u, what):
    x0 = np.array([0.0, 0.125, 0.75, 1.375, 1.0])
    x_true, tr = _uniform(x0, step, 24, u)
    assert np.all((tr["x"] >= 0.0) & (tr["x"] < DL))
    crossings = np.count_nonzero(np.abs(np.diff(tr["x"], axis=0)) > 0.5 * DL, axis=0)
    assert np.all(crossings >= 3), (what, crossings)
    got = profmod.unwrap_tracers(tr, DL)
    assert np.array_equal(got["x_unwrapped"], x_true), what
    assert got["x"] is tr["x"] and "x_unwrapped" not in tr            # a copy of the dict, the series untouched


def test_unwrap_a_particle_sitting_on_the_seam(profmod):
    # x = DL exactly is held as x = 0: records at 1.25, 1.5 (-> 0.0), 1.75 (-> 0.25), and back down again through 0
    x_true = np.array([[1.25], [1.5], [1.75], [1.5], [1.25], [1.5], [1.5]])
    t = 0.125 * np.arange(len(x_true))
    u = np.array([[2.0], [2.0], [0.0], [-2.0], [0.0], [2.0], [0.0]])
    tr = tc.synthetic_series(x_true, 0.5, u, t, DL)
    assert tr["x"][:, 0].tolist() == [1.25, 0.0, 0.25, 0.0, 1.25, 0.0, 0.0]
    assert np.array_equal(profmod.unwrap_tracers(tr, DL)["x_unwrapped"], x_true)
    # at rest on x = 0 from the first record on: stays 0, never DL
    rest = tc.synthetic_series(np.zeros((5, 1)), 0.5, 0.0, t[:5], DL)
    assert np.array_equal(profmod.unwrap_tracers(rest, DL)["x_unwrapped"], np.zeros((5, 1)))


def test_unwrap_refuses_a_series_too_coarse(profmod):
    x_true, tr = _uniform([0.0, 0.5], 0.75, 6, 1.0)                # |u| dt = DL / 2 exactly: not unwrappable
    with pytest.raises(ValueError, match="too coarse"):
        profmod.unwrap_tracers(tr, DL)
    x_true, tr = _uniform([0.0, 0.5], 0.75 - 2.0 ** -20, 6, 1.0)   # just below: fine
    assert np.array_equal(profmod.unwrap_tracers(tr, DL)["x_unwrapped"], x_true)
    fast = dict(tr, u_x=np.where(np.arange(6)[:, None] == 3, 40.0, tr["u_x"]))   # one record of one tracer too fast
    with pytest.raises(ValueError, match="too coarse"):
        profmod.unwrap_tracers(fast, DL)
    with pytest.raises(ValueError):
        profmod.unwrap_tracers(dict(tr, t=tr["t"][::-1].copy()), DL)


def test_one_record_and_tracer_rows(profmod):
    tr = tc.synthetic_series(np.array([[0.25, 2.0]]), 0.5, 1.0, [0.0], DL)
    assert np.array_equal(profmod.unwrap_tracers(tr, DL)["x_unwrapped"], tr["x"])
    rng = np.random.default_rng(1)
    pos, vel = rng.random((9, 2)), rng.random((9, 2))
    rows = profmod.tracer_rows(pos, vel, [7, 0, 3])
    assert rows["x"].tolist() == pos[[7, 0, 3], 0].tolist() and rows["y"].tolist() == pos[[7, 0, 3], 1].tolist()
    assert rows["u_x"].tolist() == vel[[7, 0, 3], 0].tolist() and rows["u_y"].tolist() == vel[[7, 0, 3], 1].tolist()


# ---- tracer_profiles ----
G, NU = 0.8, 0.1


def _series(y, t, u=None, x=None):
    """a tracers dict of paths y [n, T] at times t: u_x the analytic profile at the path's y unless given, x its integral"""
    y = np.asarray(y, dtype=np.float64)
    n, T = y.shape
    u = G / (2 * NU) * y * (DH - y) if u is None else np.broadcast_to(np.asarray(u, dtype=np.float64), (n, T))
    if x is None:
        x = np.concatenate([np.zeros((1, T)), np.cumsum(0.5 * (u[1:] + u[:-1]) * np.diff(t)[:, None], axis=0)])
    return dict(ids=np.arange(T, dtype=np.int32), step=np.arange(n, dtype=np.int64), t=np.asarray(t, dtype=np.float64), x=x - np.floor(x / DL) * DL,
                y=y, u_x=np.array(u), u_y=np.zeros((n, T)), n_dropped=0, n_missing=0, x_unwrapped=x)


def test_ballistic_paths_give_a_squared_tau_squared(profmod):
    a, dt, n = 0.03125, 0.015625, 65
    t = dt * np.arange(n)
    y = np.array([0.25, 0.375, 0.5])[None, :] + a * t[:, None]
    f = profmod.tracer_profiles(_series(y, t), DL, DH, G, NU, lags=[1, 2, 4, 16, 64])
    assert f["lags"].tolist() == [1, 2, 4, 16, 64] and f["n_tracers"] == 3 and f["n_records"] == n
    assert np.allclose(f["tau"], dt * f["lags"], rtol=1e-14, atol=0)
    assert np.allclose(f["msd_y"], (a * f["tau"]) ** 2, rtol=1e-12, atol=0)
    assert abs(f["y_drift"] - a) <= 1e-14 * a
    # the default lags: 1, 2, 4, ... up to a quarter of the series
    assert profmod.tracer_profiles(_series(y, t), DL, DH, G, NU)["lags"].tolist() == [1, 2, 4, 8, 16]


def test_a_random_walk_of_known_D(profmod):
    D, dt, T, R = 2.5e-4, 0.01, 400, 513
    rng = np.random.default_rng(20240)
    t = dt * np.arange(R)
    y = 0.5 + np.concatenate([np.zeros((1, T)), np.cumsum(np.sqrt(2 * D * dt) * rng.standard_normal((R - 1, T)), axis=0)])
    for lags in ([1], [8], [1, 2, 4, 8], [4, 16, 64]):
        f = profmod.tracer_profiles(_series(y, t), DL, DH, G, NU, lags=lags)
        se = D * np.sqrt(2.0 / (T * (R // max(lags))))
        print(f"lags {lags}: D_y = {f['D_y']:.6e}, off by {abs(f['D_y'] - D) / se:.2f} standard errors")
        assert abs(f["D_y"] - D) <= 5 * se, (lags, f["D_y"], se)
    assert abs(f["y_drift"]) < 5 * np.sqrt(2 * D * t[-1] / T) / t[-1]


def test_the_analytic_field_has_no_velocity_error(profmod):
    rng = np.random.default_rng(3)
    t = 0.01 * np.arange(40)
    y = np.tile(rng.random(50) * 0.8 + 0.1, (40, 1))                 # every tracer on its streamline
    f = profmod.tracer_profiles(_series(y, t), DL, DH, G, NU, lags=[1, 4])
    assert f["u_dev_rms"] == 0.0 and np.all(f["msd_y"] == 0.0) and f["D_y"] == 0.0 and f["y_drift"] == 0.0
    assert np.all(f["msd_x_rel"] <= (1e-15 * DL) ** 2)                # x moved with u_exact(y0)
    # a uniform excess velocity of 1 % of U_max shows as that
    U_max = G * DH ** 2 / (8 * NU)
    s = _series(y, t)
    s["u_x"] = s["u_x"] + 0.01 * U_max
    assert abs(profmod.tracer_profiles(s, DL, DH, G, NU, lags=[1])["u_dev_rms"] - 0.01) < 1e-12
    # the margin: tracers that start within y_margin of a wall are left out
    y2 = y.copy()
    y2[:, :5] = 0.01
    assert profmod.tracer_profiles(_series(y2, t), DL, DH, G, NU, lags=[1], y_margin=0.05)["n_tracers"] == 45
    with pytest.raises(ValueError):
        profmod.tracer_profiles(_series(y2[:, :5], t), DL, DH, G, NU, lags=[1], y_margin=0.05)
    with pytest.raises(ValueError):
        profmod.tracer_profiles(_series(y, t), DL, DH, G, NU, lags=[40])


# ---- pool_tracers ----
def test_pool_refuses_members_that_differ(profmod):
    t = 0.01 * np.arange(6)
    a = _series(np.full((6, 3), 0.5), t)
    b = _series(np.full((6, 3), 0.25), t)
    p = profmod.pool_tracers([a, b])
    assert p["x"].shape == (6, 6) and p["ids"].tolist() == [0, 1, 2, 0, 1, 2] and p["member"].tolist() == [0, 0, 0, 1, 1, 1]
    assert np.array_equal(p["y"][:, 3:], b["y"]) and np.array_equal(p["x_unwrapped"][:, :3], a["x_unwrapped"]) and p["n_members"] == 2
    for k, other in (("ids", np.array([0, 1, 3], dtype=np.int32)), ("step", a["step"] + 1), ("t", t * (1 + 1e-15))):
        with pytest.raises(ValueError, match=k):
            profmod.pool_tracers([a, dict(b, **{k: other})])
    with pytest.raises(ValueError):
        profmod.pool_tracers([])


# ---- the binding and the driver, before any device ----
def test_tracers_config_refusals(capi):
    nf, nt = 100, 140
    cfg, ids = capi.tracers_config(nf, nt, [99, 0, 5], every=2, capacity=7, t_from=0.5)
    assert (cfg.n_tracers, cfg.every, cfg.capacity, cfg.t_from) == (3, 2, 7, 0.5) and ids.dtype == np.int32 and ids.tolist() == [99, 0, 5]
    assert [cfg.ids[k] for k in range(3)] == [99, 0, 5]
    for bad in (dict(ids=None), dict(ids=[]), dict(ids=[1, 1]), dict(ids=[-1]), dict(ids=[nf]), dict(ids=[nt - 1]), dict(ids=[nt]),
                dict(ids=[0.5]), dict(ids=[[1, 2]]), dict(ids=[True]), dict(ids=list(range(nf)) + [0]), dict(every=0), dict(every=1.5),
                dict(capacity=0), dict(capacity=(1 << 27) // 12 + 1), dict(capacity=(1 << 27) // 24 + 1, n_members=2),
                dict(t_from=float("nan")), dict(t_from=float("inf")), dict(t_from="soon")):
        kw = dict(dict(ids=[99, 0, 5]), **bad)
        with pytest.raises(capi.SphxError) as e:
            capi.tracers_config(nf, nt, kw.pop("ids"), **kw)
        assert e.value.identifier == "SPHX:Tracers:config" and e.value.code == capi.SPHX_ERR_ARG, bad
    assert capi.tracers_config(nf, nt, np.arange(nf), capacity=(1 << 27) // (4 * nf))[0].n_tracers == nf
    d = capi.tracers_dict([4, 2], np.array([[3.0, 0.5]]), np.arange(8.0).reshape(1, 2, 4), 1, 0)
    assert d["step"].tolist() == [3] and d["x"].tolist() == [[0.0, 4.0]] and d["u_y"].tolist() == [[3.0, 7.0]] and d["n_dropped"] == 1


def test_the_driver_refuses_bad_tracers_before_a_device(cfgmod, driver, capi, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device object was created")
    monkeypatch.setattr(capi.Context, "from_parts", classmethod(no_device))
    monkeypatch.setattr(capi.Batch, "from_parts", classmethod(no_device))
    prm = cfgmod.params_from_values(dp=0.1, DL=0.6, end_time=0.01, output_interval=0.01)
    nf = driver.init_particles(prm)["n_fluid"]
    for bad in ("some", 0, -3, nf + 1, True):
        with pytest.raises(ValueError, match="tracers"):
            driver.run(prm, tracers=bad)
        with pytest.raises(ValueError, match="tracers"):
            driver.run_sweep([prm, prm], tracers=bad)
    for bad in ([0, 0], [nf], [-1], [], [0.5]):
        with pytest.raises(capi.SphxError) as e:
            driver.run(prm, tracers=bad)
        assert e.value.identifier == "SPHX:Tracers:config", bad
    for kw in (dict(tracers_every=0), dict(tracers_capacity=0), dict(tracers_from=float("nan"))):
        with pytest.raises(capi.SphxError) as e:
            driver.run_sweep([prm, prm], tracers=4, **kw)
        assert e.value.identifier == "SPHX:Tracers:config", kw
    with pytest.raises(ValueError, match="resident"):
        driver.run(prm, engine="mex", tracers=4)
    # what an int means: that many distinct fluid rows, the same ones every time
    ids = driver.tracer_ids(16, nf)
    assert len(ids) == 16 == len(set(ids.tolist())) and ids.min() >= 0 and ids.max() < nf and np.array_equal(ids, driver.tracer_ids(16, nf))
    assert driver.tracer_ids("all", nf).tolist() == list(range(nf))


def test_tracer_figures_scale_by_nu(cfgmod, driver, profmod):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.5)
    rng = np.random.default_rng(5)
    D, dt, T, R = 1e-4, 0.01, 200, 129
    t = dt * np.arange(R)
    y = 0.5 * prm.DH + np.concatenate([np.zeros((1, T)), np.cumsum(np.sqrt(2 * D * dt) * rng.standard_normal((R - 1, T)), axis=0)])
    u = prm.gravity_g / (2 * prm.nu) * y * (prm.DH - y)
    x = np.concatenate([np.zeros((1, T)), np.cumsum(0.5 * (u[1:] + u[:-1]) * dt, axis=0)])
    tr = dict(ids=np.arange(T, dtype=np.int32), step=np.arange(R, dtype=np.int64), t=t, x=x - np.floor(x / prm.DL) * prm.DL, y=y, u_x=u,
              u_y=np.zeros((R, T)), n_dropped=0, n_missing=0)
    f = driver.tracer_figures(prm, tr)
    assert f["D_y_nu"] == f["D_y"] / prm.nu and abs(f["D_y"] - D) < 0.25 * D and f["u_dev_rms"] == 0.0 and f["n_tracers"] == T


def test_the_library_exports_the_tracer_symbols(capi):
    L = capi.lib()
    names = [f"sphx_{who}_tracers_{what}" for who in ("ctx", "batch") for what in ("enable", "disable", "sample", "read")]
    assert len(names) == 8
    for n in names:
        assert n in capi.EXPORTS and getattr(L, n) is not None
    # no call reaches a device: a NULL handle is refused first
    assert L.sphx_ctx_tracers_sample(None) == capi.SPHX_ERR_ARG and L.sphx_last_error_id() == b"SPHX:Ctx:null"
    assert L.sphx_batch_tracers_disable(None) == capi.SPHX_ERR_ARG and L.sphx_last_error_id() == b"SPHX:Batch:null"
