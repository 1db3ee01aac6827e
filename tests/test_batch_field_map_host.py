"""Field maps of batches (include/sphx.h section 2g) without a GPU: the C ABI declares and exports the five entry points and
refuses a NULL batch, capi.Batch checks its arguments and its state before anything reaches the library, the node bound
counts the members, profile.pool_field_maps is checked on hand-built planes, and the three batch drivers refuse or pass on the
field keywords -- followed through a stand-in for capi.Batch that records what the driver asks of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sphx_batch_field_map_enable", "sphx_batch_field_map_disable", "sphx_batch_field_map_reset",
           "sphx_batch_field_map_sample", "sphx_batch_field_map_read")
PLANES = ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")


def test_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert "Batches (section 2b) and slabs have no field maps" not in raw   # only slabs remain without


def test_null_batch_is_refused(capi):
    L = capi.lib()
    cfg = capi.SphxFieldMapConfig(nx=0, ny=0, every=1, with_walls=0, t_from=0.0)
    calls = {"sphx_batch_field_map_enable": (C.byref(cfg),), "sphx_batch_field_map_disable": (),
             "sphx_batch_field_map_reset": (), "sphx_batch_field_map_sample": (),
             "sphx_batch_field_map_read": (0, None, None, *[None] * 6, None, None, None)}
    assert set(calls) == set(SYMBOLS)
    for name, args in calls.items():
        rc = getattr(L, name)(None, *args)
        assert rc == capi.SPHX_ERR_ARG, name
        assert L.sphx_last_error_id().decode() == "SPHX:Batch:null", name


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} made before the arguments were checked")


def _bare(capi, monkeypatch, cls, members=4):
    monkeypatch.setattr(capi, "lib", lambda: _NoLib())
    b = object.__new__(cls)
    b._h = C.c_void_p()  # (nothing to destroy)
    b._field_map = None
    prm = capi.SphxParams(DL=3.0, DH=1.0, dp=0.05)
    if cls is capi.Batch:
        b.n_members, b.params = members, [prm] * members
    else:
        b.params = prm
    return b


@pytest.mark.parametrize("kw", [dict(nx=1), dict(ny=1), dict(nx=-3), dict(nx=2.0), dict(every=0), dict(every=1.5),
                                dict(t_from=float("nan")), dict(t_from="soon"), dict(with_walls=2),
                                dict(nx=1 << 12, ny=(1 << 11) + 1)])  # 4 members: n_members * nx * ny > 1 << 25
def test_enable_checks_arguments_before_the_device(capi, monkeypatch, kw):
    b = _bare(capi, monkeypatch, capi.Batch)
    with pytest.raises(capi.SphxError) as e:
        b.field_map_enable(**kw)
    assert e.value.identifier == "SPHX:Field:config" and e.value.code == capi.SPHX_ERR_ARG
    assert b._field_map is None


def test_state_is_checked_before_the_device(capi, monkeypatch):
    for cls, where in ((capi.Batch, "batch"), (capi.Context, "context")):
        b = _bare(capi, monkeypatch, cls)
        for call in (b.field_map, b.field_map_sums, b.field_map_sample, b.field_map_reset):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:Field:disabled" and e.value.code == capi.SPHX_ERR_STATE
            assert e.value.message == f"the field map is not enabled on this {where}"


def test_the_node_bound_counts_the_members(capi):
    nx, ny = 1 << 12, 1 << 11                                          # 1 << 23 nodes a member
    assert capi.field_map_config(nx=nx, ny=ny, n_members=4).nx == nx   # 4 << 23 = 1 << 25: allowed
    assert capi.field_map_config(nx=nx, ny=ny + 1).ny == ny + 1        # one channel: far below the bound
    for kw in (dict(nx=nx, ny=ny + 1, n_members=4), dict(nx=nx, ny=ny, n_members=5), dict(nx=2, ny=2, n_members=(1 << 23) + 1)):
        with pytest.raises(capi.SphxError) as e:
            capi.field_map_config(**kw)
        assert e.value.identifier == "SPHX:Field:config" and "n_members * nx * ny" in e.value.message, kw
    with pytest.raises(capi.SphxError) as e:                           # a context's text stays what it was
        capi.field_map_config(nx=1 << 13, ny=(1 << 12) + 1)
    assert e.value.message == "nx * ny must not exceed 1 << 25 nodes"


# ---- profile.pool_field_maps on hand-built planes ----
def _planes(u_samples, v_samples, hit):
    """The six planes of a [ny, nx] map after the samples u_samples / v_samples (lists of [ny, nx] arrays), at the nodes `hit`."""
    z = lambda a: np.where(hit, a, 0.0)
    n = float(len(u_samples))
    return dict(count=z(np.full(hit.shape, n)), sum_w=z(np.full(hit.shape, 0.5 * n)), sum_ux=z(sum(u_samples)),
                sum_uy=z(sum(v_samples)), sum_ux2=z(sum(u * u for u in u_samples)), sum_uy2=z(sum(v * v for v in v_samples)))


def test_pool_of_two_members_by_hand(profmod):
    DL, DH, ny, nx = 3.0, 1.0, 2, 3
    every = np.ones((ny, nx), dtype=bool)
    only_a = every.copy()
    only_a[1, 2] = False                                               # member b never sampled node (1, 2)
    ua = [np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]), np.array([[3.0, 2.0, 1.0], [0.0, 5.0, 8.0]])]   # two samples: means 2 2 2 / 2 5 7
    ub = [np.array([[4.0, 2.0, 0.0], [6.0, 1.0, 9.0]])]                                                # one sample
    va = [np.full((ny, nx), 0.5), np.full((ny, nx), -0.5)]
    vb = [np.full((ny, nx), 0.25)]
    a = dict(_planes(ua, va, every), n_samples=2, t_first=0.3, t_last=0.5)
    b = dict(_planes(ub, vb, only_a), n_samples=1, t_first=0.2, t_last=0.4)
    out = profmod.pool_field_maps(DL, DH, [a, b])
    assert out["n_members"] == 2 and out["n_samples"] == 3 and (out["t_first"], out["t_last"]) == (0.2, 0.5)
    assert np.array_equal(out["count"], np.array([[3.0, 3.0, 3.0], [3.0, 3.0, 2.0]]))
    # pooled mean = all samples of both members over their number; at (1, 2) only member a's two samples
    want = np.array([[8.0 / 3, 2.0, 4.0 / 3], [10.0 / 3, 11.0 / 3, 7.0]])
    np.testing.assert_allclose(out["u_x"], want, rtol=1e-15)
    np.testing.assert_allclose(out["u_y"], np.array([[0.25 / 3] * 3, [0.25 / 3, 0.25 / 3, 0.0]]), rtol=1e-15, atol=1e-17)
    np.testing.assert_allclose(out["u_x_std"][1, 2], 1.0, rtol=1e-15)                  # samples 6 and 8
    np.testing.assert_allclose(out["u_x_std"][0, 0], np.std([1.0, 3.0, 4.0]), rtol=1e-14)
    assert np.all(out["weight"] == 0.5)
    assert np.array_equal(out["x"], np.linspace(0.0, DL, nx)) and np.array_equal(out["y"], np.linspace(0.0, DH, ny))
    # u_x_se: std(ddof = 1) of the two members' own time means / sqrt(2) = |mean_a - mean_b| / 2; NaN where b has no mean
    mean_a, mean_b = np.array([[2.0, 2.0, 2.0], [2.0, 5.0, 7.0]]), ub[0]
    se = np.abs(mean_a - mean_b) / 2.0
    assert np.isnan(out["u_x_se"][1, 2])
    np.testing.assert_allclose(out["u_x_se"][only_a], se[only_a], rtol=1e-14, atol=0.0)
    assert out["u_x_se"][0, 1] == 0.0
    # the total is what field_map_means makes of the planes added in member order
    total = {k: a[k] + b[k] for k in PLANES}
    ref = profmod.field_map_means(DL, DH, **total, n_samples=3, t_first=0.2, t_last=0.5)
    for k in ("count", "weight", "u_x", "u_y", "u_x_std", "u_y_std"):
        assert np.array_equal(out[k], ref[k], equal_nan=True), k


def test_pool_of_one_member_and_of_none(profmod):
    hit = np.array([[True, False], [True, True]])
    s = dict(_planes([np.array([[1.0, 9.0], [2.0, 3.0]])], [np.zeros((2, 2))], hit), n_samples=1, t_first=0.1, t_last=0.1)
    one = profmod.pool_field_maps(2.0, 1.0, [s])
    ref = profmod.field_map_means(2.0, 1.0, **s)
    for k in ("count", "weight", "u_x", "u_y", "u_x_std", "u_y_std", "x", "y"):
        assert np.array_equal(one[k], ref[k], equal_nan=True), k
    assert np.isnan(one["u_x"][0, 1]) and one["n_samples"] == 1 and one["n_members"] == 1
    assert one["u_x_se"].shape == (2, 2) and np.all(np.isnan(one["u_x_se"]))
    never = dict(s, n_samples=0, t_first=float("nan"), t_last=float("nan"))
    assert np.isnan(profmod.pool_field_maps(2.0, 1.0, [never])["t_first"])
    with pytest.raises(ValueError, match="at least one"):
        profmod.pool_field_maps(2.0, 1.0, [])
    with pytest.raises(ValueError):
        profmod.pool_field_maps(2.0, 1.0, iter(()))


# ---- the drivers ----
class _NoBatch:
    def __init__(self, *a, **k):
        raise AssertionError("a batch was created before the arguments were checked")

    @classmethod
    def from_parts(cls, *a, **k):
        cls()


def test_run_batch_refuses_field_from(cfgmod, driver, monkeypatch):
    monkeypatch.setattr(driver.capi, "Batch", _NoBatch)
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu) for mu in (0.1, 0.2)]
    with pytest.raises(ValueError, match=r"run_batch.*field map.*run_ensemble and run_sweep"):
        driver.run_batch(prms, field_from=0.0)
    with pytest.raises(ValueError, match="at least one"):
        driver.run_ensemble([], average_from=0.0, field_from=0.0)
    with pytest.raises(ValueError, match="at least one"):
        driver.run_sweep([], field_from=0.0)


def _stand_in(capi, profmod, nx, ny):
    """A stand-in for capi.Batch: no device, the calls a batch driver makes recorded in order, field-map planes with known values."""

    class FakeBatch:
        made = []

        def __init__(self, prms, parts_list, launch):
            self.prms, self.parts, self.launch, self.calls, self.n_adv = list(prms), list(parts_list), launch, [], 0
            self.n_members = len(self.prms)
            FakeBatch.made.append(self)

        @classmethod
        def from_parts(cls, prms, parts_list, **kw):
            return cls(prms, parts_list, kw)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.calls.append(("close",))

        def field_map_enable(self, **kw):
            self.calls.append(("field_map_enable", kw))

        def flow_stats_enable(self, **kw):
            self.calls.append(("flow_stats_enable", kw))
            self.n_bins = kw["n_bins"]

        def history_enable(self, **kw):
            self.calls.append(("history_enable", kw))

        def advance(self, target):
            self.n_adv += 1
            self.calls.append(("advance", target))
            return [dict(t=target, step=10 * self.n_adv + m, dt_last=1e-3, vmax=1.0) for m in range(self.n_members)]

        def history(self, drain=False):
            rows = np.array([[10.0 * self.n_adv + k, 0.02 * (self.n_adv - 1) + 0.005 * (k + 1), 0.005, 1.0, 0.1, 0.1, 0.5, 0.6]
                             for k in range(3)])
            return [capi.history_dict(rows) for _ in range(self.n_members)]

        def flow_stats_sums(self, band):
            one = np.ones(self.n_bins)
            return [dict(count=one.copy(), sum_ux=0.5 * one, sum_ux2=0.3 * one, sum_uy=0.0 * one, sum_uy2=0.01 * one, n_samples=4,
                         t_first=0.02, t_last=0.06) for _ in range(self.n_members)]

        def field_map_sums(self):
            self.calls.append(("field_map_sums",))
            out = []
            for m, p in enumerate(self.prms):
                y = np.linspace(0.0, p.DH, ny)
                u = np.repeat((p.gravity_g / (2.0 * p.nu) * y * (p.DH - y))[:, None], nx, axis=1) * (1.0 + 0.01 * m)
                u[ny // 2, nx - 1 - m] += 0.1                     # every member its own bump along x
                hit = np.ones((ny, nx), dtype=bool)
                hit[0, m] = False                                  # ... and its own node never sampled
                z = lambda a: np.where(hit, a, 0.0)
                out.append(dict(count=z(np.full((ny, nx), 2.0)), sum_w=z(np.full((ny, nx), 2.0)), sum_ux=z(2.0 * u),
                                sum_uy=z(np.full((ny, nx), 0.02)), sum_ux2=z(2.0 * u * u), sum_uy2=z(np.full((ny, nx), 2e-4)),
                                n_samples=2, t_first=0.03 + 0.001 * m, t_last=0.06))
            return out

        def info(self):
            return dict(rebuild_every=5, skin=0.1, forced_rebuilds=0, realignments=0)

        def monitor(self, m, tau=True):
            return 0.1, 0.1, 0.0

        def download(self, m, fields=()):
            return dict(pos=self.parts[m]["pos"], vel=self.parts[m]["vel"])

    return FakeBatch


def _names(b):
    return [c[0] for c in b.calls]


def test_run_ensemble_passes_the_field_keywords_on(cfgmod, capi, driver, profmod, monkeypatch):
    nx, ny = 12, 9
    Fake = _stand_in(capi, profmod, nx, ny)
    monkeypatch.setattr(driver.capi, "Batch", Fake)
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.06, output_interval=0.02) for _ in range(3)]
    res = driver.run_ensemble(prms, average_from=0.02, field_from=0.03, field_every=4, field_shape=(nx, ny), field_walls=True)
    b = Fake.made[-1]
    names = _names(b)
    assert ("field_map_enable", dict(nx=nx, ny=ny, every=4, t_from=0.03, with_walls=True)) in b.calls
    assert names.count("field_map_enable") == 1 and names.index("field_map_enable") < names.index("advance")
    assert names.count("field_map_sums") == 1 and names.index("field_map_sums") > len(names) - 1 - names[::-1].index("advance")
    planes = b.field_map_sums()
    for m, r in enumerate(res.members):
        ref = profmod.field_map_means(3.0, prms[m].DH, **planes[m])
        for k in ("u_x", "u_y", "count", "u_x_std"):
            assert np.array_equal(r.field_avg[k], ref[k], equal_nan=True), (m, k)
        assert np.isnan(r.field_avg["u_x"][0, m]) and r.field_avg["t_first"] == 0.03 + 0.001 * m
    pf = res.pooled_field
    assert res.pooled is not None and pf["n_members"] == 3 and pf["n_samples"] == 6 and pf["t_first"] == 0.03
    assert np.array_equal(pf["count"], sum(p["count"] for p in planes))
    assert np.isnan(pf["u_x_se"][0, :3]).all() and np.isfinite(pf["u_x_se"][1:]).all() and np.isfinite(pf["u_x"]).all()
    # the reference's shape by default, and fluid only
    driver.run_ensemble(prms, average_from=0.02, field_from=0.0)
    assert ("field_map_enable", dict(nx=0, ny=0, every=1, t_from=0.0, with_walls=False)) in Fake.made[-1].calls
    # members that differ in their physics: every member its map, nothing pooled
    sweep = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.06, output_interval=0.02) for mu in (0.1, 0.2)]
    res = driver.run_ensemble(sweep, average_from=0.02, field_from=0.03, field_shape=(nx, ny))
    assert res.pooled is None and res.pooled_field is None and all(r.field_avg is not None for r in res.members)
    # without field_from the batch is not asked for a map at all
    res = driver.run_ensemble(prms, average_from=0.02)
    assert not {"field_map_enable", "field_map_sums"} & set(_names(Fake.made[-1]))
    assert res.pooled_field is None and all(r.field_avg is None for r in res.members)
    assert driver.EnsembleResult(members=[], pooled=None, wall_seconds=0.0).pooled_field is None


def test_run_sweep_adds_the_field_columns(cfgmod, capi, driver, profmod, monkeypatch):
    nx, ny = 12, 9
    Fake = _stand_in(capi, profmod, nx, ny)
    monkeypatch.setattr(driver.capi, "Batch", Fake)
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.06, output_interval=0.02) for mu in (0.1, 0.15, 0.2)]
    res = driver.run_sweep(prms, field_from=0.03, field_every=2, field_shape=(nx, ny))
    b = Fake.made[-1]
    names = _names(b)
    assert ("field_map_enable", dict(nx=nx, ny=ny, every=2, t_from=0.03, with_walls=False)) in b.calls
    assert names.index("field_map_enable") < names.index("advance") and names.count("field_map_sums") == 1
    cols = {"field_L2": "L2", "field_x_spread": "x_spread", "field_ix": "ix", "field_uy_rms": "uy_rms"}
    for m, r in enumerate(res.members):
        fig = driver.field_figures(prms[m], r.field_avg)
        assert fig["ix"] == nx - 1 - m and fig["x_spread"] > 0                 # the member's own bump
        for col, k in cols.items():
            assert res.table[col].shape == (3,) and res.table[col][m] == fig[k], (m, col)
    assert set(driver.field_table(prms, [r.field_avg for r in res.members])) == set(cols)
    plain = driver.run_sweep(prms)
    assert not set(cols) & set(plain.table) and all(r.field_avg is None for r in plain.members)
    assert not {"field_map_enable", "field_map_sums"} & set(_names(Fake.made[-1]))
