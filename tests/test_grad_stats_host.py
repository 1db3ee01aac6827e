"""Gradient statistics (include/sphx.h sections 2n / 2o) without a GPU: profile.velocity_gradients -- the kernel's definition --
on linear fields (exact whatever the arrangement), on the lattice with the analytic parabola (exact away from the walls), its
counts against the flow statistics' bin rule, the skip rule on hand-built states, pooling, grad_figures on the analytic state,
the library's ten entry points and the config struct, the bindings' checks, the floating-point bound the GPU comparisons
use (tests/grad_stats_cases.py), and the drivers' keywords, followed through stand-ins for capi.Context and capi.Batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grad_stats_cases as gc
from helpers import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = tuple(f"sphx_{who}_grad_stats_{what}" for who in ("ctx", "batch") for what in ("enable", "disable", "reset", "sample", "read"))


@pytest.fixture(scope="module")
def anchor_states(cfgmod, geom):
    """name -> (prm, parts) of gc.ANCHOR, made once"""
    return {name: make_case(cfgmod, geom, dp=dp, DL=DL, jitter=jitter, seed=11, developed=True) for name, (dp, DL, jitter) in gc.ANCHOR.items()}


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.ANCHOR))
@pytest.mark.parametrize("walls", [False, True])
def test_linear_field_is_recovered(profmod, anchor_states, name, walls):
    prm, parts = anchor_states[name]
    lin, want = gc.linear_field(prm, parts)
    g = gc.gradients(profmod, prm, lin, lin, walls)
    err = float(np.max(np.abs(g["G"] - np.array(want))))
    print(f"{name} walls {walls}: linear field off by {err:.3e}, det M min {g['det'].min():.3f} median {np.median(g['det']):.3f}")
    assert err <= 1e-12 * max(abs(want[1]), abs(want[3]))
    assert np.all(g["det"] > 0.05)


# 2 ---------------------------------------------------------------------------------------------------------------
def test_linear_field_in_x_away_from_the_seam(profmod, anchor_states):
    prm, parts = anchor_states["jittered"]
    nf, c = parts["n_fluid"], 0.9
    pos = parts["pos"]
    vel = np.zeros_like(pos)
    vel[:, 1] = c * (pos[:, 0] - 0.5 * prm.DL)   # u_y = c (x - DL/2): jumps by c DL at the periodic seam
    state = dict(pos=pos, vel=vel)
    g = gc.gradients(profmod, prm, parts, state, False)["G"]
    near = profmod.in_band(pos[:nf, 0], prm.DL, 0.5 * prm.DL, 0.25 * prm.DL)   # the band (DL/2, DL/4): farther than 2h from the seam
    assert 0.25 * prm.DL > 2.0 * prm.h and near.sum() > nf // 3
    assert float(np.max(np.abs(g[near] - np.array([0.0, 0.0, c, 0.0])))) <= 1e-12 * c
    seam = profmod.in_band(pos[:nf, 0], prm.DL, 0.0, prm.h)
    assert float(np.max(np.abs(g[seam, 2] - c))) > 1.0                         # (the jump shows at the seam)
    sums = gc.numpy_sums(profmod, prm, parts, state, 20, [(0.5 * prm.DL, 0.25 * prm.DL)], dict(G=g, det=np.ones(nf)))
    prof = profmod.grad_stats_profiles(prm.DH, sums[1])
    assert np.allclose(prof["gyx_mean"], c, rtol=0, atol=1e-12 * c) and np.allclose(prof["vort_mean"], c, rtol=0, atol=1e-12 * c)


# 3 ---------------------------------------------------------------------------------------------------------------
def _parabola(prm, parts):
    nf = parts["n_fluid"]
    y = parts["pos"][:nf, 1]
    vel = np.zeros((parts["n_total"], 2))
    vel[:nf, 0] = prm.gravity_g / (2.0 * prm.nu) * y * (prm.DH - y)
    return dict(pos=parts["pos"], vel=vel)


def test_lattice_with_the_parabola(cfgmod, geom, profmod):
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=1.0, jitter=0.0, developed=False)
    state = _parabola(prm, parts)
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    sums = gc.numpy_sums(profmod, prm, parts, state, n_bins, [], gc.gradients(profmod, prm, parts, state, False))
    prof = profmod.grad_stats_profiles(prm.DH, sums[0])
    y = prof["y_mid"]
    exact = prm.gravity_g / (2.0 * prm.nu) * (prm.DH - 2.0 * y)
    inner = (y >= 2.0 * prm.h) & (y <= prm.DH - 2.0 * prm.h)
    assert inner.sum() >= n_bins - 6
    rel = np.abs(prof["gxy_mean"][inner] - exact[inner]) / np.max(np.abs(exact))
    print(f"lattice, parabola: interior shear off by {rel.max():.3e}; wall bin {prof['gxy_mean'][0]:.4f} against {exact[0]:.4f}")
    assert rel.max() <= 1e-12
    assert np.all(sums[0]["skipped"] == 0) and sums[0]["count"].sum() == parts["n_fluid"]
    assert 0.9 < prof["gxy_mean"][0] / exact[0] < 1.0      # one-sided support: first order, reads low


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.ANCHOR))
def test_count_plus_skipped_is_the_flow_statistics_count(profmod, anchor_states, name):
    prm, parts = anchor_states[name]
    nf = parts["n_fluid"]
    pos = parts["pos"].copy()
    pos[5, 1], pos[9, 1] = -1e-9, prm.DH + 1e-9   # two particles outside [0, DH]: dropped by both
    state = dict(pos=pos, vel=parts["vel"])
    xbands = gc.bands(prm)
    for n_bins in gc.BINS:
        # a det_min above the wall particles' det M skips some of them
        sums = gc.numpy_sums(profmod, prm, parts, state, n_bins, xbands, gc.gradients(profmod, prm, parts, state, False), det_min=0.6)
        edges = np.linspace(0.0, prm.DH, n_bins + 1)
        y = pos[:nf, 1]
        inside = (y >= edges[0]) & (y <= edges[-1])
        k = np.minimum(np.searchsorted(edges, y, side="right") - 1, n_bins - 1)
        for b, mine in enumerate([inside] + [inside & profmod.in_band(pos[:nf, 0], prm.DL, x, hw) for x, hw in xbands]):
            want = np.bincount(k[mine], minlength=n_bins)
            assert np.array_equal(sums[b]["count"] + sums[b]["skipped"], want), (name, n_bins, b)
        assert sums[0]["skipped"].sum() > 0 and sums[0]["count"].sum() > 0 and inside.sum() == nf - 2


# 5 ---------------------------------------------------------------------------------------------------------------
def test_skip_rule_on_hand_built_states(profmod):
    DL, DH, h = 2.0, 1.0, 0.065
    pos = np.array([[0.3, 0.5], [1.2, 0.5], [1.2 + 0.05, 0.52], [1.7, 0.2], [1.75, 0.2], [1.7, 0.25], [1.75, 0.26]])
    vel = np.array([[1.0, 0.0], [0.5, 0.1], [0.7, -0.1], [0.1, 0.0], [0.2, 0.0], [0.3, 0.1], [0.2, 0.2]])
    vol = np.full(len(pos), 0.05 ** 2)
    g = profmod.velocity_gradients(pos, vel, vol, DL, h)
    assert g["det"][0] == 0.0 and np.all(np.isnan(g["G"][0]))             # isolated: no partner
    assert abs(g["det"][1]) < 1e-12 and abs(g["det"][2]) < 1e-12            # a single partner: M has rank one
    assert np.all(g["det"][3:] > 1e-3) and np.all(np.isfinite(g["G"][3:]))   # (three partners each: a thin support)
    (s,) = profmod.grad_stats_sums(pos, vel, vol, DL, DH, h, 4, det_min=1e-3, vmax=1.0)
    assert s["skipped"].tolist() == [0.0, 0.0, 3.0, 0.0] and s["count"].tolist() == [2.0, 2.0, 0.0, 0.0]
    assert all(np.all(np.isfinite(s[f])) for f in gc.FIELDS) and all(s[f][2] == 0.0 for f in gc.SUMMED)
    (s,) = profmod.grad_stats_sums(pos, vel, vol, DL, DH, h, 4, det_min=1e-3, vmax=1e-6)   # a bound below every estimate
    assert s["skipped"].sum() == 7 and s["count"].sum() == 0
    prof = profmod.grad_stats_profiles(DH, s)
    assert np.all(np.isnan(prof["gxy_mean"])) and np.all(np.isnan(prof["div_rms"]))


# 6 ---------------------------------------------------------------------------------------------------------------
def test_profiles_and_pooling(profmod):
    DH, n = 1.0, 6

    def sums(seed, empty=()):
        r = np.random.default_rng(seed)
        cnt = r.integers(1, 9, n).astype(np.float64)
        cnt[list(empty)] = 0.0
        d = {f: r.standard_normal(n) * cnt for f in gc.SUMMED}
        for f in gc.FIELDS[5:11]:
            d[f] = np.abs(d[f]) + 4.0 * cnt
        d.update(count=cnt, skipped=r.integers(0, 3, n).astype(np.float64), n_samples=int(seed), t_first=0.1 * seed, t_last=1.0 + seed)
        return d

    a, b = sums(1, empty=(2,)), sums(2)
    pa = profmod.grad_stats_profiles(DH, a)
    ok = a["count"] > 0
    assert np.array_equal(np.isnan(pa["gxy_mean"]), ~ok) and np.array_equal(np.isnan(pa["vort_rms"]), ~ok)
    assert np.array_equal(pa["gxy_mean"][ok], a["sum_gxy"][ok] / a["count"][ok])
    assert np.array_equal(pa["vort_mean"][ok], (a["sum_gyx"][ok] - a["sum_gxy"][ok]) / a["count"][ok])
    assert np.array_equal(pa["div_rms"][ok], np.sqrt(a["sum_div2"][ok] / a["count"][ok]))
    m = a["sum_gyy"][ok] / a["count"][ok]
    assert np.array_equal(pa["gyy_std"][ok], np.sqrt(np.maximum(a["sum_gyy2"][ok] / a["count"][ok] - m * m, 0.0)))
    edges = np.linspace(0.0, DH, n + 1)
    assert np.array_equal(pa["y_mid"], 0.5 * (edges[:-1] + edges[1:])) and (pa["n_samples"], pa["t_last"]) == (1, 2.0)
    pooled = profmod.pool_grad_stats(DH, [a, b])
    for f in gc.FIELDS:
        assert np.array_equal(pooled[f], a[f] + b[f]), f              # pooled sums are the sums
    assert (pooled["n_samples"], pooled["t_first"], pooled["t_last"], pooled["n_members"]) == (3, 0.1, 3.0, 2)
    both = profmod.grad_stats_profiles(DH, {f: a[f] + b[f] for f in gc.FIELDS})
    assert np.array_equal(pooled["gxy_mean"], both["gxy_mean"]) and np.array_equal(pooled["div_rms"], both["div_rms"])
    one = profmod.pool_grad_stats(DH, [a])
    assert np.array_equal(one["gxx_std"], pa["gxx_std"], equal_nan=True)
    with pytest.raises(ValueError):
        profmod.pool_grad_stats(DH, [])


# 7 ---------------------------------------------------------------------------------------------------------------
def test_figures_on_the_analytic_state(cfgmod, geom, profmod, driver):
    """The lattice with the analytic parabola.  The sums are the device's: every particle's terms on the sample's fixed-point
    grid (quantise=True), where the 1e-16 that the symmetric lattice leaves in g_xx is the exact zero the device records."""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=1.0, jitter=0.0, developed=False)
    state = _parabola(prm, parts)
    nf = parts["n_fluid"]
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    gs = profmod.grad_stats_sums(state["pos"][:nf], state["vel"][:nf], parts["mass"][:nf] / prm.rho0, prm.DL, prm.DH, prm.h, n_bins,
                                 bands=[(0.5 * prm.DL, prm.h)], quantise=True)
    fig = driver.grad_figures(prm, gs)
    target = prm.gravity_g * prm.rho0 * prm.DH / 2
    assert fig["tau_target"] == target and target > 0
    # The line is fitted to the bins at least 2h from a wall and read at the walls.  A least-squares prediction at x0 is a
    # weighted sum of the fitted values with weights 1/n + (x0 - xm)(x_i - xm) / Sxx, whose absolute sum over uniform x on
    # [2h, DH - 2h] is below 1 + 0.5 DH * 1.5 / (DH/2 - 2h) = 3.03 at DH = 1, h = 0.065: an error of at most `residual` in
    # every fitted value moves the wall value by less than 4 residuals; 16 eps of the target for the fit's own arithmetic.
    allowed = 4.0 * fig["tau_fit_residual"] + 16 * np.finfo(float).eps * target
    print(f"tau_wall {fig['tau_wall_bottom']!r} {fig['tau_wall_top']!r} target {target!r} residual {fig['tau_fit_residual']:.3e}")
    assert abs(fig["tau_wall_bottom"] - target) <= allowed and abs(fig["tau_wall_top"] - target) <= allowed
    assert fig["div_rms"] == 0.0
    assert fig["L2_shear"] <= 1e-12 and 1e-3 < fig["L2_shear_all"] < 0.05 and abs(fig["vort_mean"]) <= 1e-12 * abs(fig["shear_exact"][0])
    assert np.array_equal(fig["tau"], prm.mu * fig["shear"]) and fig["shear_exact"][0] > 0 > fig["shear_exact"][-1]
    left = cfgmod.params_from_values(dp=0.05, DL=1.0, U_bulk=-0.666667)
    assert left.gravity_g < 0 and driver.grad_figures(left, gs)["shear_exact"][0] < 0   # the sign follows the body force
    mid = driver.grad_figures(prm, gs, band=1)
    assert mid["L2_shear"] <= 1e-12 and mid["div_rms"] == 0.0
    with pytest.raises(ValueError, match="gradients_from needs the resident engine"):
        driver.run(prm, engine="mex", gradients_from=0.0)


# 8 ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert len(SYMBOLS) == 10
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert not any("slab" in n and "grad" in n for n in declared)  # slab rings are a follow-up
    assert re.search(r"^#define SPHX_GRAD_STATS_FIELDS 12\s*$", hdr, re.M) and len(gc.FIELDS) == 12
    assert re.search(r"^#define SPHX_GRAD_STATS_MAX_BINS 640\s*$", hdr, re.M)
    assert "2n. Gradient statistics" in raw and "2o. Gradient statistics of a batch" in raw


def test_config_struct_matches_the_header(capi, profmod):
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_grad_stats_config \{(.*?)\} sphx_grad_stats_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for t, names in re.findall(r"(int32_t|double)\s*([\w\s,\[\]]+);", body):
        members += [(t, n.strip()) for n in names.split(",")]
    assert members == [("int32_t", "n_bins"), ("int32_t", "every"), ("double", "t_from"), ("double", "det_min"), ("int32_t", "with_walls"),
                       ("int32_t", "n_bands"), ("double", "band_x[2]"), ("double", "band_hw[2]")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    want = [(n.split("[")[0], ctype[t] * 2 if "[" in n else ctype[t]) for t, n in members]
    assert want == list(capi.SphxGradStatsConfig._fields_)
    S = capi.SphxGradStatsConfig
    assert (C.sizeof(S), S.t_from.offset, S.det_min.offset, S.with_walls.offset, S.n_bands.offset, S.band_x.offset, S.band_hw.offset) == \
        (64, 8, 16, 24, 28, 32, 48)
    assert profmod.GRAD_FIELDS == gc.FIELDS and profmod.GRAD_MAX_BINS == 640


def test_null_handles_are_refused(capi):
    L = capi.lib()
    cfg = capi.SphxGradStatsConfig(n_bins=8, every=1, det_min=0.05)
    nothing = (None,) * 5
    for who, ident in (("ctx", "SPHX:Ctx:null"), ("batch", "SPHX:Batch:null")):
        calls = {"enable": (C.byref(cfg),), "disable": (), "reset": (), "sample": (), "read": (0, 0, *nothing)}
        for what, args in calls.items():
            rc = getattr(L, f"sphx_{who}_grad_stats_{what}")(None, *args)
            assert rc == capi.SPHX_ERR_ARG and L.sphx_last_error_id().decode() == ident, (who, what)


@pytest.mark.parametrize("kw", [dict(n_bins=-1), dict(n_bins=2.5), dict(every=0), dict(t_from=float("nan")), dict(det_min=-0.1),
                                dict(det_min=float("inf")), dict(det_min="x"), dict(with_walls=2), dict(bands=[(0.5, 0.1)] * 3),
                                dict(bands=[(0.5, -0.1)]), dict(n_bins=641), dict(n_bins=321, bands=[(0.5, 0.1)]),
                                dict(n_bins=214, bands=[(0.5, 0.1), (0.0, 0.1)])])
def test_binding_checks_the_config_first(cfgmod, capi, kw):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0)
    with pytest.raises(capi.SphxError) as e:
        capi.grad_stats_config(prm, **kw)
    assert e.value.identifier == "SPHX:GradStats:config" and e.value.code == capi.SPHX_ERR_ARG


def test_binding_accepts_the_limits(cfgmod, capi):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0)
    cfg = capi.grad_stats_config(prm, n_bins=213, bands=[(0.5, 0.1), (0.0, 0.1)], det_min=0.0, with_walls=True)   # 639 <= 640
    assert (cfg.n_bins, cfg.n_bands, cfg.with_walls, cfg.det_min, cfg.band_x[1], cfg.band_hw[0]) == (213, 2, 1, 0.0, 0.0, 0.1)
    cfg = capi.grad_stats_config(prm)
    assert (cfg.n_bins, cfg.every, cfg.t_from, cfg.det_min, cfg.with_walls, cfg.n_bands) == (0, 1, 0.0, 0.05, 0, 0)
    assert capi.grad_stats_config(prm, n_bins=640).n_bins == 640


# 9 ---------------------------------------------------------------------------------------------------------------
def test_floating_point_bound(cfgmod, geom, profmod):
    """The rounding error of the reference's own sums: float64 against np.longdouble in reversed partner order, on the states of
    gc.CASES as they are uploaded.  The GPU tests compare with numpy's sums seven steps later, on nearly the same arrangements
    and velocities; no CPU test can hold those states.  A case that starts at rest (one_col) has only zero sums as uploaded, so
    its arrangement is measured with the analytic parabola on it.  (The linear field and the lattice at rest are compared with
    their exact values.)  gc.FP_DEVIATION must cover every case."""
    import probe_cases
    worst = (0.0, None, None, None)
    states = {name: probe_cases.case(make_case, cfgmod, geom, name)[:2] for name in gc.CASES}
    for name, (prm, parts) in states.items():
        n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
        at_rest = not np.any(parts["vel"][:parts["n_fluid"]])
        state = _parabola(prm, parts) if at_rest else parts
        for walls in (False, True):
            a = gc.numpy_sums(profmod, prm, parts, state, n_bins, gc.bands(prm), gc.gradients(profmod, prm, parts, state, walls))
            b = gc.numpy_sums(profmod, prm, parts, state, n_bins, gc.bands(prm),
                              gc.gradients(profmod, prm, parts, state, walls, acc=np.longdouble, reverse=True))
            for f in gc.COUNTS:
                assert all(np.array_equal(x[f], y[f]) for x, y in zip(a, b)), (name, walls, f)
            dev, f, band = gc.deviation(a, b)
            print(f"{name} walls {walls}{' (at rest: the parabola)' if at_rest else ''}: float64 against longdouble reversed: "
                  f"{dev:.3e} ({f}, band {band})")
            assert 0.0 < dev <= gc.FP_DEVIATION, (name, walls)      # every case contributes a figure
            worst = max(worst, (dev, name, walls, f), key=lambda w: w[0])
    print(f"worst {worst}")
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    assert 0.0 < worst[0] <= gc.FP_DEVIATION and gc.BOUND == max(16 * gc.FP_DEVIATION, 1e-12) == 1e-12


# 10 --------------------------------------------------------------------------------------------------------------
def _fake_sums(prm, member, band, n_bins):
    """gradient sums with known values: the analytic shear in every bin, scaled by member and band"""
    edges = np.linspace(0.0, prm.DH, n_bins + 1)
    y = 0.5 * (edges[:-1] + edges[1:])
    cnt = np.full(n_bins, 10.0 * (band + 1))
    shear = prm.gravity_g / (2.0 * prm.nu) * (prm.DH - 2.0 * y) * (1.0 + 0.01 * member)
    d = {f: np.zeros(n_bins) for f in gc.FIELDS}
    d.update(count=cnt, sum_gxy=shear * cnt, sum_gxy2=shear * shear * cnt, sum_div2=1e-4 * cnt, n_samples=5 + member, t_first=0.03, t_last=0.06)
    return d


def _stand_ins(capi):
    """Stand-ins for capi.Context and capi.Batch: no device, the calls a driver makes recorded in order."""

    class Fake:
        made = []

        def __init__(self, prms, parts_list, launch, many):
            self.prms, self.parts, self.calls, self.n_adv, self.many = list(prms), list(parts_list), [], 0, many
            self.n_members = len(self.prms)
            Fake.made.append(self)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.close()

        def close(self):
            self.calls.append(("close",))

        def _each(self, v):
            return v if self.many else v[0]

        def grad_stats_enable(self, **kw):
            self.calls.append(("grad_stats_enable", kw))
            self.grad = (kw["n_bins"], len(kw["bands"]) + 1)

        def grad_stats_sums(self, band=0):
            self.calls.append(("grad_stats_sums", band))
            assert 0 <= band < self.grad[1]
            return self._each([_fake_sums(p, m, band, self.grad[0]) for m, p in enumerate(self.prms)])

        def flow_stats_enable(self, **kw):
            self.n_bins = kw["n_bins"]

        def flow_stats_sums(self, band):
            one = np.ones(self.n_bins)
            return [dict(count=one.copy(), sum_ux=0.5 * one, sum_ux2=0.3 * one, sum_uy=0.0 * one, sum_uy2=0.01 * one, n_samples=4,
                         t_first=0.02, t_last=0.06) for _ in range(self.n_members)]

        def history_enable(self, **kw):
            pass

        def history(self, drain=False):
            rows = np.array([[10.0 * self.n_adv + k, 0.02 * (self.n_adv - 1) + 0.005 * (k + 1), 0.005, 1.0, 0.1, 0.1, 0.5, 0.6] for k in range(3)])
            return [capi.history_dict(rows) for _ in range(self.n_members)]

        def substeps(self):
            return 1

        def grid_policy(self):
            return dict(rebuild_every=5, skin=0.1)

        def info(self):
            return dict(rebuild_every=5, skin=0.1, forced_rebuilds=0, realignments=0)

        def advance(self, target, max_steps=0):
            self.n_adv += 1
            self.calls.append(("advance", target))
            return self._each([dict(t=target, step=10 * self.n_adv + m, dt_last=1e-3, vmax=1.0) for m in range(self.n_members)])

        def monitor(self, *m, tau=True):
            return 0.1, 0.1, 0.0

        def download(self, *m, fields=()):
            p = self.parts[m[0] if m else 0]
            return dict(pos=p["pos"], vel=p["vel"])

    class FakeContext(Fake):
        @classmethod
        def from_parts(cls, prm, parts, **kw):
            return cls([prm], [parts], kw, False)

    class FakeBatch(Fake):
        @classmethod
        def from_parts(cls, prms, parts_list, **kw):
            return cls(prms, parts_list, kw, True)

    return Fake, FakeContext, FakeBatch


def test_the_drivers_pass_the_gradient_keywords_on(cfgmod, capi, driver, profmod, monkeypatch):
    Fake, FakeContext, FakeBatch = _stand_ins(capi)
    monkeypatch.setattr(driver.capi, "Context", FakeContext)
    monkeypatch.setattr(driver.capi, "Batch", FakeBatch)
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.06, output_interval=0.02)
    mid = [(0.5 * prm.DL, max(prm.dp, prm.h))]
    res = driver.run(prm, gradients_from=0.03, gradients_every=4, gradients_walls=True)
    ctx = Fake.made[-1]
    names = [c[0] for c in ctx.calls]
    assert ("grad_stats_enable", dict(n_bins=20, every=4, t_from=0.03, with_walls=True, bands=mid)) in ctx.calls   # band 1: mid-channel
    assert names.count("grad_stats_enable") == 1 and names.index("grad_stats_enable") < names.index("advance")
    assert [c for c in ctx.calls if c[0] == "grad_stats_sums"] == [("grad_stats_sums", 0), ("grad_stats_sums", 1)]
    assert len(res.grad_stats) == 2 and res.grad_stats[1]["count"][0] == 20.0
    assert np.array_equal(res.grad_stats[0]["gxy_mean"], profmod.grad_stats_profiles(prm.DH, _fake_sums(prm, 0, 0, 20))["gxy_mean"])
    fig = driver.grad_figures(prm, res.grad_stats)
    assert fig["L2_shear"] <= 1e-14 and abs(fig["tau_wall_bottom"] - fig["tau_target"]) <= 1e-12 * fig["tau_target"]
    driver.run(prm, gradients_from=0.0, gradients_bands=[(1.0, 0.2), (0.0, 0.1)])    # the defaults: every step, walls off
    assert ("grad_stats_enable", dict(n_bins=20, every=1, t_from=0.0, with_walls=False, bands=[(1.0, 0.2), (0.0, 0.1)])) in Fake.made[-1].calls
    res = driver.run(prm)                                                          # off by default: the context is not asked at all
    assert res.grad_stats is None and not {"grad_stats_enable", "grad_stats_sums"} & {c[0] for c in Fake.made[-1].calls}
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.06, output_interval=0.02) for mu in (0.1, 0.1, 0.1)]
    sweep = driver.run_sweep(prms, gradients_from=0.02, gradients_every=2)
    assert ("grad_stats_enable", dict(n_bins=20, every=2, t_from=0.02, with_walls=False, bands=mid)) in Fake.made[-1].calls
    for k in ("L2_shear", "tau_wall_dev", "div_rms"):
        assert sweep.table[k].shape == (3,), k
    assert np.allclose(sweep.table["L2_shear"], [0.0, 0.01, 0.02], atol=1e-12) and all(len(r.grad_stats) == 2 for r in sweep.members)
    assert not {"L2_shear", "tau_wall_dev", "div_rms"} & set(driver.run_sweep(prms).table)
    ens = driver.run_ensemble(prms, average_from=0.02, gradients_from=0.02)
    assert len(ens.pooled_grad) == 2 and ens.pooled_grad[0]["n_members"] == 3 and ens.pooled_grad[0]["n_samples"] == 5 + 6 + 7
    assert np.array_equal(ens.pooled_grad[1]["count"], 3 * _fake_sums(prms[0], 0, 1, 20)["count"])
    assert driver.run_ensemble(prms, average_from=0.02).pooled_grad is None
