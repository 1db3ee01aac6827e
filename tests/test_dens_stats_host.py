"""Density statistics (include/sphx.h sections 2r / 2s) without a GPU: profile.summation_density -- the kernel's definition --
against the oracle's density_correction, the lattice at rest, the binning identities against the flow statistics' bin rule, the
fixed-point grid, profiles, pooling and density_figures on hand-made sums, the library's ten entry points and the config
struct, the bindings' checks, the floating-point bound and the edge premise the GPU comparisons use (tests/dens_stats_cases.py),
and the drivers' keywords, followed through stand-ins for capi.Context and capi.Batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dens_stats_cases as dc
import probe_cases
from helpers import make_case, make_variant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = tuple(f"sphx_{who}_dens_stats_{what}" for who in ("ctx", "batch") for what in ("enable", "disable", "reset", "sample", "read"))


@pytest.fixture(scope="module")
def anchor_states(cfgmod, geom):
    """name -> (prm, parts) of dc.ANCHOR, made once"""
    return {name: make_case(cfgmod, geom, dp=dp, DL=DL, jitter=jitter, seed=11, developed=True) for name, (dp, DL, jitter) in dc.ANCHOR.items()}


@pytest.fixture(scope="module")
def lattice(cfgmod, geom, profmod):
    """the lattice at rest, dp = 0.05, DL = 3: (prm, parts, (rho, wall))"""
    prm, parts = make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.0, developed=False)
    return prm, parts, dc.density(profmod, prm, parts, parts["pos"])


# 1 ---------------------------------------------------------------------------------------------------------------
def test_summation_density_is_the_oracles(cfgmod, geom, profmod, oracle, anchor_states):
    states = dict(anchor_states, variant=make_variant(cfgmod, geom, seed=11), dp025=make_case(cfgmod, geom, dp=0.025, DL=1.5, seed=11))
    worst = 0.0
    for name, (prm, parts) in states.items():
        nf, nt = parts["n_fluid"], parts["n_total"]
        nb = oracle.neighbor_search(parts["pos"], nf, nt, prm.h, prm.DL)
        rho, _, _ = oracle.density_correction(nb, parts["mass"], nf, nt, prm.rho0, prm.h, prm.inv_sigma0)
        got, wall = dc.density(profmod, prm, parts, parts["pos"])
        err = float(np.max(np.abs(got - rho[:nf]))) / prm.rho0
        d = got / prm.rho0 - 1.0
        print(f"{name}: summation density off by {err:.3e} rho0; delta {d.min():.4f} .. {d.max():.4f} rms {np.sqrt(np.mean(d * d)):.4f}; "
              f"wall share up to {wall.max():.3f}")
        assert err <= 1e-13, name
        assert np.all(wall >= 0.0) and np.all(wall < got / prm.rho0) and wall.max() > 0.2
        worst = max(worst, err)
    print(f"worst {worst:.3e}")


# 2 ---------------------------------------------------------------------------------------------------------------
def test_lattice_at_rest(profmod, lattice):
    prm, parts, dens = lattice
    nf = parts["n_fluid"]
    delta = dens[0] / prm.rho0 - 1.0
    assert nf == 1200 and np.all(np.abs(delta - dc.LATTICE_DELTA) <= 1e-13)   # the wall rows too: the walls continue the lattice
    n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
    for n_hist, hist_range in dc.HIST:
        (s,) = dc.numpy_sums(profmod, prm, parts, parts["pos"], n_bins, [], dens, n_hist=n_hist, hist_range=hist_range)
        assert s["d_max"].max() - s["d_min"].min() <= 1e-13 and np.all(s["d_min"] <= s["d_max"])
        assert s["hist"][31] == 1200 and s["hist"].sum() == 1200 and (s["below"], s["above"]) == (0, 0)
        assert s["count"].sum() == 1200 and s["outliers"].sum() == 0
    # the walls' share: non-zero exactly in the bins that hold a particle within 2h of a wall particle
    y, yw = parts["pos"][:nf, 1], parts["pos"][nf:, 1]
    edges = np.linspace(0.0, prm.DH, n_bins + 1)
    k = np.minimum(np.searchsorted(edges, y, side="right") - 1, n_bins - 1)
    near = np.min(np.abs(y[:, None] - yw[None, :]), axis=1) < 2.0 * prm.h
    want = np.bincount(k[near], minlength=n_bins) > 0
    assert np.array_equal(s["sum_wall"] != 0.0, want) and 0 < want.sum() < n_bins
    prof = profmod.dens_stats_profiles(prm.DH, prm.p0, s, hist_range=dc.HIST[1][1])
    assert np.allclose(prof["d_mean"], dc.LATTICE_DELTA, rtol=0, atol=1e-13) and np.all(prof["d_std"] <= 1e-7)
    assert 0.2 < prof["wall_mean"][0] < 0.25 and np.allclose(prof["packing"], 1.0 / (1.0 + dc.LATTICE_DELTA), rtol=0, atol=1e-12)


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.ANCHOR))
def test_binning_identities(profmod, anchor_states, name):
    prm, parts = anchor_states[name]
    nf = parts["n_fluid"]
    pos = parts["pos"].copy()
    pos[5, 1], pos[9, 1] = -1e-9, prm.DH + 1e-9   # two particles outside [0, DH]: dropped by both
    dens = dc.density(profmod, prm, parts, pos)
    xbands = dc.bands(prm)
    for n_bins in dc.BINS:
        # a delta_bound inside the jittered states' range makes some particles outliers
        sums = dc.numpy_sums(profmod, prm, parts, pos, n_bins, xbands, dens, hist_range=0.02, delta_bound=0.04)
        edges = np.linspace(0.0, prm.DH, n_bins + 1)
        y = pos[:nf, 1]
        inside = (y >= edges[0]) & (y <= edges[-1])
        k = np.minimum(np.searchsorted(edges, y, side="right") - 1, n_bins - 1)
        for b, mine in enumerate([inside] + [inside & profmod.in_band(pos[:nf, 0], prm.DL, x, hw) for x, hw in xbands]):
            want = np.bincount(k[mine], minlength=n_bins)
            assert np.array_equal(sums[b]["count"] + sums[b]["outliers"], want), (name, n_bins, b)
            assert sums[b]["hist"].sum() + sums[b]["below"] + sums[b]["above"] == sums[b]["count"].sum(), (name, n_bins, b)
        assert inside.sum() == nf - 2
        if name != "lattice":
            assert sums[0]["outliers"].sum() > 0 and sums[0]["count"].sum() > 0 and sums[0]["below"] > 0 and sums[0]["above"] > 0


def test_outlier_rule_on_hand_built_values(profmod):
    DL, DH, h, rho0 = 2.0, 1.0, 0.065, 1.0
    pos = np.column_stack([np.linspace(0.1, 1.9, 8), np.full(8, 0.55)])
    rho = rho0 * (1.0 + np.array([0.0, 0.5, 0.5000001, -0.5, -0.6, np.nan, np.inf, 0.0499999]))
    (s,) = profmod.dens_stats_sums(pos, 1.0, DL, DH, h, rho0, 1.0, 2, density=(rho, np.zeros(8)))
    assert s["count"].tolist() == [0.0, 4.0] and s["outliers"].tolist() == [0.0, 4.0]
    assert (s["d_min"][1], s["d_max"][1]) == (-0.5, 0.5) and np.isinf(s["d_min"][0]) and np.isinf(s["d_max"][0])
    assert s["hist"].sum() == 2 and (s["below"], s["above"]) == (1, 1) and s["hist"][32] == 1 and s["hist"][63] == 1
    # (delta comes back out of rho0 (1 + delta): off by up to an eps of 1 per particle)
    assert np.isfinite(s["sum_d"]).all() and abs(s["sum_d"][1] - 0.0499999) <= 4 * np.finfo(float).eps


# 4 ---------------------------------------------------------------------------------------------------------------
def test_scales_and_the_fixed_point_grid(profmod, anchor_states):
    sc = profmod.dens_scales(0.5, 1200)       # L = 11, e = -1
    assert sc == dict(s_d=52, s_d2=53, s_dvol=51, s_wall=50, e=-1)
    assert profmod.dens_scales(0.25, 1024) == dict(s_d=54, s_d2=56, s_dvol=53, s_wall=51, e=-2)   # L = 10, a power of two is its own bound
    assert profmod.dens_scales(0.3, 1025)["e"] == -1 and profmod.dens_scales(0.04, 1)["e"] == -4
    for db in (0.5, 0.3, 0.25, 0.04, 1e-3):
        e = profmod.dens_scales(db, 7)["e"]
        assert 2.0 ** e >= db > 2.0 ** (e - 1) and e <= -1
    prm, parts = anchor_states["jittered"]
    nf = parts["n_fluid"]
    dens = dc.density(profmod, prm, parts, parts["pos"])
    plain = dc.numpy_sums(profmod, prm, parts, parts["pos"], 20, dc.bands(prm), dens)
    grid = dc.numpy_sums(profmod, prm, parts, parts["pos"], 20, dc.bands(prm), dens, quantise=True)
    sc = profmod.dens_scales(0.5, nf)
    quant = dc.quantisation(plain, sc)
    for band, (a, b, q) in enumerate(zip(grid, plain, quant)):
        for f in dc.COUNTS + dc.EXTREMES:
            assert np.array_equal(a[f], b[f])
        assert np.array_equal(a["hist"], b["hist"])
        for f in dc.SUMMED:
            s = sc[dc.SCALE_OF[f]]
            assert np.all(np.ldexp(a[f], s) == np.rint(np.ldexp(a[f], s))), (band, f)    # on the grid of its own scale
            assert np.all(np.abs(a[f] - b[f]) <= q[f] + 1e-15 * np.abs(b[f])), (band, f)   # and within the quantisation term
    # the overflow argument: no term exceeds 2^(62 - L) in units of its scale
    rho, wall = dens
    d = rho / prm.rho0 - 1.0
    top = 2.0 ** (62 - 11)
    assert np.all(np.abs(np.ldexp(d, sc["s_d"])) <= top) and np.all(np.ldexp(d * d, sc["s_d2"]) <= top)
    assert np.all(np.abs(np.ldexp(prm.rho0 / rho - 1.0, sc["s_dvol"])) <= top) and np.all(np.ldexp(wall, sc["s_wall"]) <= top)


# 5 ---------------------------------------------------------------------------------------------------------------
def _hand_sums(seed, n=6, n_hist=8, empty=()):
    r = np.random.default_rng(seed)
    cnt = r.integers(1, 9, n).astype(np.float64)
    cnt[list(empty)] = 0.0
    mean = 0.02 * r.standard_normal(n)
    d = dict(count=cnt, sum_d=mean * cnt, sum_d2=(mean * mean + 1e-4) * cnt, sum_dvol=-mean * cnt, sum_wall=0.1 * cnt,
             outliers=r.integers(0, 3, n).astype(np.float64), d_min=np.where(cnt > 0, mean - 0.03, np.inf),
             d_max=np.where(cnt > 0, mean + 0.03, -np.inf), hist=r.integers(0, 5, n_hist).astype(np.int64), below=int(seed), above=2,
             hist_range=0.04, n_samples=int(seed), t_first=0.1 * seed, t_last=1.0 + seed)
    return d


def test_profiles_and_pooling(profmod):
    DH, p0 = 1.0, 250.0
    a, b = _hand_sums(1, empty=(2,)), _hand_sums(2)
    pa = profmod.dens_stats_profiles(DH, p0, a)
    ok = a["count"] > 0
    for k in ("d_mean", "d_std", "d_min", "d_max", "p_mean", "p_std", "wall_mean", "packing"):
        assert np.array_equal(np.isnan(pa[k]), ~ok), k
    m = a["sum_d"][ok] / a["count"][ok]
    sd = np.sqrt(np.maximum(a["sum_d2"][ok] / a["count"][ok] - m * m, 0.0))
    assert np.array_equal(pa["d_mean"][ok], m) and np.array_equal(pa["d_std"][ok], sd)
    assert np.array_equal(pa["p_mean"][ok], p0 * m) and np.array_equal(pa["p_std"][ok], p0 * sd)
    assert np.array_equal(pa["packing"][ok], 1.0 + a["sum_dvol"][ok] / a["count"][ok])
    assert np.array_equal(pa["wall_mean"][ok], a["sum_wall"][ok] / a["count"][ok]) and np.array_equal(pa["d_min"][ok], a["d_min"][ok])
    edges = np.linspace(0.0, DH, 7)
    assert np.array_equal(pa["y_mid"], 0.5 * (edges[:-1] + edges[1:])) and (pa["n_samples"], pa["t_last"]) == (1, 2.0)
    total = a["hist"].sum() + a["below"] + a["above"]
    assert np.allclose(pa["hist_density"], a["hist"] / (total * 0.01), rtol=1e-15) and np.allclose(pa["hist_centres"], -0.035 + 0.01 * np.arange(8))
    assert abs(pa["hist_density"].sum() * 0.01 - a["hist"].sum() / total) < 1e-15
    pooled = profmod.pool_dens_stats(DH, p0, [a, b])
    for f in dc.COUNTS + dc.SUMMED:
        assert np.array_equal(pooled[f], a[f] + b[f]), f
    assert np.array_equal(pooled["d_min"], np.minimum(a["d_min"], b["d_min"])) and np.array_equal(pooled["d_max"], np.maximum(a["d_max"], b["d_max"]))
    assert np.array_equal(pooled["hist"], a["hist"] + b["hist"]) and (pooled["below"], pooled["above"]) == (3, 4)
    assert (pooled["n_samples"], pooled["t_first"], pooled["t_last"], pooled["n_members"]) == (3, 0.1, 3.0, 2)
    both = profmod.dens_stats_profiles(DH, p0, profmod.add_dens_stats(a, b), hist_range=0.04)
    assert np.array_equal(pooled["d_mean"], both["d_mean"]) and np.array_equal(pooled["hist_density"], both["hist_density"])
    one = profmod.pool_dens_stats(DH, p0, [a])
    assert np.array_equal(one["d_std"], pa["d_std"], equal_nan=True) and np.array_equal(one["hist"], a["hist"])
    with pytest.raises(ValueError):
        profmod.pool_dens_stats(DH, p0, [])


def test_figures_on_hand_made_sums(cfgmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0)
    n = 20
    edges = np.linspace(0.0, prm.DH, n + 1)
    y = 0.5 * (edges[:-1] + edges[1:])
    inner = (y >= 2.0 * prm.h) & (y <= prm.DH - 2.0 * prm.h)
    assert inner.sum() == 14
    cnt = np.full(n, 10.0)
    mean = np.where(inner, 0.001 + 0.002 * (np.arange(n) == 7), 0.004)   # interior 0.001, one bin 0.003; wall bins 0.004
    s = dict(count=cnt, sum_d=mean * cnt, sum_d2=(mean * mean + 1e-6) * cnt, sum_dvol=-mean * cnt, sum_wall=np.where(inner, 0.0, 2.0),
             outliers=np.r_[3.0, np.zeros(n - 1)], d_min=mean - 0.01, d_max=mean + 0.02, hist=np.zeros(4, dtype=np.int64), below=0, above=0)
    fig = driver.density_figures(prm, [s])
    u_max = prm.gravity_g * prm.DH ** 2 / (8.0 * prm.nu)
    assert fig["ma2"] == u_max * u_max * prm.rho0 / prm.p0 and 0 < fig["ma2"] < 0.02
    assert np.isclose(fig["delta_mean"], mean.mean(), rtol=1e-14) and np.isclose(fig["delta_rms"], np.sqrt(np.mean(mean * mean + 1e-6)), rtol=1e-14)
    assert np.isclose(fig["delta_max"], 0.024, rtol=1e-14) and fig["outliers"] == 3
    assert np.isclose(fig["p_spread"], prm.p0 * 0.002 / (prm.rho0 * u_max * u_max), rtol=1e-12)
    assert np.isclose(fig["wall_bias"], 0.004 - (0.001 * 13 + 0.003) / 14, rtol=1e-12)
    assert np.isclose(fig["packing"], 1.0 - mean.mean(), rtol=1e-14)
    empty = dict(s, count=np.zeros(n), d_min=np.full(n, np.inf), d_max=np.full(n, -np.inf))
    fe = driver.density_figures(prm, [s, empty], band=1)
    assert all(np.isnan(fe[k]) for k in ("delta_rms", "delta_mean", "delta_max", "p_spread", "wall_bias", "packing"))
    with pytest.raises(ValueError, match="density_from needs the resident engine"):
        driver.run(prm, engine="mex", density_from=0.0)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert len(SYMBOLS) == 10
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert not any("slab" in n and "dens" in n for n in declared)  # slab rings are a follow-up
    assert re.search(r"^#define SPHX_DENS_STATS_FIELDS 8\s*$", hdr, re.M) and len(dc.FIELDS) == 8
    assert re.search(r"^#define SPHX_DENS_STATS_MAX_HIST 1024\s*$", hdr, re.M)
    assert "2r. Density statistics" in raw and "2s. Density statistics of a batch" in raw


def test_config_struct_matches_the_header(capi, profmod):
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_dens_stats_config \{(.*?)\} sphx_dens_stats_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for t, names in re.findall(r"(int32_t|double)\s*([\w\s,\[\]]+);", body):
        members += [(t, n.strip()) for n in names.split(",")]
    assert members == [("int32_t", "n_bins"), ("int32_t", "every"), ("double", "t_from"), ("int32_t", "n_hist"), ("int32_t", "n_bands"),
                       ("double", "hist_range"), ("double", "delta_bound"), ("double", "band_x[2]"), ("double", "band_hw[2]")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    want = [(n.split("[")[0], ctype[t] * 2 if "[" in n else ctype[t]) for t, n in members]
    assert want == list(capi.SphxDensStatsConfig._fields_)
    S = capi.SphxDensStatsConfig
    assert (C.sizeof(S), S.t_from.offset, S.n_hist.offset, S.n_bands.offset, S.hist_range.offset, S.delta_bound.offset, S.band_x.offset,
            S.band_hw.offset) == (72, 8, 16, 20, 24, 32, 40, 56)
    assert profmod.DENS_FIELDS == dc.FIELDS and profmod.DENS_MAX_HIST == 1024 and profmod.DENS_MAX_WORDS * 8 == 60 * 1024


def test_null_handles_are_refused(capi):
    L = capi.lib()
    cfg = capi.SphxDensStatsConfig(n_bins=8, every=1, n_hist=64, hist_range=0.05, delta_bound=0.5)
    nothing = (None,) * 9
    for who, ident in (("ctx", "SPHX:Ctx:null"), ("batch", "SPHX:Batch:null")):
        read = (0, 0, 0, *nothing) if who == "ctx" else (0, 0, 0, 0, *nothing)
        calls = {"enable": (C.byref(cfg),), "disable": (), "reset": (), "sample": (), "read": read}
        for what, args in calls.items():
            rc = getattr(L, f"sphx_{who}_dens_stats_{what}")(None, *args)
            assert rc == capi.SPHX_ERR_ARG and L.sphx_last_error_id().decode() == ident, (who, what)


@pytest.mark.parametrize("kw", [dict(n_bins=-1), dict(n_bins=2.5), dict(every=0), dict(t_from=float("nan")), dict(n_hist=0), dict(n_hist=1025),
                                dict(n_hist=8.0), dict(hist_range=0.0), dict(hist_range=-0.01), dict(hist_range=0.6),
                                dict(hist_range=0.3, delta_bound=0.25), dict(hist_range=float("nan")), dict(hist_range="x"),
                                dict(delta_bound=0.0), dict(delta_bound=0.5000001), dict(delta_bound=float("nan")),
                                dict(bands=[(0.5, 0.1)] * 3), dict(bands=[(0.5, -0.1)]), dict(n_bins=952), dict(n_bins=832, n_hist=1024),
                                dict(n_bins=472, bands=[(0.5, 0.1)]), dict(n_bins=312, bands=[(0.5, 0.1), (0.0, 0.1)])])
def test_binding_checks_the_config_first(cfgmod, capi, kw):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0)
    with pytest.raises(capi.SphxError) as e:
        capi.dens_stats_config(prm, **kw)
    assert e.value.identifier == "SPHX:DensStats:config" and e.value.code == capi.SPHX_ERR_ARG


def test_binding_accepts_the_limits(cfgmod, capi):
    prm = cfgmod.params_from_values(dp=0.05, DL=1.0)
    cfg = capi.dens_stats_config(prm, n_bins=311, bands=[(0.5, 0.1), (0.0, 0.1)], hist_range=0.5)   # 3 * (2488 + 66) = 7662 <= 7680
    assert (cfg.n_bins, cfg.n_bands, cfg.n_hist, cfg.hist_range, cfg.delta_bound, cfg.band_x[1], cfg.band_hw[0]) == (311, 2, 64, 0.5, 0.5, 0.0, 0.1)
    cfg = capi.dens_stats_config(prm)
    assert (cfg.n_bins, cfg.every, cfg.t_from, cfg.n_hist, cfg.hist_range, cfg.delta_bound, cfg.n_bands) == (0, 1, 0.0, 64, 0.05, 0.5, 0)
    assert capi.dens_stats_config(prm, n_bins=951).n_bins == 951                       # 8 * 951 + 66 = 7674
    assert capi.dens_stats_config(prm, n_bins=831, n_hist=1024).n_hist == 1024         # 8 * 831 + 1026 = 7674
    assert capi.dens_stats_config(prm, n_hist=1, hist_range=1e-6, delta_bound=1e-6).n_hist == 1


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uploaded_states(cfgmod, geom, anchor_states):
    """every state the GPU tests upload and compare integer for integer, and the ANCHOR states"""
    states = {name: probe_cases.case(make_case, cfgmod, geom, name)[:2] for name in dc.CASES}
    states.update({f"anchor {k}": v for k, v in anchor_states.items()})
    return states


def test_floating_point_bound(profmod, uploaded_states):
    """The rounding error of the reference's own sums: float64 against np.longdouble in reversed partner order, on every state
    as it is uploaded.  dc.FP_DEVIATION must cover every case."""
    worst = (0.0, None, None, None)
    for name, (prm, parts) in uploaded_states.items():
        n_bins = profmod.n_profile_bins(prm.DH, prm.dp)
        a = dc.numpy_sums(profmod, prm, parts, parts["pos"], n_bins, dc.bands(prm), dc.density(profmod, prm, parts, parts["pos"]), hist_range=0.25)
        b = dc.numpy_sums(profmod, prm, parts, parts["pos"], n_bins, dc.bands(prm),
                          dc.density(profmod, prm, parts, parts["pos"], acc=np.longdouble, reverse=True), hist_range=0.25)
        for x, y in zip(a, b):
            assert all(np.array_equal(x[f], y[f]) for f in dc.COUNTS) and np.array_equal(x["hist"], y["hist"]), name
        dev, f, band = dc.deviation(a, b)
        print(f"{name}: float64 against longdouble reversed: {dev:.3e} ({f}, band {band})")
        if name == "anchor lattice":
            # every delta is -5.3e-05 here, taken out of a rho that is rho0 to 1.1e-16: the sums are 1e-4 of the jittered
            # states' and their own rounding error, relative to them, 1e4 times larger.  The lattice is compared with its known
            # value particle by particle, within 1e-13 absolute (test_lattice_at_rest and its GPU twin), not by this bound.
            assert dev * float(np.max(np.abs(b[band][f]))) <= 1e-13 * float(np.max(b[band]["count"])), name
            assert 0.0 < dev <= dc.LATTICE_FP_DEVIATION, name
            continue
        assert 0.0 < dev <= dc.FP_DEVIATION, name      # every case contributes a figure
        worst = max(worst, (dev, name, f, band), key=lambda w: w[0])
    print(f"worst {worst}")
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    assert 0.0 < worst[0] <= dc.FP_DEVIATION and dc.BOUND == max(16 * dc.FP_DEVIATION, 1e-12) == 1e-12


def test_no_uploaded_state_has_a_particle_on_an_edge(cfgmod, geom, profmod, uploaded_states, lattice):
    """The premise of the exact integer comparisons on uploaded states: no delta within dc.EDGE of a histogram edge or of
    +-delta_bound, for either histogram of dc.HIST -- nor within the outlier test's bound of 0.5."""
    states = dict(uploaded_states, lattice=lattice[:2])
    closest = (np.inf, None)
    for name, (prm, parts) in states.items():
        rho, _ = dc.density(profmod, prm, parts, parts["pos"])
        delta = rho / prm.rho0 - 1.0
        for n_hist, hist_range in dc.HIST:
            assert not dc.near_edges(delta, n_hist, hist_range, 0.5).any(), (name, n_hist, hist_range)
            edges = -hist_range + (2.0 * hist_range / n_hist) * np.arange(n_hist + 1)
            gap = float(np.min(np.abs(delta[:, None] - np.r_[edges, -0.5, 0.5][None, :])))
            closest = min(closest, (gap, name), key=lambda w: w[0])
    print(f"closest to an edge: {closest[0]:.3e} ({closest[1]})")
    assert closest[0] > dc.EDGE
    # near_edges itself: one particle on an edge, one at the bound, one clear of both
    assert dc.near_edges([0.025 + 5e-11, -0.5 + 5e-11, 0.0123], 64, 0.05, 0.5).tolist() == [True, True, False]


# 8 ---------------------------------------------------------------------------------------------------------------
def _fake_sums(prm, member, band, n_bins, n_hist):
    """density sums with known values: a flat delta in every bin, scaled by member and band"""
    cnt = np.full(n_bins, 10.0 * (band + 1))
    mean = np.full(n_bins, 1e-3 * (1 + member))
    return dict(count=cnt, sum_d=mean * cnt, sum_d2=mean * mean * cnt, sum_dvol=-mean * cnt, sum_wall=0.0 * cnt, outliers=0.0 * cnt,
                d_min=mean - 1e-4, d_max=mean + 2e-4, hist=np.full(n_hist, 3, dtype=np.int64), below=1, above=2, hist_range=0.05,
                n_samples=5 + member, t_first=0.03, t_last=0.06)


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

        def dens_stats_enable(self, **kw):
            self.calls.append(("dens_stats_enable", kw))
            self.dens = (kw["n_bins"], len(kw["bands"]) + 1, kw["n_hist"])

        def dens_stats_sums(self, band=0):
            self.calls.append(("dens_stats_sums", band))
            assert 0 <= band < self.dens[1]
            return self._each([_fake_sums(p, m, band, self.dens[0], self.dens[2]) for m, p in enumerate(self.prms)])

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


def test_the_drivers_pass_the_density_keywords_on(cfgmod, capi, driver, profmod, monkeypatch):
    Fake, FakeContext, FakeBatch = _stand_ins(capi)
    monkeypatch.setattr(driver.capi, "Context", FakeContext)
    monkeypatch.setattr(driver.capi, "Batch", FakeBatch)
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.06, output_interval=0.02)
    mid = [(0.5 * prm.DL, max(prm.dp, prm.h))]
    res = driver.run(prm, density_from=0.03, density_every=4, density_hist=(32, 0.1))
    ctx = Fake.made[-1]
    names = [c[0] for c in ctx.calls]
    assert ("dens_stats_enable", dict(n_bins=20, every=4, t_from=0.03, n_hist=32, hist_range=0.1, bands=mid)) in ctx.calls   # band 1: mid-channel
    assert names.count("dens_stats_enable") == 1 and names.index("dens_stats_enable") < names.index("advance")
    assert [c for c in ctx.calls if c[0] == "dens_stats_sums"] == [("dens_stats_sums", 0), ("dens_stats_sums", 1)]
    assert len(res.dens_stats) == 2 and res.dens_stats[1]["count"][0] == 20.0 and len(res.dens_stats[0]["hist"]) == 32
    assert np.array_equal(res.dens_stats[0]["p_mean"], profmod.dens_stats_profiles(prm.DH, prm.p0, _fake_sums(prm, 0, 0, 20, 32))["p_mean"])
    fig = driver.density_figures(prm, res.dens_stats)
    assert np.isclose(fig["delta_rms"], 1e-3, rtol=1e-12) and np.isclose(fig["delta_max"], 1.2e-3, rtol=1e-12) and abs(fig["p_spread"]) < 1e-12
    driver.run(prm, density_from=0.0, density_bands=[(1.0, 0.2), (0.0, 0.1)])    # the defaults: every step, 64 bins on +-0.05
    assert ("dens_stats_enable", dict(n_bins=20, every=1, t_from=0.0, n_hist=64, hist_range=0.05, bands=[(1.0, 0.2), (0.0, 0.1)])) in Fake.made[-1].calls
    res = driver.run(prm)                                                          # off by default: the context is not asked at all
    assert res.dens_stats is None and not {"dens_stats_enable", "dens_stats_sums"} & {c[0] for c in Fake.made[-1].calls}
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.06, output_interval=0.02) for mu in (0.1, 0.1, 0.1)]
    sweep = driver.run_sweep(prms, density_from=0.02, density_every=2)
    assert ("dens_stats_enable", dict(n_bins=20, every=2, t_from=0.02, n_hist=64, hist_range=0.05, bands=mid)) in Fake.made[-1].calls
    for k in ("delta_rms", "delta_max", "p_spread"):
        assert sweep.table[k].shape == (3,), k
    assert np.allclose(sweep.table["delta_rms"], [1e-3, 2e-3, 3e-3], rtol=1e-12) and all(len(r.dens_stats) == 2 for r in sweep.members)
    assert not {"delta_rms", "delta_max", "p_spread"} & set(driver.run_sweep(prms).table)
    ens = driver.run_ensemble(prms, average_from=0.02, density_from=0.02)
    assert len(ens.pooled_density) == 2 and ens.pooled_density[0]["n_members"] == 3 and ens.pooled_density[0]["n_samples"] == 5 + 6 + 7
    assert np.array_equal(ens.pooled_density[1]["count"], 3 * _fake_sums(prms[0], 0, 1, 20, 64)["count"])
    assert np.array_equal(ens.pooled_density[0]["hist"], np.full(64, 9)) and ens.pooled_density[0]["below"] == 3
    want = profmod.pool_dens_stats(prm.DH, prm.p0, [r.dens_stats[0] for r in ens.members])
    assert np.array_equal(ens.pooled_density[0]["d_mean"], want["d_mean"])
    assert driver.run_ensemble(prms, average_from=0.02).pooled_density is None
