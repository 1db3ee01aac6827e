"""Pair statistics (include/sphx.h sections 2l / 2m) without a GPU: the library exports the ten entry points and the ctypes
struct has the header's layout; profile.pair_histogram -- the kernel's oracle -- against the oracle's own pair list on four
states (the anchor), on the lattice's known table and on hand-placed pairs exactly on bin edges; pooling and the figures on
hand-built sums; the bindings check their arguments before the device; the drivers' keywords, followed through stand-ins for
capi.Context and capi.Batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pair_dist_cases as pc
from helpers import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = tuple(f"sphx_{who}_pair_dist_{what}" for who in ("ctx", "batch") for what in ("enable", "disable", "reset", "sample", "read"))


# 1 ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert len(SYMBOLS) == 10
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert not any("slab" in n and "pair_dist" in n for n in declared)  # slab rings are a follow-up
    assert re.search(r"^#define SPHX_PAIR_DIST_MAX_BINS 1024\s*$", hdr, re.M) and capi.PAIR_DIST_MAX_BINS == 1024
    assert "2l. Pair statistics" in raw and "2m. Pair statistics of a batch" in raw


def test_config_struct_matches_the_header(capi):
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.search(r"typedef struct sphx_pair_dist_config \{(.*?)\} sphx_pair_dist_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for t, names in re.findall(r"(int32_t|double)\s*([\w\s,\[\]]+);", body):
        members += [(t, n.strip()) for n in names.split(",")]
    assert members == [("int32_t", "n_bins"), ("int32_t", "every"), ("double", "t_from"), ("double", "r_max"), ("double", "y_margin"),
                       ("int32_t", "with_walls"), ("int32_t", "n_bands"), ("double", "band_x[2]"), ("double", "band_hw[2]")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    want = [(n.split("[")[0], ctype[t] * 2 if "[" in n else ctype[t]) for t, n in members]
    assert want == list(capi.SphxPairDistConfig._fields_)
    S = capi.SphxPairDistConfig
    assert (C.sizeof(S), S.t_from.offset, S.r_max.offset, S.y_margin.offset, S.with_walls.offset, S.n_bands.offset, S.band_x.offset,
            S.band_hw.offset) == (72, 8, 16, 24, 32, 36, 40, 56)


def test_null_handles_are_refused(capi):
    L = capi.lib()
    cfg = capi.SphxPairDistConfig(n_bins=8, every=1)
    nothing = (None,) * 8
    for who, ident in (("ctx", "SPHX:Ctx:null"), ("batch", "SPHX:Batch:null")):
        calls = {"enable": (C.byref(cfg),), "disable": (), "reset": (), "sample": (), "read": (0, 0, *nothing)}
        for what, args in calls.items():
            rc = getattr(L, f"sphx_{who}_pair_dist_{what}")(None, *args)
            assert rc == capi.SPHX_ERR_ARG and L.sphx_last_error_id().decode() == ident, (who, what)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anchor_states(cfgmod, geom):
    """name -> (prm, parts) of pc.ANCHOR, made once"""
    return {name: make_case(cfgmod, geom, dp=dp, DL=DL, jitter=jitter, seed=11, developed=True) for name, (dp, DL, jitter) in pc.ANCHOR.items()}


def _oracle_hist(oracle, profmod, prm, parts, n_bins):
    """(ff, fw) histograms of the oracle's pair list at 2h, binned from its dx, dy columns by the rule of section 2l"""
    nf, nt = parts["n_fluid"], parts["n_total"]
    nb = oracle.neighbor_search(parts["pos"], nf, nt, prm.h, prm.DL)
    pj = nb[1].astype(np.int64) - 1
    assert np.all(nb[0].astype(np.int64) - 1 < nf)                 # i is always a fluid particle
    r2 = nb[2] * nb[2] + nb[3] * nb[3]
    e2 = profmod.pair_edges(2.0 * prm.h, n_bins)[1]

    def hist(v):
        v = v[v < e2[-1]]
        return np.bincount(np.searchsorted(e2, v, side="right") - 1, minlength=n_bins).astype(np.int64)

    return hist(r2[pj < nf]), hist(r2[pj >= nf])


@pytest.mark.parametrize("name", list(pc.ANCHOR))
def test_numpy_histogram_against_the_oracles_pair_list(oracle, profmod, anchor_states, name):
    """The anchor: at r_max = 2h the fluid-fluid histogram is twice that of the oracle's fluid-fluid pairs (it lists a pair once,
    a centre counts every partner) and the fluid-wall histogram equals that of its fluid-wall pairs -- the oracle's
    de-duplication at the seam and the minimum image agree, also on one and two cell columns."""
    prm, parts = anchor_states[name]
    nf = parts["n_fluid"]
    ff, fw = _oracle_hist(oracle, profmod, prm, parts, 64)
    (got,) = profmod.pair_histogram(parts["pos"][:nf], prm.DL, prm.DH, 2.0 * prm.h, 64, wall_pos=parts["pos"][nf:])
    assert ff.sum() > 0 and fw.sum() > 0
    assert np.array_equal(got["ff"], 2 * ff) and np.array_equal(got["fw"], fw)
    assert got["centres"] == int(np.count_nonzero((parts["pos"][:nf, 1] >= 0.0) & (parts["pos"][:nf, 1] <= prm.DH)))


def test_the_lattice_table(profmod, anchor_states):
    prm, parts = anchor_states["lattice"]
    nf = parts["n_fluid"]
    assert (nf, parts["n_total"] - nf) == (1200, 480) and prm.h == 1.3 * prm.dp
    fluid, walls = parts["pos"][:nf], parts["pos"][nf:]
    (whole,) = profmod.pair_histogram(fluid, prm.DL, prm.DH, 2.0 * prm.h, 64, wall_pos=walls)
    want = np.zeros(64, dtype=np.int64)
    for k, v in pc.LATTICE_FF.items():
        want[k] = v
    assert np.array_equal(whole["ff"], want) and whole["ff"].sum() == 22680 == 2 * 11340
    assert whole["fw"].sum() == pc.LATTICE_FW_TOTAL and whole["centres"] == 1200
    assert abs(whole["r_min"] / prm.dp - 1.0) <= 1e-14
    (bulk,) = profmod.pair_histogram(fluid, prm.DL, prm.DH, 2.0 * prm.h, 64, y_margin=2.0 * prm.h)
    assert (bulk["centres"], bulk["ff"].sum() / bulk["centres"]) == pc.LATTICE_BULK and bulk["fw"].sum() == 0
    prof = profmod.pair_dist_profiles(bulk, prm.dp)
    assert prof["n_neigh"] == 20.0 and prof["r_min"] == bulk["r_min"] and np.all(prof["g_wall"] == 0)
    e = bulk["r_edges"]
    k = 24   # the first shell: 4 partners of each centre in the ring of bin 24
    assert prof["g"][k] == 4.0 * 840 / (840 * np.pi * (e[k + 1] ** 2 - e[k] ** 2) / prm.dp ** 2)


def test_the_bin_rule_on_hand_placed_pairs(profmod):
    pairs = pc.edge_pairs()
    pos = np.array([p for ab in pairs for p in ab])
    (got,) = profmod.pair_histogram(pos, 3.0, 1.0, pc.EDGE_R_MAX, pc.EDGE_BINS)
    assert np.array_equal(got["ff"], pc.edge_bins()) and got["centres"] == len(pos) and got["r2_min"] == 0.0
    w = pc.EDGE_R_MAX / pc.EDGE_BINS
    for k in pc.EDGE_KS + (0,):                        # one pair at a time: dx = k w lands in bin k (the lower edge is inclusive)
        (one,) = profmod.pair_histogram(np.array([[0.25, 0.5], [0.25 + k * w, 0.5]]), 3.0, 1.0, pc.EDGE_R_MAX, pc.EDGE_BINS)
        assert np.flatnonzero(one["ff"]).tolist() == [k] and one["ff"][k] == 2 and one["r2_min"] == (k * w) ** 2
    (out,) = profmod.pair_histogram(np.array([[0.25, 0.5], [0.25 + pc.EDGE_R_MAX, 0.5]]), 3.0, 1.0, pc.EDGE_R_MAX, pc.EDGE_BINS)
    assert out["ff"].sum() == 0 and out["r2_min"] == np.inf and out["r_min"] == np.inf and out["centres"] == 2   # dx = r_max: not counted
    below = np.nextafter(pc.EDGE_R_MAX, 0.0)
    (last,) = profmod.pair_histogram(np.array([[0.0, 0.5], [below, 0.5]]), 3.0, 1.0, pc.EDGE_R_MAX, pc.EDGE_BINS)  # (from x = 0: not rounded)
    assert np.flatnonzero(last["ff"]).tolist() == [pc.EDGE_BINS - 1]


def test_minimum_image_margin_bands_and_walls(profmod):
    DL, DH = 1.0, 1.0
    pos = np.array([[0.01, 0.5], [0.99, 0.5], [0.5, 0.05], [0.5, 0.95], [0.5, 0.5]])
    walls = np.array([[0.5, -0.02], [0.52, 1.03]])
    bands = [(0.5, 0.1), (0.0, 0.05)]
    got = profmod.pair_histogram(pos, DL, DH, 0.1, 10, bands=bands, wall_pos=walls)
    assert [g["centres"] for g in got] == [5, 3, 2]
    assert got[0]["ff"].tolist() == [0, 0, 2, 0, 0, 0, 0, 0, 0, 0]            # the pair across the seam, 0.02 apart, both ways
    assert got[2]["ff"].tolist() == got[0]["ff"].tolist() and got[1]["ff"].sum() == 0
    assert got[0]["fw"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1, 0]            # 0.07 from (0.5, 0.05); 0.0825 from (0.5, 0.95)
    assert got[1]["fw"].tolist() == got[0]["fw"].tolist() and got[2]["fw"].sum() == 0
    inner = profmod.pair_histogram(pos, DL, DH, 0.1, 10, bands=bands, y_margin=0.1, wall_pos=walls)
    assert [g["centres"] for g in inner] == [3, 1, 2] and inner[0]["fw"].sum() == 0 and inner[0]["ff"].sum() == 2
    assert profmod.pair_histogram(pos, DL, DH, 0.1, 10)[0]["fw"].sum() == 0   # no walls given: zeros
    shared = profmod.pair_separations(pos, DL, 0.1, walls)
    again = profmod.pair_histogram(pos, DL, DH, 0.05, 5, bands=bands, wall_pos=walls, separations=shared)
    fresh = profmod.pair_histogram(pos, DL, DH, 0.05, 5, bands=bands, wall_pos=walls)
    pc.assert_counts_equal(again, fresh, "a shared pair search at a larger range")


def test_chunks_and_windows_do_not_change_a_count(profmod, anchor_states):
    prm, parts = anchor_states["jittered"]
    nf = parts["n_fluid"]
    fluid, walls = parts["pos"][:nf].copy(), parts["pos"][nf:]
    fluid[::7, 0] -= prm.DL                                  # some not wrapped: the minimum image folds them
    a = profmod.pair_separations(fluid, prm.DL, 2.0 * prm.h, walls, chunk=512)
    b = profmod.pair_separations(fluid, prm.DL, 2.0 * prm.h, walls, chunk=10 ** 9)   # one chunk: every partner, no window
    for kind in ("ff", "fw"):
        ka, kb = np.lexsort((a["r2_" + kind], a["i_" + kind])), np.lexsort((b["r2_" + kind], b["i_" + kind]))
        assert np.array_equal(a["i_" + kind][ka], b["i_" + kind][kb]) and np.array_equal(a["r2_" + kind][ka], b["r2_" + kind][kb])


# 3 ---------------------------------------------------------------------------------------------------------------
def _sums(ff, fw, centres, r2_min, r_max=0.13, **head):
    e = np.linspace(0.0, r_max, len(ff) + 1)
    return dict(r_edges=e, ff=np.array(ff, dtype=np.int64), fw=np.array(fw, dtype=np.int64), centres=centres, r2_min=r2_min,
                r_min=float(np.sqrt(r2_min)), **head)


def test_pooling_adds_the_integers(profmod):
    a = _sums([1, 2, 3], [0, 1, 0], 10, 0.0025, n_samples=2, t_first=0.3, t_last=0.5)
    b = _sums([4, 0, 1], [2, 0, 0], 7, 0.0016, n_samples=1, t_first=0.2, t_last=0.4)
    never = _sums([0, 0, 0], [0, 0, 0], 0, np.inf, n_samples=0, t_first=float("nan"), t_last=float("nan"))
    out = profmod.pool_pair_dist([a, b, never])
    assert out["ff"].tolist() == [5, 2, 4] and out["fw"].tolist() == [2, 1, 0] and out["ff"].dtype == np.int64
    assert (out["centres"], out["r2_min"], out["r_min"]) == (17, 0.0016, 0.04)
    assert (out["n_samples"], out["t_first"], out["t_last"]) == (3, 0.2, 0.5)
    per_member = profmod.pool_pair_dist([[a, b], [b, never]])              # one list of bands per channel: band by band
    assert per_member[0]["ff"].tolist() == [5, 2, 4] and per_member[1]["ff"].tolist() == [4, 0, 1] and per_member[1]["centres"] == 7
    alone = profmod.pool_pair_dist([never])
    assert alone["r2_min"] == np.inf and np.isnan(alone["t_first"]) and alone["n_samples"] == 0
    with pytest.raises(AssertionError, match="different bins"):
        profmod.pool_pair_dist([a, _sums([1, 2], [0, 0], 1, 0.01)])
    with pytest.raises(AssertionError, match="nothing to pool"):
        profmod.pool_pair_dist([])


def test_profiles_and_figures_on_hand_built_sums(cfgmod, profmod, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0)
    dp, r_max, n = prm.dp, 2.0 * prm.h, 26
    e = np.linspace(0.0, r_max, n + 1)                      # bins 0.1 dp wide: mid-points 0.05, 0.15, ... dp
    ff = np.zeros(n, dtype=np.int64)
    ff[9], ff[10], ff[14] = 300, 100, 400                   # first shell at 0.95 and 1.05 dp, second at 1.45 dp
    whole = dict(r_edges=e, ff=ff, fw=np.zeros(n, dtype=np.int64), centres=100, r2_min=(0.93 * dp) ** 2, r_min=0.93 * dp)
    prof = profmod.pair_dist_profiles(whole, dp)
    assert prof["n_neigh"] == 8.0 and prof["r_min"] == 0.93 * dp and np.array_equal(prof["r_mid"], 0.5 * (e[:-1] + e[1:]))
    ring = np.pi * (e[10] ** 2 - e[9] ** 2) / dp ** 2
    assert prof["g"][9] == 300 / (100 * ring) and prof["g"][0] == 0.0 and np.all(prof["g_wall"] == 0.0)
    fig = driver.pair_dist_figures(prm, [whole])
    assert fig["r_min_dp"] == 0.93 * dp / dp and fig["n_neigh"] == 8.0 and np.isnan(fig["seam_dev"])
    r = prof["r_mid"][[9, 10]] / dp                         # the pairs below 1.207 dp: 300 at 0.95, 100 at 1.05
    mean = (300 * r[0] + 100 * r[1]) / 400
    np.testing.assert_allclose(fig["sigma1_dp"], np.sqrt((300 * (r[0] - mean) ** 2 + 100 * (r[1] - mean) ** 2) / 400), rtol=1e-12)
    lattice = dict(whole, ff=np.where(np.arange(n) == 9, 400, 0).astype(np.int64))
    assert driver.pair_dist_figures(prm, [lattice])["sigma1_dp"] == 0.0    # one bin: zero, i.e. within a bin width
    empty = dict(whole, ff=np.zeros(n, dtype=np.int64), centres=0, r2_min=np.inf, r_min=np.inf)
    fig0 = driver.pair_dist_figures(prm, [empty])
    assert np.isnan(fig0["n_neigh"]) and np.isnan(fig0["sigma1_dp"]) and fig0["r_min_dp"] == np.inf
    assert np.all(np.isnan(profmod.pair_dist_profiles(empty, dp)["g"]))
    # the seam against mid-channel: a seam that misses a tenth of the first shell
    mid = dict(whole, centres=10, ff=ff // 10)
    seam = dict(mid, ff=np.where(np.arange(n) == 9, 27, ff // 10).astype(np.int64))
    fig = driver.pair_dist_figures(prm, [whole, mid, seam])
    g_mid, g_seam = profmod.pair_dist_profiles(mid, dp)["g"], profmod.pair_dist_profiles(seam, dp)["g"]
    assert fig["seam_dev"] == np.max(np.abs(g_seam - g_mid)) / max(g_mid.max(), g_seam.max()) > 0.0
    assert driver.pair_dist_figures(prm, [whole, mid, mid])["seam_dev"] == 0.0


# 4 ---------------------------------------------------------------------------------------------------------------
class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} made before the arguments were checked")


def _bare(capi, monkeypatch, cls, members=3):
    monkeypatch.setattr(capi, "lib", lambda: _NoLib())
    b = object.__new__(cls)
    b._h = C.c_void_p()  # (nothing to destroy)
    b._pair_dist = None
    prm = capi.SphxParams(DL=3.0, DH=1.0, dp=0.05, h=0.065)
    if cls is capi.Batch:
        b.n_members, b.params = members, [prm] * members
    else:
        b.params = prm
    return b


BAD = [dict(n_bins=0), dict(n_bins=-1), dict(n_bins=1025), dict(n_bins=2.5), dict(every=0), dict(every=1.5), dict(t_from=float("nan")),
       dict(t_from="soon"), dict(r_max=-0.01), dict(r_max=0.1300001), dict(r_max=float("nan")), dict(r_max=float("inf")), dict(r_max="far"),
       dict(y_margin=-0.1), dict(y_margin=float("nan")), dict(with_walls=2), dict(with_walls="yes"), dict(bands=[(1.5, 0.1)] * 3),
       dict(bands=[(1.5,)]), dict(bands=[(float("inf"), 0.1)]), dict(bands=[(1.5, -0.1)])]


@pytest.mark.parametrize("kw", BAD)
def test_binding_checks_the_config_first(capi, monkeypatch, kw):
    for cls in (capi.Context, capi.Batch):
        b = _bare(capi, monkeypatch, cls)
        with pytest.raises(capi.SphxError) as e:
            b.pair_dist_enable(**kw)
        assert e.value.identifier == "SPHX:PairDist:config" and e.value.code == capi.SPHX_ERR_ARG
        assert b._pair_dist is None


def test_binding_accepts_the_limits(capi):
    prm = capi.SphxParams(DL=3.0, DH=1.0, dp=0.05, h=0.065)
    cfg = capi.pair_dist_config(prm)
    assert (cfg.n_bins, cfg.every, cfg.t_from, cfg.r_max, cfg.y_margin, cfg.with_walls, cfg.n_bands) == (64, 1, 0.0, 0.0, 0.0, 0, 0)
    cfg = capi.pair_dist_config(prm, n_bins=1024, every=7, t_from=-1.0, r_max=2.0 * prm.h, y_margin=0.6, with_walls=True,
                                bands=[(1.5, 0.1), (0.0, 0.2)])
    assert (cfg.n_bins, cfg.r_max, cfg.with_walls, cfg.n_bands, list(cfg.band_x), list(cfg.band_hw)) == (1024, 0.13, 1, 2, [1.5, 0.0], [0.1, 0.2])
    assert capi.pair_dist_config(prm, n_bins=1, r_max=1e-6).n_bins == 1


def test_state_is_checked_before_the_device(capi, monkeypatch):
    for cls, where in ((capi.Batch, "batch"), (capi.Context, "context")):
        b = _bare(capi, monkeypatch, cls)
        for call in (b.pair_dist, b.pair_dist_sums, b.pair_dist_sample, b.pair_dist_reset):
            with pytest.raises(capi.SphxError) as e:
                call()
            assert e.value.identifier == "SPHX:PairDist:disabled" and e.value.code == capi.SPHX_ERR_STATE
            assert e.value.message == f"pair statistics are not enabled on this {where}"
        b._pair_dist = (64, 3, 0.13)
        for band in (-1, 3, 1.0):
            with pytest.raises(capi.SphxError) as e:
                b.pair_dist(band)
            assert e.value.identifier == "SPHX:PairDist:band"
    assert not hasattr(__import__("importlib").import_module(capi.__name__.rsplit(".", 1)[0] + ".slab").HipSlabEngine, "pair_dist_enable")


# 5 ---------------------------------------------------------------------------------------------------------------
def _fake_sums(prm, m, n_bins, n_bands):
    """known sums of member m: band b's first-shell bin holds 100 (m + 1) (b + 1) pairs"""
    e = np.append(np.arange(n_bins) * (2.0 * prm.h / n_bins), 2.0 * prm.h)
    out = []
    for b in range(n_bands):
        ff = np.zeros(n_bins, dtype=np.int64)
        ff[int(n_bins * prm.dp / (2.0 * prm.h))] = 100 * (m + 1) * (b + 1)
        r2 = ((0.9 + 0.01 * m) * prm.dp) ** 2
        out.append(dict(r_edges=e, ff=ff, fw=np.zeros(n_bins, dtype=np.int64), centres=25 * (b + 1), r2_min=r2, r_min=float(np.sqrt(r2)),
                        n_samples=4, t_first=0.02 + 0.001 * m, t_last=0.06))
    return out


def _stand_ins(capi):
    """Stand-ins for capi.Context and capi.Batch: no device, the calls a driver makes recorded in order, pair sums with known values."""

    class Fake:
        made = []

        def __init__(self, prms, parts_list, launch, many):
            self.prms, self.parts, self.launch, self.calls, self.n_adv, self.many = list(prms), list(parts_list), launch, [], 0, many
            self.n_members = len(self.prms)
            self.pairs = None
            Fake.made.append(self)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.close()

        def close(self):
            self.calls.append(("close",))

        def _each(self, v):
            return v if self.many else v[0]

        def pair_dist_enable(self, **kw):
            self.calls.append(("pair_dist_enable", kw))
            self.pairs = (kw["n_bins"], len(kw["bands"]) + 1)

        def pair_dist_sums(self):
            self.calls.append(("pair_dist_sums",))
            return self._each([_fake_sums(p, m, *self.pairs) for m, p in enumerate(self.prms)])

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


def _names(b):
    return [c[0] for c in b.calls]


def test_run_passes_the_pair_keywords_on(cfgmod, capi, driver, profmod, monkeypatch):
    Fake, FakeContext, _ = _stand_ins(capi)
    monkeypatch.setattr(driver.capi, "Context", FakeContext)
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.06, output_interval=0.02)
    hw = max(prm.dp, prm.h)
    res = driver.run(prm, pairs_from=0.03, pairs_every=4, pairs_bins=32, pairs_walls=True)
    ctx = Fake.made[-1]
    names = _names(ctx)
    want = dict(n_bins=32, every=4, t_from=0.03, y_margin=2.0 * prm.h, with_walls=True, bands=[(0.5 * prm.DL, hw), (0.0, hw)])
    assert ("pair_dist_enable", want) in ctx.calls                        # mid-channel and seam, centres 2h from the walls
    assert names.count("pair_dist_enable") == 1 and names.index("pair_dist_enable") < names.index("advance")
    assert names.count("pair_dist_sums") == 1 and names.index("pair_dist_sums") > len(names) - 1 - names[::-1].index("advance")
    assert len(res.pair_dist) == 3
    for b, band in enumerate(res.pair_dist):
        ref = _fake_sums(prm, 0, 32, 3)[b]
        assert np.array_equal(band["ff"], ref["ff"]) and band["centres"] == ref["centres"]
        assert np.array_equal(band["g"], profmod.pair_dist_profiles(ref, prm.dp)["g"]) and band["n_neigh"] == 100.0 * (b + 1) / (25 * (b + 1))
    driver.run(prm, pairs_from=0.0, pairs_bands=[(1.0, 0.2)])              # the defaults: 64 bins, every step, fluid only
    assert ("pair_dist_enable", dict(n_bins=64, every=1, t_from=0.0, y_margin=2.0 * prm.h, with_walls=False, bands=[(1.0, 0.2)])) in Fake.made[-1].calls
    res = driver.run(prm)                                                  # off by default: the context is not asked at all
    assert res.pair_dist is None and not {"pair_dist_enable", "pair_dist_sums"} & set(_names(Fake.made[-1]))
    with pytest.raises(ValueError, match="pairs_from needs the resident engine"):
        driver.run(prm, engine="mex", pairs_from=0.0)


def test_run_sweep_adds_the_pair_columns(cfgmod, capi, driver, monkeypatch):
    Fake, _, FakeBatch = _stand_ins(capi)
    monkeypatch.setattr(driver.capi, "Batch", FakeBatch)
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, transport_coeff=tc, end_time=0.06, output_interval=0.02) for tc in (0.1, 0.2, 0.3)]
    res = driver.run_sweep(prms, pairs_from=0.03, pairs_every=2)
    b = Fake.made[-1]
    names = _names(b)
    assert names.count("pair_dist_enable") == 1 and names.index("pair_dist_enable") < names.index("advance") and names.count("pair_dist_sums") == 1
    (asked,) = [c[1] for c in b.calls if c[0] == "pair_dist_enable"]
    assert asked["y_margin"] == 2.0 * prms[0].h and asked["every"] == 2 and asked["t_from"] == 0.03 and len(asked["bands"]) == 2
    for m, r in enumerate(res.members):
        fig = driver.pair_dist_figures(prms[m], r.pair_dist)
        assert fig["r_min_dp"] == (0.9 + 0.01 * m) * prms[m].dp / prms[m].dp and fig["n_neigh"] == 4.0 * (m + 1) and fig["sigma1_dp"] == 0.0
        for col in ("r_min_dp", "n_neigh", "sigma1_dp"):
            assert res.table[col].shape == (3,) and res.table[col][m] == fig[col], (m, col)
    assert "seam_dev" not in res.table
    plain = driver.run_sweep(prms)
    assert not {"r_min_dp", "n_neigh", "sigma1_dp"} & set(plain.table) and all(r.pair_dist is None for r in plain.members)
    assert not {"pair_dist_enable", "pair_dist_sums"} & set(_names(Fake.made[-1]))


def test_run_ensemble_pools_the_pairs(cfgmod, capi, driver, profmod, monkeypatch):
    Fake, _, FakeBatch = _stand_ins(capi)
    monkeypatch.setattr(driver.capi, "Batch", FakeBatch)
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.06, output_interval=0.02) for _ in range(3)]
    res = driver.run_ensemble(prms, average_from=0.02, pairs_from=0.03, pairs_bins=16)
    pooled = res.pooled_pairs
    assert len(pooled) == 3
    for b in range(3):
        mine = [_fake_sums(prms[m], m, 16, 3)[b] for m in range(3)]
        assert np.array_equal(pooled[b]["ff"], sum(s["ff"] for s in mine)) and pooled[b]["centres"] == 75 * (b + 1)
        assert pooled[b]["r2_min"] == mine[0]["r2_min"] and pooled[b]["n_samples"] == 12 and pooled[b]["t_first"] == 0.02
        assert pooled[b]["n_neigh"] == 600.0 * (b + 1) / (75 * (b + 1))
    sweep = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.06, output_interval=0.02) for mu in (0.1, 0.2)]
    res = driver.run_ensemble(sweep, average_from=0.02, pairs_from=0.03)    # members that differ in their physics: nothing pooled
    assert res.pooled_pairs is None and all(r.pair_dist is not None for r in res.members)
    res = driver.run_ensemble(prms, average_from=0.02)
    assert res.pooled_pairs is None and all(r.pair_dist is None for r in res.members)
    assert driver.EnsembleResult(members=[], pooled=None, wall_seconds=0.0).pooled_pairs is None
