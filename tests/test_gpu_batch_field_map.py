"""-m gpu: the velocity-field maps of batches (include/sphx.h section 2g, k_field_map_b) -- every member's flow sampled on a
regular grid in x and y by one launch inside the batch's step loop.  A member's planes must be bit for bit those of a
standalone context with the same config; a sample is checked against profile.shepard_field (the same definition in numpy) of
the member's own download, with shared moving walls too; idle members are not sampled; the lifecycle (reset, toggling,
no feedback on the physics, independence of the batch's statistics and history, repeatability, the read's member stride);
the C ABI names its errors and a refused call leaves a running map alone; driver.run_ensemble and driver.run_sweep.

The channel is dp = 0.05, DL = 3: 1 200 fluid particles per member, and a default map of 120 x 40 nodes = 75 wave tiles = 19
workgroups per member, the last one with three tiles.

The bound of the comparisons with numpy is that of tests/test_gpu_field_map.py: a node sums up to about 150 non-negative
weights, each product rounded to 1.1e-16, then divides once -- about 1e-13 of the largest |value| of a plane; 1e-12 is allowed."""
import ctypes as C

import numpy as np
import pytest

from helpers import batch_members, err_id, make_variant

pytestmark = pytest.mark.gpu

PLANES = ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")
STATS = ("count", "sum_ux", "sum_ux2", "sum_uy", "sum_uy2")
BOUND = 1e-12
VARIANTS = [dict(mu=0.1, c_f=15.0, transport_coeff=0.30, seed=7), dict(mu=0.15, c_f=17.0, transport_coeff=0.20, seed=8),
            dict(mu=0.08, c_f=13.0, transport_coeff=0.30, seed=9), dict(mu=0.12, c_f=15.0, transport_coeff=0.10, seed=10)]
# (nx, ny), wave tiles, workgroups per member
SHAPES = {
    "default": ((0, 0), 75, 19),       # 120 x 40: the last workgroup has three tiles
    "ragged": ((37, 19), 15, 4),       # ragged in both directions
    "half_empty": ((13, 7), 2, 1),     # two half-empty tiles
}


def _numpy_planes(prm, f):
    """One sample's six planes from shepard_field's sums."""
    hit = f["S0"] > 0.0
    z = lambda v: np.where(hit, v, 0.0)
    return dict(count=hit.astype(np.float64), sum_w=z(f["S0"] * prm.dp ** 2), sum_ux=z(f["u_x"]), sum_uy=z(f["u_y"]),
                sum_ux2=z(f["u_x"] ** 2), sum_uy2=z(f["u_y"] ** 2))


def _assert_planes_close(got, want, what):
    """count exactly, the other planes to BOUND of the plane's largest |value|; every figure is printed before it is asserted"""
    assert np.array_equal(got["count"], want["count"]), what + ": count"
    for k in PLANES[1:]:
        scale = max(float(np.max(np.abs(want[k]))), 1e-300)
        err = float(np.max(np.abs(got[k] - want[k])))
        print(f"{what}: {k} off by {err / scale:.3e} of the largest |value|")
        assert err <= BOUND * scale, f"{what}: {k} off by {err / scale:.3e} of the largest |value|"


def _assert_identical(got, want, what):
    for k in PLANES:
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"
    assert (got["n_samples"], got["t_first"], got["t_last"]) == (want["n_samples"], want["t_first"], want["t_last"]), what


def _assert_members_apart(refs, what):
    """A read from another member's block cannot pass: for every pair of members at least 90 % of the nodes of sum_ux differ by
    more than 1e-4 of the plane's largest |value|."""
    for a in range(len(refs)):
        for c in range(a + 1, len(refs)):
            x, y = refs[a]["sum_ux"], refs[c]["sum_ux"]
            scale = max(float(np.max(np.abs(x))), float(np.max(np.abs(y))))
            share = float(np.mean(np.abs(x - y) > 1e-4 * scale))
            print(f"{what}: members {a} and {c} differ at {100 * share:.1f} % of the nodes")
            assert share >= 0.9, (what, a, c, share)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpp", [16, 32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_members_equal_standalone_contexts(cfgmod, geom, capi, shape, lpp):
    (nx, ny), tiles, groups = SHAPES[shape]
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)
    assert members[0][1]["n_fluid"] == 1200
    gx, gy = capi.field_map_shape(members[0][0], nx, ny)
    assert -(-gx // 8) * -(-gy // 8) == tiles and -(-tiles // 4) == groups
    kw = dict(t_end=1e9, lanes_per_particle=lpp)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        K = b.info()["rebuild_every"]
        assert b.info()["lanes_per_particle"] == lpp and K > 1
    n = 3 * K + 1  # crosses re-binnings
    with capi.Context.from_parts(*members[0], **kw) as ctx:
        t_mid = ctx.advance(1e9, max_steps=n // 2)["t"]
    cfg = dict(nx=nx, ny=ny, every=3, t_from=t_mid)
    refs = []
    for prm, parts in members:
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.field_map_enable(**cfg)
            assert ctx.advance(1e9, max_steps=n)["step"] == n
            assert ctx.schedule()["rebins"] >= 2
            refs.append(ctx.field_map_sums())
    assert all(0 < r["n_samples"] < n // 3 + 1 and r["count"].shape == (gy, gx) for r in refs)
    _assert_members_apart(refs, f"{shape} lpp={lpp}")
    for eager in (False, True):
        with capi.Batch.from_parts(*zip(*members), **kw) as b:
            b.field_map_enable(**cfg)
            if eager:
                for _ in range(n):
                    sts = b.advance(1e9, max_steps=1)
                assert b.graph_stats()["slots_eager"] >= n
            else:
                sts = b.advance(1e9, max_steps=n)
                assert b.graph_stats()["slots_replayed"] > 0
            got = b.field_map_sums()
            assert b.info()["realignments"] == 0
        assert len(got) == len(members)
        for m in range(len(members)):
            assert sts[m]["step"] == n
            _assert_identical(got[m], refs[m], f"{shape} lpp={lpp} eager={eager} member {m}")


# 2 ---------------------------------------------------------------------------------------------------------------
def test_sample_now_matches_numpy(cfgmod, geom, capi, profmod):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)
    nf = members[0][1]["n_fluid"]
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.field_map_enable(every=10 ** 9)
        b.advance(1e9, max_steps=7)
        b.field_map_sample()
        downs = [b.download(m, fields=("pos", "vel")) for m in range(len(members))]
        sts = b.sync()
        got = b.field_map_sums()
    nx, ny = capi.field_map_shape(members[0][0])
    want = []
    for m, (prm, parts) in enumerate(members):
        assert got[m]["count"].shape == (ny, nx)
        assert got[m]["n_samples"] == 1 and got[m]["t_first"] == got[m]["t_last"] == sts[m]["t"], m
        assert np.all(got[m]["count"] == got[m]["n_samples"]), m           # every node has a contributor
        f = profmod.shepard_field(downs[m]["pos"][:nf], downs[m]["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny)
        print(f"member {m}: min S0 dp^2 = {np.min(f['S0']) * prm.dp ** 2:.3f}")
        want.append(_numpy_planes(prm, f))
        _assert_planes_close(got[m], want[m], f"member {m}")
    _assert_members_apart(want, "numpy")


# 3 ---------------------------------------------------------------------------------------------------------------
def test_shared_moving_walls(cfgmod, geom, capi, profmod):
    members = []
    for v in VARIANTS:
        prm, parts = make_variant(cfgmod, geom, dp=0.05, DL=1.5, jitter=0.2, seed=v["seed"], developed=True, rho0=2.5, mu=v["mu"],
                                  c_f=v["c_f"], transport_coeff=v["transport_coeff"])
        if members:  # walls and masses are the batch's, not the member's
            parts.update(mass=members[0][1]["mass"], wall_vel=members[0][1]["wall_vel"])
        members.append((prm, parts))
    nf = members[0][1]["n_fluid"]
    kw = dict(t_end=1e9, lanes_per_particle=16)
    cfg = dict(every=2, with_walls=True)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.field_map_enable(**cfg)
        b.advance(1e9, max_steps=7)
        in_loop = b.field_map_sums()
        b.field_map_reset()
        b.field_map_sample()
        now = b.field_map_sums()
        downs = [b.download(m, fields=("pos", "vel")) for m in range(len(members))]
        assert b.info()["realignments"] == 0
    nx, ny = capi.field_map_shape(members[0][0])
    for m, (prm, parts) in enumerate(members):
        assert in_loop[m]["n_samples"] == 3 and now[m]["n_samples"] == 1
        f = profmod.shepard_field(downs[m]["pos"][:nf], downs[m]["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny,
                                  wall_pos=parts["pos"][nf:], wall_vel=parts["wall_vel"][nf:])
        _assert_planes_close(now[m], _numpy_planes(prm, f), f"walls, member {m}")
        fluid_only = profmod.shepard_field(downs[m]["pos"][:nf], downs[m]["vel"][:nf], prm.DL, prm.DH, prm.h, nx, ny)
        assert np.all(now[m]["sum_w"][0] > 1.5 * fluid_only["S0"][0] * prm.dp ** 2)   # the wall rows did enter
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.field_map_enable(**cfg)
            ctx.advance(1e9, max_steps=7)
            ref_loop = ctx.field_map_sums()
            ctx.field_map_reset()
            ctx.field_map_sample()
            ref_now = ctx.field_map_sums()
        _assert_identical(in_loop[m], ref_loop, f"walls, in the loop, member {m}")
        _assert_identical(now[m], ref_now, f"walls, sample now, member {m}")


# 4 ---------------------------------------------------------------------------------------------------------------
def _dt_members(cfgmod, geom):
    """members whose dt differ (c_f 15 / 21 / 11): they need different step counts to one target time"""
    variants = [dict(VARIANTS[0], c_f=15.0), dict(VARIANTS[1], c_f=21.0), dict(VARIANTS[2], c_f=11.0)]
    members = batch_members(cfgmod, geom, 0.05, 3.0, variants)
    dt0 = 0.25 * members[0][0].h / (15.0 + 1.5)
    return members, 10.3 * dt0, 17.9 * dt0


def test_idle_members_are_not_sampled_and_realignment(cfgmod, geom, capi):
    members, t1, t2 = _dt_members(cfgmod, geom)
    kw = dict(t_end=1e9, lanes_per_particle=16)
    every, t_from = 2, 0.45 * t1
    cfg = dict(every=every, t_from=t_from)
    with capi.Batch.from_parts(*zip(*members), **kw) as b:
        b.field_map_enable(**cfg)
        b.advance(t1)
        sts = b.advance(t2)
        assert b.info()["realignments"] >= 1
        got = b.field_map_sums()
    steps = [s["step"] for s in sts]
    assert len(set(steps)) == 3, steps
    for m, (prm, parts) in enumerate(members):
        # the member's own steps, one by one, on a standalone context fed the same targets
        own = []
        with capi.Context.from_parts(prm, parts, **kw) as ctx:
            ctx.field_map_enable(**cfg)
            for target in (t1, t2):
                st = ctx.sync()
                while st["t"] < target - 1e-12:
                    st = ctx.advance(target, max_steps=1)
                    own.append(st)
            ref = ctx.field_map_sums()
        assert own[-1]["step"] == steps[m] and abs(sts[m]["t"] - t2) < 1e-12, (m, steps)
        due = [s for s in own if s["step"] % every == 0 and s["t"] >= t_from]
        assert 0 < len(due) < steps[m] // every, (m, len(due))                 # t_from cut some of them off
        assert min(abs(s["t"] - t_from) for s in own) > 1e-9                    # no step ends on the gate's edge
        g = got[m]
        print(f"member {m}: {steps[m]} steps, {g['n_samples']} samples, {len(due)} due")
        assert g["n_samples"] == len(due) == ref["n_samples"], (m, g["n_samples"], len(due))
        # ... and no slot the member sat out was sampled: no node was visited more often, no sample is later than its last step
        assert np.all(g["count"] == g["n_samples"]), m
        assert abs(g["t_first"] - due[0]["t"]) <= 1e-12 and abs(g["t_last"] - due[-1]["t"]) <= 1e-12, m
        _assert_planes_close(g, ref, f"after the realignment, member {m}")   # summation order only
    assert len({g["n_samples"] for g in got}) > 1


# 5 ---------------------------------------------------------------------------------------------------------------
def test_reset_zeroes_every_member_and_the_read_stride(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)
    M, L = len(members), capi.lib()
    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        b.field_map_enable(nx=13, ny=7, every=1)
        b.advance(1e9, max_steps=5)
        got = b.field_map_sums()
        assert all(g["n_samples"] == 5 and np.all(g["count"] == 5) for g in got)
        # a read with capacity > nx * ny: member m at m * capacity, the gaps untouched
        nn, cap = 13 * 7, 13 * 7 + 9
        bufs = [np.full(M * cap, -7.0) for _ in PLANES]
        ns, t0, t1 = np.zeros(M, dtype=np.int64), np.zeros(M), np.zeros(M)
        gx, gy = C.c_int(0), C.c_int(0)
        assert L.sphx_batch_field_map_read(b._h, cap, C.byref(gx), C.byref(gy), *[capi.ptr(a) for a in bufs],
                                           ns.ctypes.data_as(C.POINTER(C.c_int64)), capi.ptr(t0), capi.ptr(t1)) == capi.SPHX_OK
        assert (gx.value, gy.value) == (13, 7) and list(ns) == [5] * M
        for m in range(M):
            assert (t0[m], t1[m]) == (got[m]["t_first"], got[m]["t_last"])
            for k, a in zip(PLANES, bufs):
                block = a[m * cap:(m + 1) * cap]
                assert np.array_equal(block[:nn].reshape(13, 7).T, got[m][k]), (m, k)
                assert np.all(block[nn:] == -7.0), (m, k)
        assert len({bufs[2][m * cap:m * cap + nn].tobytes() for m in range(M)}) == M   # each member's own sum_ux
        b.field_map_reset()
        for g in b.field_map_sums():
            assert g["n_samples"] == 0 and np.isnan(g["t_first"]) and np.isnan(g["t_last"])
            assert all(np.all(g[k] == 0) for k in PLANES)
        b.advance(1e9, max_steps=2)                                  # ... and sampling goes on
        assert [g["n_samples"] for g in b.field_map_sums()] == [2] * M


def test_toggling_recaptures_graphs(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:3])
    with capi.Batch.from_parts(*zip(*members), t_end=1e9, lanes_per_particle=16) as b:
        b.advance(1e9, max_steps=32)                       # graphs without the sampling kernel
        g0 = b.graph_stats()["graphs_captured"]
        b.field_map_enable(every=1)
        b.advance(1e9, max_steps=32)
        g1 = b.graph_stats()["graphs_captured"]
        assert g1 > g0
        assert [g["n_samples"] for g in b.field_map_sums()] == [32] * 3
        b.field_map_disable()
        b.advance(1e9, max_steps=32)
        assert b.graph_stats()["graphs_captured"] > g1
        with pytest.raises(capi.SphxError) as e:
            b.field_map()
        assert e.value.identifier == "SPHX:Field:disabled"
        b.field_map_enable(nx=31, ny=17, every=2)          # re-enabling starts from zero, in the new shape
        assert all(g["n_samples"] == 0 and g["count"].shape == (17, 31) for g in b.field_map_sums())
        sts = b.advance(1e9, max_steps=24)
        maps = b.field_map()
        for m, g in enumerate(maps):
            assert g["n_samples"] == 12 and g["t_last"] == sts[m]["t"] and np.all(g["count"] == 12), m
            assert g["u_x"].shape == (17, 31) and np.all(np.isfinite(g["u_x"]))


def test_no_feedback_and_independent_of_statistics_and_history(cfgmod, geom, capi):
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS[:3])
    runs = {}
    for fmap, others in ((False, False), (False, True), (True, True), (True, False), (True, False)):
        with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
            if others:
                b.flow_stats_enable(every=3)
                b.history_enable(every=2)
            if fmap:
                b.field_map_enable(every=2, with_walls=True)
            sts = b.advance(1e9, max_steps=30)
            run = dict(sts=sts, states=[b.download(m) for m in range(3)], stats=b.flow_stats_sums(0) if others else None,
                       hist=b.history_records() if others else None, maps=b.field_map_sums() if fmap else None)
            runs.setdefault((fmap, others), []).append(run)
    off, others_only, all_on = runs[(False, False)][0], runs[(False, True)][0], runs[(True, True)][0]
    first, second = runs[(True, False)]
    assert off["sts"] == all_on["sts"]
    for m in range(3):
        for k, v in off["states"][m].items():                         # the map, statistics and history on: the same states
            assert v.tobytes() == all_on["states"][m][k].tobytes(), (m, k)
        for k in STATS:                                               # the statistics and the history do not see the map
            assert others_only["stats"][m][k].tobytes() == all_on["stats"][m][k].tobytes(), (m, k)
        assert others_only["stats"][m]["n_samples"] == all_on["stats"][m]["n_samples"] == 10
        assert others_only["hist"][m][0].shape == (15, 8) and others_only["hist"][m][1] == all_on["hist"][m][1] == 0
        assert others_only["hist"][m][0].tobytes() == all_on["hist"][m][0].tobytes(), m
        assert all_on["maps"][m]["n_samples"] == 15
        _assert_identical(all_on["maps"][m], first["maps"][m], f"the map beside the other samplers, member {m}")
        _assert_identical(first["maps"][m], second["maps"][m], f"two identical runs, member {m}")


# 6 ---------------------------------------------------------------------------------------------------------------
def test_error_identifiers(cfgmod, geom, capi):
    L = capi.lib()
    members = batch_members(cfgmod, geom, 0.05, 3.0, VARIANTS)
    M = len(members)
    nothing = (None, None, *[None] * 6, None, None, None)
    ok = capi.SphxFieldMapConfig(nx=0, ny=0, every=1, with_walls=0, t_from=0.0)
    for fn, args in ((L.sphx_batch_field_map_enable, (C.byref(ok),)), (L.sphx_batch_field_map_disable, ()),
                     (L.sphx_batch_field_map_reset, ()), (L.sphx_batch_field_map_sample, ()),
                     (L.sphx_batch_field_map_read, (0, *nothing))):
        assert err_id(capi, fn, None, *args) == ("SPHX:Batch:null", capi.SPHX_ERR_ARG)
    # (nx = 1 << 12, ny = (1 << 11) + 1: within the bound for one channel, beyond it for four -- refused by arithmetic)
    assert (1 << 12) * ((1 << 11) + 1) <= 1 << 25 < M * (1 << 12) * ((1 << 11) + 1)
    bad_configs = (dict(nx=1), dict(ny=1), dict(nx=-2), dict(every=0), dict(every=-1), dict(t_from=float("nan")),
                   dict(with_walls=2), dict(with_walls=-1), dict(nx=1 << 12, ny=(1 << 11) + 1))

    def refused(h):
        for bad in bad_configs:
            c2 = capi.SphxFieldMapConfig(nx=0, ny=0, every=1, with_walls=0, t_from=0.0)
            for k, v in bad.items():
                setattr(c2, k, v)
            assert err_id(capi, L.sphx_batch_field_map_enable, h, C.byref(c2)) == ("SPHX:Field:config", capi.SPHX_ERR_ARG), bad
        assert err_id(capi, L.sphx_batch_field_map_enable, h, None) == ("SPHX:Field:config", capi.SPHX_ERR_ARG)

    with capi.Batch.from_parts(*zip(*members), t_end=1e9) as b:
        h = b._h
        assert err_id(capi, L.sphx_batch_field_map_read, h, 0, *nothing) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_batch_field_map_sample, h) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        assert err_id(capi, L.sphx_batch_field_map_reset, h) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)
        assert L.sphx_batch_field_map_disable(h) == capi.SPHX_OK       # a no-op when off
        refused(h)
        with pytest.raises(capi.SphxError) as e:
            b.field_map_enable(every=0)
        assert e.value.identifier == "SPHX:Field:config"
        # a refused config leaves the batch without a map, and stepping
        assert err_id(capi, L.sphx_batch_field_map_read, h, 0, *nothing)[0] == "SPHX:Field:disabled"
        assert [s["step"] for s in b.advance(1e9, max_steps=3)] == [3] * M
        b.field_map_enable(every=1)
        b.advance(1e9, max_steps=4)
        before = b.field_map_sums()
        assert [g["n_samples"] for g in before] == [4] * M
        refused(h)                                                     # a refused enable leaves the running map and its sums
        gx, gy = C.c_int(0), C.c_int(0)
        assert L.sphx_batch_field_map_read(h, 0, C.byref(gx), C.byref(gy), *[None] * 6, None, None, None) == capi.SPHX_OK
        assert (gx.value, gy.value) == (120, 40)                       # all NULL: capacity is not checked
        nn = 4800
        buf = np.full(M * nn, -1.0)
        for slot in range(6):
            arrs = [capi.ptr(buf) if k == slot else None for k in range(6)]
            assert err_id(capi, L.sphx_batch_field_map_read, h, nn - 1, None, None, *arrs, None, None, None) == \
                ("SPHX:Field:capacity", capi.SPHX_ERR_ARG)
        assert np.all(buf == -1.0)
        after = b.field_map_sums()
        for m in range(M):
            _assert_identical(after[m], before[m], f"after the refused calls, member {m}")
        b.field_map_disable()
        assert err_id(capi, L.sphx_batch_field_map_sample, h) == ("SPHX:Field:disabled", capi.SPHX_ERR_STATE)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_run_ensemble_fills_the_maps(cfgmod, geom, driver):
    prm = cfgmod.params_from_values(dp=0.05, DL=3.0, end_time=0.06, output_interval=0.02)
    parts = [geom.init_particles(prm)] + [geom.perturbed_particles(prm, 0.01, k) for k in (1, 2)]
    res = driver.run_ensemble([prm] * 3, average_from=0.02, field_from=0.02, parts_list=parts)
    assert len(res.members) == 3 and res.pooled is not None
    for m, r in enumerate(res.members):
        fa = r.field_avg
        assert fa["u_x"].shape == (40, 120) and 0 < fa["n_samples"] < r.steps and fa["t_first"] >= 0.02 and fa["t_last"] == r.t, m
        assert np.all(fa["count"] == fa["n_samples"]) and np.all(np.isfinite(fa["u_x"]))
    pf = res.pooled_field
    assert pf["n_members"] == 3 and pf["n_samples"] == sum(r.field_avg["n_samples"] for r in res.members)
    assert np.array_equal(pf["count"], sum(r.field_avg["count"] for r in res.members))
    assert pf["u_x_se"].shape == (40, 120) and np.all(np.isfinite(pf["u_x_se"])) and np.all(pf["u_x_se"] >= 0.0)
    assert np.any(pf["u_x_se"] > 0.0)                                  # the perturbed members do differ
    plain = driver.run_ensemble([prm] * 3, average_from=0.02, parts_list=parts)
    assert plain.pooled_field is None and all(r.field_avg is None for r in plain.members)
    for a, c in zip(res.members, plain.members):                       # the map does not touch the run
        assert (a.steps, a.t) == (c.steps, c.t) and a.pos.tobytes() == c.pos.tobytes() and a.vel.tobytes() == c.vel.tobytes()


def test_run_sweep_adds_the_field_columns(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu, end_time=0.06, output_interval=0.02) for mu in (0.1, 0.15, 0.2)]
    res = driver.run_sweep(prms, history_capacity=256, field_from=0.02)
    cols = {"field_L2": "L2", "field_x_spread": "x_spread", "field_ix": "ix", "field_uy_rms": "uy_rms"}
    for m, r in enumerate(res.members):
        assert r.field_avg["n_samples"] > 0 and r.field_avg["t_first"] >= 0.02 and r.field_avg["t_last"] == r.t, m
        fig = driver.field_figures(prms[m], r.field_avg)
        assert np.isfinite(fig["L2"]) and np.isfinite(fig["x_spread"]) and 0 <= fig["ix"] < 120
        for col, k in cols.items():
            assert res.table[col].shape == (3,) and res.table[col][m] == fig[k], (m, col)
    assert len({r.field_avg["u_x"].tobytes() for r in res.members}) == 3   # each member's own map
