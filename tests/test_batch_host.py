"""Batched contexts (include/sphx.h section 2b) without a GPU: the C ABI declares and exports the sphx_batch_* entry points,
every refusal of sphx_batch_create / capi.Batch comes with its SPHX:Batch:* id before the device is touched, and
driver.run_batch refuses what only single-channel runs do."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SYMBOLS = ("sphx_batch_create", "sphx_batch_destroy", "sphx_batch_advance", "sphx_batch_enqueue_steps",
                 "sphx_batch_sync", "sphx_batch_download", "sphx_batch_monitor", "sphx_batch_info",
                 "sphx_batch_graph_stats")


def test_batch_symbols_declared_and_exported(capi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert "sphx_batch" in hdr
    for name in BATCH_SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)


def _case(cfgmod, geom, seed=1, **kw):
    return make_case(cfgmod, geom, dp=0.05, DL=3.0, jitter=0.2, seed=seed, developed=True, **kw)


def _members(cfgmod, geom, n=3, **kw):
    return [_case(cfgmod, geom, seed=10 + k, **kw) for k in range(n)]


def _refused(capi, ident, fn):
    with pytest.raises(capi.SphxError) as e:
        fn()
    assert e.value.identifier == ident, e.value
    return e.value


def test_mismatched_dp_is_refused(cfgmod, geom, capi):
    members = _members(cfgmod, geom)
    prm1 = cfgmod.params_from_values(dp=0.05000001, DL=3.0)
    members[1] = (prm1, members[1][1])
    err = _refused(capi, "SPHX:Batch:geometry", lambda: capi.Batch.from_parts(*zip(*members), t_end=1.0))
    assert "member 1" in err.message and "dp" in err.message


def test_mismatched_t_end_is_refused_by_the_c_abi(cfgmod, geom, capi):
    members = _members(cfgmod, geom, n=2)
    p = [capi.make_params(m[0], t_end=1.0 + k) for k, m in enumerate(members)]
    arr = (capi.SphxParams * 2)(*p)
    nf, nt = members[0][1]["n_fluid"], members[0][1]["n_total"]
    pos = np.concatenate([m[1]["pos"].ravel(order="F") for m in members])
    vel = np.concatenate([m[1]["vel"].ravel(order="F") for m in members])
    drho = np.concatenate([m[1]["drho_dt"] for m in members])
    mass, wv = members[0][1]["mass"], capi.f64(members[0][1]["wall_vel"])
    h = C.c_void_p()
    rc = capi.lib().sphx_batch_create(C.byref(h), C.c_int(2), arr, C.c_int(nf), C.c_int(nt), capi.ptr(pos), capi.ptr(vel),
                                      capi.ptr(drho), capi.ptr(mass), capi.ptr(wv), C.c_double(0.0), C.c_int64(0))
    assert rc == capi.SPHX_ERR_ARG and not h.value
    assert capi.lib().sphx_last_error_id().decode() == "SPHX:Batch:geometry"
    assert b"t_end" in capi.lib().sphx_last_error() and b"member 1" in capi.lib().sphx_last_error()


def test_mismatched_n_total_is_refused(cfgmod, geom, capi):
    members = _members(cfgmod, geom, n=2)
    prm, parts = members[1]
    short = dict(parts, pos=parts["pos"][:-1], vel=parts["vel"][:-1], drho_dt=parts["drho_dt"][:-1])
    members[1] = (prm, short)
    err = _refused(capi, "SPHX:Batch:geometry", lambda: capi.Batch.from_parts(*zip(*members), t_end=1.0))
    assert "member 1" in err.message


def test_different_walls_are_refused(cfgmod, geom, capi):
    members = _members(cfgmod, geom, n=2)
    prm, parts = members[1]
    moved = dict(parts, pos=parts["pos"].copy(order="F"))
    moved["pos"][parts["n_fluid"] + 2, 1] += 1e-3
    members[1] = (prm, moved)
    err = _refused(capi, "SPHX:Batch:geometry", lambda: capi.Batch.from_parts(*zip(*members), t_end=1.0))
    assert "wall positions" in err.message


@pytest.mark.parametrize("kw", [dict(dual_rate=2), dict(dynamic_rebin=1)])
def test_refused_modes(cfgmod, geom, capi, kw):
    _refused(capi, "SPHX:Batch:mode", lambda: capi.Batch.from_parts(*zip(*_members(cfgmod, geom)), t_end=1.0, **kw))


@pytest.mark.parametrize("lpp", [2, 8])
def test_large_channel_lane_counts_are_refused(cfgmod, geom, capi, lpp):
    _refused(capi, "SPHX:Batch:size",
             lambda: capi.Batch.from_parts(*zip(*_members(cfgmod, geom)), t_end=1.0, lanes_per_particle=lpp))


def test_member_count(cfgmod, geom, capi):
    _refused(capi, "SPHX:Batch:members", lambda: capi.Batch([], 10, 20, [], [], [], np.ones(20), np.zeros((20, 2))))
    members = _members(cfgmod, geom, n=2)
    p0 = members[0][1]
    _refused(capi, "SPHX:Batch:members",
             lambda: capi.Batch([m[0] for m in members], p0["n_fluid"], p0["n_total"], [p0["pos"]], [p0["vel"]],
                                [p0["drho_dt"]], p0["mass"], p0["wall_vel"], t_end=1.0))
    arr = (capi.SphxParams * 1)(capi.make_params(members[0][0], t_end=1.0))
    h = C.c_void_p()
    rc = capi.lib().sphx_batch_create(C.byref(h), C.c_int(0), arr, C.c_int(p0["n_fluid"]), C.c_int(p0["n_total"]),
                                      None, None, None, None, None, C.c_double(0.0), C.c_int64(0))
    assert rc == capi.SPHX_ERR_ARG and capi.lib().sphx_last_error_id().decode() == "SPHX:Batch:members"


def test_member_index_is_checked_without_a_batch(capi):
    # a NULL batch is refused before any member lookup
    rc = capi.lib().sphx_batch_download(None, C.c_int(0), None, None, None, None, None, None, None, None, None)
    assert rc == capi.SPHX_ERR_ARG
    assert capi.lib().sphx_last_error_id().decode() == "SPHX:Batch:null"


def test_run_batch_refusals(cfgmod, driver):
    prms = [cfgmod.params_from_values(dp=0.05, DL=3.0, mu=mu) for mu in (0.1, 0.2)]
    with pytest.raises(ValueError, match="resident"):
        driver.run_batch(prms, engine="mex")
    with pytest.raises(ValueError, match="restart"):
        driver.run_batch(prms, restart_path="x.mat")
    with pytest.raises(ValueError, match="restart"):
        driver.run_batch(prms, postprocess_path="x.mat")
    with pytest.raises(ValueError, match="averag"):
        driver.run_batch(prms, average_from=1.0)
    other = cfgmod.params_from_values(dp=0.05, DL=3.0, output_interval=0.5)
    with pytest.raises(ValueError, match="output_interval"):
        driver.run_batch([prms[0], other])
