"""The poison-at-free mode of the device-memory pool (include/sphx.h, beside sphx_pool_scrub) and the scene table of
tests/live_worker.py without a GPU: the C ABI declares and exports both calls with the documented signatures, neither needs a
device, and every scene of tests/test_gpu_live_neighbours.py names calls that exist, has moments, and holds objects of one
size -- the counterpart of tests/test_dense_cases.py for these scripts."""
import ctypes as C
import importlib
import os
import re

import live_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {"sphx_pool_poison_on_free": "int sphx_pool_poison_on_free(int on, uint32_t word);",
              "sphx_pool_poison_stats": "int sphx_pool_poison_stats(uint64_t out[2]);"}


def test_poison_symbols_declared_and_exported(capi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sphx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    flat = re.sub(r"\s+", " ", hdr)
    for name, signature in SIGNATURES.items():
        assert name in declared and name in capi.EXPORTS
        assert signature in flat, signature
        getattr(capi.lib(), name)
    assert "int sphx_pool_stats(uint64_t out[4]);" in flat  # the layout of sphx_pool_stats has not changed
    doc = open(os.path.join(ROOT, "include", "sphx.h")).read()
    assert doc.index("sphx_pool_scrub:") < doc.index("sphx_pool_poison_on_free:") < doc.index("int sphx_pool_stats(")


def test_poison_mode_needs_no_device(capi):
    """Toggling the mode makes no HIP call and the counters are plain reads: without a device both calls return SPHX_OK and the
    stats are zeros.  With one, nothing is released in here, so the counters do not move either."""
    L = capi.lib()
    before, pool = capi.pool_poison_stats(), capi.pool_stats()
    assert list(before) == ["filled", "skipped_in_capture"] and all(isinstance(v, int) and v >= 0 for v in before.values())
    try:
        assert L.sphx_pool_poison_on_free(C.c_int(1), C.c_uint32(3)) == capi.SPHX_OK
        out = (C.c_uint64 * 2)(7, 7)
        assert L.sphx_pool_poison_stats(out) == capi.SPHX_OK
        assert [int(v) for v in out] == list(before.values())
        assert capi.pool_scrub(3) <= pool["cached_blocks"]  # (the scrub is not the mode's business)
    finally:
        assert L.sphx_pool_poison_on_free(C.c_int(0), C.c_uint32(0)) == capi.SPHX_OK
    capi.pool_poison_on_free(True)
    capi.pool_poison_on_free(False, word=0xFFFFFFFF)
    assert capi.pool_poison_stats() == before and capi.pool_stats() == pool
    if capi.device_count() == 0:
        assert before == dict(filled=0, skipped_in_capture=0)
    assert L.sphx_pool_poison_stats(None) == capi.SPHX_ERR_ARG and L.sphx_last_error_id().decode() == "SPHX:Pool:args"


def test_scene_table_census(capi):
    """Every call a scene names exists on the class it is called on, every scene has at least one moment, all objects of a
    scene have equal n_total, and the moments are named once."""
    pkg = importlib.import_module("sph-poiseuille-flow_amd")
    where = dict(Context=capi.Context, Batch=capi.Batch, HipSlabEngine=importlib.import_module("sph-poiseuille-flow_amd.slab").HipSlabEngine,
                 mex_surface=pkg.mex_surface, pool=capi)
    assert set(live_worker.SCENES) == {"solo", "samplers_in_flight", "reads_in_flight", "close_in_flight", "neighbour_churn", "ring",
                                       "threads"}
    base = dict(live_worker.phw.BASE)
    try:
        for name, sc in live_worker.SCENES.items():
            assert len(sc["moments"]) >= 1, name
            labels = [m[0] for m in sc["moments"]]
            assert len(set(labels)) == len(labels), name
            for label, cls, call in sc["moments"]:
                assert callable(getattr(where[cls], call, None)), (name, label, cls, call)
            live_worker.phw.BASE = dict(base)
            envs = live_worker.scene_envs(name)
            assert set(envs) == {subject for _, subject in sc["objects"]}
            if sc["state"] == "own":  # (solo: one object at a time, each on the state pool_history_worker gives it)
                continue
            sizes = {(e.parts["n_total"], e.parts["n_fluid"]) for e in envs.values()}
            assert len(sizes) == 1, (name, sizes)
            if sc["state"] == "wall":
                assert sizes == {(2880, next(iter(sizes))[1])}, sizes
            for e in envs.values():
                if e.kind == "batch":
                    prms, parts_list = e.members(e.prm, e.parts)
                    assert len(prms) == 4 and all(p["n_total"] == e.parts["n_total"] for p in parts_list)
    finally:
        live_worker.phw.BASE = base
    # every sampler of a context has its moments: a reallocating enable and a disable, a reset / sample-now / draining read where it has one
    calls = {m[2] for m in live_worker.SCENES["samplers_in_flight"]["moments"]}
    for s, (reset, sample, drain) in live_worker.SAMPLERS.items():
        want = {s + "_enable", s + "_disable"} | ({s + "_reset"} if reset else set()) | ({s + "_sample"} if sample else set()) | ({drain} if drain else set())
        assert want <= calls, (s, want - calls)
        for suffix, has in (("_reset", reset), ("_sample", sample)):
            assert hasattr(capi.Context, s + suffix) == has, (s, suffix)
    assert len(live_worker.SAMPLERS) == 9
