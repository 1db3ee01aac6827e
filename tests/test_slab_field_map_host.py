"""Field maps of a slab ring (include/sphx.h section 3a) without a GPU: the C ABI declares and exports the four entry points,
the engine has the field_part_* methods (and none of a context's field_map_* names), slab.pool_ring_field_map puts the ranks'
blocks of node columns side by side -- bit for bit the unsplit planes -- and refuses blocks that do not partition the grid or
ranks that disagree about the samples, and slab.all_reduce_ring_field_map does the same between two gloo processes on the
CPU."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_field_map_worker.py")
SYMBOLS = ("sphx_slab_field_map_enable", "sphx_slab_field_map_disable", "sphx_slab_field_map_reset", "sphx_slab_field_map_read")
PLANES = ("count", "sum_w", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")
HEAD = dict(n_samples=1, t_first=0.25, t_last=0.25)


@pytest.fixture(scope="module")
def slab(pkg):
    return importlib.import_module(pkg.__name__ + ".slab")


def test_slab_field_map_symbols_declared_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "sphx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(sphx_[a-z0-9_]+)\s*\(", hdr))
    assert "3a. Samplers of a slab ring" in raw and "no field map on slabs" not in raw
    for name in SYMBOLS:
        assert name in declared and name in capi.EXPORTS
        getattr(capi.lib(), name)


def test_engine_has_the_field_part_methods_under_names_of_their_own(slab):
    eng = slab.HipSlabEngine
    for name in ("field_part_enable", "field_part_disable", "field_part_reset", "field_part_sums"):
        assert callable(getattr(eng, name)), name
    for name in ("flow_stats_sample", "field_map_enable", "field_map_sums"):  # a slab holds a PART of a map
        assert not hasattr(eng, name), name
    for name in ("pool_ring_field_map", "ring_field_map", "all_reduce_ring_field_map"):
        assert callable(getattr(slab, name)), name


def _whole(profmod, seed=3, n=800, DL=3.0, DH=1.0, h=0.13, nx=17, ny=7):
    """The six planes of one sample of a random particle set over all nodes ([ny, nx]; some nodes near the ends of y are void)."""
    rng = np.random.default_rng(seed)
    pos = np.column_stack([rng.uniform(0.0, DL, n), rng.uniform(0.3, DH - 0.05, n)])
    vel = np.column_stack([rng.normal(1.0, 0.3, n), rng.normal(0.0, 0.1, n)])
    f = profmod.shepard_field(pos, vel, DL, DH, h, nx, ny)
    hit = f["S0"] > 0.0
    z = lambda v: np.where(hit, v, 0.0)
    return dict(zip(PLANES, (hit.astype(np.float64), z(f["S0"]), z(f["u_x"]), z(f["u_y"]), z(f["u_x"] ** 2), z(f["u_y"] ** 2))))


def _cut(whole, ranges, head=HEAD):
    ny, nx = whole["count"].shape
    return [dict({k: np.ascontiguousarray(whole[k][:, lo:hi]) for k in PLANES}, i_lo=lo, i_hi=hi, nx=nx, ny=ny, **head)
            for lo, hi in ranges]


def test_pool_ring_field_map_puts_the_blocks_side_by_side(profmod, slab):
    whole = _whole(profmod)
    assert 0 < whole["count"].sum() < whole["count"].size  # hit and void nodes
    for ranges in (((0, 6), (6, 11), (11, 17)), ((0, 9), (9, 9), (9, 17)), ((0, 0), (0, 17), (17, 17))):  # (an empty block is fine)
        got = slab.pool_ring_field_map(_cut(whole, ranges))
        for k in PLANES:
            assert got[k].shape == whole[k].shape and got[k].tobytes() == whole[k].tobytes(), (ranges, k)
        assert (got["n_samples"], got["t_first"], got["t_last"]) == (1, 0.25, 0.25)
    nan = float("nan")
    empty = _cut({k: np.zeros_like(v) for k, v in whole.items()}, ((0, 6), (6, 17)), dict(n_samples=0, t_first=nan, t_last=nan))
    assert slab.pool_ring_field_map(empty)["n_samples"] == 0  # no sample yet: NaN times on every rank agree


def test_pool_ring_field_map_means_go_into_field_means(profmod, slab):
    whole = _whole(profmod)
    pooled = slab.pool_ring_field_map(_cut(whole, ((0, 6), (6, 11), (11, 17))))
    a, b = profmod.field_map_means(3.0, 1.0, **pooled), profmod.field_map_means(3.0, 1.0, **dict(whole, **HEAD))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("what,ranges", [("gap", ((0, 6), (7, 11), (11, 17))), ("overlap", ((0, 6), (5, 11), (11, 17))),
                                         ("short", ((0, 6), (6, 11), (11, 16))), ("long", ((0, 6), (6, 11), (11, 18))),
                                         ("late start", ((1, 6), (6, 11), (11, 17)))])
def test_pool_ring_field_map_refuses_blocks_that_do_not_partition(profmod, slab, what, ranges):
    whole = _whole(profmod)
    wide = {k: np.pad(v, ((0, 0), (0, 1))) for k, v in whole.items()}  # (so that every block has the shape its range says)
    parts = [dict(p, nx=17) for p in _cut(wide, ranges)]
    with pytest.raises(ValueError):
        slab.pool_ring_field_map(parts)


def test_pool_ring_field_map_refuses_shapes_and_heads_that_disagree(profmod, slab):
    whole = _whole(profmod)
    ranges = ((0, 6), (6, 11), (11, 17))
    parts = _cut(whole, ranges)
    parts[1] = dict(parts[1], sum_ux=parts[1]["sum_ux"][:, :-1])  # a plane narrower than its block
    with pytest.raises(ValueError):
        slab.pool_ring_field_map(parts)
    parts = _cut(whole, ranges)
    parts[2] = dict(parts[2], **{k: parts[2][k][:-1] for k in PLANES}, ny=6)  # another ny
    with pytest.raises(ValueError, match="rank 2"):
        slab.pool_ring_field_map(parts)
    parts = _cut(whole, ranges)
    parts[1] = dict(parts[1], nx=18)
    with pytest.raises(ValueError, match="rank 1"):
        slab.pool_ring_field_map(parts)
    for key, value in (("n_samples", 2), ("t_first", 0.125), ("t_last", 0.5)):
        parts = _cut(whole, ranges)
        parts[1] = dict(parts[1], **{key: value})
        with pytest.raises(ValueError, match="rank 1"):
            slab.pool_ring_field_map(parts)
    with pytest.raises(ValueError):
        slab.pool_ring_field_map([])


def test_all_reduce_ring_field_map_in_two_gloo_processes():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29598", WORKER]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("OK") == 2, r.stdout
