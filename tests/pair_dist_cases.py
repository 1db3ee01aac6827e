"""Cases, settings and comparisons shared by tests/test_pair_dist_host.py, tests/test_gpu_pair_dist.py and
tests/test_gpu_batch_pair_dist.py (pair statistics, include/sphx.h sections 2l / 2m).  Every comparison of counts is
np.array_equal on integers: no tolerance anywhere."""
import itertools

import numpy as np

import probe_cases

CASES = probe_cases.CASES      # compact, walk, dynamic and dual-rate forms, two columns, one column, 30 k particles, a wide skin
COUNTS = ("ff", "fw")

# the four states of the oracle anchor: (dp, DL, jitter) of make_case(seed=11, developed=True)
ANCHOR = {"lattice": (0.05, 3.0, 0.0), "jittered": (0.05, 3.0, 0.2), "two_cols": (0.1, 0.6, 0.2), "one_col": (0.1, 0.4, 0.2)}

# the lattice at rest, dp = 0.05, DL = 3, h = 1.3 dp, r_max = 2h, 64 bins: 1 200 fluid and 480 wall particles
LATTICE_FF = {24: 4680, 34: 4560, 49: 4560, 55: 8880}   # every other bin is 0; 22 680 = 2 x 11 340 pairs
LATTICE_FW_TOTAL = 1320
LATTICE_BULK = (840, 20.0)                              # centres with 2h <= y <= DH - 2h, partners of each


def bands(prm):
    hw = max(prm.dp, prm.h)
    return [(0.5 * prm.DL, hw), (0.0, hw)]  # mid-channel and the periodic seam


def settings(prm):
    """The sweep of the sample-now test: (n_bins, r_max, y_margin, with_walls), the two x-bands always on."""
    return list(itertools.product((1, 64, 1024), (2.0 * prm.h, 1.2 * prm.dp), (0.0, 2.0 * prm.h), (False, True)))


def numpy_sums(profmod, prm, parts, pos, n_bins, r_max, y_margin, with_walls, xbands, sep=None):
    """profile.pair_histogram of the fluid positions pos [n_fluid, 2] with the walls of parts: one dict per band"""
    nf = parts["n_fluid"]
    return profmod.pair_histogram(pos[:nf], prm.DL, prm.DH, r_max, n_bins, bands=xbands, y_margin=y_margin,
                                  wall_pos=parts["pos"][nf:] if with_walls else None, separations=sep)


def separations(profmod, prm, parts, pos):
    """the pair search of numpy_sums at 2h with the walls, shared between the settings of one state"""
    nf = parts["n_fluid"]
    return profmod.pair_separations(pos[:nf], prm.DL, 2.0 * prm.h, parts["pos"][nf:])


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def assert_counts_equal(got, want, what, head=False):
    """two lists of sums, one dict per band: ff, fw and centres equal, r2_min bit for bit; head: the sample window too"""
    assert len(got) == len(want), what
    for b, (x, y) in enumerate(zip(got, want)):
        for k in COUNTS:
            gx, wy = np.asarray(x[k]), np.asarray(y[k])
            assert gx.dtype == np.int64 and wy.dtype == np.int64, f"{what}: band {b} {k} is not int64"
            assert np.array_equal(gx, wy), f"{what}: band {b} {k}: {int(np.sum(gx != wy))} bins differ, totals {gx.sum()} {wy.sum()}"
        assert int(x["centres"]) == int(y["centres"]), f"{what}: band {b} centres {x['centres']} {y['centres']}"
        assert same_bits(x["r2_min"], y["r2_min"]), f"{what}: band {b} r2_min {x['r2_min']!r} {y['r2_min']!r}"
        assert np.array_equal(x["r_edges"], y["r_edges"]), f"{what}: band {b} r_edges"
        if head:
            assert (x["n_samples"], x["t_first"], x["t_last"]) == (y["n_samples"], y["t_first"], y["t_last"]), f"{what}: band {b} window"


def add_counts(a, b):
    """the integer sums of two lists of sums (one dict per band) added, the smaller r2_min"""
    out = []
    for x, y in zip(a, b):
        out.append(dict(r_edges=x["r_edges"], ff=x["ff"] + y["ff"], fw=x["fw"] + y["fw"], centres=x["centres"] + y["centres"],
                        r2_min=min(x["r2_min"], y["r2_min"])))
    return out


EDGE_R_MAX, EDGE_BINS = 0.125, 64   # bin width 2^-9: every coordinate below and every r2 is exact in binary (2h = 0.13 at dp = 0.05)
EDGE_KS = (1, 2, 7, 31, 63)          # pairs at dx = k * 2^-9: r2 = e2[k] exactly, and the lower edge is inclusive: bin k


def edge_pairs(y=0.5):
    """Hand-placed pairs [(a, b), ...] with dy = 0: dx = k * (EDGE_R_MAX / EDGE_BINS) for k in EDGE_KS, then dx = EDGE_R_MAX
    (r2 = e2[n_bins]: not counted) and dx = 0 (coincident: bin 0).  The pairs are 0.375 apart in x: none meets another."""
    w = EDGE_R_MAX / EDGE_BINS
    dxs = [k * w for k in EDGE_KS] + [EDGE_R_MAX, 0.0]
    return [((0.25 + 0.375 * i, y), (0.25 + 0.375 * i + dx, y)) for i, dx in enumerate(dxs)]


def edge_bins():
    """the ff histogram of edge_pairs() alone: both particles of a pair are centres, so a counted pair counts twice"""
    want = np.zeros(EDGE_BINS, dtype=np.int64)
    for k in EDGE_KS + (0,):
        want[k] += 2
    return want
