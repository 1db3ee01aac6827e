"""The device index helpers one by one (gpu): list codecs, the tile layout, lane-group and block primitives, bins and fixed-point
scales of csrc/sphx_kernels.hpp, sphx_flow_stats.hpp, sphx_pair_dist.hpp and sphx_grad_stats.hpp, called alone through the
harness library (tests/devtest.py).  Everything here is exact: the references are plain Python / numpy statements of the rule
(tests/device_cases.py), and a result either is the reference's or is wrong.

Each test prints `function: worst error ... (allowed ...)` -- here the number of wrong values, allowed 0."""
from fractions import Fraction

import numpy as np
import pytest

import dense_cases
import device_cases as dc
import devtest

pytestmark = pytest.mark.gpu
na = np.nextafter


def report(name, wrong, of):
    print("%s: worst error %d wrong of %d (allowed 0)" % (name, int(wrong), int(of)))


def same(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    wrong = got != ref
    report(name, wrong.sum(), wrong.size)
    assert not wrong.any(), (name, np.argwhere(wrong)[:3].tolist(), got[wrong][:3], ref[wrong][:3])


# ---- C. list codecs and the tile layout ----
@pytest.mark.parametrize("lpp", (1, 2, 4, 8, 16, 32))
def test_list_row_counts(lpp):
    cols, rows, fluid = dc.row_count_cases(lpp, dense_cases.LIST_CAPACITY[lpp])
    _, (packed, got_rows, got_fluid) = devtest.call("C_LIST_ROW_COUNTS", i=list(cols), ipar=[lpp])
    same("list_rows<%d>" % lpp, got_rows, rows)
    same("list_fluid_rows<%d>" % lpp, got_fluid, fluid)
    assert not np.any(packed & 0xC000)  # bits 14 and 15 (kFarForcesBit, kFarTileBit) stay clear
    # over the lanes of a group the rows add up to the list
    cnt, cnt_fl, sub = cols
    key = cnt.astype(np.int64) * 100000 + cnt_fl
    for k in np.unique(key)[:: max(1, np.unique(key).size // 200)]:
        m = key == k
        assert got_rows[m].sum() == cnt[m][0] and got_fluid[m].sum() == cnt_fl[m][0] and m.sum() == lpp


@pytest.mark.parametrize("odd_row", (0, 1))
def test_put_delta_round_trip_of_every_16_bit_value(odd_row):
    stride, rows = 4099, 32  # an odd stride; 16 words down, so 65 584 halves of either parity
    rng = np.random.default_rng(310 + odd_row)
    words = (rows // 2) * stride
    before = rng.integers(-2 ** 31, 2 ** 31, words, dtype=np.int64).astype(np.int32)
    v = np.arange(65536)
    rng.shuffle(v)
    e = np.arange(65536)
    row, col = 2 * (e // stride) + odd_row, e % stride
    for as_code in (0, 1):  # a signed difference, or the same bits as an unsigned code
        d = v if as_code else np.where(v >= 32768, v - 65536, v)
        after, delta, code = devtest.put_delta(before, rows, stride, row, col, d)
        same("delta_of_row (row parity %d)" % odd_row, delta, np.where(v >= 32768, v - 65536, v))
        same("code_of_row (row parity %d)" % odd_row, code, v)
        assert delta.min() == -32768 and delta.max() == 32767 and code.min() == 0 and code.max() == 65535
        b16, a16 = before.view(np.uint16).reshape(-1, 2), after.view(np.uint16).reshape(-1, 2)
        same("put_delta: the other half of every word", a16[:, 1 - odd_row], b16[:, 1 - odd_row])
        written = np.zeros(words, dtype=bool)
        written[(row // 2) * stride + col] = True
        same("put_delta: words it was not asked to touch", after[~written], before[~written])
        same("put_delta: the half it writes", a16[(row // 2) * stride + col, odd_row], v.astype(np.uint16))


def test_word_halves():
    rng = np.random.default_rng(311)
    w = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 4000, dtype=np.int64), [0, -1, 0x7fff, 0x8000, 0xffff, 0x10000, 0x7fff0000, -2 ** 31, 0x8000 << 16 | 0x8000]])
    w = (w & 0xffffffff).astype(np.uint32).view(np.int32)
    _, (dlo, dhi, clo, chi) = devtest.call("C_WORD_HALVES", i=[w])
    u = w.view(np.uint32).astype(np.int64)
    lo, hi = u & 0xffff, u >> 16
    same("delta_lo", dlo, np.where(lo >= 32768, lo - 65536, lo))
    same("delta_hi", dhi, np.where(hi >= 32768, hi - 65536, hi))
    same("code_lo", clo, lo)
    same("code_hi", chi, hi)


def test_encode_delta_and_wrap_index():
    cols = dc.encode_cases()
    k, i, n, per, lim = cols.astype(np.int64)
    _, (d, flag, back) = devtest.call("C_ENCODE_DELTA", i=list(cols))
    d = d.astype(np.int64)
    same("encode_delta: wrap_index(i + d, n) == k", back, k)
    same("encode_delta: open grids store k - i", d[per == 0], (k - i)[per == 0])
    assert np.all(np.abs(d[per == 1]) <= (n >> 1)[per == 1])  # periodic: the representative nearest to zero
    same("encode_delta: flag raised exactly beyond the limit", flag, (np.abs(d) > lim).astype(int))
    on = np.abs(d) == lim
    assert on.sum() >= 8 and not flag[on].any()  # +-limit itself is accepted


def _tile_cols(layouts, extra):
    """One row per (layout, extra value) -> the int columns lo0 .. len2, extra."""
    rows = [tuple(m) + tuple(x) for m, xs in zip(layouts, extra) for x in xs]
    return np.array(rows, dtype=np.int32).T, rows


def test_tile_map_slot_index_capped():
    L = dc.tile_layouts()
    # index, ranges_index of every staged slot; slot of it is the slot again
    cols, rows = _tile_cols(L, [[(sl,) for sl in range(m[3] + m[4] + m[5])] for m in L])
    _, (index, ridx) = devtest.call("C_TILE_INDEX", i=list(cols))
    ref = np.array([dc.tile_index(r[:6], r[6]) for r in rows])
    same("TileMap::index", index, ref)
    same("ranges_index", ridx, ref)
    cols_s = cols.copy()
    cols_s[6] = ref  # (the reference's index, not the device's: no result is fed back)
    _, (slot,) = devtest.call("C_TILE_SLOT", i=list(cols_s))
    same("TileMap::slot(index(sl))", slot, cols[6])
    # just outside every range end: not staged (unless another range holds it)
    out = []
    for m in L:
        held = {dc.tile_index(m, sl) for sl in range(m[3] + m[4] + m[5])}
        ks = {m[j] - 1 for j in range(3)} | {m[j] + m[3 + j] for j in range(3)} | {m[j] - 2 ** 20 for j in range(3)} | {-1, 2 ** 30}
        out.append([(k,) for k in sorted(ks) if k not in held])
    cols_o, rows_o = _tile_cols(L, out)
    _, (slot,) = devtest.call("C_TILE_SLOT", i=list(cols_o))
    same("TileMap::slot outside the ranges", slot, np.full(slot.size, -1))
    # capped(c): a prefix of the same layout
    caps = (0, 1, 16, dc.K_FORCE_SLOTS, dc.K_SLOT_CODES, 100000)
    cols_c, rows_c = _tile_cols(L, [[(c, sl) for c in caps for sl in sorted({0, min(c, sum(m[3:])) // 2, max(min(c, sum(m[3:])) - 1, 0)})] for m in L])
    _, (total, idx, l0, l1, l2) = devtest.call("C_TILE_CAPPED", i=list(cols_c))
    capped = [dc.tile_capped(r[:6], r[6]) for r in rows_c]
    same("capped().total()", total, [min(sum(r[3:6]), r[6]) for r in rows_c])
    same("capped() lengths", np.stack([l0, l1, l2], 1), np.array([c[3:] for c in capped]))
    live = np.array([r[7] < min(sum(r[3:6]), r[6]) for r in rows_c])
    same("capped().index below the cap", idx[live], np.array([dc.tile_index(r[:6], r[7]) for r in rows_c])[live])


def test_tile_map_slot_prefers_the_first_range_that_holds_the_particle():
    cols, rows = _tile_cols(dc.TILE_OVERLAPS, [[(k,) for k in range(min(m[:3]) - 2, max(m[j] + m[3 + j] for j in range(3)) + 2)] for m in dc.TILE_OVERLAPS])
    _, (slot,) = devtest.call("C_TILE_SLOT", i=list(cols))
    same("TileMap::slot on overlapping ranges", slot, [dc.tile_slot_smallest(r[:6], r[6]) for r in rows])


def test_coded_index():
    L = [m for m in dc.tile_layouts() if sum(m[3:]) <= dc.K_SLOT_CODES]
    n = 70001
    # slot codes: every code below the layout's total names index(code), whatever i is
    cols, rows = _tile_cols(L, [[(code, i, n) for code in range(sum(m[3:])) for i in ((0,) if code % 7 else (0, n - 1))] for m in L])
    _, (k,) = devtest.call("C_CODED_INDEX", i=list(cols))
    same("coded_index of slot codes", k, [dc.tile_index(r[:6], r[6]) for r in rows])
    # far codes: the whole range kCodeBias +- kCodedDeltaMax, i near 0, in the middle and near n - 1
    m = L[0]
    codes = np.arange(dc.K_CODE_BIAS - dc.K_CODED_DELTA_MAX, dc.K_CODE_BIAS + dc.K_CODED_DELTA_MAX + 1)
    assert codes.min() >= dc.K_SLOT_CODES and codes.max() <= 65535
    for i in (0, 1, 31000, n // 2, n - 32000, n - 2, n - 1):
        _, (k,) = devtest.call("C_CODED_INDEX", i=[m[0], m[1], m[2], m[3], m[4], m[5], codes, i, n], n=codes.size)
        same("coded_index of far codes, i = %d" % i, k, [dc.wrap_index(i + int(c) - dc.K_CODE_BIAS, n) for c in codes])
    _, (w,) = devtest.call("C_WRAP_INDEX", i=[np.array([-n, -1, 0, n - 1, n, 2 * n - 1]), n])
    same("wrap_index", w, [0, n - 1, 0, n - 1, 0, n - 1])


@pytest.mark.parametrize("lpp", (1, 2, 4, 8))
def test_tile_ranges(lpp):
    per = 256 // lpp
    wrong = total = 0
    for name, ncx, ncy, periodic, cell, start in dc.tile_ranges_cases():
        n = cell.size
        for n_now, cap in ((n, dc.K_SLOT_CODES), (n, dc.K_FORCE_SLOTS), (n, 16), (n - per // 2 - 1, dc.K_SLOT_CODES)):
            n_blk = -(-n // per) + 2  # the last, partial workgroup and two beyond n_now
            got = devtest.tile_ranges(lpp, ncx, ncy, periodic, cell, start, n_now, cap, n_blk)
            ref = np.array([dc.tile_ranges_rule(lpp, ncx, ncy, periodic, cell, start, b, n_now, cap) for b in range(n_blk)])
            wrong += int((got != ref).any(1).sum()); total += n_blk
            assert np.array_equal(got, ref), (name, n_now, cap, np.argwhere((got != ref).any(1))[:3].tolist())
            assert np.all(got[-1] == 0) and np.all(got[:, 3:].sum(1) <= cap)
            # (the cases do what they are for: some workgroup runs across a column end, some layout is cut by the cap)
    report("tile_ranges<%d>" % lpp, wrong, total)


def test_tile_ranges_cases_cross_column_ends_and_hit_the_cap():
    crossing = capped = 0
    for lpp in (1, 2, 4, 8):
        per = 256 // lpp
        for name, ncx, ncy, periodic, cell, start in dc.tile_ranges_cases():
            for b in range(-(-cell.size // per)):
                p0, p1 = b * per, min((b + 1) * per, cell.size) - 1
                crossing += cell[p0] // ncy != cell[p1] // ncy
                full = dc.tile_ranges_rule(lpp, ncx, ncy, periodic, cell, start, b, cell.size, 10 ** 6)
                capped += sum(full[3:]) > dc.K_FORCE_SLOTS
    assert crossing >= 10 and capped >= 10


# ---- D. lane groups, waves, scans ----
@pytest.mark.parametrize("lpp", (1, 2, 4, 8, 16, 32))
def test_group_sum(lpp):
    n = 1024
    lane, group = np.arange(n) % lpp, np.arange(n) // lpp
    v = 2.0 ** lane * (2 * group + 1)  # distinct powers of two times an odd factor per group: every sum is exact
    (s,), _ = devtest.call_whole_blocks("L_GROUP_SUM", [v], ipar=[lpp])
    ref = (2.0 ** lpp - 1) * (2 * group + 1)
    same("group_sum<%d>" % lpp, dc.bits(s), dc.bits(ref))
    assert np.unique(s).size == n // lpp  # every group its own total


@pytest.mark.parametrize("mx", (1, 0))
@pytest.mark.parametrize("lpp", (1, 2, 4, 8, 16, 32))
def test_group_extreme(lpp, mx):
    n = 2048
    rng = np.random.default_rng(320 + lpp)
    lane, group = np.arange(n) % lpp, np.arange(n) // lpp
    v = rng.integers(-1000, 1000, n)
    v[lane == group % lpp] = (5000 + group[lane == group % lpp]) * (1 if mx else -1)  # the extreme in each lane position in turn
    _, (e,) = devtest.call_whole_blocks("L_GROUP_EXTREME", i=[v], ipar=[lpp, mx])
    ref = (5000 + group) * (1 if mx else -1)
    same("group_extreme<%d, %s>" % (lpp, "MAX" if mx else "MIN"), e, ref)


def test_wave_max():
    rng = np.random.default_rng(321)
    v = rng.uniform(0.0, 1.0, (68, 64))
    for w in range(64):
        v[w, w] = 2.0 + w  # the maximum in each of the 64 lanes in turn
    v[64] = 0.0
    v[65] = 0.0; v[65, 37] = 5e-324
    v[66, 5] = np.inf
    v[67] = 0.0; v[67, 63] = 1e-310
    (m,), _ = devtest.call_whole_blocks("L_WAVE_MAX", [v.ravel()])
    same("wave_max", dc.bits(m), dc.bits(np.repeat(v.max(1), 64)))


def test_pair_partner():
    v = np.arange(1024) * 7 + 3
    _, (p,) = devtest.call_whole_blocks("L_PAIR_PARTNER", i=[v])
    same("pair_partner", p, v[np.arange(1024) ^ 1])


@pytest.mark.parametrize("kind", ("random", "zero", "one_cell"))
def test_block_exclusive_scan_t(kind):
    v = dc.scan_inputs(8 * 256, kind)
    _, (ex, total) = devtest.call_whole_blocks("L_BLOCK_SCAN_T", i=[v])
    b = v.reshape(-1, 256).astype(np.int64)
    same("block_exclusive_scan_t<256> prefix, " + kind, ex, (np.cumsum(b, 1) - b).ravel())
    same("block_exclusive_scan_t<256> total, " + kind, total, np.repeat(b.sum(1), 256))


@pytest.mark.parametrize("n", dc.SCAN_SIZES)
def test_scan_counts(n):
    for kind in ("random", "zero", "one_cell"):
        c = dc.scan_inputs(n, kind)
        same("scan_counts n=%d %s" % (n, kind), devtest.scan_counts(c), dc.scan_expected(c))


@pytest.mark.parametrize("n", dc.BIG_SCAN_SIZES)
def test_big_scan(n):
    for kind in ("random", "zero", "one_cell"):
        c = dc.scan_inputs(n, kind)
        start = devtest.big_scan(c)
        same("big scan n=%d %s" % (n, kind), start, dc.scan_expected(c))
        assert start[n] == c.sum()


# ---- E. bins and fixed point ----
@pytest.mark.parametrize("DH", (1.0, 0.7))
@pytest.mark.parametrize("n_bins", (1, 7, 20, 213, 640))
def test_stats_bin(n_bins, DH):
    bin_w, y = dc.stats_bin_inputs(n_bins, DH)
    _, (k,) = devtest.call("B_STATS_BIN", [y], dpar=[bin_w], ipar=[n_bins])
    same("stats_bin n_bins=%d DH=%g" % (n_bins, DH), k, dc.profile_bin(y, DH, n_bins))


@pytest.mark.parametrize("xc_at_seam", (True, False))
def test_stats_in_band(xc_at_seam, profmod):
    DL = 3.0
    for xc, hw in ((0.0 if xc_at_seam else 1.5, 0.25), (0.0 if xc_at_seam else 1.5, 0.0), (0.0 if xc_at_seam else 1.3, 0.1)):
        x = dc.band_inputs(DL, xc, hw)
        _, (m,) = devtest.call("B_STATS_IN_BAND", [x], dpar=[DL, xc, hw])
        same("stats_in_band xc=%g hw=%g" % (xc, hw), m, profmod.in_band(x, DL, xc, hw).astype(int))
        assert m.sum() > 0 and (hw == 0 or m.sum() > 100)


def test_pair_r2_is_numpys_double():
    rng = np.random.default_rng(330)
    dx, dy = rng.uniform(-0.3, 0.3, 100000), rng.uniform(-0.3, 0.3, 100000)
    (r2,), _ = devtest.call("B_PAIR_R2", [dx, dy])
    ref = dx * dx + dy * dy
    same("pair_r2", dc.bits(r2), dc.bits(ref))
    fused = np.array([float(Fraction(a) * Fraction(a) + Fraction(float(b * b))) for a, b in zip(dx[:2000], dy[:2000])])
    assert np.sum(fused != ref[:2000]) > 100  # (the inputs can tell: a fused multiply-add rounds differently on many of them)


@pytest.mark.parametrize("n_bins", (1, 64, 500))
def test_pair_edge2_and_pair_bin(n_bins):
    bin_w, e2, r2 = dc.pair_bin_inputs(n_bins, 0.26)
    k = np.arange(n_bins)
    (edge,), _ = devtest.call("B_PAIR_EDGE2", i=[k], dpar=[bin_w])
    same("pair_edge2 n_bins=%d" % n_bins, dc.bits(edge), dc.bits((k * bin_w) ** 2))
    _, (b,) = devtest.call("B_PAIR_BIN", [r2], dpar=[bin_w], ipar=[n_bins])
    same("pair_bin n_bins=%d" % n_bins, b, np.searchsorted(e2, r2, side="right") - 1)


def _no_overflow(n, bound, s, factor=1):
    return Fraction(int(n)) * factor * Fraction(bound) * Fraction(2) ** int(s) <= 2 ** 62


def test_stats_scales():
    v = dc.scale_vmax()
    vm, nn = np.repeat(v, len(dc.SCALE_N)), np.tile(dc.SCALE_N, v.size)
    (bound,), (s1, s2) = devtest.call("B_STATS_SCALES", [vm], [nn])
    ref = [dc.stats_scales(a, int(b)) for a, b in zip(vm, nn)]
    same("stats_scales", np.stack([s1, s2, dc.bits(bound)], 1), np.array([(r[0], r[1], dc.bits([r[2]])[0]) for r in ref]))
    fin = np.isfinite(vm)
    for a, n, b, e1, e2 in zip(vm[fin], nn[fin], bound[fin], s1[fin], s2[fin]):
        assert b > 2.0 * a and b >= 2.0 ** -59                                # 2^e strictly above 2 vmax
        assert _no_overflow(n, b, e1) and _no_overflow(n, Fraction(b) * Fraction(b), e2)
    assert np.all(bound[vm == 0] == 2.0 ** -59) and np.all(bound[np.isnan(vm)] == 2.0 ** -59)  # the floor


def test_grad_scales(profmod):
    h = dc.h_of(0.05)
    v = dc.scale_vmax(h)
    vm, nn = np.repeat(v, len(dc.SCALE_N)), np.tile(dc.SCALE_N, v.size)
    (bound,), (s1, s2, s3) = devtest.call("B_GRAD_SCALES", [vm, h], [nn])
    ref = [profmod.grad_scales(a, h, int(b)) for a, b in zip(vm, nn)]
    same("grad_scales", np.stack([s1, s2, s3, dc.bits(bound)], 1), np.array([(r["s1"], r["s2"], r["s3"], dc.bits([r["bound"]])[0]) for r in ref]))
    fin = np.isfinite(vm)
    for a, n, b, e1, e2, e3 in zip(vm[fin], nn[fin], bound[fin], s1[fin], s2[fin], s3[fin]):
        assert Fraction(b) > 16 * Fraction(a) / Fraction(h)                   # 2^e strictly above 16 vmax / h
        b2 = Fraction(b) * Fraction(b)
        assert _no_overflow(n, b, e1) and _no_overflow(n, b2, e2) and _no_overflow(n, b2, e3, 4)
    assert np.all(bound[vm == 0] == 2.0 ** -59) and np.all(bound[np.isnan(vm)] == 2.0 ** -59)


def test_quantisation_round_trips_within_half_a_unit():
    rng = np.random.default_rng(331)
    for vmax, n in ((1.5, 5760), (2.0 ** -20, 3), (1e300, 2 ** 31 - 1), (0.0, 1)):
        s1, s2, bound = dc.stats_scales(vmax, n)
        g = np.concatenate([rng.uniform(-bound, bound, 2000), [bound, -bound, 0.0, bound / 3, na(bound, 0.0)]])
        g = np.concatenate([g, -g])
        _, (lo, hi) = devtest.call("B_QUANTISE", [g], [np.full(g.size, s1)])
        q = [(int(h_) << 32) | (int(l_) & 0xffffffff) for l_, h_ in zip(lo, hi)]
        err = max(abs(Fraction(v) * Fraction(2) ** -s1 - Fraction(x)) for v, x in zip(q, g))
        assert err <= Fraction(2) ** -(s1 + 1), float(err)
        half = g.size // 2
        assert q[:half] == [-v for v in q[half:]]                              # -g gives the negative
        assert max(abs(v) for v in q) * n <= 2 ** 62
        print("quantise vmax=%g n=%d: worst error %.3g (allowed %.3g)" % (vmax, n, float(err), 2.0 ** -(s1 + 1)))
