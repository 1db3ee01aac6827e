// sphx_devtest.hip -- TEST-ONLY harness: the small __device__ functions of the production headers, each called alone.
//
// Built into csrc/libsphx_devtest.so (build.py), never linked into libsphx.so and not part of its C ABI.  It includes the
// production headers and calls the production functions -- no formula is restated here -- so tests/test_gpu_device_*.py can
// compare every one of them with an exact reference on hand-placed inputs (tests/device_cases.py).
//
// Layout of the element-wise entries (sphx_devtest_formulas / _geometry / _codecs / _lanes / _bins): element i of n reads
// column c of the double inputs at din[c * n + i], of the int inputs at iin[c * n + i], and writes its results the same way
// to dout / iout; dpar / ipar are up to kPars scalars shared by all elements.  kOps states how many columns an operation
// takes and gives; an entry refuses any other count, and an operation of another family.
//
// Rules the kernels keep:
//   * no result of a function under test is ever used as an address: results are only written out, to the element's own
//     place.  A wrong helper gives a wrong number, never a stray access;
//   * functions that take pointers get buffers sized here from the inputs, and the host entry checks every row, column and
//     count before it launches (hipErrorInvalidValue otherwise);
//   * blocks of kBlock = 256 threads, and whole blocks for the lane-group and block primitives (n a multiple of 256), so they
//     see full wavefronts.  The one-workgroup scan and the big-scan kernels are launched as the host's cell scan launches
//     them (launch_scan_around, sphx_resident.hip): kScanBlock threads, a null clock.
#include <vector>

#include "sphx_common.hpp"
#include "sphx_kernels.hpp"
#include "sphx_flow_stats.hpp"
#include "sphx_pair_dist.hpp"
#include "sphx_grad_stats.hpp"

#define DEVTEST_API extern "C" __attribute__((visibility("default")))

namespace sphx {
namespace devtest {

constexpr int kPars = 8;

enum Op : int {
    // formulas (sphx_device.hpp, half_state)
    F_RCP_NR = 0, F_RSQRT_NR, F_PAIR_GEOM, F_SPLINE, F_SPLINE_DW, F_SPLINE_W, F_SPLINE_DW_SEL, F_SPLINE_DW_IN, F_SPLINE_W_SEL,
    F_KGC_MOMENT_ADD, F_CONTINUITY_ADD, F_WALL_PAIR, F_WALL_PRESSURE_ADD, F_KGC_FROM_A, F_RIEMANN_BETA, F_TRANSPORT_SHIFT,
    F_DENSITY_FROM_SIGMA, F_HALF_STATE, F_EOS_PRESSURE,
    // geometry and the clock
    G_WRAP_X, G_CELL_OF, G_MIN_IMAGE, G_NEIGHBOUR_COLUMN, G_REBIN_NEAR, G_OWNS, G_TRACKED_DRIFT2, G_NEXT_DT, G_LOOP_CONTINUES,
    // list codecs and the tile layout
    C_LIST_ROW_COUNTS, C_ENCODE_DELTA, C_WORD_HALVES, C_WRAP_INDEX, C_TILE_SLOT, C_TILE_INDEX, C_TILE_CAPPED, C_CODED_INDEX,
    // lane groups, waves, the block scan
    L_GROUP_SUM, L_GROUP_EXTREME, L_WAVE_MAX, L_PAIR_PARTNER, L_BLOCK_SCAN_T,
    // bins and fixed point
    B_STATS_BIN, B_STATS_IN_BAND, B_PAIR_R2, B_PAIR_EDGE2, B_PAIR_BIN, B_STATS_SCALES, B_GRAD_SCALES, B_QUANTISE,
    N_OPS
};

struct OpInfo {
    int kdi, kii, kdo, kio;  // columns: double in, int in, double out, int out
};
// (one line per Op, in its order)
constexpr OpInfo kOps[N_OPS] = {
    {1, 0, 1, 0},   // F_RCP_NR            x -> 1/x
    {1, 0, 1, 0},   // F_RSQRT_NR          x -> 1/sqrt(x)
    {2, 0, 3, 0},   // F_PAIR_GEOM         dx dy -> r ex ey
    {1, 0, 2, 0},   // F_SPLINE            r -> W dW              dpar: h inv_h sigma sigma_over_h rcut2 (all spline forms)
    {1, 0, 1, 0},   // F_SPLINE_DW         r -> dW
    {1, 0, 1, 0},   // F_SPLINE_W          r -> W
    {1, 0, 1, 0},   // F_SPLINE_DW_SEL     r -> dW
    {1, 0, 1, 0},   // F_SPLINE_DW_IN      r -> dW
    {1, 0, 1, 0},   // F_SPLINE_W_SEL      r -> W
    {3, 0, 4, 0},   // F_KGC_MOMENT_ADD    dx dy Volj -> a11 a12 a21 a22 (added to zeros)          dpar: kernel constants
    {7, 0, 1, 0},   // F_CONTINUITY_ADD    dx dy vxi vyi ujx ujy Volj -> rate (added to zero)       dpar: kernel constants
    {7, 0, 5, 0},   // F_WALL_PAIR         dx dy Volw b11 b12 b21 b22 -> r dWVj tx ty eBe           dpar: kernel constants
    {11, 0, 2, 0},  // F_WALL_PRESSURE_ADD dx dy Volw b11 b12 b21 b22 acx acy p_i rhoh_i -> px py   dpar: kernel constants
    {4, 0, 4, 0},   // F_KGC_FROM_A        a11 a12 a21 a22 -> b11 b12 b21 b22
    {3, 0, 1, 0},   // F_RIEMANN_BETA      un_l un_r c_f -> beta
    {4, 0, 2, 0},   // F_TRANSPORT_SHIFT   inc_x inc_y h coeff -> sx sy
    {5, 0, 1, 0},   // F_DENSITY_FROM_SIGMA sigma_inner sigma_contact mass rho0 inv_sigma0 -> rho
    {5, 0, 2, 0},   // F_HALF_STATE        rho drho dt rho0 p0 -> rho_half p_half
    {3, 0, 1, 0},   // F_EOS_PRESSURE      rho rho0 p0 -> p
    {2, 0, 1, 0},   // G_WRAP_X            x DL -> x wrapped
    {2, 0, 0, 2},   // G_CELL_OF           x y -> cx cy          dpar: x0 y0 inv_csx inv_csy DL; ipar: ncx ncy wrap_first
    {1, 0, 1, 0},   // G_MIN_IMAGE         dx -> dx folded       dpar: DL half_DL
    {0, 4, 0, 3},   // G_NEIGHBOUR_COLUMN  ncx cx ox periodic -> ok col duplicate_column
    {0, 5, 0, 1},   // G_REBIN_NEAR        ncx ncy periodic c_old c_new -> near
    {1, 1, 0, 1},   // G_OWNS              x | cell -> owns      dpar: own_lo own_hi; ipar: own_by_cell ncy own_c0 own_c1
    {4, 1, 1, 0},   // G_TRACKED_DRIFT2    xo yo pbx pby | cell -> d2   dpar: DL half_DL; ipar: own_by_cell ncy own_c0 own_c1
    {8, 1, 1, 0},   // G_NEXT_DT           t t_target t_end vmax h c_f dt_viscous dt_body | n_in -> dt
    {2, 3, 0, 1},   // G_LOOP_CONTINUES    t t_target | steps_left status need_rebuild -> continues
    {0, 3, 0, 3},   // C_LIST_ROW_COUNTS   cnt cnt_fl sub -> packed list_rows list_fluid_rows        ipar: LPP
    {0, 5, 0, 3},   // C_ENCODE_DELTA      k i n periodic limit -> d flag wrap_index(i + d, n)
    {0, 1, 0, 4},   // C_WORD_HALVES       word -> delta_lo delta_hi code_lo code_hi
    {0, 2, 0, 1},   // C_WRAP_INDEX        k n -> index
    {0, 7, 0, 1},   // C_TILE_SLOT         lo0 lo1 lo2 len0 len1 len2 k -> slot
    {0, 7, 0, 2},   // C_TILE_INDEX        lo0 lo1 lo2 len0 len1 len2 sl -> index ranges_index
    {0, 8, 0, 5},   // C_TILE_CAPPED       lo0 lo1 lo2 len0 len1 len2 cap sl -> total index(sl) len0 len1 len2 of capped(cap)
    {0, 9, 0, 1},   // C_CODED_INDEX       lo0 lo1 lo2 len0 len1 len2 code i n -> index
    {1, 0, 1, 0},   // L_GROUP_SUM         v -> sum over the lane group                     ipar: LPP
    {0, 1, 0, 1},   // L_GROUP_EXTREME     v -> extreme over the lane group                 ipar: LPP MAX
    {1, 0, 1, 0},   // L_WAVE_MAX          v -> max over the wave
    {0, 1, 0, 1},   // L_PAIR_PARTNER      v -> the partner lane's v
    {0, 1, 0, 2},   // L_BLOCK_SCAN_T      v -> exclusive prefix within the block, block total   (block_exclusive_scan_t<kBlock>)
    {1, 0, 0, 1},   // B_STATS_BIN         y -> bin              dpar: bin_w; ipar: n_bins
    {1, 0, 0, 1},   // B_STATS_IN_BAND     x -> member           dpar: DL xc hw
    {2, 0, 1, 0},   // B_PAIR_R2           dx dy -> r2
    {0, 1, 1, 0},   // B_PAIR_EDGE2        k -> e2               dpar: bin_w
    {1, 0, 0, 1},   // B_PAIR_BIN          r2 -> bin             dpar: bin_w; ipar: n_bins
    {1, 1, 1, 2},   // B_STATS_SCALES      vmax | n -> bound | s1 s2
    {2, 1, 1, 3},   // B_GRAD_SCALES       vmax h | n -> bound | s1 s2 s3
    {1, 1, 0, 2},   // B_QUANTISE          g | s -> low word, high word of __double2ll_rn(ldexp(g, s))
};

struct Cols {
    const double *din;
    const int *iin;
    double *dout;
    int *iout;
    int n;
};
struct Pars {
    double d[kPars];
    int i[kPars];
};

template <int LPP>
__device__ __forceinline__ int extreme_of(int v, bool mx)
{
    return mx ? group_extreme<LPP, true>(v) : group_extreme<LPP, false>(v);
}

__global__ __launch_bounds__(kBlock) void k_map(int op, Cols c, Pars p)
{
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    const bool live = i < c.n;
    if (op < L_GROUP_SUM || op > L_BLOCK_SCAN_T) {
        if (!live) return;  // (the lane and block primitives run in whole blocks: every thread takes part)
    }
    const size_t n = (size_t)c.n;
    auto D = [&](int col) { return c.din[col * n + i]; };
    auto I = [&](int col) { return c.iin[col * n + i]; };
    auto outD = [&](int col, double v) { c.dout[col * n + i] = v; };
    auto outI = [&](int col, int v) { c.iout[col * n + i] = v; };
    const KernelConst kc{p.d[0], p.d[1], p.d[2], p.d[3], p.d[4]};  // (where the operation's dpar are the kernel constants)
    auto grid_own = [&]() {
        Grid g{};
        g.own_by_cell = p.i[0]; g.ncy = p.i[1]; g.own_c0 = p.i[2]; g.own_c1 = p.i[3];
        return g;
    };
    auto tile_map = [&]() { return TileMap{I(0), I(1), I(2), I(3), I(4), I(5)}; };
    switch (op) {
    case F_RCP_NR: outD(0, rcp_nr(D(0))); break;
    case F_RSQRT_NR: outD(0, rsqrt_nr(D(0))); break;
    case F_PAIR_GEOM: {
        const PairGeom pg = pair_geom(D(0), D(1));
        outD(0, pg.r); outD(1, pg.ex); outD(2, pg.ey);
        break;
    }
    case F_SPLINE: {
        double W, dW;
        spline(kc, D(0), W, dW);
        outD(0, W); outD(1, dW);
        break;
    }
    case F_SPLINE_DW: outD(0, spline_dW(kc, D(0))); break;
    case F_SPLINE_W: outD(0, spline_W(kc, D(0))); break;
    case F_SPLINE_DW_SEL: outD(0, spline_dW_sel(kc, D(0))); break;
    case F_SPLINE_DW_IN: outD(0, spline_dW_in(kc, D(0))); break;
    case F_SPLINE_W_SEL: outD(0, spline_W_sel(kc, D(0))); break;
    case F_KGC_MOMENT_ADD: {
        double a11 = 0.0, a12 = 0.0, a21 = 0.0, a22 = 0.0;
        kgc_moment_add(kc, D(0), D(1), D(2), a11, a12, a21, a22);
        outD(0, a11); outD(1, a12); outD(2, a21); outD(3, a22);
        break;
    }
    case F_CONTINUITY_ADD: {
        double rate = 0.0;
        continuity_add(kc, D(0), D(1), D(2), D(3), D(4), D(5), D(6), rate);
        outD(0, rate);
        break;
    }
    case F_WALL_PAIR: {
        const WallPair w = wall_pair(kc, D(0), D(1), D(2), make_double4(D(3), D(4), D(5), D(6)));
        outD(0, w.r); outD(1, w.dWVj); outD(2, w.tx); outD(3, w.ty); outD(4, w.eBe);
        break;
    }
    case F_WALL_PRESSURE_ADD: {
        double px = 0.0, py = 0.0;
        wall_pressure_add(kc, D(0), D(1), D(2), make_double4(D(3), D(4), D(5), D(6)), D(7), D(8), D(9), D(10), px, py);
        outD(0, px); outD(1, py);
        break;
    }
    case F_KGC_FROM_A: {
        const Mat2 B = kgc_from_A(D(0), D(1), D(2), D(3));
        outD(0, B.m11); outD(1, B.m12); outD(2, B.m21); outD(3, B.m22);
        break;
    }
    case F_RIEMANN_BETA: outD(0, riemann_beta(D(0), D(1), D(2))); break;
    case F_TRANSPORT_SHIFT: {
        double sx, sy;
        transport_shift(D(0), D(1), D(2), D(3), sx, sy);
        outD(0, sx); outD(1, sy);
        break;
    }
    case F_DENSITY_FROM_SIGMA: outD(0, density_from_sigma(D(0), D(1), D(2), D(3), D(4))); break;
    case F_HALF_STATE: {
        Phys ph{};
        ph.rho0 = D(3); ph.p0 = D(4);
        double rhoh, p_half;
        half_state(ph, D(0), D(1), D(2), rhoh, p_half);
        outD(0, rhoh); outD(1, p_half);
        break;
    }
    case F_EOS_PRESSURE: outD(0, eos_pressure(D(0), D(1), D(2))); break;

    case G_WRAP_X: outD(0, wrap_x(D(0), D(1))); break;
    case G_CELL_OF: {
        Grid g{};
        g.x0 = p.d[0]; g.y0 = p.d[1]; g.inv_csx = p.d[2]; g.inv_csy = p.d[3];
        g.ncx = p.i[0]; g.ncy = p.i[1];
        const double x = p.i[2] ? wrap_x(D(0), p.d[4]) : D(0);
        int cx, cy;
        cell_of(g, x, D(1), cx, cy);
        outI(0, cx); outI(1, cy);
        break;
    }
    case G_MIN_IMAGE: {
        Grid g{};
        g.DL = p.d[0]; g.half_DL = p.d[1];
        outD(0, min_image(g, D(0)));
        break;
    }
    case G_NEIGHBOUR_COLUMN: {
        Grid g{};
        g.ncx = I(0); g.periodic = I(3);
        int col;
        const bool ok = neighbour_column(g, I(1), I(2), col);
        outI(0, ok ? 1 : 0); outI(1, col); outI(2, duplicate_column(g, I(2)) ? 1 : 0);
        break;
    }
    case G_REBIN_NEAR: {
        Grid g{};
        g.ncx = I(0); g.ncy = I(1); g.periodic = I(2);
        outI(0, rebin_near(g, I(3), I(4)) ? 1 : 0);
        break;
    }
    case G_OWNS: {
        Grid g = grid_own();
        g.own_lo = p.d[0]; g.own_hi = p.d[1];
        outI(0, owns(g, D(0), I(0)) ? 1 : 0);
        break;
    }
    case G_TRACKED_DRIFT2: {
        Grid g = grid_own();
        g.DL = p.d[0]; g.half_DL = p.d[1];
        FluidSet s{};
        s.cell = const_cast<int *>(c.iin);  // column 0: the cell of slot i, read at the element's own index
        outD(0, tracked_drift2(g, s, i, D(0), D(1), make_double2(D(2), D(3))));
        break;
    }
    case G_NEXT_DT: {
        Clock ck{};
        ck.t = D(0); ck.t_target = D(1); ck.t_end = D(2); ck.vmax = D(3); ck.n_in = I(0);
        Phys ph{};
        ph.kc.h = D(4); ph.c_f = D(5); ph.dt_viscous = D(6); ph.dt_body = D(7);
        outD(0, next_dt(ck, ph));
        break;
    }
    case G_LOOP_CONTINUES: {
        Clock ck{};
        ck.t = D(0); ck.t_target = D(1); ck.steps_left = I(0); ck.status = I(1); ck.need_rebuild = I(2);
        outI(0, loop_continues(ck) ? 1 : 0);
        break;
    }

    case C_LIST_ROW_COUNTS: {
        int w = 0;
        switch (p.i[0]) {
        case 1: w = list_row_counts<1>(I(0), I(1), I(2)); break;
        case 2: w = list_row_counts<2>(I(0), I(1), I(2)); break;
        case 4: w = list_row_counts<4>(I(0), I(1), I(2)); break;
        case 8: w = list_row_counts<8>(I(0), I(1), I(2)); break;
        case 16: w = list_row_counts<16>(I(0), I(1), I(2)); break;
        default: w = list_row_counts<32>(I(0), I(1), I(2)); break;
        }
        outI(0, w); outI(1, list_rows(w)); outI(2, list_fluid_rows(w));
        break;
    }
    case C_ENCODE_DELTA: {
        // (the flag word: the element's own, zero before the launch)
        const int d = encode_delta(I(0), I(1), I(2), I(3) != 0, &c.iout[1 * n + i], I(4));
        outI(0, d); outI(2, wrap_index(I(1) + d, I(2)));
        break;
    }
    case C_WORD_HALVES: outI(0, delta_lo(I(0))); outI(1, delta_hi(I(0))); outI(2, code_lo(I(0))); outI(3, code_hi(I(0))); break;
    case C_WRAP_INDEX: outI(0, wrap_index(I(0), I(1))); break;
    case C_TILE_SLOT: outI(0, tile_map().slot(I(6))); break;
    case C_TILE_INDEX: {
        const TileMap m = tile_map();
        outI(0, m.index(I(6))); outI(1, ranges_index(m.lo0, m.lo1, m.lo2, m.len0, m.len1, I(6)));
        break;
    }
    case C_TILE_CAPPED: {
        const TileMap m = tile_map().capped(I(6));
        outI(0, m.total()); outI(1, m.index(I(7))); outI(2, m.len0); outI(3, m.len1); outI(4, m.len2);
        break;
    }
    case C_CODED_INDEX: outI(0, coded_index(tile_map(), I(6), I(7), I(8))); break;

    case L_GROUP_SUM: {
        const double v = D(0);
        double r = v;
        switch (p.i[0]) {
        case 1: r = group_sum<1>(v); break;
        case 2: r = group_sum<2>(v); break;
        case 4: r = group_sum<4>(v); break;
        case 8: r = group_sum<8>(v); break;
        case 16: r = group_sum<16>(v); break;
        default: r = group_sum<32>(v); break;
        }
        outD(0, r);
        break;
    }
    case L_GROUP_EXTREME: {
        const int v = I(0);
        const bool mx = p.i[1] != 0;
        int r = v;
        switch (p.i[0]) {
        case 1: r = extreme_of<1>(v, mx); break;
        case 2: r = extreme_of<2>(v, mx); break;
        case 4: r = extreme_of<4>(v, mx); break;
        case 8: r = extreme_of<8>(v, mx); break;
        case 16: r = extreme_of<16>(v, mx); break;
        default: r = extreme_of<32>(v, mx); break;
        }
        outI(0, r);
        break;
    }
    case L_WAVE_MAX: outD(0, wave_max(D(0))); break;
    case L_PAIR_PARTNER: outI(0, pair_partner(I(0))); break;
    case L_BLOCK_SCAN_T: {
        __shared__ int s_wave[kBlock / 64 + 1];
        int total;
        const int ex = block_exclusive_scan_t<kBlock>(I(0), total, s_wave);
        outI(0, ex); outI(1, total);
        break;
    }

    case B_STATS_BIN: outI(0, stats_bin(D(0), p.d[0], p.i[0])); break;
    case B_STATS_IN_BAND: outI(0, stats_in_band(D(0), p.d[0], p.d[1], p.d[2]) ? 1 : 0); break;
    case B_PAIR_R2: outD(0, pair_r2(D(0), D(1))); break;
    case B_PAIR_EDGE2: outD(0, pair_edge2(I(0), p.d[0])); break;
    case B_PAIR_BIN: outI(0, pair_bin(D(0), p.d[0], p.i[0])); break;
    case B_STATS_SCALES: {
        int s1, s2;
        double bound;
        stats_scales(D(0), I(0), s1, s2, bound);
        outD(0, bound); outI(0, s1); outI(1, s2);
        break;
    }
    case B_GRAD_SCALES: {
        const GradScales sc = grad_scales(D(0), D(1), I(0));
        outD(0, sc.bound); outI(0, sc.s1); outI(1, sc.s2); outI(2, sc.s3);
        break;
    }
    case B_QUANTISE: {
        const long long v = __double2ll_rn(ldexp(D(0), I(0)));  // as the samplers quantise (stats_bin_sample, k_grad_stats)
        outI(0, (int)(unsigned)((unsigned long long)v & 0xffffffffull)); outI(1, (int)(v >> 32));
        break;
    }
    default: break;
    }
}

// put_delta, then (a second launch) delta_of_row / code_of_row of the same rows
__global__ __launch_bounds__(kBlock) void k_put_delta(int *pk, int stride, const int *row, const int *col, const int *d, int n)
{
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < n) put_delta(pk, stride, row[i], col[i], d[i]);
}
__global__ __launch_bounds__(kBlock) void k_read_rows(const int *pk, int stride, const int *row, const int *col, int *delta, int *code, int n)
{
    const int i = blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < n) {
        delta[i] = delta_of_row(pk, stride, row[i], col[i]);
        code[i] = code_of_row(pk, stride, row[i], col[i]);
    }
}

template <int LPP>
__global__ __launch_bounds__(kBlock) void k_tile_ranges(Grid g, const int *cell, const int *start, int n_now, int cap, int n_blk, int *out)
{
    const int blk = blockIdx.x * kBlock + (int)threadIdx.x;
    if (blk >= n_blk) return;
    FluidSet s{};
    s.cell = const_cast<int *>(cell); s.start = const_cast<int *>(start);
    const TileMap m = tile_ranges<LPP>(g, s, blk, n_now, cap);
    int *o = out + 6 * (size_t)blk;
    o[0] = m.lo0; o[1] = m.lo1; o[2] = m.lo2; o[3] = m.len0; o[4] = m.len1; o[5] = m.len2;
}

// ---- host side ----
struct Run {
    hipError_t err = hipSuccess;
    std::vector<void *> owned;
    bool ok() const { return err == hipSuccess; }
    void note(hipError_t e) { if (err == hipSuccess) err = e; }
    template <typename T>
    T *alloc(size_t count, const T *host)  // a device array of `count` elements: a copy of host[], or zeros
    {
        void *d = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (!ok()) return nullptr;
        note(hipMalloc(&d, bytes));
        if (!ok()) return nullptr;
        owned.push_back(d);
        if (host && count) note(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
        else note(hipMemset(d, 0, bytes));
        return (T *)d;
    }
    template <typename T>
    void back(T *host, const T *dev, size_t count)
    {
        if (ok() && count) note(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
    }
    void launched()
    {
        note(hipGetLastError());
        note(hipDeviceSynchronize());
    }
    int done()
    {
        for (void *d : owned) (void)hipFree(d);
        owned.clear();
        return (int)err;
    }
};

int blocks_of(int n) { return n > 0 ? (n + kBlock - 1) / kBlock : 1; }

int run_map(int first, int last, int op, const double *din, int kdi, const int *iin, int kii, double *dout, int kdo, int *iout,
            int kio, int n, const double *dpar, int ndpar, const int *ipar, int nipar)
{
    if (op < first || op > last || n < 1 || n > (1 << 24)) return (int)hipErrorInvalidValue;
    const OpInfo &o = kOps[op];
    if (kdi != o.kdi || kii != o.kii || kdo != o.kdo || kio != o.kio) return (int)hipErrorInvalidValue;
    if ((kdi && !din) || (kii && !iin) || (kdo && !dout) || (kio && !iout)) return (int)hipErrorInvalidValue;
    if (ndpar < 0 || ndpar > kPars || nipar < 0 || nipar > kPars || (ndpar && !dpar) || (nipar && !ipar)) return (int)hipErrorInvalidValue;
    if (op >= L_GROUP_SUM && op <= L_BLOCK_SCAN_T && n % kBlock != 0) return (int)hipErrorInvalidValue;
    Pars p{};
    for (int k = 0; k < ndpar; ++k) p.d[k] = dpar[k];
    for (int k = 0; k < nipar; ++k) p.i[k] = ipar[k];
    if (op == C_LIST_ROW_COUNTS || op == L_GROUP_SUM || op == L_GROUP_EXTREME) {
        const int l = p.i[0];
        if (!(l == 1 || l == 2 || l == 4 || l == 8 || l == 16 || l == 32)) return (int)hipErrorInvalidValue;
    }
    if ((op == B_STATS_BIN || op == B_PAIR_BIN) && (p.i[0] < 1 || p.i[0] > (1 << 20))) return (int)hipErrorInvalidValue;
    Run r;
    const size_t sn = (size_t)n;
    Cols c{};
    c.n = n;
    c.din = r.alloc<double>(kdi * sn, din);
    c.iin = r.alloc<int>(kii * sn, iin);
    c.dout = r.alloc<double>(kdo * sn, nullptr);
    c.iout = r.alloc<int>(kio * sn, nullptr);
    if (r.ok()) {
        hipLaunchKernelGGL(k_map, dim3(blocks_of(n)), dim3(kBlock), 0, 0, op, c, p);
        r.launched();
    }
    r.back(dout, c.dout, kdo * sn);
    r.back(iout, c.iout, kio * sn);
    return r.done();
}

}  // namespace devtest
}  // namespace sphx

using namespace sphx;
using namespace sphx::devtest;

#define DEVTEST_FAMILY(name, first, last)                                                                                        \
    DEVTEST_API int name(int op, const double *din, int kdi, const int *iin, int kii, double *dout, int kdo, int *iout, int kio, \
                         int n, const double *dpar, int ndpar, const int *ipar, int nipar)                                       \
    {                                                                                                                            \
        return run_map(first, last, op, din, kdi, iin, kii, dout, kdo, iout, kio, n, dpar, ndpar, ipar, nipar);                   \
    }
DEVTEST_FAMILY(sphx_devtest_formulas, F_RCP_NR, F_EOS_PRESSURE)
DEVTEST_FAMILY(sphx_devtest_geometry, G_WRAP_X, G_LOOP_CONTINUES)
DEVTEST_FAMILY(sphx_devtest_codecs, C_LIST_ROW_COUNTS, C_CODED_INDEX)
DEVTEST_FAMILY(sphx_devtest_lanes, L_GROUP_SUM, L_BLOCK_SCAN_T)
DEVTEST_FAMILY(sphx_devtest_bins, B_STATS_BIN, B_QUANTISE)

// the table above, for the Python side: columns of operation `op` -> info[4]; the number of operations
DEVTEST_API int sphx_devtest_op_info(int op, int *info)
{
    if (op < 0 || op >= N_OPS || !info) return -1;
    info[0] = kOps[op].kdi; info[1] = kOps[op].kii; info[2] = kOps[op].kdo; info[3] = kOps[op].kio;
    return N_OPS;
}

DEVTEST_API int sphx_devtest_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

// pk[words] (in: the words before, out: after), words = ceil(rows / 2) * stride; element e stores d[e] at (row[e], col[e]) with
// put_delta and reads it back with delta_of_row and code_of_row.  Two elements must not name the same (row, col).
DEVTEST_API int sphx_devtest_put_delta(int *pk, int rows, int stride, const int *row, const int *col, const int *d, int *delta,
                                       int *code, int n)
{
    if (!pk || !row || !col || !d || !delta || !code || n < 1 || n > (1 << 24) || rows < 1 || stride < 1) return (int)hipErrorInvalidValue;
    const size_t words = (size_t)((rows + 1) / 2) * (size_t)stride;
    if (words > ((size_t)1 << 26)) return (int)hipErrorInvalidValue;
    for (int e = 0; e < n; ++e)
        if (row[e] < 0 || row[e] >= rows || col[e] < 0 || col[e] >= stride) return (int)hipErrorInvalidValue;
    Run r;
    int *d_pk = r.alloc<int>(words, pk);
    const int *d_row = r.alloc<int>(n, row), *d_col = r.alloc<int>(n, col), *d_d = r.alloc<int>(n, d);
    int *d_delta = r.alloc<int>(n, nullptr), *d_code = r.alloc<int>(n, nullptr);
    if (r.ok()) {
        hipLaunchKernelGGL(k_put_delta, dim3(blocks_of(n)), dim3(kBlock), 0, 0, d_pk, stride, d_row, d_col, d_d, n);
        r.launched();
    }
    if (r.ok()) {
        hipLaunchKernelGGL(k_read_rows, dim3(blocks_of(n)), dim3(kBlock), 0, 0, (const int *)d_pk, stride, d_row, d_col, d_delta, d_code, n);
        r.launched();
    }
    r.back(pk, d_pk, words);
    r.back(delta, d_delta, (size_t)n);
    r.back(code, d_code, (size_t)n);
    return r.done();
}

// tile_ranges<lpp> of workgroups 0 .. n_blk-1 on a layout of n_now slots: cell[n_now] (the cell of every slot, 0 <= cell <
// ncx * ncy), start[ncx * ncy + 1] (read as values only) -> out[n_blk][6] = lo0 lo1 lo2 len0 len1 len2
DEVTEST_API int sphx_devtest_tile_ranges(int lpp, int ncx, int ncy, int periodic, const int *cell, const int *start, int n_now,
                                         int cap, int n_blk, int *out)
{
    if (!cell || !start || !out || ncx < 1 || ncy < 1 || (long long)ncx * ncy > (1 << 20) || n_now < 1 || n_now > (1 << 24) ||
        n_blk < 1 || n_blk > (1 << 20) || cap < 0)
        return (int)hipErrorInvalidValue;
    if (!(lpp == 1 || lpp == 2 || lpp == 4 || lpp == 8)) return (int)hipErrorInvalidValue;
    const int ncells = ncx * ncy;
    for (int k = 0; k < n_now; ++k)
        if (cell[k] < 0 || cell[k] >= ncells) return (int)hipErrorInvalidValue;
    Grid g{};
    g.ncx = ncx; g.ncy = ncy; g.ncells = ncells; g.periodic = periodic ? 1 : 0;
    Run r;
    const int *d_cell = r.alloc<int>(n_now, cell), *d_start = r.alloc<int>((size_t)ncells + 1, start);
    int *d_out = r.alloc<int>(6 * (size_t)n_blk, nullptr);
    if (r.ok()) {
        const dim3 gr(blocks_of(n_blk)), bl(kBlock);
        switch (lpp) {
        case 1: hipLaunchKernelGGL(k_tile_ranges<1>, gr, bl, 0, 0, g, d_cell, d_start, n_now, cap, n_blk, d_out); break;
        case 2: hipLaunchKernelGGL(k_tile_ranges<2>, gr, bl, 0, 0, g, d_cell, d_start, n_now, cap, n_blk, d_out); break;
        case 4: hipLaunchKernelGGL(k_tile_ranges<4>, gr, bl, 0, 0, g, d_cell, d_start, n_now, cap, n_blk, d_out); break;
        default: hipLaunchKernelGGL(k_tile_ranges<8>, gr, bl, 0, 0, g, d_cell, d_start, n_now, cap, n_blk, d_out); break;
        }
        r.launched();
    }
    r.back(out, d_out, 6 * (size_t)n_blk);
    return r.done();
}

// scan_counts by one workgroup (k_scan_only, a null clock): count[n] -> start[n + 1]
DEVTEST_API int sphx_devtest_scan_counts(const int *count, int *start, int n)
{
    if (!count || !start || n < 1 || n > (1 << 22)) return (int)hipErrorInvalidValue;
    Run r;
    const int *d_count = r.alloc<int>(n, count);
    int *d_start = r.alloc<int>((size_t)n + 1, nullptr);
    if (r.ok()) {
        hipLaunchKernelGGL(k_scan_only, dim3(1), dim3(kScanBlock), 0, 0, (const Clock *)nullptr, 0, d_count, d_start, n);
        r.launched();
    }
    r.back(start, d_start, (size_t)n + 1);
    return r.done();
}

// the three kernels of the big scan in the host's order (launch_scan_around): k_scan_tiles, the one-workgroup scan of the tile
// sums, k_scan_add -- count[n] -> start[n + 1]
DEVTEST_API int sphx_devtest_big_scan(const int *count, int *start, int n)
{
    if (!count || !start || n < 1 || n > (1 << 22)) return (int)hipErrorInvalidValue;
    const int n_tiles = (n + kScanBlock - 1) / kScanBlock;
    Run r;
    const int *d_count = r.alloc<int>(n, count);
    int *d_start = r.alloc<int>((size_t)n + 1, nullptr);
    int *tile_sum = r.alloc<int>(n_tiles, nullptr), *tile_off = r.alloc<int>((size_t)n_tiles + 1, nullptr);
    const Clock *no_clock = nullptr;
    if (r.ok()) {
        hipLaunchKernelGGL(k_scan_tiles, dim3(n_tiles), dim3(kScanBlock), 0, 0, no_clock, 0, d_count, d_start, tile_sum, n);
        hipLaunchKernelGGL(k_scan_only, dim3(1), dim3(kScanBlock), 0, 0, no_clock, 0, (const int *)tile_sum, tile_off, n_tiles);
        hipLaunchKernelGGL(k_scan_add, dim3(n_tiles), dim3(kScanBlock), 0, 0, no_clock, 0, d_start, (const int *)tile_off, n, n_tiles);
        r.launched();
    }
    r.back(start, d_start, (size_t)n + 1);
    return r.done();
}
