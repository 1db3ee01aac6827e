// sphx_dens_stats.hpp -- density statistics of a resident context (include/sphx.h section 2r), of every member of a batch
// (section 2s, k_dens_stats_b) and of a slab of a ring (section 3a, k_dens_stats_s, at the end): a slot sampler (sphx_slot_sample.hpp) that re-sums, from positions and masses alone, the
// density the next step will start from at every fluid particle, and bins the relative deviation delta = rho / rho0 - 1, its
// square, the volume defect rho0 / rho - 1 and the walls' share of rho / rho0 into the flow statistics' y-bins and x-bands, with
// the running extremes of delta per bin and a histogram of delta per band.  The one sampler that describes the STATE of
// compression (the gradient statistics' div v is its rate): hence the pressure p0 delta and the packing sum m / rho.
// profile.summation_density is the numpy definition, profile.dens_stats_sums the binned sample.
//
// One sample.  For every fluid slot i < clk->n the fluid partners j != i are the fluid slots with kR2Min < r2 < (2h)^2 (nearest
// image, min_image), the wall partners the wall particles in the same range -- always: this is the solver's density:
//     s_in  = W(0) + sum over the fluid partners of W(r_ij)
//     s_ct  = sum over the wall partners of W(r_ij) V_j                       V_j = Walls::a.x
//     rho_i = density_from_sigma(s_in, s_ct, mass_i, rho0, inv_sigma0)         (pass A's function, its floor included)
//     delta_i = rho_i / rho0 - 1,   wall_i = s_ct rho0 inv_sigma0 / mass_i,   dvol_i = rho0 / rho_i - 1
// with pass A's W (spline_W_sel on r2 rsqrt_nr(r2)).  Nothing of FluidTmp is read: rho / Vol there are output-only, written
// lazily and in the layout of the step that made them.  A particle is an OUTLIER -- counted in `outliers`, summed nowhere, in no
// histogram -- when |delta_i| > delta_bound or delta_i is not finite.  y outside [0, DH] is dropped, as the flow statistics drop
// it: per bin and band count + outliers is the flow statistics' count.  Per band a histogram of delta: n_hist uniform bins on
// [-hist_range, hist_range), bin floor((delta + hist_range) * n_hist / (2 hist_range)), `below` and `above` for the rest.
//
// Why the 3 x 3 sweep suffices: the header of sphx_pair_dist.hpp -- partners within 2h now were binned in the same cell or an
// adjacent one.  Only the nearest image counts.
//
// Mapping: pair_dist_body's.  kDensLanes LANES PER PARTICLE sweep the three cell columns around the cell it was binned into,
// rows cy - 1 .. cy + 1, first of the fluid's cell ranges, then of the walls'; lane l takes candidates lo + l, lo + l +
// kDensLanes, ... of each run and keeps two partial sums; a wall candidate's volume is loaded only where it is in range.  The
// partial sums are reduced over the group by __shfl_xor, after which every lane holds the same totals; lane 0 forms rho,
// quantises and does the LDS adds.  A particle's partners are added in SLOT order (lane-strided, then the shuffle tree): the
// sums depend on the layout within the floating-point rounding of s_in and s_ct, not beyond.
//
// Exact sums.  A sample is summed in int64 fixed point as sphx_grad_stats.hpp does, but the scales come from the
// configuration's delta_bound, not from the clock.  With n <= 2^L particles and 2^e >= delta_bound (e <= -1, because
// delta_bound <= 0.5): a summed particle has |delta| <= delta_bound <= 2^e, so delta times 2^(62-L-e) is at most 2^(62-L) and
// delta^2 <= 2^(2e) times 2^(62-L-2e) likewise; dvol = 1 / (1 + delta) - 1 = -delta / (1 + delta) and 1 + delta >= 0.5, so
// |dvol| <= 2 |delta| <= 2^(e+1) and it takes 2^(61-L-e); wall_i >= 0 (W >= 0, V_j > 0, mass_i > 0) and, unless the floor of
// density_from_sigma acted, rho_i / rho0 = s_in inv_sigma0 + wall_i with s_in > 0, so wall_i < 1 + delta <= 1.5 < 2 and it
// takes 2^(61-L) (where the floor acted the whole sum was below 1e-12).  No sum of n <= 2^L such terms exceeds 2^62 in
// magnitude: no overflow.  count, outliers and the histogram are plain integers.  A workgroup keeps its counters in LDS, adds
// the non-zero ones to the global integer sums with one atomic each, and the last workgroup out converts them, adds them to
// the running double sums and clears them; one workgroup finishes a small sample by itself (stats_finish_sample).  d_min and
// d_max go through order-preserving integer keys (dens_key) and integer atomic maxima, first in LDS, then straight into the
// running keys: a maximum needs no sample in flight.  A key of 0 says "no particle yet" (d_max = -inf, d_min = +inf), so
// zeroed memory is the empty state.  Integer adds and maxima commute: the sums do not depend on the dispatch order of the
// workgroups, are bit-identical between runs, and a batch member's are a standalone context's.
#pragma once
#include "sphx_flow_stats.hpp"

namespace sphx {

constexpr int kDensFields = 6;    // per bin and band: count, sum delta, sum delta^2, sum dvol, sum wall, outliers
constexpr int kDensKeys = 2;      // per bin and band: the keys of d_max and of -d_min
constexpr int kDensMaxHist = 1024;
constexpr int kDensBlock = 256;
#ifndef SPHX_EXP_DENS_LANES  // (measurement builds: tools/probes/build_variant_lib.sh dlanes4 -DSPHX_EXP_DENS_LANES=4)
#define SPHX_EXP_DENS_LANES 8
#endif
constexpr int kDensLanes = SPHX_EXP_DENS_LANES;        // lanes per particle (a power of two up to 64)
constexpr int kDensCentres = kDensBlock / kDensLanes;  // particles per workgroup trip
constexpr int kDensTrips = 2;                          // trips a workgroup takes before another is added
constexpr int kDensMaxBlocks = 2048;                   // every workgroup flushes its counters: no more than 8 per CU
constexpr size_t kDensMaxShmem = 60 * 1024;            // the LDS a workgroup may ask for: counters, keys and histograms

// words of LDS of a workgroup: [n_bands][n_bins][kDensFields] counters, [n_bands][n_hist + 2] histogram with below and above
// -- the words that are added -- and [n_bands][n_bins][kDensKeys] keys behind them
__host__ __device__ inline size_t dens_sum_words(int n_bands, int n_bins, int n_hist)
{
    return (size_t)n_bands * ((size_t)n_bins * kDensFields + (size_t)n_hist + 2);
}
__host__ __device__ inline size_t dens_key_words(int n_bands, int n_bins) { return (size_t)n_bands * (size_t)n_bins * kDensKeys; }

struct DensStatsHead {
    long long n_samples;
    double t_first, t_last;
    int ticket;  // last workgroup out (zero between launches)
};

struct DensStatsArgs {
    unsigned long long *isum;  // [block] integer sums of the sample in flight (zero in between)
    double *dsum;              // same layout: running sums over all samples
    unsigned long long *keys;  // [kblock] running keys of d_max and -d_min (0: no particle yet)
    DensStatsHead *head;       // (of a batch: [M]; isum / dsum / keys: member m's block behind member 0's)
    double DH, bin_w, DL;      // bin_w = DH / n_bins, the step of numpy's linspace
    double t_from;
    double delta_bound, hist_range, hist_scale;  // hist_scale = n_hist / (2 hist_range)
    double band_x[2], band_hw[2];
    int n_bins, n_bands;       // n_bands counts band 0 (the whole channel)
    int n_hist;
    int block, kblock;         // words of one channel's sums (dens_sum_words) and keys (dens_key_words)
    int e;                     // 2^e >= delta_bound, e <= -1
    int every;                 // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
};

// the fixed-point scales of one sample of n particles: delta, delta^2, dvol, wall
struct DensScales {
    int s_d, s_d2, s_dvol, s_wall;
};

__host__ __device__ inline DensScales dens_scales(int e, int n)
{
    int L = 0;
    while (L < 31 && (1 << L) < n) ++L;
    return DensScales{62 - L - e, 62 - L - 2 * e, 61 - L - e, 61 - L};
}

// order-preserving key of a finite double, never 0: a < b <=> dens_key(a) < dens_key(b)
__device__ __forceinline__ unsigned long long dens_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// counter k of a sample as the double it stands for: within the binned counters field k % kDensFields, its scale taken back out
__device__ __forceinline__ double dens_value(int k, int n_binned, unsigned long long v, const DensScales &sc)
{
    int s = 0;
    if (k < n_binned) {
        const int f = k % kDensFields;
        s = f == 1 ? sc.s_d : (f == 2 ? sc.s_d2 : (f == 3 ? sc.s_dvol : (f == 4 ? sc.s_wall : 0)));
    }
    return ldexp((double)(long long)v, -s);
}

// The sample of one channel closing the step slot of parity q, on clock clk, by the gridDim.x workgroups of a grid row; s is the
// state the step left (pos, mass and the cell ranges and binned cells of the layout it is stored in); isum / dsum / keys / h are
// that channel's own.
// kSlab: the channel is a slab of a ring -- of the clk->n slots it holds only those it owns (owns()) are particles of the
// sample, every held slot is a partner (k_dens_stats_s).
template <bool kSlab = false>
__device__ __forceinline__ void dens_stats_body(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s, const Walls &w,
                                                const DensStatsArgs &a, unsigned long long *isum, double *dsum, unsigned long long *keys,
                                                DensStatsHead *h)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    const int n = clk->n;
    const double t_now = clk->t;
    const DensScales sc = dens_scales(a.e, n);
    extern __shared__ unsigned long long s_cnt[];  // counters, histograms, keys (dens_sum_words, dens_key_words)
    const int n_binned = a.n_bands * a.n_bins * kDensFields;
    const int nc = a.block, nk = a.kblock;
    unsigned long long *s_hist = s_cnt + n_binned, *s_key = s_cnt + nc;
    for (int k = threadIdx.x; k < nc + nk; k += kDensBlock) s_cnt[k] = 0ull;
    __syncthreads();

    const int lane = (int)threadIdx.x & (kDensLanes - 1), grp = (int)threadIdx.x / kDensLanes;
    // (no barrier inside the loop: a group that has no particle, or whose particle is outside [0, DH], goes on to its next)
    for (long long i0 = (long long)blockIdx.x * kDensCentres + grp; i0 < (long long)n; i0 += (long long)gridDim.x * kDensCentres) {
        const int i = (int)i0;
        const double2 pi = s.pos[i];
        if constexpr (kSlab) {
            if (!owns(g, pi.x, s.cell[i])) continue;  // (a halo copy: its owner bins it)
        }
        if (!(pi.y >= 0.0 && pi.y <= a.DH)) continue;  // outside [0, DH]: dropped, as discretize does
        int cx, cy;
        binned_cell(g, s, i, cx, cy);
        const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
        double s_in = 0.0, s_ct = 0.0;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            int col;
            if (!neighbour_column(g, cx, u - 1, col)) continue;
            const int base = col * g.ncy;
            const int lo = s.start[base + cylo], hi = s.start[base + cyhi + 1];
            for (int j = lo + lane; j < hi; j += kDensLanes) {
                const double2 pj = s.pos[j];
                const double dx = min_image(g, pi.x - pj.x), dy = pi.y - pj.y;
                const double r2 = dx * dx + dy * dy;
                if (j != i && r2 > kR2Min && r2 < ph.kc.rcut2) s_in += spline_W_sel(ph.kc, r2 * rsqrt_nr(r2));
            }
        }
        if (w.n > 0) {
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                int col;
                if (!neighbour_column(g, cx, u - 1, col)) continue;
                const int base = col * g.ncy;
                const int lo = w.start[base + cylo], hi = w.start[base + cyhi + 1];
                for (int j = lo + lane; j < hi; j += kDensLanes) {
                    const double2 pj = w.pos[j];
                    const double dx = min_image(g, pi.x - pj.x), dy = pi.y - pj.y;
                    const double r2 = dx * dx + dy * dy;
                    if (r2 > kR2Min && r2 < ph.kc.rcut2) s_ct += spline_W_sel(ph.kc, r2 * rsqrt_nr(r2)) * w.a[j].x;
                }
            }
        }
        // the lanes of the particle took the same path to here: the totals over them, in every lane; then lane 0 for the particle
#pragma unroll
        for (int off = kDensLanes / 2; off > 0; off >>= 1) {
            s_in += __shfl_xor(s_in, off, kDensLanes);
            s_ct += __shfl_xor(s_ct, off, kDensLanes);
        }
        if (lane != 0) continue;
        const double mass_i = s.mass[i];
        const double rho = density_from_sigma(ph.w0 + s_in, s_ct, mass_i, ph.rho0, ph.inv_sigma0);
        const double d = rho / ph.rho0 - 1.0;
        const bool ok = fabs(d) <= a.delta_bound;  // (a NaN or an infinity fails the comparison)
        const int k = stats_bin(pi.y, a.bin_w, a.n_bins);
        long long v[4];
        int hb = 0;
        unsigned long long kmax = 0ull, kmin = 0ull;
        if (ok) {
            const double dvol = ph.rho0 / rho - 1.0;
            const double wall = s_ct * ph.rho0 * ph.inv_sigma0 / mass_i;
            v[0] = __double2ll_rn(ldexp(d, sc.s_d));
            v[1] = __double2ll_rn(ldexp(d * d, sc.s_d2));
            v[2] = __double2ll_rn(ldexp(dvol, sc.s_dvol));
            v[3] = __double2ll_rn(ldexp(wall, sc.s_wall));
            kmax = dens_key(d);
            kmin = dens_key(-d);
            // the histogram's word: bins 0 .. n_hist - 1, then below, then above
            if (d < -a.hist_range) hb = a.n_hist;
            else if (d >= a.hist_range) hb = a.n_hist + 1;
            else hb = min(max((int)floor((d + a.hist_range) * a.hist_scale), 0), a.n_hist - 1);
        }
        for (int b = 0; b < a.n_bands; ++b) {
            if (b > 0 && !stats_in_band(pi.x, a.DL, a.band_x[b - 1], a.band_hw[b - 1])) continue;
            unsigned long long *c = s_cnt + ((size_t)b * a.n_bins + k) * kDensFields;
            if (!ok) { atomicAdd(c + kDensFields - 1, 1ull); continue; }
            atomicAdd(c, 1ull);
#pragma unroll
            for (int f = 0; f < 4; ++f)
                if (v[f]) atomicAdd(c + 1 + f, (unsigned long long)v[f]);  // (two's complement: signed sums wrap back to the right value)
            atomicAdd(s_hist + (size_t)b * (a.n_hist + 2) + hb, 1ull);
            unsigned long long *km = s_key + ((size_t)b * a.n_bins + k) * kDensKeys;
            atomicMax(km, kmax);
            atomicMax(km + 1, kmin);
        }
    }
    __syncthreads();
    // the extremes the workgroup met go straight into the running keys; then the sums, one thread per counter: the running
    // sums grow in sample order, each by its own bin -- no summation tree
    for (int k = threadIdx.x; k < nk; k += kDensBlock) {
        const unsigned long long v = s_key[k];
        if (v) atomicMax(keys + k, v);
    }
    stats_finish_sample<kDensBlock>(s_cnt, nc, isum, h, t_now, [&](int k, unsigned long long v) { dsum[k] += dens_value(k, n_binned, v, sc); });
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kDensBlock) void k_dens_stats(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w, DensStatsArgs a)
{
    dens_stats_body(clk, q, g, ph, s, w, a, a.isum, a.dsum, a.keys, a.head);
}

// batch (sphx_batch_dens_stats_*): member m = blockIdx.y samples its own state (member_set of the view, which is member 0's) on
// its own clock, with its own Phys, into its own blocks of sums and keys and its own head; Grid, Walls, the bins and the
// histogram are shared.  The sums are exact and the per-particle arithmetic is the single form's, so a member's are a
// standalone context's, bit for bit.  A member whose gate is closed returns before it touches anything.
__global__ __launch_bounds__(kDensBlock) void k_dens_stats_b(Members mb, int q, Grid g, FluidSet s, Walls w, DensStatsArgs a)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    const size_t off = (size_t)m * (size_t)a.block, koff = (size_t)m * (size_t)a.kblock;
    dens_stats_body(mb.clk + m, q, g, ph, member_set(mb, m, s), w, a, a.isum + off, a.dsum + off, a.keys + koff, a.head + m);
}

// Slab of a ring (sphx_slab_dstats_*): the sample is a sum over PARTICLES, so it is divided like the flow statistics' -- a slab
// bins the densities of the particles it OWNS (owns(): the column the slot was binned into, own_c0 <= cx < own_c1) and the
// ring's sums and histograms are the element-wise sums of the slabs', count and outliers included, its d_min / d_max their
// minimum / maximum.  Nothing about a particle's density changes: the two sums, density_from_sigma, the quantisation, the keys,
// the LDS counters and stats_finish_sample are the body's.  The loop runs over the clk->n slots held, owned and copies alike,
// with the workgroups of the slab's CAPACITY (a captured step graph outlives a re-binning); a copy is passed over as a particle
// of the sample and met as a partner: every held fluid slot j != i in the columns cx - 1 .. cx + 1 of the layout's cell ranges,
// and -- always, there is no with_walls here -- the slab's wall particles in the same columns (Walls::pos, Walls::a.x).
//
// Why the three-column sweep still suffices.  The argument of sphx_pair_dist.hpp is about the columns a particle and its
// partner were BINNED into, and a slab bins what it holds, copies included, into one grid of its window (Grid::periodic = 0:
// neighbour_column leaves out only columns beyond the window).  An owned particle has own_c0 <= cx < own_c1, so cx - 1 and
// cx + 1 lie in [own_c0 - 1, own_c1]: at most the FIRST halo column on either side, of the halo_cols >= 4 the window holds.
// The slab's wall particles are binned into the same grid and cover the whole window, halo columns included.
//
// Why the halo copies are usable.  Of a partner only the POSITION is read -- a fluid partner contributes W(r_ij), a wall
// partner W(r_ij) V_j with the wall's own volume -- and of the particle itself pos and mass_i, which is an owned slot's: the
// density is mass_i times a number density, so nothing is asked of a copy's mass or velocity.  The copies binned in own - 1 and
// own + 1 are complete and were stepped like everything held: in front of phase 3 -- where launch_slab_samplers sits, behind
// k_slab_pack3 -- they carry the finished step's position up to the summation order of their own neighbour lists, the premise
// k_pair_dist_s counts pairs on.  Unlike a count, W(r) is continuous in the copy's position: a copy that is a few ulps off
// moves its partners' densities by as little, amplified by the slope of W (tests/slab_dens_stats_cases.py: SENSITIVITY); a
// MISSING copy, or one a period off, changes every partner's density by a whole W(r).
//
// The window is open (half_DL = +inf: min_image is a no-op).  The first slab holds the last slab's particles at x - DL and the
// last slab the first slab's at x + DL, in the slab's own frame, so a pair across the periodic seam has its plain dx: there
// is nothing to fold.  A copy is never the particle's own image within 2h: the image lies DL away, and a ring needs
// n_ranks >= 2 slabs of at least halo_cols + 1 >= 5 columns of >= 2h each (SPHX:Slab:width), so DL >= 20h; nor does one
// window hold a partner twice, because it covers less than one period (SPHX:Slab:width).  Band membership goes by
// stats_in_band on the slab-frame x, whose fmod brings x < 0 and x >= DL back into [0, DL), as k_flow_stats_s relies on.
//
// The scales.  e comes from the configuration's delta_bound and is every rank's: whether a particle is summed or an outlier
// is decided the same way on every rank.  L comes from the held count clk->n, which bounds the owned count, so no overflow; it
// differs between the slabs, and with it only the fixed-point quantum a slab rounds to.  The keys of d_min / d_max are exact.
//
// Every slab finishes the sample (stats_finish_sample: the last workgroup out, or the one workgroup of a small slab) and
// stamps its head, whether or not it owns a particle of any band: n_samples, t_first and t_last come from the clock and agree
// between the ranks.  The dynamic LDS is k_dens_stats's, up to kDensMaxShmem, which a launch is granted without an attribute
// of the kernel symbol (k_flow_stats_s asks for as much).
__global__ __launch_bounds__(kDensBlock) void k_dens_stats_s(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w, DensStatsArgs a)
{
    dens_stats_body<true>(clk, q, g, ph, s, w, a, a.isum, a.dsum, a.keys, a.head);
}

}  // namespace sphx
