// sphx_pair_dist.hpp -- pair-distance statistics of a resident context (include/sphx.h section 2l), of every member of a
// batch (section 2m, k_pair_dist_b) and of a slab of a ring (section 3a, k_pair_dist_s, at the end): a slot sampler (sphx_slot_sample.hpp) that counts, for the fluid particles of a band (the
// CENTRES), their partners within r_max by distance: the histogram behind g(r), the mean neighbour count, the width of the
// first shell and the smallest separation.  The one sampler that describes the particle ARRANGEMENT, not the velocity field,
// and the one whose result is exact: integer counts and a minimum, reproduced count for count by profile.pair_histogram.
//
// One sample.  A centre is a fluid slot i < clk->n with y_lo <= y_i <= y_hi (y_margin, DH - y_margin); it counts for band 0 and
// for every x-band it lies in (stats_in_band, the flow statistics' rule).  A partner is every other fluid slot j != i and, with
// walls, every wall particle, in a histogram of its own.  dx = min_image(x_i - x_j), dy = y_i - y_j, and
// r2 = dx * dx + dy * dy WITHOUT contraction (pair_r2: fp contract(off)): the very double numpy computes.  The bin is decided by
// comparisons against the squared edges e2[k] = (k * bin_w)^2 (k < n_bins), e2[n_bins] = r_max^2 -- pair_bin, the square root
// gives a first guess only, as stats_bin's quotient does; r2 >= e2[n_bins] is not counted, r2 = 0 counts in bin 0.  The smallest
// fluid-fluid r2 among the COUNTED pairs of a band is kept beside the counts.
//
// Why the 3 x 3 sweep suffices.  A centre sweeps the three cell columns around the cell it was BINNED into (binned_cell, as
// the step's passes do), rows cy - 1 .. cy + 1, through neighbour_column: a period of one or two columns is visited once per
// distinct column and the minimum-image fold picks the nearest image.  A cell is 2h + skin wide and the clock stops or re-bins
// before anybody has drifted skin / 2 from where it was binned, so two particles within r_max <= 2h of each other now were
// within 2h + skin when they were binned: in the same cell or in adjacent ones.  Walls do not move.  Beyond 2h the argument
// fails, which is why the host refuses r_max > 2h.  Only the nearest image counts: a channel shorter than 4h can hold a
// second image of a partner within 2h, which is missed (the step's passes and the reference miss it too).
//
// Mapping: kPairLanes = 8 LANES PER CENTRE, kPairBlock / kPairLanes = 32 centres per workgroup trip, grid-stride over the
// centres.  A centre has 3 column runs of ~3 cells, ~110-150 candidates at h = 1.3 dp, ~20 of them in range: lane l takes
// candidates lo + l, lo + l + 8, ... of each run, so a run is 5-6 trips whose loads do not depend on one another, and the
// eight lanes read consecutive slots (one 128-byte line).  A thread per centre (k_field_map's mapping) walks ~40 trips and
// leaves a 1 200-particle channel with 19 waves of one long chain each; a wave per centre (k_point_probes' mapping) leaves 16
// of 64 lanes idle on every run of 48 and needs 30 k waves at C2.  Eight lanes keep a run's trips short and a wave full.
// Measured per launch (profiles/r30_pair_dist.txt; re-binning every step / the context's own policy, lattice): four lanes
// 21.6 / 30.8 us at C2 and 88 / 118 us at 0.25 M particles, eight 16.0 / 18.4 and 95 / 123, sixteen 16.7 / 17.1 and 123 / 141:
// four lose a third at C2 to win 4-7 % on the large channel, sixteen lose 15-30 % there for 7 % at C2.  Eight it is.
//
// The counters.  Everything summed is an INTEGER: no fixed-point staging, no conversion pass, no last workgroup out; arrival
// order cannot change a bit.  A workgroup bins into 64-bit LDS counters [band][ff | fw][bin] followed by [band] centres and
// [band] r2_min bit patterns (non-negative doubles order as unsigned integers: atomicMin).  The known trap (kStatsPerThread):
// the LDS adds of a workgroup serialise on the few bins a lattice has -- every pair falls into four.  It does not bite here,
// and nothing is done against it: about one candidate in six is within range, so a centre's ~20 adds are spread over eight
// lanes and ~17 trips of loads and arithmetic.  Measured (profiles/r30_pair_dist.txt): the lattice costs no more than a
// developed state (C2 16.0 / 16.9 us, 0.25 M particles 95 / 97 us), and a build in which a lane kept a pending (bin, count)
// and touched LDS only when the bin changed was 2-4 % SLOWER on both.  At the end a workgroup adds its non-zero counters to
// the global uint64 sums with one atomic each; r2_min goes by one atomicMin per band.  Thread 0 of workgroup 0 notes the
// sample (note_sample): the head depends on nobody else's work.  Plain vector stores and global atomics only.
//
// Determinism: integer adds and a minimum, in any order, give the same integers: the sums cannot depend on particle order,
// layout, re-binning phase, workgroup count or batch membership.  A member of a batch runs the same body.
#pragma once
#include "sphx_flow_stats.hpp"

namespace sphx {

constexpr int kPairBlock = 256;
#ifndef SPHX_EXP_PAIR_LANES  // (measurement builds: tools/probes/build_variant_lib.sh lanes4 -DSPHX_EXP_PAIR_LANES=4)
#define SPHX_EXP_PAIR_LANES 8
#endif
constexpr int kPairLanes = SPHX_EXP_PAIR_LANES;            // lanes per centre (a power of two up to 64)
constexpr int kPairCentres = kPairBlock / kPairLanes;      // centres per workgroup trip
constexpr int kPairMaxBlocks = 2048;                       // every workgroup flushes its counters: no more than 8 per CU
constexpr int kPairMaxBins = 1024;
constexpr int kPairMaxBands = 3;                           // band 0 and two x-bands
constexpr int kPairMaxCounters = kPairMaxBands * 2 * kPairMaxBins;  // the LDS budget: (n_bands + 1) * n_bins * (1 + with_walls)
                                                                    // <= 6 144 counters of 8 bytes, and with the centres and
                                                                    // r2_min words of three bands 49 200 B a workgroup.  The
                                                                    // limits on bins and bands keep every configuration within
                                                                    // it: there is nothing left to refuse.
static_assert((kPairMaxCounters + 2 * kPairMaxBands) * sizeof(unsigned long long) <= 64 * 1024, "the LDS a workgroup may ask for");
constexpr unsigned long long kPairInfBits = 0x7ff0000000000000ull;  // +inf: "no pair yet"

struct PairDistHead {
    long long n_samples;
    double t_first, t_last;
};

// the sums of one channel: [n_bands][kinds][n_bins] counts, [n_bands] centres, [n_bands] r2_min bit patterns
struct PairDistArgs {
    unsigned long long *sums;  // (of a batch: member 0's, member m's block of `block` words behind)
    PairDistHead *head;        // (of a batch: [M])
    double bin_w;              // r_max / n_bins
    double rmax2;              // e2[n_bins] = r_max * r_max
    double y_lo, y_hi;         // y_margin, DH - y_margin
    double DL, t_from;
    double band_x[2], band_hw[2];
    int n_bins, n_bands;       // n_bands counts band 0
    int kinds;                 // 1: fluid-fluid; 2: and fluid-wall
    int block;                 // words of one channel's sums: n_bands * (kinds * n_bins + 2)
    int every;                 // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
};

// dx * dx + dy * dy with every operation rounded: hipcc contracts a * b + c into a fused multiply-add by default, which rounds
// once where numpy rounds twice, and HIP's __dmul_rn / __dadd_rn are plain operators that do not stop it.  The pragma does.
__device__ __forceinline__ double pair_r2(double dx, double dy)
{
#pragma clang fp contract(off)
    const double xx = dx * dx, yy = dy * dy;
    return xx + yy;
}

// squared lower edge of bin k (k < n_bins): numpy's (k * bin_w) ** 2
__device__ __forceinline__ double pair_edge2(int k, double bin_w)
{
#pragma clang fp contract(off)
    const double e = (double)k * bin_w;
    return e * e;
}

// bin of r2 < rmax2: e2[k] <= r2 < e2[k+1] with e2[n_bins] = rmax2 -- numpy's searchsorted(e2, r2, side="right") - 1.  The
// square root is a first guess only: the comparisons against the edges decide.
__device__ __forceinline__ int pair_bin(double r2, double bin_w, int n_bins)
{
    int k = (int)(sqrt(r2) / bin_w);
    k = k < 0 ? 0 : (k > n_bins - 1 ? n_bins - 1 : k);
    while (k > 0 && r2 < pair_edge2(k, bin_w)) --k;
    while (k < n_bins - 1 && r2 >= pair_edge2(k + 1, bin_w)) ++k;
    return k;
}

// one candidate at pj of centre pi: where it counts, one more pair of kind `kind` in its bin for every band of `bands` (bit b:
// band b); r2m: the lane's smallest counted r2 of this kind
__device__ __forceinline__ void pair_add(const Grid &g, const PairDistArgs &a, unsigned long long *s_cnt, unsigned bands, int kind, double2 pi,
                                         double2 pj, double &r2m)
{
    const double dx = min_image(g, pi.x - pj.x), dy = pi.y - pj.y;
    const double r2 = pair_r2(dx, dy);
    if (!(r2 < a.rmax2)) return;
    r2m = fmin(r2m, r2);
    const int k = pair_bin(r2, a.bin_w, a.n_bins);
#pragma unroll
    for (int b = 0; b < kPairMaxBands; ++b)
        if (bands >> b & 1u) atomicAdd(s_cnt + ((size_t)b * a.kinds + kind) * a.n_bins + k, 1ull);
}

// The sample of one channel closing the step slot of parity q, on clock clk, by the gridDim.x workgroups of a grid row; s is the
// state the step left (pos and the cell ranges and binned cells of the layout it is stored in); sums / h are that channel's own.
// kSlab: the channel is a slab of a ring -- of the clk->n slots it holds only those it owns (owns()) are centres, every held
// slot is a partner (k_pair_dist_s).
template <bool kSlab = false>
__device__ __forceinline__ void pair_dist_body(const Clock *clk, int q, const Grid &g, const FluidSet &s, const Walls &w, const PairDistArgs &a,
                                               unsigned long long *sums, PairDistHead *h)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    const int n = clk->n;
    extern __shared__ unsigned long long s_cnt[];  // [n_bands][kinds][n_bins], [n_bands] centres, [n_bands] r2_min
    const int nc = a.n_bands * a.kinds * a.n_bins;
    unsigned long long *s_ctr = s_cnt + nc, *s_min = s_ctr + a.n_bands;
    for (int k = threadIdx.x; k < nc + a.n_bands; k += kPairBlock) s_cnt[k] = 0ull;
    if ((int)threadIdx.x < a.n_bands) s_min[threadIdx.x] = kPairInfBits;
    __syncthreads();

    const int lane = (int)threadIdx.x & (kPairLanes - 1), grp = (int)threadIdx.x / kPairLanes;
    const bool walls = a.kinds > 1;
    const double inf = __builtin_inf();
    // (no barrier inside the loop: a group that has no centre, or whose centre is outside the margins, goes on to its next)
    for (long long i0 = (long long)blockIdx.x * kPairCentres + grp; i0 < (long long)n; i0 += (long long)gridDim.x * kPairCentres) {
        const int i = (int)i0;
        const double2 pi = s.pos[i];
        if constexpr (kSlab) {
            if (!owns(g, pi.x, s.cell[i])) continue;  // (a halo copy: its owner counts it as a centre)
        }
        if (!(pi.y >= a.y_lo && pi.y <= a.y_hi)) continue;
        unsigned bands = 1u;
        for (int b = 1; b < a.n_bands; ++b)
            if (stats_in_band(pi.x, a.DL, a.band_x[b - 1], a.band_hw[b - 1])) bands |= 1u << b;
        int cx, cy;
        binned_cell(g, s, i, cx, cy);
        const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
        double r2m = inf, r2w = inf;  // (the walls' minimum is not kept)
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            int col;
            if (!neighbour_column(g, cx, u - 1, col)) continue;
            const int base = col * g.ncy;
            const int lo = s.start[base + cylo], hi = s.start[base + cyhi + 1];
            for (int j = lo + lane; j < hi; j += kPairLanes)
                if (j != i) pair_add(g, a, s_cnt, bands, 0, pi, s.pos[j], r2m);
        }
        if (walls) {
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                int col;
                if (!neighbour_column(g, cx, u - 1, col)) continue;
                const int base = col * g.ncy;
                const int lo = w.start[base + cylo], hi = w.start[base + cyhi + 1];
                for (int j = lo + lane; j < hi; j += kPairLanes) pair_add(g, a, s_cnt, bands, 1, pi, w.pos[j], r2w);
            }
        }
        // the eight lanes of the centre took the same path to here: the minimum over them, then lane 0 for the centre
#pragma unroll
        for (int off = kPairLanes / 2; off > 0; off >>= 1) r2m = fmin(r2m, __shfl_xor(r2m, off, kPairLanes));
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < kPairMaxBands; ++b)
                if (bands >> b & 1u) {
                    atomicAdd(s_ctr + b, 1ull);
                    if (r2m < inf) atomicMin(s_min + b, (unsigned long long)__double_as_longlong(r2m));
                }
        }
    }
    __syncthreads();
    // the workgroup's non-zero counters and centres, one atomic each; the minima, where it met a pair
    for (int k = threadIdx.x; k < nc + a.n_bands; k += kPairBlock) {
        const unsigned long long v = s_cnt[k];
        if (v) atomicAdd(sums + k, v);
    }
    if ((int)threadIdx.x < a.n_bands) {
        const unsigned long long v = s_min[threadIdx.x];
        if (v != kPairInfBits) atomicMin(sums + nc + a.n_bands + threadIdx.x, v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) note_sample(h, clk->t);
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kPairBlock) void k_pair_dist(const Clock *clk, int q, Grid g, FluidSet s, Walls w, PairDistArgs a)
{
    pair_dist_body(clk, q, g, s, w, a, a.sums, a.head);
}

// batch (sphx_batch_pair_dist_*): member m = blockIdx.y samples its own state (member_set of the view, which is member 0's) on
// its own clock into its own block of sums (m * a.block words) and its own head; Grid, Walls and the bins are shared.  The sums
// are exact, so a member's are a standalone context's.  A member whose gate is closed returns before it touches anything.
__global__ __launch_bounds__(kPairBlock) void k_pair_dist_b(Members mb, int q, Grid g, FluidSet s, Walls w, PairDistArgs a)
{
    const int m = (int)blockIdx.y;
    pair_dist_body(mb.clk + m, q, g, member_set(mb, m, s), w, a, a.sums + (size_t)m * (size_t)a.block, a.head + m);
}

// Slab of a ring (sphx_slab_pairs_*): the sample is a sum over CENTRES, so it is divided like the flow statistics' -- a slab
// counts the pairs whose centre it OWNS (owns(): the column the slot was binned into, own_c0 <= cx < own_c1), the ring's
// histogram is the element-wise sum of the slabs' and its r2_min their minimum; integers and a minimum, so the ring's sums do
// not depend on how the channel is cut.  The loop runs over the clk->n slots held, owned and copies alike, with the
// workgroups of the slab's CAPACITY (a captured step graph outlives a re-binning); a copy is passed over as a centre and
// met as a partner: every held fluid slot j != i in the columns cx - 1 .. cx + 1 of the layout's cell ranges, and with walls
// the slab's wall particles in the same columns.
//
// Why the three-column sweep still suffices.  The argument above is about the columns a centre and its partner were BINNED
// into, and a slab bins what it holds, copies included, into one grid of its window (Grid::periodic = 0: neighbour_column
// leaves out only columns beyond the window).  An owned centre has own_c0 <= cx < own_c1, so cx - 1 and cx + 1 lie in
// [own_c0 - 1, own_c1]: at most the FIRST halo column on either side, and the window holds halo_cols >= 4 of them.  The halo
// premise is that the copies binned in own - 1 and own + 1 are complete and carry the finished step's
// position in front of phase 3, up to the summation order of their own neighbour lists: what the field map and the probes
// of a slab rely on.  Only pos, cell and start are read.
//
// The window is open (half_DL = +inf: min_image is a no-op).  The first slab holds the last slab's particles at x - DL and the
// last slab the first slab's at x + DL, in the slab's own frame, so a pair across the periodic seam has its plain dx: there
// is nothing to fold.  A copy can never be the centre's own image within r_max <= 2h: the image lies DL away, and a ring
// needs n_ranks >= 2 slabs of at least halo_cols + 1 >= 5 columns of >= 2h each (SPHX:Slab:width), so DL >= 20h; nor can one
// window hold a partner twice, because it covers less than one period (SPHX:Slab:width).  Band membership goes by
// stats_in_band on the slab-frame x, whose fmod brings x < 0 and x >= DL back into [0, DL), as k_flow_stats_s relies on.
//
// The head is noted by thread 0 of workgroup 0 of every slab, whether or not the slab owns a centre of any band: n_samples,
// t_first and t_last come from the clock and agree between the ranks.
__global__ __launch_bounds__(kPairBlock) void k_pair_dist_s(const Clock *clk, int q, Grid g, FluidSet s, Walls w, PairDistArgs a)
{
    pair_dist_body<true>(clk, q, g, s, w, a, a.sums, a.head);
}

}  // namespace sphx
