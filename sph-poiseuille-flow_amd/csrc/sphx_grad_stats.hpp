// sphx_grad_stats.hpp -- velocity-gradient statistics of a resident context (include/sphx.h section 2n), of every member of
// a batch (section 2o, k_grad_stats_b) and of a slab of a ring (section 3a, k_grad_stats_s, at the end): a slot sampler (sphx_slot_sample.hpp) that estimates the velocity gradient
// G_ab = d u_a / d x_b at every fluid particle and bins g_xx, g_xy, g_yx, g_yy, their squares, the squared divergence and the
// squared vorticity into the flow statistics' y-bins and x-bands.  The one sampler that describes the GRADIENT of the velocity:
// the shear-rate profile du_x/dy (hence tau(y) = mu du_x/dy), div v and the vorticity.  profile.velocity_gradients is the numpy
// definition, profile.grad_stats_sums the binned sample.
//
// One sample.  For every fluid slot i < clk->n the partners j are every other fluid slot within 2h (nearest image, min_image;
// kR2Min < r2 < (2h)^2) and, with walls, every wall particle within 2h:
//     d = r_i - r_j,   w_j = V_j W'(|d|) / |d|          V_j = mass_j / rho0 (fluid), Walls::a.x (wall; velocity Walls::a.y, .z)
//     M_i = - sum_j w_j d (x) d                          (symmetric; ~ I at full support)
//     A_i = sum_j w_j (v_j - v_i) (x) d
//     G_i = A_i M_i^-1
// A and M carry the same weights, so a linear field v = v_0 + L r gives A = L M exactly and G = L whatever the arrangement: no
// summation density, no second pass, first order at a one-sided support.  A particle is SKIPPED -- counted in `skipped`,
// summed nowhere -- when det M_i <= det_min (no or collinear partners), when a component of G_i is not finite, or when one
// exceeds the sample's bound in magnitude.  y outside [0, DH] is dropped, as the flow statistics drop it: per bin and band
// count + skipped is the flow statistics' count.
//
// Why the 3 x 3 sweep suffices: the header of sphx_pair_dist.hpp -- partners within 2h now were binned in the same cell or an
// adjacent one.  Only the nearest image counts.
//
// Mapping: pair_dist_body's.  kGradLanes LANES PER PARTICLE sweep the three cell columns around the cell it was binned into,
// rows cy - 1 .. cy + 1; lane l takes candidates lo + l, lo + l + kGradLanes, ... of each run and keeps seven partial sums
// (m11, m12, m22, a11, a12, a21, a22); velocity and mass of a candidate are loaded only where it is in range (about one in
// six).  The partial sums are reduced over the group by __shfl_xor, after which every lane of the group holds the same totals;
// lane 0 solves the 2 x 2 system, quantises and does the LDS adds.  A particle's partners are added in SLOT order (lane-strided,
// then the shuffle tree): the sums depend on the layout within floating-point rounding, not beyond.
// Measured per launch (profiles/r32_grad_stats.txt; re-binning every step / the context's own policy, lattice): four lanes
// 32.0 / 40.4 us at C2 and 135 / 177 us at 0.25 M particles, eight 25.8 / 29.6 and 167 / 206, sixteen 23.3 / 24.9 and 247 / 269:
// four lose a quarter to a third at C2 to win 14-19 % on the large channel, sixteen lose 30-50 % there for 10-16 % at C2.  Eight
// it is, as for the pair statistics.  A build in which the lanes of a group shared the particle's LDS adds (field f by lane
// f % 8; 83 registers for 101, five waves per SIMD for four) cost the same within 1 % in all eight cases and was taken out:
// the time is in the sweep, not in lane 0's tail.
//
// Exact sums.  A sample is summed in int64 fixed point as sphx_flow_stats.hpp does.  With n <= 2^L particles and the bound
// 2^e > 16 Clock::vmax / h (over the 2h of a support the velocity cannot change by more than 2 vmax, so a well-conditioned
// estimate stays below vmax / h times a small factor; a larger component can only come from an ill-conditioned M and is
// skipped), a component |g| <= 2^e times 2^(62-L-e) is at most 2^(62-L), a square g^2 <= 2^(2e) times 2^(62-L-2e) likewise, and
// |div| = |g_xx + g_yy| and |omega| = |g_yx - g_xy| reach 2^(e+1), their squares 2^(2e+2): they take the scale 2^(60-L-2e).  No
// sum of n <= 2^L such terms exceeds 2^62 in magnitude: no overflow.  vmax = 0 leaves the floor bound 2^-59, at which a fluid
// at rest (A = 0 exactly) sums to exact zeros.  count and skipped are plain integers.  A workgroup keeps its counters in LDS,
// adds the non-zero ones to the global integer sums with one atomic each, and the last workgroup out converts them, adds them
// to the running double sums and clears them; one workgroup finishes a small sample by itself (stats_finish_sample, shared
// with the flow statistics).  Integer adds commute: the sums do not depend on the dispatch order of the workgroups, are
// bit-identical between runs, and a batch member's are a standalone context's.
#pragma once
#include "sphx_flow_stats.hpp"

namespace sphx {

constexpr int kGradFields = 12;   // per bin and band: count, sum g_xx, g_xy, g_yx, g_yy, their four squares, sum div^2, sum omega^2, skipped
constexpr int kGradMaxBins = 640; // n_bands * n_bins (incl. band 0): 61 440 B of LDS counters per workgroup
constexpr int kGradBlock = 256;
#ifndef SPHX_EXP_GRAD_LANES  // (measurement builds: tools/probes/build_variant_lib.sh glanes4 -DSPHX_EXP_GRAD_LANES=4)
#define SPHX_EXP_GRAD_LANES 8
#endif
constexpr int kGradLanes = SPHX_EXP_GRAD_LANES;        // lanes per particle (a power of two up to 64)
constexpr int kGradCentres = kGradBlock / kGradLanes;  // particles per workgroup trip
constexpr int kGradTrips = 2;                          // trips a workgroup takes before another is added: up to 64 particles ONE
                                                       // workgroup finishes the sample by itself (no flush, no ticket)
constexpr int kGradMaxBlocks = 2048;                   // every workgroup flushes its counters: no more than 8 per CU
static_assert(kGradMaxBins * kGradFields * sizeof(unsigned long long) <= 60 * 1024, "the LDS a workgroup may ask for");

struct GradStatsHead {
    long long n_samples;
    double t_first, t_last;
    int ticket;  // last workgroup out (zero between launches)
};

struct GradStatsArgs {
    unsigned long long *isum;  // [n_bands][n_bins][kGradFields] integer sums of the sample in flight (zero in between)
    double *dsum;              // same layout: running sums over all samples
    GradStatsHead *head;       // (of a batch: [M]; isum / dsum: member m's block of `block` words behind member 0's)
    double DH, bin_w, DL;      // bin_w = DH / n_bins, the step of numpy's linspace
    double t_from, det_min;
    double band_x[2], band_hw[2];
    int n_bins, n_bands;       // n_bands counts band 0 (the whole channel)
    int block;                 // words of one channel's sums: n_bands * n_bins * kGradFields
    int with_walls;
    int every;                 // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
};

// the fixed-point scales of one sample: s1 for a component, s2 for its square, s3 for div^2 and omega^2; |g| <= bound
struct GradScales {
    int s1, s2, s3;
    double bound;
};

__device__ __forceinline__ GradScales grad_scales(double vmax, double h, int n)
{
    int L = 0;
    while (L < 31 && (1 << L) < n) ++L;
    int e = 0;
    (void)frexp(fmax(16.0 * vmax / h, 0x1p-60), &e);  // 16 vmax / h < 2^e  (a NaN vmax leaves the floor: every |g| is then out of range)
    return GradScales{62 - L - e, 62 - L - 2 * e, 60 - L - 2 * e, ldexp(1.0, e)};
}

// the seven partial sums of a particle's estimate
struct GradSums {
    double m11, m12, m22, a11, a12, a21, a22;
};

// one candidate at separation (dx, dy) = r_i - r_j with volume vol and velocity jump (dvx, dvy) = v_j - v_i, already in range
__device__ __forceinline__ void grad_add(const KernelConst &kc, double dx, double dy, double r2, double vol, double dvx, double dvy, GradSums &t)
{
    const double inv_r = rsqrt_nr(r2), r = r2 * inv_r;
    const double wj = vol * spline_dW(kc, r) * inv_r;
    const double wx = wj * dx, wy = wj * dy;
    t.m11 -= wx * dx; t.m12 -= wx * dy; t.m22 -= wy * dy;
    t.a11 += dvx * wx; t.a12 += dvx * wy; t.a21 += dvy * wx; t.a22 += dvy * wy;
}

// counter k of a sample as the double it stands for: field k % kGradFields, its scale taken back out
__device__ __forceinline__ double grad_value(int k, unsigned long long v, const GradScales &sc)
{
    const int f = k % kGradFields;
    const int s = (f == 0 || f == kGradFields - 1) ? 0 : (f <= 4 ? sc.s1 : (f <= 8 ? sc.s2 : sc.s3));
    return ldexp((double)(long long)v, -s);
}

// The sample of one channel closing the step slot of parity q, on clock clk, by the gridDim.x workgroups of a grid row; s is the
// state the step left (pos, vel, mass and the cell ranges and binned cells of the layout it is stored in); isum / dsum / h are
// that channel's own.
// kSlab: the channel is a slab of a ring -- of the clk->n slots it holds only those it owns (owns()) are particles of the
// sample, every held slot is a partner (k_grad_stats_s).
template <bool kSlab = false>
__device__ __forceinline__ void grad_stats_body(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s, const Walls &w,
                                                const GradStatsArgs &a, unsigned long long *isum, double *dsum, GradStatsHead *h)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    const int n = clk->n;
    const double t_now = clk->t;
    const GradScales sc = grad_scales(clk->vmax, ph.kc.h, n);
    extern __shared__ unsigned long long s_cnt[];  // [n_bands][n_bins][kGradFields]
    const int nc = a.n_bands * a.n_bins * kGradFields;
    for (int k = threadIdx.x; k < nc; k += kGradBlock) s_cnt[k] = 0ull;
    __syncthreads();

    const int lane = (int)threadIdx.x & (kGradLanes - 1), grp = (int)threadIdx.x / kGradLanes;
    const double inv_rho0 = 1.0 / ph.rho0;
    // (no barrier inside the loop: a group that has no particle, or whose particle is outside [0, DH], goes on to its next)
    for (long long i0 = (long long)blockIdx.x * kGradCentres + grp; i0 < (long long)n; i0 += (long long)gridDim.x * kGradCentres) {
        const int i = (int)i0;
        const double2 pi = s.pos[i];
        if constexpr (kSlab) {
            if (!owns(g, pi.x, s.cell[i])) continue;  // (a halo copy: its owner bins it)
        }
        if (!(pi.y >= 0.0 && pi.y <= a.DH)) continue;  // outside [0, DH]: dropped, as discretize does
        const double2 vi = s.vel[i];
        int cx, cy;
        binned_cell(g, s, i, cx, cy);
        const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
        GradSums t{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            int col;
            if (!neighbour_column(g, cx, u - 1, col)) continue;
            const int base = col * g.ncy;
            const int lo = s.start[base + cylo], hi = s.start[base + cyhi + 1];
            for (int j = lo + lane; j < hi; j += kGradLanes) {
                const double2 pj = s.pos[j];
                const double dx = min_image(g, pi.x - pj.x), dy = pi.y - pj.y;
                const double r2 = dx * dx + dy * dy;
                if (j != i && r2 > kR2Min && r2 < ph.kc.rcut2) {
                    const double2 vj = s.vel[j];
                    grad_add(ph.kc, dx, dy, r2, s.mass[j] * inv_rho0, vj.x - vi.x, vj.y - vi.y, t);
                }
            }
        }
        if (a.with_walls) {
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                int col;
                if (!neighbour_column(g, cx, u - 1, col)) continue;
                const int base = col * g.ncy;
                const int lo = w.start[base + cylo], hi = w.start[base + cyhi + 1];
                for (int j = lo + lane; j < hi; j += kGradLanes) {
                    const double2 pj = w.pos[j];
                    const double dx = min_image(g, pi.x - pj.x), dy = pi.y - pj.y;
                    const double r2 = dx * dx + dy * dy;
                    if (r2 > kR2Min && r2 < ph.kc.rcut2) {
                        const double4 wj = w.a[j];
                        grad_add(ph.kc, dx, dy, r2, wj.x, wj.y - vi.x, wj.z - vi.y, t);
                    }
                }
            }
        }
        // the lanes of the particle took the same path to here: the totals over them, in every lane; then lane 0 for the particle
#pragma unroll
        for (int off = kGradLanes / 2; off > 0; off >>= 1) {
            t.m11 += __shfl_xor(t.m11, off, kGradLanes); t.m12 += __shfl_xor(t.m12, off, kGradLanes); t.m22 += __shfl_xor(t.m22, off, kGradLanes);
            t.a11 += __shfl_xor(t.a11, off, kGradLanes); t.a12 += __shfl_xor(t.a12, off, kGradLanes);
            t.a21 += __shfl_xor(t.a21, off, kGradLanes); t.a22 += __shfl_xor(t.a22, off, kGradLanes);
        }
        if (lane != 0) continue;
        const double det = t.m11 * t.m22 - t.m12 * t.m12;
        bool ok = det > a.det_min;
        double gxx = 0.0, gxy = 0.0, gyx = 0.0, gyy = 0.0;
        if (ok) {
            const double inv = 1.0 / det;
            gxx = (t.a11 * t.m22 - t.a12 * t.m12) * inv; gxy = (t.a12 * t.m11 - t.a11 * t.m12) * inv;
            gyx = (t.a21 * t.m22 - t.a22 * t.m12) * inv; gyy = (t.a22 * t.m11 - t.a21 * t.m12) * inv;
            // (a NaN or an infinity fails the comparison)
            ok = fabs(gxx) <= sc.bound && fabs(gxy) <= sc.bound && fabs(gyx) <= sc.bound && fabs(gyy) <= sc.bound;
        }
        const int k = stats_bin(pi.y, a.bin_w, a.n_bins);
        long long v[kGradFields - 2];
        if (ok) {
            const double dv = gxx + gyy, om = gyx - gxy;
            v[0] = __double2ll_rn(ldexp(gxx, sc.s1)); v[1] = __double2ll_rn(ldexp(gxy, sc.s1));
            v[2] = __double2ll_rn(ldexp(gyx, sc.s1)); v[3] = __double2ll_rn(ldexp(gyy, sc.s1));
            v[4] = __double2ll_rn(ldexp(gxx * gxx, sc.s2)); v[5] = __double2ll_rn(ldexp(gxy * gxy, sc.s2));
            v[6] = __double2ll_rn(ldexp(gyx * gyx, sc.s2)); v[7] = __double2ll_rn(ldexp(gyy * gyy, sc.s2));
            v[8] = __double2ll_rn(ldexp(dv * dv, sc.s3)); v[9] = __double2ll_rn(ldexp(om * om, sc.s3));
        }
        for (int b = 0; b < a.n_bands; ++b) {
            if (b > 0 && !stats_in_band(pi.x, a.DL, a.band_x[b - 1], a.band_hw[b - 1])) continue;
            unsigned long long *c = s_cnt + ((size_t)b * a.n_bins + k) * kGradFields;
            if (!ok) { atomicAdd(c + kGradFields - 1, 1ull); continue; }
            atomicAdd(c, 1ull);
#pragma unroll
            for (int f = 0; f < kGradFields - 2; ++f)
                if (v[f]) atomicAdd(c + 1 + f, (unsigned long long)v[f]);  // (two's complement: signed sums wrap back to the right value)
        }
    }
    __syncthreads();
    // one thread per counter: the running sums grow in sample order, each by its own bin -- no summation tree
    stats_finish_sample<kGradBlock>(s_cnt, nc, isum, h, t_now, [&](int k, unsigned long long v) { dsum[k] += grad_value(k, v, sc); });
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kGradBlock) void k_grad_stats(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w, GradStatsArgs a)
{
    grad_stats_body(clk, q, g, ph, s, w, a, a.isum, a.dsum, a.head);
}

// batch (sphx_batch_grad_stats_*): member m = blockIdx.y samples its own state (member_set of the view, which is member 0's) on
// its own clock, with its own Phys, into its own block of sums (m * a.block words) and its own head; Grid, Walls and the bins
// are shared.  The sums are exact and the per-particle arithmetic is the single form's, so a member's are a standalone
// context's, bit for bit.  A member whose gate is closed returns before it touches anything.
__global__ __launch_bounds__(kGradBlock) void k_grad_stats_b(Members mb, int q, Grid g, FluidSet s, Walls w, GradStatsArgs a)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    const size_t off = (size_t)m * (size_t)a.block;
    grad_stats_body(mb.clk + m, q, g, ph, member_set(mb, m, s), w, a, a.isum + off, a.dsum + off, a.head + m);
}

// Slab of a ring (sphx_slab_gstats_*): the sample is a sum over PARTICLES, so it is divided like the flow statistics' -- a slab
// bins the estimates of the particles it OWNS (owns(): the column the slot was binned into, own_c0 <= cx < own_c1) and the
// ring's sums are the element-wise sums of the slabs', count and skipped included.  Nothing about the estimate changes:
// grad_add, the 2 x 2 solve, the quantisation, the LDS counters and stats_finish_sample are the body's.  The loop runs over the
// clk->n slots held, owned and copies alike, with the workgroups of the slab's CAPACITY (a captured step graph outlives a
// re-binning); a copy is passed over as a particle of the sample and met as a partner: every held fluid slot j != i in the
// columns cx - 1 .. cx + 1 of the layout's cell ranges, and with walls the slab's wall particles in the same columns
// (Walls::a: volume and velocity).
//
// Why the three-column sweep still suffices.  The argument of sphx_pair_dist.hpp is about the columns a particle and its
// partner were BINNED into, and a slab bins what it holds, copies included, into one grid of its window (Grid::periodic = 0:
// neighbour_column leaves out only columns beyond the window).  An owned particle has own_c0 <= cx < own_c1, so cx - 1 and
// cx + 1 lie in [own_c0 - 1, own_c1]: at most the FIRST halo column on either side, of the halo_cols >= 4 the window holds.
//
// Why the halo copies are usable.  Unlike the pair statistics this sampler reads pos, VEL and MASS of a partner, and it
// differentiates them.  The copies binned in own - 1 and own + 1 are complete and were stepped like everything held: in front
// of phase 3 -- where launch_slab_samplers sits, behind k_slab_pack3 -- they carry the finished step's position and velocity
// up to the summation order of their own neighbour lists, the premise k_field_map_s reads vel on.  The view's mass is the
// layout array of the layout the step ran in, which a copy entered with its particle's mass at the last re-binning: the
// premise of k_point_probes_s.  A copy's state is therefore its owner's only to a few ulps, and the estimate amplifies such a
// difference a few hundred times (tests/slab_grad_stats_cases.py: SENSITIVITY): a ring's sums are a single context's within
// that, not to the 1e-12 of two single contexts.
//
// The window is open (half_DL = +inf: min_image is a no-op).  The first slab holds the last slab's particles at x - DL and the
// last slab the first slab's at x + DL, in the slab's own frame, so a pair across the periodic seam has its plain dx: there
// is nothing to fold.  A copy is never the particle's own image within 2h: the image lies DL away, and a ring needs
// n_ranks >= 2 slabs of at least halo_cols + 1 >= 5 columns of >= 2h each (SPHX:Slab:width), so DL >= 20h; nor does one
// window hold a partner twice, because it covers less than one period (SPHX:Slab:width).  Band membership goes by
// stats_in_band on the slab-frame x, whose fmod brings x < 0 and x >= DL back into [0, DL), as k_flow_stats_s relies on.
//
// The scales.  clk->vmax at the sampling point is the ring's all-reduced maximum, not the slab's own (k_flow_stats_s and
// k_profile_series_s quantise with it too), and h is every rank's: the bound 2^e, hence whether a particle is summed or
// skipped, is decided the same way on every rank.  L comes from the held count clk->n, which bounds the owned count, so no
// overflow; it differs between the slabs, and with it only the fixed-point quantum 2^-(62-L-e) a slab rounds to.
//
// Every slab finishes the sample (stats_finish_sample: the last workgroup out, or the one workgroup of a small slab) and
// stamps its head, whether or not it owns a particle of any band: n_samples, t_first and t_last come from the clock and agree
// between the ranks.  The dynamic LDS is k_grad_stats's, up to 61 440 B, which a launch is granted without an attribute of
// the kernel symbol (k_flow_stats_s asks for as much).
__global__ __launch_bounds__(kGradBlock) void k_grad_stats_s(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w, GradStatsArgs a)
{
    grad_stats_body<true>(clk, q, g, ph, s, w, a, a.isum, a.dsum, a.head);
}

}  // namespace sphx
