// sphx_flow_stats.hpp -- time-averaged velocity profiles of a resident context (include/sphx.h section 2a, "flow
// statistics"), of every member of a batch (section 2c, k_flow_stats_b) and of a slab of a ring (section 3a,
// k_flow_stats_s: the particles the slab owns): a slot sampler (sphx_slot_sample.hpp) that
// bins the state the step left into the reference's profile bins (SPH_Poiseuille.m:579-605) and adds it to running sums.
//
// Determinism: a sample is summed EXACTLY, in int64 fixed point -- integer adds do not depend on the order they arrive
// in, so neither the particle order (layouts, re-binnings) nor the dispatch order of the workgroups can change a bit.
// Per sample the scales are powers of two picked from the particle count and a bound of 2 max|v| (Clock::vmax): with
// n <= 2^L particles and |u| <= 2^e, u * 2^(62-L-e) and u^2 * 2^(62-L-2e) are below 2^(62-L), so no sum of n of them can
// overflow.  A |u| above the bound (only a non-finite state can have one) raises a sticky flag and the read fails.
// Each workgroup keeps the sample's counters in LDS, adds every non-zero one to the global integer sums with one
// atomic, and the last workgroup out (last_out_fenced) converts the integer sums to double, adds them to the running
// sums bin by bin and clears them for the next sample.  The binning itself (stats_bin_sample) is shared with the profile
// series (sphx_profile_series.hpp), which stores the sample as a record where this sampler adds it.
#pragma once
#include "sphx_slot_sample.hpp"

namespace sphx {

constexpr int kStatsFields = 5;            // per bin and band: count, sum u_x, sum u_x^2, sum u_y, sum u_y^2
constexpr int kStatsMaxBins = 1536;        // n_bands * n_bins (incl. band 0): 61 440 B of LDS counters per workgroup
constexpr int kStatsBlock = 512;
constexpr int kStatsMaxBlocks = 256;       // one workgroup per CU at most: every one of them flushes its counters
constexpr int kStatsPerThread = 8;         // particles a thread takes before another workgroup is added: up to 4 096
                                           // particles ONE workgroup finishes the sample by itself (no flush, no ticket).
                                           // (32, i.e. one workgroup up to 16 k particles: C2 29.3 -> 32.2 us/step -- the
                                           // LDS adds of one workgroup serialise on the few bins a wave's particles share)

struct FlowStatsHead {
    long long n_samples;
    double t_first, t_last;
    int range;   // sticky: some |u| of some sample exceeded the bound of that sample
    int ticket;  // last workgroup out (zero between launches)
};

struct FlowStatsArgs {
    const double2 *pos, *vel;   // the state to sample (fluid slots 0 .. clk->n-1, any order)
    unsigned long long *isum;   // [n_bands][n_bins][kStatsFields] integer sums of the sample in flight (zero in between)
    double *dsum;               // same layout: running sums over all samples
    FlowStatsHead *head;
    double DH, bin_w, DL;       // bin_w = DH / n_bins, the step of numpy's linspace
    double t_from;
    double band_x[2], band_hw[2];
    int n_bins, n_bands;        // n_bands counts band 0 (the whole channel)
    int every;                  // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
};

// y-bin of the reference's binning (numpy linspace edges, discretize semantics): edges[k] = k * bin_w for k < n_bins,
// edges[n_bins] = DH; bin k holds edges[k] <= y < edges[k+1], the last bin also y == DH.  The quotient is a first guess
// only: the comparisons against the edges decide, so a particle exactly on an edge lands where the host puts it.
__device__ __forceinline__ int stats_bin(double y, double bin_w, int n_bins)
{
    int k = (int)(y / bin_w);
    k = k < 0 ? 0 : (k > n_bins - 1 ? n_bins - 1 : k);
    while (k > 0 && y < (double)k * bin_w) --k;
    while (k < n_bins - 1 && y >= (double)(k + 1) * bin_w) ++k;
    return k;
}

// compute_mid_channel_profile's membership: xw = x mod DL (numpy's sign rule), d = min(|xw - xc|, DL - |xw - xc|) <= hw
__device__ __forceinline__ bool stats_in_band(double x, double DL, double xc, double hw)
{
    double m = fmod(x, DL);
    if (m != 0.0 && m < 0.0) m += DL;
    double d = fabs(m - xc);
    d = fmin(d, DL - d);
    return d <= hw;
}

__device__ __forceinline__ void stats_scales(double vmax, int n, int &s1, int &s2, double &bound)
{
    int L = 0;
    while (L < 31 && (1 << L) < n) ++L;
    int e = 0;
    (void)frexp(fmax(2.0 * vmax, 0x1p-60), &e);  // 2 vmax < 2^e  (a NaN vmax leaves the floor: every |u| is then out of range)
    bound = ldexp(1.0, e);
    s1 = 62 - L - e;
    s2 = 62 - L - 2 * e;
}

__device__ __forceinline__ void stats_add(unsigned long long *h, long long ux, long long ux2, long long uy, long long uy2)
{
    atomicAdd(h + 0, 1ull);
    atomicAdd(h + 1, (unsigned long long)ux);  // (two's complement: signed sums wrap back to the right value)
    atomicAdd(h + 2, (unsigned long long)ux2);
    atomicAdd(h + 3, (unsigned long long)uy);
    atomicAdd(h + 4, (unsigned long long)uy2);
}

// where the arrays of the sampled channel are, and which of its slots count (mine): the context's own, all of them ...
struct StatsOwn {
    __device__ bool mine(int, double) const { return true; }
    __device__ const double2 *pos(const FlowStatsArgs &a) const { return a.pos; }
    __device__ const double2 *vel(const FlowStatsArgs &a) const { return a.vel; }
    __device__ unsigned long long *isum(const FlowStatsArgs &a) const { return a.isum; }
    __device__ double *dsum(const FlowStatsArgs &a) const { return a.dsum; }
    __device__ FlowStatsHead *head(const FlowStatsArgs &a) const { return a.head; }
};

// ... or member m's blocks of a batch's: state at m * part, sums at m * n_bands * n_bins * kStatsFields, head m
struct StatsMember {
    long long part;
    int m;
    __device__ bool mine(int, double) const { return true; }
    __device__ long long sums(const FlowStatsArgs &a) const { return (long long)m * a.n_bands * a.n_bins * kStatsFields; }
    __device__ const double2 *pos(const FlowStatsArgs &a) const { return a.pos + part * m; }
    __device__ const double2 *vel(const FlowStatsArgs &a) const { return a.vel + part * m; }
    __device__ unsigned long long *isum(const FlowStatsArgs &a) const { return a.isum + sums(a); }
    __device__ double *dsum(const FlowStatsArgs &a) const { return a.dsum + sums(a); }
    __device__ FlowStatsHead *head(const FlowStatsArgs &a) const { return a.head + m; }
};

// ... or a slab's own, of which the particles it owns count (owns(): by position on a protocol grid, by the column slot i was
// binned into on a skinned slab): the halo copies are sampled by the slabs that own them, so the sums of the ring's slabs
// add up to the channel's.  cell: the layout the step ran in.
struct StatsSlab : StatsOwn {
    Grid g;
    const int *cell;
    __device__ bool mine(int i, double x) const { return owns(g, x, g.own_by_cell ? cell[i] : 0); }
};

// the fixed-point scales of one sample (stats_scales)
struct StatsScales {
    int s1, s2;
};

// The binning of one sample, stated once for its two finishers -- flow_stats_body adds the sample to running sums,
// profile_series_body (sphx_profile_series.hpp) stores it as a record: the workgroup's share of the n particles, binned into
// its LDS counters s_cnt [n_bands][n_bins][kStatsFields], from zeroing them to the barrier behind the particle loop.  range():
// the sticky flag of the head that owns the sample (looked up only by a thread that raises it).  By every thread of the workgroup.
template <typename At, typename Range>
__device__ __forceinline__ StatsScales stats_bin_sample(const FlowStatsArgs &a, const At &at, int n, double vmax, unsigned long long *s_cnt,
                                                        int nc, Range &&range)
{
    for (int k = threadIdx.x; k < nc; k += kStatsBlock) s_cnt[k] = 0ull;
    __syncthreads();

    int s1, s2;
    double bound;
    stats_scales(vmax, n, s1, s2, bound);
    const int chunk = (n + (int)gridDim.x - 1) / (int)gridDim.x;  // a contiguous run of slots per workgroup (cell order:
    const int i0 = (int)blockIdx.x * chunk;                        // only the workgroups over a band's columns touch it)
    const int i1 = min(n, i0 + chunk);
    bool out_of_range = false;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += kStatsBlock) {
        const double2 p = at.pos(a)[i], v = at.vel(a)[i];
        if (!at.mine(i, p.x)) continue;
        if (!(p.y >= 0.0 && p.y <= a.DH)) continue;  // outside [0, DH]: dropped, as discretize does
        if (!(fabs(v.x) <= bound && fabs(v.y) <= bound)) { out_of_range = true; continue; }
        const int k = stats_bin(p.y, a.bin_w, a.n_bins);
        const long long ux = __double2ll_rn(ldexp(v.x, s1)), uy = __double2ll_rn(ldexp(v.y, s1));
        const long long ux2 = __double2ll_rn(ldexp(v.x * v.x, s2)), uy2 = __double2ll_rn(ldexp(v.y * v.y, s2));
        stats_add(s_cnt + (size_t)k * kStatsFields, ux, ux2, uy, uy2);
        for (int b = 1; b < a.n_bands; ++b)
            if (stats_in_band(p.x, a.DL, a.band_x[b - 1], a.band_hw[b - 1]))
                stats_add(s_cnt + ((size_t)b * a.n_bins + k) * kStatsFields, ux, ux2, uy, uy2);
    }
    if (out_of_range) atomicOr(range(), 1);
    __syncthreads();
    return StatsScales{s1, s2};
}

// counter k of a sample as the double it stands for: field k % kStatsFields, its scale taken back out
__device__ __forceinline__ double stats_value(int k, unsigned long long v, const StatsScales &sc)
{
    const int f = k % kStatsFields;
    const int s = f == 0 ? 0 : ((f & 1) ? sc.s1 : sc.s2);
    return ldexp((double)(long long)v, -s);
}

// The end of a sample whose workgroups have binned their shares into integer LDS counters s_cnt[nc] (behind the barrier that
// closes the binning), stated once for the samplers that add a sample to running sums -- the flow statistics and the gradient
// statistics (sphx_grad_stats.hpp): finish(k, v) adds counter k's integer total v to its running sum.  One workgroup holds the
// whole sample of a small channel: no global sums, no ticket.  Otherwise every workgroup adds its non-zero counters to the
// global integer sums isum with one atomic each, and the last one out (last_out_fenced on head->ticket) finishes every counter
// and clears it for the next sample.  By every thread of a workgroup of kThreads.
template <int kThreads, typename Head, typename Finish>
__device__ __forceinline__ void stats_finish_sample(const unsigned long long *s_cnt, int nc, unsigned long long *isum, Head *head, double t_now,
                                                    Finish &&finish)
{
    __shared__ int s_last;
    if (gridDim.x == 1) {  // small channels: one workgroup holds the whole sample -- no global sums, no ticket
        for (int k = threadIdx.x; k < nc; k += kThreads)
            if (s_cnt[k]) finish(k, s_cnt[k]);
        if (threadIdx.x == 0) note_sample(head, t_now);
        return;
    }
    for (int k = threadIdx.x; k < nc; k += kThreads) {
        const unsigned long long v = s_cnt[k];
        if (v) atomicAdd(isum + k, v);
    }
    last_out_fenced(&head->ticket, s_last);
    if (!s_last) return;
    for (int k = threadIdx.x; k < nc; k += kThreads) {
        const unsigned long long v = atomicExch(isum + k, 0ull);
        if (v) finish(k, v);
    }
    if (threadIdx.x == 0) {
        note_sample(head, t_now);
        __hip_atomic_store(&head->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The sample of one channel closing the step slot of parity q, on clock clk, shared by the gridDim.x workgroups of a grid
// row; `at` says where the channel's arrays are: a's own pointers (StatsOwn) or a batch member's blocks (StatsMember).
template <typename At>
__device__ __forceinline__ void flow_stats_body(const Clock *clk, int q, const FlowStatsArgs &a, const At &at)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    const int n = clk->n;
    const double vmax = clk->vmax, t_now = clk->t;
    extern __shared__ unsigned long long s_cnt[];  // [n_bands][n_bins][kStatsFields]
    const int nc = a.n_bands * a.n_bins * kStatsFields;
    const StatsScales sc = stats_bin_sample(a, at, n, vmax, s_cnt, nc, [&] { return &at.head(a)->range; });
    // one thread per counter: the running sums grow in sample order, each by its own bin -- no summation tree
    stats_finish_sample<kStatsBlock>(s_cnt, nc, at.isum(a), at.head(a), t_now,
                                     [&](int k, unsigned long long v) { at.dsum(a)[k] += stats_value(k, v, sc); });
}

__global__ __launch_bounds__(kStatsBlock) void k_flow_stats(const Clock *clk, int q, FlowStatsArgs a)
{
    flow_stats_body(clk, q, a, StatsOwn{});
}

// batch (sphx_batch_flow_stats_*): member m = blockIdx.y samples its own state (pos / vel at m * Members::part) on its own
// clock into its own block of sums (m * n_bands * n_bins * kStatsFields) and its own head; gridDim.x workgroups per member.
// The sums are exact, so the workgroup count gives the same bits as a context's.
__global__ __launch_bounds__(kStatsBlock) void k_flow_stats_b(Members mb, int q, FlowStatsArgs a)
{
    const int m = (int)blockIdx.y;
    flow_stats_body(mb.clk + m, q, a, StatsMember{mb.part, m});
}

// slab of a ring (sphx_slab_flow_stats_*): the particles this slab owns, of the clk->n it holds, into its own partial sums --
// exact integers, so the ring's sums (the slabs' added up) do not depend on how the channel is cut.  x is in the frame of the
// slab's window: the first slab may hold x < 0 and the last x >= DL, which stats_in_band's fmod brings back into [0, DL).
__global__ __launch_bounds__(kStatsBlock) void k_flow_stats_s(const Clock *clk, int q, FlowStatsArgs a, Grid g, const int *cell)
{
    StatsSlab at;
    at.g = g;
    at.cell = cell;
    flow_stats_body(clk, q, a, at);
}

}  // namespace sphx
