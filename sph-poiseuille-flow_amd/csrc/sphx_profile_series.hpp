// sphx_profile_series.hpp -- the profile series of a resident context (include/sphx.h section 2j) and of every member of a
// batch (section 2k, k_profile_series_b) and of a slab of a ring (section 3a, k_profile_series_s: the particles the slab
// owns): a slot sampler (sphx_slot_sample.hpp) that bins the state the step left into the
// reference's profile bins exactly as the flow statistics do (sphx_flow_stats.hpp) and, where they add the sample to running
// sums, appends it as one record -- {step, t} and n_bands x n_bins x kStatsFields doubles -- to a record buffer in device
// memory.  "Flow statistics that record instead of accumulate": the velocity profile at every sampled step, the one
// diagnostic with a y-profile AND a time axis.
//
// The sample is stats_bin_sample, the flow statistics' own binning loop: stats_bin / stats_in_band / stats_scales, int64
// fixed-point sums in LDS counters per workgroup, one workgroup alone up to kStatsPerThread * kStatsBlock particles, above
// that global int64 sums (isum) and last_out_fenced, a sticky range flag for a |u| above the bound.
//
// The record.  The finishing workgroup -- the only one, or the last one out -- is the only writer of a sample: it reads
// slot = head->n_records (nobody else writes it during the launch, a kernel boundary published it), and when slot < capacity
// it stores EVERY counter of the sample, zeros included, as stats_value(k, v) = ldexp((double)(long long)v, -s) into
// records[slot * block + k] -- the expression flow_stats_body adds to its running sums, so adding the records of a series in
// order, one by one, reproduces the flow statistics' sums to the bit (x + 0.0 == x for every sum the statistics hold).  The
// record buffer is never cleared: a slot is complete because every counter of it is written.  Behind a barrier (every thread of
// the workgroup has read n_records) thread 0 stamps {step, t} and counts the record, or counts a dropped one; either way the
// global int64 sums are back at zero (atomicExch) and the ticket is cleared.
//
// Determinism: integer adds in any order give the same integers, and each counter is converted once by one thread: no
// floating-point atomics, no dependence on particle order, layout, re-binning or workgroup count.  A member of a batch runs
// the same body: bit for bit a standalone context's records.
#pragma once
#include "sphx_flow_stats.hpp"

namespace sphx {

constexpr long long kSeriesMaxTotal = 1ll << 27;  // doubles (1 GiB) of records of all members together

struct ProfileSeriesHead {
    long long n_records, n_dropped;
    int range;   // sticky: some |u| of some sample exceeded the bound of that sample
    int ticket;  // last workgroup out (zero between launches)
};

struct ProfileSeriesArgs {
    FlowStatsArgs bin;        // the sample: pos, vel, isum, the bins, the bands and the gate (dsum, head: unused, nullptr)
    double *times;            // [capacity][2]: step, t (of a batch: member 0's, member m's block behind)
    double *records;          // [capacity][n_bands][n_bins][kStatsFields]
    ProfileSeriesHead *head;  // (of a batch: [M])
    int capacity;
};

// The record of one channel closing the step slot of parity q, on clock clk, shared by the gridDim.x workgroups of a grid row;
// `at` says where the channel's state and int64 sums are (StatsOwn, StatsMember); times / records / h are that channel's own.
template <typename At>
__device__ __forceinline__ void profile_series_body(const Clock *clk, int q, const ProfileSeriesArgs &a, const At &at, double *times,
                                                    double *records, ProfileSeriesHead *h)
{
    const FlowStatsArgs &b = a.bin;
    if (!sample_due(clk, q, b.every, b.t_from)) return;
    const int n = clk->n;
    const double vmax = clk->vmax, t_now = clk->t, step_now = (double)clk->step;
    extern __shared__ unsigned long long s_cnt[];  // [n_bands][n_bins][kStatsFields]
    __shared__ int s_last;
    const int nc = b.n_bands * b.n_bins * kStatsFields;
    const StatsScales sc = stats_bin_sample(b, at, n, vmax, s_cnt, nc, [&] { return &h->range; });
    const bool alone = gridDim.x == 1;  // small channels: one workgroup holds the whole sample -- no global sums, no ticket
    if (!alone) {
        for (int k = threadIdx.x; k < nc; k += kStatsBlock) {
            const unsigned long long v = s_cnt[k];
            if (v) atomicAdd(at.isum(b) + k, v);
        }
        last_out_fenced(&h->ticket, s_last);
        if (!s_last) return;
    }
    // the finishing workgroup: the only writer of this sample
    const long long slot = h->n_records;
    const bool keep = slot < (long long)a.capacity;
    double *rec = records + (size_t)slot * (size_t)nc;  // (not dereferenced unless keep)
    for (int k = threadIdx.x; k < nc; k += kStatsBlock) {
        const unsigned long long v = alone ? s_cnt[k] : atomicExch(at.isum(b) + k, 0ull);
        if (keep) rec[k] = stats_value(k, v, sc);  // every counter, zeros included: the buffer is never cleared
    }
    __syncthreads();  // every thread has read n_records
    if (threadIdx.x != 0) return;
    if (keep) {
        *reinterpret_cast<double2 *>(times + (size_t)slot * 2) = make_double2(step_now, t_now);
        h->n_records = slot + 1;
    } else {
        h->n_dropped += 1;
    }
    if (!alone) __hip_atomic_store(&h->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kStatsBlock) void k_profile_series(const Clock *clk, int q, ProfileSeriesArgs a)
{
    profile_series_body(clk, q, a, StatsOwn{}, a.times, a.records, a.head);
}

// batch (sphx_batch_profile_series_*): member m = blockIdx.y records its own state (pos / vel at m * Members::part) on its own
// clock into its own block of records (m * capacity rows), its own int64 sums (m * n_bands * n_bins * kStatsFields), its own
// head and ticket; gridDim.x workgroups per member.  The sums are exact, so a member's records are bit for bit a standalone
// context's.  A member whose gate is closed returns before it touches its head or its records.
__global__ __launch_bounds__(kStatsBlock) void k_profile_series_b(Members mb, int q, ProfileSeriesArgs a)
{
    const int m = (int)blockIdx.y;
    const size_t nc = (size_t)a.bin.n_bands * (size_t)a.bin.n_bins * kStatsFields;
    profile_series_body(mb.clk + m, q, a, StatsMember{mb.part, m}, a.times + (size_t)m * (size_t)a.capacity * 2,
                        a.records + (size_t)m * (size_t)a.capacity * nc, a.head + m);
}

// slab of a ring (sphx_slab_pseries_*): the particles this slab owns, of the clk->n it holds, into its own records, its own
// int64 sums, head and ticket -- a PARTIAL record: exact integers converted once, so the ring's record (the slabs' added up,
// field by field, count included) does not depend on how the channel is cut; a slab that owns nothing in a band stores that
// band's zeros.  x is in the frame of the slab's window: the first slab may hold x < 0 and the last x >= DL, which
// stats_in_band's fmod brings back into [0, DL).
__global__ __launch_bounds__(kStatsBlock) void k_profile_series_s(const Clock *clk, int q, ProfileSeriesArgs a, Grid g, const int *cell)
{
    StatsSlab at;
    at.g = g;
    at.cell = cell;
    profile_series_body(clk, q, a, at, a.times, a.records, a.head);
}

}  // namespace sphx
